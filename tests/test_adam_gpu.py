"""The second-moment updates on the GPU: x3dstep_adam and the three x3dstep_lamb_* launches against the library's CPU twins
(which tests/test_adam_host.py holds against the numpy restatement, torch.optim.AdamW / Adam and a LAMB in fp64), bit for
bit on w, m, v, the partials, wsumsq, rsumsq, trust and the state words, at every alignment and inside guard bands, with
every tensor at its own scales; subnormal second moments; planted non-finite values; a counter of 0; the per-item and
per-tensor tests; the flagship layout; and both forms captured into a graph."""
import numpy as np
import pytest
import torch

from tests import adam_cases as ac
from tests import group_cases as grc
from tests import guard_cases as gc
from tests import lars_cases as lc
from tests import step_ref
from tests.test_group_gpu import DeviceGroup, _hyper_tensor
from tests.test_guard_gpu import FILL, GUARD, DeviceKeep, _banded, _bits, _dev
from x3dhip import _steplib, stepops

pytestmark = pytest.mark.gpu

N = ac.N
SENTINEL = -3.0


class DeviceAdam(DeviceGroup):
    """DeviceGroup with the second-moment buffer and, for LAMB, the adaptation flags, the workspace and the outputs."""

    def __init__(self, seg_off, dev, hyper=None, adapt=None, R=4, shifts=(0, 0, 0, 0)):
        super().__init__(seg_off, dev, hyper=hyper, R=R, shifts=tuple(shifts[:3]))
        self.shifts4 = tuple(shifts)
        self.vbig, self.v = _banded(self.t.n, shifts[3], dev)
        self.adapt = torch.from_numpy(ac.adapts(self.t.S) if adapt is None else np.asarray(adapt, np.uint8)).to(dev)
        self.lws = torch.zeros(stepops.lamb_workspace_bytes(self.t.nitems), dtype=torch.uint8, device=dev)
        self.wsumsq = torch.full((self.t.S,), SENTINEL, dtype=torch.float64, device=dev)
        self.rsumsq = torch.full((self.t.S,), SENTINEL, dtype=torch.float64, device=dev)
        self.trust = torch.full((self.t.S,), SENTINEL, dtype=torch.float32, device=dev)

    def load(self, w=None, g=None, m=None, v=None):
        super().load(w, g, m)
        if v is not None:
            self.v.copy_(torch.from_numpy(v))

    def _st(self, state):
        return (self.state, self.ring, self.R) if state else (None, None, 0)

    def adam(self, a, count, lr=ac.LR, state=True, tables=None):
        stepops.adam(self.w, self.g, self.m, self.v, self.t if tables is None else tables, self.hyper, *self._st(state), count, lr,
                     a.get("betas", ac.BETAS), a.get("eps", ac.EPS["adam"]), a["wd"], a["gs"], a["decoupled"])

    def lamb(self, a, count, lr=ac.LR, state=True, tables=None, trust_tables=None):
        betas, eps = a.get("betas", ac.BETAS), a.get("eps", ac.EPS["lamb"])
        st, t = self._st(state), self.t if tables is None else tables
        stepops.lamb_moments(self.w, self.g, self.m, self.v, t, self.hyper, *st, count, self.lws, betas, eps, a["wd"], a["gs"])
        stepops.lamb_trust(self.t if trust_tables is None else trust_tables, self.hyper, self.adapt, *st, count, self.lws,
                           self.wsumsq, self.rsumsq, self.trust)
        stepops.lamb_apply(self.w, self.m, self.v, t, self.hyper, self.trust, *st, count, lr, betas, eps, a["wd"])

    def run(self, a, g, count, max_norm=0.0, lr=ac.LR):
        """The twin's run with the count the twin worked out (the device's words are not read here)."""
        self.load(g=g)
        if a["state"]:
            self.measure(max_norm)
        (self.lamb if a["opt"] == "lamb" else self.adam)(a, count, lr, state=a["state"])

    def guards_intact(self):
        lo, hi = GUARD + self.shifts4[3], GUARD + self.shifts4[3] + self.t.n
        return super().guards_intact() and bool((self.vbig[:lo] == FILL).all()) and bool((self.vbig[hi:] == FILL).all())


def _both(d, h, a, g, max_norm=0.0):
    """One case on the twin and on the device, as update a['k']."""
    h.load(g=g)
    if a["state"]:
        h.measure(max_norm)
    count = h.count_for(a)
    (h.lamb if a["opt"] == "lamb" else h.adam)(a, count, state=a["state"])
    d.run(a, g, count, max_norm)


def _same_as_twin(d, h, lamb=True):
    torch.cuda.synchronize()
    for x, y in ((d.w, h.w), (d.m, h.m), (d.v, h.v), (d.g, h.g)):
        assert torch.equal(_bits(x), _bits(y))
    if lamb:
        assert torch.equal(d.lws.cpu(), torch.from_numpy(np.ascontiguousarray(h.lws)))
        assert torch.equal(d.wsumsq.cpu().view(torch.int64), torch.from_numpy(h.wsumsq).view(torch.int64))
        assert torch.equal(d.rsumsq.cpu().view(torch.int64), torch.from_numpy(h.rsumsq).view(torch.int64))
        assert torch.equal(_bits(d.trust), _bits(h.trust))
    assert torch.equal(d.state.cpu(), torch.from_numpy(h.state))
    assert torch.equal(d.ring.cpu(), torch.from_numpy(np.ascontiguousarray(h.ring)))
    assert d.guards_intact()


def _tables_with(t, dev, items=None, seg_item=None):
    """Another StepTables over the same buffers with one device table replaced (the per-item and per-tensor tests)."""
    other = stepops.StepTables(t.seg_off, dev)
    if items is not None:
        other.d_items = torch.from_numpy(items.view(np.uint8).copy()).to(dev)
    if seg_item is not None:
        other.d_seg_item = torch.from_numpy(seg_item.copy()).to(dev)
    return other


def _start(off, dev, shifts, seed, hyper=None, adapt=None, R=4):
    d = DeviceAdam(off, dev, hyper=hyper, adapt=adapt, R=R, shifts=shifts)
    h = ac.HostAdam(off, hyper=hyper, adapt=adapt, R=R, shifts=shifts)
    n = h.t.n
    w0, m0, v0 = gc.normals(n, seed), gc.normals(n, seed + 1, 0.1), ac.second_moments(n, seed + 2)
    for x in (d, h):
        x.load(w0, None, m0, v0)
    return d, h, (w0, m0, v0)


@pytest.mark.parametrize("shifts", ac.SHIFTS, ids=ac.shift_id)
def test_the_kernels_equal_the_twins_over_the_grid(shifts):
    dev = _dev()
    off = gc.synthetic()
    d, _, (w0, m0, v0) = _start(off, dev, shifts, 6)
    state0 = torch.from_numpy(stepops.new_state()).to(dev)
    for i, a in enumerate(ac.GRID):
        g, max_norm = ac.gradient_for(a, N, 5 + i % 3)
        h = ac.HostAdam(off, shifts=shifts)
        d.state.copy_(state0)
        d.ring.zero_()
        for x in (d, h):
            x.load(w0, g, m0, v0)
        if a["opt"] == "adam":                           # the LAMB outputs of the case before are not this case's
            for x in (d, h):
                x.lws[:] = 0
                x.wsumsq[:] = SENTINEL
                x.rsumsq[:] = SENTINEL
                x.trust[:] = SENTINEL
        _both(d, h, a, g, max_norm)
        _same_as_twin(d, h)
        assert not torch.equal(_bits(d.w), _bits(w0)) and not torch.equal(_bits(d.v), _bits(v0)), ac.case_id(a)


EDGE_CASES = [dict(opt="adam", decoupled=1, gs=0.5, wd=0.01, state=True, clipped=False, k=3),
              dict(opt="adam", decoupled=0, gs=1.0, wd=0.01, state=False, clipped=False, k=1),
              dict(opt="lamb", decoupled=1, gs=0.5, wd=0.01, state=True, clipped=False, k=2)]


def test_the_kernels_on_every_edge_length():
    dev = _dev()
    for n in step_ref.EDGE_LENGTHS:
        off = step_ref.seg_off_of([n, 5, n])
        g = gc.normals(2 * n + 5, 25)
        for shifts in ((n % 4,) * 4, (2, 0, 1, 3)):
            for a in EDGE_CASES:
                d, h, _ = _start(off, dev, shifts, 26, hyper=grc.scales(3))
                _both(d, h, a, g, 0.5)
                _same_as_twin(d, h, lamb=a["opt"] == "lamb")


@pytest.mark.parametrize("shifts", ac.SHIFTS, ids=ac.shift_id)
def test_the_kernels_on_tensors_around_a_group_an_item_and_many_items(shifts):
    dev = _dev()
    off = lc.lengths_seg_off()
    g = gc.normals(int(off[-1]), 45)
    for a in EDGE_CASES:
        d, h, (w0, _, _) = _start(off, dev, shifts, 46)
        _both(d, h, a, g)
        _same_as_twin(d, h, lamb=a["opt"] == "lamb")
    # wsumsq is what x3dstep_measure records on w (the last case is LAMB's)
    ref = DeviceGroup(off, dev)
    ref.load(g=w0)
    ref.measure()
    torch.cuda.synchronize()
    rec = stepops.parse_record(ref.ring.cpu().numpy()[:ref.t.record_bytes], ref.t.S)
    assert d.wsumsq.cpu().numpy().tobytes() == np.ascontiguousarray(rec[1]).tobytes()


def test_subnormal_second_moments_and_a_denominator_of_eps():
    dev = _dev()
    off = gc.synthetic()
    w0 = gc.normals(N, 330)
    g = (gc.normals(N, 331) * np.float32(1e-19)).astype(np.float32)
    zeros = np.zeros(N, np.float32)
    for opt in ("adam", "lamb"):
        a = dict(opt=opt, decoupled=1, gs=1.0, wd=0.0, state=False, clipped=False, k=1, eps=1e-3)
        for shifts in ((0, 0, 0, 0), (0, 1, 2, 3)):
            d, h = DeviceAdam(off, dev, shifts=shifts), ac.HostAdam(off, shifts=shifts)
            for x in (d, h):
                x.load(w0, None, zeros, zeros)
            _both(d, h, a, g)
            _same_as_twin(d, h, lamb=opt == "lamb")
            v = d.v.cpu().numpy()
            assert np.count_nonzero((v > 0) & (v < float(np.finfo(np.float32).tiny))) > N // 2


@pytest.mark.parametrize("opt", ["adam", "lamb"])
@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf], ids=["nan", "+inf", "-inf"])
def test_a_planted_nonfinite_leaves_w_m_and_v_bitwise_as_before(opt, value):
    dev = _dev()
    off = gc.synthetic()
    a = dict(opt=opt, decoupled=1, gs=1.0, wd=0.01, state=True, clipped=False)
    good = gc.normals(N, 35)
    s = 9
    for shifts, at in (((0, 0, 0, 0), int(off[s])), ((1, 1, 1, 1), int(off[s + 1]) - 1), ((0, 1, 2, 3), int(off[s]) + 7)):
        bad = good.copy()
        bad[at] = value
        d, h, _ = _start(off, dev, shifts, 36, R=2)
        _both(d, h, dict(a, k=1), good, 1.0)
        torch.cuda.synchronize()
        before = (d.w.clone(), d.m.clone(), d.v.clone(), d.trust.clone())
        _both(d, h, dict(a, k=2), bad, 1.0)
        _same_as_twin(d, h, lamb=opt == "lamb")
        assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip((d.w, d.m, d.v, d.trust), before))
        assert d.state.cpu()[5:].tolist() == [1, 1, 1] == list(h.words())
        _both(d, h, dict(a, k=2), good, 1.0)             # the skipped update did not advance the count
        assert h.count_for(dict(a, k=2)) == 0
        _same_as_twin(d, h, lamb=opt == "lamb")
        assert d.state.cpu()[5:].tolist() == [0, 1, 0] and not torch.equal(d.w, before[0])


def test_a_counter_of_zero_or_a_count_below_one_stores_nothing_and_the_wrappers_check():
    dev = _dev()
    d, _, (w0, m0, v0) = _start(gc.synthetic(), dev, (0, 0, 0, 0), 41)
    d.load(g=gc.normals(N, 43))
    d.lws.fill_(0x5a)
    a = dict(opt="lamb", decoupled=1, gs=1.0, wd=0.0)
    d.trust.fill_(0.5)
    d.adam(a, 1)
    d.lamb(a, 1)
    torch.cuda.synchronize()

    def nothing_stored(state):
        torch.cuda.synchronize()
        assert bool((d.lws == 0x5a).all()) and bool((d.wsumsq == SENTINEL).all()) and bool((d.rsumsq == SENTINEL).all())
        assert bool((d.trust == 0.5).all())
        assert all(torch.equal(_bits(x), _bits(y)) for x, y in ((d.w, w0), (d.m, m0), (d.v, v0)))
        assert torch.equal(d.state.cpu(), state) and d.guards_intact()

    nothing_stored(torch.from_numpy(stepops.new_state()))
    # something measured, but the count makes this update number 0 and -2: nothing either, the skip words included
    d.measure()
    torch.cuda.synchronize()
    measured = d.state.cpu().clone()
    for count in (-1, -3):
        d.adam(a, count)
        d.lamb(a, count)
        nothing_stored(measured)
    with pytest.raises(ValueError):
        stepops.adam(d.w.cpu(), d.g, d.m, d.v, d.t, d.hyper, None, None, 0, 1, 0.1)
    with pytest.raises(ValueError):
        stepops.adam(d.w, d.g, d.m, d.v[:-1], d.t, d.hyper, None, None, 0, 1, 0.1)
    with pytest.raises(ValueError):
        stepops.adam(d.w, d.g, d.m, d.v, d.t, d.hyper, None, None, 0, 1, 0.1, betas=(0.9, 1.0))
    with pytest.raises(ValueError):
        stepops.adam(d.w, d.g, d.m, d.v, d.t, d.hyper, None, None, 0, 1, 0.1, eps=-1.0)
    with pytest.raises(ValueError):
        stepops.lamb_moments(d.w, d.g, d.m, d.v, d.t, d.hyper, None, None, 0, 1, d.lws[:-8])
    with pytest.raises(ValueError):
        stepops.lamb_trust(d.t, d.hyper, d.adapt.float(), None, None, 0, 1, d.lws, d.wsumsq, d.rsumsq, d.trust)
    with pytest.raises(ValueError):
        stepops.lamb_apply(d.w, d.m, d.v, d.t, d.hyper, d.trust.double(), None, None, 0, 1, 0.1)
    with pytest.raises(Exception):
        stepops.adam(d.w, d.g, d.m, d.m, d.t, d.hyper, None, None, 0, 1, 0.1)                # m and v the same buffer
    with pytest.raises(Exception):
        stepops.adam(d.w, d.g, d.m, d.v, d.t, d.hyper, None, None, 0, 0, 0.1)                # no state and no count
    nothing_stored(measured)


def test_an_item_that_fails_its_tests_is_exactly_what_is_left_untouched():
    """The tables are device memory nobody checked: one bad item of each kind (tests/group_cases.py) and, for launch 3 of
    LAMB, one bad trust of each kind -- every element of that item keeps its bytes and every other element is the twin's
    on the good table; in launch 1 of LAMB a bad item also gives NaN partials, so that its tensor has NaN sums and a trust
    of exactly 1, and every other tensor is the twin's."""
    dev = _dev()
    off = gc.synthetic()
    g = gc.normals(N, 61)
    shifts = (1, 1, 1, 1)
    d, h, (w0, m0, v0) = _start(off, dev, shifts, 62)
    frozen_of = lambda bad: np.isin(np.repeat(np.arange(h.t.nitems), h.t.items["len"]), bad)          # noqa: E731
    for opt in ("adam", "lamb"):
        a = dict(opt=opt, decoupled=1, gs=0.5, wd=0.01, state=False, clipped=False, k=3)
        h.load(w0, g, m0, v0)
        (h.lamb if opt == "lamb" else h.adam)(a, 3, state=False)
        trust0 = np.linspace(0.25, 2.0, h.t.S).astype(np.float32)
        cases = [(name, items, hy, None, bad) for name, items, hy, bad in grc.bad_item_tables(h.t)]
        assert len(cases) == 10
        for name, items, hy, _, bad in cases:
            d.load(w0, g, m0, v0)
            d.hyper = _hyper_tensor(hy, dev)
            tables = _tables_with(d.t, dev, items=items)
            if opt == "adam":
                d.adam(a, 3, state=False, tables=tables)
            else:
                d.lamb(a, 3, state=False, tables=tables)
            torch.cuda.synchronize()
            frozen = frozen_of(bad)
            assert 0 < frozen.sum() <= 2 * _steplib.ITEM + 1
            if opt == "lamb" and name.endswith(("scale-negative", "scale-nan", "scale-inf")):
                continue                                 # the tensor fails launch 2's tests as well: see the per-tensor test
            for dv, before, after in ((d.m, m0, h.m), (d.v, v0, h.v)):
                assert torch.equal(_bits(dv), _bits(np.where(frozen, before, np.asarray(after)))), (opt, name)
            if opt == "adam":
                assert torch.equal(_bits(d.w), _bits(np.where(frozen, w0, np.asarray(h.w)))), name
            else:
                s = int(h.t.items["seg"][bad[0]])
                rs, wsq, tr = d.rsumsq.cpu().numpy(), d.wsumsq.cpu().numpy(), d.trust.cpu().numpy()
                assert np.isnan(rs[s]) and np.isnan(wsq[s]) and tr[s] == 1.0, name
                assert np.delete(rs, s).tobytes() == np.delete(h.rsumsq, s).tobytes(), name
                assert np.delete(tr, s).tobytes() == np.delete(h.trust, s).tobytes(), name
                inside = np.repeat(np.arange(h.t.S), np.diff(off)) == s      # the rest of the tensor moved at a trust of 1
                dw = d.w.cpu().numpy()
                assert dw[~inside].tobytes() == h.w[~inside].tobytes() and dw[frozen].tobytes() == w0[frozen].tobytes(), name
            assert d.guards_intact(), name
        if opt == "lamb":                                # launch 3 alone, with one bad trust of each kind
            d.hyper = _hyper_tensor(grc.scales(h.t.S), dev)
            h.load(w0, g, m0, v0)
            stepops.lamb_apply_host(h.w, h.m, h.v, h.t, h.hyper, trust0, None, None, 0, 3, ac.LR, ac.BETAS, ac.EPS["lamb"], a["wd"])
            for value in (-0.5, np.nan, np.inf):
                t = trust0.copy()
                t[9] = value
                d.load(w0, g, m0, v0)
                stepops.lamb_apply(d.w, d.m, d.v, d.t, d.hyper, torch.from_numpy(t).to(dev), None, None, 0, 3, ac.LR, ac.BETAS,
                                   ac.EPS["lamb"], a["wd"])
                frozen = frozen_of(list(range(int(h.t.seg_item[9]), int(h.t.seg_item[10]))))
                assert torch.equal(_bits(d.w), _bits(np.where(frozen, w0, np.asarray(h.w)))), value
                assert torch.equal(_bits(d.m), _bits(m0)) and torch.equal(_bits(d.v), _bits(v0)) and d.guards_intact()


def test_a_tensor_that_fails_its_tests_is_exactly_what_gets_no_store():
    dev = _dev()
    off = gc.synthetic()
    a = dict(opt="lamb", decoupled=1, gs=0.5, wd=0.01, state=False, clipped=False, k=2)
    d, h, _ = _start(off, dev, (2, 2, 2, 2), 64)
    g = gc.normals(N, 65)
    _both(d, h, a, g)
    _same_as_twin(d, h)
    cases = [c for c in lc.bad_tensor_tables(h.t) if not c[0].startswith("eta")]
    assert len(cases) == 4
    for name, hy, _, si, bad in cases:
        for x in (d.wsumsq, d.rsumsq, d.trust):
            x.fill_(SENTINEL)
        stepops.lamb_trust(_tables_with(d.t, dev, seg_item=si), _hyper_tensor(hy, dev), d.adapt, None, None, 0, 2, d.lws,
                           d.wsumsq, d.rsumsq, d.trust)
        torch.cuda.synchronize()
        ws, rs, tr = d.wsumsq.cpu().numpy(), d.rsumsq.cpu().numpy(), d.trust.cpu().numpy()
        skip = set(bad) | ({bad[0] + 1} if name == "items-empty" else set())        # the neighbour took the items over
        for s in range(h.t.S):
            if s in bad:
                assert ws[s] == SENTINEL and rs[s] == SENTINEL and tr[s] == SENTINEL, name
            elif s not in skip:
                assert ws[s].tobytes() == h.wsumsq[s].tobytes() and rs[s].tobytes() == h.rsumsq[s].tobytes(), (name, s)
                assert tr[s].tobytes() == h.trust[s].tobytes(), (name, s)
    assert d.guards_intact()


def test_the_flagship_layout_once():
    dev = _dev()
    off, names = step_ref.model_seg_off("M")
    n, S = int(off[-1]), len(names)
    assert S == 316 and 3.7e6 < n < 3.9e6
    hy = grc.ones(S)
    one_d = [i for i, k in enumerate(names) if off[i + 1] - off[i] <= 2048 and ("bn" in k or k.endswith("bias"))]
    hy["wd_scale"][one_d] = 0.0
    adapt = np.ones(S, np.uint8)
    adapt[one_d] = 0
    assert len(one_d) > 100
    g, w0 = gc.normals(n, 51, 0.02), gc.normals(n, 52, 0.05)
    m0, v0 = gc.normals(n, 53, 0.01), ac.second_moments(n, 54, 0.02)
    for opt in ("adam", "lamb"):
        a = dict(opt=opt, decoupled=1, gs=0.125, wd=0.01, state=True, clipped=False, k=5)
        d, h = DeviceAdam(off, dev, hyper=hy, adapt=adapt), ac.HostAdam(off, hyper=hy, adapt=adapt)
        for x in (d, h):
            x.load(w0, None, m0, v0)
        _both(d, h, a, g, 2.0)
        _same_as_twin(d, h, lamb=opt == "lamb")
        assert float(h.coef()) < 1.0
        if opt == "lamb":
            tr = d.trust.cpu().numpy()
            assert np.all(tr[one_d] == 1.0) and np.all(np.delete(tr, one_d) != 1.0)
        bad = g.copy()
        bad[n // 2] = np.nan
        _both(d, h, dict(a, k=6), bad, 2.0)
        _same_as_twin(d, h, lamb=opt == "lamb")
        assert d.state.cpu()[5:].tolist() == [1, 1, 1]


@pytest.mark.parametrize("opt", ["adam", "lamb"])
def test_the_guarded_sequence_captured_into_one_graph(opt):
    """What a guarded step enqueues after the backward pass -- measure, the update, restore -- captured once and replayed on
    new contents: good, bad, good.  The count is part of the captured launches; k comes from the state words."""
    dev = _dev()
    off = gc.synthetic()
    a = dict(opt=opt, decoupled=1, gs=1.0, wd=0.01, state=True, clipped=False)
    max_norm = 10.0
    d, h, _ = _start(off, dev, (0, 0, 0, 0), 81, R=8)
    hk = gc.HostKeep(seed=80)
    hk.state = h.state
    dk = DeviceKeep(dev)
    dk.state = d.state
    for b, v in zip(dk.live, hk.live):
        b.copy_(torch.from_numpy(v))
    good1, bad, good2 = gc.normals(N, 83), gc.normals(N, 84), gc.normals(N, 85)
    bad[int(off[5])] = np.inf
    d.load(g=good1)
    host_update = h.lamb if opt == "lamb" else h.adam

    def device_tail():
        d.measure(max_norm)
        (d.lamb if opt == "lamb" else d.adam)(a, 0)
        stepops.keep(dk.kt, d.state, _steplib.KEEP_RESTORE)

    def host_tail(g):
        h.load(g=g)
        h.measure(max_norm)
        host_update(a, 0)
        hk.keep(_steplib.KEEP_RESTORE)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                           # one eager step first, as a capture's warm-up does
        stepops.keep(dk.kt, d.state, _steplib.KEEP_SAVE)
        device_tail()
    torch.cuda.current_stream().wait_stream(s)
    hk.keep(_steplib.KEEP_SAVE)
    host_tail(good1)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        device_tail()
    words = []
    for i, g in enumerate((good1, bad, good2)):
        stepops.keep(dk.kt, d.state, _steplib.KEEP_SAVE)
        hk.keep(_steplib.KEEP_SAVE)
        d.load(g=g)
        fresh = [gc.normals(b.size, 90 + 10 * i + j) for j, b in enumerate(hk.live)]
        for b, hb, v in zip(dk.live, hk.live, fresh):
            b.copy_(torch.from_numpy(v))
            hb[:] = v
        graph.replay()
        host_tail(g)
        torch.cuda.synchronize()
        for b, hb in zip(dk.live, hk.live):
            assert torch.equal(_bits(b), _bits(hb))
        words.append(d.state.cpu()[5:].tolist())
        _same_as_twin(d, h, lamb=opt == "lamb")
    assert words == [[0, 0, 0], [1, 1, 1], [0, 1, 0]] and dk.guards_intact() and h.applied() == 3


@pytest.mark.parametrize("opt", ["adam", "lamb"])
def test_the_unguarded_form_captured_and_replayed_on_new_contents(opt):
    """observe and the update with state = NULL captured: the launches read the scales (and LAMB its flags) from device
    memory, so a table changed between replays (outside the graph) is what the next replay applies.  Without a state the
    count is k itself and part of the captured launch: every replay is update 4."""
    dev = _dev()
    off = gc.synthetic()
    a = dict(opt=opt, decoupled=0 if opt == "adam" else 1, gs=0.5, wd=0.01, state=False, clipped=False, k=4)
    d, h, _ = _start(off, dev, (0, 0, 0, 0), 71)
    grads = [gc.normals(N, 73 + i) for i in range(3)]
    d.load(g=grads[0])
    host_update = h.lamb if opt == "lamb" else h.adam

    def device_tail():
        d.measure()
        (d.lamb if opt == "lamb" else d.adam)(a, 4, state=False)

    def host_tail(g):
        h.load(g=g)
        h.measure()
        host_update(a, 4, state=False)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        device_tail()
    torch.cuda.current_stream().wait_stream(s)
    host_tail(grads[0])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        device_tail()
    for i, g in enumerate(grads):
        if i == 2:                                       # new scales and flags, copied outside the graph into the same tensors
            h.hyper = grc.scales(h.t.S)[::-1].copy()
            d.hyper.copy_(_hyper_tensor(h.hyper, dev))
            h.adapt = ac.adapts(h.t.S)[::-1].copy()
            d.adapt.copy_(torch.from_numpy(h.adapt))
        d.load(g=g)
        graph.replay()
        host_tail(g)
        _same_as_twin(d, h, lamb=opt == "lamb")
    assert d.state.cpu()[5:].tolist() == [0, 0, 0] and int(d.state[0]) == 4
