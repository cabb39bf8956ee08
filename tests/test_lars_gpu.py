"""The trust ratios on the GPU: x3dstep_trust and x3dstep_apply_lars against the library's CPU twins (which
tests/test_lars_host.py holds against the numpy restatement and a LARS in plain torch), bit for bit, at every alignment and
inside guard bands, with every tensor at its own rate of trust and scales; the identity with x3dstep_apply_groups; planted
non-finite values; a counter of 0; the per-item and per-tensor tests; the flagship layout; and both forms captured into a
graph."""
import numpy as np
import pytest
import torch

from tests import group_cases as grc
from tests import guard_cases as gc
from tests import lars_cases as lc
from tests import step_ref
from tests.test_group_gpu import DeviceGroup, _hyper_tensor
from tests.test_guard_gpu import DeviceKeep, _bits, _dev
from x3dhip import _steplib, stepops

pytestmark = pytest.mark.gpu

N = lc.N
SENTINEL = -3.0


class DeviceLars(DeviceGroup):
    """DeviceGroup with the rates of trust, the outputs wsumsq and trust and the workspace of the partials on the device."""

    def __init__(self, seg_off, dev, hyper=None, eta=None, R=4, shifts=(0, 0, 0)):
        super().__init__(seg_off, dev, hyper=hyper, R=R, shifts=shifts)
        self.eta = torch.from_numpy(lc.etas(self.t.S) if eta is None else np.asarray(eta, np.float32)).to(dev)
        self.tws = torch.zeros(stepops.trust_workspace_bytes(self.t.nitems), dtype=torch.uint8, device=dev)
        self.wsumsq = torch.full((self.t.S,), SENTINEL, dtype=torch.float64, device=dev)
        self.trust = torch.full((self.t.S,), SENTINEL, dtype=torch.float32, device=dev)

    def trust_dev(self, a, lr=gc.LR, tables=None):
        stepops.trust(self.w, self.t if tables is None else tables, self.hyper, self.eta, self.state, self.ring, self.R,
                      self.tws, self.wsumsq, self.trust, lr, a["wd"], a["gs"], a.get("eps", lc.EPS), a.get("clip", 0))

    def apply_lars(self, a, lr=gc.LR, state=True, trust=None, tables=None):
        stepops.apply_lars(self.w, self.g, self.m, self.t if tables is None else tables, self.hyper,
                           self.trust if trust is None else trust, self.state if state else None,
                           self.ring if state else None, self.R, lr, a["mu"], a["wd"], a["gs"], a["first"],
                           a.get("nesterov", 0))

    def run(self, a, g, max_norm=0.0, lr=gc.LR):
        self.load(g=g)
        self.measure(max_norm)
        self.trust_dev(a, lr)
        self.apply_lars(a, lr, state=a["state"])


def _same_as_twin(d, h):
    torch.cuda.synchronize()
    assert torch.equal(d.wsumsq.cpu().view(torch.int64), torch.from_numpy(h.wsumsq).view(torch.int64))
    assert torch.equal(_bits(d.trust), _bits(h.trust))
    assert torch.equal(_bits(d.w), _bits(h.w)) and torch.equal(_bits(d.m), _bits(h.m)) and torch.equal(_bits(d.g), _bits(h.g))
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


@pytest.mark.parametrize("shifts", grc.SHIFTS, ids=lambda s: "shift%d%d%d" % s)
def test_the_kernels_equal_the_twins_over_the_grid(shifts):
    dev = _dev()
    off = gc.synthetic()
    w0, m0 = gc.normals(N, 6), gc.normals(N, 7, 0.1)
    d = DeviceLars(off, dev, shifts=shifts)
    state0 = torch.from_numpy(stepops.new_state()).to(dev)
    for a in lc.GRID:
        g, max_norm = grc.gradient_for(a, N, 5)
        h = lc.HostLars(off, shifts=shifts)
        d.state.copy_(state0)
        d.ring.zero_()
        for x in (d, h):
            x.load(w0, g, m0)
            x.run(a, g, max_norm)
        _same_as_twin(d, h)
        assert not torch.equal(_bits(d.w), _bits(w0)), lc.case_id(a)


def test_the_kernels_on_every_edge_length():
    dev = _dev()
    a = dict(first=0, gs=1.0, wd=5e-5, mu=0.9, nesterov=1, clip=0, state=True)
    for n in step_ref.EDGE_LENGTHS:
        off = step_ref.seg_off_of([n, 5, n])
        k = 2 * n + 5
        g, w0, m0 = gc.normals(k, 25), gc.normals(k, 26), gc.normals(k, 27, 0.1)
        for shifts in ((n % 4,) * 3, (2, 0, 1)):
            d, h = DeviceLars(off, dev, shifts=shifts), lc.HostLars(off, shifts=shifts)
            for x in (d, h):
                x.load(w0, g, m0)
                x.run(a, g, 0.5)
            _same_as_twin(d, h)


@pytest.mark.parametrize("shifts", grc.SHIFTS, ids=lambda s: "shift%d%d%d" % s)
def test_the_kernels_on_tensors_around_a_group_an_item_and_many_items(shifts):
    dev = _dev()
    off = lc.lengths_seg_off()
    k = int(off[-1])
    a = dict(first=0, gs=0.5, wd=5e-5, mu=0.9, nesterov=0, clip=1, state=True)
    g, w0, m0 = gc.normals(k, 45), gc.normals(k, 46), gc.normals(k, 47, 0.1)
    d, h = DeviceLars(off, dev, shifts=shifts), lc.HostLars(off, shifts=shifts)
    for x in (d, h):
        x.load(w0, g, m0)
        x.run(a, g)
    _same_as_twin(d, h)
    # wsumsq is what x3dstep_measure records on w at the same alignment
    ref = DeviceLars(off, dev, shifts=(0, shifts[0], 0))
    ref.load(g=w0)
    ref.measure()
    torch.cuda.synchronize()
    rec = stepops.parse_record(ref.ring.cpu().numpy()[:ref.t.record_bytes], ref.t.S)
    assert d.wsumsq.cpu().numpy().tobytes() == np.ascontiguousarray(rec[1]).tobytes()


def test_all_trust_one_gives_the_bits_of_apply_groups():
    dev = _dev()
    off = gc.synthetic()
    w0, m0 = gc.normals(N, 6), gc.normals(N, 7, 0.1)
    for a in grc.GRID[::3]:
        g, max_norm = grc.gradient_for(a, N, 5)
        old, new = DeviceGroup(off, dev), DeviceLars(off, dev)
        for x in (old, new):
            x.load(w0, g, m0)
            if a["state"]:
                x.measure(max_norm)
        old.apply_groups(a, state=a["state"])
        new.apply_lars(a, state=a["state"], trust=torch.ones(new.t.S, dtype=torch.float32, device=dev))
        torch.cuda.synchronize()
        assert torch.equal(_bits(new.w), _bits(old.w)) and torch.equal(_bits(new.m), _bits(old.m)), grc.case_id(a)
        assert torch.equal(new.state, old.state) and new.guards_intact()
        assert not torch.equal(_bits(new.w), _bits(w0))


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf], ids=["nan", "+inf", "-inf"])
def test_a_planted_nonfinite_leaves_w_and_m_bitwise_as_before(value):
    dev = _dev()
    off = gc.synthetic()
    a = dict(first=0, gs=1.0, wd=5e-5, mu=0.9, nesterov=1, clip=0, state=True)
    good, w0, m0 = gc.normals(N, 35), gc.normals(N, 36), gc.normals(N, 37, 0.1)
    s = 9
    for shifts, at in (((0, 0, 0), int(off[s])), ((1, 1, 1), int(off[s + 1]) - 1), ((0, 1, 2), int(off[s]) + 7)):
        bad = good.copy()
        bad[at] = value
        d, h = DeviceLars(off, dev, R=2, shifts=shifts), lc.HostLars(off, R=2, shifts=shifts)
        for x in (d, h):
            x.load(w0, None, m0)
            x.run(a, good, 1.0)
        torch.cuda.synchronize()
        before = (d.w.clone(), d.m.clone())
        for x in (d, h):
            x.run(a, bad, 1.0)
        _same_as_twin(d, h)
        assert torch.equal(_bits(d.w), _bits(before[0])) and torch.equal(_bits(d.m), _bits(before[1]))
        assert float(d.trust[s]) == 1.0 and d.state.cpu()[5:].tolist() == [1, 1, 1] == list(h.words())
        for x in (d, h):
            x.run(a, good, 1.0)
        _same_as_twin(d, h)
        assert d.state.cpu()[5:].tolist() == [0, 1, 0] and not torch.equal(d.w, before[0])
    # a NaN and an Inf among the weights: a trust of exactly 1 for those tensors, as the twin says
    w1 = w0.copy()
    w1[int(off[10]) + 3] = np.nan
    w1[int(off[11]) + 5] = np.inf
    d, h = DeviceLars(off, dev), lc.HostLars(off)
    for x in (d, h):
        x.load(w1, good, m0)
        x.measure()
        x.trust_dev(a) if x is d else x.trust_host(a)
    torch.cuda.synchronize()
    dn, hn = d.wsumsq.cpu().numpy(), h.wsumsq
    assert np.isnan(dn[10]) and np.isnan(hn[10]) and np.isinf(dn[11])
    assert np.delete(dn, 10).tobytes() == np.delete(hn, 10).tobytes() and torch.equal(_bits(d.trust), _bits(h.trust))
    assert float(d.trust[10]) == 1.0 and float(d.trust[11]) == 1.0


def test_a_counter_of_zero_stores_nothing_and_the_wrappers_check():
    dev = _dev()
    d = DeviceLars(gc.synthetic(), dev)
    w0, m0 = gc.normals(N, 41), gc.normals(N, 42)
    d.load(w0, gc.normals(N, 43), m0)
    d.tws.fill_(0x5a)
    a = dict(first=0, gs=1.0, wd=0.0, mu=0.9, nesterov=0)
    d.trust_dev(a)
    d.trust.fill_(0.5)
    d.apply_lars(a)
    torch.cuda.synchronize()
    assert bool((d.tws == 0x5a).all()) and bool((d.wsumsq == SENTINEL).all()) and bool((d.trust == 0.5).all())
    assert torch.equal(_bits(d.w), _bits(w0)) and torch.equal(_bits(d.m), _bits(m0))
    assert torch.equal(d.state.cpu(), torch.from_numpy(stepops.new_state())) and d.guards_intact()
    with pytest.raises(ValueError):
        stepops.trust(d.w.cpu(), d.t, d.hyper, d.eta, d.state, d.ring, d.R, d.tws, d.wsumsq, d.trust, 0.1)
    with pytest.raises(ValueError):
        stepops.trust(d.w, d.t, d.hyper, d.eta[:-1], d.state, d.ring, d.R, d.tws, d.wsumsq, d.trust, 0.1)
    with pytest.raises(ValueError):
        stepops.trust(d.w, d.t, d.hyper, d.eta, d.state, d.ring, d.R, d.tws[:-8], d.wsumsq, d.trust, 0.1)
    with pytest.raises(ValueError):
        stepops.trust(d.w, d.t, d.hyper, d.eta, d.state, d.ring, d.R, d.tws, d.wsumsq, d.trust, 0.1, eps=-1.0)
    with pytest.raises(ValueError):
        stepops.trust(d.w, d.t, d.hyper, d.eta, d.state, d.ring, d.R, d.tws, d.wsumsq, d.trust, 0.1, clip=2)
    with pytest.raises(ValueError):
        stepops.apply_lars(d.w, d.g, d.m, d.t, d.hyper, d.trust.cpu(), None, None, 0, 0.1)
    with pytest.raises(ValueError):
        stepops.apply_lars(d.w, d.g, d.m, d.t, d.hyper, d.trust.double(), None, None, 0, 0.1)
    with pytest.raises(Exception):
        stepops.apply_lars(d.g, d.g, d.m, d.t, d.hyper, d.trust, None, None, 0, 0.1)         # w and g the same buffer
    torch.cuda.synchronize()
    assert torch.equal(_bits(d.w), _bits(w0)) and d.guards_intact()


def test_an_item_that_fails_its_tests_is_exactly_what_is_left_untouched():
    """The tables are device memory nobody checked: one bad item of each kind (tests/group_cases.py) and one bad trust of
    each kind -- every element of that item keeps its bytes and every other element is the twin's on the good table; in
    x3dstep_trust a bad item gives its tensor a NaN sum and a trust of 1, and every other tensor is the twin's."""
    dev = _dev()
    off = gc.synthetic()
    a = dict(first=0, gs=0.5, wd=5e-5, mu=0.9, nesterov=1, clip=0)
    g, w0, m0 = gc.normals(N, 61), gc.normals(N, 62), gc.normals(N, 63, 0.1)
    h = lc.HostLars(off)
    h.load(w0, g, m0)
    h.measure()
    h.trust_host(a)
    clean = (h.wsumsq.copy(), h.trust.copy())
    trust0 = np.linspace(0.25, 2.0, h.t.S).astype(np.float32)
    h.apply_lars(a, state=False, trust=trust0)
    d = DeviceLars(off, dev, shifts=(1, 1, 1))
    cases = [(name, items, hy, trust0, bad) for name, items, hy, bad in grc.bad_item_tables(h.t)]
    for name, value in (("trust-negative", -0.5), ("trust-nan", np.nan), ("trust-inf", np.inf)):
        t = trust0.copy()
        t[9] = value
        cases.append((name, h.t.items.copy(), grc.scales(h.t.S), t, list(range(int(h.t.seg_item[9]), int(h.t.seg_item[10])))))
    assert len(cases) == 13
    for name, items, hy, trust, bad in cases:
        d.load(w0, g, m0)
        d.hyper = _hyper_tensor(hy, dev)
        tables = _tables_with(d.t, dev, items=items)
        d.apply_lars(a, state=False, trust=torch.from_numpy(trust).to(dev), tables=tables)
        torch.cuda.synchronize()
        frozen = np.zeros(N, bool)
        for i in bad:
            s, k = int(h.t.items["start"][i]), int(h.t.items["len"][i])
            frozen[s:s + k] = True
        assert 0 < frozen.sum() <= 2 * _steplib.ITEM + 1
        for dv, before, after in ((d.w, w0, h.w), (d.m, m0, h.m)):
            want = np.where(frozen, before, np.asarray(after))
            assert torch.equal(_bits(dv), _bits(want)), name
        assert d.guards_intact(), name
    # the partials launch: the tensor of a bad item has a NaN sum and a trust of exactly 1
    d.hyper = _hyper_tensor(grc.scales(h.t.S), dev)
    for name, items, hy, bad in grc.bad_item_tables(h.t)[:6]:
        d.load(w0, g, m0)
        d.state.copy_(torch.from_numpy(stepops.new_state()))
        d.measure()
        d.trust_dev(a, tables=_tables_with(d.t, dev, items=items))
        torch.cuda.synchronize()
        s = int(h.t.items["seg"][bad[0]])
        ss, tr = d.wsumsq.cpu().numpy(), d.trust.cpu().numpy()
        assert np.isnan(ss[s]) and tr[s] == 1.0, name
        assert np.delete(ss, s).tobytes() == np.delete(clean[0], s).tobytes(), name
        assert np.delete(tr, s).tobytes() == np.delete(clean[1], s).tobytes(), name


def test_a_tensor_that_fails_its_tests_is_exactly_what_gets_no_store():
    dev = _dev()
    off = gc.synthetic()
    a = dict(gs=0.5, wd=5e-5, clip=0)
    g, w0 = gc.normals(N, 61), gc.normals(N, 62)
    h = lc.HostLars(off)
    h.load(w0, g, None)
    h.measure()
    h.trust_host(a)
    d = DeviceLars(off, dev, shifts=(2, 2, 2))
    d.load(w0, g, None)
    d.measure()
    cases = lc.bad_tensor_tables(h.t)
    assert len(cases) == 7
    for name, hy, eta, si, bad in cases:
        d.hyper = _hyper_tensor(hy, dev)
        d.eta = torch.from_numpy(eta).to(dev)
        d.wsumsq.fill_(SENTINEL)
        d.trust.fill_(SENTINEL)
        d.trust_dev(a, tables=_tables_with(d.t, dev, seg_item=si))
        torch.cuda.synchronize()
        ss, tr = d.wsumsq.cpu().numpy(), d.trust.cpu().numpy()
        skip = set(bad) | ({bad[0] + 1} if name == "items-empty" else set())        # the neighbour took the items over
        for s in range(h.t.S):
            if s in bad:
                assert ss[s] == SENTINEL and tr[s] == SENTINEL, name
            elif s not in skip:
                assert ss[s].tobytes() == h.wsumsq[s].tobytes() and tr[s].tobytes() == h.trust[s].tobytes(), (name, s)
    assert torch.equal(_bits(d.w), _bits(w0)) and d.guards_intact()


def test_the_flagship_layout_once():
    dev = _dev()
    off, names = step_ref.model_seg_off("M")
    n, S = int(off[-1]), len(names)
    assert S == 316 and 3.7e6 < n < 3.9e6
    hy = grc.ones(S)
    one_d = [i for i, k in enumerate(names) if off[i + 1] - off[i] <= 2048 and ("bn" in k or k.endswith("bias"))]
    hy["wd_scale"][one_d] = 0.0
    eta = np.full(S, 0.001, np.float32)
    eta[one_d] = 0.0
    assert len(one_d) > 100
    a = dict(first=0, gs=0.125, wd=5e-5, mu=0.9, nesterov=1, clip=0, state=True)
    g, w0, m0 = gc.normals(n, 51, 0.02), gc.normals(n, 52, 0.05), gc.normals(n, 53, 0.01)
    d, h = DeviceLars(off, dev, hyper=hy, eta=eta), lc.HostLars(off, hyper=hy, eta=eta)
    for x in (d, h):
        x.load(w0, g, m0)
        x.run(a, g, 2.0)
    _same_as_twin(d, h)
    tr = d.trust.cpu().numpy()
    assert float(h.coef()) < 1.0 and np.all(tr[one_d] == 1.0) and np.all(np.delete(tr, one_d) != 1.0)
    bad = g.copy()
    bad[n // 2] = np.nan
    for x in (d, h):
        x.run(a, bad, 2.0)
    _same_as_twin(d, h)
    assert d.state.cpu()[5:].tolist() == [1, 1, 1]


def test_measure_trust_apply_lars_and_keep_captured_into_one_graph():
    """What a guarded LARS step enqueues after the backward pass -- measure, trust, apply_lars, restore -- captured once and
    replayed on new contents: good, bad, good."""
    dev = _dev()
    off = gc.synthetic()
    a = dict(first=0, gs=1.0, wd=5e-5, mu=0.9, nesterov=1, clip=0, state=True)
    max_norm = 10.0
    d, h = DeviceLars(off, dev, R=8), lc.HostLars(off, R=8)
    hk = gc.HostKeep(seed=80)
    hk.state = h.state
    dk = DeviceKeep(dev)
    dk.state = d.state
    for b, v in zip(dk.live, hk.live):
        b.copy_(torch.from_numpy(v))
    w0, m0 = gc.normals(N, 81), gc.normals(N, 82, 0.1)
    good1, bad, good2 = gc.normals(N, 83), gc.normals(N, 84), gc.normals(N, 85)
    bad[int(off[5])] = np.inf
    d.load(w0, good1, m0)
    h.load(w0, good1, m0)

    def device_tail():
        d.measure(max_norm)
        d.trust_dev(a)
        d.apply_lars(a)
        stepops.keep(dk.kt, d.state, _steplib.KEEP_RESTORE)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                           # one eager step first, as a capture's warm-up does
        stepops.keep(dk.kt, d.state, _steplib.KEEP_SAVE)
        device_tail()
    torch.cuda.current_stream().wait_stream(s)
    hk.keep(_steplib.KEEP_SAVE)
    h.run(a, good1, max_norm)
    hk.keep(_steplib.KEEP_RESTORE)
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
        h.run(a, g, max_norm)
        hk.keep(_steplib.KEEP_RESTORE)
        torch.cuda.synchronize()
        for b, hb in zip(dk.live, hk.live):
            assert torch.equal(_bits(b), _bits(hb))
        words.append(d.state.cpu()[5:].tolist())
        _same_as_twin(d, h)
    assert words == [[0, 0, 0], [1, 1, 1], [0, 1, 0]] and dk.guards_intact()


def test_the_unguarded_form_captured_and_replayed_on_new_contents():
    """observe, trust and apply_lars(state = NULL) captured: the launches read eta and the scales from device memory, so a
    table changed between replays (outside the graph) is what the next replay applies."""
    dev = _dev()
    off = gc.synthetic()
    a = dict(first=0, gs=0.5, wd=5e-5, mu=0.9, nesterov=1, clip=1, state=False)
    d, h = DeviceLars(off, dev), lc.HostLars(off)
    w0, m0 = gc.normals(N, 71), gc.normals(N, 72, 0.1)
    grads = [gc.normals(N, 73 + i) for i in range(3)]
    d.load(w0, grads[0], m0)
    h.load(w0, grads[0], m0)

    def device_tail():
        d.measure()
        d.trust_dev(a)
        d.apply_lars(a, state=False)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        device_tail()
    torch.cuda.current_stream().wait_stream(s)
    h.run(a, grads[0])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        device_tail()
    for i, g in enumerate(grads):
        if i == 2:                                       # new rates, copied outside the graph into the same tensor
            h.eta = lc.etas(h.t.S)[::-1].copy()
            d.eta.copy_(torch.from_numpy(h.eta))
        d.load(g=g)
        graph.replay()
        h.run(a, g)
        _same_as_twin(d, h)
    assert d.state.cpu()[5:].tolist() == [0, 0, 0] and int(d.state[0]) == 4
