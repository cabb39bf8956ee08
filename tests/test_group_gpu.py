"""The grouped update on the GPU: x3dstep_apply_groups against the library's CPU twin (which tests/test_group_host.py holds
against the numpy restatement and torch.optim.SGD), bit for bit, at every alignment and inside guard bands, with every
tensor at its own pair of scales; the identity with ops.sgd_fused and x3dstep_apply; planted non-finite values; the
per-item tests; the flagship layout; and both forms captured into a graph."""
import numpy as np
import pytest
import torch

from tests import group_cases as grc
from tests import guard_cases as gc
from tests import step_ref
from tests.test_guard_gpu import DeviceGuard, DeviceKeep, _bits, _dev, _sgd_fused
from x3dhip import _steplib, stepops

pytestmark = pytest.mark.gpu

N = grc.N


def _hyper_tensor(hy, dev):
    return torch.from_numpy(np.stack([hy["lr_scale"], hy["wd_scale"]], axis=1).astype(np.float32)).to(dev).contiguous()


class DeviceGroup(DeviceGuard):
    """DeviceGuard with a hyper table on the device."""

    def __init__(self, seg_off, dev, hyper=None, R=4, shifts=(0, 0, 0)):
        super().__init__(seg_off, dev, R=R, shifts=shifts)
        self.hyper = _hyper_tensor(grc.scales(self.t.S) if hyper is None else hyper, dev)

    def apply_groups(self, a, lr=gc.LR, state=True, items=None):
        t = self.t
        if items is not None:                            # another item table over the same buffers (the per-item tests)
            t = stepops.StepTables(self.t.seg_off, self.t.device)
            t.d_items = items
        stepops.apply_groups(self.w, self.g, self.m, t, self.hyper, self.state if state else None,
                             self.ring if state else None, self.R, lr, a["mu"], a["wd"], a["gs"], a["first"],
                             a.get("nesterov", 0))

    def run(self, a, g, max_norm=0.0, lr=gc.LR):
        self.load(g=g)
        if a["state"]:
            self.measure(max_norm)
        self.apply_groups(a, lr, state=a["state"])


def _same_as_twin(d, h):
    torch.cuda.synchronize()
    assert torch.equal(_bits(d.w), _bits(h.w)) and torch.equal(_bits(d.m), _bits(h.m)) and torch.equal(_bits(d.g), _bits(h.g))
    assert torch.equal(d.state.cpu(), torch.from_numpy(h.state))
    assert torch.equal(d.ring.cpu(), torch.from_numpy(np.ascontiguousarray(h.ring)))
    assert d.guards_intact()


@pytest.mark.parametrize("shifts", grc.SHIFTS, ids=lambda s: "shift%d%d%d" % s)
def test_the_kernel_equals_the_twin_over_the_grid(shifts):
    dev = _dev()
    off = gc.synthetic()
    w0, m0 = gc.normals(N, 6), gc.normals(N, 7, 0.1)
    d = DeviceGroup(off, dev, shifts=shifts)
    state0 = torch.from_numpy(stepops.new_state()).to(dev)
    for a in grc.GRID:
        g, max_norm = grc.gradient_for(a, N, 5)
        h = grc.HostGroup(off, shifts=shifts)
        d.state.copy_(state0)
        d.ring.zero_()
        for x in (d, h):
            x.load(w0, g, m0)
            x.run(a, g, max_norm)
        _same_as_twin(d, h)
        assert not torch.equal(_bits(d.w), _bits(w0)), grc.case_id(a)


def test_the_kernel_on_every_edge_length():
    dev = _dev()
    a = dict(first=0, gs=1.0, wd=5e-5, mu=0.9, nesterov=1, state=True)
    for n in step_ref.EDGE_LENGTHS:
        off = step_ref.seg_off_of([n, 5, n])
        k = 2 * n + 5
        g, w0, m0 = gc.normals(k, 25), gc.normals(k, 26), gc.normals(k, 27, 0.1)
        for shifts in ((n % 4,) * 3, (2, 0, 1)):
            d, h = DeviceGroup(off, dev, shifts=shifts), grc.HostGroup(off, shifts=shifts)
            for x in (d, h):
                x.load(w0, g, m0)
                x.run(a, g, 0.5)
            _same_as_twin(d, h)


def test_all_ones_without_nesterov_is_sgd_fused_and_apply():
    dev = _dev()
    off = gc.synthetic()
    S = len(off) - 1
    w0, m0 = gc.normals(N, 6), gc.normals(N, 7, 0.1)
    for a in gc.ARITH:
        g, max_norm = gc.gradient_for(a, N, 5)
        old, new = DeviceGuard(off, dev), DeviceGroup(off, dev, hyper=grc.ones(S))
        for x in (old, new):
            x.load(w0, g, m0)
            x.measure(max_norm)
        old.apply(a)
        new.apply_groups(a)
        torch.cuda.synchronize()
        assert torch.equal(_bits(new.w), _bits(old.w)) and torch.equal(_bits(new.m), _bits(old.m)), gc.arith_id(a)
        assert torch.equal(new.state, old.state) and new.guards_intact()
        w, m = _sgd_fused(w0, g, m0, a, dev, scale_by=(off, max_norm) if a["clipped"] else None)
        assert torch.equal(_bits(new.w), _bits(w)) and torch.equal(_bits(new.m), _bits(m)), gc.arith_id(a)
        if not a["clipped"]:
            free = DeviceGroup(off, dev, hyper=grc.ones(S))
            free.load(w0, g, m0)
            free.apply_groups(a, state=False)
            assert torch.equal(_bits(free.w), _bits(w)) and torch.equal(_bits(free.m), _bits(m))
            assert torch.equal(free.state.cpu(), torch.from_numpy(stepops.new_state()))


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf], ids=["nan", "+inf", "-inf"])
def test_a_planted_nonfinite_leaves_w_and_m_bitwise_as_before(value):
    dev = _dev()
    off = gc.synthetic()
    a = dict(first=0, gs=1.0, wd=5e-5, mu=0.9, nesterov=1, state=True)
    good, w0, m0 = gc.normals(N, 35), gc.normals(N, 36), gc.normals(N, 37, 0.1)
    for shifts, at in (((0, 0, 0), 0), ((1, 1, 1), N - 1), ((0, 1, 2), 7000)):
        bad = good.copy()
        bad[at] = value
        d, h = DeviceGroup(off, dev, R=2, shifts=shifts), grc.HostGroup(off, R=2, shifts=shifts)
        for x in (d, h):
            x.load(w0, None, m0)
            x.run(a, good, 1.0)
        torch.cuda.synchronize()
        before = (d.w.clone(), d.m.clone())
        for x in (d, h):
            x.run(a, bad, 1.0)
            x.run(a, bad, 1.0)
        torch.cuda.synchronize()
        assert torch.equal(_bits(d.w), _bits(before[0])) and torch.equal(_bits(d.m), _bits(before[1]))
        assert d.state.cpu()[5:].tolist() == [1, 2, 2] == list(h.words())
        for x in (d, h):
            x.run(a, good, 1.0)
        _same_as_twin(d, h)
        assert d.state.cpu()[5:].tolist() == [0, 2, 0] and not torch.equal(d.w, before[0])
        # without a state the same gradient is applied as the arithmetic gives, and no word is written
        words = d.state.clone()
        free = dict(a, state=False)
        for x in (d, h):
            x.run(free, bad, 0.0)
        torch.cuda.synchronize()
        for dv, hv in ((d.w, h.w), (d.m, h.m)):
            dn, hn = dv.cpu().numpy(), np.asarray(hv)
            nan = np.isnan(hn)
            assert np.array_equal(np.isnan(dn), nan) and dn[~nan].tobytes() == hn[~nan].tobytes()
        assert not np.isfinite(d.m.cpu().numpy()[at]) and torch.equal(d.state, words) and d.guards_intact()


def test_apply_groups_before_any_measure_stores_nothing_and_the_wrapper_checks():
    dev = _dev()
    d = DeviceGroup(gc.synthetic(), dev)
    w0, m0 = gc.normals(N, 41), gc.normals(N, 42)
    d.load(w0, gc.normals(N, 43), m0)
    a = dict(first=0, gs=1.0, wd=0.0, mu=0.9, nesterov=0)
    d.apply_groups(a)
    torch.cuda.synchronize()
    assert torch.equal(_bits(d.w), _bits(w0)) and torch.equal(_bits(d.m), _bits(m0))
    assert torch.equal(d.state.cpu(), torch.from_numpy(stepops.new_state())) and d.guards_intact()
    with pytest.raises(ValueError):
        stepops.apply_groups(d.w.cpu(), d.g, d.m, d.t, d.hyper, None, None, 0, 0.1)
    with pytest.raises(ValueError):
        stepops.apply_groups(d.w, d.g, d.m, d.t, d.hyper[:-1], None, None, 0, 0.1)
    with pytest.raises(ValueError):
        stepops.apply_groups(d.w, d.g, d.m, d.t, d.hyper.cpu(), None, None, 0, 0.1)
    with pytest.raises(ValueError):
        stepops.apply_groups(d.w, d.g, d.m, d.t, d.hyper, None, None, 0, 0.1, momentum=0.0, nesterov=True)
    with pytest.raises(Exception):
        stepops.apply_groups(d.g, d.g, d.m, d.t, d.hyper, None, None, 0, 0.1)        # w and g the same buffer
    torch.cuda.synchronize()
    assert torch.equal(_bits(d.w), _bits(w0)) and d.guards_intact()


def test_an_item_that_fails_its_tests_is_exactly_what_is_left_untouched():
    """The tables are device memory nobody checked: one bad item of each kind (tests/group_cases.py) -- every element of
    that item keeps its bytes and every other element is the twin's on the good table."""
    dev = _dev()
    off = gc.synthetic()
    a = dict(first=0, gs=0.5, wd=5e-5, mu=0.9, nesterov=1)
    g, w0, m0 = gc.normals(N, 61), gc.normals(N, 62), gc.normals(N, 63, 0.1)
    h = grc.HostGroup(off)
    h.load(w0, g, m0)
    h.apply_groups(a, state=False)
    d = DeviceGroup(off, dev, shifts=(1, 1, 1))
    for name, items, hy, bad in grc.bad_item_tables(h.t):
        d.load(w0, g, m0)
        d.hyper = _hyper_tensor(hy, dev)
        d.apply_groups(a, state=False, items=torch.from_numpy(items.view(np.uint8).copy()).to(dev))
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


def test_the_flagship_layout_once():
    dev = _dev()
    off, names = step_ref.model_seg_off("M")
    n, S = int(off[-1]), len(names)
    hy = grc.ones(S)
    one_d = [i for i, k in enumerate(names) if off[i + 1] - off[i] <= 2048 and ("bn" in k or k.endswith("bias"))]
    hy["wd_scale"][one_d] = 0.0
    hy["lr_scale"][[i for i, k in enumerate(names) if k.startswith("fc2.")]] = 10.0
    assert len(one_d) > 100 and (hy["lr_scale"] == 10.0).sum() == 2
    a = dict(first=0, gs=0.125, wd=5e-5, mu=0.9, nesterov=1, state=True)
    g, w0, m0 = gc.normals(n, 51, 0.02), gc.normals(n, 52, 0.05), gc.normals(n, 53, 0.01)
    d, h = DeviceGroup(off, dev, hyper=hy), grc.HostGroup(off, hyper=hy)
    for x in (d, h):
        x.load(w0, g, m0)
        x.measure(2.0, 0.125)
        x.apply_groups(a)
    _same_as_twin(d, h)
    assert float(h.coef()) < 1.0
    bad = g.copy()
    bad[n // 2] = np.nan
    for x in (d, h):
        x.load(g=bad)
        x.measure(2.0, 0.125)
        x.apply_groups(a)
    _same_as_twin(d, h)
    assert d.state.cpu()[5:].tolist() == [1, 1, 1]


def test_measure_apply_groups_and_keep_captured_into_one_graph():
    """What a guarded grouped step enqueues after the backward pass -- measure, apply_groups, restore -- captured once and
    replayed on new contents: good, bad, good."""
    dev = _dev()
    off = gc.synthetic()
    a = dict(first=0, gs=1.0, wd=5e-5, mu=0.9, nesterov=1, state=True)
    max_norm = 10.0
    d, h = DeviceGroup(off, dev, R=8), grc.HostGroup(off, R=8)
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
        d.apply_groups(a)
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
        kept = [b.copy() for b in hk.live]
        d.load(g=g)
        fresh = [gc.normals(b.size, 90 + 10 * i + j) for j, b in enumerate(hk.live)]
        for b, hb, v in zip(dk.live, hk.live, fresh):
            b.copy_(torch.from_numpy(v))
            hb[:] = v
        graph.replay()
        h.run(a, g, max_norm)
        hk.keep(_steplib.KEEP_RESTORE)
        torch.cuda.synchronize()
        for b, hb, old, v in zip(dk.live, hk.live, kept, fresh):
            assert torch.equal(_bits(b), _bits(hb)) and torch.equal(_bits(b), _bits(old if i == 1 else v))
        words.append(d.state.cpu()[5:].tolist())
    _same_as_twin(d, h)
    assert words == [[0, 0, 0], [1, 1, 1], [0, 1, 0]] and dk.guards_intact()


def test_the_unguarded_form_captured_and_replayed_on_new_contents():
    """state = NULL captured: the launch reads the scales from device memory, so a table changed between replays (outside
    the graph) is what the next replay applies."""
    dev = _dev()
    off = gc.synthetic()
    a = dict(first=0, gs=0.5, wd=5e-5, mu=0.9, nesterov=1, state=False)
    d, h = DeviceGroup(off, dev), grc.HostGroup(off)
    w0, m0 = gc.normals(N, 71), gc.normals(N, 72, 0.1)
    grads = [gc.normals(N, 73 + i) for i in range(3)]
    d.load(w0, grads[0], m0)
    h.load(w0, grads[0], m0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        d.apply_groups(a, state=False)
    torch.cuda.current_stream().wait_stream(s)
    h.apply_groups(a, state=False)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        d.apply_groups(a, state=False)
    for i, g in enumerate(grads):
        if i == 2:                                       # new scales, copied outside the graph into the same tensor
            h.hyper = grc.scales(h.t.S)[::-1].copy()
            d.hyper.copy_(_hyper_tensor(h.hyper, dev))
        d.load(g=g)
        h.load(g=g)
        graph.replay()
        h.apply_groups(a, state=False)
        _same_as_twin(d, h)
    assert torch.equal(d.state.cpu(), torch.from_numpy(stepops.new_state()))
