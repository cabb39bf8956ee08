"""The guarded update on the GPU: x3dstep_measure, x3dstep_apply and x3dstep_keep against ops.sgd_fused (the kernel the
update replaces) and against the library's CPU twin (which tests/test_guard_host.py holds against the numpy restatement),
bit for bit, at every alignment, inside guard bands, after planted non-finite values, and captured into one graph."""
import numpy as np
import pytest
import torch

from tests import guard_cases as gc
from tests import step_ref
from x3dhip import _steplib, stepops

pytestmark = pytest.mark.gpu

N = 16384
GUARD, FILL = gc.GUARD, gc.FILL


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _banded(n, shift, dev):
    big = torch.full((GUARD + shift + n + GUARD,), FILL, dtype=torch.float32, device=dev)
    view = big[GUARD + shift:GUARD + shift + n]
    assert view.data_ptr() % 16 == 4 * (shift % 4)
    return big, view


class DeviceGuard:
    """The device's buffers for one segment table: w, g and m inside guard bands at the given element shifts."""

    def __init__(self, seg_off, dev, R=4, shifts=(0, 0, 0)):
        self.t = stepops.StepTables(seg_off, dev)
        self.R, self.shifts = R, shifts
        self.state = torch.from_numpy(stepops.new_state()).to(dev)
        self.ws = torch.zeros(self.t.workspace_bytes, dtype=torch.uint8, device=dev)
        self.ring = torch.zeros(R * self.t.record_bytes, dtype=torch.uint8, device=dev)
        (self.wbig, self.w), (self.gbig, self.g), (self.mbig, self.m) = (_banded(self.t.n, s, dev) for s in shifts)

    def load(self, w=None, g=None, m=None):
        for dst, src in ((self.w, w), (self.g, g), (self.m, m)):
            if src is not None:
                dst.copy_(torch.from_numpy(src))

    def measure(self, max_norm=0.0, inv_world=1.0):
        stepops.measure(self.g, self.t, self.ws, self.state, self.ring, self.R, max_norm, inv_world)

    def apply(self, a, lr=gc.LR):
        stepops.apply(self.w, self.g, self.m, self.t, self.state, self.ring, self.R, lr, a["mu"], a["wd"], a["gs"],
                      bool(a["first"]))

    def step(self, g, a, max_norm=0.0):
        self.load(g=g)
        self.measure(max_norm)
        self.apply(a)

    def guards_intact(self):
        ok = True
        for big, s in zip((self.wbig, self.gbig, self.mbig), self.shifts):
            lo, hi = GUARD + s, GUARD + s + self.t.n
            ok = ok and bool((big[:lo] == FILL).all()) and bool((big[hi:] == FILL).all())
        return ok


def _bits(t):
    return (t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))).cpu().view(torch.int32)


def _same_as_twin(d, h):
    torch.cuda.synchronize()
    assert torch.equal(_bits(d.w), _bits(h.w)) and torch.equal(_bits(d.m), _bits(h.m)) and torch.equal(_bits(d.g), _bits(h.g))
    assert torch.equal(d.state.cpu(), torch.from_numpy(h.state))
    assert torch.equal(d.ring.cpu(), torch.from_numpy(np.ascontiguousarray(h.ring)))
    assert d.guards_intact()


def _sgd_fused(w0, g, m0, a, dev, scale_by=None):
    """ops.sgd_fused on the same inputs: (w, m).  scale_by: (tables-sized observe) -- the gradient x3dstep_observe scaled."""
    from x3dhip import ops
    w, m, gg = (torch.from_numpy(v.copy()).to(dev) for v in (w0, m0, g))
    if scale_by is not None:
        t = stepops.StepTables(scale_by[0], dev)
        ws = torch.zeros(t.workspace_bytes, dtype=torch.uint8, device=dev)
        ring = torch.zeros(t.record_bytes, dtype=torch.uint8, device=dev)
        state = torch.from_numpy(stepops.new_state()).to(dev)
        stepops.observe(gg, t, ws, state, ring, 1, scale_by[1], 1.0)
    ops.sgd_fused(w, gg, m, gc.LR, a["mu"], a["wd"], a["gs"], first=bool(a["first"]))
    return w, m


def test_apply_equals_sgd_fused_and_the_twin_over_the_arithmetic_grid():
    dev = _dev()
    off = gc.synthetic()
    w0, m0 = gc.normals(N, 6), gc.normals(N, 7, 0.1)
    for a in gc.ARITH:
        g, max_norm = gc.gradient_for(a, N, 5)
        d, h = DeviceGuard(off, dev), gc.HostGuard(off)
        for x in (d, h):
            x.load(w0, g, m0)
            x.measure(max_norm)
            x.apply(a)
        _same_as_twin(d, h)
        w, m = _sgd_fused(w0, g, m0, a, dev, scale_by=(off, max_norm) if a["clipped"] else None)
        assert torch.equal(d.w, w) and torch.equal(d.m, m), gc.arith_id(a)
        assert torch.equal(_bits(d.g), _bits(g)), "g is left unscaled"
        assert d.state.cpu()[5:].tolist() == [0, 0, 0]


@pytest.mark.parametrize("shifts", [(0, 0, 0), (1, 1, 1), (2, 2, 2), (3, 3, 3), (0, 1, 2)], ids=lambda s: "shift%d%d%d" % s)
@pytest.mark.parametrize("max_norm", [0.0, 10.0], ids=["coef1", "clipped"])
def test_apply_at_every_alignment(shifts, max_norm):
    dev = _dev()
    off = gc.synthetic()
    a = dict(first=0, gs=0.5, wd=5e-5, mu=0.9)
    g, w0, m0 = gc.normals(N, 15), gc.normals(N, 16), gc.normals(N, 17, 0.1)
    d, h = DeviceGuard(off, dev, shifts=shifts), gc.HostGuard(off, shifts=shifts)
    for x in (d, h):
        x.load(w0, g, m0)
        x.measure(max_norm)
        x.apply(a)
    _same_as_twin(d, h)
    w, m = _sgd_fused(w0, g, m0, a, dev, scale_by=(off, max_norm) if max_norm > 0 else None)
    assert torch.equal(d.w, w) and torch.equal(d.m, m) and not torch.equal(d.w.cpu(), torch.from_numpy(w0))
    assert (float(h.coef()) < 1.0) == (max_norm > 0)


def test_apply_on_every_edge_length():
    dev = _dev()
    a = dict(first=0, gs=1.0, wd=5e-5, mu=0.9)
    for n in step_ref.EDGE_LENGTHS + [4096 + 5, 3 * 4096]:      # ... and around a workgroup's run of 1024 groups
        for shifts in ((n % 4,) * 3, (2, 0, 1)):
            off = step_ref.seg_off_of([n])
            g, w0, m0 = gc.normals(n, 25), gc.normals(n, 26), gc.normals(n, 27, 0.1)
            d, h = DeviceGuard(off, dev, shifts=shifts), gc.HostGuard(off, shifts=shifts)
            for x in (d, h):
                x.load(w0, g, m0)
                x.measure(0.5)
                x.apply(a)
            _same_as_twin(d, h)


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf], ids=["nan", "+inf", "-inf"])
def test_a_planted_nonfinite_leaves_w_and_m_bitwise_as_before(value):
    dev = _dev()
    off = gc.synthetic()
    a = dict(first=0, gs=1.0, wd=5e-5, mu=0.9)
    good, w0, m0 = gc.normals(N, 35), gc.normals(N, 36), gc.normals(N, 37, 0.1)
    for shifts, at in (((0, 0, 0), 0), ((1, 1, 1), N - 1), ((0, 1, 2), 7000)):
        bad = good.copy()
        bad[at] = value
        d, h = DeviceGuard(off, dev, R=2, shifts=shifts), gc.HostGuard(off, R=2, shifts=shifts)
        for x in (d, h):
            x.load(w0, None, m0)
            x.step(good, a, 1.0)
        torch.cuda.synchronize()
        before = (d.w.clone(), d.m.clone())
        for x in (d, h):
            x.step(bad, a, 1.0)
            x.step(bad, a, 1.0)
        torch.cuda.synchronize()
        assert torch.equal(_bits(d.w), _bits(before[0])) and torch.equal(_bits(d.m), _bits(before[1]))
        assert d.state.cpu()[5:].tolist() == [1, 2, 2] == list(h.words())
        for x in (d, h):
            x.step(good, a, 1.0)
        _same_as_twin(d, h)
        assert d.state.cpu()[5:].tolist() == [0, 2, 0] and not torch.equal(d.w, before[0])


def test_apply_before_any_measure_stores_nothing():
    dev = _dev()
    d = DeviceGuard(gc.synthetic(), dev)
    w0, m0 = gc.normals(N, 41), gc.normals(N, 42)
    d.load(w0, gc.normals(N, 43), m0)
    d.apply(dict(first=0, gs=1.0, wd=0.0, mu=0.9))
    torch.cuda.synchronize()
    assert torch.equal(_bits(d.w), _bits(w0)) and torch.equal(_bits(d.m), _bits(m0))
    assert torch.equal(d.state.cpu(), torch.from_numpy(stepops.new_state())) and d.guards_intact()
    with pytest.raises(ValueError):
        stepops.apply(d.w.cpu(), d.g, d.m, d.t, d.state, d.ring, d.R, 0.1)
    with pytest.raises(ValueError):
        stepops.apply(d.w[:-1], d.g, d.m, d.t, d.state, d.ring, d.R, 0.1)
    with pytest.raises(ValueError):
        stepops.measure(d.g.cpu(), d.t, d.ws, d.state, d.ring, d.R)
    with pytest.raises(Exception):
        stepops.apply(d.g, d.g, d.m, d.t, d.state, d.ring, d.R, 0.1)             # w and g the same buffer


def test_the_flagship_layout_once():
    dev = _dev()
    off = step_ref.model_seg_off("M")[0]
    n = int(off[-1])
    a = dict(first=0, gs=0.125, wd=5e-5, mu=0.9)
    g, w0, m0 = gc.normals(n, 51, 0.02), gc.normals(n, 52, 0.05), gc.normals(n, 53, 0.01)
    d, h = DeviceGuard(off, dev), gc.HostGuard(off)
    for x in (d, h):
        x.load(w0, g, m0)
        x.measure(2.0, 0.125)
        x.apply(a)
    _same_as_twin(d, h)
    assert float(h.coef()) < 1.0
    bad = g.copy()
    bad[n // 2] = np.nan
    for x in (d, h):
        x.load(g=bad)
        x.measure(2.0, 0.125)
        x.apply(a)
    _same_as_twin(d, h)
    assert d.state.cpu()[5:].tolist() == [1, 1, 1]


# -- keep -----------------------------------------------------------------------------------------------------------------------
class DeviceKeep:
    def __init__(self, dev, lengths=gc.KEEP_LENGTHS, stagger=True, seed=0):
        pairs = [_banded(k, (i % 4) if stagger else 0, dev) for i, k in enumerate(lengths)]
        self.bigs, self.live = [p[0] for p in pairs], [p[1] for p in pairs]
        self.kt = stepops.KeepTable(self.live, dev)
        self.state = torch.from_numpy(stepops.new_state()).to(dev)

    def guards_intact(self):
        ok = True
        for big, b in zip(self.bigs, self.live):
            lo = (b.data_ptr() - big.data_ptr()) // 4
            ok = ok and bool((big[:lo] == FILL).all()) and bool((big[lo + b.numel():] == FILL).all())
        return ok


@pytest.mark.parametrize("stagger", [False, True], ids=["aligned", "staggered"])
@pytest.mark.parametrize("skip_word", [0, 1])
def test_keep_equals_the_twin(stagger, skip_word):
    dev = _dev()
    h = gc.HostKeep(stagger=stagger, seed=60)
    d = DeviceKeep(dev, stagger=stagger)
    assert np.array_equal(d.kt.table["offset"], h.kt.table["offset"]) and d.kt.nitems == h.kt.nitems
    for b, v in zip(d.live, h.live):
        b.copy_(torch.from_numpy(v))
    stepops.keep(d.kt, d.state, _steplib.KEEP_SAVE)
    h.keep(_steplib.KEEP_SAVE)
    torch.cuda.synchronize()
    assert torch.equal(_bits(d.kt.snap), _bits(h.kt.snap)) and d.guards_intact()
    new = [gc.normals(b.size, 70 + i) for i, b in enumerate(h.live)]
    for b, hb, v in zip(d.live, h.live, new):
        b.copy_(torch.from_numpy(v))
        hb[:] = v
    d.state[_steplib.S_SKIP] = skip_word
    h.state[_steplib.S_SKIP] = skip_word
    stepops.keep(d.kt, d.state, _steplib.KEEP_RESTORE)
    h.keep(_steplib.KEEP_RESTORE)
    torch.cuda.synchronize()
    for b, hb, v in zip(d.live, h.live, new):
        assert torch.equal(_bits(b), _bits(hb))
        assert torch.equal(_bits(b), _bits(v)) == (skip_word == 0)       # a no-op when S_SKIP is 0
    assert torch.equal(_bits(d.kt.snap), _bits(h.kt.snap)) and d.guards_intact()
    with pytest.raises(ValueError):
        stepops.keep(d.kt, d.state.cpu(), _steplib.KEEP_SAVE)
    with pytest.raises(ValueError):
        stepops.keep(d.kt, d.state, 2)


# -- one graph ------------------------------------------------------------------------------------------------------------------
def test_measure_apply_and_keep_captured_into_one_graph():
    """What a guarded step enqueues after the backward pass -- measure, apply, restore -- captured once and replayed on
    new contents: good, bad, good.  (The save runs before each replay, as the Trainer runs it before each forward.)"""
    dev = _dev()
    off = gc.synthetic()
    a = dict(first=0, gs=1.0, wd=5e-5, mu=0.9)
    max_norm = 10.0
    d, h = DeviceGuard(off, dev, R=8), gc.HostGuard(off, R=8)
    hk = gc.HostKeep(seed=80)
    hk.state = h.state                                   # one state for the update and the kept buffers
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
        d.apply(a)
        stepops.keep(dk.kt, d.state, _steplib.KEEP_RESTORE)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                           # one eager step first, as a capture's warm-up does
        stepops.keep(dk.kt, d.state, _steplib.KEEP_SAVE)
        device_tail()
    torch.cuda.current_stream().wait_stream(s)
    hk.keep(_steplib.KEEP_SAVE)
    h.step(good1, a, max_norm)
    hk.keep(_steplib.KEEP_RESTORE)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        device_tail()
    # the capture ran nothing: the twin does not step for it
    expect_words = []
    for i, g in enumerate((good1, bad, good2)):
        stepops.keep(dk.kt, d.state, _steplib.KEEP_SAVE)
        hk.keep(_steplib.KEEP_SAVE)
        kept = [b.copy() for b in hk.live]
        d.load(g=g)
        fresh = [gc.normals(b.size, 90 + 10 * i + j) for j, b in enumerate(hk.live)]   # what a forward pass would write
        for b, hb, v in zip(dk.live, hk.live, fresh):
            b.copy_(torch.from_numpy(v))
            hb[:] = v
        graph.replay()
        h.step(g, a, max_norm)
        hk.keep(_steplib.KEEP_RESTORE)
        torch.cuda.synchronize()
        skipped = i == 1
        for b, hb, old, v in zip(dk.live, hk.live, kept, fresh):
            assert torch.equal(_bits(b), _bits(hb)) and torch.equal(_bits(b), _bits(old if skipped else v))
        expect_words.append(d.state.cpu()[5:].tolist())
    _same_as_twin(d, h)
    assert expect_words == [[0, 0, 0], [1, 1, 1], [0, 1, 0]] and dk.guards_intact()
    assert int(d.state[_steplib.S_STEP]) == 4
