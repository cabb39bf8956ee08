"""The weight average on the GPU: x3dstep_ema, x3dstep_ema_keep, x3dstep_swap and x3dstep_swap_keep against the library's CPU
twins (which tests/test_ema_host.py holds against the numpy restatement), bit for bit, over the same grids of lengths,
alignments, decays and counts, inside guard bands, with a skip word, and captured into one graph with the guarded update."""
import numpy as np
import pytest
import torch

from tests import ema_cases as ec
from tests import guard_cases as gc
from tests.test_guard_gpu import DeviceGuard, DeviceKeep, _banded, _bits
from x3dhip import _steplib, stepops

pytestmark = pytest.mark.gpu

N = 16384
GUARD, FILL = gc.GUARD, gc.FILL


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _intact(big, shift, n):
    lo, hi = GUARD + shift, GUARD + shift + n
    return bool((big[:lo] == FILL).all()) and bool((big[hi:] == FILL).all())


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _dstate(state, dev):
    return None if state is None else _up(state, dev)


def _bit_patterns(n, seed):
    bits = np.random.default_rng(seed).integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    special = np.array([0x7fc00001, 0xffc12345, 0x7f800001, 0xff8fffff, 0x7f800000, 0xff800000, 0x80000000, 0, 1, 0x80000001],
                       np.uint32)
    m = min(n, special.size)
    bits[:m] = special[:m]
    return bits.view(np.float32)


@pytest.mark.parametrize("n", ec.LENGTHS + [4 * 4096 + 5])          # ... and past one workgroup's run of 1024 groups
def test_ema_equals_the_twin_over_the_grid(n):
    dev = _dev()
    e0, w = gc.normals(n, 100 + n), gc.normals(n, 200 + n, 0.5)
    de0, dw0 = _up(e0, dev), _up(w, dev)
    moved = 0
    for se, sw in ec.SHIFTS:
        (ebig, e), (wbig, wv) = _banded(n, se, dev), _banded(n, sw, dev)
        (_, he), (_, hw) = gc.banded(n, se), gc.banded(n, sw)
        wv.copy_(dw0)
        hw[:] = w
        for decay in ec.DECAYS:
            for warmup in (True, False):
                for k in ec.KS:
                    he[:] = e0
                    stepops.ema_host(he, hw, None, k, decay, warmup)
                    want = _up(he, dev)
                    moved += int(not torch.equal(_bits(want), _bits(de0)))
                    for with_state in (False, True):
                        for state, count in ec.counts(k, with_state):
                            ds = _dstate(state, dev)
                            e.copy_(de0)
                            stepops.ema(e, wv, ds, count, decay, warmup)
                            assert torch.equal(e.view(torch.int32), want.view(torch.int32)), (se, sw, decay, warmup, k, count)
                            assert ds is None or torch.equal(ds.cpu(), torch.from_numpy(state))     # only read
        assert torch.equal(_bits(wv), _bits(dw0)), "w is only read"
        assert _intact(ebig, se, n) and _intact(wbig, sw, n)
    assert moved > 0


def test_a_skip_word_of_1_and_a_count_of_zero_store_nothing():
    dev = _dev()
    n = 4097
    e0, w = _up(gc.normals(n, 1), dev), _up(gc.normals(n, 2), dev)
    for se, sw in ec.SHIFTS:
        (ebig, e), (wbig, wv) = _banded(n, se, dev), _banded(n, sw, dev)
        e.copy_(e0)
        wv.copy_(w)
        stepops.ema(e, wv, _up(ec.state_for(4, 0, skip=1), dev), 0, 0.9, True)
        stepops.ema(e, wv, _up(ec.state_for(4, 0), dev), -4, 0.9, True)          # k = 0: the kernel leaves
        stepops.ema(e, wv, _up(ec.state_for(4, 0), dev), -9, 0.9, True)          # k < 0
        stepops.ema(e, wv, None, 0, 0.9, True)
        torch.cuda.synchronize()
        assert torch.equal(_bits(e), _bits(e0)) and torch.equal(_bits(wv), _bits(w))
        assert _intact(ebig, se, n) and _intact(wbig, sw, n)
        stepops.ema(e, wv, _up(ec.state_for(4, 0, skip=2), dev), 0, 0.9, True)   # only the value 1 skips
        assert not torch.equal(_bits(e), _bits(e0))
    with pytest.raises(ValueError):
        stepops.ema(e.cpu(), wv, None, 1, 0.9)
    with pytest.raises(ValueError):
        stepops.ema(e, wv[:-1], None, 1, 0.9)
    with pytest.raises(ValueError):
        stepops.ema(e, wv, None, 1, 1.0)
    with pytest.raises(Exception):
        stepops.ema(e, e, None, 1, 0.9)                                          # e and w the same buffer


class DeviceEmaKeep(DeviceKeep):
    """The device's copy of an ec.HostEmaKeep: the same lengths and shifts, the same contents."""

    def __init__(self, dev, h, rot):
        pairs = [_banded(k, (i + rot) % 4, dev) for i, k in enumerate(h.lengths)]
        self.bigs, self.live = [p[0] for p in pairs], [p[1] for p in pairs]
        for b, v in zip(self.live, h.live):
            b.copy_(torch.from_numpy(v))
        self.kt = stepops.KeepTable(self.live, dev)
        self.ebig, self.esnap = _banded(self.kt.snap_n, 0, dev)
        self.esnap.copy_(torch.from_numpy(h.esnap))

    def all_intact(self):
        return self.guards_intact() and _intact(self.ebig, 0, self.kt.snap_n)


@pytest.mark.parametrize("rot", [0, 1, 2, 3])
def test_ema_keep_and_swap_keep_equal_the_twins(rot):
    dev = _dev()
    h = ec.HostEmaKeep(rot=rot, seed=10 * rot)
    d = DeviceEmaKeep(dev, h, rot)
    assert np.array_equal(d.kt.table["offset"], h.kt.table["offset"]) and d.kt.nitems == h.kt.nitems
    for decay, warmup, kk, with_state in ((0.9, True, 1, True), (0.9, True, 10, False), (0.9999, True, 89991, True),
                                          (0.5, False, 2, True), (0.0, False, 9, False)):
        for state, count in ec.counts(kk, with_state):
            fresh = gc.normals(h.kt.snap_n, 33 + count)
            h.esnap[:] = fresh
            d.esnap.copy_(torch.from_numpy(fresh))
            stepops.ema_keep_host(h.kt, h.esnap, state, count, decay, warmup)
            stepops.ema_keep(d.kt, d.esnap, _dstate(state, dev), count, decay, warmup)
            assert torch.equal(_bits(d.esnap), _bits(h.esnap)) and not torch.equal(_bits(d.esnap), _bits(fresh))
    skipped = d.esnap.clone()
    stepops.ema_keep(d.kt, d.esnap, _up(ec.state_for(3, 0, skip=1), dev), 0, 0.9, True)
    stepops.ema_keep(d.kt, d.esnap, _up(ec.state_for(3, 0), dev), -3, 0.9, True)
    assert torch.equal(_bits(d.esnap), _bits(skipped))
    for b, v in zip(d.live, h.live):
        assert torch.equal(_bits(b), _bits(v)), "the live buffers are only read"
    assert d.all_intact()
    # the exchange, on bit patterns
    for i, (b, v) in enumerate(zip(d.live, h.live)):
        v[:] = _bit_patterns(v.size, 300 + i)
        b.copy_(torch.from_numpy(v))
    h.esnap[:] = _bit_patterns(h.kt.snap_n, 400)
    d.esnap.copy_(torch.from_numpy(h.esnap))
    live0, snap0 = [b.clone() for b in d.live], d.esnap.clone()
    stepops.swap_keep_host(h.kt, h.esnap)
    stepops.swap_keep(d.kt, d.esnap)
    assert torch.equal(_bits(d.esnap), _bits(h.esnap)) and not torch.equal(_bits(d.esnap), _bits(snap0))
    for b, v in zip(d.live, h.live):
        assert torch.equal(_bits(b), _bits(v))
    stepops.swap_keep(d.kt, d.esnap)
    assert torch.equal(_bits(d.esnap), _bits(snap0)) and all(torch.equal(_bits(b), _bits(v)) for b, v in zip(d.live, live0))
    assert d.all_intact()
    with pytest.raises(ValueError):
        stepops.swap_keep(d.kt, d.esnap[:-4])
    with pytest.raises(ValueError):
        stepops.ema_keep(d.kt, d.esnap, d.esnap, 1, 0.9)


@pytest.mark.parametrize("n", ec.LENGTHS + [4 * 4096 + 5])
def test_swap_exchanges_bits_and_twice_is_the_identity(n):
    dev = _dev()
    a0, b0 = _up(_bit_patterns(n, n), dev), _up(_bit_patterns(n, 5000 + n)[::-1].copy(), dev)
    for sa, sb in ec.SHIFTS:
        (abig, a), (bbig, b) = _banded(n, sa, dev), _banded(n, sb, dev)
        a.copy_(a0)
        b.copy_(b0)
        stepops.swap(a, b)
        assert torch.equal(_bits(a), _bits(b0)) and torch.equal(_bits(b), _bits(a0))
        stepops.swap(a, b)
        assert torch.equal(_bits(a), _bits(a0)) and torch.equal(_bits(b), _bits(b0))
        assert _intact(abig, sa, n) and _intact(bbig, sb, n)
    with pytest.raises(Exception):
        stepops.swap(a, a)


def test_the_flagship_layout_once():
    """X3D-M: the flat buffer of 3.79 M elements and its 168 running-statistics buffers."""
    import x3d
    from x3dhip.weightema import running_stat_buffers
    dev = _dev()
    net = x3d.generate_model("M", n_classes=400)
    n = sum(p.numel() for p in net.parameters())
    lengths = [b.numel() for _, b in running_stat_buffers(net)]
    assert len(lengths) == 168 and n > 3_700_000
    e0, w = gc.normals(n, 51, 0.05), gc.normals(n, 52, 0.05)
    state = ec.state_for(7, -2)
    he, hw = stepops.aligned_bytes(4 * n).view(np.float32), stepops.aligned_bytes(4 * n).view(np.float32)
    he[:], hw[:] = e0, w
    e, wv = _up(e0, dev), _up(w, dev)
    stepops.ema_host(he, hw, state, -2, 0.9999, True)
    stepops.ema(e, wv, _up(state, dev), -2, 0.9999, True)
    assert torch.equal(_bits(e), _bits(he)) and torch.equal(_bits(wv), _bits(w)) and not torch.equal(_bits(e), _bits(e0))
    stepops.swap(e, wv)
    assert torch.equal(_bits(wv), _bits(he)) and torch.equal(_bits(e), _bits(w))
    h = ec.HostEmaKeep(lengths=lengths, rot=0, seed=60)
    d = DeviceEmaKeep(dev, h, 0)
    stepops.ema_keep_host(h.kt, h.esnap, state, -2, 0.9999, True)
    stepops.ema_keep(d.kt, d.esnap, _up(state, dev), -2, 0.9999, True)
    assert torch.equal(_bits(d.esnap), _bits(h.esnap)) and d.all_intact()
    stepops.swap_keep_host(h.kt, h.esnap)
    stepops.swap_keep(d.kt, d.esnap)
    assert torch.equal(_bits(d.esnap), _bits(h.esnap)) and d.all_intact()
    assert all(torch.equal(_bits(b), _bits(v)) for b, v in zip(d.live, h.live))


def test_measure_apply_ema_and_ema_keep_captured_into_one_graph():
    """What a guarded step with a weight average enqueues after the backward pass, captured once and replayed on new
    contents: good, bad, good.  The eager warm-up step is absorbed by a count of -1 (k = 0: the kernels leave without a
    store, and the twin is not called), so that the average moves twice and k ends at 2."""
    dev = _dev()
    off = gc.synthetic()
    a = dict(first=0, gs=1.0, wd=5e-5, mu=0.9)
    max_norm, decay, count = 10.0, 0.9, -1
    d, h = DeviceGuard(off, dev, R=8), gc.HostGuard(off, R=8)
    hk = ec.HostEmaKeep(lengths=gc.KEEP_LENGTHS, rot=0, seed=80)
    dk = DeviceEmaKeep(dev, hk, 0)
    hstate_keep = stepops.KeepTable(hk.live)             # the Trainer's own table of the same buffers: save / restore
    dstate_keep = stepops.KeepTable(dk.live, dev)
    w0, m0 = gc.normals(N, 81), gc.normals(N, 82, 0.1)
    good1, bad, good2 = gc.normals(N, 83), gc.normals(N, 84), gc.normals(N, 85)
    bad[int(off[5])] = np.inf
    d.load(w0, good1, m0)
    h.load(w0, good1, m0)
    (ebig, e), (_, he) = _banded(N, 0, dev), gc.banded(N, 0)
    he[:] = w0
    e.copy_(torch.from_numpy(w0))

    def device_tail():
        d.measure(max_norm)
        d.apply(a)
        stepops.keep(dstate_keep, d.state, _steplib.KEEP_RESTORE)
        stepops.ema(e, d.w, d.state, count, decay, True)
        stepops.ema_keep(dk.kt, dk.esnap, d.state, count, decay, True)

    def host_tail(g, average=True):
        h.step(g, a, max_norm)
        stepops.keep_host(hstate_keep, h.state, _steplib.KEEP_RESTORE)
        if average:
            stepops.ema_host(he, h.w, h.state, count, decay, True)
            stepops.ema_keep_host(hk.kt, hk.esnap, h.state, count, decay, True)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                           # one eager step first, as a capture's warm-up does
        stepops.keep(dstate_keep, d.state, _steplib.KEEP_SAVE)
        device_tail()
    torch.cuda.current_stream().wait_stream(s)
    stepops.keep_host(hstate_keep, h.state, _steplib.KEEP_SAVE)
    host_tail(good1, average=False)
    with pytest.raises(Exception, match="nothing to average"):
        stepops.ema_host(he, h.w, h.state, count, decay, True)
    torch.cuda.synchronize()
    assert torch.equal(_bits(e), _bits(w0)) and torch.equal(_bits(dk.esnap), _bits(hk.esnap))       # k = 0: nothing moved
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        device_tail()
    moved = []
    for i, g in enumerate((good1, bad, good2)):
        stepops.keep(dstate_keep, d.state, _steplib.KEEP_SAVE)
        stepops.keep_host(hstate_keep, h.state, _steplib.KEEP_SAVE)
        d.load(g=g)
        fresh = [gc.normals(b.size, 90 + 10 * i + j) for j, b in enumerate(hk.live)]   # what a forward pass would write
        for b, hb, v in zip(dk.live, hk.live, fresh):
            b.copy_(torch.from_numpy(v))
            hb[:] = v
        before = (e.clone(), dk.esnap.clone())
        graph.replay()
        host_tail(g)
        torch.cuda.synchronize()
        assert torch.equal(_bits(e), _bits(he)) and torch.equal(_bits(dk.esnap), _bits(hk.esnap))
        assert torch.equal(_bits(d.w), _bits(h.w)) and torch.equal(d.state.cpu(), torch.from_numpy(h.state))
        for b, hb in zip(dk.live, hk.live):
            assert torch.equal(_bits(b), _bits(hb))
        moved.append((not torch.equal(_bits(e), _bits(before[0])), not torch.equal(_bits(dk.esnap), _bits(before[1]))))
    assert moved == [(True, True), (False, False), (True, True)]
    st = d.state.cpu()
    assert count + int(st[_steplib.S_STEP]) - int(st[_steplib.S_SKIPPED]) == 2
    assert d.guards_intact() and dk.all_intact() and _intact(ebig, 0, N)
