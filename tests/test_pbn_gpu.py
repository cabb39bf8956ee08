"""Precise BN statistics on the GPU: x3dstep_pbn_accum and x3dstep_pbn_finish against the library's CPU twins (which
tests/test_pbn_host.py holds against the numpy restatement), bit for bit, over the same grid of channels, splits, batches and
ranks, inside guard bands; the NaN rule; the X3D-M layout once; and keep + accum x 2 + swap_keep + finish captured into one
graph and replayed on new contents."""
import numpy as np
import pytest
import torch

from tests import guard_cases as gc
from tests import pbn_cases as pc
from tests.test_guard_gpu import _banded, _bits
from x3dhip import _steplib, stepops

pytestmark = pytest.mark.gpu

GUARD, FILL = gc.GUARD, gc.FILL


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _bits64(t):
    return (t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))).cpu().view(torch.int64)


class DevicePbn:
    """The device's copy of a pc.HostPbn: the same shapes and shifts."""

    def __init__(self, dev, h, rot):
        pairs = []
        for l, (C, S) in enumerate(h.shapes):
            pairs += [_banded(C * S, (2 * l + rot) % 4, dev), _banded(C * S, (2 * l + 1 + rot) % 4, dev)]
        self.bigs, self.live = [p[0] for p in pairs], [p[1] for p in pairs]
        self.kt = stepops.KeepTable(self.live, dev)
        self.pt = stepops.PbnTable(self.kt, [S for _, S in h.shapes])
        self.sbig, self.snap = _banded(self.kt.snap_n, 0, dev)
        self.snap.fill_(h.SNAP_FILL)
        assert np.array_equal(self.pt.work, h.pt.work) and self.pt.channels == h.pt.channels
        for f in ("mean_off", "var_off", "first", "C", "S"):
            assert np.array_equal(self.pt.layers[f], h.pt.layers[f])

    def load(self, h):
        for b, v in zip(self.live, h.live):
            b.copy_(torch.from_numpy(v))

    def live_equals(self, h):
        return all(torch.equal(_bits(b), _bits(v)) for b, v in zip(self.live, h.live))

    def guards_intact(self):
        n = self.kt.snap_n
        ok = bool((self.sbig[:GUARD] == FILL).all()) and bool((self.sbig[GUARD + n:] == FILL).all())
        for big, b in zip(self.bigs, self.live):
            lo = (b.data_ptr() - big.data_ptr()) // 4
            ok = ok and bool((big[:lo] == FILL).all()) and bool((big[lo + b.numel():] == FILL).all())
        return ok


def _run_both(h, d, kind, K, W):
    """The twin and the kernel over W ranks' batches: (host acc_all, device acc_all, cells)."""
    S = h.shapes[0][1]
    hacc_all = h.pt.new_acc(W).reshape(W, -1)
    dacc_all = d.pt.new_acc(W).view(W, -1)
    at = 0
    for r, kb in enumerate(pc.rank_batches(K, W)):
        hacc, dacc = h.pt.new_acc(), d.pt.new_acc()
        for _ in range(kb):
            h.load_batch(kind, at)
            d.load(h)
            at += S
            stepops.pbn_accum_host(h.pt, hacc)
            stepops.pbn_accum(d.pt, dacc)
            assert d.live_equals(h), "the live buffers are only read"
        hacc_all[r] = hacc
        dacc_all[r].copy_(dacc)
    return hacc_all.reshape(-1), dacc_all.view(-1), at


@pytest.mark.parametrize("S", pc.SPLITS)
@pytest.mark.parametrize("rot", [0, 1, 2, 3])
def test_both_kernels_equal_the_twins_over_the_grid(S, rot):
    dev = _dev()
    h = pc.HostPbn(pc.grid_shapes(S), rot=rot)
    d = DevicePbn(dev, h, rot)
    for kind in pc.KINDS:
        for K in pc.BATCHES:
            for W in pc.RANKS:
                hacc, dacc, cells = _run_both(h, d, kind, K, W)
                assert torch.equal(_bits64(dacc), _bits64(hacc)), (kind, K, W)
                h.snap[:] = h.SNAP_FILL
                d.snap.fill_(h.SNAP_FILL)
                stepops.pbn_finish_host(h.pt, hacc, W, cells, h.snap)
                stepops.pbn_finish(d.pt, dacc, W, cells, d.snap)
                assert torch.equal(_bits(d.snap), _bits(h.snap)), (kind, K, W)
                assert not bool(torch.isnan(d.snap).any()) and d.live_equals(h)
                assert torch.equal(_bits64(dacc), _bits64(hacc)), "finish only reads the accumulators"
    assert d.guards_intact() and h.guards_intact()


def test_the_nan_rule_and_the_wrappers_checks():
    dev = _dev()
    h = pc.HostPbn([(24, 2), (300, 2)])
    d = DevicePbn(dev, h, 0)
    hacc, dacc, cells = _run_both(h, d, "normal", 2, 1)
    odd = [0, 5, 23, 24, 24 + 255, 24 + 256, 24 + 299]
    hacc.reshape(-1, 4)[odd, 0] += 1.0
    dacc.view(-1, 4)[odd, 0] += 1.0
    stepops.pbn_finish_host(h.pt, hacc, 1, cells, h.snap)
    stepops.pbn_finish(d.pt, dacc, 1, cells, d.snap)
    assert torch.equal(_bits(d.snap), _bits(h.snap))
    assert int(torch.isnan(d.snap).sum()) == len(odd) * 2 * 2 and d.guards_intact()
    d.snap.fill_(h.SNAP_FILL)
    stepops.pbn_finish(d.pt, dacc, 1, cells + 1, d.snap)                      # every other channel now miscounts
    assert int(torch.isnan(d.snap).sum()) == (324 - len(odd)) * 2 * 2
    with pytest.raises(ValueError):
        stepops.pbn_accum(d.pt, dacc[:-4])
    with pytest.raises(ValueError):
        stepops.pbn_accum(d.pt, dacc.float())
    with pytest.raises(ValueError):
        stepops.pbn_finish(d.pt, dacc, 2, cells, d.snap)
    with pytest.raises(ValueError):
        stepops.pbn_finish(d.pt, dacc, 1, cells, d.snap[:-4])
    with pytest.raises(ValueError):
        stepops.pbn_accum(h.pt, dacc)
    with pytest.raises(Exception, match="x3dstep_pbn_finish"):
        stepops.pbn_finish(d.pt, dacc, 1, 0, d.snap)


def test_the_flagship_layout_once():
    """X3D-M: 84 BN layers, two splits, 168 buffers."""
    import x3d
    dev = _dev()
    net = x3d.generate_model("M", n_classes=400, base_bn_splits=2)
    shapes = [(m.num_features, m.num_splits) for m in net.modules() if isinstance(m, x3d.SubBatchNorm3d)]
    assert len(shapes) == 84 and {S for _, S in shapes} == {2}
    h = pc.HostPbn(shapes)
    d = DevicePbn(dev, h, 0)
    assert d.kt.nbuf == 168
    hacc, dacc, cells = _run_both(h, d, "normal", 3, 2)
    assert torch.equal(_bits64(dacc), _bits64(hacc))
    stepops.pbn_finish_host(h.pt, hacc, 2, cells, h.snap)
    stepops.pbn_finish(d.pt, dacc, 2, cells, d.snap)
    assert torch.equal(_bits(d.snap), _bits(h.snap)) and d.guards_intact() and not bool(torch.isnan(d.snap).any())


def test_save_two_accums_swap_and_finish_captured_into_one_graph():
    """What PreciseBN.compute enqueues around two forward passes, captured once and replayed on new contents: the `passes`
    are copies from staging buffers the test refills between replays."""
    dev = _dev()
    shapes = [(24, 2), (257, 2), (3, 2)]
    h = pc.HostPbn(shapes)
    d = DevicePbn(dev, h, 0)
    hkt = h.kt                                             # the twin's own snapshot is the keep table's
    state = torch.from_numpy(stepops.new_state()).to(dev)
    hstate = stepops.new_state()
    stage = [[torch.zeros_like(b) for b in d.live] for _ in range(2)]
    dacc = d.pt.new_acc()
    snap = d.kt.snap

    def device_pass():
        stepops.keep(d.kt, state, _steplib.KEEP_SAVE)
        dacc.zero_()
        for k in range(2):
            for b, s in zip(d.live, stage[k]):
                b.copy_(s)
            stepops.pbn_accum(d.pt, dacc)
        stepops.swap_keep(d.kt, snap)
        stepops.pbn_finish(d.pt, dacc, 1, 4, snap)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        device_pass()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        device_pass()
    for i, kind in enumerate(("normal", "hard", "normal")):
        saved = [gc.normals(b.size, 900 + 10 * i + j) for j, b in enumerate(h.live)]
        for b, hb, v in zip(d.live, h.live, saved):
            b.copy_(torch.from_numpy(v))
            hb[:] = v
        stepops.keep_host(hkt, hstate, _steplib.KEEP_SAVE)
        hacc = h.pt.new_acc()
        for k in range(2):
            h.load_batch(kind, 4 * i + 2 * k)
            for s_, v in zip(stage[k], h.live):
                s_.copy_(torch.from_numpy(v))
            stepops.pbn_accum_host(h.pt, hacc)
        stepops.swap_keep_host(hkt, hkt.snap)
        stepops.pbn_finish_host(h.pt, hacc, 1, 4, hkt.snap)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(snap), _bits(hkt.snap)), i
        assert torch.equal(_bits64(dacc), _bits64(hacc))
        for b, hb, v in zip(d.live, h.live, saved):
            assert torch.equal(_bits(b), _bits(v)) and torch.equal(_bits(hb), _bits(v))      # the live values are back
    assert d.guards_intact()
