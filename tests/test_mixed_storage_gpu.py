"""Mixed-storage mode (BASELINE config 5: bf16 storage / fp32 accumulate; include/x3dhip.h X3D_MX_*), kernel level.

The contract under test: a kernel that reads a bf16 tensor computes exactly what its fp32 build computes on the same
values widened to fp32, and a kernel that writes a bf16 tensor stores the round-to-nearest-even bf16 of what its fp32
build would have stored -- nothing else changes (fp32 products and accumulators, fp32 statistics, fp32 weight gradients).
So every case runs the op twice on the GPU through the C ABI -- bf16 tensors, then the same values as fp32 tensors --
and compares BITWISE (fp32 outputs, their statistics, weight gradients) or against torch's RNE `.bfloat16()` of the fp32
result (bf16 outputs).  Statistics that describe a bf16 OUTPUT (BN sums of a forward result, BN-backward sums of a
gradient) are taken from the values as stored, so that the BN which follows sees the statistics of the tensor it reads:
they are compared with fp64 sums over the stored tensor.
The fp32 builds themselves are pinned to the fp64 oracle in tests/test_ops_gpu.py, so parity is transitive.
Where the mixed mode picks another kernel than the fp32 default (P % 4 != 0 at the large-channel layers, the conv1 data
gradient with Cin = 96 and 128 < Cout < 256), the comparison HERE, on random floats, is the fp32 tolerance of test_ops_gpu.py
instead of bitwise; those shapes are held exactly, bf16 rounding and the statistics of the stored tensors included, by
section 5 of tests/test_exact_gpu.py (`torch.equal` against fp64 on integer inputs whose bf16 stores round), which also holds
the same-kernel shapes, the BN-finalize forms of the channelwise kernels and round-to-nearest-even on exact ties."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _canary_bands_around_every_output(request):
    """Every KERNEL-LEVEL test of this file runs with guard-band allocation (x3dhip.ops.set_guard): each buffer the ops layer allocates sits
    between two 4 KB canary bands, checked at teardown -- a kernel that writes outside its output at ANY of these shapes
    (odd planes, P % 4 != 0, tail tiles, strided gathers) fails the test even when its own output is right."""
    kernel_level = request.node.name.startswith(("test_pw", "test_dw333", "test_stem", "test_elementwise", "test_head",
                                                 "test_reduce", "test_three_term"))
    if not torch.cuda.is_available() or not kernel_level:       # (block / model / trainer tests measure memory and hold graphs)
        yield
        return
    from x3dhip import ops
    prev = ops.set_guard(True)
    yield
    torch.cuda.synchronize()
    bad = ops.check_guards()
    ops.set_guard(prev)
    assert not bad, "%d buffers written out of bounds, first: %s" % (len(bad), bad[:6])

BF = torch.bfloat16


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _g(*shape, seed=0, dev=None):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float32).to(dev)


def _q(t):
    """Values exactly representable in bf16, as fp32."""
    return t.bfloat16().float()


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((a == b).all())


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def _stats_of(partial, first, second):
    """partial [N, C, tiles, 2] against the fp64 sums of `first` and `first * second` over (T, H, W)."""
    st = partial.double().sum(2)
    a, b = first.double(), second.double()
    assert _rel(st[..., 0], a.sum(dim=(2, 3, 4))) < 1e-4 + 1e-6
    assert _rel(st[..., 1], (a * b).sum(dim=(2, 3, 4))) < 1e-4


def _coef(N, C, n, seed, dev):
    cols = [1 + 0.2 * _g(N, C, seed=seed, dev=dev)] + [0.2 * _g(N, C, seed=seed + 1 + i, dev=dev) for i in range(n - 1)]
    return torch.stack(cols, -1).contiguous()


PW_FWD = [
    # N, Cin, Cout, T, H, W, act, x bf16, y bf16           kernel the shape lands on
    (2, 24, 54, 4, 16, 16, 1, False, True),     # conv1 stage 1: streaming split-bf16 kernel (pwfs), wide output
    (3, 48, 108, 2, 20, 20, 0, False, True),    # conv1 stage 2 (pwfs), tail chunk
    (2, 54, 24, 4, 16, 16, 2, True, False),     # conv3 stage 1: fp32-MFMA streaming kernel (pw3), wide input
    (2, 108, 48, 2, 14, 14, 2, True, False),    # conv3 stage 2 (pw3)
    (2, 48, 216, 4, 6, 6, 0, False, True),      # layer3.0 conv1: K < 64 -> pw3 with a wide output
    (1, 24, 54, 2, 9, 7, 1, False, True),       # P % 4 != 0: pw3 scalar form, bf16 element stores
    (1, 54, 24, 2, 9, 7, 2, True, False),       # P % 4 != 0: bf16 element loads
    (2, 96, 216, 4, 12, 12, 0, False, True),    # conv1 stage 3: whole-K item kernel (pw6), wide output
    (2, 216, 96, 4, 12, 12, 2, True, False),    # conv3 stage 3 (pw6), wide input
    (2, 432, 192, 2, 6, 6, 2, True, False),     # conv3 stage 4 (pw6, K = 432: dynamic LDS > 64 KB)
    (2, 192, 432, 2, 6, 6, 0, False, True),     # conv1 stage 4 (pw6)
    (2, 54, 54, 2, 8, 8, 2, True, True),        # both sides bf16 (not a model shape: the flags are independent)
    (1, 96, 216, 2, 7, 7, 0, False, True),      # stage 3 with P % 4 != 0 (odd clip sizes): streaming kernel
    (1, 216, 96, 2, 7, 7, 2, True, False),
]


@pytest.mark.parametrize("case", PW_FWD)
def test_pw_fwd_mx(case):
    from x3dhip import ops
    dev = _dev()
    N, Ci, Co, T, H, W, act, xb, yb = case
    x = _q(_g(N, Ci, T, H, W, seed=1, dev=dev)) if xb else _g(N, Ci, T, H, W, seed=1, dev=dev)
    w = _g(Co, Ci, seed=2, dev=dev) / np.sqrt(Ci)
    pre = _coef(N, Ci, 2, 3, dev) if act else None
    wp = ops.pw_pack(w)
    y0, p0 = ops.pw_fwd(x, w, pre=pre, pre_act=act, wp=wp)
    y1, p1 = ops.pw_fwd(x.to(BF) if xb else x, w, pre=pre, pre_act=act, wp=wp, out_dtype=BF if yb else torch.float32)
    assert y1.dtype == (BF if yb else torch.float32)
    # directly against the fp64 oracle on the same (bf16-representable) inputs, not only through the fp32 build: fp32
    # arithmetic error for an fp32 output, one RNE rounding (2^-9 relative per element) on top for a bf16 output
    from oracle import x3d_oracle as xo
    xd = x.double().cpu()
    if act:
        sd = pre.double().cpu()[..., 0, None, None, None] * xd + pre.double().cpu()[..., 1, None, None, None]
        xd = torch.relu(sd) if act == 1 else sd * torch.sigmoid(sd)
    y_ref = xo.pw(xd, w.double().cpu().view(Co, Ci, 1, 1, 1), 1)
    assert _rel(y1.float().cpu(), y_ref) < (3e-3 if yb else 2e-5)
    if yb:
        assert bool(((y1.float().cpu().double() - y_ref).abs() <= y_ref.abs() * 2.0 ** -8 + 1e-5).all())
    if Ci >= 64 and Co >= 96 and (T * H * W) % 4 != 0:
        # the fp32 default for this shape is the LDS-tiled kernel, the mixed mode streams: another summation order
        assert _rel(y1.float(), y0) < (3e-3 if yb else 2e-5)
        if not yb:
            assert _rel(p1.sum(2), p0.sum(2)) < 1e-4
            return
    else:
        assert _same(y1, y0.to(BF) if yb else y0)
    if yb:
        _stats_of(p1, y1, y1)                    # {sum y, sum y^2} of the tensor as stored
    else:
        assert _same(p1, p0)


def test_pw_fwd_mx_needs_a_packed_dense_kernel():
    """No silent fallback: shapes / forms without a mixed-storage kernel raise."""
    from x3dhip import ops, _lib
    dev = _dev()
    x = _g(1, 24, 2, 8, 8, seed=1, dev=dev)
    w = _g(54, 24, seed=2, dev=dev)
    with pytest.raises(_lib.X3DHipError):
        ops.pw_fwd(x, w, wp=None, out_dtype=BF)                 # unpacked weights: generic fp32 kernel only
    with pytest.raises(_lib.X3DHipError):
        ops.pw_fwd(x.double(), w)


FUSED = [
    # N, Cin, Cout, T, H, W      (stage 1-2 shapes: the fused data + weight gradient kernel)
    (2, 24, 54, 4, 16, 16),      # conv1 stage 1 (64 x 32)
    (2, 54, 24, 4, 16, 16),      # conv3 stage 1 (32 x 64)
    (3, 48, 108, 2, 20, 20),     # conv1 stage 2 (128 x 64)
    (2, 108, 48, 2, 14, 14),     # conv3 stage 2 (64 x 128)
    (2, 24, 108, 4, 12, 12),     # layer2.0 conv1 (128 x 32)
]


@pytest.mark.parametrize("case", FUSED)
def test_pw_bwd_fused_mx(case):
    from x3dhip import ops
    dev = _dev()
    N, Ci, Co, T, H, W = case
    w = _g(Co, Ci, seed=2, dev=dev) / np.sqrt(Ci)
    wpt = ops.pw_pack(w, transposed=True)
    cb = _coef(N, Co, 3, 7, dev)
    pre = _coef(N, Ci, 2, 3, dev)
    g, a = _g(N, Co, T, H, W, seed=5, dev=dev), _g(N, Co, T, H, W, seed=6, dev=dev)
    x = _g(N, Ci, T, H, W, seed=1, dev=dev)
    add = _g(N, Ci, T, H, W, seed=10, dev=dev)
    add2 = _g(N, Ci, T, (H - 1) // 2 + 1, (W - 1) // 2 + 1, seed=11, dev=dev)
    ex = _g(N, Ci, T, H, W, seed=13, dev=dev)
    if Co < Ci:
        # conv3 of a bottleneck: the wide tensors are x (its raw input) and dx; activation backward, no addend
        xq = _q(x)
        d0, s0, w0 = ops.pw_bwd_fused(g, a, cb, (Co, Ci), wpt, xq, xpre=pre, xact=2, mode=1)
        d1, s1, w1 = ops.pw_bwd_fused(g, a, cb, (Co, Ci), wpt, xq.to(BF), xpre=pre, xact=2, mode=1)
        assert d1.dtype == BF and _same(d1, d0.to(BF)) and _same(w1, w0)
        _stats_of(s1, d1, xq)                    # {sum dx, sum dx * x} of the gradient as stored
        return
    # conv1: the wide tensors are g and a; all three epilogues, dense and stride-2 addend
    gq, aq = _q(g), _q(a)
    xr = torch.relu(x)
    for kw in (dict(mode=0), dict(mode=0, addend=add), dict(mode=0, addend=add2, addend_stride=2),
               dict(mode=1, xpre=pre, xact=1, addend=add2, addend_stride=2), dict(mode=1, xpre=pre, xact=1),
               dict(mode=2, ex=ex, addend=add), dict(mode=2, ex=ex, addend=add2, addend_stride=2)):
        xin = xr if kw["mode"] == 2 else x
        d0, s0, w0 = ops.pw_bwd_fused(gq, aq, cb, (Co, Ci), wpt, xin, **kw)
        d1, s1, w1 = ops.pw_bwd_fused(gq.to(BF), aq.to(BF), cb, (Co, Ci), wpt, xin, **kw)
        assert d1.dtype == torch.float32 and _same(d1, d0) and _same(w1, w0)
        assert (s0 is None and s1 is None) or _same(s1, s0)


PW_BWD = [
    # N, Cin, Cout, T, H, W, kind        stage 3-4 shapes (separate data-gradient and weight-gradient kernels)
    (2, 216, 96, 4, 12, 12, "conv3"),    # pw7, M = 216
    (2, 432, 192, 2, 6, 6, "conv3"),     # pw7, M = 432
    (1, 216, 96, 2, 7, 7, "conv3"),      # P % 4 != 0 at stage 3 (odd clip sizes): streaming kernel, element loads / stores
    (2, 96, 216, 4, 12, 12, "conv1"),    # K = 216 -> M = 96: fp32 default is the chunked kernel, mixed mode the item kernel
    (2, 192, 432, 2, 6, 6, "conv1"),     # pw7, K = 432
    (2, 48, 216, 4, 6, 6, "conv1"),      # layer3.0 conv1: M = 48 < 96 -> streaming kernel (pw3) with bf16 g, a
    (1, 96, 216, 2, 7, 7, "conv1"),      # P % 4 != 0 at stage 3
]


@pytest.mark.parametrize("case", PW_BWD)
def test_pw_bwd_data_mx(case):
    from x3dhip import ops
    dev = _dev()
    N, Ci, Co, T, H, W, kind = case
    w = _g(Co, Ci, seed=2, dev=dev) / np.sqrt(Ci)
    wpt = ops.pw_pack(w, transposed=True)
    cb = _coef(N, Co, 3, 7, dev)
    pre = _coef(N, Ci, 2, 3, dev)
    g, a = _g(N, Co, T, H, W, seed=5, dev=dev), _g(N, Co, T, H, W, seed=6, dev=dev)
    x = _g(N, Ci, T, H, W, seed=1, dev=dev)
    if kind == "conv3":
        xq = _q(x)
        o0, s0 = ops.pw_bwd_data(g, a, cb, w, x=xq, pre=pre, pre_act=2, wpt=wpt)
        o1, s1 = ops.pw_bwd_data(g, a, cb, w, x=xq.to(BF), pre=pre, pre_act=2, wpt=wpt, out_dtype=BF)
        assert o1.dtype == BF
        if (T * H * W) % 4 != 0:        # fp32 default: LDS-tiled kernel; mixed mode: streaming kernel
            assert _rel(o1.float(), o0) < 3e-3
        else:
            assert _same(o1, o0.to(BF))
        _stats_of(s1, o1, xq)
        return
    gq, aq = _q(g), _q(a)
    add = _g(N, Ci, T, H, W, seed=10, dev=dev)
    res_out, res_raw = torch.relu(x), _g(N, Ci, T, H, W, seed=13, dev=dev)
    same_kernel = not (128 < Co < 256 and Ci == 96) and (T * H * W) % 4 == 0
    o0, _ = ops.pw_bwd_data(gq, aq, cb, w, addend=add, wpt=wpt)
    o1, _ = ops.pw_bwd_data(gq.to(BF), aq.to(BF), cb, w, addend=add, wpt=wpt)
    assert _same(o1, o0) if same_kernel else _rel(o1, o0) < 2e-5
    (o0, s0) = ops.pw_bwd_data_res(gq, aq, cb, w, res_out, res_raw, addend=add, wpt=wpt)
    (o1, s1) = ops.pw_bwd_data_res(gq.to(BF), aq.to(BF), cb, w, res_out, res_raw, addend=add, wpt=wpt)
    if same_kernel:
        assert _same(o1, o0) and _same(s1, s0)
    else:
        assert _rel(o1, o0) < 2e-5 and _rel(s1.sum(2), s0.sum(2)) < 1e-4


@pytest.mark.parametrize("case", PW_BWD + [(2, 54, 24, 4, 16, 16, "conv3"), (2, 24, 54, 4, 16, 16, "conv1")])
@pytest.mark.parametrize("batched", [False, True])
def test_pw_bwd_weight_mx(case, batched):
    from x3dhip import ops
    dev = _dev()
    N, Ci, Co, T, H, W, kind = case
    cb = _coef(N, Co, 3, 7, dev)
    pre = _coef(N, Ci, 2, 3, dev)
    g, a = _g(N, Co, T, H, W, seed=5, dev=dev), _g(N, Co, T, H, W, seed=6, dev=dev)
    x = _g(N, Ci, T, H, W, seed=1, dev=dev)
    if kind == "conv3":
        x = _q(x)
        lo = dict(g=g, a=a, x=x.to(BF), kw=dict(pre=pre, pre_act=2))
        hi = dict(g=g, a=a, x=x, kw=dict(pre=pre, pre_act=2))
    else:
        g, a = _q(g), _q(a)
        lo = dict(g=g.to(BF), a=a.to(BF), x=x, kw={})
        hi = dict(g=g, a=a, x=x, kw={})
    outs = []
    for v in (hi, lo):
        d = ops.DeferredGrads() if batched else None
        dw = ops.pw_bwd_weight(v["g"], v["a"], cb, v["x"], (Co, Ci), defer=d, **v["kw"])
        if d is not None:
            d.flush()
        outs.append(dw)
    assert _same(outs[0], outs[1])


DW = [
    # N, C, T, H, W, stride
    (2, 6, 4, 14, 14, 1),
    (1, 5, 5, 13, 9, 1),      # W % 4 != 0: bf16 element loads / stores
    (2, 4, 4, 16, 16, 2),
    (1, 3, 3, 15, 11, 2),     # odd sizes, stride 2
    (1, 33, 2, 4, 4, 2),      # 16 channels per block + tail
    (1, 2, 3, 40, 56, 1),     # 3 row tiles
    (1, 3, 4, 112, 112, 2),   # one channel per workgroup
    (2, 10, 16, 14, 14, 1),   # stage-3 geometry, T = 16
    (8, 54, 2, 56, 56, 1),    # base-shape stage-1 plane
]


@pytest.mark.parametrize("case", DW)
def test_dw333_mx(case):
    from x3dhip import ops
    dev = _dev()
    N, C, T, H, W, s = case
    Ho, Wo = (H - 1) // 2 + 1 if s == 2 else H, (W - 1) // 2 + 1 if s == 2 else W
    x = _q(_g(N, C, T, H, W, seed=1, dev=dev))
    w = _g(C, 1, 3, 3, 3, seed=2, dev=dev) / 3
    pre = _coef(N, C, 2, 3, dev)
    y0, p0 = ops.dw333_fwd(x, w, stride=s, pre=pre, pre_act=1)
    y1, p1 = ops.dw333_fwd(x.to(BF), w, stride=s, pre=pre, pre_act=1)
    assert y1.dtype == BF and _same(y1, y0.to(BF))
    _stats_of(p1, y1, y1)
    # directly against the fp64 oracle on the same bf16-representable input: one RNE rounding of the output on top of fp32
    from oracle import x3d_oracle as xo
    pd_ = pre.double().cpu()
    hin = torch.relu(pd_[..., 0, None, None, None] * x.double().cpu() + pd_[..., 1, None, None, None])
    y_ref = xo.dw333(hin, w.double().cpu(), s)
    assert _rel(y1.float().cpu(), y_ref) < 3e-3
    assert bool(((y1.float().cpu().double() - y_ref).abs() <= y_ref.abs() * 2.0 ** -8 + 1e-5).all())
    # training form (producer BN finalize in the prologue)
    sp = torch.rand(N, C, 3, 2, device=dev) + 0.5
    sp[..., 1] += 4.0
    gamma, beta = 1 + 0.1 * _g(C, seed=20, dev=dev), 0.1 * _g(C, seed=21, dev=dev)
    r0 = [torch.zeros(1, C, device=dev), torch.ones(1, C, device=dev)]
    r1 = [t.clone() for t in r0]
    o0 = ops.dw333_fwd_stats(x, w, sp, 1, 7, gamma, beta, r0[0].view(-1), r0[1].view(-1), stride=s)
    o1 = ops.dw333_fwd_stats(x.to(BF), w, sp, 1, 7, gamma, beta, r1[0].view(-1), r1[1].view(-1), stride=s)
    assert _same(o1[0], o0[0].to(BF)) and all(_same(u, v) for u, v in zip(o1[2:], o0[2:]))
    _stats_of(o1[1], o1[0], o1[0])
    assert _same(r0[0], r1[0]) and _same(r0[1], r1[1])
    # backward: g, a (output resolution), x and the result are the four wide tensors
    g = _q(_g(N, C, T, Ho, Wo, seed=5, dev=dev))
    a = _q(_g(N, C, T, Ho, Wo, seed=6, dev=dev))
    cb = _coef(N, C, 3, 7, dev)
    d0, w0, b0 = ops.dw333_bwd(g, a, cb, w, x, stride=s, pre=pre, pre_act=1)
    d1, w1, b1 = ops.dw333_bwd(g.to(BF), a.to(BF), cb, w, x.to(BF), stride=s, pre=pre, pre_act=1)
    assert d1.dtype == BF and _same(d1, d0.to(BF)) and _same(w1, w0)
    _stats_of(b1, d1, x)
    # the form the engine calls in every bottleneck: the producer BN's backward finalize in the prologue (bn=...,
    # x3d_dw333_bwd_stats, one split).  The finalize reads fp32 partials only: cb, dgamma and dbeta cannot depend on the storage
    spb = torch.stack([_g(N, C, 3, seed=13, dev=dev), 2 * _g(N, C, 3, seed=14, dev=dev)], -1).contiguous()
    save = torch.stack([0.1 * _g(1, C, seed=15, dev=dev), 1 + 0.1 * _g(1, C, seed=16, dev=dev).abs()], 0).contiguous()
    runs = []
    for gg, aa, xx in ((g, a, x), (g.to(BF), a.to(BF), x.to(BF))):
        dgamma, dbeta = torch.full((C,), float("nan"), device=dev), torch.full((C,), float("nan"), device=dev)
        runs.append(ops.dw333_bwd(gg, aa, None, w, xx, stride=s, pre=pre, pre_act=1,
                                  bn=(spb, T * Ho * Wo, gamma, save, dgamma, dbeta)) + (dgamma, dbeta))
    (d0, w0, b0, dg0, db0), (d1, w1, b1, dg1, db1) = runs
    assert d1.dtype == BF and _same(d1, d0.to(BF)) and _same(w1, w0)
    assert bool(torch.isfinite(dg0).all()) and _same(dg1, dg0) and _same(db1, db0)
    _stats_of(b1, d1, x)


def test_dw333_mx_rejects_mixed_dtypes():
    from x3dhip import ops, _lib
    dev = _dev()
    x = _g(1, 4, 2, 8, 8, seed=1, dev=dev)
    w = _g(4, 1, 3, 3, 3, seed=2, dev=dev)
    cb = _coef(1, 4, 3, 7, dev)
    with pytest.raises(_lib.X3DHipError):
        ops.dw333_bwd(x.to(BF), x, cb, w, x)


# ------------------------------------------------------------------------------------------------------------------
# Block and model level.
#
# The oracle of this mode is the CPU restatement of x3d.py with four rounding hooks switched on (oracle/x3d_oracle.py
# BF16_WIDE): RNE rounding of exactly the tensors the product stores as bf16, at the places it stores them.
#
# What CAN agree, and to what tolerance.  Rounding is a discontinuous map: two evaluations of the same tensor that differ
# by fp32 summation order (1e-7) round a fraction ~ 1e-7 / 2^-8 of its elements to DIFFERENT bf16 neighbours, i.e. they
# leave the rounding with an rms difference of ~ sqrt(1e-7 * 2^-8) -- far more than they entered with -- and after a few
# bottlenecks two such trajectories are as far apart as two independent draws of the bf16 rounding noise itself.  The
# network then amplifies that noise the way it amplifies fp32 noise (fixtures: logits fp32 vs fp64 8e-6, i.e. ~100x the
# unit roundoff).  Hence:
#   * ONE bottleneck from identical inputs (test_block_bf16_vs_oracle): the discrepancy has had one or two roundings to
#     grow -- forward 3e-3, gradients 3e-2 of the norm (measured: ~5e-4 / ~5e-3) -- this pins which tensors are rounded
#     and where;
#   * the whole network (test_train_step_bf16_storage): the product in bf16 mode is as close to the reference's fp32
#     golden vectors as the rounding oracle is (same noise process, independent draws: ratio bound 3), with stated
#     absolute ceilings BF16_RTOL for X3D-M -- logits 0.15, loss 5e-3, global gradient norm 0.15 (measured on MI355X:
#     2-7e-2, 3-6e-4, 3-7e-2; the rounding oracle itself: 2-7e-2, -, 2-4e-2) -- and twice those at the 55-block depth.
#     The gradient DIRECTION of one step is not a criterion in this mode: ReLU decisions of near-zero pre-activations
#     already move it by 1-3e-2 between the reference's own fp32 and fp64 runs (tests/parity.py), and bf16 storage noise is
#     2^15 times larger; what training needs is checked by test_trainer_bf16_storage_trains.
# ------------------------------------------------------------------------------------------------------------------
BF16_RTOL = dict(logits=0.15, loss=5e-3, grad_norm=0.15)


@pytest.mark.parametrize("shape", [(4, 4, 40, 2), (2, 2, 31, 1)])        # the second: P % 4 != 0 in every stage
def test_block_bf16_vs_oracle(shape):
    import x3d
    from oracle import x3d_oracle as xo
    from tests import parity
    from x3dhip import engine, synthetic
    dev = _dev()
    B, T, H, S = shape
    sd = synthetic.procedural_state_dict(xo.state_template("M", 400, S), 0)
    net = x3d.generate_model("M", n_classes=400, dropout=0.0, base_bn_splits=S, act_dtype=BF)
    net.load_state_dict(sd)
    net = net.to(dev).train(True)
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    rows = {r[0]: r for r in xo.block_table("M")}
    gen = torch.Generator().manual_seed(5)
    worst = [0.0, 0.0]
    for name in ["layer1.0", "layer1.1", "layer2.0", "layer3.3", "layer4.0", "layer4.2"]:
        p, cin, cm, co, stride, se, ds = rows[name]
        li, bi = name.split(".")
        blk = getattr(net, li)[int(bi)]
        x = torch.relu(torch.randn(B, cin, T, H, H, generator=gen, dtype=torch.float64))
        leaf = {k: v.clone().requires_grad_(True) for k, v in sd64.items() if k.startswith(p + ".") and xo.is_parameter(k)}
        full = dict(sd64)
        full.update(leaf)
        xr = x.clone().requires_grad_(True)
        xo.BF16_WIDE = True
        try:
            out_ref = xo.bottleneck(xr, full, p, stride, se, ds, S, True, None)
            dout = torch.randn(out_ref.shape, generator=gen, dtype=torch.float64)
            out_ref.backward(dout)
        finally:
            xo.BF16_WIDE = False
        ctx = engine.TrunkContext()
        packs = engine.weight_packs(net)
        packs.refresh()
        out, _ = engine._block_forward(blk, x.float().to(dev), None, S, True, ctx, packs, BF)
        rec = ctx.blocks[0]
        assert rec["a1"].dtype == BF and rec["a2"].dtype == BF and out.dtype == torch.float32
        e_f = parity.rel(out.cpu().numpy(), out_ref.detach().numpy())
        sink = engine._GradSink(False)
        dprev, _ = engine._block_backward(rec, dout.float().to(dev), sink)
        sink.flush()
        e_b = parity.rel(dprev.cpu().numpy(), xr.grad.numpy())
        for k, v in leaf.items():
            mod = blk
            for part in k[len(p) + 1:].split("."):
                mod = getattr(mod, part) if not part.isdigit() else mod[int(part)]
            e_b = max(e_b, parity.rel(sink.written[mod].cpu().numpy().reshape(-1), v.grad.numpy().reshape(-1)))
        worst = [max(worst[0], e_f), max(worst[1], e_b)]
        assert e_f < 3e-3 and e_b < 3e-2, (name, e_f, e_b)
    print("\n[block bf16 vs rounding oracle %s] worst forward %.2e, worst gradient %.2e" % (shape, worst[0], worst[1]))


def _golden_step(golden_dir, case, dev, act_dtype):
    import os
    import x3d
    from oracle import x3d_oracle as xo
    from x3dhip import synthetic
    g = np.load(os.path.join(golden_dir, case + ".npz"))
    B, T, H, S = [int(v) for v in g["shape"]]
    version = case.split("_")[1]
    sd = synthetic.procedural_state_dict(xo.state_template(version, 400, S), int(g["seed"][0]))
    net = x3d.generate_model(version, n_classes=400, dropout=0.0, base_bn_splits=S, act_dtype=act_dtype)
    net.load_state_dict(sd)
    net = net.to(dev).train(True)
    x = synthetic.synthetic_clips(B, T, H, H, seed=int(g["seed"][1]))
    y = synthetic.synthetic_labels(B, seed=int(g["seed"][1]))
    logits = net(x.to(dev))
    loss = torch.nn.CrossEntropyLoss()(logits, y.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().cpu().numpy() for k, p in net.named_parameters()}
    return g, logits.detach().cpu().numpy()[:, :, 0], loss.item(), grads, net, (x, y, sd, version, S)


@pytest.mark.parametrize("case", ["train_M_8x4x64_s2", "train_M_2x8x112_s1", "train_L_4x4x96_s1", "train_XL_2x4x64_s1",
                                  "train_L_2x16x312_s1"])        # the last: BASELINE config 5's literal clip shape, B = 2
def test_train_step_bf16_storage(golden_dir, case):
    from oracle import x3d_oracle as xo
    from tests import parity
    dev = _dev()
    g, logits, loss, grads, net, (x, y, sd, version, S) = _golden_step(golden_dir, case, dev, BF)
    xo.BF16_WIDE = True
    try:
        o_logits, o_loss, o_grads, _ = xo.train_step_grads(x, y, sd, version, S)
    finally:
        xo.BF16_WIDE = False
    gnorm = lambda gr: float(np.sqrt(sum(float((np.asarray(v, dtype=np.float64) ** 2).sum()) for v in gr.values())))
    ref_gn = float(g["grad_global_norm64"])
    hip = dict(logits=parity.rel(logits, g["logits"]), loss=abs(loss - float(g["loss"])) / abs(float(g["loss"])),
               grad_norm=abs(gnorm(grads) - ref_gn) / ref_gn)
    orc = dict(logits=parity.rel(o_logits.numpy()[:, :, 0], g["logits"]),
               loss=abs(o_loss.item() - float(g["loss"])) / abs(float(g["loss"])),
               grad_norm=abs(gnorm({k: v.numpy() for k, v in o_grads.items()}) - ref_gn) / ref_gn)
    print("\n[%s, bf16 storage vs the reference's fp32 golden] HIP: %s | rounding oracle: %s | HIP vs rounding oracle: logits %.2e"
          % (case, " ".join("%s %.2e" % kv for kv in hip.items()), " ".join("%s %.2e" % kv for kv in orc.items()),
             parity.rel(logits, o_logits.numpy()[:, :, 0])))
    depth = 2.0 if version in ("L", "XL") else 1.0       # 55 blocks (XL also: 630-channel layers on the streaming kernels)
    for k in ("logits", "loss", "grad_norm"):
        assert hip[k] < depth * BF16_RTOL[k], (k, hip[k])
    # the same noise process as the CPU restatement with the same rounding points (independent draws): logits, whose error is
    # a norm over B x 400 values and therefore a stable estimate, within a factor 2; loss and gradient norm are single
    # signed numbers (a draw can land near zero), so they only have the ceilings above
    assert hip["logits"] < 2 * orc["logits"] + 1e-3, (hip, orc)
    # eval forward in the same mode after the BN aggregation (x3d.py:306-313)
    net.train(False)
    net.aggregate_sub_bn_stats()
    with torch.no_grad():
        ev = net(x.to(dev))
    assert parity.rel(ev.cpu().numpy()[:, :, 0], g["eval_logits"]) < depth * BF16_RTOL["logits"]


def test_fp32_mode_is_untouched_by_the_mixed_storage_build(golden_dir):
    """act_dtype=torch.float32 (the default) keeps the 1e-3 parity of tests/test_model_gpu.py on the 'L' depth too."""
    from tests import parity
    from x3dhip import synthetic
    dev = _dev()
    g, logits, loss, grads, _, _ = _golden_step(golden_dir, "train_L_4x4x96_s1", dev, torch.float32)
    parity.check_forward(logits, loss, g)
    from tests import gradhash
    rep = parity.check_grads(grads, g, synthetic.gradient_sketch, cond=parity.conditioning("train_L_4x4x96_s1"),
                             case="train_L_4x4x96_s1", pinned="train_L_4x4x96_s1" in gradhash.pinned_cases())
    print("\n[train_L_4x4x96_s1 fp32] " + parity.fmt(rep))


def test_trainer_bf16_storage_trains():
    """Graph-captured training steps in the mixed-storage mode: finite, loss falls on a fixed batch, and the wide
    tensors really are bf16 (the step allocates less than the fp32 mode)."""
    import x3d
    from x3dhip import synthetic
    from x3dhip.trainer import Trainer
    dev = _dev()
    losses, peak = {}, {}
    for dt in (torch.float32, BF):
        torch.manual_seed(0)
        net = x3d.generate_model("M", n_classes=400, dropout=0.0, base_bn_splits=2, act_dtype=dt).to(dev).train(True)
        tr = Trainer(net, lr=0.05, momentum=0.9, weight_decay=1e-5, use_graph=True)
        x = synthetic.synthetic_clips(4, 4, 64, 64, seed=3).to(dev)
        y = synthetic.synthetic_labels(4, seed=3).to(dev)
        torch.cuda.reset_peak_memory_stats()
        ls = [float(tr.train_step(x, y)[0]) for _ in range(8)]
        torch.cuda.synchronize()
        peak[dt] = torch.cuda.max_memory_allocated()
        losses[dt] = ls
        assert all(np.isfinite(ls)), ls
        assert ls[-1] < ls[0], ls
        del tr, net
    print("\nloss fp32 %s\nloss bf16 %s\npeak bytes fp32 %d bf16 %d" % (losses[torch.float32], losses[BF], peak[torch.float32], peak[BF]))
    assert abs(losses[BF][0] - losses[torch.float32][0]) / losses[torch.float32][0] < BF16_RTOL["loss"]
    assert peak[BF] < peak[torch.float32]


def test_multigrid_loop_in_bf16_storage(tmp_path, capsys):
    """The reference's training loop (multigrid shape changes, long-cycle BN-split switches, graph cache, validation phase,
    checkpoint) with act_dtype=torch.bfloat16: every shape of the schedule has a mixed-storage kernel (odd sizes included)."""
    _dev()
    import train_x3d_kinetics_multigrid as tr
    save = str(tmp_path / "ck_")
    steps, cps = tr.run(init_lr=0.01, warmup_steps=5, max_epochs=4, batch_size=2, steps=0, max_steps_run=24,
                        iterations_per_epoch=10, save_model=save, save_every=20, use_graph=True, log_every=10,
                        val_every=15, val_batches=1, val_batch_size=1, act_dtype=BF)
    out = capsys.readouterr().out
    assert steps == 24 and cps > 0
    assert "nan" not in out.lower()
    assert out.count(" val after step") == 1
    import os
    assert os.path.exists(save + "000020.pt")
