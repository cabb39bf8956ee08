"""Inputs on which the arithmetic of the conv kernels is EXACT, with the proof obligations that make a bitwise
comparison against fp64 meaningful (tests/test_exact_inputs_host.py proves them on the CPU, tests/test_exact_gpu.py
compares the kernels with `torch.equal`).

Three families:

* Integer sets.  Effective activations in {0, +-1, +-2}, weights in {0, +-1/2, +-1} (sparse rows whose non-zeros walk over
  all of K from row to row), BN prologue coefficients with power-of-two scales and dyadic shifts, BN-backward combine
  coefficients likewise, small-integer upstream gradients; activation ReLU or none (Swish is not exact).  Every quantity
  a kernel forms is then a multiple of a power of two u (its grid), and a sum of such terms is exact in fp32 IN ANY
  ORDER as long as sum |terms| / u < 2^24: every partial sum is a multiple of u below 2^24 u, hence representable.  Every
  generator returns, next to the fp64 reference of each output kind, sum |terms| and u, and `assert_exact` checks the
  condition per output element -- it is checked for every case, not assumed.

* Split-term probes.  v = 1 + 2^-10 + 2^-20 has three non-zero bf16 terms (hi = 1, mid = 2^-10, lo = 2^-20); against an
  operand in {0, +-1} (pure hi) with at most 8 non-zero products per contraction every partial sum is a multiple of
  2^-20 below 2^4 (the same any-order condition), and the result needs every product the kernels keep: the probe on the
  activation side needs hi.hi, hi.mid, hi.lo (weight term first), the probe on the weight side lo.hi and mid.hi, and both
  operands 1 + 2^-10 need mid.mid (product 1 + 2^-9 + 2^-20).  The products the kernels drop by design (mid.lo, lo.mid,
  lo.lo) are zero on these inputs.  Signs are constant within a contraction, so the signed count of non-zero products of
  an output is 0 only where no product is non-zero at all.

* Hot integer sets, for the mixed-storage mode (bf16 storage of the wide tensors): the integer sets with a large power of two
  on a few voxels, so that a bf16 store of an output rounds; see "mixed storage" below.
"""
import math
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

LIMIT = float(2 ** 24)
F64 = torch.float64


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def pick(shape, values, probs, seed):
    """Independent draws from `values` with probabilities `probs`, fp64."""
    n = int(np.prod(shape)) if len(shape) else 1
    idx = torch.multinomial(torch.tensor(probs, dtype=F64), n, replacement=True, generator=_gen(seed))
    return torch.tensor(values, dtype=F64)[idx].view(*shape)


def ints(shape, seed):
    """Activations / gradients: {0, +-1, +-2}, 40 % zeros."""
    return pick(shape, (0., 1., -1., 2., -2.), (0.4, 0.2, 0.2, 0.1, 0.1), seed)


def halves(shape, seed, density=0.25):
    """Dense weights: {0, +-1/2, +-1}."""
    d = density / 4
    return pick(shape, (0., 0.5, -0.5, 1., -1.), (1 - density, d, d, d, d), seed)


def unit_of(*ts):
    """The grid of the tensors: the largest power of two that divides every element (1.0 when all are zero)."""
    e_min = None
    for t in ts:
        v = t.detach().double().reshape(-1).numpy()
        v = v[v != 0]
        if v.size == 0:
            continue
        m, e = np.frexp(v)                                              # v = m 2^e, 0.5 <= |m| < 1
        mi = np.abs(np.ldexp(m, 53)).astype(np.int64)                   # the 53-bit significand as an integer
        tz = np.round(np.log2((mi & -mi).astype(np.float64))).astype(np.int64)      # its trailing zeros
        k = int((e.astype(np.int64) - 53 + tz).min())
        e_min = k if e_min is None else min(e_min, k)
    return 1.0 if e_min is None else 2.0 ** e_min


def assert_exact(mags, what=""):
    """mags: {output kind: (sum |terms| per output element, grid u)}.  The any-order exactness condition; a violation is a
    bug in the case list."""
    for name, (mag, u) in mags.items():
        worst = float(mag.max()) / u if mag.numel() else 0.0
        assert worst < LIMIT, "%s %s: sum |terms| / u = %.4g >= 2^24 (u = %g): this case is not exact in fp32" % (
            what, name, worst, u)


def sparse_rows(M, K, nnz, seed):
    """[M, K] weights in {0, +-1/2, +-1}: `nnz` non-zeros per row (at least ceil(K / M), so that the rows together hit every
    column), their positions walking over K from row to row: row r holds the images of r nnz, r nnz + 1, ... under
    k -> k q mod K with q coprime to K (a bijection of the columns that spreads a row's non-zeros over the K chunks)."""
    nnz = min(K, max(nnz, -(-K // M)))
    q = max(1, int(K * 0.38))
    while math.gcd(q, K) != 1:
        q += 1
    pos = ((torch.arange(M).view(M, 1) * nnz + torch.arange(nnz).view(1, nnz)) * q) % K
    vals = pick((M, nnz), (0.5, -0.5, 1., -1.), (0.25, 0.25, 0.25, 0.25), seed)
    w = torch.zeros(M, K, dtype=F64)
    w.scatter_(1, pos, vals)
    assert int((w != 0).sum(1).min()) == nnz                            # (no position twice in a row)
    assert bool((w != 0).any(0).all()), "a column no row hits"
    return w


def prologue(N, C, seed):
    """BN prologue coefficients [N, C, 2]: power-of-two scales (both signs), dyadic shifts."""
    sc = pick((N, C), (1., -1., 2., 0.5), (0.4, 0.2, 0.2, 0.2), seed)
    sh = pick((N, C), (0., 0.5, -0.5, 1., -1.), (0.2, 0.2, 0.2, 0.2, 0.2), seed + 1)
    return torch.stack([sc, sh], -1)


def raw_for(target, pre):
    """The raw tensor x with pre[..., 0] * x + pre[..., 1] == target exactly (scales are powers of two)."""
    return (target - pre[..., 1, None, None, None]) / pre[..., 0, None, None, None]


def combine(N, C, seed):
    """BN-backward combine coefficients cb [N, C, 3]: dY = cb0 g + cb1 a + cb2."""
    c0 = pick((N, C), (1., -1., 2., 0.5), (0.4, 0.2, 0.2, 0.2), seed)
    c1 = pick((N, C), (0., 0.5, -0.5), (0.4, 0.3, 0.3), seed + 1)
    c2 = pick((N, C), (0., 0.5, -0.5), (0.4, 0.3, 0.3), seed + 2)
    return torch.stack([c0, c1, c2], -1)


def _bc(c, k):
    return c[..., k, None, None, None]


def affine(pre, x):
    return _bc(pre, 0) * x + _bc(pre, 1)


def dy_of(cb, g, a):
    return _bc(cb, 0) * g + _bc(cb, 1) * a + _bc(cb, 2)


def dy_mag(cb, g, a):
    return _bc(cb, 0).abs() * g.abs() + _bc(cb, 1).abs() * a.abs() + _bc(cb, 2).abs()


def _u_dy(c, dY):
    """Grid of the terms of dY = cb0 g + cb1 a + cb2."""
    u = min(unit_of(c.cb[..., 0]) * unit_of(c.g), unit_of(c.cb[..., 1]) * unit_of(c.a), unit_of(c.cb[..., 2]))
    assert unit_of(dY) >= u
    return u


def out_hw(h, s):
    return (h - 1) // 2 + 1 if s == 2 else h


def spread2(add2, H, W):
    """A stride-2 (compact) addend on the dense plane."""
    N, C, T = add2.shape[:3]
    full = torch.zeros(N, C, T, H, W, dtype=add2.dtype)
    full[:, :, :, ::2, ::2] = add2
    return full


def rowsum(t, order=0):
    """Sum over the voxels of every (n, c) row; order 1 adds them back to front."""
    t = t.flatten(2)
    return t.flip(2).sum(2) if order else t.sum(2)


# ----------------------------------------------------------------------------------------------------- pointwise
# the large-P rows (P = 24 964 and 50 176) that the whole-tensor norms of tests/test_ops_gpu.py cannot resolve: a voxel more
# or less moves a row's sum of squares by 1 / P.  (N, Cin, Cout, T, H, W, stride, act)
PW_LARGE_P = [
    (2, 24, 54, 4, 79, 79, 1, 1),       # streaming forward kernel, fp32-MFMA / fused backward; last 32-voxel tile holds 4
    (2, 54, 24, 4, 79, 79, 1, 1),
    (1, 24, 54, 16, 56, 56, 1, 1),      # P = 50 176
    (1, 96, 96, 16, 56, 56, 1, 1),      # whole-K persistent forward (pw8), data gradient pw7, 1568 items per sample
    (1, 160, 112, 4, 79, 79, 1, 1),     # whole-K forward pw6 (K > 128), pw7 with M = 160
]
FUSED_LARGE_P = [(2, 24, 54, 16, 56, 56, 1)]      # 1568 chunks on 512 workgroups


def pw_case(case, seed=0):
    """Integer inputs of every pointwise entry point at one shape.  act 2 (Swish) in a shared case list becomes ReLU."""
    N, Ci, Co, T, H, W, s, act = case
    act = 1 if act else 0
    Ho, Wo = out_hw(H, s), out_hw(W, s)
    c = SimpleNamespace(shape=(N, Ci, Co, T, H, W), s=s, act=act)
    c.w = sparse_rows(Co, Ci, 4, seed + 2)
    if act:
        c.pre = prologue(N, Ci, seed + 3)
        c.x = raw_for(ints((N, Ci, T, H, W), seed + 1), c.pre)
    else:
        c.pre = None
        c.x = ints((N, Ci, T, H, W), seed + 1)
    c.g = ints((N, Co, T, Ho, Wo), seed + 5)
    c.a = ints((N, Co, T, Ho, Wo), seed + 6)
    c.cb = combine(N, Co, seed + 7)
    if s == 1:
        c.addend = ints((N, Ci, T, H, W), seed + 10)
        c.add2 = ints((N, Ci, T, out_hw(H, 2), out_hw(W, 2)), seed + 11)
        c.res_out = torch.relu(ints((N, Ci, T, H, W), seed + 12))
        c.res_raw = ints((N, Ci, T, H, W), seed + 13)
    return c


def _pw_conv(xin, w, s, order):
    if order == 0:
        return F.conv3d(xin, w[:, :, None, None, None], stride=(1, s, s))
    perm = torch.arange(w.shape[1] - 1, -1, -1)                         # K back to front, as a batched matrix product
    return torch.einsum("ok,nkthw->nothw", w[:, perm], xin[:, :, :, ::s, ::s][:, perm])


def _pw_dgrad(dY, w, order):
    if order == 0:
        return F.conv_transpose3d(dY, w[:, :, None, None, None])
    perm = torch.arange(w.shape[0] - 1, -1, -1)
    return torch.einsum("oi,nothw->nithw", w[perm], dY[:, perm])


def _pw_wgrad(dY, xin, s, order):
    xs = xin[:, :, :, ::s, ::s]
    if order == 0:
        return torch.einsum("nothw,nithw->oi", dY, xs)
    return torch.einsum("nop,nip->oi", dY.flatten(2).flip(2).flip(0), xs.flatten(2).flip(2).flip(0))


def pw_ref(c, dt=F64, order=0):
    """Every output kind of the pointwise entry points on the case's inputs, evaluated in `dt`; order 1 is a second
    summation order (K back to front, voxels and samples back to front)."""
    t = lambda v: None if v is None else v.to(dt)
    x, w, g, a, cb, pre = t(c.x), t(c.w), t(c.g), t(c.a), t(c.cb), t(c.pre)
    s = c.s
    r = {}
    sx = affine(pre, x) if c.act else x
    xin = torch.relu(sx) if c.act else x
    r["y"] = _pw_conv(xin, w, s, order)
    r["sy"], r["sy2"] = rowsum(r["y"], order), rowsum(r["y"] * r["y"], order)
    dY = dy_of(cb, g, a)
    r["dw"] = _pw_wgrad(dY, xin, s, order)
    din = _pw_dgrad(dY, w, order)
    r["din"] = din                                                      # at output resolution (what a strided conv's backward-data computes)
    if s == 1:
        H, W = c.shape[4], c.shape[5]
        m = (sx > 0).to(dt) if c.act else None
        full = spread2(t(c.add2), H, W)
        r["dx_add"] = (din + t(c.addend)) * m if c.act else din + t(c.addend)
        if c.act:
            r["dx_sg"], r["dx_sgx"] = rowsum(r["dx_add"], order), rowsum(r["dx_add"] * x, order)
        r["dx_add2"] = din + full
        rm = (t(c.res_out) > 0).to(dt)
        for name, base in (("res0", din), ("res1", din + t(c.addend)), ("res2", din + full)):
            o = base * rm
            r[name], r[name + "_sg"], r[name + "_sgx"] = o, rowsum(o, order), rowsum(o * t(c.res_raw), order)
    return r


def pw_mags(c, r):
    """sum |terms| and the grid of every output kind of `pw_ref` (r: its fp64 result)."""
    sx = affine(c.pre, c.x) if c.act else c.x
    xin = torch.relu(sx) if c.act else c.x
    u_x, u_w, u_raw = unit_of(xin), unit_of(c.w), unit_of(c.x)
    dY, dYm = dy_of(c.cb, c.g, c.a), dy_mag(c.cb, c.g, c.a)
    u_dy = _u_dy(c, dY)
    u_y, u_din = u_x * u_w, u_w * u_dy
    m = {"prologue": (_bc(c.pre, 0).abs() * c.x.abs() + _bc(c.pre, 1).abs(), min(unit_of(c.pre), u_raw) ** 2)} if c.act else {}
    m["dY"] = (dYm, u_dy)
    m["y"] = (_pw_conv(xin.abs(), c.w.abs(), c.s, 0), u_y)
    m["sy"], m["sy2"] = (rowsum(r["y"].abs()), u_y), (rowsum(r["y"] ** 2), u_y * u_y)
    m["dw"] = (_pw_wgrad(dY.abs(), xin.abs(), c.s, 0), u_dy * u_x)
    dinm = _pw_dgrad(dY.abs(), c.w.abs(), 0)
    m["din"] = (dinm, u_din)
    if c.s == 1:
        u_o = min(u_din, unit_of(c.addend), unit_of(c.add2))
        m["dx_add"] = (dinm + c.addend.abs(), u_o)
        m["dx_add2"] = (dinm + spread2(c.add2, c.shape[4], c.shape[5]).abs(), u_o)
        if c.act:
            m["dx_sg"], m["dx_sgx"] = (rowsum(r["dx_add"].abs()), u_o), (rowsum((r["dx_add"] * c.x).abs()), u_o * u_raw)
        for name in ("res0", "res1", "res2"):
            m[name + "_sg"] = (rowsum(r[name].abs()), u_o)
            m[name + "_sgx"] = (rowsum((r[name] * c.res_raw).abs()), u_o * unit_of(c.res_raw))
    return m


def fused_case(case, seed=0):
    """Integer inputs of x3d_pw_bwd_fused in its three epilogue modes.  (N, Cin, Cout, T, H, W, act); act 2 becomes ReLU."""
    N, Ci, Co, T, H, W, act = case
    c = SimpleNamespace(shape=(N, Ci, Co, T, H, W), act=1 if act else 0)
    c.w = sparse_rows(Co, Ci, 4, seed + 2)
    c.pre = prologue(N, Ci, seed + 3)
    c.x = raw_for(ints((N, Ci, T, H, W), seed + 1), c.pre)              # modes 0 / 1 read it raw (mode 0 as the conv's input)
    c.xo = torch.relu(ints((N, Ci, T, H, W), seed + 14))                # mode 2: the producing block's output
    c.ex = ints((N, Ci, T, H, W), seed + 13)                            # ... and its raw conv3 output
    c.g = ints((N, Co, T, H, W), seed + 5)
    c.a = ints((N, Co, T, H, W), seed + 6)
    c.cb = combine(N, Co, seed + 7)
    c.addend = ints((N, Ci, T, H, W), seed + 10)
    c.add2 = ints((N, Ci, T, out_hw(H, 2), out_hw(W, 2)), seed + 11)
    return c


def fused_ref(c, dt=F64, order=0):
    t = lambda v: v.to(dt)
    x, w, g, a, cb, pre = t(c.x), t(c.w), t(c.g), t(c.a), t(c.cb), t(c.pre)
    H, W = c.shape[4], c.shape[5]
    dY = dy_of(cb, g, a)
    din = _pw_dgrad(dY, w, order)
    full = spread2(t(c.add2), H, W)
    r = {"m0_dx0": din, "m0_dx1": din + t(c.addend), "m0_dx2": din + full, "m0_dw": _pw_wgrad(dY, x, 1, order)}
    if c.act:
        sx = affine(pre, x)
        m = (sx > 0).to(dt)
        r["m1_dw"] = _pw_wgrad(dY, torch.relu(sx), 1, order)
        for name, base in (("m1_dx0", din), ("m1_dx2", din + full)):
            o = base * m
            r[name], r[name + "_sg"], r[name + "_sgx"] = o, rowsum(o, order), rowsum(o * x, order)
    xo_, ex = t(c.xo), t(c.ex)
    rm = (xo_ > 0).to(dt)
    r["m2_dw"] = _pw_wgrad(dY, xo_, 1, order)
    for name, base in (("m2_dx1", din + t(c.addend)), ("m2_dx2", din + full)):
        o = base * rm
        r[name], r[name + "_sg"], r[name + "_sgx"] = o, rowsum(o, order), rowsum(o * ex, order)
    return r


def fused_mags(c, r):
    dY, dYm = dy_of(c.cb, c.g, c.a), dy_mag(c.cb, c.g, c.a)
    u_dy = _u_dy(c, dY)
    u_w, u_raw = unit_of(c.w), unit_of(c.x)
    dinm = _pw_dgrad(dY.abs(), c.w.abs(), 0)
    u_o = min(u_w * u_dy, unit_of(c.addend), unit_of(c.add2))
    m = {"dY": (dYm, u_dy), "m0_dx": (dinm + c.addend.abs() + spread2(c.add2, c.shape[4], c.shape[5]).abs(), u_o),
         "m0_dw": (_pw_wgrad(dY.abs(), c.x.abs(), 1, 0), u_dy * u_raw),
         "m2_dw": (_pw_wgrad(dY.abs(), c.xo, 1, 0), u_dy * unit_of(c.xo))}
    if c.act:
        sx = affine(c.pre, c.x)
        m["prologue"] = (_bc(c.pre, 0).abs() * c.x.abs() + _bc(c.pre, 1).abs(), min(unit_of(c.pre), u_raw) ** 2)
        m["m1_dw"] = (_pw_wgrad(dY.abs(), torch.relu(sx), 1, 0), u_dy * unit_of(sx))
    for name, other in (("m1_dx0", c.x), ("m1_dx2", c.x), ("m2_dx1", c.ex), ("m2_dx2", c.ex)):
        if name in r:
            m[name + "_sg"] = (rowsum(r[name].abs()), u_o)
            m[name + "_sgx"] = (rowsum((r[name] * other).abs()), u_o * unit_of(other))
    return m


# ----------------------------------------------------------------------------------------------------- channelwise 3x3x3
DW_LARGE_P = [(1, 3, 16, 56, 56, 1)]              # a T = 16 plane of 56^2: P = 50 176


def dw_case(case, seed=0):
    N, C, T, H, W, s = case
    Ho, Wo = out_hw(H, s), out_hw(W, s)
    c = SimpleNamespace(shape=(N, C, T, H, W), s=s)
    c.w = sparse_rows(C, 27, 3, seed + 2).view(C, 1, 3, 3, 3)           # every one of the 27 taps is hit by some channel
    c.pre = prologue(N, C, seed + 3)
    c.x = raw_for(ints((N, C, T, H, W), seed + 1), c.pre)
    c.g = ints((N, C, T, Ho, Wo), seed + 5)
    c.a = ints((N, C, T, Ho, Wo), seed + 6)
    c.cb = combine(N, C, seed + 7)
    return c


def _taps(kt, kh, kw, order):
    taps = [(a, b, d) for a in range(kt) for b in range(kh) for d in range(kw)]
    return taps[::-1] if order else taps


def _dw_loop(hin, w, dY, s, pad, order):
    """Depthwise convolution, its data gradient and its weight gradient as explicit loops over the taps (order 1: the taps
    back to front).  w [C, 1, kt, kh, kw], stride (1, s, s), padding `pad` = (pt, ph, pw)."""
    N, C, T, H, W = hin.shape
    kt, kh, kw = w.shape[2:]
    pt, ph, pw = pad
    To, Ho, Wo = T + 2 * pt - kt + 1, (H + 2 * ph - kh) // s + 1, (W + 2 * pw - kw) // s + 1
    xp = F.pad(hin, (pw, pw, ph, ph, pt, pt))
    y = torch.zeros(N, C, To, Ho, Wo, dtype=hin.dtype)
    dxp = torch.zeros_like(xp)
    dw = torch.zeros_like(w)
    for (a, b, d) in _taps(kt, kh, kw, order):
        sl = (slice(None), slice(None), slice(a, a + To), slice(b, b + s * (Ho - 1) + 1, s), slice(d, d + s * (Wo - 1) + 1, s))
        wt = w[:, 0, a, b, d].view(1, C, 1, 1, 1)
        y += wt * xp[sl]
        if dY is not None:
            dxp[sl] += wt * dY
            prod = dY * xp[sl]
            dw[:, 0, a, b, d] = (prod.flatten(2).flip(2).flip(0) if order else prod.flatten(2)).sum(2).sum(0)
    dx = dxp[:, :, pt:pt + T, ph:ph + H, pw:pw + W]
    return y, dx, dw


def _dw_auto(hin, w, dY, stride, pad):
    hin = hin.detach().clone().requires_grad_(True)
    w = w.detach().clone().requires_grad_(True)
    y = F.conv3d(hin, w, stride=stride, padding=pad, groups=hin.shape[1])
    if dY is None:
        return y.detach(), None, None
    (y * dY).sum().backward()
    return y.detach(), hin.grad, w.grad


def dw_ref(c, dt=F64, order=0):
    t = lambda v: v.to(dt)
    x, w, g, a, cb, pre = t(c.x), t(c.w), t(c.g), t(c.a), t(c.cb), t(c.pre)
    sx = affine(pre, x)
    hin = torch.relu(sx)
    dY = dy_of(cb, g, a)
    if order == 0:
        y, dh, dw = _dw_auto(hin, w, dY, (1, c.s, c.s), 1)
    else:
        y, dh, dw = _dw_loop(hin, w, dY, c.s, (1, 1, 1), 1)
    out = dh * (sx > 0).to(dt)
    return {"y": y, "sy": rowsum(y, order), "sy2": rowsum(y * y, order), "dx": out, "dw": dw,
            "sg": rowsum(out, order), "sgx": rowsum(out * x, order)}


def dw_mags(c, r):
    sx = affine(c.pre, c.x)
    hin = torch.relu(sx)
    dY, dYm = dy_of(c.cb, c.g, c.a), dy_mag(c.cb, c.g, c.a)
    u_dy = _u_dy(c, dY)
    u_h, u_w, u_raw = unit_of(hin), unit_of(c.w), unit_of(c.x)
    ym, dxm, dwm = _dw_loop(hin, c.w.abs(), dY.abs(), c.s, (1, 1, 1), 0)
    return {"prologue": (_bc(c.pre, 0).abs() * c.x.abs() + _bc(c.pre, 1).abs(), min(unit_of(c.pre), u_raw) ** 2),
            "dY": (dYm, u_dy), "y": (ym, u_h * u_w), "sy": (rowsum(r["y"].abs()), u_h * u_w),
            "sy2": (rowsum(r["y"] ** 2), (u_h * u_w) ** 2), "dx": (dxm, u_w * u_dy), "dw": (dwm, u_dy * u_h),
            "sg": (rowsum(r["dx"].abs()), u_w * u_dy), "sgx": (rowsum((r["dx"] * c.x).abs()), u_w * u_dy * u_raw)}


# ----------------------------------------------------------------------------------------------------- stem
def stem_case(shape, seed=0):
    N, Ci, T, H, W = shape
    Co = 24
    c = SimpleNamespace(shape=shape)
    c.x = ints(shape, seed + 1)
    c.ws = sparse_rows(Co, Ci * 9, 4, seed + 2).view(Co, Ci, 1, 3, 3)   # all 9 taps of all 3 input channels
    c.wt = sparse_rows(Co, 5, 2, seed + 3).view(Co, 1, 5, 1, 1)         # all 5 temporal taps
    Ho, Wo = out_hw(H, 2), out_hw(W, 2)
    c.g = ints((N, Co, T, Ho, Wo), seed + 5)
    c.a = ints((N, Co, T, Ho, Wo), seed + 6)
    c.cb = combine(N, Co, seed + 7)
    return c


def _stem_loop(x, ws, dys, order):
    """stem133 (1 x 3 x 3, stride 2, padding 1) and its weight gradient as loops over taps and input channels."""
    N, Ci, T, H, W = x.shape
    Co = ws.shape[0]
    Ho, Wo = out_hw(H, 2), out_hw(W, 2)
    xp = F.pad(x, (1, 1, 1, 1))
    ys = torch.zeros(N, Co, T, Ho, Wo, dtype=x.dtype)
    dws = torch.zeros_like(ws)
    terms = [(i, b, d) for i in range(Ci) for b in range(3) for d in range(3)]
    for (i, b, d) in (terms[::-1] if order else terms):
        xs = xp[:, i:i + 1, :, b:b + 2 * (Ho - 1) + 1:2, d:d + 2 * (Wo - 1) + 1:2]
        ys += ws[:, i, 0, b, d].view(1, Co, 1, 1, 1) * xs
        if dys is not None:
            prod = dys * xs
            dws[:, i, 0, b, d] = (prod.flatten(2).flip(2).flip(0) if order else prod.flatten(2)).sum(2).sum(0)
    return ys, dws


def stem_ref(c, dt=F64, order=0):
    t = lambda v: v.to(dt)
    x, ws, wt, g, a, cb = t(c.x), t(c.ws), t(c.wt), t(c.g), t(c.a), t(c.cb)
    dY = dy_of(cb, g, a)
    if order == 0:
        ys = F.conv3d(x, ws, stride=(1, 2, 2), padding=(0, 1, 1))
        yt, dys, dwt = _dw_auto(ys, wt, dY, 1, (2, 0, 0))
        wl = ws.detach().clone().requires_grad_(True)
        (F.conv3d(x, wl, stride=(1, 2, 2), padding=(0, 1, 1)) * dys).sum().backward()
        dws = wl.grad
    else:
        ys, _ = _stem_loop(x, ws, None, 1)
        yt, dys, dwt = _dw_loop(ys, wt, dY, 1, (2, 0, 0), 1)
        _, dws = _stem_loop(x, ws, dys, 1)
    return {"ys": ys, "yt": yt, "sy": rowsum(yt, order), "sy2": rowsum(yt * yt, order), "dys": dys, "dwt": dwt, "dws": dws}


def stem_mags(c, r):
    dY, dYm = dy_of(c.cb, c.g, c.a), dy_mag(c.cb, c.g, c.a)
    u_dy = _u_dy(c, dY)
    u_ys = unit_of(c.x) * unit_of(c.ws)
    u_yt, u_dys = u_ys * unit_of(c.wt), u_dy * unit_of(c.wt)
    ysm, _ = _stem_loop(c.x.abs(), c.ws.abs(), None, 0)
    ytm, dysm, dwtm = _dw_loop(ysm, c.wt.abs(), dY.abs(), 1, (2, 0, 0), 0)
    _, dwsm = _stem_loop(c.x.abs(), c.ws.abs(), dysm, 0)
    return {"dY": (dYm, u_dy), "ys": (ysm, u_ys), "yt": (ytm, u_yt), "sy": (rowsum(r["yt"].abs()), u_yt),
            "sy2": (rowsum(r["yt"] ** 2), u_yt * u_yt), "dys": (dysm, u_dys), "dwt": (dwtm, u_dy * u_ys),
            "dws": (dwsm, u_dys * unit_of(c.x))}


# ----------------------------------------------------------------------------------------------------- head
HEAD_R, HEAD_K, HEAD_C = (1, 7, 8, 9, 65, 70), (48, 432, 630, 640), (1, 10, 157, 400)
HEAD_J = 2048


def head_case(R, K, J, C, seed=0):
    c = SimpleNamespace(shape=(R, K, J, C))
    c.pooled = torch.relu(ints((R, K), seed + 1))
    c.w1 = halves((J, K), seed + 2)
    c.w2 = halves((C, J), seed + 3)
    c.b2 = pick((C,), (0., 0.5, -0.5, 1.), (0.25, 0.25, 0.25, 0.25), seed + 4)
    c.dlg = ints((R, C), seed + 5)
    return c


def _mm(a, b, order):
    """a [m, k] @ b [k, n]; order 1 contracts k back to front."""
    if order == 0:
        return a @ b
    perm = torch.arange(a.shape[1] - 1, -1, -1)
    return a[:, perm] @ b[perm]


def head_ref(c, dt=F64, order=0):
    t = lambda v: v.to(dt)
    pooled, w1, w2, b2, dlg = t(c.pooled), t(c.w1), t(c.w2), t(c.b2), t(c.dlg)
    h = torch.relu(_mm(pooled, w1.t(), order))
    logits = _mm(h, w2.t(), order) + b2
    dh = _mm(dlg, w2, order) * (h > 0).to(dt)
    return {"hidden": h, "logits": logits, "dw1": _mm(dh.t(), pooled, order), "dw2": _mm(dlg.t(), h, order),
            "db2": dlg.flip(0).sum(0) if order else dlg.sum(0), "dpooled": _mm(dh, w1, order)}


def head_mags(c, r):
    u_p, u_w1, u_w2, u_g = unit_of(c.pooled), unit_of(c.w1), unit_of(c.w2), unit_of(c.dlg)
    u_h = u_p * u_w1
    hm = c.pooled @ c.w1.abs().t()
    dhm = c.dlg.abs() @ c.w2.abs()
    dh = (c.dlg @ c.w2) * (r["hidden"] > 0).double()
    return {"hidden": (hm, u_h), "logits": (r["hidden"] @ c.w2.abs().t() + c.b2.abs(), min(u_h * u_w2, unit_of(c.b2))),
            "dh": (dhm, u_g * u_w2), "dw1": (dh.abs().t() @ c.pooled, u_g * u_w2 * u_p),
            "dw2": (c.dlg.abs().t() @ r["hidden"], u_g * u_h), "db2": (c.dlg.abs().sum(0), u_g),
            "dpooled": (dh.abs() @ c.w1.abs(), u_g * u_w2 * u_w1)}


# ----------------------------------------------------------------------------------------------------- split-term probes
PROBE_V = 1.0 + 2.0 ** -10 + 2.0 ** -20          # hi 1, mid 2^-10, lo 2^-20
PROBE_B = 1.0 + 2.0 ** -10                       # hi 1, mid 2^-10: the square needs mid.mid
PROBE_KINDS = ("act", "weight", "both")
KEPT = (("hi", "hi"), ("hi", "mid"), ("mid", "hi"), ("mid", "mid"), ("hi", "lo"), ("lo", "hi"))     # (A term, B term)
# the kept products a probe kind needs (all others are identically zero on its inputs); together: all six
NEEDS = {"act": (("hi", "hi"), ("hi", "mid"), ("hi", "lo")), "weight": (("hi", "hi"), ("mid", "hi"), ("lo", "hi")),
         "both": (("hi", "hi"), ("hi", "mid"), ("mid", "hi"), ("mid", "mid"))}
CARRIES_LO = ("act", "weight")                   # the two-term form (hi + mid) cannot reproduce these


def probe_operands(M, K, cols, kind, seed=0):
    """A [M, K] (the sparse side: 8 non-zeros per row, one sign per row) and B [K, cols] (half of the entries non-zero, one
    sign per column), so that an output A B has at most 8 non-zero products, all of one sign.  kind: which side carries the
    probe value -- 'act' B, 'weight' A, 'both' (1 + 2^-10 on either side)."""
    va, vb = {"act": (1.0, PROBE_V), "weight": (PROBE_V, 1.0), "both": (PROBE_B, PROBE_B)}[kind]
    nnz = min(8, K)
    q = max(1, int(K * 0.38))
    while math.gcd(q, K) != 1:
        q += 1
    pos = ((torch.arange(M).view(M, 1) * nnz + torch.arange(nnz).view(1, nnz)) * q) % K
    sa = pick((M, 1), (1., -1.), (0.5, 0.5), seed + 1)
    A = torch.zeros(M, K, dtype=F64)
    A.scatter_(1, pos, (sa * va).expand(M, nnz).contiguous())
    sb = pick((1, cols), (1., -1.), (0.5, 0.5), seed + 2)
    B = pick((K, cols), (0., 1.), (0.5, 0.5), seed + 3) * sb * vb
    return A, B


def split3(t):
    """The three bf16 terms of fp32 values (round to nearest even, as the kernels split), as fp64."""
    t = t.float()
    hi = t.bfloat16().float()
    mid = (t - hi).bfloat16().float()
    lo = (t - hi - mid).bfloat16().float()
    assert torch.equal(hi + mid + lo, t)
    return {"hi": hi.double(), "mid": mid.double(), "lo": lo.double()}


def probe_count(A, B):
    """Non-zero products per output (the signed count m is this times the common sign)."""
    return (A != 0).double() @ (B != 0).double()


def tiles_resolved(changed, rows=16, cols=32):
    """Smallest fraction of changed outputs over the rows x cols tiles (tail tiles included) of a [..., M, P] mask."""
    M, P = changed.shape[-2:]
    worst = 1.0
    ch = changed.reshape(-1, M, P).double()
    for r0 in range(0, M, rows):
        for c0 in range(0, P, cols):
            worst = min(worst, float(ch[:, r0:r0 + rows, c0:c0 + cols].mean(dim=(1, 2)).min()))
    return worst


# Probe shapes, shared by the host proof and the GPU tests.  (N, Cin, Cout, T, H, W) of the CONVOLUTION; each list names the
# kernel its shapes must land on.  Tail tiles (P = 100, 72, 180: P % 32 != 0), M not a multiple of 16, K not a multiple of 32
# (and of 4), K = 432.
PROBE_FWD = {
    "pw8_kernel": [(2, 96, 216, 4, 5, 5), (2, 70, 98, 2, 6, 6), (1, 100, 130, 3, 6, 6)],
    "pw6_kernel": [(2, 432, 192, 4, 5, 5), (2, 200, 120, 3, 6, 10), (2, 96, 216, 4, 5, 5)],      # (the last one: option no_pw8)
    "pw_fwd_stream_kernel": [(2, 24, 54, 4, 5, 5), (1, 40, 60, 3, 6, 6), (1, 64, 80, 1, 10, 10), (2, 48, 108, 2, 6, 6)],
}
# data gradient: the GEMM's K is Cout, its M rows are Cin
PROBE_DGRAD = [(2, 216, 96, 4, 5, 5), (2, 192, 432, 4, 5, 5), (1, 130, 200, 3, 6, 10)]           # pw7_kernel / pw7r_kernel
PROBE_FUSED = [(2, 24, 54, 4, 5, 5), (2, 54, 24, 4, 5, 5), (2, 48, 108, 2, 6, 6), (1, 40, 60, 3, 6, 6)]
PROBE_WGRAD = [(2, 24, 54, 4, 5, 5), (2, 96, 216, 4, 5, 5), (2, 432, 192, 4, 5, 5), (1, 40, 60, 3, 6, 6)]


def probe_fwd(shape, kind, seed=0):
    """(w [Co, Ci], x [N, Ci, T, H, W], y [N, Co, T, H, W]) of a forward probe."""
    N, Ci, Co, T, H, W = shape
    P = T * H * W
    A, B = probe_operands(Co, Ci, N * P, kind, seed)
    x = B.view(Ci, N, P).transpose(0, 1).contiguous()
    return A, x.view(N, Ci, T, H, W), torch.einsum("ok,nkp->nop", A, x).view(N, Co, T, H, W)


def probe_dgrad(shape, kind, seed=0):
    """(w [Co, Ci], dY [N, Co, T, H, W], dX [N, Ci, T, H, W]): the weight is the sparse side, 8 non-zeros per input channel."""
    N, Ci, Co, T, H, W = shape
    P = T * H * W
    A, B = probe_operands(Ci, Co, N * P, kind, seed)
    dY = B.view(Co, N, P).transpose(0, 1).contiguous()
    return A.t().contiguous(), dY.view(N, Co, T, H, W), torch.einsum("ik,nkp->nip", A, dY).view(N, Ci, T, H, W)


def probe_wgrad(shape, kind, seed=0):
    """(dY [N, Co, T, H, W], x [N, Ci, T, H, W], dW [Co, Ci]): the contraction runs over the N P voxels; dY is the sparse
    side (8 non-zero voxels per output channel); 'weight' puts the probe value on dY, 'act' on x."""
    N, Ci, Co, T, H, W = shape
    P = T * H * W
    A, B = probe_operands(Co, N * P, Ci, kind, seed)                    # A [Co, N P], B [N P, Ci]
    dY = A.view(Co, N, P).transpose(0, 1).contiguous().view(N, Co, T, H, W)
    x = B.t().contiguous().view(Ci, N, P).transpose(0, 1).contiguous().view(N, Ci, T, H, W)
    return dY, x, A @ B


# ----------------------------------------------------------------------------------------------------- mixed storage
# bf16 storage of the wide tensors (include/x3dhip.h X3D_MX_*).  The integer sets above give outputs of at most 8
# significant bits: a bf16 store of them never rounds.  The HOT variant puts a large power of two on a few voxels of a
# sample in some channels (of x: what a forward output is large from; of g: what a data gradient is large from); an output
# there is a large term plus a small one (128.5, 257.5, 130.25) of 9 to 11 significant bits, on the same power-of-two grid,
# so the store rounds: ties where the small part is half an ulp, non-ties where the grid is finer than that (magnitude
# 256 against a grid of 1/2; the gradients' grid of 1/4).  The reference of a bf16 output is the fp64 result, which is an
# fp32 number, cast by torch's CPU round-to-nearest-even; the statistics that describe it are the fp64 sums over THAT
# tensor.  tests/test_exact_inputs_host.py proves per case that the rounding really is exercised.
HOT = (64., -64., 128., -128., 256., -256.)
HOT_P = (0.05, 0.05, 0.1, 0.1, 0.35, 0.35)
HOT_ROW_P = (0.03, 0.02, 0.45, 0.2, 0.18, 0.12)        # (channelwise: what follows a ReLU is better positive)


def bf16_ok(t):
    """Every element is a bf16 number."""
    return torch.equal(t.float().bfloat16().double(), t.double())


def stored(v):
    """v as a kernel stores it in a bf16 tensor: round to nearest even (torch's CPU cast) of the fp32 value, in v's dtype."""
    f = v.float()
    assert torch.equal(f.double(), v.double()), "not an fp32 number (bug in the case)"
    return f.bfloat16().to(v.dtype)


def _bits(v):
    f = v.float()
    assert torch.equal(f.double(), v.double())
    return f.contiguous().view(torch.int32)


def stored_by_truncation(v):
    """Control: the low 16 bits dropped."""
    return (_bits(v) & -65536).view(torch.float32).to(v.dtype)


def stored_half_away(v):
    """Control: 0x8000 added to the (sign-magnitude) bits, then truncated -- round half away from zero."""
    return ((_bits(v) + 0x8000) & -65536).view(torch.float32).to(v.dtype)


def rounding_census(v):
    """How the bf16 store of v (fp64 holding fp32 numbers) rounds: counts of elements that are not bf16 numbers, of ties
    rounded up / down in magnitude (to the even neighbour) and of non-ties rounded up / down in magnitude."""
    low = _bits(v) & 0xFFFF
    up = stored(v).abs() > v.abs()
    tie, ne = low == 0x8000, low != 0
    cnt = lambda m: int(m.sum())
    return {"inexact": cnt(ne), "tie_up": cnt(tie & up), "tie_down": cnt(tie & ~up), "up": cnt(ne & ~tie & up),
            "down": cnt(ne & ~tie & ~up)}


def _fit_raw(t, pre):
    """With a prologue the RAW tensor (raw_for) must stay a bf16 tensor: a hot value whose raw image needs a ninth bit
    (128 + 1/2) is halved until it fits."""
    for _ in range(3):
        raw = raw_for(t, pre)
        t = torch.where(raw.float().bfloat16().double() != raw, t / 2, t)
    assert bf16_ok(raw_for(t, pre))
    return t


def heat(target, seed, pre=None):
    """The hot variant of an activation / gradient tensor [N, C, T, H, W] of effective values: on P / 2 voxels of a sample (at
    most 48) every channel takes, with probability 1 / 8 (at least two channels per voxel on average), a value of HOT -- other
    channels at each voxel, so that the hot terms reach every output row but seldom two of them the same output."""
    N, C = target.shape[:2]
    t = target.clone().flatten(2)
    P = t.shape[2]
    nv = min(max(P // 2, 1), 48)
    q = max(1.0 / 8, 2.0 / C)
    g = _gen(seed)
    for n in range(N):
        vox = torch.randperm(P, generator=g)[:nv]
        vals = pick((C, nv), (0.,) + HOT, (1 - q,) + tuple(q * p for p in HOT_P), seed + 1 + n)
        t[n][:, vox] = torch.where(vals != 0, vals, t[n][:, vox])
    t = t.view_as(target)
    return t if pre is None else _fit_raw(t, pre)


def heat_rows(target, seed, pre=None, frac=4, most=24):
    """heat() for the channelwise convs, where every (n, c) row is a convolution of its own: each row gets its own hot voxels,
    1 / frac of the row's at most, `most` at most."""
    N, C = target.shape[:2]
    t = target.clone().flatten(2)
    P = t.shape[2]
    nv = min(max(int(P / frac), 1), most)
    g = _gen(seed)
    vox = torch.stack([torch.randperm(P, generator=g)[:nv] for _ in range(N * C)]).view(N, C, nv)
    t.scatter_(2, vox, pick((N, C, nv), HOT, HOT_ROW_P, seed + 1))
    t = t.view_as(target)
    return t if pre is None else _fit_raw(t, pre)


def _st(r, name, second=None, order=0):
    """Adds to r the stored form of the bf16 output r[name] and the two statistics of the stored tensor: {sum y, sum y^2}, or
    {sum dx, sum dx * second} for a gradient."""
    st = stored(r[name])
    r[name + "_st"] = st
    r[name + "_st_s0"] = rowsum(st, order)
    r[name + "_st_s1"] = rowsum(st * (st if second is None else second), order)


def _st_mags(m, r, name, second=None):
    st = r[name + "_st"]
    u = unit_of(st)
    m[name + "_st_s0"] = (rowsum(st.abs()), u)
    m[name + "_st_s1"] = (rowsum((st * (st if second is None else second)).abs()), u * (u if second is None else unit_of(second)))


# pointwise rows of the case tables of tests/test_mixed_storage_gpu.py (PW_FWD, PW_BWD): the smallest row on each mixed-storage
# kernel, and every row where the mixed mode runs ANOTHER kernel than fp32 (marked *).  (N, Cin, Cout, T, H, W, act)
PW_MX = [
    (2, 24, 54, 4, 16, 16, 1),      # forward: streaming split-bf16 kernel, wide output; backward: the fused kernel's shapes
    (2, 54, 24, 4, 16, 16, 1),      # fp32-MFMA streaming kernel (pw3), wide input
    (2, 48, 216, 4, 6, 6, 0),       # K < 64: pw3 with a wide output; data gradient M = 48: pw3 with bf16 g, a
    (1, 24, 54, 2, 9, 7, 1),        # * P % 4 != 0: pw3 scalar form, bf16 element stores
    (1, 54, 24, 2, 9, 7, 1),        # * P % 4 != 0: bf16 element loads
    (2, 96, 216, 4, 12, 12, 0),     # * whole-K item kernel pw6 (fp32: pw8); conv1 data gradient: item kernel pw7 (fp32, two terms: chunked)
    (2, 216, 96, 4, 12, 12, 1),     # pw6, wide input; data gradient pw7, M = 216
    (2, 432, 192, 2, 6, 6, 1),      # K = 432: dynamic LDS > 64 KB
    (2, 192, 432, 2, 6, 6, 0),
    (2, 54, 54, 2, 8, 8, 1),        # both sides bf16
    (1, 96, 216, 2, 7, 7, 0),       # * stage 3 with P % 4 != 0: streaming kernel instead of the LDS-tiled ones
    (1, 216, 96, 2, 7, 7, 1),       # *
]
FUSED_MX = [(2, 24, 54, 4, 16, 16, 1), (2, 54, 24, 4, 16, 16, 1), (3, 48, 108, 2, 20, 20, 1), (2, 108, 48, 2, 14, 14, 1),
            (2, 24, 108, 4, 12, 12, 1)]                                 # the five tile shapes of x3d_pw_bwd_fused (FUSED)
PW_MX_GRID = [(3, 24, 54, 4, 20, 20, 1)]                                # persistent loops (option fb_grid): the streaming forward ...
FUSED_MX_GRID = [(3, 24, 54, 4, 20, 20, 1)]                             # ... and the fused backward
# DW rows: W % 4 != 0 and odd sizes (element loads / stores), the 16-channel block with a tail, float2 and float4 rows,
# stride 2, three row tiles.  The base-shape planes add nothing about rounding or tails.
DW_MX = [(2, 6, 4, 14, 14, 1), (1, 5, 5, 13, 9, 1), (2, 4, 4, 16, 16, 2), (1, 3, 3, 15, 11, 2), (1, 33, 2, 4, 4, 2), (1, 2, 3, 40, 56, 1)]


# the seeds at which every case below meets the "rounding is exercised" conditions of tests/test_exact_inputs_host.py (how many
# outputs round, and how, is a property of the draw; the conditions are asserted there, per case)
MX_SEED = 3
DW_MX_SEED = {(2, 6, 4, 14, 14, 1): 6}
DW_MX_SEED_DEFAULT = 7
DW_BN_SEED = {(1, 33, 2, 4, 4, 2): 3}                  # (of the BN side of x3d_dw333_fwd_stats)


def pw_mx_case(case, seed=MX_SEED):
    """pw_case with hot x (effective values; the raw tensor stays bf16) and hot g.  The other tensors a kernel may read as
    bf16 (a) are integers."""
    N, Ci, Co, T, H, W, act = case
    c = pw_case((N, Ci, Co, T, H, W, 1, act), seed)
    eff = affine(c.pre, c.x) if c.act else c.x
    hot = heat(eff, seed + 20, c.pre if c.act else None)
    c.x = raw_for(hot, c.pre) if c.act else hot
    c.g = heat(c.g, seed + 30)
    return c


def pw_mx_ref(c, dt=F64, order=0):
    """pw_ref plus, for the outputs a mixed-storage call writes as bf16 (y; dx of the ReLU-backward form without addend),
    the stored tensor and its statistics.  What is computed FROM bf16 tensors keeps pw_ref's entry."""
    r = pw_ref(c, dt, order)
    _st(r, "y", order=order)
    if c.act:
        x = c.x.to(dt)
        r["dx_act"] = r["din"] * (affine(c.pre.to(dt), x) > 0).to(dt)
        r["dx_act_s0"], r["dx_act_s1"] = rowsum(r["dx_act"], order), rowsum(r["dx_act"] * x, order)
        _st(r, "dx_act", second=x, order=order)
    return r


def pw_mx_mags(c, r):
    m = pw_mags(c, r)
    _st_mags(m, r, "y")
    if c.act:
        m["dx_act_s0"] = (rowsum(r["dx_act"].abs()), m["din"][1])
        m["dx_act_s1"] = (rowsum((r["dx_act"] * c.x).abs()), m["din"][1] * unit_of(c.x))
        _st_mags(m, r, "dx_act", c.x)
    return m


def fused_mx_case(case, seed=MX_SEED):
    c = fused_case(case, seed)
    c.x = raw_for(heat(affine(c.pre, c.x), seed + 20, c.pre), c.pre)
    c.g = heat(c.g, seed + 30)
    return c


def fused_mx_ref(c, dt=F64, order=0):
    r = fused_ref(c, dt, order)
    _st(r, "m1_dx0", second=c.x.to(dt), order=order)                   # X | Y: mode 1 without addend
    return r


def fused_mx_mags(c, r):
    m = fused_mags(c, r)
    _st_mags(m, r, "m1_dx0", c.x)
    return m


def dw_mx_case(case, seed=None, pre=None, cb=None):
    """dw_case with hot x and g and NINE taps per channel instead of three: an output next to a hot voxel then has small terms
    too, whose half decides the rounding."""
    seed = DW_MX_SEED.get(tuple(case), DW_MX_SEED_DEFAULT) if seed is None else seed
    c = dw_case(case, seed)
    c.w = sparse_rows(case[1], 27, 9, seed + 2).view(case[1], 1, 3, 3, 3)
    eff = affine(c.pre, c.x)
    eff = torch.where(eff == -1, -eff, eff)                            # more odd terms behind the ReLU (-2 stays)
    if pre is not None:
        c.pre = pre
    if cb is not None:
        c.cb = cb
    # a hot voxel of x reaches nine outputs at stride 1 but two or three at stride 2; sum y^2 of a row bounds how many it may hold
    c.x = raw_for(heat_rows(eff, seed + 20, c.pre, *((4, 32) if c.s == 1 else (1.5, 96))), c.pre)
    c.g = heat_rows(c.g, seed + 30, None, 4 if c.s == 1 else 2, 24)
    return c


def dw_mx_ref(c, dt=F64, order=0):
    r = dw_ref(c, dt, order)
    _st(r, "y", order=order)
    _st(r, "dx", second=c.x.to(dt), order=order)
    return r


def dw_mx_mags(c, r):
    m = dw_mags(c, r)
    _st_mags(m, r, "y")
    _st_mags(m, r, "dx", c.x)
    return m


# the BN finalizes folded into the channelwise kernels (x3d_dw333_fwd_stats, x3d_dw333_bwd_stats) are fp64 arithmetic on the
# statistics partials; on dyadic statistics every step of it is exact (quotients by a count whose numerator is a multiple of
# it, the square root of 1 or 1/4), so the coefficients they derive are the case's pre / cb and everything else follows.
BN_EPS, BN_MOMENTUM = 2.0 ** -6, 0.25


def _spread(total, N, tiles=3):
    """[N, C, tiles, ...] partials (dyadic fractions 1/2, 1/4, 1/4 per sample) that sum to total [C, ...] over samples and tiles."""
    f = torch.tensor([0.5, 0.25, 0.25], dtype=F64)[:tiles].view(1, 1, tiles, 1)
    return (total[None, :, None] / N * f).expand(N, -1, -1, -1).contiguous()


def dw_bn_fwd(N, C, S, seed=0):
    """Statistics partials of a producer conv, BN parameters and running statistics of x3d_dw333_fwd_stats with S splits, and
    what its finalize makes of them: coef [N, C, 2] (the prologue the conv then applies), save [2, S, C], the updated running
    statistics.  The element count of a split is 9 or 2: cnt - 1 is a power of two, so the unbiased variance is exact."""
    ns = N // S
    assert N % S == 0 and ns in (1, 2)
    b = SimpleNamespace(S=S, count=9 if ns == 1 else 1, eps=BN_EPS, momentum=BN_MOMENTUM)
    cnt = float(b.count * ns)
    b.gamma = pick((C,), (1., -1., 0.5), (0.4, 0.3, 0.3), seed + 40)
    b.beta = pick((C,), (0., 0.5, -0.5, 1.), (0.25, 0.25, 0.25, 0.25), seed + 41)
    mean = pick((S, C), (0., 0.5, -0.5), (0.4, 0.3, 0.3), seed + 42)
    invstd = pick((S, C), (1., 2.), (0.5, 0.5), seed + 43)
    var = 1 / (invstd * invstd) - b.eps
    b.rm = pick((S, C), (0., 0.5, -1.), (0.4, 0.3, 0.3), seed + 44)
    b.rv = pick((S, C), (1., 0.5, 2.), (0.4, 0.3, 0.3), seed + 45)
    tot = torch.stack([mean * cnt, (var + mean * mean) * cnt], -1)      # [S, C, 2]: the sums over a split
    b.sp = torch.cat([_spread(tot[j], ns) for j in range(S)], 0)        # samples j, j + S, ... of split j
    b.sp = b.sp.view(S, ns, C, 3, 2).transpose(0, 1).reshape(N, C, 3, 2).contiguous()
    sc = b.gamma * invstd
    coef = torch.stack([sc, b.beta - mean * sc], -1)                    # [S, C, 2]
    b.coef = coef.repeat(ns, 1, 1)                                      # sample n belongs to split n % S
    b.save = torch.stack([mean, invstd], 0)
    b.rm_new = (1 - b.momentum) * b.rm + b.momentum * mean
    b.rv_new = (1 - b.momentum) * b.rv + b.momentum * (var * cnt / (cnt - 1))
    return b


def dw_bn_bwd(N, C, seed=0):
    """Statistics partials {sum g, sum g a} of a BN backward, gamma and the saved mean / invstd of x3d_dw333_bwd_stats (one
    split), and what its finalize makes of them: cb [N, C, 3], dgamma, dbeta.  N count = 16."""
    b = SimpleNamespace(count=16 // N)
    M = float(b.count * N)
    b.gamma = pick((C,), (1., -1., 0.5), (0.4, 0.3, 0.3), seed + 50)
    mean = pick((C,), (0., 0.5, -0.5), (0.4, 0.3, 0.3), seed + 51)
    invstd = pick((C,), (1., 2.), (0.5, 0.5), seed + 52)
    b.save = torch.stack([mean, invstd], 0).view(2, 1, C)
    k = b.gamma * invstd
    c1 = pick((C,), (0., 0.5, -0.5), (0.4, 0.3, 0.3), seed + 53)
    c2 = pick((C,), (0., 0.5, -0.5), (0.4, 0.3, 0.3), seed + 54)
    sgx = -c1 * M / (k * invstd)
    sg = -(c2 + mean * c1) * M / k
    sga = sgx / invstd + mean * sg
    b.sp = _spread(torch.stack([sg, sga], -1), N)
    b.dgamma, b.dbeta = sgx, sg
    # the kernel's own expressions
    sgx_k = (sga - mean * sg) * invstd
    cb = torch.stack([k, -k * invstd * sgx_k / M, -k * sg / M + k * invstd * mean * sgx_k / M], -1)
    assert torch.equal(cb, torch.stack([k, c1, c2], -1)) and torch.equal(sgx_k, sgx)
    b.cb = cb[None].repeat(N, 1, 1)
    return b


def dw_mx_bn_fwd_case(case, S, seed=None):
    """(case, BN side) of x3d_dw333_fwd_stats: the hot case whose prologue is what the finalize derives."""
    b = dw_bn_fwd(case[0], case[1], S, DW_BN_SEED.get(tuple(case), 0) if seed is None else seed)
    return dw_mx_case(case, seed, pre=b.coef), b


def dw_mx_bn_bwd_case(case, seed=None):
    """(case, BN side) of x3d_dw333_bwd_stats: the hot case whose combine coefficients are what the finalize derives."""
    b = dw_bn_bwd(case[0], case[1], 0 if seed is None else seed)
    return dw_mx_case(case, seed, cb=b.cb), b


def dw_bn_splits(case):
    """The split counts the forward BN form is run with: one split per sample, and one split over both samples."""
    return [case[0]] + ([1] if case[0] == 2 else [])


# ----------------------------------------------------------------------------------------------------- case lists
# the shared lists of tests/test_ops_gpu.py (none dropped) plus the large-P rows
from tests.test_ops_gpu import DW_CASES, FUSED_CASES, PW_CASES, STEM_SHAPES  # noqa: E402

# the option-grid tests of tests/test_exact_gpu.py: persistent loops on 3 / 40 workgroups, 8- / 16-wave whole-K kernels, T segments
PW_GRID = [(2, 96, 216, 4, 10, 10, 1, 1), (3, 72, 162, 4, 10, 10, 1, 0), (2, 162, 100, 5, 6, 6, 1, 1), (5, 200, 120, 3, 6, 10, 1, 0),
           (3, 24, 54, 4, 20, 20, 1, 0), (2, 48, 108, 2, 14, 14, 1, 1), (2, 24, 54, 4, 79, 79, 1, 1)]
FUSED_GRID = [(3, 24, 54, 4, 20, 20, 1), (3, 54, 24, 4, 20, 20, 2), (2, 48, 108, 2, 14, 14, 1)]
PW_WAVES16 = [(2, 432, 192, 4, 5, 5, 1, 1), (2, 448, 256, 2, 4, 4, 1, 0), (2, 192, 432, 4, 5, 5, 1, 1), (2, 128, 512, 2, 4, 4, 1, 1),
              (2, 216, 300, 3, 6, 6, 1, 0), (3, 352, 150, 2, 5, 8, 1, 1)]
DW_TSEG = [(8, 432, 16, 7, 7, 1), (1, 7, 9, 7, 7, 1), (2, 40, 11, 5, 5, 2), (1, 2, 8, 40, 56, 1), (2, 5, 18, 14, 14, 2), (1, 3, 17, 7, 7, 1)]


# tests/test_dispatch_options_gpu.py: the kernels and plans behind the library's run-time options (x3d_set_option).
# X3D-XL widths (630 channels: K beyond the whole-K kernels' LDS tile, 40 M tiles); the last two have P = 50, P % 4 != 0
PW_XL = [(2, 280, 630, 4, 5, 5, 1, 0), (2, 630, 280, 4, 5, 5, 1, 2), (2, 630, 280, 2, 5, 5, 1, 1), (2, 280, 630, 2, 5, 5, 1, 1)]
PW_OPT_DENSE = [(2, 96, 216, 4, 10, 10, 1, 0), (2, 432, 192, 4, 5, 5, 1, 2), (2, 216, 96, 4, 10, 10, 1, 2)]     # pw4 / pw2 forward
PW_OPT_STREAM = [(2, 24, 54, 4, 8, 8, 1, 0), (2, 54, 24, 4, 14, 14, 1, 2), (3, 24, 54, 4, 20, 20, 1, 0)]        # pw3 for the stream kernel
# (N, P) on both sides of the float4 / 16-voxel choice of pw_plan: 2, 196 and 294 workgroups of 256 voxels
PW_OPT_NT4 = [(2, 24, 54, 4, 8, 8, 1, 0), (2, 24, 54, 4, 79, 79, 1, 1), (3, 24, 54, 4, 79, 79, 1, 1)]
PW_OPT_WHOLE_K = [(2, 108, 48, 4, 4, 4, 1, 2)]                          # K = 108, M = 48: the whole-K kernels at three M tiles
PW_OPT_DGRAD = [(2, 216, 96, 4, 10, 10, 1, 2), (2, 192, 432, 4, 5, 5, 1, 0), (2, 96, 216, 4, 12, 12, 1, 2)]    # pw4 / pw5 data gradient
PW_OPT_WGRAD = [(20, 96, 112, 8, 14, 14, 1, 2), (2, 48, 96, 4, 16, 16, 2, 1)]      # 500 chunks; the gathered stride-2 kernel
# one full 256-voxel tile per sample: the float4 form of the streaming kernels under pw_nt4_min = 0; 24 <-> 54 channels give M
# blocks of four and of two tiles in either direction, with raw and with activated input
PW_OPT_FLOAT4 = [(2, 24, 54, 4, 8, 8, 1, 0), (2, 54, 24, 4, 8, 8, 1, 0), (2, 24, 54, 4, 8, 8, 1, 1), (2, 54, 24, 4, 8, 8, 1, 1)]
PW_OPT_TILED = [(1, 96, 216, 2, 7, 7, 1, 0)]                            # P = 98, raw input, 14 M tiles: pw2's element loads, two tiles per wave
PW_OPT = (PW_XL + PW_OPT_DENSE + PW_OPT_STREAM + PW_OPT_NT4 + PW_OPT_WHOLE_K + PW_OPT_DGRAD + PW_OPT_WGRAD + PW_OPT_FLOAT4 +
          PW_OPT_TILED)
DW_OPT = [(2, 9, 2, 24, 24, 2), (2, 20, 2, 6, 6, 2), (2, 3, 8, 28, 28, 2), (2, 216, 4, 10, 10, 1), (2, 216, 4, 20, 20, 2),
          (4, 216, 2, 40, 40, 1), (1, 3, 3, 15, 11, 2), (2, 54, 4, 79, 79, 2)]
# stem weight gradient: N T 8 = 576 groups > the cap of 512; Wo = 130: two runs per output row (the second holds 2 voxels),
# 6 tiles on 8 groups -- float4 row loads (W % 4 == 0) and element loads
STEM_OPT = [(9, 3, 8, 16, 16), (1, 3, 1, 6, 260), (1, 3, 2, 5, 259)]


def _uniq(cases):
    return [c for i, c in enumerate(cases) if c not in cases[:i]]


PW_EXACT = PW_CASES + PW_LARGE_P
FUSED_EXACT = FUSED_CASES + FUSED_LARGE_P
DW_EXACT = DW_CASES + DW_LARGE_P
# every case shape the GPU tests use (what tests/test_exact_inputs_host.py proves exact)
PW_ALL, FUSED_ALL = _uniq(PW_EXACT + PW_GRID + PW_WAVES16 + PW_OPT), _uniq(FUSED_EXACT + FUSED_GRID)
DW_ALL = _uniq(DW_EXACT + DW_TSEG + DW_OPT)
STEM_EXACT = _uniq(list(STEM_SHAPES) + STEM_OPT)
HEAD_EXACT = [(R, K, HEAD_J, C) for R in HEAD_R for K in HEAD_K for C in HEAD_C]
