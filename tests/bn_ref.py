"""Plain restatements of every entry point of csrc/bn.hip (include/x3dhip.h: split-BN finalize, SE branch, residual
epilogue, head pooling, stand-alone SubBatchNorm3d, gradient accumulation, SGD), CPU only, torch only.

Each function takes THE ARRAYS THE KERNEL TAKES (fp32 values, widened to `dt`) and evaluates x3d.py's semantics in `dt`
(float64 by default), so that a comparison isolates the kernel.  Scalars a kernel receives as `float` (momentum, eps,
scale, lr ...) are rounded to fp32 first, as the C ABI does.  `dt=torch.float32` evaluates the same function in plain
fp32: the tests use it to MEASURE the fp32 floor of the SE arithmetic (never as a reference).

tests/test_bn_ref_host.py proves the closed forms against torch autograd in fp64 on whole tensors.

Functions with `with_scale=True` also return, per output, the largest-magnitude term of that output's expression (the
`scale` of the tolerance rule |got - ref| <= 2^-23 |ref| + 2^-23 scale; it matters for differences such as shift and C).
"""
import numpy as np
import torch

D = torch.float64


def _t(x, dt=D):
    return None if x is None else torch.as_tensor(x).detach().cpu().to(dt)


def _s(v, dt=D):
    """A `float` argument of the C ABI: rounded to fp32, then widened."""
    return torch.tensor(float(v), dtype=torch.float32).to(dt)


def _split_sum(x, S):
    """[N, ...] -> [S, ...]: sum over the samples of each split (sample n is in split n % S, x3d.py:50)."""
    return x.reshape((x.shape[0] // S, S) + tuple(x.shape[1:])).sum(0)


def _per_sample(v, N):
    """[S, ...] -> [N, ...]: row n = v[n % S]."""
    return v.repeat((N // v.shape[0],) + (1,) * (v.dim() - 1))


def _mx(*ts):
    out = ts[0].abs()
    for t in ts[1:]:
        out = torch.maximum(out, t.abs())
    return out


def _bc(c, k, nd):
    """coef[N, C, K] -> component k broadcast over the trailing dims of an [N, C, ...] tensor with nd dims."""
    return c[..., k].reshape(c.shape[:2] + (1,) * (nd - 2))


# ----------------------------------------------------------------------------------------------------------- partial sums
def tile_bounds(P, tiles, seed=0):
    """Start offsets of `tiles` contiguous, deliberately UNEVEN, non-empty chunks of range(P)."""
    assert 1 <= tiles <= P
    if tiles == 1:
        return np.zeros(1, dtype=np.int64)
    rng = np.random.RandomState(1000 + seed)
    cuts = np.sort(rng.choice(np.arange(1, P), size=tiles - 1, replace=False))
    return np.concatenate([[0], cuts]).astype(np.int64)


def partials_of(t, tiles, u=None, seed=0, dtype=torch.float32):
    """Statistics tiles of a real tensor: cut the P axis of t[N, C, P] (fp64) into `tiles` uneven chunks and return
    partial[N, C, tiles, 2] = {sum t, sum t * (t if u is None else u)} per chunk, rounded to `dtype`
    (u is None: {sum x, sum x^2} for the forward; t = g, u = raw: {sum g, sum g * raw} for the backward)."""
    t = _t(t).reshape(t.shape[0], t.shape[1], -1)
    v = t * (t if u is None else _t(u).reshape(t.shape))
    idx = tile_bounds(t.shape[2], tiles, seed)
    a = np.add.reduceat(t.numpy(), idx, axis=2)
    b = np.add.reduceat(v.numpy(), idx, axis=2)
    return torch.from_numpy(np.stack([a, b], -1)).to(dtype)


def ew_tile_sums(*terms, tile=2048):
    """Per-tile fp64 sums over the flattened trailing dims of [N, C, ...] tensors, tiles of `tile` elements (EW_TILE):
    returns [N, C, ceil(P / tile), len(terms)]."""
    outs = []
    for t in terms:
        t = _t(t)
        t = t.reshape(t.shape[0], t.shape[1], -1)
        idx = np.arange(0, t.shape[2], tile)
        outs.append(np.add.reduceat(t.numpy(), idx, axis=2))
    return torch.from_numpy(np.stack(outs, -1))


# ------------------------------------------------------------------------------------------------------ split BN finalize
def bn_fwd_finalize(partial, S, count, gamma, beta, rmean=None, rvar=None, momentum=0.1, eps=1e-5, dt=D, with_scale=False):
    """x3d_bn_fwd_finalize.  -> coef[N, C, 2], save[2, S, C], nsum[N, C], rmean'[S, C], rvar'[S, C] (None without rmean).
    Biased variance for invstd, unbiased (cnt / (cnt - 1); cnt == 1: the biased one, which is 0) for the running update;
    var < 0 clamps to 0."""
    p, g, b = _t(partial, dt), _t(gamma, dt), _t(beta, dt)
    N = p.shape[0]
    mom, e = _s(momentum, dt), _s(eps, dt)
    d = p.sum(2)                                           # [N, C, 2]
    cnt = float(count) * (N // S)
    s = _split_sum(d, S)                                   # [S, C, 2]
    mean = s[..., 0] / cnt
    var = (s[..., 1] / cnt - mean * mean).clamp_min(0)
    invstd = 1 / torch.sqrt(var + e)
    sc, t = g * invstd, mean * g * invstd
    coef = torch.stack([_per_sample(sc, N), _per_sample(b - t, N)], -1)
    save = torch.stack([mean, invstd], 0)
    nsum = d[..., 0]
    rm = rv = srm = srv = None
    if rmean is not None:
        unb = var * cnt / (cnt - 1) if cnt > 1 else var
        r0, v0 = _t(rmean, dt).reshape(mean.shape), _t(rvar, dt).reshape(mean.shape)
        rm, rv = (1 - mom) * r0 + mom * mean, (1 - mom) * v0 + mom * unb
        srm, srv = _mx((1 - mom) * r0, mom * mean), _mx((1 - mom) * v0, mom * unb)
    out = (coef, save, nsum, rm, rv)
    if not with_scale:
        return out
    scale = (torch.stack([_per_sample(sc.abs(), N), _per_sample(_mx(b.expand_as(t), t), N)], -1), save.abs(), nsum.abs(),
             srm, srv)
    return out, scale


def bn_eval_coef(rmean, rvar, gamma, beta, N, eps=1e-5, dt=D, with_scale=False):
    """x3d_bn_eval_coef: coef[N, C, 2] from the (aggregated) running statistics."""
    m, v, g, b = _t(rmean, dt), _t(rvar, dt), _t(gamma, dt), _t(beta, dt)
    invstd = 1 / torch.sqrt(v + _s(eps, dt))
    sc, t = g * invstd, m * g * invstd
    coef = torch.stack([sc, b - t], -1).unsqueeze(0).repeat(N, 1, 1)
    if not with_scale:
        return coef
    return coef, torch.stack([sc.abs(), _mx(b, t)], -1).unsqueeze(0).repeat(N, 1, 1)


def bn_bwd_finalize(partial, S, count, gamma, save, dgamma0=None, dbeta0=None, dt=D, with_scale=False):
    """x3d_bn_bwd_finalize.  partial = {sum g, sum g * raw}; -> cb[N, C, 3] = {A, B, C} with d raw = A g + B raw + C,
    dgamma[C], dbeta[C] (added to dgamma0 / dbeta0 when given: accumulate = 1)."""
    p, g, sv = _t(partial, dt), _t(gamma, dt), _t(save, dt)
    N = p.shape[0]
    M = float(count) * (N // S)
    s = _split_sum(p.sum(2), S)
    sg, sga = s[..., 0], s[..., 1]
    mean, invstd = sv[0], sv[1]
    k = g * invstd
    sgx = (sga - mean * sg) * invstd
    A = k.expand_as(sgx)
    B = -k * invstd * sgx / M
    Cc = -k * sg / M + k * invstd * mean * sgx / M
    cb = torch.stack([_per_sample(A, N), _per_sample(B, N), _per_sample(Cc, N)], -1)
    dg, db = sgx.sum(0), sg.sum(0)
    sdg = _mx(sga * invstd, mean * sg * invstd).max(0).values
    sdb = sg.abs().max(0).values
    if dgamma0 is not None:
        g0, b0 = _t(dgamma0, dt), _t(dbeta0, dt)
        dg, db, sdg, sdb = dg + g0, db + b0, _mx(sdg, g0), _mx(sdb, b0)
    if not with_scale:
        return cb, dg, db
    q = k * invstd * invstd / M
    sB = _mx(q * sga, q * mean * sg)
    sC = _mx(k * sg / M, q * mean * sga, q * mean * mean * sg)
    return (cb, dg, db), (torch.stack([_per_sample(A.abs(), N), _per_sample(sB, N), _per_sample(sC, N)], -1), sdg, sdb)


# ------------------------------------------------------------------------------------------------------------ SE branch
def se_fwd(coef, nsum, count, w1, b1, w2, b2, dt=D):
    """x3d_se_fwd (x3d.py:153-159 on pooled statistics) -> coef_out[N, C, 2], se[N, C], z[N, Wd], pool[N, C]."""
    cf, ns = _t(coef, dt), _t(nsum, dt)
    w1, b1, w2, b2 = _t(w1, dt), _t(b1, dt), _t(w2, dt), _t(b2, dt)
    pool = cf[..., 0] * ns / float(count) + cf[..., 1]
    z = torch.relu(pool @ w1.t() + b1)
    se = torch.sigmoid(z @ w2.t() + b2)
    return cf * se.unsqueeze(-1), se, z, pool


def se_bn_fwd(partial, S, count, gamma, beta, rmean, rvar, w1, b1, w2, b2, momentum=0.1, eps=1e-5, dt=D, with_scale=False):
    """x3d_se_bn_fwd = bn_fwd_finalize (bn2) + se_fwd -> coef_out, save, nsum, se, z, pool, rmean', rvar'."""
    r = bn_fwd_finalize(partial, S, count, gamma, beta, rmean, rvar, momentum, eps, dt=dt, with_scale=with_scale)
    (coef, save, nsum, rm, rv), scale = r if with_scale else (r, None)
    coef_out, se, z, pool = se_fwd(coef, nsum, count, w1, b1, w2, b2, dt=dt)
    out = (coef_out, save, nsum, se, z, pool, rm, rv)
    return (out, scale) if with_scale else out


def se_bn_bwd_finalize(partial, S, count, gamma, beta, save, nsum, w1, w2, se, z, pool, dt=D):
    """x3d_se_bn_bwd_finalize.  partial = {sum ds, sum ds * raw}, ds = gradient w.r.t. s = bn2(raw) * se.
    -> cb[N, C, 3] (d raw = A ds + B raw + C) and dict(dgamma, dbeta, dw1, db1, dw2, db2)."""
    p, g, b, sv, ns = _t(partial, dt), _t(gamma, dt), _t(beta, dt), _t(save, dt), _t(nsum, dt)
    w1, w2, se, z, pool = _t(w1, dt), _t(w2, dt), _t(se, dt), _t(z, dt), _t(pool, dt)
    N = p.shape[0]
    cntf = float(count)
    M = cntf * (N // S)
    d = p.sum(2)
    d0, d1 = d[..., 0], d[..., 1]
    mean, invstd = _per_sample(sv[0], N), _per_sample(sv[1], N)       # [N, C]
    k = g * invstd
    h = b - mean * k
    dse = k * d1 + h * d0                                  # sum_p ds * bn2(raw)
    dz2 = dse * se * (1 - se)
    dz1 = (dz2 @ w2) * (z > 0).to(dt)                      # [N, Wd]
    dpool = dz1 @ w1                                       # [N, C]
    grads = dict(dw2=dz2.t() @ z, db2=dz2.sum(0), dw1=dz1.t() @ pool, db1=dz1.sum(0))
    # gradient w.r.t. y = bn2(raw): se * ds + dpool / count at every voxel
    sg = _split_sum(se * d0 + dpool, S)
    sgx = _split_sum(se * (d1 - mean * d0) * invstd + (dpool / cntf) * (ns - cntf * mean) * invstd, S)
    ks, ms, iv = g * sv[1], sv[0], sv[1]
    B = -ks * iv * sgx / M
    Cb = -ks * sg / M + ks * iv * ms * sgx / M
    cb = torch.stack([k * se, _per_sample(B, N), _per_sample(Cb, N) + k * dpool / cntf], -1)
    grads["dgamma"], grads["dbeta"] = sgx.sum(0), sg.sum(0)
    return cb, grads


# ----------------------------------------------------------------------------------------- residual epilogue, head pooling
def bn_add_relu_fwd(a3, c3, res, cd=None, dt=D, with_terms=False):
    """x3d_bn_add_relu_fwd: out = relu(c3 * a3 + (cd * res if cd is given else res))."""
    a, c, r = _t(a3, dt), _t(c3, dt), _t(res, dt)
    t1, t2 = _bc(c, 0, a.dim()) * a, _bc(c, 1, a.dim()).expand_as(a)
    if cd is not None:
        q = _t(cd, dt)
        t3, t4 = _bc(q, 0, a.dim()) * r, _bc(q, 1, a.dim()).expand_as(a)
    else:
        t3, t4 = r, torch.zeros_like(r)
    out = torch.relu(t1 + t2 + t3 + t4)
    return (out, t1.abs() + t2.abs() + t3.abs() + t4.abs()) if with_terms else out


def bn_add_relu_bwd(dout, out, a3, ad=None, dt=D):
    """x3d_bn_add_relu_bwd: g = dout * (out > 0); fp64 tile sums partial {sum g, sum g a3} (partial_d {sum g, sum g ad})
    and the per-tile sums of |terms| (same layout) for the tolerance."""
    d, o, a = _t(dout, dt), _t(out, dt), _t(a3, dt)
    g = torch.where(o > 0, d, torch.zeros_like(d))
    part, mag = ew_tile_sums(g, g * a), ew_tile_sums(g.abs(), (g * a).abs())
    if ad is None:
        return g, part, None, mag, None
    b = _t(ad, dt)
    return g, part, ew_tile_sums(g, g * b), mag, ew_tile_sums(g.abs(), (g * b).abs())


def bn_relu_pool_fwd(a5, c5, segs=1, dt=D):
    """x3d_bn_relu_pool_fwd: pooled[N, C, segs] = mean over segment (P / segs contiguous elements) of relu(c5 * a5);
    also the mean of |sc a| + |sh| per segment (magnitude of the terms)."""
    a, c = _t(a5, dt), _t(c5, dt)
    N, C = a.shape[:2]
    a = a.reshape(N, C, segs, -1)
    t1, t2 = _bc(c, 0, 4) * a, _bc(c, 1, 4).expand_as(a)
    return torch.relu(t1 + t2).mean(-1), (t1.abs() + t2.abs()).mean(-1)


def bn_relu_pool_bwd(a5, c5, dpooled, segs=1, dt=D):
    """x3d_bn_relu_pool_bwd: g = dpooled[n, c, s] / (P / segs) * (c5 * a5 > 0) -> g [N, C, P], d (g without the mask),
    pre = c5 * a5 (the mask's argument) and |sc a| + |sh|."""
    a, c, dp = _t(a5, dt), _t(c5, dt), _t(dpooled, dt)
    N, C = a.shape[:2]
    a = a.reshape(N, C, segs, -1)
    t1, t2 = _bc(c, 0, 4) * a, _bc(c, 1, 4).expand_as(a)
    d = (dp.reshape(N, C, segs, 1) / a.shape[-1]).expand_as(a)
    pre = t1 + t2
    g = torch.where(pre > 0, d, torch.zeros_like(d))
    r = lambda t: t.reshape(N, C, -1)
    return r(g), r(d), r(pre), r(t1.abs() + t2.abs())


# ----------------------------------------------------------------------------------------------- stand-alone SubBatchNorm3d
def bn_rowstats(x, g=None, dt=D):
    """x3d_bn_rowstats: fp64 tile sums {sum x, sum x^2} (g is None) or {sum g, sum g x}, and the sums of |terms|."""
    x = _t(x, dt)
    if g is None:
        return ew_tile_sums(x, x * x), ew_tile_sums(x.abs(), x * x)
    g = _t(g, dt)
    return ew_tile_sums(g, g * x), ew_tile_sums(g.abs(), (g * x).abs())


def bn_affine(x, coef, g=None, dt=D, with_terms=False):
    """x3d_bn_affine: out = c0 x + c1 (coef[N, C, 2]) or c0 g + c1 x + c2 (coef[N, C, 3])."""
    x, c = _t(x, dt), _t(coef, dt)
    if c.shape[-1] == 2:
        ts = (_bc(c, 0, x.dim()) * x, _bc(c, 1, x.dim()).expand_as(x))
    else:
        ts = (_bc(c, 0, x.dim()) * _t(g, dt), _bc(c, 1, x.dim()) * x, _bc(c, 2, x.dim()).expand_as(x))
    out = sum(ts)
    return (out, sum(t.abs() for t in ts)) if with_terms else out


# ------------------------------------------------------------------------------------------ gradient accumulation and SGD
def grad_accumulate(acc, g, scale, first, dt=D, with_terms=False):
    """x3d_grad_accumulate: acc' = (0 if first else acc) + scale * g."""
    a, g = _t(acc, dt), _t(g, dt)
    t = _s(scale, dt) * g
    out = t if first else a + t
    return (out, t.abs() if first else a.abs() + t.abs()) if with_terms else out


def sgd(w, g, m, lr, momentum=0.9, weight_decay=5e-5, grad_scale=1.0, first=False, dt=D, with_terms=False):
    """x3d_sgd_fused (torch.optim.SGD): g' = grad_scale g + wd w; m' = g' if first else mu m + g'; w' = w - lr m'."""
    w, g, m = _t(w, dt), _t(g, dt), _t(m, dt)
    lr, mu, wd, gs = _s(lr, dt), _s(momentum, dt), _s(weight_decay, dt), _s(grad_scale, dt)
    gi = g * gs + wd * w
    mi = gi if first else mu * m + gi
    wo = w - lr * mi
    if not with_terms:
        return wo, mi
    tm = (g * gs).abs() + (wd * w).abs() + (0 if first else (mu * m).abs())
    return wo, mi, w.abs() + lr * tm, tm
