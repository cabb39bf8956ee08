"""tests/bn_ref.py (the fp64 restatements the kernel-level GPU tests of csrc/bn.hip compare with) proved against torch
autograd in fp64 ON WHOLE TENSORS: a closed form is not trusted because it looks like the kernel.  CPU only.

Criterion: 1e-10 relative (fp64 against fp64; statistics tiles kept in fp64)."""
import pytest
import torch
import torch.nn.functional as F

from tests import bn_ref

D = torch.float64
EPS = 1e-5
TOL = 1e-10


def _g(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=D)


def _rel(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def _raw(N, C, P, seed=0, constant_channel=False):
    raw = _g(N, C, P, seed=seed) * (0.5 + _g(C, seed=seed + 1).abs()).view(1, C, 1) + _g(C, seed=seed + 2).view(1, C, 1)
    if constant_channel:
        raw[:, C - 1, :] = 1.625
    return raw


def _split_bn(raw, S, gamma, beta, eps):
    """SubBatchNorm3d.forward in training (x3d.py:47-58): sample n is normalised with the statistics of split n % S."""
    out = torch.empty_like(raw)
    for j in range(S):
        x = raw[j::S]
        mean = x.mean(dim=(0, 2), keepdim=True)
        var = x.var(dim=(0, 2), unbiased=False, keepdim=True)
        out[j::S] = (x - mean) / torch.sqrt(var + eps) * gamma.view(1, -1, 1) + beta.view(1, -1, 1)
    return out


# (N, C, P, S, tiles, constant channel): S in 1, 2, 3, 4; N = S (one sample per split); a constant channel (variance clamp)
BN_CASES = [(4, 5, 24, 1, 3, False), (4, 10, 24, 2, 5, False), (6, 7, 15, 3, 1, False), (8, 3, 9, 4, 9, False),
            (3, 4, 20, 3, 4, False), (4, 6, 11, 4, 2, False), (1, 3, 7, 1, 2, False),
            (4, 5, 24, 2, 3, True), (2, 4, 16, 2, 1, True), (16, 24, 98, 2, 7, False)]


@pytest.mark.parametrize("case", BN_CASES)
@pytest.mark.parametrize("momentum", [0.1, 0.25])
def test_bn_fwd_finalize_is_batch_norm_per_split(case, momentum):
    N, C, P, S, tiles, const = case
    raw = _raw(N, C, P, seed=1, constant_channel=const)
    gamma, beta = 1 + 0.2 * _g(C, seed=4), 0.3 * _g(C, seed=5)
    rm0, rv0 = 0.1 * _g(S, C, seed=6), 1 + 0.1 * _g(S, C, seed=7).abs()
    eps32, mom32 = float(bn_ref._s(EPS)), float(bn_ref._s(momentum))         # (what the C ABI's `float` arguments hold)
    part = bn_ref.partials_of(raw, tiles, dtype=D)
    assert part.shape == (N, C, tiles, 2)
    coef, save, nsum, rm, rv = bn_ref.bn_fwd_finalize(part, S, P, gamma, beta, rm0, rv0, momentum, EPS)
    y = bn_ref.bn_affine(raw, coef)
    for j in range(S):
        a, b = rm0[j].clone(), rv0[j].clone()
        yj = F.batch_norm(raw[j::S], a, b, gamma, beta, training=True, momentum=mom32, eps=eps32)
        assert _rel(y[j::S], yj) < TOL
        assert _rel(rm[j], a) < TOL and _rel(rv[j], b) < TOL               # running statistics: momentum, UNBIASED variance
        x = raw[j::S]
        assert _rel(save[0, j], x.mean(dim=(0, 2))) < TOL
        if not const:
            assert _rel(save[1, j], 1 / torch.sqrt(x.var(dim=(0, 2), unbiased=False) + eps32)) < TOL
    if const:                                                                # clamp: var = 0 -> invstd = 1 / sqrt(eps)
        assert _rel(save[1, :, C - 1], torch.full((S,), eps32 ** -0.5, dtype=D)) < 1e-6
    assert _rel(nsum, raw.sum(2)) < TOL
    # eval: coefficients from the running statistics
    ce = bn_ref.bn_eval_coef(rm[0], rv[0], gamma, beta, N, EPS)
    ye = F.batch_norm(raw, rm[0].clone(), rv[0].clone(), gamma, beta, training=False, eps=eps32)
    assert _rel(bn_ref.bn_affine(raw, ce), ye) < TOL


def test_bn_fwd_finalize_single_element_groups_are_finite():
    """count * N / S == 1: the unbiased factor cnt / (cnt - 1) is not applied (the biased variance, 0, is used)."""
    raw = _raw(3, 4, 1, seed=2)
    part = bn_ref.partials_of(raw, 1, dtype=D)
    rm0, rv0 = torch.zeros(3, 4, dtype=D), torch.ones(3, 4, dtype=D)
    coef, save, nsum, rm, rv = bn_ref.bn_fwd_finalize(part, 3, 1, torch.ones(4, dtype=D), torch.zeros(4, dtype=D), rm0, rv0)
    for t in (coef, save, rm, rv):
        assert bool(torch.isfinite(t).all())
    assert _rel(rv, torch.full((3, 4), 1 - float(bn_ref._s(0.1)), dtype=D)) < 1e-12


@pytest.mark.parametrize("case", BN_CASES)
def test_bn_bwd_finalize_is_the_autograd_gradient(case):
    N, C, P, S, tiles, const = case
    raw = _raw(N, C, P, seed=1, constant_channel=const).requires_grad_(True)
    gamma, beta = (1 + 0.2 * _g(C, seed=4)).requires_grad_(True), (0.3 * _g(C, seed=5)).requires_grad_(True)
    eps32 = float(bn_ref._s(EPS))
    g = _g(N, C, P, seed=8)
    (_split_bn(raw, S, gamma, beta, eps32) * g).sum().backward()
    _, save, _, _, _ = bn_ref.bn_fwd_finalize(bn_ref.partials_of(raw, tiles, dtype=D), S, P, gamma, beta, eps=EPS)
    part = bn_ref.partials_of(g, tiles, raw, seed=3, dtype=D)
    cb, dgamma, dbeta = bn_ref.bn_bwd_finalize(part, S, P, gamma, save)
    draw = bn_ref.bn_affine(raw, cb, g)
    assert _rel(draw, raw.grad) < TOL
    assert _rel(dgamma, gamma.grad) < TOL and _rel(dbeta, beta.grad) < TOL
    # accumulate = 1
    _, dg1, db1 = bn_ref.bn_bwd_finalize(part, S, P, gamma, save, dgamma0=_g(C, seed=9), dbeta0=_g(C, seed=10))
    assert _rel(dg1, gamma.grad + _g(C, seed=9)) < TOL and _rel(db1, beta.grad + _g(C, seed=10)) < TOL


# (N, C, Wd, P, S, tiles, constant channel)
SE_CASES = [(4, 10, 3, 24, 2, 5, False), (3, 7, 4, 15, 3, 2, False), (2, 5, 2, 9, 1, 9, False), (4, 6, 5, 12, 4, 1, False),
            (8, 12, 4, 10, 4, 3, False), (4, 10, 3, 24, 2, 4, True), (16, 216, 16, 784, 2, 13, False),
            (8, 432, 32, 196, 1, 7, False)]


@pytest.mark.parametrize("case", SE_CASES)
def test_se_bn_closed_forms_are_the_autograd_gradients(case):
    """s = bn(raw) * sigmoid(W2 relu(W1 mean_p(bn(raw)) + b1) + b2): the forward restatement gives s, and A ds + B raw + C
    and the six parameter gradients of se_bn_bwd_finalize equal autograd's."""
    N, C, Wd, P, S, tiles, const = case
    raw = _raw(N, C, P, seed=11, constant_channel=const).requires_grad_(True)
    leaf = lambda t: t.requires_grad_(True)
    gamma, beta = leaf(1 + 0.2 * _g(C, seed=12)), leaf(0.3 * _g(C, seed=13))
    w1, b1 = leaf(_g(Wd, C, seed=14) / C ** 0.5), leaf(0.1 * _g(Wd, seed=15))
    w2, b2 = leaf(_g(C, Wd, seed=16) / Wd ** 0.5), leaf(0.1 * _g(C, seed=17))
    eps32 = float(bn_ref._s(EPS))
    y = _split_bn(raw, S, gamma, beta, eps32)
    gate = torch.sigmoid(torch.relu(y.mean(2) @ w1.t() + b1) @ w2.t() + b2)
    s = y * gate.unsqueeze(-1)
    ds = _g(N, C, P, seed=18)
    (s * ds).sum().backward()
    part = bn_ref.partials_of(raw, tiles, dtype=D)
    coef_out, save, nsum, se, z, pool, _, _ = bn_ref.se_bn_fwd(part, S, P, gamma, beta, None, None, w1, b1, w2, b2, eps=EPS)
    assert _rel(bn_ref.bn_affine(raw, coef_out), s) < TOL
    assert _rel(se, gate) < TOL and _rel(pool, y.mean(2)) < TOL
    bpart = bn_ref.partials_of(ds, tiles, raw, seed=5, dtype=D)
    cb, gr = bn_ref.se_bn_bwd_finalize(bpart, S, P, gamma, beta, save, nsum, w1, w2, se, z, pool)
    assert _rel(bn_ref.bn_affine(raw, cb, ds), raw.grad) < TOL
    for name, leaf_t in (("dgamma", gamma), ("dbeta", beta), ("dw1", w1), ("db1", b1), ("dw2", w2), ("db2", b2)):
        assert _rel(gr[name], leaf_t.grad) < TOL, name


def test_elementwise_restatements_are_the_autograd_gradients():
    N, C, T, HW = 3, 4, 5, 6
    a3, res = _g(N, C, T, HW, seed=1).requires_grad_(True), _g(N, C, T, HW, seed=2)
    c3 = torch.stack([1 + 0.2 * _g(N, C, seed=3), 0.3 * _g(N, C, seed=4)], -1)
    cd = torch.stack([1 + 0.2 * _g(N, C, seed=5), 0.3 * _g(N, C, seed=6)], -1)
    bc = lambda c, k: c[..., k, None, None]
    dout = _g(N, C, T, HW, seed=7)
    for q in (None, cd):
        ref = torch.relu(bc(c3, 0) * a3 + bc(c3, 1) + (bc(q, 0) * res + bc(q, 1) if q is not None else res))
        out = bn_ref.bn_add_relu_fwd(a3, c3, res, q)
        assert _rel(out, ref.detach()) < 1e-14
        g, part, part_d, _, _ = bn_ref.bn_add_relu_bwd(dout, out, a3, res if q is not None else None)
        a3.grad = None
        (ref * dout).sum().backward()
        assert _rel(g * bc(c3, 0), a3.grad) < 1e-14
        assert _rel(part.sum(2)[..., 1], (g * a3.detach()).sum(dim=(2, 3))) < 1e-13
    for segs in (1, T):
        a5 = _g(N, C, T, HW, seed=8).requires_grad_(True)
        pooled = torch.relu(bc(c3, 0) * a5 + bc(c3, 1)).reshape(N, C, segs, -1).mean(-1)
        got, _ = bn_ref.bn_relu_pool_fwd(a5, c3, segs)
        assert _rel(got, pooled) < 1e-14
        dp = _g(N, C, segs, seed=9)
        (pooled * dp).sum().backward()
        g, _, _, _ = bn_ref.bn_relu_pool_bwd(a5, c3, dp, segs)
        assert _rel(g.reshape(N, C, T, HW) * bc(c3, 0), a5.grad) < 1e-14


def test_near_tie_share_of_the_pool_backward_mask_rule():
    """The exclusion rule of the GPU test (|sc a + sh| < 2^-22 (|sc a| + |sh|)) leaves out far less than 1e-5 of
    standard-normal inputs."""
    a = _g(4000000, seed=3)
    t1 = 1.13 * a
    share = ((t1 + 0.27).abs() < 2.0 ** -22 * (t1.abs() + 0.27)).double().mean().item()
    assert share <= 1e-5


@pytest.mark.parametrize("wd,mu", [(5e-5, 0.9), (0.0, 0.9), (5e-5, 0.0)])
def test_sgd_and_grad_accumulate_restatements(wd, mu):
    n, lr, gs = 257, 0.1, 0.125
    w0, gr = _g(n, seed=1), _g(n, seed=2)
    f32 = lambda v: float(bn_ref._s(v))
    p = torch.nn.Parameter(w0.clone())
    opt = torch.optim.SGD([p], lr=f32(lr), momentum=f32(mu), weight_decay=f32(wd))
    w, m = w0.clone(), torch.zeros(n, dtype=D)
    for it in range(3):
        p.grad = gr * (it + 1) * gs
        opt.step()
        w, m = bn_ref.sgd(w, gr * (it + 1), m, lr, mu, wd, gs, first=(it == 0))
    assert _rel(w, p.detach()) < 1e-13
    acc = bn_ref.grad_accumulate(torch.full((n,), float("nan"), dtype=D), gr, 1 / 3, True)
    acc = bn_ref.grad_accumulate(acc, w0, 1 / 3, False)
    assert _rel(acc, f32(1 / 3) * (gr + w0)) < 1e-14
