"""A numpy restatement of the second-moment updates of include/x3dstep.h (x3dstep_adam, x3dstep_lamb_*), independent of the
library: the correction rule in Python's fp64 with one rounding per operation, the element rules in fp32 with numpy's
correctly rounded multiply, divide and square root and every fused multiply-add exact and rounded once
(tests/guard_ref.py), the LAMB trust rule in fp64."""
import numpy as np

from tests import group_ref, guard_ref

F32 = np.float32
F64 = np.float64
EPS = group_ref.EPS


def _pair_mul(x, y):
    """The product of two unevaluated sums of two doubles: the exact product of the leading parts by Veltkamp's split."""
    p = x[0] * y[0]
    c = 134217729.0 * x[0]
    xh = c - (c - x[0])
    xl = x[0] - xh
    c = 134217729.0 * y[0]
    yh = c - (c - y[0])
    yl = y[0] - yh
    e0 = ((xh * yh - p) + xh * yl + xl * yh) + xl * yl
    e = e0 + (x[0] * y[1] + x[1] * y[0])
    hi = p + e
    return hi, e - (hi - p)


def pow_count(b, k):
    """b ** k (k >= 0) by binary exponentiation on pairs of doubles: the leading part."""
    b, k = float(b), int(k)
    r, x = (1.0, 0.0), (b, 0.0)
    while k > 0:
        if k & 1:
            r = _pair_mul(r, x)
        k >>= 1
        if k > 0:
            x = _pair_mul(x, x)
    return r[0]


class Corr:
    """The correction rule of update k: fp64, each value rounded once."""

    def __init__(self, k, b1, b2):
        self.b1, self.b2 = F32(b1), F32(b2)
        self.bc1 = F64(1.0) - F64(pow_count(float(self.b1), k))
        self.bc2 = F64(1.0) - F64(pow_count(float(self.b2), k))
        self.rbc2 = F32(np.sqrt(self.bc2))
        self.omb1 = F32(F64(1.0) - F64(self.b1))
        self.omb2 = F32(F64(1.0) - F64(self.b2))
        self.bc1f, self.bc2f = F32(self.bc1), F32(self.bc2)

    def step_size(self, lr_s):
        return (np.asarray(lr_s, F32).astype(F64) / self.bc1).astype(F32)


def _grad(g, coef, gs):
    g = np.asarray(g, F32)
    gi = g if F32(coef) == F32(1.0) else g * F32(coef)
    return gi * F32(gs)


def _moments(t, m, v, c):
    m1 = guard_ref.fma_f32(c.b1, m, c.omb1 * t)
    v1 = guard_ref.fma_f32(c.b2, v, c.omb2 * (t * t))
    return m1.astype(F32), v1.astype(F32)


def adam_rule(w, g, m, v, coef, lr_s, wd_s, k, b1, b2, eps, gs, decoupled):
    """(w', m', v') of the applied update; lr_s and wd_s are per element."""
    w, m, v, lr_s, wd_s = (np.asarray(x, dtype=F32) for x in (w, m, v, lr_s, wd_s))
    c = Corr(k, b1, b2)
    t = _grad(g, coef, gs)
    if not decoupled:
        t = guard_ref.fma_f32(wd_s, w, t)
    m1, v1 = _moments(t, m, v, c)
    den = np.sqrt(v1) / c.rbc2 + F32(eps)
    w1 = guard_ref.fma_f32(-(lr_s * wd_s), w, w) if decoupled else w
    step = c.step_size(lr_s) * (m1 / den)
    return (w1 - step).astype(F32), m1, v1


def lamb_dir(w, m1, v1, wd_s, c, eps):
    mh = m1 / c.bc1f
    vh = v1 / c.bc2f
    return guard_ref.fma_f32(wd_s, w, mh / (np.sqrt(vh) + F32(eps))).astype(F32)


def lamb_moments(w, g, m, v, coef, wd_s, k, b1, b2, eps, gs):
    """(m', v', r) of launch 1."""
    w, m, v, wd_s = (np.asarray(x, dtype=F32) for x in (w, m, v, wd_s))
    c = Corr(k, b1, b2)
    m1, v1 = _moments(_grad(g, coef, gs), m, v, c)
    return m1, v1, lamb_dir(w, m1, v1, wd_s, c, eps)


def lamb_trust(wsumsq, rsumsq, adapt, nonfinite):
    """trust fp32 [S] from the per-tensor sums of squares (fp64 [S])."""
    with np.errstate(all="ignore"):
        a, b = np.sqrt(np.asarray(wsumsq, F64)), np.sqrt(np.asarray(rsumsq, F64))
        q = (a / b).astype(F32)
    ok = (np.asarray(adapt) != 0) & (a > 0) & (b > 0) & (np.asarray(nonfinite) == 0) & np.isfinite(q)
    return np.where(ok, q, F32(1.0)).astype(F32)


def lamb_apply(w, r, lr_s, trust):
    """w' of launch 3; lr_s and trust are per element."""
    w, r, lr_s, trust = (np.asarray(x, dtype=F32) for x in (w, r, lr_s, trust))
    return (w - (lr_s * trust) * r).astype(F32)
