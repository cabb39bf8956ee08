"""A numpy restatement of the grouped update of include/x3dstep.h (x3dstep_apply_groups), independent of the library: the
tensor rule as two fp32 multiplies, the element rule with every fused multiply-add exact and rounded to fp32 once
(tests/guard_ref.py), and the bound that holds it against torch.optim.SGD run in fp64."""
import numpy as np

from tests import guard_ref

F32 = np.float32
EPS = 2.0 ** -24                 # half an ulp of fp32 relative to the result: one rounding to nearest


def tensor_rule(lr, wd, lr_scale, wd_scale):
    """(lr_s [S], wd_s [S]): lr * lr_scale and weight_decay * wd_scale, numpy's fp32 multiply (rounded once)."""
    return (F32(lr) * np.asarray(lr_scale, dtype=F32)).astype(F32), (F32(wd) * np.asarray(wd_scale, dtype=F32)).astype(F32)


def per_element(values, seg_off):
    """A per-tensor array spread over the elements of the flat buffer."""
    return np.repeat(np.asarray(values), np.diff(np.asarray(seg_off, dtype=np.int64)))


def group_rule(w, g, m, coef, lr_s, wd_s, mu, gs, first, nesterov):
    """(w', m') of the applied update; lr_s and wd_s are per element (per_element(tensor_rule(..)))."""
    w, g, m, lr_s, wd_s = (np.asarray(v, dtype=F32) for v in (w, g, m, lr_s, wd_s))
    coef, mu, gs = F32(coef), F32(mu), F32(gs)
    gi = g if coef == F32(1.0) else g * coef
    t = gi * gs
    gg = guard_ref.fma_f32(wd_s, w, t)
    mi = gg if first else guard_ref.fma_f32(mu, m, gg)
    u = guard_ref.fma_f32(mu, mi, gg) if nesterov else mi
    step = lr_s * u
    return (w - step).astype(F32), mi.astype(F32)


def group_rule_nonfinite(w, g, m, lr_s, wd_s, mu, gs, first, nesterov):
    """The unguarded form on a gradient with non-finite elements (coefficient 1): the finite elements through group_rule;
    for a non-finite g every fused multiply-add has a finite product and a non-finite addend, so it gives what the plain
    fp32 multiply and add give (an Inf of that sign, or a NaN)."""
    w, g, m, lr_s, wd_s = (np.asarray(v, dtype=F32) for v in (w, g, m, lr_s, wd_s))
    bad = ~np.isfinite(g)
    w1, m1 = group_rule(w, np.where(bad, F32(0), g), m, 1.0, lr_s, wd_s, mu, gs, first, nesterov)
    with np.errstate(all="ignore"):
        t = g[bad] * F32(gs)
        gg = wd_s[bad] * w[bad] + t
        mi = gg if first else F32(mu) * m[bad] + gg
        u = F32(mu) * mi + gg if nesterov else mi
        w1[bad] = w[bad] - lr_s[bad] * u
        m1[bad] = mi
    return w1, m1


def same_floats(a, b):
    """Byte for byte, except that a NaN equals any NaN (the payload and sign of a produced NaN are the hardware's)."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb)) and a[~na].tobytes() == b[~nb].tobytes()


class TorchBound:
    """The elementwise distance allowed between the fp32 rule and the same recursion in exact arithmetic (torch.optim.SGD
    in fp64, whose own roundings of 2^-53 are far below), carried over the steps.

    One step has seven roundings on the way to w' (gi = g * coef, t = gi * gs, gg, m', u, lr_s * u, the subtraction) and
    four on the way to m'; each is at most EPS times the sum of the absolute values of its operation's terms.  With
        T = |g coef gs|,  G = |wd_s w| + T,  M = mu |m| + G (G when first),  U = mu M + G (M without nesterov),
        X = lr_s U,  W = |w| + X
    the error of each stage is at most the number of roundings so far times EPS times the stage's magnitude (errors are
    carried forward by the same non-negative factors that build the magnitudes): 4 EPS M for m' and 7 EPS W for w'.  The
    step is linear in (w, m), so the errors Ew, Em of its inputs are carried as
        Emi = mu Em + wd_s Ew,  Eu = mu Emi + wd_s Ew (Emi without nesterov),  Ew' = Ew + lr_s Eu + 7 EPS W,
        Em' = Emi + 4 EPS M.
    (1 + 2^-20) covers the second-order terms ((1 + EPS)^7 - 1 - 7 EPS < 2^-43).  The magnitudes are taken from the fp64
    values."""

    def __init__(self, n):
        self.ew = np.zeros(n, np.float64)
        self.em = np.zeros(n, np.float64)

    def step(self, w, g, m, coef, lr_s, wd_s, mu, gs, first, nesterov):
        """w, m: the fp64 values before the step; returns (bound on w', bound on m') and keeps them for the next step."""
        w, g, m, lr_s, wd_s = (np.asarray(v, dtype=np.float64) for v in (w, g, m, lr_s, wd_s))
        mu = float(F32(mu))
        T = np.abs(g * float(F32(coef)) * float(F32(gs)))
        G = np.abs(wd_s * w) + T
        M = G if first else mu * np.abs(m) + G
        U = mu * M + G if nesterov else M
        W = np.abs(w) + lr_s * U
        emi = wd_s * self.ew if first else mu * self.em + wd_s * self.ew
        eu = mu * emi + wd_s * self.ew if nesterov else emi
        k = 1.0 + 2.0 ** -20
        self.ew = self.ew + lr_s * eu + 7 * EPS * W * k
        self.em = emi + 4 * EPS * M * k
        return self.ew, self.em
