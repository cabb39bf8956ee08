"""A numpy restatement of the trust ratios of include/x3dstep.h (x3dstep_trust, x3dstep_apply_lars), independent of the
library: the trust rule in fp64 with one rounding per operation, the element rule in fp32 with every fused multiply-add
exact and rounded once (tests/guard_ref.py), and the bound that holds it against a LARS written with plain torch in fp64."""
import numpy as np

from tests import group_ref, guard_ref

F32 = np.float32
F64 = np.float64
EPS = group_ref.EPS


def trust_rule(wsumsq, gsumsq, nonfinite, eta, lr_scale, wd_scale, lr, wd, gs, coef, eps, clip):
    """trust fp32 [S] from the per-tensor sums of squares of the weights and of the recorded gradient (fp64 [S]), the
    count of non-finite gradient elements, eta and the scales (fp32 [S]) and the scalars of the call."""
    wsumsq, gsumsq = np.asarray(wsumsq, F64), np.asarray(gsumsq, F64)
    eta = np.asarray(eta, F32)
    lr_s, wd_s = group_ref.tensor_rule(lr, wd, lr_scale, wd_scale)
    with np.errstate(all="ignore"):
        a = np.sqrt(wsumsq)
        b = np.sqrt(gsumsq) * F64(F32(gs)) * F64(F32(coef))
        den = (b + wd_s.astype(F64) * a) + F64(F32(eps))
        r = (eta.astype(F64) * a) / den
        if clip:
            r = np.where(lr_s > 0, np.minimum(r / np.where(lr_s > 0, lr_s, F32(1)).astype(F64), 1.0), 1.0)
        r32 = r.astype(F32)
    ok = (eta > 0) & (a > 0) & (b > 0) & (np.asarray(nonfinite) == 0) & np.isfinite(r32)
    return np.where(ok, r32, F32(1.0)).astype(F32)


def lars_rule(w, g, m, coef, lr_s, wd_s, trust, mu, gs, first, nesterov):
    """(w', m') of the applied update; lr_s, wd_s and trust are per element."""
    w, g, m, lr_s, wd_s, trust = (np.asarray(v, dtype=F32) for v in (w, g, m, lr_s, wd_s, trust))
    coef, mu, gs = F32(coef), F32(mu), F32(gs)
    gi = g if coef == F32(1.0) else g * coef
    t = gi * gs
    gg = guard_ref.fma_f32(wd_s, w, t)
    gl = np.where(trust == F32(1.0), gg, gg * trust).astype(F32)
    mi = gl if first else guard_ref.fma_f32(mu, m, gl)
    u = guard_ref.fma_f32(mu, mi, gl) if nesterov else mi
    step = lr_s * u
    return (w - step).astype(F32), mi.astype(F32)


class TorchBound:
    """group_ref.TorchBound with the trust ratio: the distance allowed between the fp32 rule and the same recursion in
    exact arithmetic (a LARS in plain torch, fp64), carried over the steps.

    The decayed gradient gg has three roundings (g * coef, * gs, the fma) relative to G = |wd_s w| + |g coef gs|.  The
    fp32 rule multiplies it by trust32, which differs from the exact ratio r by the fp32 rounding of the ratio (2^-24)
    and the fp64 work before it (`dr`, relative; the caller counts it: the norms' n 2^-53 and a handful of 2^-53), and
    rounds the product once more: gl has 3 + 2 roundings relative to r G, plus dr r G.  Then m' has one more (6 + dr),
    u one more with Nesterov, lr_s * u and the subtraction two more: 9 relative to W = |w| + lr_s U for w' (7 + 2) and 6
    relative to M for m' (4 + 2).  The errors Ew, Em of the inputs are carried as in group_ref.TorchBound with the decay
    term scaled by r: Emi = mu Em + r wd_s Ew.  The ratio also depends on w through its norm a, and the two sides hold
    different w: | |w32| - |w64| | <= |Ew|_2 over the tensor, and r = eta a / (b + wd_s a + eps) rises with a no faster
    than in proportion (d log r / d log a = (b + eps) / den <= 1; the clip's division is a constant factor and its
    minimum does not stretch distances), so ratio_slack() gives dr = |Ew|_2 / a plus n 2^-53 for the order of each of
    the two fp64 sums of n non-negative terms and 16 * 2^-53 for the dozen fp64 operations of the rule on both sides."""

    def ratio_slack(self, w, seg_off):
        """dr per element for the step about to be taken, from the errors carried so far (w: the fp64 values)."""
        off = np.asarray(seg_off, dtype=np.int64)
        w = np.asarray(w, dtype=np.float64)
        out = np.zeros(len(off) - 1)
        for s in range(len(off) - 1):
            sl = slice(int(off[s]), int(off[s + 1]))
            a = float(np.sqrt(np.sum(w[sl] ** 2)))
            n = sl.stop - sl.start
            out[s] = (float(np.sqrt(np.sum(self.ew[sl] ** 2))) / a if a > 0 else 0.0) + (2 * n + 16) * 2.0 ** -53
        return group_ref.per_element(out, off)

    def __init__(self, n):
        self.ew = np.zeros(n, np.float64)
        self.em = np.zeros(n, np.float64)

    def step(self, w, g, m, coef, lr_s, wd_s, r, dr, mu, gs, first, nesterov):
        w, g, m, lr_s, wd_s, r, dr = (np.asarray(v, dtype=np.float64) for v in (w, g, m, lr_s, wd_s, r, dr))
        mu = float(F32(mu))
        T = np.abs(g * float(F32(coef)) * float(F32(gs)))
        G = r * (np.abs(wd_s * w) + T)
        M = G if first else mu * np.abs(m) + G
        U = mu * M + G if nesterov else M
        W = np.abs(w) + lr_s * U
        k = 1.0 + 2.0 ** -20
        eg = r * wd_s * self.ew + dr * G * k                 # what the inputs' errors and the ratio's make of gl
        emi = eg if first else mu * self.em + eg
        eu = mu * emi + eg if nesterov else emi
        self.ew = self.ew + lr_s * eu + 9 * EPS * W * k
        self.em = emi + 6 * EPS * M * k
        return self.ew, self.em
