"""What tests/test_lars_host.py and tests/test_lars_gpu.py share: the per-tensor rates of trust, the case grid of the trust
ratios and the CPU twins' buffers with guard bands (HostLars)."""
import itertools

import numpy as np

from tests import group_cases as grc
from tests import guard_cases as gc
from tests import step_ref
from x3dhip import _steplib, stepops

N = grc.N
ETAS = (0.001, 0.0, 0.02, 1.0, 0.5, 0.25, 0.125)     # seven: out of step with the five lr scales and the three wd scales
EPS = 1e-8
# tensors of these lengths as one buffer: around a group of four, around an item, and 70 items and one element, so that a
# tensor's item-order sum spans many items
LENGTHS = [1, 3, 4, 5, 2047, 2048, 2049, 70 * 2048 + 1]


def etas(S):
    """Tensor s takes ETAS[s mod 7]: with grc.scales every tensor of the synthetic table has its own triple."""
    return np.array([ETAS[s % 7] for s in range(S)], dtype=np.float32)


# nesterov x first x grad_scale x weight_decay x clip x (no state for the update | state, coefficient 1 | state, clipped)
GRID = [dict(first=f, nesterov=nv, mu=0.9, gs=gs, wd=wd, clip=cl, state=st, clipped=c)
        for nv, f, gs, wd, cl, (st, c) in itertools.product(
            (0, 1), (0, 1), (1.0, 0.5), (0.0, 5e-5), (0, 1), ((False, False), (True, False), (True, True)))]


def case_id(a):
    return "nest%d-first%d-gs%g-wd%g-clip%d-%s" % (a["nesterov"], a["first"], a["gs"], a["wd"], a["clip"],
                                                  ("clipped" if a["clipped"] else "coef1") if a["state"] else "nostate")


class HostLars(grc.HostGroup):
    """HostGroup with the rates of trust, the twin's outputs wsumsq and trust, and the workspace of the partials."""

    def __init__(self, seg_off, hyper=None, eta=None, R=4, shifts=(0, 0, 0)):
        super().__init__(seg_off, hyper=hyper, R=R, shifts=shifts)
        self.eta = etas(self.t.S) if eta is None else np.asarray(eta, dtype=np.float32)
        self.tws = stepops.aligned_bytes(stepops.trust_workspace_bytes(self.t.nitems))
        self.wsumsq = np.full(self.t.S, -3.0, dtype=np.float64)
        self.trust = np.full(self.t.S, -3.0, dtype=np.float32)

    def trust_host(self, a, lr=gc.LR):
        stepops.trust_host(self.w, self.t, self.hyper, self.eta, self.state, self.ring, self.R, self.tws, self.wsumsq,
                           self.trust, lr, a["wd"], a["gs"], a.get("eps", EPS), a.get("clip", 0))

    def apply_lars(self, a, lr=gc.LR, state=True, trust=None):
        stepops.apply_lars_host(self.w, self.g, self.m, self.t, self.hyper, self.trust if trust is None else trust,
                                self.state if state else None, self.ring if state else None, self.R, lr, a["mu"], a["wd"],
                                a["gs"], a["first"], a.get("nesterov", 0))

    def run(self, a, g, max_norm=0.0, lr=gc.LR):
        """One case of GRID: load g, measure (the trust needs the record whatever the update's form), trust, apply."""
        self.load(g=g)
        self.measure(max_norm)
        self.trust_host(a, lr)
        self.apply_lars(a, lr, state=a["state"])

    def record(self):
        """(header, sumsq, hash, nonfinite) of the latest record."""
        c = int(self.state[_steplib.S_STEP])
        rb = self.t.record_bytes
        slot = (c - 1) % self.R
        return stepops.parse_record(self.ring[slot * rb:(slot + 1) * rb], self.t.S)


def bad_tensor_tables(t):
    """[(name, hyper, eta, seg_item, the tensors left out)]: the tables of StepTables t with one tensor spoilt in each way
    the per-tensor tests of x3dstep_trust name."""
    out = []
    s = 9
    for name, value in (("eta-negative", -0.001), ("eta-nan", np.nan), ("eta-inf", np.inf)):
        e = etas(t.S)
        e[s] = value
        out.append((name, grc.scales(t.S), e, t.seg_item.copy(), [s]))
    for name, field, value in (("lr-scale-nan", "lr_scale", np.nan), ("wd-scale-negative", "wd_scale", -0.5)):
        hy = grc.scales(t.S)
        hy[field][s] = value
        out.append((name, hy, etas(t.S), t.seg_item.copy(), [s]))
    si = t.seg_item.copy()
    si[s + 1] = si[s]                                   # tensor s has no items; tensor s + 1 takes them over
    out.append(("items-empty", grc.scales(t.S), etas(t.S), si, [s]))
    si = t.seg_item.copy()
    si[t.S] = t.nitems + 1
    out.append(("items-past-end", grc.scales(t.S), etas(t.S), si, [t.S - 1]))
    return out


def lengths_seg_off():
    return step_ref.seg_off_of(LENGTHS)
