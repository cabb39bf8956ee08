"""What tests/test_adam_host.py and tests/test_adam_gpu.py share: the case grid of the second-moment updates, the alignment
shifts of four buffers, the CPU twins' buffers with guard bands (HostAdam) and the expectation of one case from the numpy
restatement (tests/adam_ref.py)."""
import itertools

import numpy as np

from tests import adam_ref, group_ref
from tests import group_cases as grc
from tests import guard_cases as gc
from x3dhip import _steplib, stepops

N = grc.N
F32 = np.float32
LR = 0.01
BETAS = (0.9, 0.999)
EPS = {"adam": 1e-8, "lamb": 1e-6}
# w, g, m, v: the four congruent alignments, one that is not, and one in which only w is off (launch 1 of LAMB walks g, m
# and v in 16-byte groups, launch 3 walks w, m and v element by element)
SHIFTS = [(0, 0, 0, 0), (1, 1, 1, 1), (2, 2, 2, 2), (3, 3, 3, 3), (0, 1, 2, 3), (1, 0, 0, 0)]
KS = (1, 2, 10, 1000)

# optimizer / decoupled x grad_scale x weight_decay x (no state | state, coefficient 1 | state, coefficient 0.5) x k
GRID = [dict(opt=o, decoupled=d, gs=gs, wd=wd, state=st, clipped=c, k=k)
        for (o, d), gs, wd, (st, c), k in itertools.product(
            (("adam", 0), ("adam", 1), ("lamb", 1)), (1.0, 0.5), (0.0, 0.01), ((False, False), (True, False), (True, True)), KS)]


def case_id(a):
    return "%s%d-gs%g-wd%g-%s-k%d" % (a["opt"], a["decoupled"], a["gs"], a["wd"],
                                     ("clipped" if a["clipped"] else "coef1") if a["state"] else "nostate", a["k"])


def shift_id(s):
    return "shift%d%d%d%d" % s


def adapts(S):
    """Every fifth tensor is exempt from the adaptation."""
    return np.array([0 if s % 5 == 2 else 1 for s in range(S)], dtype=np.uint8)


def second_moments(n, seed, scale=0.1):
    """A second-moment buffer: squares."""
    x = gc.normals(n, seed, scale)
    return (x * x).astype(F32)


class HostAdam(grc.HostGroup):
    """HostGroup with the second-moment buffer, and for LAMB the adaptation flags, the workspace of the partials and the
    twin's outputs."""

    def __init__(self, seg_off, hyper=None, adapt=None, R=4, shifts=(0, 0, 0, 0)):
        super().__init__(seg_off, hyper=hyper, R=R, shifts=tuple(shifts[:3]))
        self.shifts4 = tuple(shifts)
        self.vbig, self.v = gc.banded(self.t.n, shifts[3])
        self.adapt = adapts(self.t.S) if adapt is None else np.asarray(adapt, dtype=np.uint8)
        self.lws = stepops.aligned_bytes(stepops.lamb_workspace_bytes(self.t.nitems))
        self.wsumsq = np.full(self.t.S, -3.0, dtype=np.float64)
        self.rsumsq = np.full(self.t.S, -3.0, dtype=np.float64)
        self.trust = np.full(self.t.S, -3.0, dtype=np.float32)

    def load(self, w=None, g=None, m=None, v=None):
        super().load(w, g, m)
        if v is not None:
            self.v[:] = v

    def applied(self):
        """The updates applied so far, as the state counts them."""
        return int(self.state[_steplib.S_STEP]) - int(self.state[_steplib.S_SKIPPED])

    def _st(self, state):
        return (self.state, self.ring, self.R) if state else (None, None, 0)

    def adam(self, a, count, lr=LR, state=True):
        stepops.adam_host(self.w, self.g, self.m, self.v, self.t, self.hyper, *self._st(state), count, lr, a.get("betas", BETAS),
                          a.get("eps", EPS["adam"]), a["wd"], a["gs"], a["decoupled"])

    def lamb(self, a, count, lr=LR, state=True):
        betas, eps = a.get("betas", BETAS), a.get("eps", EPS["lamb"])
        st = self._st(state)
        stepops.lamb_moments_host(self.w, self.g, self.m, self.v, self.t, self.hyper, *st, count, self.lws, betas, eps, a["wd"],
                                  a["gs"])
        stepops.lamb_trust_host(self.t, self.hyper, self.adapt, *st, count, self.lws, self.wsumsq, self.rsumsq, self.trust)
        stepops.lamb_apply_host(self.w, self.m, self.v, self.t, self.hyper, self.trust, *st, count, lr, betas, eps, a["wd"])

    def count_for(self, a):
        """The host's count that makes this call update k = a['k'] (after the measure, when there is a state)."""
        return a["k"] - (self.applied() if a["state"] else 0)

    def run(self, a, g, max_norm=0.0, lr=LR):
        """One case of GRID: load g, measure when the case has a state, the update as update k."""
        self.load(g=g)
        if a["state"]:
            self.measure(max_norm)
        (self.lamb if a["opt"] == "lamb" else self.adam)(a, self.count_for(a), lr, state=a["state"])

    def partials(self):
        """(rpart, wpart) fp64 [nitems] of the latest launch 1."""
        p = self.lws[:16 * self.t.nitems].view(np.float64)
        return p[:self.t.nitems], p[self.t.nitems:]

    def guards_intact(self):
        lo, hi = gc.GUARD + self.shifts4[3], gc.GUARD + self.shifts4[3] + self.t.n
        return super().guards_intact() and bool(np.all(self.vbig[:lo] == gc.FILL)) and bool(np.all(self.vbig[hi:] == gc.FILL))


def gradient_for(a, n, seed):
    return grc.gradient_for(a, n, seed)


def per_element(hy, off, lr, wd):
    lr_s, wd_s = group_ref.tensor_rule(lr, wd, hy["lr_scale"], hy["wd_scale"])
    return group_ref.per_element(lr_s, off), group_ref.per_element(wd_s, off)


def expected(a, off, hy, adapt, w, g, m, v, coef, lr=LR, nonfinite=None):
    """What the restatement makes of one case: dict(w, m, v) and for LAMB also r, rsumsq / wsumsq (the correctly rounded
    sums: the twins' own are held against measure_host elsewhere) and a function trust(wsumsq, rsumsq) -> (trust, w')."""
    lr_s, wd_s = per_element(hy, off, lr, a["wd"])
    betas = a.get("betas", BETAS)
    if a["opt"] == "adam":
        w1, m1, v1 = adam_ref.adam_rule(w, g, m, v, coef, lr_s, wd_s, a["k"], betas[0], betas[1], a.get("eps", EPS["adam"]),
                                        a["gs"], a["decoupled"])
        return dict(w=w1, m=m1, v=v1)
    m1, v1, r = adam_ref.lamb_moments(w, g, m, v, coef, wd_s, a["k"], betas[0], betas[1], a.get("eps", EPS["lamb"]), a["gs"])
    nf = np.zeros(len(off) - 1, np.int32) if nonfinite is None else nonfinite

    def finish(wsumsq, rsumsq):
        tr = adam_ref.lamb_trust(wsumsq, rsumsq, adapt, nf)
        return tr, adam_ref.lamb_apply(w, r, lr_s, group_ref.per_element(tr, off))

    return dict(m=m1, v=v1, r=r, finish=finish)
