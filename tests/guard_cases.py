"""What tests/test_guard_host.py and tests/test_guard_gpu.py share: the CPU twin's buffers with guard bands (HostGuard,
HostKeep), the hyper-parameter grid and the gradients of the guarded-update tests."""
import itertools

import numpy as np

from tests import step_ref
from x3dhip import _steplib, stepops

GUARD = 64                      # elements on both sides of w, g, m and of every kept buffer
FILL = 7.25
LR = 0.05
KEEP_LENGTHS = [1, 3, 64, 65, 2049]

# first x grad_scale x weight_decay x momentum x (coefficient 1 | below 1)
ARITH = [dict(first=f, gs=gs, wd=wd, mu=mu, clipped=c)
         for f, gs, wd, mu, c in itertools.product((0, 1), (1.0, 0.5), (0.0, 5e-5), (0.0, 0.9), (False, True))]


def arith_id(a):
    return "first%d-gs%g-wd%g-mu%g-%s" % (a["first"], a["gs"], a["wd"], a["mu"], "clipped" if a["clipped"] else "coef1")


def normals(n, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(n) * scale).astype(np.float32)


def eights(n, seed):
    """Every element +-8: over 16384 elements the norm is 1024 exactly, and max_norm 512 gives the coefficient 0.5
    (the perfect-square case of tests/test_step_host.py)."""
    return np.where(np.random.default_rng(seed).integers(0, 2, n) == 1, 8.0, -8.0).astype(np.float32)


def gradient_for(a, n, seed):
    """(g, max_norm) of an arithmetic case."""
    if a["clipped"]:
        assert n == 16384
        return eights(n, seed), 512.0
    return normals(n, seed), 0.0


def banded(n, shift):
    """(big, view): a float32 [n] view `shift` elements off the 16-byte grid inside a buffer filled with FILL."""
    big = stepops.aligned_bytes(4 * (GUARD + shift + n + GUARD)).view(np.float32)
    big[:] = FILL
    view = big[GUARD + shift:GUARD + shift + n]
    assert view.ctypes.data % 16 == 4 * (shift % 4)
    return big, view


class HostGuard:
    """The twin's buffers for one segment table: w, g and m inside guard bands at the given element shifts."""

    def __init__(self, seg_off, R=4, shifts=(0, 0, 0)):
        self.t = stepops.StepTables(seg_off)
        self.R = R
        self.shifts = shifts
        self.state = stepops.new_state()
        self.ws = stepops.aligned_bytes(self.t.workspace_bytes)
        self.ring = stepops.aligned_bytes(R * self.t.record_bytes)
        (self.wbig, self.w), (self.gbig, self.g), (self.mbig, self.m) = (banded(self.t.n, s) for s in shifts)

    def load(self, w=None, g=None, m=None):
        for dst, src in ((self.w, w), (self.g, g), (self.m, m)):
            if src is not None:
                dst[:] = src

    def measure(self, max_norm=0.0, inv_world=1.0):
        stepops.measure_host(self.g, self.t, self.ws, self.state, self.ring, self.R, max_norm, inv_world)

    def apply(self, a, lr=LR):
        stepops.apply_host(self.w, self.g, self.m, self.t, self.state, self.ring, self.R, lr, a["mu"], a["wd"], a["gs"],
                           bool(a["first"]))

    def step(self, g, a, max_norm=0.0, inv_world=1.0, lr=LR):
        self.load(g=g)
        self.measure(max_norm, inv_world)
        self.apply(a, lr)

    def coef(self):
        return self.state[_steplib.S_COEF:_steplib.S_COEF + 1].view(np.float32)[0]

    def words(self):
        return tuple(int(self.state[i]) for i in (_steplib.S_SKIP, _steplib.S_SKIPPED, _steplib.S_RUN))

    def guards_intact(self):
        ok = True
        for big, s in zip((self.wbig, self.gbig, self.mbig), self.shifts):
            lo, hi = GUARD + s, GUARD + s + self.t.n
            ok = ok and bool(np.all(big[:lo] == FILL)) and bool(np.all(big[hi:] == FILL))
        return ok


class HostKeep:
    """Live buffers of the given lengths inside guard bands (buffer b sits b mod 4 elements off the 16-byte grid when
    `stagger`), their keep table and a state."""

    def __init__(self, lengths=KEEP_LENGTHS, stagger=True, seed=0):
        self.lengths = list(lengths)
        pairs = [banded(k, (i % 4) if stagger else 0) for i, k in enumerate(self.lengths)]
        self.bigs, self.live = [p[0] for p in pairs], [p[1] for p in pairs]
        for i, b in enumerate(self.live):
            b[:] = normals(b.size, seed + i)
        self.kt = stepops.KeepTable(self.live)
        self.state = stepops.new_state()

    def offsets(self):
        return [int(o) for o in self.kt.table["offset"]]

    def keep(self, mode):
        stepops.keep_host(self.kt, self.state, mode)

    def guards_intact(self):
        ok = True
        for big, b in zip(self.bigs, self.live):
            lo = (b.ctypes.data - big.ctypes.data) // 4
            ok = ok and bool(np.all(big[:lo] == FILL)) and bool(np.all(big[lo + b.size:] == FILL))
        return ok


def synthetic():
    return step_ref.synthetic_seg_off()
