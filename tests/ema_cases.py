"""What tests/test_ema_host.py and tests/test_ema_gpu.py share: the grids of the weight-average tests, states with a given
count of applied updates, and the CPU twin's kept buffers inside guard bands."""
import numpy as np

from tests import guard_cases as gc
from x3dhip import _steplib, stepops

LENGTHS = [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4095, 4096, 4097]
SHIFTS = [(0, 0), (1, 1), (2, 2), (3, 3), (1, 3)]                 # (e, w): the four congruent alignments, one that is not
DECAYS = [0.0, 0.5, 0.9, 0.9999]
KS = [1, 2, 9, 10, 89991]                                        # (1 + k) / (10 + k) = 0.9999 at k = 89989
KEEP_LENGTHS = [1, 2, 3, 24, 63, 64, 65, 2047, 2048, 2049, 4097]


def state_for(k, count, skipped=3, skip=0):
    """A state whose applied-update count makes count + S_STEP - S_SKIPPED == k."""
    st = stepops.new_state()
    st[_steplib.S_SKIPPED] = skipped
    st[_steplib.S_STEP] = k - count + skipped
    st[_steplib.S_SKIP] = skip
    return st


def counts(k, with_state):
    """(state, count) pairs that all mean update k: no state; a state with a zero, a positive and a negative offset."""
    if not with_state:
        return [(None, k)]
    return [(state_for(k, c), c) for c in (0, 5, -7)]


class HostEmaKeep:
    """Live buffers of the given lengths inside guard bands, buffer b (b + rot) mod 4 elements off the 16-byte grid, their
    keep table, and an averaged snapshot of the table's layout inside guard bands of its own."""

    def __init__(self, lengths=KEEP_LENGTHS, rot=0, seed=0):
        self.lengths = list(lengths)
        pairs = [gc.banded(k, (i + rot) % 4) for i, k in enumerate(self.lengths)]
        self.bigs, self.live = [p[0] for p in pairs], [p[1] for p in pairs]
        for i, b in enumerate(self.live):
            b[:] = gc.normals(b.size, seed + i)
        self.kt = stepops.KeepTable(self.live)
        self.ebig, self.esnap = gc.banded(self.kt.snap_n, 0)
        self.esnap[:] = gc.normals(self.kt.snap_n, seed + 1000)

    def offsets(self):
        return [int(o) for o in self.kt.table["offset"]]

    def guards_intact(self):
        ok = bool(np.all(self.ebig[:gc.GUARD] == gc.FILL)) and bool(np.all(self.ebig[gc.GUARD + self.kt.snap_n:] == gc.FILL))
        for big, b in zip(self.bigs, self.live):
            lo = (b.ctypes.data - big.ctypes.data) // 4
            ok = ok and bool(np.all(big[:lo] == gc.FILL)) and bool(np.all(big[lo + b.size:] == gc.FILL))
        return ok
