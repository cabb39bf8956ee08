"""What tests/test_pbn_host.py and tests/test_pbn_gpu.py share: the grid of the precise-BN tests, the pool of input lists
(so that the Fraction bound can be shown for every list the tests use) and the CPU twin's buffers inside guard bands."""
import numpy as np

from tests import guard_cases as gc
from tests import pbn_ref
from x3dhip import stepops

CHANNELS = [1, 2, 3, 24, 63, 64, 65, 255, 256, 257, 432]      # around a wave, around a run of 256, two runs and a rest
SPLITS = [1, 2, 3, 8]
BATCHES = [1, 2, 5]
RANKS = [1, 2, 3]
KINDS = ("normal", "hard")
COLUMNS = 8
MAX_CELLS = 8 * (5 + 7)                                        # S = 8, W = 3: batches 5 + 0 + 7


def rank_batches(K, W):
    """Batches per rank: unequal counts, and with three ranks an empty one in the middle."""
    return {1: [K], 2: [K, K + 1], 3: [K, 0, K + 2]}[W]


def _pool(kind):
    rng = np.random.default_rng(7 if kind == "normal" else 8)
    if kind == "normal":
        mu = rng.standard_normal((MAX_CELLS, COLUMNS)) * np.array([1, 1, 10, 0.1, 1, 3, 1, 100.0]) + np.arange(COLUMNS) - 3
        v = rng.chisquare(6, (MAX_CELLS, COLUMNS)) / 6 * np.array([1, 0.01, 5, 1, 1e-3, 1, 30, 1.0])
    else:      # cell means 1000 +- 1e-3 with variances near 1e-6: the between-cell term is as large as the within-cell one
        mu = 1000.0 + rng.uniform(-1e-3, 1e-3, (MAX_CELLS, COLUMNS))
        v = 1e-6 * rng.uniform(0.5, 1.5, (MAX_CELLS, COLUMNS))
    return mu.astype(np.float32), v.astype(np.float32)


POOL = {k: _pool(k) for k in KINDS}


def column(layer, c):
    return (layer + c) % COLUMNS


def cell(kind, layer, C, i):
    """Cell i of a layer with C channels: (mu32 [C], v32 [C]); channel c reads column (layer + c) mod COLUMNS, row i."""
    mu, v = POOL[kind]
    cols = (layer + np.arange(C)) % COLUMNS
    return mu[i, cols].copy(), v[i, cols].copy()


class HostPbn:
    """Per layer (C, S) a means' and a variances' buffer inside guard bands, buffer b (b + rot) mod 4 elements off the
    16-byte grid, their keep table, the layer and work tables, and a snapshot of the keep table's layout inside guard bands
    of its own, filled with a value no statistic takes."""
    SNAP_FILL = -3.5

    def __init__(self, shapes, rot=0):
        self.shapes = list(shapes)
        pairs = []
        for l, (C, S) in enumerate(self.shapes):
            pairs += [gc.banded(C * S, (2 * l + rot) % 4), gc.banded(C * S, (2 * l + 1 + rot) % 4)]
        self.bigs, self.live = [p[0] for p in pairs], [p[1] for p in pairs]
        for b in self.live:
            b[:] = 0.0
        self.kt = stepops.KeepTable(self.live)
        self.pt = stepops.PbnTable(self.kt, [S for _, S in self.shapes])
        self.sbig, self.snap = gc.banded(self.kt.snap_n, 0)
        self.snap[:] = self.SNAP_FILL

    def offsets(self):
        return [int(o) for o in self.kt.table["offset"]]

    def load_batch(self, kind, first_cell):
        """What a momentum-1 pass leaves: split j of the batch is cell first_cell + j.  Returns the cells per layer."""
        out = []
        for l, (C, S) in enumerate(self.shapes):
            cells = [cell(kind, l, C, first_cell + j) for j in range(S)]
            self.live[2 * l][:] = np.concatenate([m for m, _ in cells])
            self.live[2 * l + 1][:] = np.concatenate([v for _, v in cells])
            out.append(cells)
        return out

    def run(self, kind, K, W):
        """The twin over W ranks with rank_batches(K, W) batches each.  Returns (acc_all, expect_n, the cells of every
        layer per rank); the snapshot is left for the caller's finish."""
        S = self.shapes[0][1]
        acc_all = self.pt.new_acc(W).reshape(W, -1)
        per_layer = [[[] for _ in range(W)] for _ in self.shapes]
        at = 0
        for r, kb in enumerate(rank_batches(K, W)):
            acc = self.pt.new_acc()
            for _ in range(kb):
                cells = self.load_batch(kind, at)
                at += S
                stepops.pbn_accum_host(self.pt, acc)
                for l, cs in enumerate(cells):
                    per_layer[l][r] += cs
            acc_all[r] = acc
        return acc_all.reshape(-1), at, per_layer

    def expected_snap(self, per_layer, expect_n, before):
        """The restatement's snapshot: `before` with the pooled values in all S slots of every layer's two buffers."""
        want = before.copy()
        offs = self.offsets()
        for l, (C, S) in enumerate(self.shapes):
            m32, v32 = pbn_ref.pooled(per_layer[l], expect_n)
            want[offs[2 * l]:offs[2 * l] + C * S] = np.tile(m32, S)
            want[offs[2 * l + 1]:offs[2 * l + 1] + C * S] = np.tile(v32, S)
        return want

    def guards_intact(self):
        ok = bool(np.all(self.sbig[:gc.GUARD] == gc.FILL)) and bool(np.all(self.sbig[gc.GUARD + self.kt.snap_n:] == gc.FILL))
        for big, b in zip(self.bigs, self.live):
            lo = (b.ctypes.data - big.ctypes.data) // 4
            ok = ok and bool(np.all(big[:lo] == gc.FILL)) and bool(np.all(big[lo + b.size:] == gc.FILL))
        return ok


def grid_shapes(S):
    return [(C, S) for C in CHANNELS]
