"""The rules of the precise BN statistics (include/x3dstep.h: cell, merge, result), restated operation by operation in numpy
fp64 over a vector of channels, and the exact pooled value in rationals.  tests/test_pbn_host.py holds the library's CPU twin
to this byte for byte; the GPU tests hold the kernels to the twin."""
from fractions import Fraction

import numpy as np


def new_acc(channels):
    """{n, mean, m2, vsum} per channel, all zero: float64 [channels, 4]."""
    return np.zeros((channels, 4), dtype=np.float64)


def cell_rule(acc, mu32, v32):
    """One cell for every channel: acc float64 [C, 4] is updated in place; mu32 / v32 float32 [C]."""
    with np.errstate(all="ignore"):
        mu = mu32.astype(np.float64)
        v = v32.astype(np.float64)
        n, mean, m2, vsum = acc[:, 0].copy(), acc[:, 1].copy(), acc[:, 2].copy(), acc[:, 3].copy()
        n1 = n + 1.0
        d = mu - mean
        q = d / n1
        mean1 = mean + q
        r = mu - mean1
        p = d * r
        acc[:, 0], acc[:, 1], acc[:, 2], acc[:, 3] = n1, mean1, m2 + p, vsum + v


def merge_rule(a, b):
    """A then B, per channel: returns the merged float64 [C, 4]."""
    with np.errstate(all="ignore"):
        nA, meanA, m2A, vsA = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
        nB, meanB, m2B, vsB = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
        n = nA + nB
        d = meanB - meanA
        f = nB / n
        t = d * f
        dd = d * d
        ab = nA * nB
        g = ab / n
        u = dd * g
        s = m2A + m2B
        out = np.stack([n, meanA + t, s + u, vsA + vsB], axis=1)
        keep_a = nB == 0.0
        take_b = (nA == 0.0) & ~keep_a
        out[keep_a] = a[keep_a]
        out[take_b] = b[take_b]
        return out


def result_rule(acc, expect_n):
    """(mean32, var32) float32 [C]: NaN in both where the count is not expect_n."""
    with np.errstate(all="ignore"):
        s = acc[:, 3] + acc[:, 2]
        mean32 = acc[:, 1].astype(np.float32)
        var32 = (s / acc[:, 0]).astype(np.float32)
        bad = ~(acc[:, 0] == float(expect_n))
        mean32[bad] = np.float32(np.nan)
        var32[bad] = np.float32(np.nan)
        return mean32, var32


def pooled(ranks, expect_n):
    """ranks: per rank a list of cells (mu32 [C], v32 [C]) in the order the rank met them.  Returns (mean32, var32)."""
    C = None
    accs = []
    for cells in ranks:
        for mu, _ in cells:
            C = mu.size
    for cells in ranks:
        a = new_acc(C)
        for mu, v in cells:
            cell_rule(a, mu, v)
        accs.append(a)
    total = accs[0]
    for b in accs[1:]:
        total = merge_rule(total, b)
    return result_rule(total, expect_n)


# -- the exact value ------------------------------------------------------------------------------------------------------------
def exact_pooled(mus, vs):
    """mean = sum mu / n and var = sum v / n + sum (mu - mean)^2 / n of one channel's cells, as Fractions."""
    n = len(mus)
    fm = [Fraction(float(x)) for x in mus]
    fv = [Fraction(float(x)) for x in vs]
    mean = sum(fm) / n
    var = sum(fv) / n + sum((x - mean) ** 2 for x in fm) / n
    return mean, var


def round32(x):
    """A Fraction rounded once to the nearest float32 (no detour through a correctly rounded double)."""
    c = np.float32(float(x))
    best = c
    for cand in (np.nextafter(c, np.float32(-np.inf)), np.nextafter(c, np.float32(np.inf))):
        if abs(Fraction(float(cand)) - x) < abs(Fraction(float(best)) - x):
            best = cand
    return np.float32(best)


def ulps32(a, b):
    """The distance of two finite float32 values in units in the last place (of the ordered integer line)."""
    def key(x):
        i = int(np.float32(x).view(np.int32))
        return i if i >= 0 else -(i & 0x7fffffff)
    return abs(key(a) - key(b))
