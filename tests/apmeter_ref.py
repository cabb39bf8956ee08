"""fp64 numpy restatement of the average precision of apmeter.APMeter (the reference's apmeter.py:98-136) with the
project's tie rule: per class a STABLE descending order (tied scores keep insertion order), -0.0 ties +0.0, NaN ranks
above +inf.  Test infrastructure only (no GPU, no reference checkout)."""
import numpy as np


def descending_order(s):
    """Stable descending order of float scores s [N]: NaN first (in insertion order), then by value, ties in insertion
    order (-0.0 == +0.0)."""
    s = np.asarray(s)
    nan = np.isnan(s)
    neg = np.where(nan, 0.0, -s.astype(np.float64))
    return np.lexsort((neg, (~nan).astype(np.int8)))


def average_precision(scores, targets, weights=None):
    """ap [K] (float64) of scores [N, K], binary targets [N, K] and optional non-negative weights [N]."""
    scores = np.asarray(scores)
    targets = np.asarray(targets)
    if scores.ndim == 1:
        scores, targets = scores.reshape(-1, 1), targets.reshape(-1, 1)
    N, K = scores.shape
    ap = np.zeros(K, dtype=np.float64)
    for k in range(K):
        order = descending_order(scores[:, k])
        truth = targets[order, k].astype(np.float64)
        if weights is None:
            rank = np.arange(1, N + 1, dtype=np.float64)
            tp = np.cumsum(truth)
        else:
            w = np.asarray(weights, dtype=np.float64)[order]
            rank = np.cumsum(w)
            tp = np.cumsum(truth * w)
        with np.errstate(invalid="ignore", divide="ignore"):
            precision = tp / rank
        ap[k] = precision[truth == 1].sum() / max(truth.sum(), 1.0)
    return ap


def _fma32(a, b, c):
    """float32 fma(a, b, c): the fp32 product is exact in fp64, the sum is rounded (twice, which leaves these inputs'
    results exact in practice)."""
    a, b, c = np.broadcast_arrays(np.float64(a) if np.isscalar(a) else np.asarray(a, np.float64), np.asarray(b, np.float64),
                                  np.asarray(c, np.float64))
    return (a * b + c).astype(np.float32)


def interp_linear(x, TL):
    """F.interpolate(x [B, K, T], TL, mode='linear', align_corners=False) in float32 numpy, bit for bit: torch fuses the
    source index fma(scale, t + 0.5, -0.5) and the value fma(l0, x0, l1 * x1); source index clamped at 0, upper tap
    clamped at T - 1."""
    x = np.asarray(x, dtype=np.float32)
    T = x.shape[2]
    scale = np.float32(T) / np.float32(TL)
    src = _fma32(scale, np.arange(TL, dtype=np.float32) + np.float32(0.5), np.float32(-0.5))
    src = np.maximum(src, np.float32(0.0))
    i0 = np.minimum(src.astype(np.int64), T - 1)
    i1 = i0 + (i0 < T - 1)
    l1 = (src - i0.astype(np.float32)).astype(np.float32)
    l0 = (np.float32(1.0) - l1).astype(np.float32)
    return _fma32(l0, x[:, :, i0], (l1 * x[:, :, i1]).astype(np.float32))
