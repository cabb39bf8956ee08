"""A numpy restatement of the three rules of include/x3dmix.h, independent of the library: the clips and the targets in fp32
step by step (every product rounded once, every fused multiply-add exact and rounded once: tests/guard_ref.py), the
soft-target cross entropy in fp64."""
import numpy as np

from tests.guard_ref import fma_f32

F32 = np.float32


def resolve(e, b, B, H, W):
    """(partner, mode, box) of plan entry e for sample b: a partner outside the batch is the sample itself; the plan's own
    box decides between CutMix and mixup, and is clipped to the plane before it selects anything."""
    p = int(e["partner"])
    if not 0 <= p < B:
        p = b
    y0, y1, x0, x1 = int(e["y0"]), int(e["y1"]), int(e["x0"]), int(e["x1"])
    if y0 >= y1 or x0 >= x1:
        return p, ("copy" if F32(e["lam"]) == F32(1.0) else "mixup"), None
    return p, "cutmix", (max(y0, 0), min(y1, H), max(x0, 0), min(x1, W))


def mix_clips(x, plan):
    """x float32 [B, planes, H, W] -> the mixed batch."""
    B, _, H, W = x.shape
    out = np.empty_like(x)
    for b in range(B):
        p, mode, box = resolve(plan[b], b, B, H, W)
        if mode == "copy":
            out[b] = x[b]
        elif mode == "mixup":
            lam = F32(plan[b]["lam"])
            om = F32(F32(1.0) - lam)
            out[b] = fma_f32(lam, x[b], (om * x[p]).astype(F32))
        else:
            y0, y1, x0, x1 = box
            out[b] = x[b]
            if y0 < y1 and x0 < x1:
                out[b][:, y0:y1, x0:x1] = x[p][:, y0:y1, x0:x1]
    return out


def mix_clips_fp64(x, plan):
    """(ref, magnitude) of the mixup samples in fp64 from the fp32 lam: lam a + (1 - lam) q and |lam a| + |(1 - lam) q|;
    NaN where the sample is not a mixup."""
    B, _, H, W = x.shape
    ref = np.full(x.shape, np.nan)
    mag = np.full(x.shape, np.nan)
    for b in range(B):
        p, mode, _ = resolve(plan[b], b, B, H, W)
        if mode == "mixup":
            lam = float(F32(plan[b]["lam"]))
            a, q = x[b].astype(np.float64), x[p].astype(np.float64)
            ref[b] = lam * a + (1.0 - lam) * q
            mag[b] = np.abs(lam * a) + np.abs((1.0 - lam) * q)
    return ref, mag


def smooth_rule(smoothing, C):
    off = F32(F32(smoothing) / F32(C))
    on = F32(F32(F32(1.0) - F32(smoothing)) + off)
    return on, off


def targets(labels, plan, C, smoothing):
    """float32 [B, C]: fmaf(lam, s(c, y_b), (1 - lam) * s(c, y_p)); a label outside [0, C) matches no class."""
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    B = labels.size
    on, off = smooth_rule(smoothing, C)
    cls = np.arange(C, dtype=np.int64)
    out = np.empty((B, C), dtype=F32)
    for b in range(B):
        p, _, _ = resolve(plan[b], b, B, 1, 1)
        so = np.where(cls == labels[b], on, off).astype(F32)
        sp = np.where(cls == labels[p], on, off).astype(F32)
        lam = F32(plan[b]["lam"])
        om = F32(F32(1.0) - lam)
        out[b] = fma_f32(lam, so, (om * sp).astype(F32))
    return out


def targets_fp64(labels, plan, C, smoothing):
    """(ref, magnitude) in fp64 from the fp32 lam and smoothing."""
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    B = labels.size
    s = float(F32(smoothing))
    off = s / C
    on = 1.0 - s + off
    cls = np.arange(C, dtype=np.int64)
    ref, mag = np.empty((B, C)), np.empty((B, C))
    for b in range(B):
        p, _, _ = resolve(plan[b], b, B, 1, 1)
        so, sp = np.where(cls == labels[b], on, off), np.where(cls == labels[p], on, off)
        lam = float(F32(plan[b]["lam"]))
        ref[b] = lam * so + (1.0 - lam) * sp
        mag[b] = np.abs(lam * so) + np.abs((1.0 - lam) * sp)
    return ref, mag


def soft_ce(z, t, grad_scale=1.0):
    """(loss, dlogits) in fp64: the mean over the rows of sum_c t_c (lse - z_c), and grad_scale / R (softmax St - t)."""
    z, t = np.asarray(z, dtype=np.float64), np.asarray(t, dtype=np.float64)
    R = z.shape[0]
    m = z.max(axis=1, keepdims=True)
    e = np.exp(z - m)
    s = e.sum(axis=1, keepdims=True)
    lse = m + np.log(s)
    loss = float((t * (lse - z)).sum(axis=1).mean())
    d = (e / s * t.sum(axis=1, keepdims=True) - t) * (float(grad_scale) / R)
    return loss, d
