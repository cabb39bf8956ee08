"""Hand-built cases of the mixing library's tests (host and GPU): clip shapes, plans that reach every branch of the clip rule
with no random draw deciding the coverage, label sets and the logits / soft targets of the cross-entropy checks."""
import numpy as np

from x3dhip._mixlib import SAMPLE_DT

F32 = np.float32

# (B, planes, H, W): one element with itself as partner; an odd clip (105 floats: clip 1 starts 4-byte aligned); the 79 x 79
# multigrid crop (6 * 6241 floats, not a multiple of 4); a multiple of everything; a small one; a 158-wide row (not a multiple
# of 4 floats)
CLIP_SHAPES = [(1, 1, 1, 1), (2, 3, 5, 7), (3, 6, 79, 79), (4, 12, 16, 16), (3, 3, 6, 10), (2, 3, 4, 158)]
# more than one pass of the clip kernel's grid needs more than 1024 runs of 4096 floats: see tests/test_mix_gpu.py
BIG_SHAPE = (8, 12, 64, 64)

LAMS = [1.0, 0.0, 0.25, 0.3]


def normals(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(F32)


def make_plan(B, partner=None, lam=1.0, box=None):
    """A plan of B entries: partner an int array (default: the next sample), lam a scalar or [B], box (y0, y1, x0, x1) for
    every sample or a list of B boxes (None: empty)."""
    plan = np.zeros(B, dtype=SAMPLE_DT)
    plan["partner"] = (np.arange(B) + 1) % B if partner is None else np.asarray(partner, dtype=np.int32)
    plan["lam"] = np.broadcast_to(np.asarray(lam, dtype=F32), (B,))
    if box is not None:
        boxes = [box] * B if isinstance(box[0], (int, np.integer)) else list(box)
        for b, bx in enumerate(boxes):
            if bx is not None:
                plan["y0"][b], plan["y1"][b], plan["x0"][b], plan["x1"][b] = bx
    return plan


def plans(B, H, W):
    """name -> plan for clips of B samples with H x W planes."""
    out = {}
    idx = np.arange(B)
    out["mixup_every_lam"] = make_plan(B, lam=[LAMS[b % 4] for b in range(B)])
    for lam in LAMS:
        out["mixup_lam_%g" % lam] = make_plan(B, lam=lam)
    out["self_partner_lam_0.3"] = make_plan(B, partner=idx, lam=0.3)
    if B >= 3:
        out["three_cycle"] = make_plan(B, partner=[1, 2, 0] + list(range(3, B)), lam=0.25)
    out["full_plane_box"] = make_plan(B, lam=0.0, box=(0, H, 0, W))
    corners = [(0, 1, 0, 1), (0, 1, W - 1, W), (H - 1, H, 0, 1), (H - 1, H, W - 1, W)]
    for k, c in enumerate(corners):
        out["corner_%d" % k] = make_plan(B, lam=0.9, box=c)
    out["corners_by_sample"] = make_plan(B, lam=0.9, box=[corners[b % 4] for b in range(B)])
    if W >= 6:
        out["odd_x0_width_5"] = make_plan(B, lam=0.5, box=(min(1, H - 1), H, 1, 6))
    out["touches_top"] = make_plan(B, lam=0.5, box=(0, max(1, H // 2), W // 3, max(W // 3 + 1, 2 * W // 3)))
    out["touches_bottom"] = make_plan(B, lam=0.5, box=(H // 2, H, W // 3, max(W // 3 + 1, 2 * W // 3)))
    out["touches_left"] = make_plan(B, lam=0.5, box=(H // 3, max(H // 3 + 1, 2 * H // 3), 0, max(1, W // 2)))
    out["touches_right"] = make_plan(B, lam=0.5, box=(H // 3, max(H // 3 + 1, 2 * H // 3), W // 2, W))
    # a copy, a mixup and a CutMix in one batch; a plan nobody should write: partners outside the batch (taken as the sample
    # itself) and boxes that reach outside the plane (clipped)
    modes = [None, None, (0, max(1, H - 1), 0, max(1, W - 1))]
    out["modes_by_sample"] = make_plan(B, lam=[[1.0, 0.75, 0.6][b % 3] for b in range(B)], box=[modes[b % 3] for b in range(B)])
    out["hostile"] = make_plan(B, partner=[-1 if b % 2 == 0 else B + 5 for b in range(B)], lam=0.3,
                               box=[(-3, H + 7, W // 2, W + 9) if b % 2 == 0 else (H + 2, H + 5, 0, 1) for b in range(B)])
    return out


def clip_cases():
    """[(name, x float32 [B, planes, H, W], plan)] over every shape and plan."""
    out = []
    for si, (B, P, H, W) in enumerate(CLIP_SHAPES):
        x = normals((B, P, H, W), 100 + si)
        for name, plan in plans(B, H, W).items():
            out.append(("%dx%dx%dx%d-%s" % (B, P, H, W, name), x, plan))
    return out


def nan_cases():
    """[(name, x, plan, expected)]: CutMix with the partner NaN outside the box and the sample NaN inside it (expected: finite,
    given bits), and lam == 1 with a NaN partner (a bit copy)."""
    out = []
    for si, (B, P, H, W) in enumerate([(2, 3, 5, 7), (3, 6, 79, 79), (2, 3, 4, 158)]):
        y0, y1, x0, x1 = H // 4, max(H // 4 + 1, 3 * H // 4), 1, max(2, W - 2)
        inside = np.zeros((H, W), dtype=bool)
        inside[y0:y1, x0:x1] = True
        own, other = normals((P, H, W), 200 + si), normals((P, H, W), 300 + si)
        x = np.empty((B, P, H, W), dtype=F32)
        x[0] = np.where(inside, F32(np.nan), own)            # sample 0: NaN where its partner shows
        x[1:] = np.where(inside, other, F32(np.nan))         # the partners: NaN where they do not
        plan = make_plan(B, partner=[1] + [b for b in range(1, B)], lam=0.5,
                         box=[(y0, y1, x0, x1)] + [None] * (B - 1))
        plan["lam"][1:] = 1.0                                 # the others: copies of clips that hold NaN
        expected = x.copy()
        expected[0] = np.where(inside, other, own)
        out.append(("nan-cutmix-%dx%dx%dx%d" % (B, P, H, W), x, plan, expected))
        xc = normals((B, P, H, W), 400 + si)
        xc[B - 1] = np.nan
        planc = make_plan(B, partner=[B - 1] * B, lam=1.0)    # every sample's partner is the NaN clip, and nobody reads it
        out.append(("nan-copy-%dx%dx%dx%d" % (B, P, H, W), xc, planc, xc.copy()))
    return out


# -- targets -----------------------------------------------------------------------------------------------------------------
TARGET_CLASSES = [1, 7, 157, 400]
SMOOTHINGS = [0.0, 0.1]


def target_cases():
    """[(name, labels int64 [B], plan, C, smoothing)]; the labels hold the first and the last class and two outside [0, C)."""
    out = []
    B = 6
    for C in TARGET_CLASSES:
        labels = np.array([0, C - 1, C // 2, -1, C, min(3, C - 1)], dtype=np.int64)
        for sm in SMOOTHINGS:
            for name, plan in (("identity", make_plan(B, partner=np.arange(B), lam=1.0)),
                               ("lams", make_plan(B, lam=[LAMS[b % 4] for b in range(B)])),
                               ("lam_0.3_cycle", make_plan(B, partner=[1, 2, 0, 4, 5, 3], lam=0.3)),
                               ("hostile", make_plan(B, partner=[-1, 99, 2, 0, 1, -7], lam=0.75, box=(0, 1, 0, 1)))):
                out.append(("C%d-s%g-%s" % (C, sm, name), labels, plan, C, sm))
    return out


# -- the soft-target cross entropy -----------------------------------------------------------------------------------------------
CE_SHAPES = [(1, 1), (1, 7), (3, 157), (8, 400), (70, 10), (5, 257), (2, 1025)]
CE_LAMS = [1.0, 0.75, 0.3]
CE_SCALES = [1.0, 0.25]
SATURATED = [100.0, -100.0, 90.0, -95.5, 60.0, -37.0]


def ce_logits(R, C, seed, saturated=True):
    """z = 4 randn with one eighth of the entries at +-100, 90, -95.5, 60, -37; saturated=False: plain randn."""
    rng = np.random.default_rng(seed)
    if not saturated:
        return rng.standard_normal((R, C)).astype(F32)
    z = (4.0 * rng.standard_normal((R, C))).astype(F32)
    flat = z.reshape(-1)
    hit = np.flatnonzero(rng.random(flat.size) < 0.125)
    flat[hit] = np.asarray(SATURATED, dtype=F32)[np.arange(hit.size) % len(SATURATED)]
    return z


def ce_targets(R, C, lam, smoothing, seed):
    """Soft targets as the mixer builds them, by plain fp32 numpy: lam of the row's smoothed one-hot and 1 - lam of the next
    row's.  (What they are exactly does not matter to the loss's tests: they are its input.)"""
    rng = np.random.default_rng(seed)
    y = rng.integers(0, C, size=R)
    off = F32(smoothing) / F32(C)
    on = F32(1.0) - F32(smoothing) + off
    s = np.full((R, C), off, dtype=F32)
    s[np.arange(R), y] = on
    return (F32(lam) * s + (F32(1.0) - F32(lam)) * np.roll(s, -1, axis=0)).astype(F32)


def ce_cases():
    """[(name, z, t, grad_scale)]"""
    out = []
    k = 0
    for (R, C) in CE_SHAPES:
        for lam in CE_LAMS:
            for sm in SMOOTHINGS:
                for gs in CE_SCALES:
                    k += 1
                    out.append(("R%d-C%d-lam%g-s%g-gs%g" % (R, C, lam, sm, gs), ce_logits(R, C, 500 + k),
                                ce_targets(R, C, lam, sm, 600 + k), gs))
    out.append(("unsaturated-R8-C400", ce_logits(8, 400, 700, saturated=False), ce_targets(8, 400, 0.75, 0.1, 701), 1.0))
    out.append(("unsaturated-R8-C400-gs0.25", ce_logits(8, 400, 702, saturated=False), ce_targets(8, 400, 0.3, 0.0, 703), 0.25))
    return out
