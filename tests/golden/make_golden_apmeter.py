"""Generate tests/golden/apmeter_cases.npz by running the REFERENCE's own apmeter.APMeter.

Run in the build container only, next to a checkout of the reference (which never travels to the GPU box):

    python tests/golden/make_golden_apmeter.py --reference DIR

Cases (every one free of score ties, where the reference's unstable CPU sort would leave the value undefined):
  rand_*     random scores over several adds, N from 1 to 3000, K up to 157
  weighted   random weights
  nopos      one class without positives
  cls_crops  10-crop logits through train_x3d_charades.py:165-175 (sigmoid, max over crops)
  loc_frames per-frame logits, labels and masks through train_x3d_charades_loc.py:165-186 (interpolate, sigmoid * mask,
             per-sample slices of the valid frames); one sample with no valid frame
Logits are drawn on a grid with gaps of at least 1e-3, and a draw is kept only if the scores the reference adds keep gaps
of many ulps, so that an ulp of difference in the sigmoid cannot reorder them.
For each case the npz holds the adds' inputs and the reference's ap."""
import argparse
import importlib.util
import os
import sys
import warnings

import numpy as np
import torch
import torch.nn.functional as F

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "apmeter_cases.npz")


def _load_reference(ref):
    sys.path.insert(0, ref)                 # apmeter.py imports the reference's meter.py
    spec = importlib.util.spec_from_file_location("ref_apmeter", os.path.join(ref, "apmeter.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _tie_free(rows, min_rel=1e-6):
    """True when every column of rows [N, K] has pairwise distinct values with relative gaps above min_rel."""
    for k in range(rows.shape[1]):
        s = np.sort(rows[:, k].astype(np.float64))
        if len(s) > 1 and np.any(np.diff(s) <= min_rel * np.maximum(np.abs(s[1:]), 1e-3)):
            return False
    return True


def _grid_logits(g, rows, K, lo=-4.0, step=1e-3):
    """[rows, K] logits, each column drawn without replacement from the grid lo + step * i (i < 8 / step)."""
    idx = np.stack([g.choice(int(8.0 / step), size=rows, replace=False) for _ in range(K)], 1)
    return (lo + step * idx).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference (holds apmeter.py, meter.py)")
    args = ap.parse_args()
    warnings.simplefilter("ignore")
    ref = _load_reference(args.reference)
    g = np.random.default_rng(20261016)
    out, names = {}, []

    def run(name, adds, weighted=False):
        m = ref.APMeter()
        for i, a in enumerate(adds):
            m.add(a["scores"], a["targets"], a.get("weights"))
            out["%s__add%d_scores" % (name, i)] = a["scores"].astype(np.float32)
            out["%s__add%d_targets" % (name, i)] = a["targets"].astype(np.uint8)
            if weighted:
                out["%s__add%d_weights" % (name, i)] = a["weights"].astype(np.float32)
        allrows = np.concatenate([a["scores"] for a in adds], 0)
        assert _tie_free(allrows, 0.0), name          # stored as given: only exact ties matter
        out["%s__ap" % name] = m.value().numpy().astype(np.float32)
        out["%s__nadds" % name] = np.array(len(adds))
        names.append(name)

    def rand_adds(sizes, K, p=0.2):
        # per class distinct multiples of 2^-24 in [0, 1) (exact in float32), split over the adds
        s = np.stack([g.choice(1 << 24, size=sum(sizes), replace=False) for _ in range(K)], 1) / float(1 << 24)
        parts = np.split(s.astype(np.float32), np.cumsum(sizes)[:-1], 0)
        return [{"scores": x, "targets": (g.random(x.shape) < p).astype(np.int64)} for x in parts]

    run("rand_n1", rand_adds([1], 4))
    run("rand_tiny", rand_adds([2, 1, 4], 3, 0.5))
    run("rand_k157", rand_adds([90, 60, 50], 157))
    run("rand_n3000", rand_adds([1000, 1500, 500], 8, 0.05))
    run("rand_n700", rand_adds([64, 63, 65, 508], 5, 0.3))
    wadds = rand_adds([300, 200, 100], 12)
    for a in wadds:
        a["weights"] = (0.1 + 1.9 * g.random(a["scores"].shape[0])).astype(np.float32)
    run("weighted", wadds, weighted=True)
    nadds = rand_adds([120, 80], 10)
    for a in nadds:
        a["targets"][:, 3] = 0
    run("nopos", nadds)

    # cls: 10-crop logits -> max over crops of the sigmoid (train_x3d_charades.py:165-175)
    K, b, n = 157, 6, 10
    while True:
        m = ref.APMeter()
        logits = np.split(_grid_logits(g, 3 * b * n, K), 3, 0)
        labels = [(g.random((b, K)) < 0.1).astype(np.float32) for _ in range(3)]
        probs = []
        for z, y in zip(logits, labels):
            p = torch.max(F.sigmoid(torch.from_numpy(z).view(b, n, K)), dim=1)[0]
            probs.append(p.numpy())
            m.add(p.numpy(), y)
        if _tie_free(np.concatenate(probs, 0)):
            break
    for i in range(3):
        out["cls_crops__add%d_logits" % i] = logits[i]
        out["cls_crops__add%d_targets" % i] = labels[i].astype(np.uint8)
    out["cls_crops__n_crops"] = np.array(n)
    out["cls_crops__ap"] = m.value().numpy().astype(np.float32)
    out["cls_crops__nadds"] = np.array(3)
    names.append("cls_crops")

    # loc: per-frame logits -> interpolate to TL, sigmoid * mask, per-sample valid slices (train_x3d_charades_loc.py:165-186)
    B, T, TL = 4, 8, 20
    while True:
        m = ref.APMeter()
        batches, rows = [], []
        for _ in range(3):
            z = np.ascontiguousarray(_grid_logits(g, B * T, K).reshape(B, T, K).transpose(0, 2, 1))
            y = (g.random((B, K, TL)) < 0.1).astype(np.float32)
            valid = g.integers(1, TL + 1, size=B)
            valid[1] = 0 if not batches else valid[1]            # a sample without a valid frame in the first batch
            masks = (np.arange(TL)[None, :] < valid[:, None]).astype(np.float32)
            batches.append((z, y, masks))
            pfl = F.interpolate(torch.from_numpy(z), TL, mode='linear')
            probs = F.sigmoid(pfl) * torch.from_numpy(masks).unsqueeze(1)
            labels_t = torch.from_numpy(y)
            valid_t = torch.sum(torch.from_numpy(masks), dim=1).int()
            for bb in range(B):
                r = probs[bb][:, :valid_t[bb].item()].transpose(0, 1).numpy()
                m.add(r, labels_t[bb][:, :valid_t[bb].item()].transpose(0, 1).numpy())
                rows.append(r)
        if _tie_free(np.concatenate(rows, 0)):
            break
    for i, (z, y, masks) in enumerate(batches):
        out["loc_frames__add%d_logits" % i] = z
        out["loc_frames__add%d_labels" % i] = y.astype(np.uint8)
        out["loc_frames__add%d_masks" % i] = masks
    out["loc_frames__ap"] = m.value().numpy().astype(np.float32)
    out["loc_frames__nadds"] = np.array(3)
    names.append("loc_frames")

    out["cases"] = np.array(names)
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes): %s" % (OUT, os.path.getsize(OUT), names))


if __name__ == "__main__":
    main()
