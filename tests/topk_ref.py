"""numpy fp64 restatement of the top-k classification meter (include/x3deval.h, csrc_eval/topk.hip): the rows of
x3deval_cls_append_crops and the totals of x3deval_cls_value, plus the seeded cases that the host and GPU tests share."""
import numpy as np

# (b, n_crops, K) per add; the append workgroup strides K by 256 and the crops by 4 waves: K below / equal to / not a
# multiple of the stride, one crop, fewer crops than waves, more, and the limits (32 crops, 4096 classes)
CASES = {
    "1x1x2": [(1, 1, 2)],
    "3x3x7": [(3, 3, 7)],
    "5x1x157": [(5, 1, 157)],
    "2x2x256": [(2, 2, 256)],
    "64x3x400": [(64, 3, 400)],
    "37x10x400": [(37, 10, 400)],
    "2x32x4096": [(2, 32, 4096)],
    "300x1x400_two_adds": [(300, 1, 400), (41, 1, 400)],
}
# seeds chosen by tests/test_topk_host.py's conditions (margin >= 1e-5, counts strictly inside (0, rows))
SEEDS = {"1x1x2": 0, "3x3x7": 0, "5x1x157": 0, "2x2x256": 0, "64x3x400": 0, "37x10x400": 0, "2x32x4096": 1,
         "300x1x400_two_adds": 0}
MIN_GAP = 1e-5


def make_case(name):
    """[(logits fp32 [b * n, K], labels int64 [b], n)] per add.  The label's logit is boosted on about half the videos so
    that hits and misses both occur."""
    rng = np.random.RandomState(1000 + SEEDS[name] + 7919 * sorted(CASES).index(name))
    adds = []
    for b, n, K in CASES[name]:
        z = rng.standard_normal((b, n, K)).astype(np.float32) * 2.0
        y = rng.randint(0, K, size=b).astype(np.int64)
        boost = rng.uniform(0.0, 6.0, size=b).astype(np.float32) * (rng.uniform(size=b) < 0.6)
        z[np.arange(b), :, y] += boost[:, None]
        adds.append((z.reshape(b * n, K), y, n))
    return adds


def rows(logits, labels, n_crops):
    """The rows of one append in fp64 from the fp32 logits: dict of loss (fp64, unrounded), rank, pred, label, batch_rows."""
    logits = np.asarray(logits)
    assert logits.dtype == np.float32
    K = logits.shape[1]
    z = logits.astype(np.float64).reshape(-1, n_crops, K)
    b = z.shape[0]
    labels = np.asarray(labels).astype(np.int64).reshape(b)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        e = np.exp(z - z.max(2, keepdims=True))
        s = (e / e.sum(2, keepdims=True)).mean(1)                     # [b, K]
        m = z.mean(1)
        mmax = m.max(1, keepdims=True)
        lse = mmax[:, 0] + np.log(np.exp(m - mmax).sum(1))
    out = {"loss": np.full(b, np.nan), "rank": np.full(b, K, np.int32), "pred": np.full(b, -1, np.int32),
           "label": np.clip(labels, -1, 2 ** 31 - 1).astype(np.int32), "batch_rows": np.full(b, b, np.int32)}
    for i in range(b):
        y = int(labels[i])
        ok = 0 <= y < K
        sl = s[i, y] if ok else s[i, 0]
        if not np.isnan(sl):
            out["pred"][i] = int(np.argmax(s[i]))                    # the first of the largest
        if ok:
            with np.errstate(invalid="ignore"):
                out["loss"][i] = lse[i] - m[i, y]
            if not np.isnan(sl):
                out["rank"][i] = int((s[i] > sl).sum() + (s[i, :y] == sl).sum())
    return out


def min_relative_gap(logits, labels, n_crops):
    """Over the videos, the smallest |s[k] - s[label]| / s[label] over k != label: how far the counts are from flipping."""
    logits = np.asarray(logits)
    K = logits.shape[1]
    z = logits.astype(np.float64).reshape(-1, n_crops, K)
    e = np.exp(z - z.max(2, keepdims=True))
    s = (e / e.sum(2, keepdims=True)).mean(1)
    gap = np.inf
    for i, y in enumerate(np.asarray(labels).reshape(-1)):
        d = np.abs(s[i] - s[i, y]) / s[i, y]
        d[y] = np.inf
        gap = min(gap, float(d.min()))
    return gap


def totals(all_rows, K, kmax):
    """x3deval_cls_value over the rows of several appends (list of rows() dicts): (totals int64 [4], loss sums fp64 [2],
    class_correct [K], class_count [K]).  The loss of a row is rounded to fp32 first, as the meter stores it."""
    cat = {k: np.concatenate([r[k] for r in all_rows]) for k in all_rows[0]}
    loss = cat["loss"].astype(np.float32).astype(np.float64)
    rank, label = cat["rank"], cat["label"]
    t = np.array([len(rank), int((rank == 0).sum()), int((rank < min(kmax, K)).sum()), len(all_rows)], np.int64)
    ls = np.array([loss.sum(), (loss / cat["batch_rows"]).sum()], np.float64)
    count = np.bincount(label, minlength=K).astype(np.int64)
    correct = np.bincount(label[rank == 0], minlength=K).astype(np.int64)
    return t, ls, correct, count


def value(all_rows, K, kmax):
    """TopKMeter.value() of the rows, as plain numbers."""
    t, ls, correct, count = totals(all_rows, K, kmax)
    with np.errstate(invalid="ignore", divide="ignore"):
        acc = np.where(count > 0, correct / np.maximum(count, 1), np.nan)
    return {"videos": int(t[0]), "top1": t[1] / max(t[0], 1), "top5": t[2] / max(t[0], 1), "cls_loss": ls[1] / max(t[3], 1),
            "loss_per_video": ls[0] / max(t[0], 1), "class_acc": acc, "mean_class_acc": float(np.nanmean(acc))}


def torch_reference(logits, labels, n_crops, dtype):
    """The reference's own expression (train_x3d_kinetics_multigrid.py:253-265) by torch on the CPU in `dtype`:
    (batch-mean loss, top-1 correct count, per-video top-5 hits, predictions)."""
    import torch
    import torch.nn.functional as F
    lg = torch.from_numpy(np.asarray(logits)).to(dtype)
    K = lg.shape[1]
    lg = lg.view(-1, n_crops, K, 1)
    b = lg.shape[0]
    y = torch.from_numpy(np.asarray(labels)).view(b, 1)
    sm = torch.mean(F.softmax(lg, dim=2), 1)
    lgm = torch.mean(lg, 1)
    preds = torch.max(sm, 1)[1]
    loss = float(F.cross_entropy(lgm, y))
    corr = int(torch.sum(preds == y))
    top5 = (sm[:, :, 0].topk(min(5, K), dim=1)[1] == y).any(1).numpy()
    return loss, corr, top5, preds.view(b).numpy()
