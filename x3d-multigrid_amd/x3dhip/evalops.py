"""Tensor-level wrappers over the evaluation C ABI (include/x3deval.h), in the style of ops.py.

Shapes, dtypes and devices are checked here, on the host, before anything is launched; values (targets that are not
0 / 1, negative weights) are checked by the kernels, which set a sticky flag in the meter's device state instead of
synchronising.  Every launch goes to the current stream.  There is no fallback: a CPU tensor raises.
"""
import torch

from . import _evallib
from ._evallib import check
from ._lib import X3DHipError, ptr, stream


def _need(name, t, dtype, dim=None):
    if not isinstance(t, torch.Tensor):
        raise X3DHipError("%s: expected a tensor (got %s)" % (name, type(t).__name__))
    if not t.is_cuda:
        raise X3DHipError("%s: needs a CUDA(HIP) tensor; got a CPU tensor (the meter has no CPU fallback)" % name)
    if t.dtype != dtype or not t.is_contiguous():
        raise X3DHipError("%s: needs a contiguous %s tensor (got %s)" % (name, dtype, t.dtype))
    if dim is not None and t.dim() != dim:
        raise X3DHipError("%s: needs %d dimensions (got shape %s)" % (name, dim, tuple(t.shape)))


def _same_device(*ts):
    devs = {t.device for t in ts if t is not None}
    if len(devs) > 1:
        raise X3DHipError("meter tensors on different devices: %s" % sorted(str(d) for d in devs))


def ap_state(dev, capacity):
    """A fresh meter state (int32 [STATE_INTS]) on `dev` with this capacity."""
    state = torch.empty(_evallib.STATE_INTS, dtype=torch.int32, device=dev)
    ap_reset(state, capacity)
    return state


def ap_reset(state, capacity):
    _need("state", state, torch.int32, 1)
    check(_evallib.lib().x3deval_ap_reset(ptr(state), int(capacity), stream()))


def ap_set_capacity(state, capacity):
    _need("state", state, torch.int32, 1)
    check(_evallib.lib().x3deval_ap_set_capacity(ptr(state), int(capacity), stream()))


def _store(state, scores, targets, weights=None):
    _need("state", state, torch.int32, 1)
    _need("scores store", scores, torch.float32, 2)
    _need("targets store", targets, torch.uint8, 2)
    if tuple(targets.shape) != tuple(scores.shape):
        raise X3DHipError("scores store %s and targets store %s differ" % (tuple(scores.shape), tuple(targets.shape)))
    if weights is not None:
        _need("weights store", weights, torch.float32, 1)
        if weights.shape[0] != scores.shape[1]:
            raise X3DHipError("weights store [%d] != capacity %d" % (weights.shape[0], scores.shape[1]))
    _same_device(state, scores, targets, weights)
    return scores.shape[0]


def ap_append(state, scores, targets, weights, in_scores, in_targets, in_weights=None):
    """Append rows in_scores [n, K], in_targets [n, K] (float32, 0 / 1) and in_weights [n] (or None) to the meter whose
    class-major stores are scores [K, capacity], targets [K, capacity] (uint8), weights [capacity] (or None)."""
    K = _store(state, scores, targets, weights)
    _need("scores", in_scores, torch.float32, 2)
    _need("targets", in_targets, torch.float32, 2)
    n = in_scores.shape[0]
    if in_scores.shape[1] != K or tuple(in_targets.shape) != (n, K):
        raise X3DHipError("ap_append: scores and targets must be [n, %d] (got %s, %s)"
                          % (K, tuple(in_scores.shape), tuple(in_targets.shape)))
    if (weights is None) != (in_weights is None):
        raise X3DHipError("ap_append: weights are given on every add or on none")
    if in_weights is not None:
        _need("weights", in_weights, torch.float32, 1)
        if in_weights.shape[0] != n:
            raise X3DHipError("ap_append: weights must be [%d] (got %s)" % (n, tuple(in_weights.shape)))
    _same_device(state, in_scores, in_targets, in_weights)
    check(_evallib.lib().x3deval_ap_append(ptr(state), ptr(scores), ptr(targets), ptr(weights), K, ptr(in_scores),
                                           ptr(in_targets), ptr(in_weights), n, stream()))


def ap_append_crops(state, scores, targets, logits, in_targets, n_crops):
    """Crop-max rows: logits [b * n_crops, K] (a sample's crops adjacent), in_targets [b, K] float32.  Appends
    max_j sigmoid(logits) and returns the max logits [b, K]."""
    K = _store(state, scores, targets)
    _need("logits", logits, torch.float32, 2)
    _need("targets", in_targets, torch.float32, 2)
    n_crops = int(n_crops)
    if n_crops < 1 or logits.shape[1] != K or logits.shape[0] % n_crops != 0 or logits.shape[0] == 0:
        raise X3DHipError("ap_append_crops: logits must be [b * %d, %d] (got %s)" % (n_crops, K, tuple(logits.shape)))
    b = logits.shape[0] // n_crops
    if tuple(in_targets.shape) != (b, K):
        raise X3DHipError("ap_append_crops: targets must be [%d, %d] (got %s)" % (b, K, tuple(in_targets.shape)))
    _same_device(state, logits, in_targets)
    maxlogit = torch.empty((b, K), dtype=torch.float32, device=logits.device)
    check(_evallib.lib().x3deval_ap_append_crops(ptr(state), ptr(scores), ptr(targets), K, ptr(logits), ptr(in_targets),
                                                 ptr(maxlogit), b, n_crops, stream()))
    return maxlogit


def ap_append_frames(state, rowoff, scores, targets, logits, labels, masks):
    """Per-frame rows: logits [B, K, T] (before interpolation), labels [B, K, TL] float32 (0 / 1), masks [B, TL] float32.
    rowoff: int32 scratch of at least B + 1 elements."""
    K = _store(state, scores, targets)
    _need("per_frame_logits", logits, torch.float32, 3)
    _need("labels", labels, torch.float32, 3)
    _need("masks", masks, torch.float32, 2)
    _need("rowoff", rowoff, torch.int32, 1)
    B, Kl, T = logits.shape
    if Kl != K or B < 1 or T < 1:
        raise X3DHipError("ap_append_frames: per_frame_logits must be [B, %d, T] (got %s)" % (K, tuple(logits.shape)))
    TL = labels.shape[2]
    if tuple(labels.shape[:2]) != (B, K) or TL < 1 or tuple(masks.shape) != (B, TL):
        raise X3DHipError("ap_append_frames: labels [%d, %d, TL] and masks [%d, TL] (got %s, %s)"
                          % (B, K, B, tuple(labels.shape), tuple(masks.shape)))
    if B > _evallib.MAX_FRAMES_B or rowoff.numel() < B + 1:
        raise X3DHipError("ap_append_frames: B = %d needs B <= %d and a row-offset scratch of B + 1" % (B, _evallib.MAX_FRAMES_B))
    _same_device(state, rowoff, logits, labels, masks)
    check(_evallib.lib().x3deval_ap_append_frames(ptr(state), ptr(rowoff), ptr(scores), ptr(targets), K, ptr(logits),
                                                  ptr(labels), ptr(masks), B, T, TL, stream()))


def ap_workspace_bytes(K, capacity):
    return int(_evallib.lib().x3deval_ap_workspace_bytes(int(K), int(capacity)))


def ap_value(state, scores, targets, weights=None, workspace=None):
    """ap [K] float32 on the device (no synchronisation).  NaN in every class while a sticky flag is set.
    workspace: uint8 scratch, by default ap_workspace_bytes(K, capacity); a given one is used as it is -- it holds
    workspace.numel() // (16 * capacity rounded up to 64) class slots (at least one), and the classes take turns on them."""
    K = _store(state, scores, targets, weights)
    cap = scores.shape[1]
    if workspace is None:
        workspace = torch.empty(ap_workspace_bytes(K, cap), dtype=torch.uint8, device=scores.device)
    _need("workspace", workspace, torch.uint8, 1)
    _same_device(scores, workspace)
    ap = torch.empty(K, dtype=torch.float32, device=scores.device)
    check(_evallib.lib().x3deval_ap_value(ptr(state), ptr(scores), ptr(targets), ptr(weights), K, cap, ptr(workspace),
                                          workspace.numel(), ptr(ap), stream()))
    return ap


def ap_marks(dev, max_marks):
    """A fresh marks buffer (int32 [1 + max_marks], no segment yet) on `dev` (include/x3deval.h)."""
    max_marks = int(max_marks)
    if max_marks < 0 or max_marks > _evallib.MERGE_MAX_MARKS:
        raise X3DHipError("ap_marks: %d marks, the meter takes up to %d" % (max_marks, _evallib.MERGE_MAX_MARKS))
    return torch.zeros(1 + max_marks, dtype=torch.int32, device=dev)


def ap_mark(state, marks):
    """Ends a segment: records the state's row count in `marks` (int32 [1 + max_marks]); capturable."""
    _need("state", state, torch.int32, 1)
    _need("marks", marks, torch.int32, 1)
    if marks.numel() < 1:
        raise X3DHipError("ap_mark: marks must be [1 + max_marks]")
    _same_device(state, marks)
    check(_evallib.lib().x3deval_ap_mark(ptr(state), ptr(marks), marks.numel() - 1, stream()))


def ap_merge_workspace_bytes(nshards, max_marks):
    return int(_evallib.lib().x3deval_ap_merge_workspace_bytes(int(nshards), int(max_marks)))


def ap_merge(states, marks, scores, targets, weights, dst_state, dst_scores, dst_targets, dst_weights=None,
             workspace=None):
    """Merges W stacked meters -- states [W, STATE_INTS], marks [W, 1 + M], scores [W, K, C], targets [W, K, C] (uint8),
    weights [W, C] or None -- into the meter (dst_state, dst_scores [K, Cd], dst_targets [K, Cd], dst_weights [Cd] or
    None) in the order segment index first, shard second (include/x3deval.h).  No synchronisation; flags are left in
    dst_state.  workspace: uint8 scratch, by default ap_merge_workspace_bytes(W, M)."""
    _need("states", states, torch.int32, 2)
    _need("marks", marks, torch.int32, 2)
    _need("scores", scores, torch.float32, 3)
    _need("targets", targets, torch.uint8, 3)
    W, K, C = scores.shape
    M = marks.shape[1] - 1
    if W < 1 or W > _evallib.MERGE_MAX_SHARDS or M < 0 or M > _evallib.MERGE_MAX_MARKS:
        raise X3DHipError("ap_merge: %d shards of %d marks; the merge takes up to %d shards and %d marks"
                          % (W, M, _evallib.MERGE_MAX_SHARDS, _evallib.MERGE_MAX_MARKS))
    if tuple(states.shape) != (W, _evallib.STATE_INTS) or marks.shape[0] != W or tuple(targets.shape) != (W, K, C) \
            or K < 1 or C < 1:
        raise X3DHipError("ap_merge: states %s, marks %s, scores %s and targets %s do not stack %d meters"
                          % (tuple(states.shape), tuple(marks.shape), tuple(scores.shape), tuple(targets.shape), W))
    if weights is not None:
        _need("weights", weights, torch.float32, 2)
        if tuple(weights.shape) != (W, C):
            raise X3DHipError("ap_merge: weights must be [%d, %d] (got %s)" % (W, C, tuple(weights.shape)))
    if (weights is None) != (dst_weights is None):
        raise X3DHipError("ap_merge: the destination is weighted exactly when the shards are")
    if _store(dst_state, dst_scores, dst_targets, dst_weights) != K or dst_scores.shape[1] < 1:
        raise X3DHipError("ap_merge: the destination stores must be [%d, capacity] (got %s)" % (K, tuple(dst_scores.shape)))
    if workspace is None:
        workspace = torch.empty(ap_merge_workspace_bytes(W, M), dtype=torch.uint8, device=scores.device)
    _need("workspace", workspace, torch.uint8, 1)
    _same_device(states, marks, scores, targets, weights, dst_state, workspace)
    check(_evallib.lib().x3deval_ap_merge(ptr(states), ptr(marks), ptr(scores), ptr(targets), ptr(weights), W, M, K, C,
                                          ptr(dst_state), ptr(dst_scores), ptr(dst_targets), ptr(dst_weights),
                                          dst_scores.shape[1], ptr(workspace), workspace.numel(), stream()))


def cls_rows(dev, capacity):
    """The row arrays of a classification meter: (loss fp32, rank, pred, label, batch_rows int32), each [capacity]."""
    return (torch.zeros(capacity, dtype=torch.float32, device=dev),) + \
        tuple(torch.zeros(capacity, dtype=torch.int32, device=dev) for _ in range(4))


def _rows(state, rows):
    _need("state", state, torch.int32, 1)
    if len(rows) != 5:
        raise X3DHipError("a classification meter has five row arrays (loss, rank, pred, label, batch_rows)")
    for name, t, dtype in zip(("loss", "rank", "pred", "label", "batch_rows"), rows, (torch.float32,) + (torch.int32,) * 4):
        _need(name + " rows", t, dtype, 1)
        if t.shape[0] != rows[0].shape[0]:
            raise X3DHipError("row arrays of different lengths")
    _same_device(state, *rows)
    return rows[0].shape[0]


def cls_append_crops(state, rows, logits, labels, n_crops):
    """One batch of the Kinetics validation (include/x3deval.h): logits [b * n_crops, K] float32 (a video's crops adjacent),
    labels [b] int64.  Appends one row per video to `rows` (cls_rows)."""
    _rows(state, rows)
    _need("logits", logits, torch.float32, 2)
    _need("labels", labels, torch.int64, 1)
    n_crops = int(n_crops)
    K = logits.shape[1]
    if n_crops < 1 or n_crops > _evallib.CLS_MAX_CROPS or logits.shape[0] % n_crops != 0 or logits.shape[0] == 0:
        raise X3DHipError("cls_append_crops: logits must be [b * n_crops, K] with 1 <= n_crops <= %d (got %s, n_crops %d)"
                          % (_evallib.CLS_MAX_CROPS, tuple(logits.shape), n_crops))
    if K < 1 or K > _evallib.CLS_MAX_K:
        raise X3DHipError("cls_append_crops: %d classes, the meter takes 1..%d" % (K, _evallib.CLS_MAX_K))
    b = logits.shape[0] // n_crops
    if labels.shape[0] != b:
        raise X3DHipError("cls_append_crops: labels must be [%d] (got %s)" % (b, tuple(labels.shape)))
    _same_device(state, logits, labels)
    check(_evallib.lib().x3deval_cls_append_crops(ptr(state), *[ptr(r) for r in rows], K, ptr(logits), ptr(labels), b,
                                                  n_crops, stream()))


def cls_value(state, rows, K, kmax):
    """(totals int64 [4], loss_sums float64 [2], class_correct int32 [K], class_count int32 [K]) on the device, without a
    synchronisation: rows / top-1 correct / top-kmax correct / batches, sum of the losses / sum of loss_i / batch_rows_i,
    the per-class top-1 histograms.  totals = -1 and loss_sums = NaN while a sticky flag is set."""
    cap = _rows(state, rows)
    dev = state.device
    totals = torch.empty(4, dtype=torch.int64, device=dev)
    loss_sums = torch.empty(2, dtype=torch.float64, device=dev)
    correct = torch.empty(int(K), dtype=torch.int32, device=dev)
    count = torch.empty(int(K), dtype=torch.int32, device=dev)
    check(_evallib.lib().x3deval_cls_value(ptr(state), *[ptr(r) for r in rows], int(K), cap, int(kmax), ptr(totals),
                                           ptr(loss_sums), ptr(correct), ptr(count), stream()))
    return totals, loss_sums, correct, count
