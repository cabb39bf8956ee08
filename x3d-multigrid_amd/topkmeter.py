"""Top-k accuracy and loss of the Kinetics validation phase (the reference's train_x3d_kinetics_multigrid.py:253-265,
293-295), resident on the GPU: one row per video is appended by a HIP kernel at a device-side row count (no host
synchronisation per batch, capturable), and `value()` reduces the rows on the device (csrc_eval/topk.hip,
include/x3deval.h).

    from topkmeter import TopKMeter
    m = TopKMeter(kmax=5)
    m.add_logits(model(clips.view(b * n, ...)), labels, n_crops=n)     # per batch
    res = m.value()          # {"videos", "top1", "top5", "cls_loss", "loss_per_video", "class_acc", "mean_class_acc"}

Per video, in fp64 from the fp32 logits: s = the mean over the crops of the softmax, m = the mean over the crops of the
logits; loss = cross entropy of m; the prediction is the largest s; top-k is correct iff fewer than k classes rank above
the label.  Ties are definite: among equal s the LOWER class index ranks first (torch.max leaves it open).  A video whose
s[label] is NaN (a NaN or +inf logit, or a crop of -inf only, makes s NaN in every class) is wrong at every k and has no
prediction (-1).  "cls_loss" is the reference's figure, the mean over the batches of the batch-mean loss;
"loss_per_video" weighs every video equally.

Each meter scores the rows of its own process; `reduce_totals` sums the raw totals of the ranks.
"""
import math

import torch

from x3dhip import _evallib, evalops

_MIN_CAPACITY = 1024


def _capturing():
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def summarise(totals):
    """The value() dict of raw totals {"totals" int64 [rows, top-1, top-kmax, batches], "loss" float64 [sum, sum of
    loss / batch_rows], "class_correct", "class_count" int64 [K]} (CPU or device tensors)."""
    t = [int(x) for x in totals["totals"].cpu()]
    ls = [float(x) for x in totals["loss"].cpu()]
    videos, batches = t[0], t[3]
    correct, count = totals["class_correct"].cpu().double(), totals["class_count"].cpu().double()
    class_acc = torch.where(count > 0, correct / count.clamp(min=1), torch.full_like(count, float("nan"))).float()
    seen = class_acc[count > 0]
    return {"videos": videos, "top1": t[1] / max(videos, 1), "top5": t[2] / max(videos, 1),
            "cls_loss": ls[1] / max(batches, 1), "loss_per_video": ls[0] / max(videos, 1), "class_acc": class_acc,
            "mean_class_acc": float(seen.double().mean()) if seen.numel() else 0.0}


def reduce_totals(totals, process_group=None):
    """SUM all-reduce of a meter's raw totals (TopKMeter.totals(check=False)) over the ranks of `process_group` (gloo or
    RCCL; the tensors may live on the host or the device and are moved to where the backend needs them).  Returns what
    value() would return for the union of the ranks' rows.  Every rank calls it; a rank without rows (K unknown) joins
    with zeros.  A rank whose meter failed (totals -1: an overflow or a label outside the classes) is counted in the
    same all-reduce and EVERY rank raises afterwards, so no rank is left waiting inside a collective."""
    import torch.distributed as dist
    dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend(process_group) == "nccl" else torch.device("cpu")
    K = torch.tensor([totals["class_count"].numel()], dtype=torch.int64, device=dev)
    dist.all_reduce(K, op=dist.ReduceOp.MAX, group=process_group)
    K = int(K)
    failed = bool(totals["totals"][0] < 0)
    hist = [totals[n].to(dev, torch.int64) if totals[n].numel() else torch.zeros(K, dtype=torch.int64, device=dev)
            for n in ("class_correct", "class_count")]
    mismatch = any(h.numel() != K for h in hist)
    if failed or mismatch:                       # join the collectives with zeros, report after them
        hist = [torch.zeros(K, dtype=torch.int64, device=dev) for _ in hist]
    t4 = torch.zeros(4, dtype=torch.int64, device=dev) if failed or mismatch else totals["totals"].to(dev, torch.int64)
    ints = torch.cat([t4] + hist + [torch.tensor([int(failed), int(mismatch)], dtype=torch.int64, device=dev)])
    loss = torch.zeros(2, dtype=torch.float64, device=dev) if failed or mismatch else totals["loss"].to(dev, torch.float64).clone()
    dist.all_reduce(ints, op=dist.ReduceOp.SUM, group=process_group)
    dist.all_reduce(loss, op=dist.ReduceOp.SUM, group=process_group)
    if failed:
        raise totals.get("error") or RuntimeError("reduce_totals: this rank's totals are those of a failed meter")
    if mismatch or int(ints[-1]):
        raise ValueError("reduce_totals: the ranks' meters have different class counts")
    if int(ints[-2]):
        raise RuntimeError("reduce_totals: the meter of %d other rank(s) failed (an add that did not fit, or a label "
                           "outside the classes)" % int(ints[-2]))
    return summarise({"totals": ints[:4], "loss": loss, "class_correct": ints[4:4 + K], "class_count": ints[4 + K:4 + 2 * K]})


class TopKMeter(object):
    """Top-1 / top-kmax accuracy, loss and per-class accuracy of a validation phase on the GPU.  See the module
    docstring."""

    def __init__(self, kmax=5):
        self.kmax = int(kmax)
        if self.kmax < 1:
            raise ValueError("TopKMeter: kmax must be at least 1")
        self._state = None
        self._captured = False      # an append into the current state and rows was captured into a graph
        self._retired = []          # states that captured graphs still point at: kept alive, capacity 0
        self.reset()

    # Storage follows APMeter (apmeter.py): a captured append keeps raw pointers to the state and the row arrays, so once
    # an append has been captured, growth moves the meter to a NEW state and retires the old one with capacity 0.  A replay
    # of an old graph then fails its capacity check on the device, writes nothing and sets the retired state's overflow
    # flag, which value() reports.
    def reset(self):
        """Resets the meter to no rows.  Device buffers are kept (a captured graph that appends to them stays valid)."""
        self._K = None
        self._bound = 0             # upper bound of the device row count
        self._stale = False         # appends were captured: the device count may be anything up to the capacity
        self._pending = 0           # reserve() before the first add
        if self._state is not None:
            with torch.cuda.device(self._dev):
                evalops.ap_reset(self._state, self._cap)
        for st in self._retired:
            with torch.cuda.device(st.device):
                evalops.ap_reset(st, 0)

    def _retire(self):
        if self._state is not None and self._captured:
            with torch.cuda.device(self._state.device):
                evalops.ap_reset(self._state, 0)
            self._retired.append(self._state)
        self._captured = False

    def _alloc(self, dev, rows):
        cap = max(_MIN_CAPACITY, int(rows), self._pending)
        if cap > _evallib.MAX_CAPACITY:
            raise ValueError("TopKMeter: %d rows exceed the meter's limit of %d" % (cap, _evallib.MAX_CAPACITY))
        self._retire()
        self._dev = dev
        self._rows = evalops.cls_rows(dev, cap)
        self._cap = cap
        self._state = evalops.ap_state(dev, cap)

    def _grow(self, rows):
        cap = min(max(int(rows), int(math.ceil(self._cap * 1.5))), _evallib.MAX_CAPACITY)
        if cap < rows:
            raise ValueError("TopKMeter: %d rows exceed the meter's limit of %d" % (rows, _evallib.MAX_CAPACITY))
        new = evalops.cls_rows(self._dev, cap)
        for n, o in zip(new, self._rows):
            n[:self._cap].copy_(o)
        if self._captured:                      # the old state stays behind for the captured graphs
            state = self._state.clone()
            self._retire()
            self._state = state
        self._rows, self._cap = new, cap
        evalops.ap_set_capacity(self._state, cap)

    def _prepare(self, dev, K, rows):
        """Row arrays for `rows` more videos of K classes on `dev`.  Host checks only; grows (outside a capture) when the
        host's upper bound of the row count would pass the capacity."""
        if self._K is not None and K != self._K:
            raise ValueError("TopKMeter: %d classes, earlier adds had %d" % (K, self._K))
        if self._K is not None and dev != self._dev:
            raise ValueError("TopKMeter: inputs on %s, the meter's rows on %s" % (dev, self._dev))
        capturing = _capturing()
        if self._state is None or self._dev != dev:
            if capturing:
                raise RuntimeError("TopKMeter: the meter has no buffers for this add inside a graph capture -- add once "
                                   "eagerly (or call reserve() after an eager add) before capturing")
            self._alloc(dev, max(rows, self._pending))
            self._bound, self._stale = 0, False
        if self._bound + rows > self._cap or (self._stale and not capturing):
            if capturing:
                raise RuntimeError("TopKMeter: the capacity (%d rows) may not hold this add and the buffers cannot grow "
                                   "inside a graph capture -- call reserve(rows) before capturing" % self._cap)
            self._bound, self._stale = int(self._state[_evallib.S_COUNT].item()), False
            if self._bound + rows > self._cap:
                self._grow(self._bound + rows)
        self._K = K
        self._bound += rows
        if capturing:
            self._stale = self._captured = True

    def reserve(self, rows):
        """Capacity for at least `rows` rows in all, so that appends captured into a graph never need to grow the buffers
        (APMeter.reserve: call it before capturing, with room for every row the replays and any eager adds in between will
        append; growth after a capture moves the meter to new buffers, so capture again after it)."""
        rows = int(rows)
        if _capturing():
            raise RuntimeError("TopKMeter.reserve: call it before the graph capture")
        if self._state is None:
            self._pending = max(self._pending, rows)
        elif rows > self._cap:
            self._grow(rows)

    def add_logits(self, logits, labels, n_crops=1):
        """One batch: logits float32 [b * n_crops, K] or [b * n_crops, K, 1] on the device (a video's crops adjacent, as
        the Trainer and model(x) return them), labels [b] (or [b, 1]) class indices.  Nothing is read back."""
        if not (isinstance(logits, torch.Tensor) and logits.is_cuda):
            raise TypeError("TopKMeter.add_logits: logits must be a device tensor (the model's output)")
        if logits.dim() == 3 and logits.shape[2] == 1:
            logits = logits.reshape(logits.shape[0], logits.shape[1])
        if logits.dim() != 2 or logits.dtype != torch.float32:
            raise ValueError("TopKMeter.add_logits: logits must be float32 [b * n_crops, K] or [b * n_crops, K, 1] "
                             "(got %s %s)" % (logits.dtype, tuple(logits.shape)))
        n_crops = int(n_crops)
        if n_crops < 1 or logits.shape[0] == 0 or logits.shape[0] % n_crops != 0:
            raise ValueError("TopKMeter.add_logits: %d logit rows are not a multiple of n_crops = %d"
                             % (logits.shape[0], n_crops))
        b, K = logits.shape[0] // n_crops, logits.shape[1]
        if K > _evallib.CLS_MAX_K or n_crops > _evallib.CLS_MAX_CROPS:
            raise ValueError("TopKMeter.add_logits: the meter takes up to %d classes and %d crops (got %d, %d)"
                             % (_evallib.CLS_MAX_K, _evallib.CLS_MAX_CROPS, K, n_crops))
        labels = torch.as_tensor(labels)
        if labels.dtype.is_floating_point or labels.dtype == torch.bool or labels.numel() != b:
            raise ValueError("TopKMeter.add_logits: labels must be %d class indices (got %s %s)"
                             % (b, labels.dtype, tuple(labels.shape)))
        self._prepare(logits.device, K, b)
        evalops.cls_append_crops(self._state, self._rows, logits.contiguous(),
                                 labels.reshape(b).to(logits.device, torch.int64).contiguous(), n_crops)

    def _totals_device(self):
        return evalops.cls_value(self._state, self._rows, self._K, self.kmax)

    def totals(self, check=True):
        """The raw totals as CPU tensors (one synchronisation): {"totals" int64 [rows, top-1 correct, top-kmax correct,
        batches], "loss" float64 [sum of the losses, sum of loss / rows of its batch], "class_correct", "class_count"
        int64 [K]}.  Raises if an add overflowed the capacity or held a label outside [0, K); with check=False the
        failure travels in the result instead -- "totals" = -1, "loss" = NaN, "error" the exception -- for
        reduce_totals, which raises on every rank together."""
        if self._state is None or self._K is None:
            return {"totals": torch.zeros(4, dtype=torch.int64), "loss": torch.zeros(2, dtype=torch.float64),
                    "class_correct": torch.zeros(0, dtype=torch.int64), "class_count": torch.zeros(0, dtype=torch.int64)}
        with torch.cuda.device(self._dev):
            t, ls, correct, count = self._totals_device()
        states = torch.cat([self._state] + [s.to(self._dev) for s in self._retired]).cpu()
        st = states[:_evallib.STATE_INTS]
        self._bound, self._stale = int(st[_evallib.S_COUNT]), False
        error = None
        if any(int(states[i + _evallib.S_OVERFLOW]) for i in range(_evallib.STATE_INTS, states.numel(),
                                                                      _evallib.STATE_INTS)):
            error = RuntimeError("TopKMeter: a graph captured before the meter's buffers were replaced was replayed and "
                                 "its rows were dropped -- capture again after reserve()")
        elif int(st[_evallib.S_OVERFLOW]):
            error = RuntimeError("TopKMeter: an add did not fit the meter's capacity (%d rows) and was dropped -- call "
                                 "reserve(rows) before capturing appends into a graph" % self._cap)
        elif int(st[_evallib.S_BAD]):
            error = ValueError("TopKMeter: an add held a label outside [0, %d)" % self._K)
        out = {"totals": t.cpu(), "loss": ls.cpu(), "class_correct": correct.cpu().long(), "class_count": count.cpu().long()}
        if error is not None:
            if check:
                raise error
            out.update(totals=torch.full((4,), -1, dtype=torch.int64), loss=torch.full((2,), float("nan"), dtype=torch.float64),
                       error=error)
        return out

    def value(self):
        """{"videos", "top1", "top5" (top-kmax), "cls_loss" (mean of the batch means), "loss_per_video", "class_acc" (CPU
        FloatTensor [K], NaN where a class has no video), "mean_class_acc"} of this process's rows."""
        return summarise(self.totals())

    def rows(self):
        """The stored rows as CPU tensors {"loss", "rank", "pred", "label", "batch_rows"} (reading synchronises)."""
        n = 0
        if self._state is not None and self._K is not None:
            n = int(self._state[_evallib.S_COUNT].item())
            self._bound, self._stale = n, False
        names = ("loss", "rank", "pred", "label", "batch_rows")
        if n == 0:
            return {k: torch.zeros(0, dtype=torch.float32 if k == "loss" else torch.int32) for k in names}
        return {k: r[:n].cpu() for k, r in zip(names, self._rows)}
