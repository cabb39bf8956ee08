"""Drop-in for the reference's `apmeter.APMeter` (apmeter.py), resident on the GPU: rows are appended by HIP kernels at a
device-side row count (no host synchronisation per step), and `value()` sorts every class on the device with a stable
radix sort and computes the average precision there (csrc_eval/apmeter.hip, include/x3deval.h).

    from apmeter import APMeter
    m = APMeter()
    m.add(probs, targets)            # numpy arrays / CPU tensors (the reference scripts) or device tensors
    ap = m.value()                   # CPU FloatTensor [K]; m.value().mean() is the mAP

Semantics (the reference's, apmeter.py:98-136, with its ties made definite): per class, rows sorted by score in
DESCENDING order, STABLE -- tied scores keep insertion order (the order of the add calls, row order within one, b-major then
t for add_frames); -0.0 ties +0.0; NaN ranks above +inf.  AP_k = sum over the positives of tp_i / rank_i, divided by
max(positives, 1), with rank_i = i and tp_i = positives up to i, or their weighted sums.  The reference's CPU
torch.sort is not stable, so its value is undefined wherever scores tie (saturated sigmoids, masked frames).

Each meter scores the rows of its own process.  AP is not a sum over ranks -- the rows of all ranks go through ONE sort, and
with ties keeping insertion order the merged rows need a defined order too -- so data-parallel evaluation uses meters that
remember where each add ended, and merges them on the device (x3deval_ap_merge):

    m = APMeter(track_segments=True)         # every add ends a segment (a device-side mark, capturable)
    ...                                      # rank r scores global batches r, r + W, ...  (or the r-th chunk of each)
    ap = apmeter.gather(m, process_group).value()      # on every rank: the AP of all rows
    ap = apmeter.merge_shards([m0, m1, ...]).value()   # the same for meters of one process

The merged order is segment index first, shard second: add 0 of shard 0, add 0 of shard 1, ..., add 1 of shard 0, ... --
the row order of one process that had seen global batch j * W + r as its (j * W + r)-th add.
"""
import math

import numpy as np
import torch

from x3dhip import _evallib, evalops

_MIN_CAPACITY = 1024
_MIN_MARKS = 4096


def _host_tensor(x):
    return torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x


def _is_device(x):
    return isinstance(x, torch.Tensor) and x.is_cuda


def _capturing():
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


class APMeter(object):
    """Average precision per class (the reference's APMeter) on the GPU.  See the module docstring."""

    def __init__(self, track_segments=False):
        self._track = bool(track_segments)
        self._marks = None          # int32 [1 + max_marks]: the row count after every add (x3deval_ap_mark)
        self._mpending = 0          # reserve(segments=) before the first add
        self._state = None
        self._captured = False      # an append into the current state and buffers was captured into a graph
        self._retired = []          # (state, rowoff) that captured graphs still point at: kept alive, capacity 0
        self._kept = []             # row-offset scratch / marks a captured graph points at, replaced since
        self.reset()

    # ------------------------------------------------------------------ storage
    #
    # A captured append keeps raw pointers to the state, the row-offset scratch and the class-major buffers; the graph does
    # not keep them alive.  So once an append has been captured, nothing it points at is resized or freed in place: when
    # the buffers grow or are replaced, the meter moves to a NEW state and retires the old one with capacity 0 (kept alive,
    # with the old row-offset scratch).  A replay of an old graph then fails its capacity check on the device, writes
    # nothing -- not even into the freed buffers, since every writer returns first -- and sets the retired state's overflow
    # flag, which value() reports.  Re-capture after the growth (call reserve() before capturing to avoid it).
    # The marks of a segment-tracking meter follow the same rule: a captured graph marks into the buffer it was captured
    # with, so a move to a new state is a move to new marks too, and marks that must grow after a capture move the state.
    def reset(self):
        """Resets the meter to no rows.  Device buffers are kept (a captured graph that appends to them stays valid)."""
        self._K = None
        self._weighted = None
        self._bound = 0             # upper bound of the device row count
        self._stale = False         # appends were captured: the device count may be anything up to the capacity
        self._pending = 0           # reserve() before the first add
        self._mbound = 0            # upper bound of the device segment count
        if self._state is not None:
            evalops.ap_reset(self._state, self._cap)
        if self._marks is not None:
            self._marks[:1].zero_()
        for st, _ in self._retired:
            with torch.cuda.device(st.device):
                evalops.ap_reset(st, 0)

    def _retire(self):
        """Leave the current state for a new one (see above); the caller installs the new state."""
        if self._state is not None and self._captured:
            with torch.cuda.device(self._state.device):
                evalops.ap_reset(self._state, 0)
            self._retired.append((self._state, self._rowoff))
            if self._marks is not None:
                self._kept.append(self._marks)
        self._captured = False

    def _move(self):
        """After a capture, before anything the graph points at is replaced: go on in a copy of the state (and marks)."""
        state = self._state.clone()
        marks = self._marks.clone() if self._marks is not None else None
        self._retire()
        self._state, self._marks = state, marks
        self._rowoff = torch.zeros_like(self._rowoff)

    @property
    def _mcap(self):
        return self._marks.numel() - 1

    def _grow_marks(self, segments):
        n = min(max(int(segments), int(math.ceil(self._mcap * 1.5))), _evallib.MERGE_MAX_MARKS)
        if n < segments:
            raise ValueError("APMeter: %d segments exceed the meter's limit of %d" % (segments, _evallib.MERGE_MAX_MARKS))
        if self._captured:
            self._move()
        marks = evalops.ap_marks(self._dev, n)
        marks[:self._marks.numel()].copy_(self._marks)
        self._marks = marks

    def _alloc(self, dev, K, weighted, rows):
        cap = max(_MIN_CAPACITY, int(rows), self._pending)
        if cap > _evallib.MAX_CAPACITY:
            raise ValueError("APMeter: %d rows exceed the meter's limit of %d" % (cap, _evallib.MAX_CAPACITY))
        self._retire()
        self._dev = dev
        self._scores = torch.zeros((K, cap), dtype=torch.float32, device=dev)
        self._targets = torch.zeros((K, cap), dtype=torch.uint8, device=dev)
        self._wbuf = torch.zeros((cap,), dtype=torch.float32, device=dev) if weighted else None
        self._rowoff = torch.zeros((64,), dtype=torch.int32, device=dev)
        self._cap = cap
        self._state = evalops.ap_state(dev, cap)
        if self._track:
            self._marks = evalops.ap_marks(dev, max(_MIN_MARKS, self._mpending))
            self._mbound = 0

    @property
    def _weights(self):
        """The weights buffer of a weighted meter (None otherwise; an unweighted meter after reset() of a weighted one
        keeps the buffer allocated, since a captured graph may write to it)."""
        return self._wbuf if self._weighted else None

    def _grow(self, rows):
        cap = max(int(rows), int(math.ceil(self._cap * 1.5)))
        cap = min(cap, _evallib.MAX_CAPACITY)
        if cap < rows:
            raise ValueError("APMeter: %d rows exceed the meter's limit of %d" % (rows, _evallib.MAX_CAPACITY))
        old = self._cap
        scores = torch.zeros((self._K, cap), dtype=torch.float32, device=self._dev)
        targets = torch.zeros((self._K, cap), dtype=torch.uint8, device=self._dev)
        scores[:, :old].copy_(self._scores)
        targets[:, :old].copy_(self._targets)
        if self._wbuf is not None:
            wbuf = torch.zeros((cap,), dtype=torch.float32, device=self._dev)
            wbuf[:old].copy_(self._wbuf)
            self._wbuf = wbuf
        if self._captured:                      # the old state, row offsets and marks stay behind for the captured graphs
            self._move()
        self._scores, self._targets = scores, targets
        self._cap = cap
        evalops.ap_set_capacity(self._state, cap)

    def _count(self):
        """The device row count (one synchronisation)."""
        return int(self._state[_evallib.S_COUNT].item())

    def _segments(self):
        """The device segment count (one synchronisation)."""
        return int(self._marks[0].item())

    def _mark(self):
        """Ends the segment of the add just enqueued (segment-tracking meters)."""
        if self._track:
            evalops.ap_mark(self._state, self._marks)

    def _prepare(self, dev, K, weighted, rows):
        """Buffers for `rows` more rows of K classes on `dev`.  Host checks only; grows (outside a capture) when the
        host's upper bound of the row count would pass the capacity."""
        if self._K is not None and K != self._K:
            raise AssertionError('dimensions for output should match previously added examples.')
        if self._weighted is not None and weighted != self._weighted:
            raise ValueError("APMeter: weights must be given on every add or on none")
        if self._K is not None and dev != self._dev:
            raise ValueError("APMeter: inputs on %s, the meter's rows on %s" % (dev, self._dev))
        capturing = _capturing()
        fresh = self._state is None or self._scores.shape[0] != K or self._dev != dev or \
            (weighted and self._wbuf is None)
        if fresh:
            if capturing:
                raise RuntimeError("APMeter: the meter has no buffers for this add inside a graph capture -- add once "
                                   "eagerly (or call reserve() after an eager add) before capturing")
            self._alloc(dev, K, weighted, max(rows, self._pending))
            self._bound = 0
            self._stale = False
        if self._bound + rows > self._cap or (self._stale and not capturing):
            if capturing:
                raise RuntimeError("APMeter: the capacity (%d rows) may not hold this add and the buffers cannot grow "
                                   "inside a graph capture -- call reserve(rows) before capturing" % self._cap)
            self._bound = self._count()
            if self._track and self._stale:
                self._mbound = self._segments()
            self._stale = False
            if self._bound + rows > self._cap:
                self._grow(self._bound + rows)
        if self._track:
            if self._mbound + 1 > self._mcap:
                if capturing:
                    raise RuntimeError("APMeter: the marks (%d segments) may not hold this add and cannot grow inside a "
                                       "graph capture -- call reserve(rows, segments) before capturing" % self._mcap)
                self._grow_marks(self._mbound + 1)
            self._mbound += 1
        self._K, self._weighted = K, weighted
        self._bound += rows
        if capturing:
            self._stale = True
            self._captured = True

    def reserve(self, rows, segments=None):
        """Capacity for at least `rows` rows in all, so that appends captured into a graph never need to grow the buffers.
        Before the first add the request is kept for the first allocation.  segments (a segment-tracking meter): room
        for that many adds in all (default 4096), under the same rules.

        Call it before capturing, with room for every row the replays AND any eager adds in between will append: the
        host learns about replays only at the first eager add after a capture, so later replays are invisible to its
        bound.  An append that does not fit is dropped on the device and value() raises.  Growing after a capture moves
        the meter to new buffers: graphs captured before it no longer append (value() raises if one is replayed), so
        capture again after it."""
        rows = int(rows)
        if _capturing():
            raise RuntimeError("APMeter.reserve: call it before the graph capture")
        if segments is not None:
            if not self._track:
                raise ValueError("APMeter.reserve: segments are kept by APMeter(track_segments=True) only")
            if int(segments) > _evallib.MERGE_MAX_MARKS:
                raise ValueError("APMeter: %d segments exceed the meter's limit of %d"
                                 % (int(segments), _evallib.MERGE_MAX_MARKS))
            if self._marks is None:
                self._mpending = max(self._mpending, int(segments))
            elif int(segments) > self._mcap:
                self._grow_marks(int(segments))
        if self._state is None or self._K is None:
            self._pending = max(self._pending, rows)
            if self._state is not None and rows > self._cap:
                self._retire()
                self._state = None
            return
        if rows > self._cap:
            self._grow(rows)

    # ------------------------------------------------------------------ appends
    def add(self, output, target, weight=None):
        """output [N, K] scores, target [N, K] binary, weight [N] (non-negative) or None -- numpy arrays, CPU tensors or
        device tensors.  Host inputs are checked as the reference asserts (apmeter.py:45-78) and copied to the device;
        device inputs are checked by the kernels (value() raises)."""
        output, target = _host_tensor(output), _host_tensor(target)
        if not torch.is_tensor(output) or not torch.is_tensor(target):
            raise TypeError("APMeter.add: output and target must be tensors or numpy arrays")
        if weight is not None:
            weight = _host_tensor(weight)
            if not torch.is_tensor(weight):
                raise TypeError("APMeter.add: weight must be a tensor or a numpy array")
            weight = weight.squeeze()
            if weight.dim() == 0:
                weight = weight.view(1)
        if output.dim() == 1:
            output = output.view(-1, 1)
        else:
            assert output.dim() == 2, 'wrong output size (should be 1D or 2D with one column per class)'
        if target.dim() == 1:
            target = target.view(-1, 1)
        else:
            assert target.dim() == 2, 'wrong target size (should be 1D or 2D with one column per class)'
        if tuple(target.shape) != tuple(output.shape):
            raise AssertionError('output %s and target %s must have the same shape' % (tuple(output.shape),
                                                                                       tuple(target.shape)))
        if weight is not None:
            assert weight.dim() == 1, 'Weight dimension should be 1'
            assert weight.numel() == target.size(0), 'Weight dimension 1 should be the same as that of target'
        for name, t in (("output", output), ("target", target), ("weight", weight)):
            if t is not None and not (t.dtype.is_floating_point or t.dtype in (torch.bool, torch.uint8, torch.int8,
                                                                                  torch.int16, torch.int32, torch.int64)):
                raise TypeError("APMeter.add: %s has an unsupported dtype %s" % (name, t.dtype))
        if not _is_device(target):
            assert torch.equal(target ** 2, target), 'targets should be binary (0 or 1)'
        if weight is not None and not _is_device(weight) and weight.numel() > 0:
            assert torch.min(weight) >= 0, 'Weight should be non-negative only'
        dev = self._device_of(output, target, weight)
        n, K = output.shape
        self._prepare(dev, K, weight is not None, n)
        if n == 0:
            self._mark()
            return
        o = output.to(dev, torch.float32).contiguous()
        t = target.to(dev, torch.float32).contiguous()
        w = weight.to(dev, torch.float32).contiguous() if weight is not None else None
        evalops.ap_append(self._state, self._scores, self._targets, self._weights, o, t, w)
        self._mark()

    def add_logits(self, logits, target, n_crops=1):
        """Crop-max rows of the classification scripts (train_x3d_charades.py:150-183): logits [b * n_crops, K] or
        [b * n_crops, K, 1] (a sample's crops adjacent, the model's output), target [b, K] binary.  Appends
        max over crops of sigmoid(logits) and returns the max logits [b, K] (the input of the validation BCE)."""
        if not _is_device(logits):
            raise TypeError("APMeter.add_logits: logits must be a device tensor (the model's output)")
        if logits.dim() == 3 and logits.shape[2] == 1:
            logits = logits.reshape(logits.shape[0], logits.shape[1])
        if logits.dim() != 2 or logits.dtype != torch.float32:
            raise ValueError("APMeter.add_logits: logits must be float32 [b * n_crops, K] or [b * n_crops, K, 1] "
                             "(got %s %s)" % (logits.dtype, tuple(logits.shape)))
        n_crops = int(n_crops)
        if n_crops < 1 or logits.shape[0] == 0 or logits.shape[0] % n_crops != 0:
            raise ValueError("APMeter.add_logits: %d logit rows are not a multiple of n_crops = %d"
                             % (logits.shape[0], n_crops))
        b, K = logits.shape[0] // n_crops, logits.shape[1]
        target = _host_tensor(target)
        if not torch.is_tensor(target) or tuple(target.shape) != (b, K):
            raise ValueError("APMeter.add_logits: target must be [%d, %d] (got %s)"
                             % (b, K, tuple(getattr(target, "shape", ()))))
        if not (target.dtype.is_floating_point or target.dtype in (torch.bool, torch.uint8, torch.int32, torch.int64)):
            raise TypeError("APMeter.add_logits: target has an unsupported dtype %s" % target.dtype)
        if not _is_device(target):
            assert torch.equal(target ** 2, target), 'targets should be binary (0 or 1)'
        if self._weighted:
            raise ValueError("APMeter: weights must be given on every add or on none")
        self._prepare(logits.device, K, False, b)
        t = target.to(logits.device, torch.float32).contiguous()
        maxlogit = evalops.ap_append_crops(self._state, self._scores, self._targets, logits.contiguous(), t, n_crops)
        self._mark()
        return maxlogit

    def add_frames(self, per_frame_logits, labels, masks):
        """Per-frame rows of the localisation script (train_x3d_charades_loc.py:165-186): per_frame_logits [B, K, T] (the
        model's output, before interpolation), labels [B, K, TL] binary, masks [B, TL].  Appends the rows
        (b, t < valid_t[b]) in b-major order, valid_t[b] = int(sum_t masks[b, t]), with scores
        sigmoid(F.interpolate(per_frame_logits, TL, mode='linear'))[b, :, t] * masks[b, t].  The row count stays on the
        device."""
        if not _is_device(per_frame_logits):
            raise TypeError("APMeter.add_frames: per_frame_logits must be a device tensor (the model's output)")
        if per_frame_logits.dim() != 3 or per_frame_logits.dtype != torch.float32:
            raise ValueError("APMeter.add_frames: per_frame_logits must be float32 [B, K, T] (got %s %s)"
                             % (per_frame_logits.dtype, tuple(per_frame_logits.shape)))
        B, K, T = per_frame_logits.shape
        labels, masks = _host_tensor(labels), _host_tensor(masks)
        if not torch.is_tensor(labels) or not torch.is_tensor(masks) or labels.dim() != 3 or \
                tuple(labels.shape[:2]) != (B, K) or labels.shape[2] < 1 or tuple(masks.shape) != (B, labels.shape[2]):
            raise ValueError("APMeter.add_frames: labels [%d, %d, TL] and masks [%d, TL] (got %s, %s)"
                             % (B, K, B, tuple(getattr(labels, "shape", ())), tuple(getattr(masks, "shape", ()))))
        if B < 1 or B > _evallib.MAX_FRAMES_B:
            raise ValueError("APMeter.add_frames: B = %d must be in [1, %d]" % (B, _evallib.MAX_FRAMES_B))
        if self._weighted:
            raise ValueError("APMeter: weights must be given on every add or on none")
        TL = labels.shape[2]
        dev = per_frame_logits.device
        self._prepare(dev, K, False, B * TL)
        if self._rowoff.numel() < B + 1:
            if _capturing():
                raise RuntimeError("APMeter.add_frames: add a batch of this size once before capturing")
            if self._captured:
                self._kept.append(self._rowoff)         # a captured graph writes its row offsets there
            self._rowoff = torch.zeros((B + 1,), dtype=torch.int32, device=dev)
        evalops.ap_append_frames(self._state, self._rowoff, self._scores, self._targets, per_frame_logits.contiguous(),
                                 labels.to(dev, torch.float32).contiguous(), masks.to(dev, torch.float32).contiguous())
        self._mark()

    # ------------------------------------------------------------------ results
    def _device_of(self, *ts):
        for t in ts:
            if _is_device(t):
                return t.device
        if self._state is not None:
            return self._dev
        if not torch.cuda.is_available():
            raise RuntimeError("APMeter needs a GPU (the meter has no CPU fallback)")
        return torch.device("cuda", torch.cuda.current_device())

    def value_device(self):
        """ap [K] as a device tensor, without a synchronisation (NaN in every class if an add overflowed the capacity or
        held a non-binary target or a negative weight; value() raises instead, and also reports the replay of a graph
        captured before the buffers were replaced)."""
        if self._state is None or self._K is None:
            dev = self._dev if self._state is not None else self._device_of()
            return torch.zeros((0,), dtype=torch.float32, device=dev)
        return evalops.ap_value(self._state, self._scores, self._targets, self._weights)

    def value(self):
        """Returns the average precision of each class: a CPU FloatTensor [K] (0 for an empty meter)."""
        if self._state is None or self._K is None:
            return 0
        ap = self.value_device()
        states = torch.cat([self._state] + [s.to(self._dev) for s, _ in self._retired]).cpu()
        st = states[:_evallib.STATE_INTS]
        self._bound, self._stale = int(st[_evallib.S_COUNT]), False
        if any(int(states[i + _evallib.S_OVERFLOW]) for i in range(_evallib.STATE_INTS, states.numel(),
                                                                      _evallib.STATE_INTS)):
            raise RuntimeError("APMeter: a graph captured before the meter's buffers were replaced (growth, reserve(), or "
                               "reset() and another class count) was replayed and its rows were dropped -- capture again "
                               "after reserve()")
        if int(st[_evallib.S_OVERFLOW]):
            raise RuntimeError("APMeter: an add did not fit the meter's capacity (%d rows) and was dropped -- call "
                               "reserve(rows) before capturing appends into a graph" % self._cap)
        if int(st[_evallib.S_BAD]):
            raise ValueError("APMeter: an add held a target that is not 0 / 1 or a weight that is negative or NaN")
        if self._bound == 0:
            return 0
        return ap.cpu()

    def _rows(self):
        if self._state is None or self._K is None:
            return 0
        n = self._count()
        self._bound, self._stale = n, False
        return n

    @property
    def scores(self):
        """The stored scores [N, K] (CPU float32; reading synchronises)."""
        n = self._rows()
        if n == 0:
            return torch.zeros((0,), dtype=torch.float32)
        return self._scores[:, :n].t().cpu().contiguous()

    @property
    def targets(self):
        """The stored targets [N, K] (CPU int64; reading synchronises)."""
        n = self._rows()
        if n == 0:
            return torch.zeros((0,), dtype=torch.int64)
        return self._targets[:, :n].t().to(torch.int64).cpu().contiguous()

    @property
    def weights(self):
        """The stored weights [N] (CPU float32, empty for an unweighted meter; reading synchronises)."""
        n = self._rows()
        if n == 0 or self._weights is None:
            return torch.zeros((0,), dtype=torch.float32)
        return self._weights[:n].cpu()


# ---------------------------------------------------------------------- merging
def _shard_bound(m):
    """Host upper bound of a meter's row count (the capacity once captured appends made the host's count stale)."""
    if m._state is None or m._K is None:
        return 0
    return m._cap if m._stale else m._bound


def _padded(m, K, weighted, cap, nmarks, dev):
    """A meter's five buffers at the common shape: (state [S], marks [1 + nmarks], scores [K, cap], targets [K, cap],
    weights [cap] or None).  Rows past the meter's count are never read, so the padding is not initialised."""
    if m._state is None or m._K is None:             # no rows: count 0, no segment
        state = torch.zeros(_evallib.STATE_INTS, dtype=torch.int32, device=dev)
        marks = torch.zeros(1 + nmarks, dtype=torch.int32, device=dev)
        return (state, marks, torch.empty((K, cap), dtype=torch.float32, device=dev),
                torch.empty((K, cap), dtype=torch.uint8, device=dev),
                torch.empty((cap,), dtype=torch.float32, device=dev) if weighted else None)
    marks = torch.zeros(1 + nmarks, dtype=torch.int32, device=dev)
    marks[:m._marks.numel()].copy_(m._marks)
    if m._cap == cap:
        return m._state, marks, m._scores, m._targets, m._weights
    scores = torch.empty((K, cap), dtype=torch.float32, device=dev)
    targets = torch.empty((K, cap), dtype=torch.uint8, device=dev)
    scores[:, :m._cap].copy_(m._scores)
    targets[:, :m._cap].copy_(m._targets)
    weights = None
    if weighted:
        weights = torch.empty((cap,), dtype=torch.float32, device=dev)
        weights[:m._cap].copy_(m._weights)
    return m._state, marks, scores, targets, weights


def _merged(states, marks, scores, targets, weights, bound):
    """The plain meter of the stacked shards (x3deval_ap_merge); bound: host upper bound of the total row count."""
    W, K, _ = scores.shape
    dev = scores.device
    cap = max(_MIN_CAPACITY, int(bound))
    if cap > _evallib.MAX_CAPACITY:
        raise ValueError("APMeter: %d rows exceed the meter's limit of %d" % (cap, _evallib.MAX_CAPACITY))
    out = APMeter()
    out._dev = dev
    out._scores = torch.zeros((K, cap), dtype=torch.float32, device=dev)
    out._targets = torch.zeros((K, cap), dtype=torch.uint8, device=dev)
    out._wbuf = torch.zeros((cap,), dtype=torch.float32, device=dev) if weights is not None else None
    out._rowoff = torch.zeros((64,), dtype=torch.int32, device=dev)
    out._cap = cap
    out._state = evalops.ap_state(dev, cap)
    out._K, out._weighted = K, weights is not None
    evalops.ap_merge(states, marks, scores, targets, weights, out._state, out._scores, out._targets, out._wbuf)
    out._bound, out._stale = cap, True               # the count is the device's: read at the next eager add or value()
    return out


def merge_shards(meters):
    """One plain meter holding the rows of the segment-tracking `meters` (all on one device) in the order segment index
    first, shard second: add 0 of meters[0], add 0 of meters[1], ..., add 1 of meters[0], ...  -- the rows of one meter that
    had been given the adds in that order, bit for bit, so value() is the AP over all rows with the same tie rule.  The
    shards' sticky flags travel: value() of the result raises what value() of a shard would.  No synchronisation.  A
    shard without rows (and so without a class count yet) is allowed; mixed class counts, mixed weighted / unweighted
    shards or a shard that does not track segments raise ValueError before anything is launched."""
    meters = list(meters)
    if not meters:
        raise ValueError("merge_shards: no meter given")
    if len(meters) > _evallib.MERGE_MAX_SHARDS:
        raise ValueError("merge_shards: %d meters, the merge takes up to %d" % (len(meters), _evallib.MERGE_MAX_SHARDS))
    for m in meters:
        if not isinstance(m, APMeter) or not m._track:
            raise ValueError("merge_shards: every shard must be an APMeter(track_segments=True)")
    live = [m for m in meters if m._state is not None and m._K is not None]
    if not live:
        return APMeter()
    K, weighted, dev = live[0]._K, live[0]._weighted, live[0]._dev
    for m in live:
        if m._K != K:
            raise ValueError("merge_shards: shards of %d and %d classes" % (K, m._K))
        if m._weighted != weighted:
            raise ValueError("merge_shards: weights must be given on every shard or on none")
        if m._dev != dev:
            raise ValueError("merge_shards: shards on %s and %s" % (dev, m._dev))
    cap = max(m._cap for m in live)
    nmarks = max(m._mcap for m in live)
    with torch.cuda.device(dev):
        parts = [_padded(m, K, weighted, cap, nmarks, dev) for m in meters]
        stacked = [torch.stack([p[i] for p in parts]) for i in range(4)]
        weights = torch.stack([p[4] for p in parts]) if weighted else None
        return _merged(stacked[0], stacked[1], stacked[2], stacked[3], weights, sum(_shard_bound(m) for m in meters))


def gather(meter, process_group=None):
    """On every rank of `process_group`: one plain meter holding the rows of all ranks' segment-tracking meters, merged as
    merge_shards does with the rank as the shard index.  The ranks agree on the class count, weightedness, padded capacity
    and marks length with one small MAX all-reduce of host bounds, all-gather the five buffers (on the device over RCCL --
    backend "nccl"; staged through the host for any other backend, as topkmeter.reduce_totals) and merge.  Every rank
    must call it; mismatched ranks raise ValueError on every rank, after the collective."""
    import torch.distributed as dist
    if not isinstance(meter, APMeter):
        raise TypeError("gather: expected an APMeter")
    world, rank = dist.get_world_size(process_group), dist.get_rank(process_group)
    if world > _evallib.MERGE_MAX_SHARDS:
        raise ValueError("gather: %d ranks, the merge takes up to %d" % (world, _evallib.MERGE_MAX_SHARDS))
    live = meter._state is not None and meter._K is not None
    dev = meter._dev if meter._state is not None else torch.device("cuda", torch.cuda.current_device())
    cdev = dev if dist.get_backend(process_group) == "nccl" else torch.device("cpu")
    none = -(1 << 40)
    K = meter._K if live else 0
    head = [K, -K if live else none, int(live and bool(meter._weighted)), int(live and not meter._weighted),
            meter._cap if live else 0, meter._mcap if live and meter._track else 0, int(not meter._track)]
    bounds = [0] * world
    bounds[rank] = _shard_bound(meter)
    with torch.cuda.device(dev):
        agreed = torch.tensor(head + bounds, dtype=torch.int64, device=cdev)
        dist.all_reduce(agreed, op=dist.ReduceOp.MAX, group=process_group)
        agreed = [int(x) for x in agreed.cpu()]
        Kmax, negKmin, has_w, has_unw, cap, nmarks, untracked = agreed[:7]
        if untracked:
            raise ValueError("gather: every rank's meter must be an APMeter(track_segments=True)")
        if Kmax == 0:
            return APMeter()
        if -negKmin != Kmax:
            raise ValueError("gather: the ranks' meters have different class counts (%d and %d)" % (-negKmin, Kmax))
        if has_w and has_unw:
            raise ValueError("gather: weights must be given on every rank or on none")
        parts = _padded(meter, Kmax, bool(has_w), cap, nmarks, dev)
        stacked = []
        for t in parts:
            if t is None:
                stacked.append(None)
                continue
            src = t.contiguous().to(cdev)
            out = torch.empty((world,) + tuple(src.shape), dtype=src.dtype, device=cdev)
            dist.all_gather(list(out.unbind(0)), src, group=process_group)
            stacked.append(out.to(dev))
        return _merged(stacked[0], stacked[1], stacked[2], stacked[3], stacked[4], sum(agreed[7:]))
