"""Host side of the GPU clip input pipeline: the integer/random logic of the reference's per-sample transforms, the
resample coefficient tables, gather_frames (lazy videos -> the frames a batch draws, decoded), and ClipPreprocessor,
which hands a Kinetics step's samples to dataops.ClipBatcher (the clip kernels of csrc_data/clipbatch.hip, libx3ddata.so).

Reference call sites mirrored (random draws in the reference's order, from Python's `random` like the reference):
  kinetics_multigrid.py:240-253 (__getitem__), transforms/temporal_transforms.py:94-117 (TemporalRandomCrop),
  transforms/spatial_transforms.py:480-503 (MultiScaleRandomCropMultigrid), :334-349 (RandomHorizontalFlip),
  :44-83,106-116 (ToTensor(255), Normalize).  The arithmetic runs on the GPU; nothing here falls back to CPU.
"""
import math
import random as _random

import numpy as np
import torch

PRECISION_BITS = 32 - 8 - 2
KINETICS_MEAN = [110.63666788 / 255, 103.16065604 / 255, 96.29023126 / 255]      # train_x3d_kinetics_multigrid.py:45
KINETICS_STD = [38.7568578 / 255, 37.88248729 / 255, 40.02898126 / 255]          # :46


def temporal_random_crop(frame_indices, size, gamma_tau, t_stride=1, trunc=None, rng=_random):
    """TemporalRandomCrop.__call__ (temporal_transforms.py:94-117), including its looping of short videos."""
    trunc = size if trunc is None else trunc
    rand_end = max(0, len(frame_indices) - size - 1)
    begin_index = rng.randint(0, rand_end)
    end_index = min(begin_index + size, len(frame_indices))
    out = list(frame_indices[begin_index:end_index:t_stride * gamma_tau])
    out = out[:trunc // gamma_tau]
    i = 0
    while i < len(out):                     # the reference appends to the list it iterates over
        if len(out) >= trunc // gamma_tau:
            break
        out.append(out[i])
        i += 1
    return out


def draw_clip_params(n_frames, width, height, scales, c_size, num_frames, gamma_tau, sample_duration, rng=_random):
    """All random draws of one __getitem__ in the reference's order (kinetics_multigrid.py:245-251):
    t_stride, TemporalRandomCrop's begin index, then Compose.randomize_parameters (scale, tl_x, tl_y, flip p)."""
    t_stride = rng.randint(1, max(1, num_frames // sample_duration))
    idx = temporal_random_crop(list(range(1, n_frames + 1)), num_frames, gamma_tau, t_stride, sample_duration, rng)
    scale = scales[rng.randint(0, len(scales) - 1)]
    tl_x = rng.random()
    tl_y = rng.random()
    p = rng.random()
    min_length = min(width, height)
    crop = int(min_length * scale)
    x1 = int(tl_x * (width - crop))
    y1 = int(tl_y * (height - crop))
    return dict(frame_idx=[i - 1 for i in idx], x1=x1, y1=y1, crop=crop, out=c_size, flip=p < 0.5, t_stride=t_stride,
                scale=scale, tl_x=tl_x, tl_y=tl_y, p=p)


def center_crop_box(width, height):
    """CenterCropScaled (spatial_transforms.py:214-228): centred square of side min(w, h); Python's round (half to even)
    like the reference."""
    crop = min(width, height)
    return int(round((width - crop) / 2.)), int(round((height - crop) / 2.)), crop


def val_crop_indices(n_frames, gamma_tau, sample_duration, crops):
    """Validation windows of kinetics.py:214-233: every gamma_tau-th frame, `crops` windows of sample_duration //
    gamma_tau frames at 0, step, 2*step (step 0 -> identical windows).  0-based frame lists."""
    strided = list(range(n_frames))[::gamma_tau]
    frames = sample_duration // gamma_tau
    step = int((len(strided) - 1 - frames) // (crops - 1))
    if step < 0 or len(strided) < frames:
        raise ValueError("video of %d frames is too short for %d-frame validation windows at stride %d" %
                         (n_frames, frames, gamma_tau))
    starts = [0] * crops if step == 0 else list(range(0, step * crops, step))
    return [strided[s0:s0 + frames] for s0 in starts]


_coeff_cache = {}


def resize_coeffs(in_size, out_size):
    """Pillow's bilinear coefficient table for in_size -> out_size (Resample.c precompute_coeffs with the triangle
    filter + normalize_coeffs_8bpc), vectorised; double precision in the same operation order as the C code."""
    key = (in_size, out_size)
    hit = _coeff_cache.get(key)
    if hit is not None:
        return hit
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    xx = np.arange(out_size, dtype=np.float64)
    center = (xx + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)          # (int) truncation of a positive value
    xmin = np.where(center - support + 0.5 < 0, 0, xmin)
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size)
    n = xmax - xmin
    x = np.arange(ksize, dtype=np.float64)[None, :]
    a = (x + xmin[:, None] - center[:, None] + 0.5) * ss
    w = np.where(np.abs(a) < 1.0, 1.0 - np.abs(a), 0.0)
    w = np.where(x < n[:, None], w, 0.0)
    ww = np.zeros(out_size)
    for i in range(ksize):                   # left-to-right accumulation like the C loop
        ww = ww + w[:, i]
    k = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    v = k * float(1 << PRECISION_BITS)
    kk = np.where(v < 0, (v - 0.5).astype(np.int64), (v + 0.5).astype(np.int64)).astype(np.int32)
    bounds = np.stack([xmin, n], axis=1).astype(np.int32)
    out = (np.ascontiguousarray(kk), np.ascontiguousarray(bounds), ksize)
    _coeff_cache[key] = out
    return out


def is_lazy(video):
    """Whether `video` is a lazy video rather than a decoded tensor: .shape = (n_frames, H, W, 3), .device, .source (an object
    with decode_into(requests, dst)) and .requests(idx), what the source takes for the 0-based frames idx (frames.py)."""
    return not isinstance(video, torch.Tensor) and all(hasattr(video, a) for a in ("shape", "device", "source", "requests"))


def gather_frames(samples):
    """samples: dicts with 'frames' and 'frame_idx' (as dataops.ClipBatcher takes them).  Every sample whose 'frames' is a
    lazy video gets, in place, the uint8 tensor of exactly its frame_idx and frame_idx = range(len): one decode_into per
    source and frame size over all samples, into one buffer.  A decoded tensor is left as it is."""
    groups = {}
    for s in samples:
        v = s["frames"]
        if is_lazy(v):
            groups.setdefault((id(v.source),) + v.shape[1:3], []).append(s)
    for group in groups.values():
        v = group[0]["frames"]
        for s in group:
            n = s["frames"].shape[0]
            if any(not 0 <= i < n for i in s["frame_idx"]):
                raise ValueError("frame index outside the video")
        requests = [r for s in group for r in s["frames"].requests(s["frame_idx"])]
        buf = torch.empty((len(requests),) + v.shape[1:], dtype=torch.uint8, device=v.device)
        v.source.decode_into(requests, buf)
        at = 0
        for s in group:
            T = len(s["frame_idx"])
            s["frames"], s["frame_idx"] = buf[at:at + T], range(T)
            at += T


class ClipPreprocessor:
    """Turns decoded uint8 videos resident on the GPU into the normalised float NCTHW batch of one training step: an
    adapter that lays the samples out for dataops.ClipBatcher (one job table, one scratch buffer, two launches).

    samples: list of dicts with 'frames' (uint8 CUDA tensor [Tsrc, H, W, 3]) and the params of draw_clip_params
    (frame_idx, x1, y1, crop, out, flip) -- what gather_frames rewrites -- or of (frames, params) pairs; all samples of
    a step share T and the output size (the multigrid schedule fixes both per step)."""

    def __init__(self, device, mean=KINETICS_MEAN, std=KINETICS_STD):
        from .dataops import ClipBatcher          # dataops imports resize_coeffs from this module
        self.device = torch.device(device)
        self._batcher = ClipBatcher(self.device, mean, std)

    def __call__(self, samples, out=None):
        pairs = [(s["frames"], s) if isinstance(s, dict) else s for s in samples]
        B = len(pairs)
        T = len(pairs[0][1]["frame_idx"])
        S = pairs[0][1]["out"]
        batch = out if out is not None else torch.empty((B, 3, T, S, S), dtype=torch.float32, device=self.device)
        jobs = []
        for b, (frames, p) in enumerate(pairs):
            if len(p["frame_idx"]) != T or p["out"] != S:
                raise ValueError("all samples of a step share T and the output size")
            jobs.append(dict(frames=frames, frame_idx=p["frame_idx"], x1=p["x1"], y1=p["y1"], crop=p["crop"],
                             flip=p["flip"], dst_off=b * 3 * T * S * S, dst_cs=T * S * S, dst_ts=S * S))
        return self._batcher(batch, jobs, S)
