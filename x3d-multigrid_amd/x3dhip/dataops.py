"""Tensor-level wrappers over the input C ABI (include/x3ddata.h), in the style of evalops.py.

Shapes, dtypes, devices, crop boxes and frame indices are checked here, on the host, before anything is launched (the
messages follow clip_input.py).  Every launch goes to the current stream.  There is no fallback: a CPU tensor raises.
"""
import numpy as np
import torch

from . import _datalib
from ._datalib import CLIP_JOB_DT, LABEL_JOB_DT, check
from ._lib import ptr, stream
from .clip_input import resize_coeffs


class AnnotationTable:
    """The device-resident annotation table of include/x3ddata.h: ann_off [V + 1], ann_cls / ann_lo / ann_hi [A], int32."""

    def __init__(self, ann_off, ann_cls, ann_lo, ann_hi, device, n_frames=None):
        arrs = [np.ascontiguousarray(a, dtype=np.int32) for a in (ann_off, ann_cls, ann_lo, ann_hi)]
        off, cls, lo, hi = arrs
        if off.ndim != 1 or off.size < 1 or off[0] != 0 or np.any(np.diff(off) < 0) or off[-1] != cls.size:
            raise ValueError("ann_off must rise from 0 to the number of annotations")
        if not (cls.shape == lo.shape == hi.shape) or cls.ndim != 1:
            raise ValueError("ann_cls, ann_lo and ann_hi must be flat arrays of one length")
        self.device = torch.device(device)
        self.V = off.size - 1
        # frames per video (optional): lets charades_labels refuse a window that runs past the end of its video
        self.n_frames = None if n_frames is None else np.asarray(n_frames, dtype=np.int64)
        if self.n_frames is not None and self.n_frames.shape != (self.V,):
            raise ValueError("n_frames must have one entry per video")
        self.host = arrs
        # at least one element each, so that an empty table still has valid pointers
        self.off, self.cls, self.lo, self.hi = (
            torch.from_numpy(a if a.size else np.zeros(1, np.int32)).to(self.device) for a in arrs)


def charades_labels(table, jobs, K, TLmax, labels=True, masks=True, cls=True):
    """jobs: (video, start, n) per window, host integers.  Returns (labels [B, K, TLmax], masks [B, TLmax], cls [B, K])
    float32 on the table's device; an output asked for as False is None, one given as a tensor is written in place."""
    jobs = np.asarray(jobs, dtype=np.int64).reshape(-1, 3)
    B = jobs.shape[0]
    K, TLmax = int(K), int(TLmax)
    if B < 1 or K < 1 or TLmax < 1:
        raise ValueError("charades_labels: needs B, K, TLmax >= 1 (got %d, %d, %d)" % (B, K, TLmax))
    if np.any(jobs[:, 0] < 0) or np.any(jobs[:, 0] >= table.V):
        raise ValueError("video index outside the annotation table")
    if np.any(jobs[:, 1] < 0) or np.any(jobs[:, 2] < 0) or np.any(jobs[:, 2] > TLmax):
        raise ValueError("label window outside [0, TLmax]")
    if table.n_frames is not None and np.any(jobs[:, 1] + jobs[:, 2] > table.n_frames[jobs[:, 0]]):
        raise ValueError("label window outside the video")
    dev = table.device
    outs = []
    for name, want, shape in (("labels", labels, (B, K, TLmax)), ("masks", masks, (B, TLmax)), ("cls", cls, (B, K))):
        if want is True:
            want = torch.empty(shape, dtype=torch.float32, device=dev)
        elif want is False or want is None:
            want = None
        elif (not isinstance(want, torch.Tensor) or want.device != dev or want.dtype != torch.float32
              or not want.is_contiguous() or tuple(want.shape) != shape):
            raise ValueError("%s: needs a contiguous float32 tensor %s on %s" % (name, shape, dev))
        outs.append(want)
    if all(o is None for o in outs):
        raise ValueError("charades_labels: no output asked for")
    tab = np.zeros(B, dtype=LABEL_JOB_DT)
    tab["video"], tab["start"], tab["n"] = jobs[:, 0], jobs[:, 1], jobs[:, 2]
    jd = torch.from_numpy(tab.view(np.uint8)).to(dev)
    check(_datalib.lib().x3ddata_charades_labels(ptr(table.off), ptr(table.cls), ptr(table.lo), ptr(table.hi), table.V,
                                                 ptr(jd), B, K, TLmax, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), stream()))
    return tuple(outs)


class ClipBatcher:
    """Fills a float32 batch tensor from decoded uint8 videos resident on the GPU: x3ddata_clip_batch with one job table,
    one frame-index array and one scratch buffer per call, and two launches whatever the number of samples."""

    def __init__(self, device, mean, std):
        self.device = torch.device(device)
        self.mean = np.asarray(mean, dtype=np.float32)
        self.std = np.asarray(std, dtype=np.float32)
        if self.mean.shape != (3,) or self.std.shape != (3,):
            raise ValueError("mean and std must have 3 entries")
        self._tables = {}

    def _table(self, crop, out):
        key = (crop, out)
        hit = self._tables.get(key)
        if hit is None:
            kk, bounds, ksize = resize_coeffs(crop, out)
            hit = (torch.from_numpy(kk).to(self.device), torch.from_numpy(bounds).to(self.device), ksize)
            self._tables[key] = hit
        return hit

    def __call__(self, batch, samples, out_size):
        """batch: contiguous float32 tensor on the device.  samples: dicts with
             frames     uint8 tensor [Tsrc, H, W, 3] on the device
             frame_idx  0-based source frames, in output order
             x1, y1, crop, flip
             dst_off    element offset of the sample in `batch`;  dst_cs, dst_ts: channel and frame strides (elements)
             Tpad       frames of the destination clip (>= len(frame_idx); the tail is zero-filled); default: no padding
             nwin, win_step, win_len, dst_ws   windows gathered from the resized frames (default: one clip)."""
        S = int(out_size)
        if (not isinstance(batch, torch.Tensor) or batch.device != self.device or batch.dtype != torch.float32
                or not batch.is_contiguous()):
            raise ValueError("batch must be a contiguous float32 tensor on %s" % self.device)
        n = len(samples)
        if n < 1 or S < 1:
            raise ValueError("clip batch needs at least one sample and a positive output size")
        jobs = np.zeros(n, dtype=CLIP_JOB_DT)
        fidx = []
        tmp_off = 0
        max_T = max_Tpad = max_crop = 0
        for b, s in enumerate(samples):
            frames = s["frames"]
            if (not isinstance(frames, torch.Tensor) or frames.device != self.device or frames.dtype != torch.uint8
                    or not frames.is_contiguous()):
                raise ValueError("frames must be contiguous uint8 tensors on %s" % self.device)
            if frames.dim() != 4 or frames.shape[3] != 3:
                raise ValueError("frames must be [T, H, W, 3]")
            Tsrc, Hs, Ws, _ = frames.shape
            x1, y1, crop = int(s["x1"]), int(s["y1"]), int(s["crop"])
            if crop <= 0 or x1 < 0 or y1 < 0 or x1 + crop > Ws or y1 + crop > Hs:
                raise ValueError("crop box outside the frame")
            idx = [int(i) for i in s["frame_idx"]]
            T = len(idx)
            if T < 1 or min(idx) < 0 or max(idx) >= Tsrc:
                raise ValueError("frame index outside the video")
            Tpad = int(s.get("Tpad", T))
            nwin, step, wlen = int(s.get("nwin", 1)), int(s.get("win_step", 0)), int(s.get("win_len", T))
            cs, ts, ws, off = int(s["dst_cs"]), int(s["dst_ts"]), int(s.get("dst_ws", 0)), int(s["dst_off"])
            if nwin == 1:
                if Tpad < T or wlen < T:
                    raise ValueError("a clip of %d frames does not fit its destination of %d" % (T, min(Tpad, wlen)))
                extent = 2 * cs + (Tpad - 1) * ts + S * S
            else:
                if Tpad != T or step < 0 or wlen < 1 or T != (nwin - 1) * step + wlen:
                    raise ValueError("windows need (nwin - 1) * win_step + win_len frames and no padding")
                extent = (nwin - 1) * ws + 2 * cs + (wlen - 1) * ts + S * S
            if off < 0 or cs < 0 or ts < S * S or ws < 0 or off + extent > batch.numel():
                raise ValueError("destination outside the batch tensor")
            kk, bounds, ksize = self._table(crop, S)
            jobs[b] = (frames.data_ptr(), batch.data_ptr() + 4 * off, kk.data_ptr(), bounds.data_ptr(), cs, ts, ws, tmp_off,
                       len(fidx), Hs, Ws, x1, y1, crop, S, ksize, T, Tpad, 1 if s.get("flip") else 0, nwin, step, wlen)
            fidx += idx
            tmp_off += T * crop * S * 3
            max_T, max_Tpad, max_crop = max(max_T, T), max(max_Tpad, Tpad), max(max_crop, crop)
        if max_Tpad > 65535 or n > 65535:
            raise ValueError("clip batch: at most 65535 samples of at most 65535 frames")
        # one upload: the job table, then the frame indices
        jb = jobs.view(np.uint8)
        host = np.concatenate([jb, np.asarray(fidx, dtype=np.int32).view(np.uint8)])
        dev_tab = torch.from_numpy(host).to(self.device)
        scratch = torch.empty(tmp_off, dtype=torch.uint8, device=self.device)
        check(_datalib.lib().x3ddata_clip_batch(dev_tab.data_ptr(), n, dev_tab.data_ptr() + jb.size, scratch.data_ptr(),
                                                max_T, max_Tpad, max_crop, S, self.mean.ctypes.data, self.std.ctypes.data,
                                                stream()))
        return batch
