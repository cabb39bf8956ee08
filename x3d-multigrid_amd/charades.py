"""Charades dataset for X3D on MI355X -- the drop-in for the reference's ``charades.py`` (make_dataset :68-104, Charades
:107-164, custom_collate_fn :167-189) over decoded uint8 videos already resident in HBM (frames.charades_videos decodes
folders of JPEG frames into that form), or over lazy videos (frames.py: the same videos as prepared JPEG scans in a frame
store, frames.StoredVideo, about 1/18 of the bytes, or as folders, frames.FolderVideo): a batch then first decodes, on the
GPU, exactly the frames it draws (frames.gather_frames).

What is the same: the dataset filters and order, the doubling of ``frames`` and ``gamma_tau``, the random draws of a
training sample in the reference's order from Python's ``random``, the label window at stride 1 under frames at stride
``gamma_tau``, the testing windows including ``step == 0``, the zero padding and masks of the collate function, and
every output bit (Pillow's bilinear resample included).

What differs (MI355X-first): a batch is made at once, by the kernels of libx3ddata.so (x3dhip/dataops.py) -- two launches
for the clips and one for the labels, whatever the batch size -- and the per-frame labels are never dense on the host:
the annotations live on the device as frame ranges (make_dataset builds that table once, with the reference's own
double-precision expression), under 1 MB for the whole annotation file instead of about 4.5 GB of float arrays.

    ds = Charades('data/charades.json', 'training', videos, task='loc')
    clips, labels, masks = ds.batch([0, 5, 9])          # straight into Trainer(objective='loc').train_step(clips, labels)
"""
import json
import random as _random

import numpy as np
import torch

from frames import gather_frames, is_lazy
from x3dhip import dataops
from x3dhip.clip_input import center_crop_box

CHARADES_MEAN = [0.413, 0.368, 0.338]           # train_x3d_charades.py:48
CHARADES_STD = [0.131, 0.125, 0.132]            # :49
MIN_FRAMES = 2 * 80 + 2                         # charades.py:88


def annotation_ranges(num_frames, duration, actions):
    """Half-open 0-based frame ranges [lo, hi) on which each annotation (class, start, end) is on, by the reference's
    expression (charades.py:93-97):  fps = num_frames / duration;  frame fr is on iff fr / fps > start and fr / fps < end
    (both strict).  fr / fps is monotonic in fr, so the frames that are on are contiguous; the bounds are found by
    searching the exact double-precision values fr / fps, not by algebra on start * fps (a frame time that equals a bound
    decides labels).  An annotation with start >= end gives an empty range (lo == hi)."""
    fps = num_frames / duration
    times = np.arange(num_frames) / fps                     # the same IEEE division as the reference's fr / fps
    out = []
    for a in actions:
        lo = int(np.searchsorted(times, float(a[1]), side="right"))     # first frame with fr / fps > start
        hi = int(np.searchsorted(times, float(a[2]), side="left"))      # first frame with fr / fps >= end
        out.append((lo, max(lo, hi)))
    return out


def make_dataset(split_file, split, videos, num_classes=157):
    """charades.py:68-104.  split_file: the annotation file's path, or its dict.  videos: {video id: uint8 CUDA tensor
    [n_frames, H, W, 3], or a lazy video of frames.py}.  Keeps the reference's filters (the subset, the video present,
    n_frames >= 162) and order.
    Returns (entries, table): entries [(vid, duration, n_frames)], table the device annotation table over them
    (dataops.AnnotationTable; video v of the table is entries[v])."""
    if isinstance(split_file, dict):
        data = split_file
    else:
        with open(split_file, "r") as f:
            data = json.load(f)
    entries, off, cls, lo, hi = [], [0], [], [], []
    device = None
    for vid in data.keys():
        if data[vid]["subset"] != split:
            continue
        if vid not in videos:
            continue
        v = videos[vid]
        if not is_lazy(v):
            if not isinstance(v, torch.Tensor) or not v.is_cuda or v.dtype != torch.uint8 or not v.is_contiguous():
                raise ValueError("frames must be contiguous uint8 tensors on a CUDA(HIP) device (video %s)" % vid)
            if v.dim() != 4 or v.shape[3] != 3:
                raise ValueError("frames must be [T, H, W, 3] (video %s)" % vid)
        if device is None:
            device = v.device
        elif v.device != device:
            raise ValueError("frames must be contiguous uint8 tensors on %s (video %s is on %s)" % (device, vid, v.device))
        num_frames = v.shape[0]
        if num_frames < MIN_FRAMES:
            continue
        acts = data[vid]["actions"]
        for a in acts:
            if not 0 <= int(a[0]) < num_classes:
                raise ValueError("class %s of video %s outside [0, %d)" % (a[0], vid, num_classes))
        for a, (l, h) in zip(acts, annotation_ranges(num_frames, data[vid]["duration"], acts)):
            cls.append(int(a[0]))
            lo.append(l)
            hi.append(h)
        off.append(len(cls))
        entries.append((vid, data[vid]["duration"], num_frames))
    if not entries:
        raise ValueError("empty split: no video of subset %r with at least %d frames" % (split, MIN_FRAMES))
    print('dataset size:%d' % len(entries))
    return entries, dataops.AnnotationTable(off, cls, lo, hi, device, n_frames=[e[2] for e in entries])


def draw_train_params(n_frames, width, height, frames, scales, rng=_random):
    """The random draws of one training __getitem__ in the reference's order: start_f (charades.py:136), then
    Compose.randomize_parameters (:146) -- scale index, tl_x, tl_y (spatial_transforms.py:497-501) and the flip's p
    (:348-349)."""
    start_f = rng.randint(1, n_frames - (frames + 1))
    scale = scales[rng.randint(0, len(scales) - 1)]
    tl_x = rng.random()
    tl_y = rng.random()
    p = rng.random()
    crop = int(min(width, height) * scale)
    return dict(start_f=start_f, scale=scale, tl_x=tl_x, tl_y=tl_y, p=p, crop=crop, x1=int(tl_x * (width - crop)),
                y1=int(tl_y * (height - crop)), flip=p < 0.5)


def testing_windows(n_strided, window, crops):
    """charades.py:150-157: (step, window starts) of the `crops` windows of `window` frames over n_strided frames."""
    if crops < 2:
        raise ValueError("the 'class' testing batch needs crops >= 2 (the reference divides by crops - 1)")
    step = int((n_strided - 1 - window) // (crops - 1))
    if step < 0:
        raise ValueError("video of %d strided frames is too short for %d-frame testing windows" % (n_strided, window))
    return step, ([0] * crops if step == 0 else list(range(0, step * crops, step)))


class Charades:
    """charades.py:107-164 over device-resident videos.  `batch(indices)` is the training batch, `test_batch(indices)`
    the testing one (with custom_collate_fn's padding for task 'loc'); both return tensors on the videos' device.

    crop_size is the output size of the testing transform (CenterCropScaled(crop_size)).  c_size is what the reference
    passes to randomize_parameters, which becomes the output size of the training crop: a hard-coded 224 whatever the
    model version (charades.py:146) -- so 'S' and 'XL' train at 224 in the reference too.  That quirk is kept as the
    default; pass c_size to change it."""

    def __init__(self, split_file, split, videos, task='class', frames=80, gamma_tau=5, crops=1, crop_size=224,
                 scales=(224 / 256., 224 / 256.), mean=CHARADES_MEAN, std=CHARADES_STD, c_size=224, rng=_random,
                 num_classes=157):
        if task not in ('class', 'loc'):
            raise ValueError("task must be 'class' or 'loc' (got %r)" % (task,))
        self.data, self.table = make_dataset(split_file, split, videos, num_classes)
        self.videos = [videos[e[0]] for e in self.data]
        self.split_file = split_file
        self.frames = frames * 2                    # charades.py:114
        self.gamma_tau = gamma_tau * 2              # :115
        self.crops = crops
        self.split = split
        self.task = task
        self.crop_size = int(crop_size)
        self.c_size = int(c_size)
        self.scales = list(scales)
        self.num_classes = num_classes
        self.rng = rng
        self.device = self.table.device
        self._clips = dataops.ClipBatcher(self.device, mean, std)

    def __len__(self):
        return len(self.data)

    def _entries(self, indices):
        indices = [int(i) for i in indices]
        if not indices:
            raise ValueError("empty batch")
        for i in indices:
            if not 0 <= i < len(self.data):
                raise ValueError("index %d outside the dataset of %d videos" % (i, len(self.data)))
        return indices

    def draw(self, index):
        """The draws of one training sample (draw_train_params on this video's geometry)."""
        (index,) = self._entries([index])
        _, H, W, _ = self.videos[index].shape
        return draw_train_params(self.data[index][2], W, H, self.frames, self.scales, self.rng)

    def batch(self, indices, params=None):
        """Training batch (charades.py:135-148): (clips [B, 3, T, c, c], labels [B, K]) for task 'class',
        (clips, labels [B, K, frames], masks [B, frames] of ones) for 'loc'; T = frames / gamma_tau (16).  params: the
        draws per sample (default: drawn here, sample by sample in batch order)."""
        indices = self._entries(indices)
        if params is None:
            params = [self.draw(i) for i in indices]
        B, S = len(indices), self.c_size
        T = len(range(0, self.frames, self.gamma_tau))
        clips = torch.empty((B, 3, T, S, S), dtype=torch.float32, device=self.device)
        samples, jobs = [], []
        for b, (i, p) in enumerate(zip(indices, params)):
            first = p["start_f"] - 1
            if first < 0 or first + self.frames > self.data[i][2]:
                raise ValueError("frame index outside the video")
            samples.append(dict(frames=self.videos[i], frame_idx=range(first, first + self.frames, self.gamma_tau),
                                x1=p["x1"], y1=p["y1"], crop=p["crop"], flip=p["flip"], dst_off=b * 3 * T * S * S,
                                dst_cs=T * S * S, dst_ts=S * S))
            jobs.append((i, first, self.frames))                    # labels at stride 1 (:140)
        gather_frames(samples)                                      # lazy videos -> the frames drawn, decoded
        self._clips(clips, samples, S)
        return (clips,) + self._labels(jobs, self.frames)

    def test_batch(self, indices):
        """Testing batch (charades.py:131-133,150-159): the whole video at stride gamma_tau from frame 1, CenterCropScaled,
        no flip.  Task 'loc': what custom_collate_fn returns -- (clips [B, 3, Tmax, S, S], labels [B, K, TLmax],
        masks [B, TLmax]), zero-padded.  Task 'class': (clips [B, crops, 3, T, S, S], labels [B, K]) with the window
        starts of :150-157."""
        indices = self._entries(indices)
        B, S = len(indices), self.crop_size
        strided = [list(range(0, self.data[i][2], self.gamma_tau)) for i in indices]
        samples = []
        if self.task == 'class':
            F = self.frames // self.gamma_tau
            clips = torch.empty((B, self.crops, 3, F, S, S), dtype=torch.float32, device=self.device)
            for b, i in enumerate(indices):
                step, _ = testing_windows(len(strided[b]), F, self.crops)
                x1, y1, crop = center_crop_box(self.videos[i].shape[2], self.videos[i].shape[1])
                samples.append(dict(frames=self.videos[i], frame_idx=strided[b][:(self.crops - 1) * step + F], x1=x1,
                                    y1=y1, crop=crop, flip=False, dst_off=b * self.crops * 3 * F * S * S,
                                    dst_cs=F * S * S, dst_ts=S * S, dst_ws=3 * F * S * S, nwin=self.crops, win_step=step,
                                    win_len=F))
        else:
            Tmax = max(len(s) for s in strided)
            clips = torch.empty((B, 3, Tmax, S, S), dtype=torch.float32, device=self.device)
            for b, i in enumerate(indices):
                x1, y1, crop = center_crop_box(self.videos[i].shape[2], self.videos[i].shape[1])
                samples.append(dict(frames=self.videos[i], frame_idx=strided[b], x1=x1, y1=y1, crop=crop, flip=False,
                                    dst_off=b * 3 * Tmax * S * S, dst_cs=Tmax * S * S, dst_ts=S * S, Tpad=Tmax))
        gather_frames(samples)                                      # lazy videos -> the frames drawn, decoded
        self._clips(clips, samples, S)
        jobs = [(i, 0, self.data[i][2]) for i in indices]
        return (clips,) + self._labels(jobs, max(j[2] for j in jobs))

    def _labels(self, jobs, TLmax):
        loc = self.task == 'loc'
        labels, masks, cls = dataops.charades_labels(self.table, jobs, self.num_classes, TLmax, labels=loc, masks=loc,
                                                     cls=not loc)
        return (labels, masks) if loc else (cls,)
