"""CPU restatement of the reference's Charades dataset (charades.py:68-189) for the tests, in the manner of
tests/apmeter_ref.py and tests/bn_ref.py: the brute-force label expression, the draw order of a training sample, the
testing windows and custom_collate_fn.  The pixels come from oracle.input_oracle (Pillow's resample restated in numpy).
tests/test_charades_data_host.py pins all of it to the goldens made by the reference's own classes; the GPU tests then
use it for the shapes no golden covers."""
import json
import os

import numpy as np

from oracle import input_oracle as io
from x3dhip.synthetic import synthetic_frames_u8

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K = 157
MIN_FRAMES = 2 * 80 + 2


def load_fixture():
    """(annotation dict in file order, cases dict) of tests/golden."""
    with open(os.path.join(GOLDEN, "charades_anno.json")) as f:
        anno = json.load(f)
    with open(os.path.join(GOLDEN, "charades_cases.json")) as f:
        cases = json.load(f)
    return anno, cases


_frames = {}


def video_frames(vid, cases):
    m = cases["videos"][vid]
    key = (vid, m["n_frames"], m["h"], m["w"], m["seed"])
    if key not in _frames:
        _frames[key] = synthetic_frames_u8(m["n_frames"], m["h"], m["w"], m["seed"])
    return _frames[key]


def dense_labels(num_frames, duration, actions, num_classes=K):
    """charades.py:91-97, frame by frame: label[c, fr] = 1 iff fr / fps > start and fr / fps < end."""
    label = np.zeros((num_classes, num_frames), np.float32)
    fps = num_frames / duration
    for ann in actions:
        for fr in range(0, num_frames, 1):
            if fr / fps > ann[1] and fr / fps < ann[2]:
                label[ann[0], fr] = 1
    return label


def entries(anno, split, n_frames):
    """make_dataset's filters and order (:80-98): [(vid, duration, n_frames)]; n_frames: {vid: count} of the videos present."""
    out = []
    for vid in anno.keys():
        if anno[vid]["subset"] != split or vid not in n_frames or n_frames[vid] < MIN_FRAMES:
            continue
        out.append((vid, anno[vid]["duration"], n_frames[vid]))
    return out


def draw_train(n_frames, frames, scales, rng):
    """The draws of one training __getitem__ in order: start_f (:136), then Compose.randomize_parameters (:146): the
    crop's scale index, tl_x, tl_y (spatial_transforms.py:497-501), the flip's p (:348-349)."""
    start_f = rng.randint(1, n_frames - (frames + 1))
    scale = scales[rng.randint(0, len(scales) - 1)]
    tl_x = rng.random()
    tl_y = rng.random()
    p = rng.random()
    return start_f, scale, tl_x, tl_y, p


def window_starts(n_strided, window, crops):
    """:150-157."""
    step = int((n_strided - 1 - window) // (crops - 1))
    return step, ([0] * crops if step == 0 else list(range(0, step * crops, step)))


def train_item(video, label, draws, task, c_size, mean, std, frames=160, gamma_tau=10):
    """__getitem__ of the training split with the draws given: (clip [3, T, c, c], label [K] or [K, frames])."""
    start_f, scale, tl_x, tl_y, p = draws
    start_f = int(start_f)
    n, h, w, _ = video.shape
    idx = [i - 1 for i in range(start_f, start_f + frames, gamma_tau) if i <= n]
    x1, y1, crop = io.crop_box(w, h, scale, tl_x, tl_y)
    clip = io.clip(video, idx, x1, y1, crop, c_size, p < 0.5, mean, std)
    lab = label[:, start_f - 1:start_f - 1 + frames]
    if task == "class":
        lab = lab.max(axis=1)
    return clip.astype(np.float32), lab


def test_item(video, label, task, out_size, mean, std, frames=160, gamma_tau=10, crops=10):
    """__getitem__ of the testing split: task 'loc' (clip [3, T_all, S, S], label [K, n]); task 'class'
    (clips [crops, 3, T, S, S], label [K])."""
    n, h, w, _ = video.shape
    idx = list(range(0, n, gamma_tau))
    x1, y1, crop = io.center_crop_box(w, h)
    clip = io.clip(video, idx, x1, y1, crop, out_size, False, mean, std).astype(np.float32)
    if task == "loc":
        return clip, label
    F = frames // gamma_tau
    _, starts = window_starts(len(idx), F, crops)
    return np.stack([clip[:, s:s + F] for s in starts], 0), label.max(axis=1)


test_item.__test__ = False


def collate(batch):
    """custom_collate_fn (:167-189): (clips [B, 3, Tmax, S, S], labels [B, K, TLmax], masks [B, TLmax]), zero-padded."""
    tmax = max(b[0].shape[1] for b in batch)
    lmax = max(b[1].shape[1] for b in batch)
    clips = np.zeros((len(batch), batch[0][0].shape[0], tmax) + batch[0][0].shape[2:], np.float32)
    labels = np.zeros((len(batch), batch[0][1].shape[0], lmax), np.float32)
    masks = np.zeros((len(batch), lmax), np.float32)
    for i, (c, l) in enumerate(batch):
        clips[i, :, :c.shape[1]] = c
        labels[i, :, :l.shape[1]] = l
        masks[i, :l.shape[1]] = 1
    return clips, labels, masks


def unpack_bits(bits, shape):
    return np.unpackbits(bits, axis=-1)[..., :shape[-1]].astype(np.float32).reshape(shape)
