"""Golden vectors of the Charades dataset, produced by the REFERENCE's own classes (charades.py Charades / make_dataset /
custom_collate_fn and transforms/spatial_transforms.py, which call PIL) on synthetic uint8 frames.
Run in the build container only:   python tests/golden/make_golden_charades.py
Fixtures are data only:
  charades_anno.json    a subset of the reference's annotation file (ids, subset, duration, actions), in its order
  charades_cases.json   per fixture video the frame count, frame size and frames' seed; which video covers which case
  charades_dense.npz    the dense labels of make_dataset for every fixture video, bit-packed
  charades_{class,loc}_{training,testing}.npz   __getitem__ outputs, the draws made, one custom_collate_fn batch
"""
import json
import os
import random
import sys
import tempfile
import types

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "x3d-multigrid_amd"))
from x3dhip.synthetic import synthetic_frames_u8 as frames_u8  # noqa: E402

# h5py, cv2 and torchvision are imported by the reference's charades.py and used for nothing beyond the loader lookup
for _name in ("h5py", "cv2", "torchvision"):
    sys.modules[_name] = types.ModuleType(_name)
sys.modules["torchvision"].set_image_backend = lambda name: None
sys.modules["torchvision"].get_image_backend = lambda: "PIL"
sys.path.insert(0, REF)
sys.modules.pop("charades", None)
import charades as ref  # noqa: E402
from transforms import spatial_transforms as st  # noqa: E402
assert os.path.dirname(os.path.abspath(ref.__file__)) == REF

MEAN = [0.413, 0.368, 0.338]
STD = [0.131, 0.125, 0.132]
SCALES = [224 / 256., 224 / 320.]           # two different scales, so that the scale draw shows
C_SIZE = 32                                 # training output (the reference passes 224; forwarded small, see SmallCompose)
S_LOC, S_CLS = 24, 16                       # testing outputs
FPS = 24

# video -> the cases it is in the fixture for (the host test asserts each is really present)
VIDEOS = {
    "BJI1D": ["exact_bound", "end_past_duration"], "7K163": ["exact_bound"], "O1NO0": [], "PHIRP": [], "P36OC": [],
    "00SL4": ["start_ge_end"], "AKKWU": ["start_ge_end"], "GWLAI": ["same_class_overlap"], "K1X2C": ["same_class_overlap"],
    "TKEKQ": ["no_action"], "14YU9": ["no_action"], "QGHR6": ["dropped_short"], "IADJE": ["dropped_short"],
    "MJPAH": ["exact_bound", "end_past_duration", "step0"], "7RDSV": ["step0"], "WZZPC": [], "CBZEP": [],
    "HYOQB": ["same_class_overlap", "step0"], "O7YEF": ["same_class_overlap"], "BVDB6": ["no_action"], "UG8WG": ["no_action"],
    "RSRK7": ["dropped_short"], "N3U9S": ["step2"], "DPLMM": [], "XNGAV": ["step1"],
}
SIZES = [(36, 48), (48, 36), (40, 40), (36, 52)]
TRAIN_BATCHES = [(1, ["BJI1D"]), (2, ["00SL4", "GWLAI", "TKEKQ"]), (3, ["K1X2C", "AKKWU"]), (4, ["7K163", "14YU9", "P36OC", "O1NO0"])]
TEST_CLASS = ["MJPAH", "XNGAV", "N3U9S"]
TEST_LOC = ["HYOQB", "BVDB6"]
COLLATE = ["MJPAH", "N3U9S", "O7YEF", "UG8WG"]      # four videos of different lengths


class SmallCompose(st.Compose):
    """randomize_parameters(224) of charades.py:146 forwards a small c_size; the draws are unchanged."""

    def randomize_parameters(self, c_size=0):
        super().randomize_parameters(C_SIZE)


def main():
    full = json.load(open(os.path.join(REF, "data", "charades.json")))
    anno = {v: full[v] for v in full if v in VIDEOS}
    assert len(anno) == len(VIDEOS)
    with open(os.path.join(HERE, "charades_anno.json"), "w") as f:
        json.dump(anno, f, separators=(",", ":"))
    meta = {}
    for i, v in enumerate(anno):
        h, w = SIZES[i % len(SIZES)]
        meta[v] = dict(n_frames=int(round(FPS * anno[v]["duration"])), h=h, w=w, seed=100 + i)
    cases = {}
    for v, cs in VIDEOS.items():
        for c in cs:
            cases.setdefault(c, []).append(v)
    cases["different_lengths"] = COLLATE
    with open(os.path.join(HERE, "charades_cases.json"), "w") as f:
        json.dump(dict(fps=FPS, videos=meta, cases=cases, scales=SCALES, c_size=C_SIZE, s_loc=S_LOC, s_cls=S_CLS,
                       mean=MEAN, std=STD), f, indent=1)

    tmp = tempfile.mkdtemp()
    root = os.path.join(tmp, "rgb")
    for v, m in meta.items():
        os.makedirs(os.path.join(root, v))
        for i in range(1, m["n_frames"] + 1):
            open(os.path.join(root, v, v + "-" + str(i).zfill(6) + ".jpg"), "w").close()
    split_file = os.path.join(tmp, "charades.json")
    with open(split_file, "w") as f:
        json.dump(anno, f)
    frames = {}

    def fr(v):
        if v not in frames:
            m = meta[v]
            frames[v] = frames_u8(m["n_frames"], m["h"], m["w"], m["seed"])
        return frames[v]

    seen = []

    def loader(image_dir, vid, frame_indices):
        seen.append(list(frame_indices))
        return [Image.fromarray(fr(vid)[i - 1]) for i in frame_indices]

    def dataset(split, task, out):
        if split == "training":
            sp = SmallCompose([st.MultiScaleRandomCropMultigrid(SCALES, 224), st.RandomHorizontalFlip(), st.ToTensor(255),
                               st.Normalize(MEAN, STD)])
        else:
            sp = st.Compose([st.CenterCropScaled(out), st.ToTensor(255), st.Normalize(MEAN, STD)])
        save = np.save
        ref.np.save = lambda *a, **k: None          # the cache write of a ragged list raises on current numpy
        try:
            ds = ref.Charades(split_file, split, root, sp, task=task, frames=80, gamma_tau=5, crops=10)
        finally:
            ref.np.save = save
        ds.loader = loader
        return ds, sp

    # dense labels of make_dataset, both splits
    dense = {}
    for split in ("training", "testing"):
        ds, _ = dataset(split, "loc", S_LOC)
        order = [e[0] for e in ds.data]
        dense["order_" + split] = np.array(order)
        for vid, label, dur, nf in ds.data:
            assert nf == meta[vid]["n_frames"] and label.shape == (157, nf)
            assert set(np.unique(label)) <= {0.0, 1.0}
            dense["bits_" + vid] = np.packbits(label.astype(np.uint8), axis=1)
    np.savez_compressed(os.path.join(HERE, "charades_dense.npz"), **dense)

    for task in ("class", "loc"):
        ds, sp = dataset("training", task, None)
        order = [e[0] for e in ds.data]
        out = dict(batches=np.array(len(TRAIN_BATCHES)))
        for bi, (seed, vids) in enumerate(TRAIN_BATCHES):
            random.seed(seed)
            idx = [order.index(v) for v in vids]
            out["b%d_seed" % bi] = np.array(seed)
            out["b%d_index" % bi] = np.array(idx)
            draws = []
            for si, i in enumerate(idx):
                del seen[:]
                clip, label = ds[i]
                crop_t, flip_t = sp.transforms[0], sp.transforms[1]
                draws.append([seen[0][0], crop_t.scale, crop_t.tl_x, crop_t.tl_y, flip_t.p])
                out["b%d_s%d_clip" % (bi, si)] = clip.numpy().astype(np.float32)
                out["b%d_s%d_label" % (bi, si)] = label.numpy().astype(np.float32)
            out["b%d_draws" % bi] = np.array(draws, dtype=np.float64)      # start_f, scale, tl_x, tl_y, p
        np.savez_compressed(os.path.join(HERE, "charades_%s_training.npz" % task), **out)
        print(task, "training", {k: v.shape for k, v in out.items() if k.endswith("clip")})

    ds, _ = dataset("testing", "class", S_CLS)
    order = [e[0] for e in ds.data]
    out = dict(videos=np.array(TEST_CLASS), index=np.array([order.index(v) for v in TEST_CLASS]))
    for v in TEST_CLASS:
        clips, label = ds[order.index(v)]
        n = len(range(0, meta[v]["n_frames"], 10))
        out["%s_clips" % v] = clips.numpy().astype(np.float32)
        out["%s_label" % v] = label.numpy().astype(np.float32)
        out["%s_step" % v] = np.array((n - 1 - 16) // 9)
    np.savez_compressed(os.path.join(HERE, "charades_class_testing.npz"), **out)
    print("class testing", {k: v.shape for k, v in out.items() if k.endswith("clips")})

    ds, _ = dataset("testing", "loc", S_LOC)
    order = [e[0] for e in ds.data]
    out = dict(videos=np.array(TEST_LOC), index=np.array([order.index(v) for v in TEST_LOC]), collate_videos=np.array(COLLATE),
               collate_index=np.array([order.index(v) for v in COLLATE]))
    for v in TEST_LOC:
        clips, label = ds[order.index(v)]
        out["%s_clips" % v] = clips.numpy().astype(np.float32)
        out["%s_label_bits" % v] = np.packbits(label.numpy().astype(np.uint8), axis=1)
        out["%s_label_shape" % v] = np.array(label.shape)
    batch = ref.custom_collate_fn([ds[order.index(v)] for v in COLLATE])
    out["collate_clips"] = batch[0].numpy().astype(np.float32)
    out["collate_labels_bits"] = np.packbits(batch[1].numpy().astype(np.uint8), axis=2)
    out["collate_labels_shape"] = np.array(batch[1].shape)
    out["collate_masks"] = batch[2].numpy().astype(np.float32)
    assert set(np.unique(batch[1].numpy())) <= {0.0, 1.0}
    np.savez_compressed(os.path.join(HERE, "charades_loc_testing.npz"), **out)
    print("loc testing", out["collate_clips"].shape, out["collate_labels_shape"], out["collate_masks"].shape)
    for f in sorted(os.listdir(HERE)):
        if f.startswith("charades_"):
            print(f, os.path.getsize(os.path.join(HERE, f)))


if __name__ == "__main__":
    main()
