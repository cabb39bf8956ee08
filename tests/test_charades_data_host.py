"""Charades input path, checks that need no GPU: the frame ranges of charades.annotation_ranges against the brute-force
expression and the reference's dense labels, the draw order, the testing windows and the collate against the goldens
(tests/golden/charades_*.npz, made by the reference's own classes), tests/charades_ref.py pinned to those goldens bit
for bit, ReduceLROnPlateau against torch's class, and the C ABI of libx3ddata.so (include/x3ddata.h <-> x3dhip/_datalib.py
<-> exports)."""
import os
import random
import re
import subprocess

import numpy as np
import pytest
import torch

import charades
import charades_train
from tests import charades_ref as cr
from x3dhip import _datalib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANNO, CASES = cr.load_fixture()
META = CASES["videos"]
NF = {v: m["n_frames"] for v, m in META.items()}
MEAN, STD = CASES["mean"], CASES["std"]


def _npz(name):
    return np.load(os.path.join(cr.GOLDEN, name))


def _dense_golden():
    z = _npz("charades_dense.npz")
    return z, {k[5:]: cr.unpack_bits(z[k], (cr.K, NF[k[5:]])) for k in z.files if k.startswith("bits_")}


# --------------------------------------------------------------------------- fixture coverage
def test_fixture_cases_are_really_present():
    c = CASES["cases"]
    kept = {s: [e[0] for e in cr.entries(ANNO, s, NF)] for s in ("training", "testing")}
    for v in c["exact_bound"]:
        times = np.arange(NF[v]) / (NF[v] / ANNO[v]["duration"])
        assert any(np.any(times == a[1]) or np.any(times == a[2]) for a in ANNO[v]["actions"]), v
    for v in c["end_past_duration"]:
        assert any(a[2] > ANNO[v]["duration"] for a in ANNO[v]["actions"]), v
    for v in c["start_ge_end"]:
        assert any(a[1] >= a[2] for a in ANNO[v]["actions"]), v
    for v in c["same_class_overlap"]:
        acts = ANNO[v]["actions"]
        rng = charades.annotation_ranges(NF[v], ANNO[v]["duration"], acts)
        assert any(acts[i][0] == acts[j][0] and max(rng[i][0], rng[j][0]) < min(rng[i][1], rng[j][1])
                   for i in range(len(acts)) for j in range(i)), v
    for v in c["no_action"]:
        assert ANNO[v]["actions"] == [] and v in kept[ANNO[v]["subset"]], v
    for v in c["dropped_short"]:
        assert NF[v] < cr.MIN_FRAMES and v not in kept[ANNO[v]["subset"]], v
    for name, step in (("step0", 0), ("step1", 1), ("step2", 2)):
        for v in c[name]:
            assert ANNO[v]["subset"] == "testing"
            assert cr.window_starts(len(range(0, NF[v], 10)), 16, 10)[0] == step, v
    assert len({NF[v] for v in c["different_lengths"]}) == len(c["different_lengths"]) >= 3
    for split in ("training", "testing"):
        assert len(kept[split]) >= 3
    # both tasks and both splits have goldens
    for task in ("class", "loc"):
        for split in ("training", "testing"):
            assert os.path.exists(os.path.join(cr.GOLDEN, "charades_%s_%s.npz" % (task, split)))


# --------------------------------------------------------------------------- frame ranges
def _from_ranges(nf, acts, ranges):
    lab = np.zeros((cr.K, nf), np.float32)
    for a, (lo, hi) in zip(acts, ranges):
        assert 0 <= lo <= hi <= nf
        lab[a[0], lo:hi] = 1
    return lab


def test_frame_ranges_equal_brute_force_and_reference_dense_labels():
    z, dense = _dense_golden()
    for split in ("training", "testing"):
        order = [e[0] for e in cr.entries(ANNO, split, NF)]
        assert order == [str(v) for v in z["order_" + split]]           # make_dataset's filters and order
        for v in order:
            acts = ANNO[v]["actions"]
            got = _from_ranges(NF[v], acts, charades.annotation_ranges(NF[v], ANNO[v]["duration"], acts))
            assert np.array_equal(got, cr.dense_labels(NF[v], ANNO[v]["duration"], acts)), v
            assert np.array_equal(got, dense[v]), v
    assert sorted(dense) == sorted(e[0] for s in ("training", "testing") for e in cr.entries(ANNO, s, NF))


def test_frame_ranges_on_bounds_that_hit_frame_times():
    rng = np.random.default_rng(5)
    for _ in range(40):
        nf = int(rng.integers(162, 400))
        dur = round(float(nf / 24 + rng.uniform(-0.02, 0.02)), 2)
        times = np.arange(nf) / (nf / dur)
        acts = []
        for _ in range(12):
            s, e = sorted(rng.uniform(-1, dur + 3, 2))
            kind = rng.integers(0, 4)
            if kind == 0:
                s = float(times[rng.integers(0, nf)])                   # a start that equals a frame time
            elif kind == 1:
                e = float(times[rng.integers(0, nf)])
            elif kind == 2:
                s, e = e, s                                             # start >= end
            acts.append([int(rng.integers(0, cr.K)), float(s), float(e)])
        got = _from_ranges(nf, acts, charades.annotation_ranges(nf, dur, acts))
        assert np.array_equal(got, cr.dense_labels(nf, dur, acts))


# --------------------------------------------------------------------------- draws, windows, collate, ref == golden
def _train_batches(task):
    z = _npz("charades_%s_training.npz" % task)
    for bi in range(int(z["batches"])):
        yield z, bi, int(z["b%d_seed" % bi]), [int(i) for i in z["b%d_index" % bi]], z["b%d_draws" % bi]


@pytest.mark.parametrize("task", ["class", "loc"])
def test_draw_order_reproduces_the_recorded_draws(task):
    ents = cr.entries(ANNO, "training", NF)
    n = 0
    for z, bi, seed, index, draws in _train_batches(task):
        r1, r2 = random.Random(seed), random.Random(seed)
        for si, i in enumerate(index):
            vid, _, nf = ents[i]
            want = tuple(draws[si])
            assert cr.draw_train(nf, 160, CASES["scales"], r1) == want
            p = charades.draw_train_params(nf, META[vid]["w"], META[vid]["h"], 160, CASES["scales"], r2)
            assert (p["start_f"], p["scale"], p["tl_x"], p["tl_y"], p["p"]) == want
            assert (p["x1"], p["y1"], p["crop"]) == cr.io.crop_box(META[vid]["w"], META[vid]["h"], *want[1:4])
            assert p["flip"] == (want[4] < 0.5)
            n += 1
    assert n >= 8


@pytest.mark.parametrize("task", ["class", "loc"])
def test_ref_training_items_equal_golden_bitwise(task):
    _, dense = _dense_golden()
    ents = cr.entries(ANNO, "training", NF)
    for z, bi, seed, index, draws in _train_batches(task):
        for si, i in enumerate(index):
            vid = ents[i][0]
            clip, lab = cr.train_item(cr.video_frames(vid, CASES), dense[vid], draws[si], task, CASES["c_size"], MEAN, STD)
            g_clip, g_lab = z["b%d_s%d_clip" % (bi, si)], z["b%d_s%d_label" % (bi, si)]
            assert g_clip.shape == (3, 16, CASES["c_size"], CASES["c_size"])
            assert g_lab.shape == ((cr.K,) if task == "class" else (cr.K, 160))
            assert clip.dtype == g_clip.dtype and np.array_equal(clip.view(np.uint32), g_clip.view(np.uint32)), (bi, si)
            assert np.array_equal(lab, g_lab), (bi, si)


def test_ref_class_testing_items_and_window_starts_equal_golden():
    _, dense = _dense_golden()
    z = _npz("charades_class_testing.npz")
    ents = cr.entries(ANNO, "testing", NF)
    steps = set()
    for vid, i in zip([str(v) for v in z["videos"]], z["index"]):
        assert ents[int(i)][0] == vid
        n = len(range(0, NF[vid], 10))
        step, starts = cr.window_starts(n, 16, 10)
        assert step == int(z[vid + "_step"]) and charades.testing_windows(n, 16, 10) == (step, starts)
        assert len(starts) == 10 and starts[-1] + 16 <= n
        steps.add(step)
        clips, lab = cr.test_item(cr.video_frames(vid, CASES), dense[vid], "class", CASES["s_cls"], MEAN, STD)
        g = z[vid + "_clips"]
        assert g.shape == (10, 3, 16, CASES["s_cls"], CASES["s_cls"])
        assert np.array_equal(clips.view(np.uint32), g.view(np.uint32)), vid
        assert np.array_equal(lab, z[vid + "_label"]), vid
    assert {0, 1, 2} <= steps


def test_ref_loc_testing_items_and_collate_equal_golden():
    _, dense = _dense_golden()
    z = _npz("charades_loc_testing.npz")
    ents = cr.entries(ANNO, "testing", NF)

    def item(vid):
        return cr.test_item(cr.video_frames(vid, CASES), dense[vid], "loc", CASES["s_loc"], MEAN, STD)

    for vid, i in zip([str(v) for v in z["videos"]], z["index"]):
        assert ents[int(i)][0] == vid
        clip, lab = item(vid)
        g = z[vid + "_clips"]
        assert g.shape == (3, len(range(0, NF[vid], 10)), CASES["s_loc"], CASES["s_loc"])
        assert np.array_equal(clip.view(np.uint32), g.view(np.uint32)), vid
        assert np.array_equal(lab, cr.unpack_bits(z[vid + "_label_bits"], tuple(z[vid + "_label_shape"]))), vid
    vids = [str(v) for v in z["collate_videos"]]
    assert [ents[int(i)][0] for i in z["collate_index"]] == vids and len(vids) >= 3
    clips, labels, masks = cr.collate([item(v) for v in vids])
    g = z["collate_clips"]
    assert g.shape == (len(vids), 3, max(len(range(0, NF[v], 10)) for v in vids), CASES["s_loc"], CASES["s_loc"])
    assert tuple(z["collate_labels_shape"]) == (len(vids), cr.K, max(NF[v] for v in vids))
    assert z["collate_masks"].shape == (len(vids), max(NF[v] for v in vids))
    assert np.array_equal(clips.view(np.uint32), g.view(np.uint32))
    assert np.array_equal(labels, cr.unpack_bits(z["collate_labels_bits"], tuple(z["collate_labels_shape"])))
    assert np.array_equal(masks, z["collate_masks"])
    assert [int(m.sum()) for m in masks] == [NF[v] for v in vids]


# --------------------------------------------------------------------------- ReduceLROnPlateau vs torch
class _Groups:
    def __init__(self, lr):
        self.param_groups = [dict(lr=lr)]


def test_reduce_lr_on_plateau_follows_torch_step_for_step():
    from torch.optim.lr_scheduler import ReduceLROnPlateau as TorchPlateau
    sgd = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.04)
    theirs = TorchPlateau(sgd, mode='min', patience=2, factor=0.1)
    mine_opt = _Groups(0.04)
    mine = charades_train.ReduceLROnPlateau(mine_opt, mode='min', patience=2, factor=0.1)
    # improvement, an improvement inside the relative threshold (counts as bad), a plateau -> first reduction,
    # a real improvement, a second plateau -> second reduction, then more
    seq = [1.0, 0.99995, 0.99999, 1.0, 1.2, 0.9, 0.9, 0.9, 0.95, 0.9, 0.5, 0.6, 0.6, 0.6, 0.6]
    lrs = []
    for i, m in enumerate(seq):
        theirs.step(m)
        mine.step(m)
        assert mine_opt.param_groups[0]['lr'] == sgd.param_groups[0]['lr'], (i, m)
        assert mine.state_dict() == theirs.state_dict(), (i, m)
        lrs.append(mine_opt.param_groups[0]['lr'])
        if i == 6:                                                    # round trip both ways, mid-sequence
            sd_t, sd_m = theirs.state_dict(), mine.state_dict()
            sgd2 = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=sgd.param_groups[0]['lr'])
            theirs = TorchPlateau(sgd2, mode='min', patience=5, factor=0.5)
            theirs.load_state_dict(sd_m)
            sgd = sgd2
            mine = charades_train.ReduceLROnPlateau(mine_opt, mode='min', patience=7, factor=0.3)
            mine.load_state_dict(sd_t)
            assert mine.state_dict() == theirs.state_dict() == sd_m
    reductions = sum(1 for a, b in zip([0.04] + lrs, lrs) if b < a)
    assert reductions >= 2 and lrs[1] == 0.04
    assert lrs[-1] == pytest.approx(0.04 * 0.1 ** reductions)
    with pytest.raises(ValueError):
        charades_train.ReduceLROnPlateau(mine_opt, factor=1.0)


def test_torch_plateau_rejects_the_trainer_like_object():
    from torch.optim.lr_scheduler import ReduceLROnPlateau as TorchPlateau
    with pytest.raises(TypeError):
        TorchPlateau(_Groups(0.1))


# --------------------------------------------------------------------------- C ABI
def _header_functions():
    src = open(os.path.join(ROOT, "include", "x3ddata.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(x3ddata_[a-z0-9_]+)\s*\(", src)))


def test_data_header_and_ctypes_table_agree():
    assert _header_functions() == sorted(_datalib.SIGNATURES.keys())


def test_data_library_loads_and_exports_every_symbol():
    if not os.path.exists(_datalib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    h = _datalib.lib()
    assert h.x3ddata_abi_version() == _datalib.ABI_VERSION
    out = subprocess.run(["nm", "-D", "--defined-only", _datalib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (x3ddata_[a-z0-9_]+)", out))
    assert set(_header_functions()) == exported
    assert h.x3ddata_label_job_bytes() == _datalib.LABEL_JOB_DT.itemsize == 16
    assert h.x3ddata_clip_job_bytes() == _datalib.CLIP_JOB_DT.itemsize
    # argument checks happen on the host, before any launch
    assert h.x3ddata_charades_labels(None, None, None, None, 0, None, 1, 157, 160, None, None, None, None) == -1
    assert b"argument check failed" in h.x3ddata_last_error()
    assert h.x3ddata_clip_batch(None, 1, None, None, 1, 1, 1, 1, None, None, None) == -1


def test_data_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_datalib, "_lib", None)
    monkeypatch.setattr(_datalib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_datalib.X3DHipError):
        _datalib.lib()


def test_stamp_covers_the_data_library():
    from tools import stamp
    a = stamp.csrc_data_sha16()
    assert re.fullmatch(r"[0-9a-f]{16}", a) and a != stamp.csrc_sha16() and a != stamp.csrc_eval_sha16()


# --------------------------------------------------------------------------- host-side input checks
def test_make_dataset_rejects_host_and_wrong_dtype_videos_before_any_launch():
    vid = cr.entries(ANNO, "training", NF)[0][0]
    with pytest.raises(ValueError):
        charades.make_dataset(ANNO, "training", {vid: torch.zeros((NF[vid], 8, 8, 3), dtype=torch.uint8)})      # on the host
    with pytest.raises(ValueError):
        charades.make_dataset(ANNO, "training", {vid: torch.zeros((NF[vid], 8, 8, 3), dtype=torch.float32)})
    with pytest.raises(ValueError):
        charades.make_dataset(ANNO, "training", {})                                                              # empty split
    with pytest.raises(ValueError):
        charades.testing_windows(20, 16, 1)
    with pytest.raises(ValueError):
        charades.testing_windows(10, 16, 10)
