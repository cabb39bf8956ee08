"""Charades input path on the GPU (libx3ddata.so through x3dhip/dataops.py and charades.Charades): labels, masks, clip-level
labels and clips against every golden of tests/golden/charades_*.npz and against tests/charades_ref.py where no golden
reaches, bit for bit (integer and copy kernels plus the three fp32 roundings the input tests already hold exact); guard
bands; the outputs fed unchanged to the Trainer and to charades_eval; run() of the two scripts; the ValueError cases."""
import math
import os
import random

import numpy as np
import pytest
import torch

from tests import charades_ref as cr

pytestmark = pytest.mark.gpu

ANNO, CASES = cr.load_fixture()
META = CASES["videos"]
NF = {v: m["n_frames"] for v, m in META.items()}
MEAN, STD = CASES["mean"], CASES["std"]
SENTINEL = 12345.0


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


_videos_cache = {}


def _videos(dev):
    if dev not in _videos_cache:
        _videos_cache[dev] = {v: torch.from_numpy(cr.video_frames(v, CASES)).to(dev) for v in ANNO}
    return _videos_cache[dev]


def _dataset(dev, split, task, c_size=None, crop_size=None, seed=0, crops=10):
    import charades
    return charades.Charades(ANNO, split, _videos(dev), task=task, frames=80, gamma_tau=5, crops=crops,
                             crop_size=crop_size or (CASES["s_cls"] if task == "class" else CASES["s_loc"]),
                             scales=CASES["scales"], mean=MEAN, std=STD, c_size=c_size or CASES["c_size"],
                             rng=random.Random(seed))


def _npz(name):
    return np.load(os.path.join(cr.GOLDEN, name))


def _dense():
    z = _npz("charades_dense.npz")
    return {k[5:]: cr.unpack_bits(z[k], (cr.K, NF[k[5:]])) for k in z.files if k.startswith("bits_")}


def _bits_equal(got, want):
    """Same shape and the same bit patterns (so that -0.0 is not +0.0)."""
    got = got.detach().cpu().contiguous()
    want = torch.from_numpy(np.ascontiguousarray(want))
    return got.shape == want.shape and got.dtype == want.dtype == torch.float32 and \
        torch.equal(got.view(torch.int32), want.view(torch.int32))


# --------------------------------------------------------------------------- goldens
@pytest.mark.parametrize("task", ["class", "loc"])
def test_training_batches_equal_reference_goldens(task):
    dev = _dev()
    ds = _dataset(dev, "training", task)
    assert [e[0] for e in ds.data] == [e[0] for e in cr.entries(ANNO, "training", NF)]
    z = _npz("charades_%s_training.npz" % task)
    for bi in range(int(z["batches"])):
        index = [int(i) for i in z["b%d_index" % bi]]
        ds.rng.seed(int(z["b%d_seed" % bi]))
        out = ds.batch(index)
        want_clips = np.stack([z["b%d_s%d_clip" % (bi, si)] for si in range(len(index))])
        want_lab = np.stack([z["b%d_s%d_label" % (bi, si)] for si in range(len(index))])
        assert _bits_equal(out[0], want_clips), bi
        assert _bits_equal(out[1], want_lab), bi
        if task == "loc":
            assert len(out) == 3 and _bits_equal(out[2], np.ones((len(index), 160), np.float32))
        else:
            assert len(out) == 2


def test_class_testing_batch_equals_reference_goldens():
    dev = _dev()
    ds = _dataset(dev, "testing", "class")
    z = _npz("charades_class_testing.npz")
    vids = [str(v) for v in z["videos"]]
    index = [int(i) for i in z["index"]]
    clips, labels = ds.test_batch(index)                     # three videos, window steps 0, 1 and 2, in one batch
    assert _bits_equal(clips, np.stack([z[v + "_clips"] for v in vids]))
    assert _bits_equal(labels, np.stack([z[v + "_label"] for v in vids]))
    for b, i in enumerate(index):                            # and one by one
        c1, l1 = ds.test_batch([i])
        assert torch.equal(c1[0], clips[b]) and torch.equal(l1[0], labels[b])


def test_loc_testing_batches_equal_reference_goldens_and_the_padding_is_plus_zero():
    dev = _dev()
    ds = _dataset(dev, "testing", "loc")
    z = _npz("charades_loc_testing.npz")
    for v, i in zip([str(v) for v in z["videos"]], z["index"]):
        clips, labels, masks = ds.test_batch([int(i)])       # B = 1: no padding at all
        assert _bits_equal(clips, z[v + "_clips"][None])
        assert _bits_equal(labels, cr.unpack_bits(z[v + "_label_bits"], tuple(z[v + "_label_shape"]))[None])
        assert _bits_equal(masks, np.ones((1, NF[v]), np.float32))
    vids = [str(v) for v in z["collate_videos"]]
    clips, labels, masks = ds.test_batch([int(i) for i in z["collate_index"]])
    assert _bits_equal(clips, z["collate_clips"])
    assert _bits_equal(labels, cr.unpack_bits(z["collate_labels_bits"], tuple(z["collate_labels_shape"])))
    assert _bits_equal(masks, z["collate_masks"])
    ci, li = clips.cpu().view(torch.int32), labels.cpu().view(torch.int32)
    padded = 0
    for b, v in enumerate(vids):
        t = len(range(0, NF[v], 10))
        assert int(ci[b, :, t:].abs().max() if t < ci.shape[2] else 0) == 0          # +0.0, on the bit pattern
        assert int(li[b, :, NF[v]:].abs().max() if NF[v] < li.shape[2] else 0) == 0
        padded += t < ci.shape[2]
    assert padded >= 2


def test_whole_video_labels_equal_the_reference_dense_labels_for_every_fixture_video():
    dev = _dev()
    dense = _dense()
    for split in ("training", "testing"):
        ds = _dataset(dev, split, "loc")
        order = [e[0] for e in ds.data]
        labels, masks = ds._labels([(i, 0, NF[v]) for i, v in enumerate(order)], max(NF[v] for v in order))
        lc, mc = labels.cpu(), masks.cpu()
        for i, v in enumerate(order):
            assert torch.equal(lc[i, :, :NF[v]], torch.from_numpy(dense[v])), v
            assert float(lc[i, :, NF[v]:].abs().sum()) == 0 and float(mc[i].sum()) == NF[v] == int((mc[i] == 1).sum())
    assert len(dense) == 22


# --------------------------------------------------------------------------- label cases no golden covers
def _guarded(dev, shape, lead):
    """A tensor view of `shape` inside a sentinel-filled buffer, `lead` floats past its (aligned) start."""
    n = int(np.prod(shape))
    buf = torch.full((lead + n + 67,), SENTINEL, dtype=torch.float32, device=dev)
    return buf, buf[lead:lead + n].view(shape)


def _guards_intact(buf, lead, n):
    return bool((buf[:lead] == SENTINEL).all()) and bool((buf[lead + n:] == SENTINEL).all())


def _ref_labels(order, dense, jobs, TLmax):
    labels = np.zeros((len(jobs), cr.K, TLmax), np.float32)
    masks = np.zeros((len(jobs), TLmax), np.float32)
    for b, (i, start, n) in enumerate(jobs):
        labels[b, :, :n] = dense[order[i]][:, start:start + n]
        masks[b, :n] = 1
    return labels, masks, labels.max(axis=2)


@pytest.mark.parametrize("name", ["last_frame", "tl_157", "tl_161_b1", "tl_3", "mixed_annotated_and_not", "tl_160_aligned"])
def test_labels_equal_the_restatement_where_no_golden_reaches(name):
    from x3dhip import dataops
    dev = _dev()
    dense = _dense()
    ds = _dataset(dev, "training", "loc")
    order = [e[0] for e in ds.data]
    un = [i for i, v in enumerate(order) if not ANNO[v]["actions"]]
    an = [i for i, v in enumerate(order) if len(ANNO[v]["actions"]) >= 3]
    assert un and an
    jobs, TLmax = {
        "last_frame": ([(i, NF[order[i]] - 160, 160) for i in an[:3]] + [(an[0], NF[order[an[0]]] - 1, 1)], 160),
        "tl_157": ([(an[0], 3, 157), (an[1], 0, 100), (un[0], 5, 0), (an[2], 40, 121)], 157),
        "tl_161_b1": ([(an[1], 1, 150)], 161),
        "tl_3": ([(an[0], 100, 3), (an[1], 50, 2)], 3),
        "mixed_annotated_and_not": ([(an[0], 0, 162), (un[0], 0, 162), (an[1], 7, 100), (un[-1], 2, 160)], 162),
        "tl_160_aligned": ([(i, 1, 160) for i in range(len(order))], 160),
    }[name]
    want = _ref_labels(order, dense, jobs, TLmax)
    B = len(jobs)
    for lead in (64, 65, 67):                                 # 16-byte aligned rows, and rows that start 4 and 12 bytes off
        bufs = [_guarded(dev, s, lead) for s in ((B, cr.K, TLmax), (B, TLmax), (B, cr.K))]
        got = dataops.charades_labels(ds.table, jobs, cr.K, TLmax, *[v for _, v in bufs])
        for (buf, view), g, w in zip(bufs, got, want):
            assert g is view and _bits_equal(g, w), (name, lead)
            assert _guards_intact(buf, lead, view.numel()), (name, lead)
    # any subset of the outputs; twice the same bits
    l2, m2, c2 = dataops.charades_labels(ds.table, jobs, cr.K, TLmax, labels=False, masks=False)
    assert l2 is None and m2 is None and _bits_equal(c2, want[2])
    l3, m3, c3 = dataops.charades_labels(ds.table, jobs, cr.K, TLmax, cls=False)
    assert c3 is None and _bits_equal(l3, want[0]) and _bits_equal(m3, want[1])
    _, m4, _ = dataops.charades_labels(ds.table, jobs, cr.K, TLmax, labels=False, cls=False)
    assert _bits_equal(m4, want[1])


# --------------------------------------------------------------------------- clips: guards, windows, restatement
def test_clip_batch_leaves_guard_bands_untouched_and_equals_the_restatement():
    from x3dhip import dataops
    dev = _dev()
    vids = ["BJI1D", "GWLAI", "XNGAV"]                       # three frame sizes
    S, Tmax = 20, 9
    lead = 96
    buf, batch = _guarded(dev, (3, 3, Tmax, S, S), lead)
    cb = dataops.ClipBatcher(dev, MEAN, STD)
    samples, want = [], np.zeros((3, 3, Tmax, S, S), np.float32)
    for b, (v, T, flip) in enumerate(zip(vids, (9, 4, 1), (True, False, True))):
        m = META[v]
        crop = min(m["h"], m["w"]) - 3 * b
        idx = list(range(NF[v] - 1, NF[v] - 1 - 7 * T, -7))          # any order, the last frame included
        samples.append(dict(frames=_videos(dev)[v], frame_idx=idx, x1=b, y1=2 * b, crop=crop, flip=flip,
                            dst_off=b * 3 * Tmax * S * S, dst_cs=Tmax * S * S, dst_ts=S * S, Tpad=Tmax))
        want[b, :, :T] = cr.io.clip(cr.video_frames(v, CASES), idx, b, 2 * b, crop, S, flip, MEAN, STD)
    cb(batch, samples, S)
    assert _bits_equal(batch, want)
    assert _guards_intact(buf, lead, batch.numel())
    first = batch.clone()
    cb(batch, samples, S)
    assert torch.equal(first, batch)


def test_ten_window_batch_equals_the_per_window_computation():
    from x3dhip import dataops
    import charades
    dev = _dev()
    ds = _dataset(dev, "testing", "class")
    order = [e[0] for e in ds.data]
    index = list(range(len(order)))
    clips, labels = ds.test_batch(index)                     # every testing video of the fixture
    S, F = ds.crop_size, 16
    cb = dataops.ClipBatcher(dev, MEAN, STD)
    per_window = torch.empty_like(clips)
    samples = []
    for b, v in enumerate(order):
        strided = list(range(0, NF[v], 10))
        _, starts = charades.testing_windows(len(strided), F, 10)
        x1, y1, crop = cr.io.center_crop_box(META[v]["w"], META[v]["h"])
        for j, s in enumerate(starts):                        # one job per window: every frame resized once per window
            samples.append(dict(frames=_videos(dev)[v], frame_idx=strided[s:s + F], x1=x1, y1=y1, crop=crop, flip=False,
                                dst_off=(b * 10 + j) * 3 * F * S * S, dst_cs=F * S * S, dst_ts=S * S))
    cb(per_window, samples, S)
    assert torch.equal(clips.view(torch.int32), per_window.view(torch.int32))
    dense = _dense()
    assert _bits_equal(labels, np.stack([dense[v].max(axis=1) for v in order]))


# --------------------------------------------------------------------------- into the Trainer and charades_eval
def _model(dev, task):
    import x3d
    torch.manual_seed(0)
    net = x3d.generate_model("M", n_classes=400, dropout=0.0, base_bn_splits=1, task=task)
    net.replace_logits(cr.K)
    return net.to(dev).train(True)


@pytest.mark.parametrize("task", ["class", "loc"])
def test_batches_go_unchanged_into_the_trainer_and_the_validation_phases(task):
    import charades_eval
    from x3dhip.trainer import Trainer
    dev = _dev()
    net = _model(dev, task)
    tr = Trainer(net, lr=0.01, momentum=0.9, weight_decay=1e-5, objective="bce" if task == "class" else "loc")
    ds = _dataset(dev, "training", task, c_size=64, seed=3)
    out = ds.batch([0, 5, 7, 9])
    before = tr.fp.flat.clone()
    loss, logits = tr.train_step(out[0], out[1])
    torch.cuda.synchronize()
    assert math.isfinite(float(loss)) and logits.shape == ((4, cr.K, 1) if task == "class" else (4, cr.K, 16))
    assert not torch.equal(before, tr.fp.flat)               # the step trained
    vs = _dataset(dev, "testing", task, crop_size=64)
    batches = [vs.test_batch([0, 1]), vs.test_batch([5])]
    res = (charades_eval.validate_cls if task == "class" else charades_eval.validate_loc)(net, batches)
    assert math.isfinite(res["loss"]) and math.isfinite(res["map"])
    want_rows = 3 if task == "class" else sum(vs.data[i][2] for i in (0, 1, 5))
    assert res["rows"] == want_rows


# --------------------------------------------------------------------------- the scripts
@pytest.mark.parametrize("task", ["class", "loc"])
def test_run_of_the_script_trains_validates_and_checkpoints(task, tmp_path, capsys):
    import charades_train
    import train_x3d_charades
    import train_x3d_charades_loc
    _dev()
    mod = train_x3d_charades if task == "class" else train_x3d_charades_loc
    assert (mod.BS, mod.BS_UPSCALE, mod.INIT_LR) == (16, 2, 0.04)
    assert mod.CHARADES_MEAN == MEAN and mod.CHARADES_STD == STD and mod.CHARADES_DATASET_SIZE == {'train': 7900, 'val': 1850}
    save = str(tmp_path / ("x3d_charades_%s_" % task))
    res = mod.run(init_lr=0.01, max_epochs=2, anno=ANNO, batch_size=4, save_model=save, save_every=4,
                  use_graph=(task == "class"), crop_size=64, c_size=64, dropout=0.5, seed=1)
    assert [p["phase"] for p in res["phases"]] == ["train", "train", "val"]
    assert [p["epoch"] for p in res["phases"]] == [1, 2, 2]
    assert res["steps"] == 6 and res["epochs"] == 2          # 11 training videos in batches of 4, twice
    maps = [m for p in res["phases"][:2] for m in p["maps"]] + [res["phases"][2]["map"]]
    assert len(maps) >= 3 and all(math.isfinite(m) for m in maps)
    assert math.isfinite(res["phases"][2]["loss"]) and res["phases"][2]["rows"] > 0
    assert [os.path.basename(p) for p in res["checkpoints"]] == [os.path.basename(save) + "000004.pt"]
    ck = torch.load(res["checkpoints"][0], map_location="cpu")
    assert sorted(ck) == ["model_state_dict", "optimizer_state_dict", "scheduler_state_dict"]
    assert ck["model_state_dict"]["fc2.weight"].shape[0] == cr.K
    sd = ck["scheduler_state_dict"]
    assert sd["patience"] == 2 and sd["factor"] == 0.1 and sd["mode"] == "min" and sd["last_epoch"] == 0
    assert res["scheduler"].last_epoch == 1 and res["scheduler"].best == res["phases"][2]["loss"]
    from torch.optim.lr_scheduler import ReduceLROnPlateau as TorchPlateau
    theirs = TorchPlateau(torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.01), patience=9)
    theirs.load_state_dict(res["scheduler"].state_dict())
    assert theirs.patience == 2 and theirs.best == res["scheduler"].best
    printed = capsys.readouterr().out
    assert printed.index("train\n") < printed.index("val\n") and " mAP: " in printed and "INIT LR: 0.010000" in printed
    # the checkpoint reloads: model, optimizer and scheduler state, and training goes on from it
    res2 = mod.run(init_lr=0.01, max_epochs=1, anno=ANNO, batch_size=4, save_model=save, save_every=0, use_graph=False,
                   crop_size=64, c_size=64, resume=res["checkpoints"][0], seed=2)
    assert [p["phase"] for p in res2["phases"]] == ["train", "train", "val"] and res2["steps"] == 6
    assert math.isfinite(res2["phases"][2]["map"])
    assert charades_train.ReduceLROnPlateau is type(res2["scheduler"])


# --------------------------------------------------------------------------- invalid input
def test_invalid_input_raises_value_error_before_anything_is_launched(monkeypatch):
    import charades
    from x3dhip import dataops, _datalib
    dev = _dev()
    ds = _dataset(dev, "training", "loc")
    vids = _videos(dev)
    v0 = ds.data[0][0]
    launched = []

    class NoLaunch:
        def __getattr__(self, name):
            def f(*a):
                launched.append(name)
                return 0
            return f
    monkeypatch.setattr(_datalib, "lib", lambda: NoLaunch())
    with pytest.raises(ValueError):
        charades.make_dataset(ANNO, "training", {**vids, v0: vids[v0].cpu()})                # on the host
    with pytest.raises(ValueError):
        charades.make_dataset(ANNO, "training", {**vids, v0: vids[v0].float()})              # wrong dtype
    with pytest.raises(ValueError):
        charades.make_dataset(ANNO, "training", {**vids, v0: vids[v0][:, :, ::2]})           # not contiguous
    with pytest.raises(ValueError):
        charades.make_dataset(ANNO, "validation", vids)                                      # empty split
    with pytest.raises(ValueError):
        charades.make_dataset(ANNO, "training", {v: t for v, t in vids.items() if NF[v] < 162})
    with pytest.raises(ValueError):
        charades.Charades(ANNO, "training", vids, task="detect")
    for bad in ([len(ds)], [-1], [0, 99], []):
        with pytest.raises(ValueError):
            ds.batch(bad)
        with pytest.raises(ValueError):
            ds.test_batch(bad)
    p = ds.draw(0)
    with pytest.raises(ValueError):
        ds.batch([0], [dict(p, x1=META[v0]["w"] - p["crop"] + 1)])                           # crop box outside the frame
    with pytest.raises(ValueError):
        ds.batch([0], [dict(p, crop=0)])
    with pytest.raises(ValueError):
        ds.batch([0], [dict(p, start_f=NF[v0] - 158)])                                       # window past the last frame
    with pytest.raises(ValueError):
        ds.batch([0], [dict(p, start_f=0)])
    with pytest.raises(ValueError):
        _dataset(dev, "testing", "class", crops=1).test_batch([0])
    with pytest.raises(ValueError):
        dataops.charades_labels(ds.table, [(len(ds), 0, 10)], cr.K, 10)
    with pytest.raises(ValueError):
        dataops.charades_labels(ds.table, [(0, 0, 11)], cr.K, 10)
    with pytest.raises(ValueError):
        dataops.charades_labels(ds.table, [(0, 0, 10)], cr.K, 10, labels=torch.zeros(1, cr.K, 10))       # output on the host
    with pytest.raises(ValueError):
        dataops.ClipBatcher(dev, MEAN, STD)(torch.zeros(10, device=dev), [
            dict(frames=vids[v0], frame_idx=[0], x1=0, y1=0, crop=8, flip=False, dst_off=0, dst_cs=16, dst_ts=16)], 4)
    assert launched == []
