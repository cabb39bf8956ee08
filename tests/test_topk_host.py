"""Top-k classification meter, checks that need no GPU: the fp64 restatement (tests/topk_ref.py) against the reference's
own expression evaluated by torch on the CPU, the tie and NaN rules on hand-made rows, the margin and the hit counts of
every seeded case the GPU tests use, topkmeter.reduce_totals over a 2-process gloo group, and the sharding of
kinetics.Kinetics.batches."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import kinetics
import topkmeter
from tests import topk_ref as tr

NAMES = list(tr.CASES)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_the_reference_expression(name):
    """Per add: top-1 count, predictions and per-video top-5 hits equal torch's in fp64 and in fp32 (the margin of
    test_seeded_cases_have_margin_and_both_outcomes is what makes fp32 safe); the batch-mean loss to 1e-12 (fp64) and to
    1e-5 relative (fp32: K terms of 6e-8 each, far inside)."""
    for logits, labels, n in tr.make_case(name):
        r = tr.rows(logits, labels, n)
        K = logits.shape[1]
        for dtype, tol in ((torch.float64, 1e-12), (torch.float32, 1e-5)):
            loss, corr, top5, preds = tr.torch_reference(logits, labels, n, dtype)
            assert corr == int((r["rank"] == 0).sum())
            assert np.array_equal(preds, r["pred"])
            assert np.array_equal(top5, r["rank"] < min(5, K))
            assert abs(r["loss"].mean() - loss) <= tol * abs(loss)


@pytest.mark.parametrize("name", NAMES)
def test_seeded_cases_have_margin_and_both_outcomes(name):
    """Relative gap between s[label] and every other class >= 1e-5 (fp32 softmax error is ~1e-7), so that counts computed
    in fp32 and in fp64 agree; top-1 and top-5 counts strictly between 0 and the rows -- wherever that can hold: a case
    of one row has no count strictly inside, and with K <= 5 every row is a top-5 hit."""
    adds = tr.make_case(name)
    K = adds[0][0].shape[1]
    assert min(tr.min_relative_gap(*a) for a in adds) >= tr.MIN_GAP
    t, _, correct, count = tr.totals([tr.rows(*a) for a in adds], K, 5)
    assert t[0] == sum(b for b, _, _ in tr.CASES[name]) and t[3] == len(adds)
    assert count.sum() == t[0] and correct.sum() == t[1]
    if t[0] >= 2:
        assert 0 < t[1] < t[0]
        if K > 5:
            assert 0 < t[2] < t[0]


def test_tie_rule():
    # classes 1 and 3 tie in every crop: the lower index ranks first and is the prediction
    z = np.array([[0.0, 2.0, 1.0, 2.0], [1.0, 3.0, 0.0, 3.0]], np.float32)
    later = tr.rows(z, [3], 2)
    assert later["rank"][0] == 1 and later["pred"][0] == 1
    earlier = tr.rows(z, [1], 2)
    assert earlier["rank"][0] == 0 and earlier["pred"][0] == 1
    assert later["loss"][0] == earlier["loss"][0]
    # all equal: rank = label, prediction 0
    r = tr.rows(np.zeros((1, 5), np.float32), [4], 1)
    assert r["rank"][0] == 4 and r["pred"][0] == 0 and r["loss"][0] == pytest.approx(np.log(5.0))


def test_nan_and_infinity_rules():
    base = np.array([[0.5, 1.5, -0.5]], np.float32)
    # -inf in another class: that class has probability 0, everything stays finite
    z = base.copy()
    z[0, 0] = -np.inf
    r = tr.rows(z, [1], 1)
    assert r["rank"][0] == 0 and r["pred"][0] == 1 and np.isfinite(r["loss"][0])
    assert r["loss"][0] == pytest.approx(np.log(1 + np.exp(-2.0)))
    # NaN anywhere, or +inf (inf - inf in the softmax): s is NaN in every class -> rank K, no prediction, NaN loss
    for bad in (np.nan, np.inf):
        for at in (0, 1):
            z = base.copy()
            z[0, at] = bad
            r = tr.rows(z, [1], 1)
            assert r["rank"][0] == 3 and r["pred"][0] == -1 and np.isnan(r["loss"][0])
    # NaN in one crop of two poisons the video, not its neighbour
    z = np.array([[0.0, 1.0], [np.nan, 0.0], [2.0, 0.0], [1.0, 0.0]], np.float32)
    r = tr.rows(z, [1, 0], 2)
    assert list(r["rank"]) == [2, 0] and list(r["pred"]) == [-1, 0]
    t, ls, correct, count = tr.totals([r], 2, 5)
    assert list(t) == [2, 1, 1, 1] and np.isnan(ls).all() and list(correct) == [1, 0] and list(count) == [1, 1]
    # a label outside [0, K): rank K
    r = tr.rows(base, [3], 1)
    assert r["rank"][0] == 3 and np.isnan(r["loss"][0])
    assert tr.rows(base, [-1], 1)["rank"][0] == 3


def test_value_of_raw_totals():
    tot = {"totals": torch.tensor([4, 1, 3, 2]), "loss": torch.tensor([6.0, 2.5], dtype=torch.float64),
           "class_correct": torch.tensor([1, 0, 0]), "class_count": torch.tensor([2, 0, 2])}
    v = topkmeter.summarise(tot)
    assert v["videos"] == 4 and v["top1"] == 0.25 and v["top5"] == 0.75
    assert v["cls_loss"] == 1.25 and v["loss_per_video"] == 1.5
    assert v["class_acc"][0] == 0.5 and torch.isnan(v["class_acc"][1]) and v["class_acc"][2] == 0
    assert v["mean_class_acc"] == 0.25
    empty = topkmeter.TopKMeter().value()
    assert empty["videos"] == 0 and empty["top1"] == 0 and empty["class_acc"].numel() == 0


def _shard_totals(rank):
    name = "64x3x400" if rank == 0 else "300x1x400_two_adds"
    adds = tr.make_case(name)
    t, ls, correct, count = tr.totals([tr.rows(*a) for a in adds], 400, 5)
    return {"totals": torch.from_numpy(t), "loss": torch.from_numpy(ls), "class_correct": torch.from_numpy(correct),
            "class_count": torch.from_numpy(count)}


def _reduce_worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    mine = _shard_totals(rank)
    keep = {k: v.clone() for k, v in mine.items()}
    res = topkmeter.reduce_totals(mine, dist.group.WORLD)
    assert all(torch.equal(mine[k], keep[k]) for k in keep)            # the caller's totals are left alone
    # a rank without rows joins with zeros
    empty = topkmeter.TopKMeter().totals() if rank == 1 else mine
    res2 = topkmeter.reduce_totals(empty, dist.group.WORLD)
    # a rank whose meter failed (TopKMeter.totals(check=False)): every rank raises, after the collectives
    failed = dict(mine, totals=torch.full((4,), -1), loss=torch.full((2,), float("nan"), dtype=torch.float64),
                  error=ValueError("TopKMeter: an add held a label outside [0, 400)")) if rank == 1 else mine
    try:
        topkmeter.reduce_totals(failed, dist.group.WORLD)
        raised = None
    except (ValueError, RuntimeError) as e:
        raised = "%s: %s" % (type(e).__name__, e)
    torch.save((res, res2, raised), os.path.join(out_dir, "res%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


def test_reduce_totals_two_rank_gloo(tmp_path):
    port = 31500 + (os.getpid() % 2000)
    mp.spawn(_reduce_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    a, b = _shard_totals(0), _shard_totals(1)
    want = topkmeter.summarise({k: a[k] + b[k] for k in a})
    alone = topkmeter.summarise(a)
    for rank in (0, 1):
        res, res2, raised = torch.load(os.path.join(str(tmp_path), "res%d.pt" % rank), weights_only=False)
        assert raised is not None and raised.startswith(("RuntimeError: reduce_totals: the meter of 1 other rank",
                                                         "ValueError: TopKMeter: an add held a label")[rank]), raised
        for got, exp in ((res, want), (res2, alone)):
            assert got["videos"] == exp["videos"] and got["top1"] == exp["top1"] and got["top5"] == exp["top5"]
            assert got["cls_loss"] == exp["cls_loss"] and got["loss_per_video"] == exp["loss_per_video"]
            assert torch.equal(torch.nan_to_num(got["class_acc"], nan=-1.0), torch.nan_to_num(exp["class_acc"], nan=-1.0))
    assert want["videos"] == 64 + 341


class _Listing:
    """val_batch of a dataset of n videos: the indices themselves."""
    sample_duration, gamma_tau = 80, 5

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def val_batch(self, indices, crops=3):
        return list(indices), crops


@pytest.mark.parametrize("n,batch,world", [(11, 4, 1), (11, 3, 2), (10, 2, 4), (3, 2, 4), (8, 8, 2)])
def test_kinetics_batches_cover_every_video_once(n, batch, world):
    ds = kinetics.Kinetics.from_dataset(_Listing(n), crops=3)
    assert len(ds) == n and ds.frames == 16
    seen = []
    for rank in range(world):
        got = list(ds.batches(batch, rank, world))
        mine = [i for idx, _ in got for i in idx]
        assert mine == list(range(rank, n, world))                      # listing order within the shard
        assert all(c == 3 for _, c in got)
        sizes = [len(idx) for idx, _ in got]
        assert all(s == batch for s in sizes[:-1]) and (not sizes or 0 < sizes[-1] <= batch)
        seen += mine
    assert sorted(seen) == list(range(n))
    with pytest.raises(ValueError):
        list(ds.batches(batch, world, world))
    with pytest.raises(ValueError):
        kinetics.Kinetics.from_dataset(_Listing(n), crops=1)


def test_kinetics_constructor_lists_the_subset_like_the_reference(tmp_path, monkeypatch):
    """Kinetics.__init__ through frames.FolderKinetics.from_annotation: the listing (make_dataset: missing folders and
    folders of 81 frames or fewer are skipped) runs for real, the dataset class is a recorder (it would need a GPU)."""
    import frames
    made = {}

    class Recorder(frames.FolderKinetics):
        def __init__(self, folders, labels, **kw):
            made.update(folders=folders, labels=labels, kw=kw)
            self.sample_duration, self.gamma_tau = kw["sample_duration"], kw["gamma_tau"]

        def __len__(self):
            return len(made["folders"])

    class Folder:
        def __init__(self, path):
            self.path = path

    monkeypatch.setattr(kinetics, "FolderKinetics", Recorder)
    monkeypatch.setattr(frames, "FrameFolder", Folder)
    root = tmp_path / "frames"
    for name, n in (("riding a bike/v1", 90), ("riding a bike/short", 81), ("juggling/v2", 82)):
        os.makedirs(str(root / name.replace(" ", "_")))
        for t in range(n):
            open(str(root / name.replace(" ", "_") / frames.FRAME_NAME.format(t + 1)), "wb").close()
    anno = {"v1": {"subset": "validate", "annotations": {"label": "riding a bike"}},
            "short": {"subset": "validate", "annotations": {"label": "riding a bike"}},
            "gone": {"subset": "validate", "annotations": {"label": "juggling"}},
            "v2": {"subset": "validate", "annotations": {"label": "juggling"}},
            "tr": {"subset": "train", "annotations": {"label": "juggling", "segment": [0, 10]}}}
    import json
    anno_path, labels_path = str(tmp_path / "anno.json"), str(tmp_path / "labels.txt")
    json.dump(anno, open(anno_path, "w"))
    open(labels_path, "w").write("juggling\nsomething else\nriding a bike\n")
    ds = kinetics.Kinetics(str(root), anno_path, labels_path, "validate", sample_duration=80, gamma_tau=5, crops=3,
                           crop_size=160, device="cuda:1", threads=3)
    assert len(ds) == 2 and ds.crops == 3 and ds.frames == 16
    assert [f.path for f in made["folders"]] == [str(root / "riding_a_bike" / "v1"), str(root / "juggling" / "v2")]
    assert made["labels"] == [2, 0]
    assert made["kw"] == dict(sample_duration=80, gamma_tau=5, crop_size=160, device="cuda:1", threads=3)
    assert kinetics.Kinetics(str(root), anno, ["juggling", "x", "riding a bike"], "validate").frames == 3     # defaults 16 // 5
    with pytest.raises(ValueError, match="no video"):
        kinetics.Kinetics(str(tmp_path / "nowhere"), anno, ["juggling", "x", "riding a bike"], "validate")


def test_checkpoint_script_passes_its_flags_on(monkeypatch):
    """test_x3d_kinetics.main: the flags reach kinetics.Kinetics and evaluate() (both recorded; the real ones need a GPU)."""
    import test_x3d_kinetics as script
    seen = {}

    def fake_kinetics(*a, **kw):
        seen["ds"] = (a, kw)
        return "dataset"

    def fake_evaluate(load, dataset, **kw):
        seen["ev"] = (load, dataset, kw)
        return {"videos": 0}

    monkeypatch.setattr(script, "Kinetics", fake_kinetics)
    monkeypatch.setattr(script, "evaluate", fake_evaluate)
    monkeypatch.delenv("LOCAL_RANK", raising=False)
    script.main(["--load", "ck.pt", "--frames-root", "R", "--anno", "A", "--labels", "L", "--subset", "testing", "--crops", "4",
                 "--batch", "5", "--version", "S", "--bf16", "--decode-threads", "2"])
    a, kw = seen["ds"]
    assert a == ("R", "A", "L", "testing")
    assert kw == dict(sample_duration=80, gamma_tau=6, crops=4, crop_size=160, device=torch.device("cuda", 0), threads=2)
    assert seen["ev"] == ("ck.pt", "dataset", dict(batch=5, x3d_version="S", act_dtype=torch.bfloat16))
    with pytest.raises(SystemExit):
        script.main(["--load", "ck.pt", "--frames-root", "R"])
