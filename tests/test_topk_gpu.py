"""Top-k classification meter on the GPU (csrc_eval/topk.hip through x3dhip.evalops and topkmeter.TopKMeter) against the
fp64 restatement of tests/topk_ref.py and against the reference's fp32 expression, the tie / NaN / infinity rules, the
sticky flags, growth, graph capture, determinism, and the Kinetics validation end to end: validate_topk against
validate(), run(val_frames=...) on frame folders and test_x3d_kinetics.py on a saved checkpoint."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import jpeg_ref as jr
from tests import parity
from tests import topk_ref as tr
from x3dhip import _evallib, evalops
from x3dhip._lib import X3DHipError

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NAMES = list(tr.CASES)


def _meter(**kw):
    from topkmeter import TopKMeter
    return TopKMeter(**kw)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


_filled = {}


def _case(name):
    """(meter, adds, restated rows per add) of a seeded case, computed once and shared (nothing modifies them)."""
    if name not in _filled:
        adds = tr.make_case(name)
        m = _meter()
        for z, y, n in adds:
            m.add_logits(_t(z), _t(y), n_crops=n)
        _filled[name] = (m, adds, [tr.rows(*a) for a in adds])
    return _filled[name]


def _check_rows(got, want):
    """Integers exact; loss within 1 fp32 ulp of the rounded fp64 value (NaN where it is NaN)."""
    for k in ("rank", "pred", "label", "batch_rows"):
        assert np.array_equal(got[k].numpy(), want[k]), k
    g = got["loss"].numpy()
    w = want["loss"].astype(np.float32)
    assert np.array_equal(np.isnan(g), np.isnan(w))
    ok = ~np.isnan(w)
    assert (np.abs(g[ok].astype(np.float64) - w[ok].astype(np.float64)) <= np.spacing(np.abs(w[ok])).astype(np.float64)).all()


def _rows_as_ref(rows):
    return {k: v.numpy().astype(np.float64) if k == "loss" else v.numpy() for k, v in rows.items()}


@pytest.mark.parametrize("name", NAMES)
def test_kernels_match_the_restatement(name):
    m, adds, want = _case(name)
    K = adds[0][0].shape[1]
    got = m.rows()
    _check_rows(got, {k: np.concatenate([w[k] for w in want]) for k in want[0]})
    tot = m.totals()
    t, _, correct, count = tr.totals(want, K, 5)
    assert np.array_equal(tot["totals"].numpy(), t)
    assert np.array_equal(tot["class_correct"].numpy(), correct) and np.array_equal(tot["class_count"].numpy(), count)
    # the fp64 sums over the rows as the meter stores them (loss rounded to fp32)
    _, ls, _, _ = tr.totals([_rows_as_ref(got)], K, 5)
    assert (np.abs(tot["loss"].numpy() - ls) <= 1e-12 * np.abs(ls)).all(), (tot["loss"].numpy(), ls)


@pytest.mark.parametrize("name", NAMES)
def test_value_matches_the_reference_fp32_expression(name):
    """Counts exact (the margin of tests/test_topk_host.py), cls_loss within the project's 1e-3 relative bound."""
    m, adds, _ = _case(name)
    K = adds[0][0].shape[1]
    corr, top5, losses = 0, 0, []
    for z, y, n in adds:
        loss, c, t5, _ = tr.torch_reference(z, y, n, torch.float32)
        corr, top5 = corr + c, top5 + int(t5.sum())
        losses.append(loss)
    v = m.value()
    videos = sum(len(y) for _, y, _ in adds)
    assert v["videos"] == videos and v["top1"] == corr / videos and v["top5"] == top5 / videos
    want = sum(losses) / len(losses)
    assert abs(v["cls_loss"] - want) <= parity.RTOL * abs(want)
    assert v["class_acc"].shape == (K,) and 0 <= v["mean_class_acc"] <= 1


def test_value_twice_is_bitwise_equal():
    m, _, _ = _case("300x1x400_two_adds")
    a, b = m.totals(), m.totals()
    for k in a:
        assert torch.equal(a[k].view(torch.int64), b[k].view(torch.int64)), k


def test_ties_nan_and_infinities_follow_the_rules():
    K = 300                                             # the tied classes sit in different strides of the workgroup
    g = np.random.RandomState(5)
    z = g.standard_normal((2 * 3, K)).astype(np.float32)
    z[:, 290] = z[:, 17] = z.max(1) + 1.0               # identical in every crop, and the largest
    base = g.standard_normal((1, K)).astype(np.float32)
    neg, nan, inf = base.copy(), base.copy(), base.copy()
    neg[0, 3], nan[0, 200], inf[0, 299] = -np.inf, np.nan, np.inf
    adds = [(z, np.array([290, 17]), 3), (neg, np.array([5]), 1), (nan, np.array([5]), 1), (inf, np.array([5]), 1),
            (np.concatenate([base, nan]), np.array([7]), 2)]
    m = _meter()
    for zz, y, n in adds:
        m.add_logits(_t(zz), _t(y), n_crops=n)
    got = m.rows()
    want = [tr.rows(*a) for a in adds]
    _check_rows(got, {k: np.concatenate([w[k] for w in want]) for k in want[0]})
    assert got["rank"].tolist() == [1, 0, got["rank"][2].item(), K, K, K]
    assert got["pred"].tolist()[:2] == [17, 17] and got["pred"].tolist()[3:] == [-1, -1, -1]
    assert math.isfinite(got["loss"][2]) and got["rank"][2] < K and got["pred"][2] >= 0
    assert torch.isnan(got["loss"][3:]).all()
    tot = m.totals()
    assert tot["totals"].tolist()[0] == 6 and tot["totals"].tolist()[3] == 5 and torch.isnan(tot["loss"]).all()


@pytest.mark.parametrize("bad", [-1, 7])
def test_a_label_outside_the_classes_sets_bad(bad):
    m = _meter()
    z = _t(np.random.RandomState(1).standard_normal((3, 7)).astype(np.float32))
    m.add_logits(z, _t(np.array([2, bad, 0])))
    rows = m.rows()
    assert rows["rank"][1] == 7 and rows["label"][1] == bad and rows["rank"][0] < 7
    t, ls, correct, count = m._totals_device()
    assert t.tolist() == [-1] * 4 and torch.isnan(ls).all()
    with pytest.raises(ValueError, match="label"):
        m.value()
    raw = m.totals(check=False)                        # what reduce_totals takes: the failure travels with the totals
    assert raw["totals"].tolist() == [-1] * 4 and torch.isnan(raw["loss"]).all() and isinstance(raw["error"], ValueError)
    m.reset()
    m.add_logits(z, _t(np.array([2, 1, 0])))
    assert m.value()["videos"] == 3


def test_argument_checks():
    m = _meter()
    with pytest.raises(TypeError):
        m.add_logits(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError):
        m.add_logits(torch.zeros(3, 4, device=DEV), torch.zeros(2, dtype=torch.int64), n_crops=2)
    with pytest.raises(ValueError):
        m.add_logits(torch.zeros(2, 4, device=DEV), torch.zeros(2))
    with pytest.raises(ValueError, match="up to"):
        m.add_logits(torch.zeros(2, _evallib.CLS_MAX_K + 1, device=DEV), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="up to"):
        m.add_logits(torch.zeros(_evallib.CLS_MAX_CROPS + 1, 4, device=DEV), torch.zeros(1, dtype=torch.int64),
                     n_crops=_evallib.CLS_MAX_CROPS + 1)
    state, rows = evalops.ap_state(DEV, 8), evalops.cls_rows(DEV, 8)
    with pytest.raises(X3DHipError):
        evalops.cls_append_crops(state, rows, torch.zeros(2, _evallib.CLS_MAX_K + 1, device=DEV),
                                 torch.zeros(2, dtype=torch.int64, device=DEV), 1)
    # the library's own limits (the wrappers check first, so call it directly)
    from x3dhip._lib import ptr, stream
    lg, lb = torch.zeros(40, 8, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    rc = _evallib.lib().x3deval_cls_append_crops(ptr(state), *[ptr(r) for r in rows], 8, ptr(lg), ptr(lb), 1, 40, stream())
    assert rc == -1
    m.add_logits(torch.zeros(2, 4, device=DEV), [1, 2])
    with pytest.raises(ValueError, match="classes"):
        m.add_logits(torch.zeros(2, 5, device=DEV), [1, 2])


def test_overflow_on_the_device_writes_nothing():
    state, rows = evalops.ap_state(DEV, 4), evalops.cls_rows(DEV, 4)
    for r in rows[1:]:
        r.fill_(-7)
    z, y, n = tr.make_case("3x3x7")[0]
    evalops.cls_append_crops(state, rows, _t(z), _t(y), n)
    evalops.cls_append_crops(state, rows, _t(z), _t(y), n)          # 3 + 3 > 4: dropped
    st = state.cpu()
    assert st[_evallib.S_COUNT] == 3 and st[_evallib.S_OVERFLOW] == 1 and st[_evallib.S_BATCHES] == 1
    assert rows[1][3].item() == -7 and rows[4].tolist() == [3, 3, 3, -7]
    t, ls, _, _ = evalops.cls_value(state, rows, 7, 5)
    assert t.tolist() == [-1] * 4 and torch.isnan(ls).all()


def test_growth_keeps_the_earlier_rows():
    import topkmeter
    z, y, n = tr.make_case("64x3x400")[0]
    m = _meter()
    reps = topkmeter._MIN_CAPACITY // 64 + 3                        # past the first capacity: the buffers grow
    for _ in range(reps):
        m.add_logits(_t(z), _t(y), n_crops=n)
    assert m._cap > topkmeter._MIN_CAPACITY
    got = m.rows()
    want = _case("64x3x400")[2][0]
    assert got["rank"].shape[0] == 64 * reps
    for k in ("rank", "pred", "label", "batch_rows"):
        assert np.array_equal(got[k].numpy(), np.tile(want[k], reps)), k
    assert torch.equal(got["loss"].view(torch.int32), got["loss"][:64].repeat(reps).view(torch.int32))
    assert m.totals()["totals"].tolist()[3] == reps


def test_graph_replays_equal_eager_and_overflow_raises():
    z, y, n = tr.make_case("3x3x7")[0]
    z, y = _t(z), _t(y)
    eager = _meter()
    for _ in range(4):
        eager.add_logits(z, y, n_crops=n)
    m = _meter()
    m.add_logits(z, y, n_crops=n)                                   # eager first add: the buffers exist before the capture
    m.reserve(12)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            m.add_logits(z, y, n_crops=n)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    a, b = m.rows(), eager.rows()
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    ta, tb = m.totals(), eager.totals()
    for k in ta:
        assert torch.equal(ta[k].view(torch.int64), tb[k].view(torch.int64)), k
    for _ in range((m._cap - 12) // 3 + 1):                         # past the capacity: nothing is written, value() raises
        graph.replay()
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="reserve"):
        m.value()


def test_growth_inside_capture_raises_and_growth_after_retires_the_state():
    z, y, n = tr.make_case("3x3x7")[0]
    z, y = _t(z), _t(y)
    m = _meter()
    m.add_logits(z, y, n_crops=n)
    torch.cuda.synchronize()
    big = torch.zeros((m._cap * 2, 7), device=DEV)
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with pytest.raises(RuntimeError, match="reserve"):
        with torch.cuda.stream(s):
            with torch.cuda.graph(graph, stream=s):
                m.add_logits(big, torch.zeros(big.shape[0], dtype=torch.int64, device=DEV))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            m.add_logits(z, y, n_crops=n)
    torch.cuda.current_stream().wait_stream(s)
    graph.replay()
    old = m._state
    m.reserve(m._cap * 2)                                           # growth after a capture: a new state, the old one retired
    assert m._state is not old and m._retired and int(old[_evallib.S_CAPACITY]) == 0
    assert m.value()["videos"] == 6
    graph.replay()                                                  # appends nothing, and is reported
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="capture again"):
        m.value()


# --------------------------------------------------------------------------- the validation phase
def test_validate_topk_equals_validate_on_the_oracle_fixture():
    """The fixture of tests/test_train_gpu.py:test_validate_matches_oracle_multi_crop: videos, the top-1 count and cls_loss
    equal validate()'s on the same batches (count exact, loss 1e-3); top5 equals the restatement on the model's logits."""
    import x3d as resnet_x3d
    import train_x3d_kinetics_multigrid as tk
    from oracle import x3d_oracle as xo
    from x3dhip import synthetic
    S = 2
    sd = synthetic.procedural_state_dict(xo.state_template("M", 400, S), 3)
    for k in list(sd):
        if "split_bn.running_mean" in k:
            sd[k] = sd[k] + 0.05 * torch.randn(sd[k].shape, generator=torch.Generator().manual_seed(len(k)))
        if "split_bn.running_var" in k:
            sd[k] = sd[k] * (1 + 0.2 * torch.rand(sd[k].shape, generator=torch.Generator().manual_seed(len(k) + 1)))
    model = resnet_x3d.generate_model(x3d_version="M", n_classes=400, dropout=0.5, base_bn_splits=S)
    model.load_state_dict(sd)
    model.to(DEV)
    b, n, T, H = 2, 3, 4, 48
    batches = []
    for i in range(2):
        x = synthetic.synthetic_clips(b * n, T, H, H, seed=50 + i).view(b, n, 3, T, H, H)
        y = synthetic.synthetic_labels(b, seed=60 + i).view(b)
        batches.append((x.to(DEV), y.to(DEV)))
    loss, acc, seen = tk.validate(model, batches)
    res = tk.validate_topk(model, batches)
    assert not model.training
    assert res["videos"] == seen == 2 * b
    assert res["top1"] * res["videos"] == acc * seen
    assert abs(res["cls_loss"] - loss) <= parity.RTOL * abs(loss)
    with torch.no_grad():
        rows = [tr.rows(model(x.view(b * n, 3, T, H, H)).view(b * n, 400).cpu().numpy(), y.cpu().numpy(), n)
                for x, y in batches]
    want = tr.value(rows, 400, 5)
    assert res["top5"] == want["top5"] and res["top1"] == want["top1"]
    assert abs(res["loss_per_video"] - want["loss_per_video"]) <= 1e-6 * abs(want["loss_per_video"])


def _val_folders(tmp_path):
    """The reference's layout for subset 'validate' (kinetics.py:74-158): <root>/<label with _>/<video id>/frame_%05d.jpg,
    an annotation json and a label file.  Two videos of 82 frames (make_dataset skips 81 or fewer): the 12 frames of
    tests/golden/jpeg_cases.npz over and over.  Class indices 3 and 5."""
    import frames
    cases = jr.load_cases()
    root = tmp_path / "val"
    for label, vid in (("class a", "vidA"), ("class b", "vidB")):
        path = root / label.replace(" ", "_") / vid
        os.makedirs(str(path))
        for t in range(82):
            with open(str(path / frames.FRAME_NAME.format(t + 1)), "wb") as f:
                f.write(cases["vid_%02d" % (t % 12)][0])
    anno = {"vidA": {"subset": "validate", "annotations": {"label": "class a"}},
            "vidB": {"subset": "validate", "annotations": {"label": "class b"}},
            "vidC": {"subset": "train", "annotations": {"label": "class b", "segment": [0, 10]}}}
    anno_path, labels_path = str(tmp_path / "val.json"), str(tmp_path / "labels.txt")
    with open(anno_path, "w") as f:
        json.dump(anno, f)
    with open(labels_path, "w") as f:
        f.write("\n".join(["c0", "c1", "c2", "class a", "c4", "class b"]) + "\n")
    return str(root), anno_path, labels_path


def _short_val_set(tmp_path):
    """kinetics.Kinetics over two folders holding the 12-frame video of tests/golden/jpeg_cases.npz: windows of 5 frames at
    stride 2 (too short for the reference's listing, which skips 81 frames or fewer, so through from_dataset)."""
    import frames
    import kinetics
    cases = jr.load_cases()
    paths = []
    for v in range(2):
        path = str(tmp_path / ("short%d" % v))
        os.makedirs(path)
        for t in range(12):
            with open(os.path.join(path, frames.FRAME_NAME.format(t + 1)), "wb") as f:
                f.write(cases["vid_%02d" % t][0])
        paths.append(path)
    ds = frames.FolderKinetics(paths, [3, 5], sample_duration=10, gamma_tau=2, crop_size=32, device=DEV, threads=2)
    return kinetics.Kinetics.from_dataset(ds, crops=3)


def test_kinetics_batches_equal_val_batch(tmp_path):
    """kinetics.Kinetics built as the reference builds it, and the 12-frame folders through from_dataset (the protocol
    the issue names: sample_duration=10, gamma_tau=2, crops=3, crop_size=32)."""
    import kinetics
    root, anno, labels = _val_folders(tmp_path)
    val = kinetics.Kinetics(root, anno, labels, "validate", sample_duration=80, gamma_tau=5, crops=3, crop_size=32,
                            device=DEV, threads=2)
    assert len(val) == 2 and val.frames == 16
    (clips, y), = list(val.batches(2))
    assert tuple(clips.shape) == (2, 3, 3, 16, 32, 32) and y.tolist() == [3, 5]
    want, _ = val.dataset.val_batch([1], crops=3)
    (c1, y1), = list(val.batches(4, rank=1, world=2))
    assert torch.equal(c1, want) and y1.tolist() == [5]
    clips, y = next(_short_val_set(tmp_path).batches(2))
    assert tuple(clips.shape) == (2, 3, 3, 5, 32, 32) and y.tolist() == [3, 5]


def test_run_validates_on_frame_folders_and_the_script_scores_the_checkpoint(tmp_path, capsys):
    import kinetics
    import train_x3d_kinetics_multigrid as tk
    import test_x3d_kinetics as script
    root, anno, labels = _val_folders(tmp_path)
    prefix = str(tmp_path / "ck_")

    def val_lines():
        lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith(" val after step ")]
        for ln in lines:
            assert "(2 videos)" in ln and "Top5:" in ln
            assert math.isfinite(float(ln.split("Cls Loss: ")[1].split()[0]))
        return len(lines)

    # a ready instance over two short folders (12 frames: windows of 5 frames at stride 2)
    steps, _ = tk.run(batch_size=2, max_steps_run=2, iterations_per_epoch=40, max_epochs=3, val_every=1,
                      val_frames=_short_val_set(tmp_path), use_graph=False, save_every=2,
                      save_model=prefix, clip_size=32, log_every=1)
    assert steps == 2 and val_lines() == 2
    # the annotation files, as the command line passes them
    steps, _ = tk.run(batch_size=2, max_steps_run=1, iterations_per_epoch=40, max_epochs=3, val_every=1,
                      val_frames=dict(root=root, anno=anno, labels=labels, threads=2), use_graph=False, save_every=0,
                      clip_size=32, log_every=1)
    assert steps == 1 and val_lines() == 1
    ckpt = prefix + "000002.pt"
    res = script.main(["--load", ckpt, "--frames-root", root, "--anno", anno, "--labels", labels, "--batch", "2",
                       "--decode-threads", "2"])
    out = capsys.readouterr().out.splitlines()
    assert any(ln.startswith(" Cls Loss: ") for ln in out)
    rec = json.loads(out[-1])
    assert rec["videos"] == 2 and rec["checkpoint"] == ckpt
    val = kinetics.Kinetics(root, anno, labels, "validate", sample_duration=80, gamma_tau=5, crops=3, crop_size=224,
                            device=DEV, threads=2)
    direct = tk.validate_topk(script.load_model(ckpt, "M", DEV), val.batches(2))
    for k in ("videos", "top1", "top5", "cls_loss", "loss_per_video"):
        assert res[k] == direct[k] == rec[k], k
    assert math.isfinite(res["cls_loss"])
