"""Trainer(skip_nonfinite=True) on the GPU: a clip with one NaN pixel among good ones leaves parameters, momentum and the
split-BN running statistics as they were, in the eager / graph / split-graph / accumulation / RCCL forms of the step, and the
run ends where a twin Trainer that never saw the bad clip ends; the defaults; the flags of the training scripts."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import x3d_oracle as xo
from x3dhip import synthetic

pytestmark = pytest.mark.gpu

CASE = "train_M_2x4x32_s1"          # the smallest fixture: its shape and its weights
LR = 0.05


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _fixture(golden_dir, dev, clips=5):
    """The fixture's weights and labels, `clips` clips of its shape, and the third clip with one NaN pixel."""
    g = np.load(os.path.join(golden_dir, CASE + ".npz"))
    B, T, H, S = [int(v) for v in g["shape"]]
    sd = synthetic.procedural_state_dict(xo.state_template("M", 400, S), int(g["seed"][0]))
    xs = [synthetic.synthetic_clips(B, T, H, H, seed=int(g["seed"][1]) + i).to(dev) for i in range(clips)]
    y = synthetic.synthetic_labels(B, seed=int(g["seed"][1])).to(dev)
    bad = xs[2].clone()
    bad[1, 0, T // 2, H // 2, 3] = float("nan")         # data: an ordinary input, nothing faults
    return sd, S, xs, bad, y


def _trainer(sd, S, dev, **kw):
    import x3d
    from x3dhip.trainer import Trainer
    net = x3d.generate_model("M", n_classes=400, dropout=0.0, base_bn_splits=S)
    net.load_state_dict(sd)
    net.to(dev).train(True)
    return Trainer(net, lr=LR, **kw)


def _running(tr):
    return {k: v.clone() for k, v in tr.model.state_dict().items() if "split_bn.running_" in k}


def _state(tr):
    torch.cuda.synchronize()
    return dict(flat=tr.fp.flat.clone(), mom=tr.fp.mom.clone(), **_running(tr))


def _assert_same(a, b, bitwise=True):
    assert sorted(a) == sorted(b) and len(a) == 2 + 2 * 84
    for k in a:
        assert a[k].shape == b[k].shape, k
        assert torch.equal(a[k], b[k]) if bitwise else bool((a[k] == b[k]).all()), k
        assert bool(torch.isfinite(a[k]).all()), k


def _five_steps(sd, S, dev, xs, bad, y, **kw):
    """Five steps, the third on the bad clip, against a twin that is given only the four good clips."""
    tr = _trainer(sd, S, dev, skip_nonfinite=True, **kw)
    assert tr.monitor.R == 64 and tr.skip_nonfinite
    for i in range(5):
        if i == 2:
            before = _state(tr)
        tr.train_step(bad if i == 2 else xs[i], y)
        if i == 2:
            _assert_same(_state(tr), before)             # parameters, momentum, every split_bn.running_*: untouched
    twin = _trainer(sd, S, dev, **kw)
    for i in (0, 1, 3, 4):
        twin.train_step(xs[i], y)
    _assert_same(_state(tr), _state(twin))
    assert int(tr.monitor.skipped()) == 1 and int(tr.monitor.skip_run()) == 0
    rec = tr.monitor.read()
    assert rec["step"].tolist() == [0, 1, 2, 3, 4]
    assert rec["nonfinite"][2] > 0 and rec["nonfinite"][[0, 1, 3, 4]].tolist() == [0, 0, 0, 0]
    assert tr.monitor.first_nonfinite()[0] == 2
    return tr


@pytest.mark.parametrize("kw", [dict(), dict(use_graph=True), dict(use_graph=True, force_split=True),
                                dict(clip_grad_norm=0.5), dict(use_graph=True, clip_grad_norm=0.5)],
                         ids=["eager", "graph", "split", "eager-clipped", "graph-clipped"])
def test_a_nan_clip_is_skipped_and_the_run_ends_where_the_good_clips_lead(golden_dir, kw):
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev)
    tr = _five_steps(sd, S, dev, xs, bad, y, **kw)
    assert tr._overlap() == bool(kw.get("force_split"))
    if "clip_grad_norm" in kw:
        coef = tr.monitor.read()["coef"]
        assert all(0.0 < c < 1.0 for c in coef[[0, 1, 3, 4]])      # clipping was active on the applied updates


def test_accumulation_skips_the_whole_update_when_its_second_micro_batch_is_bad(golden_dir):
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev, clips=10)
    tr = _trainer(sd, S, dev, skip_nonfinite=True, num_steps_per_update=2)
    for u in range(5):
        if u == 2:
            before = _state(tr)
        tr.train_step(xs[2 * u], y)
        assert not tr.stepped
        tr.train_step(bad if u == 2 else xs[2 * u + 1], y)
        assert tr.stepped
        if u == 2:
            _assert_same(_state(tr), before)
    twin = _trainer(sd, S, dev, num_steps_per_update=2)
    for u in (0, 1, 3, 4):
        twin.train_step(xs[2 * u], y)
        twin.train_step(xs[2 * u + 1], y)
    _assert_same(_state(tr), _state(twin))
    assert int(tr.monitor.skipped()) == 1 and tr.monitor.read()["nonfinite"][2] > 0


def test_one_rank_rccl_group_skips_alike(golden_dir, monkeypatch):
    import torch.distributed as dist
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev)
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", "29541")
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        tr = _five_steps(sd, S, dev, xs, bad, y, use_graph=True, process_group=dist.group.WORLD, world_size=1,
                         force_split=True, force_collectives=True)
        assert tr.reducer.active and tr._overlap()
    finally:
        dist.destroy_process_group()


def test_without_the_guard_the_same_clips_leave_nan_parameters(golden_dir):
    """What the feature is for: the monitor alone reports the step, and the update is applied all the same."""
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev)
    tr = _trainer(sd, S, dev, monitor=True)
    for i in range(5):
        tr.train_step(bad if i == 2 else xs[i], y)
    torch.cuda.synchronize()
    assert tr.monitor.first_nonfinite()[0] == 2
    assert not bool(torch.isfinite(tr.fp.flat).all()) and not bool(torch.isfinite(tr.fp.mom).all())
    assert any(not bool(torch.isfinite(v).all()) for v in _running(tr).values())
    assert not tr.skip_nonfinite


def test_a_skipped_first_step(golden_dir):
    """`first` is a host value: after a skipped first update the next runs with first=False on a momentum of zeros, which
    gives the values of first=True (fmaf(mu, 0, g) == g) and can differ only in the sign of a zero: compared under ==."""
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev)
    tr = _trainer(sd, S, dev, skip_nonfinite=True)
    before = _state(tr)
    tr.train_step(bad, y)
    _assert_same(_state(tr), before)
    assert int(tr.monitor.skipped()) == 1 and int(tr.monitor.skip_run()) == 1
    twin = _trainer(sd, S, dev)
    for i in (0, 1):
        tr.train_step(xs[i], y)
        twin.train_step(xs[i], y)
    _assert_same(_state(tr), _state(twin), bitwise=False)
    assert int(tr.monitor.skip_run()) == 0


def test_a_long_cycle_switch_then_a_bad_step_restores_the_new_buffers(golden_dir):
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev)
    tr = _trainer(sd, S, dev, skip_nonfinite=True, use_graph=True)
    tr.train_step(xs[0], y)
    old_table = tr._keep
    assert tr.model.update_bn_splits_long_cycle(2) == 2 * S
    tr.invalidate_graphs()
    tr.train_step(xs[1], y)                              # the new buffers take their first statistics
    assert tr._keep is not old_table and tr._keep_old is old_table
    live = {id(b) for b in tr._keep.buffers}
    for mod in tr.model.modules():
        if hasattr(mod, "split_bn"):
            assert id(mod.split_bn.running_mean) in live and id(mod.split_bn.running_var) in live
    before = _state(tr)
    tr.train_step(bad, y)
    _assert_same(_state(tr), before)
    assert int(tr.monitor.skipped()) == 1
    tr.train_step(xs[3], y)
    after = _state(tr)
    assert not torch.equal(after["flat"], before["flat"]) and all(bool(torch.isfinite(v).all()) for v in after.values())


def test_defaults_are_off_and_an_all_good_run_is_the_parents(golden_dir):
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev)
    plain = _trainer(sd, S, dev)
    assert not hasattr(plain, "monitor") and not plain.skip_nonfinite and plain._keep is None
    for clip in (None, 0.5):
        parent = _trainer(sd, S, dev, clip_grad_norm=clip) if clip else plain
        guard = _trainer(sd, S, dev, clip_grad_norm=clip, skip_nonfinite=True)
        for i in range(3):
            parent.train_step(xs[i], y)
            guard.train_step(xs[i], y)
        _assert_same(_state(guard), _state(parent))
        assert int(guard.monitor.skipped()) == 0
        a, b = parent.state_dict(), guard.state_dict()
        assert sorted(a) == sorted(b) == ["param_groups", "state"]
        assert sorted(a["param_groups"][0]) == sorted(b["param_groups"][0]) == sorted(
            ["lr", "momentum", "dampening", "weight_decay", "nesterov", "params"])
        assert sorted(a["state"]) == sorted(b["state"]) == list(range(316))
        assert all(list(v) == ["momentum_buffer"] for v in b["state"].values())
        assert all(torch.equal(a["state"][i]["momentum_buffer"], b["state"][i]["momentum_buffer"]) for i in range(316))
    assert plain._keep is None and not hasattr(plain, "monitor")


# -- the scripts ----------------------------------------------------------------------------------------------------------------
def _kinetics_run(capsys, **kw):
    import train_x3d_kinetics_multigrid as tr
    torch.manual_seed(5)
    steps, _ = tr.run(init_lr=0.01, warmup_steps=2, max_epochs=1, batch_size=2, steps=0, max_steps_run=3,
                      iterations_per_epoch=9, save_every=0, use_graph=False, log_every=1, clip_size=32, **kw)
    return steps, [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith(" step ")]


def test_kinetics_skip_flags(capsys, monkeypatch):
    import train_x3d_kinetics_multigrid as tr
    from x3dhip.gradmonitor import SkippedRunError
    _dev()
    steps, lines = _kinetics_run(capsys, skip_nonfinite=True)
    assert steps == 3 and len(lines) == 3
    assert all(re.search(r" gnorm \d\.\d{4}e[+-]\d+ clip 1\.0000 skipped 0$", ln) for ln in lines)
    steps, off = _kinetics_run(capsys)
    assert all(" skipped " not in ln for ln in off)
    loss = re.compile(r" loss (\d+\.\d+) ")
    assert [loss.search(ln).group(1) for ln in off] == [loss.search(ln).group(1) for ln in lines]
    real = tr.device_batch

    def all_nan(*a, **k):                                # a synthetic source whose every clip is NaN
        x, y = real(*a, **k)
        return torch.full_like(x, float("nan")), y

    monkeypatch.setattr(tr, "device_batch", all_nan)
    names = [k for k, _ in __import__("x3d").generate_model("M", n_classes=400).named_parameters()]
    with pytest.raises(SkippedRunError) as e:
        _kinetics_run(capsys, skip_nonfinite=True, max_skip_run=2)
    msg = str(e.value)
    assert "2 updates in a row" in msg and "step 0" in msg
    assert any(msg.endswith("parameter " + k) for k in names), msg
    out = capsys.readouterr().out
    assert " skipped 1" in out and " first non-finite gradient: step 0 parameter " in out


def test_charades_script_skip_flag(tmp_path, capsys):
    from tests import charades_ref as cr
    import train_x3d_charades as mod
    _dev()
    anno, _ = cr.load_fixture()
    torch.manual_seed(5)
    res = mod.run(init_lr=0.01, max_epochs=1, anno=anno, batch_size=4, save_model=str(tmp_path / "g"), save_every=0,
                  use_graph=False, crop_size=64, c_size=64, dropout=0.5, seed=1, skip_nonfinite=True)
    assert res["steps"] == 6 and res["optimizer"].skip_nonfinite
    lines = [ln for ln in capsys.readouterr().out.splitlines() if " train steps: " in ln]
    assert lines and all(re.search(r" gnorm \d\.\d{4}e[+-]\d+ clip 1\.0000 skipped 0$", ln) for ln in lines)
