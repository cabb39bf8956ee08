"""Trainer(ema_decay=) on the GPU: the average of the weights and of all 168 running statistics against tests/ema_ref.py over
the iterates of a twin Trainer without it, in the eager / graph / split-graph / accumulation / RCCL forms of the step; with
and without the guard on a NaN clip; the exchange for validation; the long-cycle switch; the checkpoint round trip; the
defaults; the flags of the training scripts."""
import contextlib
import re

import numpy as np
import pytest
import torch

from tests import ema_ref
from tests.test_trainer_guard_gpu import _dev, _fixture, _running, _trainer
from x3dhip import stepops

pytestmark = pytest.mark.gpu

DECAY = 0.9
_REF = {}


def _iterate(tr):
    torch.cuda.synchronize()
    return tr.fp.flat.cpu().numpy().copy(), {k: v.cpu().numpy().reshape(-1).copy() for k, v in _running(tr).items()}


def _average(start, history, first_k=1):
    """ema_ref over a list of iterates (flat, {name: stats}), from `start`, the first of them being update first_k."""
    e = start[0].copy()
    stats = {k: v.copy() for k, v in start[1].items()}
    for i, (flat, st) in enumerate(history):
        d, omd = ema_ref.decay_rule(first_k + i, DECAY, True)
        e = ema_ref.element_rule(e, flat, d, omd)
        stats = {k: ema_ref.element_rule(stats[k], st[k], d, omd) for k in stats}
    return e, stats


def _reference(golden_dir, dev, name):
    """The averages a run must hold, computed once per kind of run from an eager twin without the average (the graph forms
    compute the eager step's bits: tests/test_trainer_monitor_gpu.py) and shared by the tests; never changed."""
    if name not in _REF:
        sd, S, xs, bad, y = _fixture(golden_dir, dev, clips=10 if name == "accum" else 5)
        twin = _trainer(sd, S, dev, **(dict(num_steps_per_update=2) if name == "accum" else {}))
        start, hist = _iterate(twin), []
        if name == "accum":
            for u in range(3):
                twin.train_step(xs[2 * u], y)
                twin.train_step(xs[2 * u + 1], y)
                hist.append(_iterate(twin))
        else:
            for i in ((0, 1, 3, 4) if name == "good4" else range(5)):
                twin.train_step(xs[i], y)
                hist.append(_iterate(twin))
        _REF[name] = _average(start, hist) + (hist[-1][0],)
    return _REF[name]


def _ema_stats(tr):
    """{state_dict name: the averaged statistics of that buffer} from the average's snapshot."""
    kt = tr.ema._table()
    snap = tr.ema.stats
    return {name: snap[int(off):int(off) + b.numel()] for name, b, off in zip(tr.ema.stat_names, kt.buffers, kt.table["offset"])}


def _assert_average(tr, ref):
    torch.cuda.synchronize()
    e, stats, last = ref
    assert torch.equal(tr.fp.flat.cpu(), torch.from_numpy(last)), "the run itself is the twin's"
    assert torch.equal(tr.ema.e.cpu(), torch.from_numpy(e))
    got = _ema_stats(tr)
    assert sorted(got) == sorted(stats) and len(got) == 168
    for k in stats:
        assert torch.equal(got[k].cpu(), torch.from_numpy(stats[k])), k
    assert not torch.equal(tr.ema.e, tr.fp.flat)


@pytest.mark.parametrize("kw", [dict(), dict(use_graph=True), dict(use_graph=True, force_split=True)],
                         ids=["eager", "graph", "split"])
def test_five_steps_average_as_the_restatement_says(golden_dir, kw):
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev)
    tr = _trainer(sd, S, dev, ema_decay=DECAY, **kw)
    assert tr.ema.decay == DECAY and tr.ema.warmup and tr.ema.monitor is None and tr.ema.updates() == 0
    assert torch.equal(tr.ema.e, tr.fp.flat) and tr.ema.e.data_ptr() != tr.fp.flat.data_ptr()
    for i in range(5):
        tr.train_step(xs[i], y)
    assert tr._overlap() == bool(kw.get("force_split"))
    _assert_average(tr, _reference(golden_dir, dev, "five"))
    assert tr.ema.updates() == 5 and tr.ema.stat_updates() == 5


def test_accumulation_averages_once_per_update(golden_dir):
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev, clips=10)
    tr = _trainer(sd, S, dev, ema_decay=DECAY, num_steps_per_update=2)
    for u in range(3):
        tr.train_step(xs[2 * u], y)
        assert not tr.stepped and tr.ema.updates() == u
        tr.train_step(xs[2 * u + 1], y)
        assert tr.stepped and tr.ema.updates() == u + 1
    _assert_average(tr, _reference(golden_dir, dev, "accum"))


def test_one_rank_rccl_group_averages_alike(golden_dir, monkeypatch):
    import torch.distributed as dist
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev)
    ref = _reference(golden_dir, dev, "five")
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", "29543")
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        tr = _trainer(sd, S, dev, ema_decay=DECAY, use_graph=True, process_group=dist.group.WORLD, world_size=1,
                      force_split=True, force_collectives=True)
        for i in range(5):
            tr.train_step(xs[i], y)
        assert tr.reducer.active and tr._overlap()
        _assert_average(tr, ref)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("kw", [dict(), dict(use_graph=True)], ids=["eager", "graph"])
def test_a_skipped_update_is_not_averaged_and_does_not_count(golden_dir, kw):
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev)
    tr = _trainer(sd, S, dev, ema_decay=DECAY, skip_nonfinite=True, **kw)
    assert tr.ema.monitor is tr.monitor
    for i in range(5):
        if i == 2:
            torch.cuda.synchronize()
            before = (tr.ema.e.clone(), tr.ema.stats.clone(), tr.ema.updates())
        tr.train_step(bad if i == 2 else xs[i], y)
        if i == 2:
            torch.cuda.synchronize()
            assert torch.equal(tr.ema.e, before[0]) and torch.equal(tr.ema.stats, before[1])
            assert tr.ema.updates() == before[2] == 2
    _assert_average(tr, _reference(golden_dir, dev, "good4"))
    assert tr.ema.updates() == 4 and tr.ema.stat_updates() == 4 and int(tr.monitor.skipped()) == 1


def test_without_the_guard_the_same_clips_leave_a_nan_average(golden_dir):
    """The rule the docstrings state: an unguarded non-finite update poisons the average for good."""
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev)
    tr = _trainer(sd, S, dev, ema_decay=DECAY)
    for i in range(5):
        tr.train_step(bad if i == 2 else xs[i], y)
    torch.cuda.synchronize()
    assert not bool(torch.isfinite(tr.ema.e).all()) and not bool(torch.isfinite(tr.ema.stats).all())
    assert tr.ema.updates() == 5
    import x3dhip.weightema as we
    from x3dhip.trainer import Trainer
    assert "poisons the average" in we.__doc__ and "poisons the average" in Trainer.__init__.__doc__


def _eval_logits(model, x):
    model.train(False)
    model.aggregate_sub_bn_stats()
    with torch.no_grad():
        return model(x).clone()


def test_applied_scores_the_average_and_leaves_no_trace(golden_dir):
    import x3d
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev)
    tr = _trainer(sd, S, dev, ema_decay=DECAY, use_graph=True)
    twin = _trainer(sd, S, dev, ema_decay=DECAY, use_graph=True)
    for i in range(3):
        tr.train_step(xs[i], y)
        twin.train_step(xs[i], y)
    torch.cuda.synchronize()
    ptrs = (tr.fp.flat.data_ptr(), [b.data_ptr() for b in tr.ema._table().buffers])
    live = (tr.fp.flat.clone(), _running(tr))
    avg = (tr.ema.e.clone(), tr.ema.stats.clone())
    esd = tr.ema.state_dict()
    assert sorted(esd) == ["decay", "model", "stat_updates", "updates", "warmup"]
    assert (esd["decay"], esd["warmup"], esd["updates"], esd["stat_updates"]) == (DECAY, True, 3, 3)
    msd = tr.model.state_dict()
    assert list(esd["model"]) == list(msd)
    for k in msd:                                        # every other key as the live model has it
        if "split_bn.running_" not in k and k not in tr.ema.names:
            assert torch.equal(esd["model"][k], msd[k]), k
    with tr.ema.applied() as inside:
        assert inside is tr.ema
        assert torch.equal(tr.fp.flat, avg[0]) and torch.equal(tr.ema.e, live[0])
        assert (tr.fp.flat.data_ptr(), [b.data_ptr() for b in tr.ema._table().buffers]) == ptrs      # no address moved
        for k, v in _running(tr).items():
            assert torch.equal(v, esd["model"][k]) and not torch.equal(v, live[1][k]), k
        got = _eval_logits(tr.model, xs[3])
    fresh = x3d.generate_model("M", n_classes=400, dropout=0.0, base_bn_splits=S)
    fresh.load_state_dict(esd["model"])
    fresh.to(dev)
    want = _eval_logits(fresh, xs[3])
    assert torch.equal(got, want)
    tr.model.train(True)
    live_logits = _eval_logits(tr.model, xs[3])
    assert not torch.equal(live_logits, got)
    tr.model.train(True)
    # an exception inside the block still swaps back
    with pytest.raises(RuntimeError, match="inside"):
        with tr.ema.applied():
            assert torch.equal(tr.fp.flat, avg[0])
            raise RuntimeError("inside")
    torch.cuda.synchronize()
    assert torch.equal(tr.fp.flat, live[0]) and torch.equal(tr.ema.e, avg[0]) and torch.equal(tr.ema.stats, avg[1])
    for k, v in _running(tr).items():
        assert torch.equal(v, live[1][k]), k
    # ... and a replayed captured step goes on as in a twin that never swapped
    for i in (3, 4):
        la, _ = tr.train_step(xs[i], y)
        lb, _ = twin.train_step(xs[i], y)
        assert torch.equal(la, lb)
    torch.cuda.synchronize()
    assert torch.equal(tr.fp.flat, twin.fp.flat) and torch.equal(tr.fp.mom, twin.fp.mom)
    assert torch.equal(tr.ema.e, twin.ema.e) and torch.equal(tr.ema.stats, twin.ema.stats)
    a, b = _running(tr), _running(twin)
    assert all(torch.equal(a[k], b[k]) for k in a)
    _assert_average(tr, _reference(golden_dir, dev, "five"))


def test_a_long_cycle_switch_restarts_the_statistics_count_only(golden_dir):
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev)
    for kw in (dict(), dict(skip_nonfinite=True)):
        tr = _trainer(sd, S, dev, ema_decay=DECAY, use_graph=True, **kw)
        for i in range(2):
            tr.train_step(xs[i], y)
        old = tr.ema._table()
        assert tr.model.update_bn_splits_long_cycle(2) == 2 * S
        tr.invalidate_graphs()
        fresh = _iterate(tr)[1]
        hist = []
        for i in (2, 3):
            tr.train_step(xs[i], y)
            hist.append((np.zeros(1, np.float32), _iterate(tr)[1]))
        assert tr.ema._table() is not old and tr.ema._kt_old is old
        assert tr.ema.updates() == 4 and tr.ema.stat_updates() == 2
        _, want = _average((np.zeros(1, np.float32), fresh), hist)
        got = _ema_stats(tr)
        assert sorted(got) == sorted(want) and len(got) == 168
        for k in want:
            assert got[k].numel() == 2 * sd[k].numel() and torch.equal(got[k].cpu(), torch.from_numpy(want[k])), k
        # the weights' decay went on with k = 3, 4: min(0.9, 4 / 13), min(0.9, 5 / 14), not 2 / 11 again
        assert ema_ref.decay_rule(3, DECAY, True)[0] != ema_ref.decay_rule(1, DECAY, True)[0]
        assert bool(torch.isfinite(tr.ema.e).all())


@pytest.mark.parametrize("kw", [dict(), dict(skip_nonfinite=True)], ids=["plain", "guarded"])
def test_checkpoint_round_trip(golden_dir, kw):
    """Save at step 3, resume in a new model and Trainer, and step 5 equals the uninterrupted run bit for bit."""
    import x3d
    from x3dhip.trainer import Trainer
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev)
    tr = _trainer(sd, S, dev, ema_decay=DECAY, **kw)
    for i in range(3):
        tr.train_step(xs[i], y)
    to_cpu = lambda d: {k: (to_cpu(v) if isinstance(v, dict) else v.cpu().clone() if isinstance(v, torch.Tensor) else v)  # noqa: E731
                        for k, v in d.items()}
    ck = dict(model=to_cpu(tr.model.state_dict()), opt=to_cpu(tr.state_dict()), ema=to_cpu(tr.ema.state_dict()))
    assert "ema" not in str(sorted(tr.state_dict()))     # not optimizer state
    for i in (3, 4):
        tr.train_step(xs[i], y)
    net = x3d.generate_model("M", n_classes=400, dropout=0.0, base_bn_splits=S)
    net.load_state_dict(ck["model"])
    net.to(dev).train(True)
    again = Trainer(net, lr=0.05, ema_decay=DECAY, **kw)
    again.load_state_dict(ck["opt"])
    assert again.ema.updates() == 0
    again.ema.load_state_dict(ck["ema"])
    assert again.ema.updates() == 3 and again.ema.stat_updates() == 3
    for i in (3, 4):
        again.train_step(xs[i], y)
    torch.cuda.synchronize()
    assert torch.equal(again.fp.flat, tr.fp.flat) and torch.equal(again.fp.mom, tr.fp.mom)
    assert torch.equal(again.ema.e, tr.ema.e) and torch.equal(again.ema.stats, tr.ema.stats)
    assert again.ema.updates() == 5 == tr.ema.updates()
    if not kw:
        _assert_average(again, _reference(golden_dir, dev, "five"))
    bad_sd = dict(ck["ema"], model={k: v for k, v in ck["ema"]["model"].items() if "layer1" not in k})
    with pytest.raises(ValueError):
        again.ema.load_state_dict(bad_sd)


@contextlib.contextmanager
def _counted(monkeypatch):
    calls = dict(ema=0, ema_keep=0, swap=0, swap_keep=0)

    def wrap(name):
        real = getattr(stepops, name)

        def f(*a, **k):
            calls[name] += 1
            return real(*a, **k)
        return f

    for name in calls:
        monkeypatch.setattr(stepops, name, wrap(name))
    yield calls


def test_defaults_are_off(golden_dir, monkeypatch):
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev)
    with _counted(monkeypatch) as calls:
        plain = _trainer(sd, S, dev)
        guard = _trainer(sd, S, dev, skip_nonfinite=True)
        on = _trainer(sd, S, dev, ema_decay=DECAY)
        assert not hasattr(plain, "ema") and not hasattr(guard, "ema") and hasattr(on, "ema")
        for i in range(3):
            plain.train_step(xs[i], y)
            guard.train_step(xs[i], y)
        assert calls == dict(ema=0, ema_keep=0, swap=0, swap_keep=0)       # not one launch of the average
        for i in range(3):
            on.train_step(xs[i], y)
        assert calls == dict(ema=3, ema_keep=3, swap=0, swap_keep=0)       # two launches per update
        with on.ema.applied():
            pass
        assert calls == dict(ema=3, ema_keep=3, swap=2, swap_keep=2)
    torch.cuda.synchronize()
    assert torch.equal(on.fp.flat, plain.fp.flat) and torch.equal(on.fp.mom, plain.fp.mom)       # training is untouched
    a, b = plain.state_dict(), on.state_dict()
    assert sorted(a) == sorted(b) == ["param_groups", "state"] and a["param_groups"] == b["param_groups"]
    assert sorted(a["state"]) == sorted(b["state"]) == list(range(316))
    assert all(list(v) == ["momentum_buffer"] for v in b["state"].values())
    assert all(torch.equal(a["state"][i]["momentum_buffer"], b["state"][i]["momentum_buffer"]) for i in range(316))
    ma, mb = plain.model.state_dict(), on.model.state_dict()
    assert list(ma) == list(mb) and all(torch.equal(ma[k], mb[k]) for k in ma)
    with pytest.raises(ValueError):
        _trainer(sd, S, dev, ema_decay=1.0)


# -- the scripts ----------------------------------------------------------------------------------------------------------------
def _kinetics_run(capsys, tmp_path, name, **kw):
    import train_x3d_kinetics_multigrid as tr
    torch.manual_seed(5)
    steps, _ = tr.run(init_lr=0.01, warmup_steps=2, max_epochs=1, batch_size=2, steps=0, max_steps_run=3,
                      iterations_per_epoch=9, save_every=3, save_model=str(tmp_path / name), use_graph=False, log_every=1,
                      clip_size=32, val_every=3, val_batches=1, val_batch_size=1, val_crops=2, **kw)
    assert steps == 3
    return capsys.readouterr().out.splitlines(), torch.load(str(tmp_path / (name + "000003.pt")), map_location="cpu")


def test_kinetics_script_ema_flags(capsys, tmp_path):
    _dev()
    on, ck_on = _kinetics_run(capsys, tmp_path, "on_", ema_decay=DECAY)
    off, ck_off = _kinetics_run(capsys, tmp_path, "off_")
    val = re.compile(r"^ val after step 3: Cls Loss: \d+\.\d{4} Acc: \d\.\d{4} \(1 videos\)$")
    ema = re.compile(r"^ EMA val after step 3: Cls Loss: \d+\.\d{4} Acc: \d\.\d{4} \(1 videos\)$")
    assert sum(bool(val.match(ln)) for ln in on) == 1 and sum(bool(ema.match(ln)) for ln in on) == 1
    assert on.index([ln for ln in on if ema.match(ln)][0]) == on.index([ln for ln in on if val.match(ln)][0]) + 1
    # without the flag: the same lines but the EMA one, the same keys but 'ema_state_dict'
    strip = lambda lines: [re.sub(r"  \d+\.\d clips/s", "", ln) for ln in lines if "EMA" not in ln]      # noqa: E731
    assert strip(on) == strip(off) and not any("EMA" in ln for ln in off)
    assert sorted(ck_off) == ["long_ind", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict"]
    assert sorted(ck_on) == sorted(list(ck_off) + ["ema_state_dict"])
    esd = ck_on["ema_state_dict"]
    # the tiny schedule switches the long cycle inside these three steps: the statistics' count restarted there
    last_switch = max(i for i, ln in enumerate(on) if ln.startswith(" ***** LR "))
    since = sum(ln.startswith(" step ") for ln in on[last_switch:])
    assert 1 <= since <= 3
    assert (esd["decay"], esd["warmup"], esd["updates"], esd["stat_updates"]) == (DECAY, True, 3, since)
    assert list(esd["model"]) == list(ck_on["model_state_dict"])
    assert [k for k in ck_off["model_state_dict"] if not torch.equal(ck_on["model_state_dict"][k], ck_off["model_state_dict"][k])] == []
    # --load restores the average
    import train_x3d_kinetics_multigrid as tr
    steps, _ = tr.run(init_lr=0.01, warmup_steps=2, max_epochs=1, batch_size=2, steps=3, max_steps_run=1,
                      iterations_per_epoch=9, save_every=4, save_model=str(tmp_path / "again_"), use_graph=False, log_every=1,
                      clip_size=32, load_ckpt=str(tmp_path / "on_000003.pt"), ema_decay=DECAY)
    capsys.readouterr()
    assert steps == 4
    assert torch.load(str(tmp_path / "again_000004.pt"), map_location="cpu")["ema_state_dict"]["updates"] == 4


@pytest.mark.parametrize("task", ["class", "loc"])
def test_charades_scripts_ema_flags(tmp_path, capsys, task):
    from tests import charades_ref as cr
    import train_x3d_charades
    import train_x3d_charades_loc
    _dev()
    mod = train_x3d_charades if task == "class" else train_x3d_charades_loc
    anno, _ = cr.load_fixture()
    out = {}
    for name, kw in (("on", dict(ema_decay=DECAY, ema_warmup=False)), ("off", {})):
        torch.manual_seed(5)
        res = mod.run(init_lr=0.01, max_epochs=1, anno=anno, batch_size=4, save_model=str(tmp_path / (name + "_")),
                      save_every=3, use_graph=False, crop_size=64, c_size=64, dropout=0.5, seed=1, **kw)
        assert res["steps"] == 6 and len(res["checkpoints"]) == 2
        out[name] = (capsys.readouterr().out.splitlines(), torch.load(res["checkpoints"][0], map_location="cpu"), res)
    on, ck_on, res_on = out["on"]
    off, ck_off, res_off = out["off"]
    ema = [ln for ln in on if re.match(r"^ EMA Epoch:\d+ val ", ln)]
    assert len(ema) == 1 and re.search(r" Tot Loss: \d+\.\d{4} mAP: \d\.\d{4}$", ema[0])
    assert [ln for ln in on if "EMA" not in ln] == off and not any("EMA" in ln for ln in off)      # the printed lines: as now
    assert sum(" Epoch:" in ln for ln in off) >= 3
    assert hasattr(res_on["optimizer"], "ema") and not hasattr(res_off["optimizer"], "ema")
    assert not res_on["optimizer"].ema.warmup and res_on["optimizer"].ema.updates() == 6
    assert "ema_map" in res_on["phases"][-1] and "ema_map" not in res_off["phases"][-1]
    assert sorted(ck_off) == ["model_state_dict", "optimizer_state_dict", "scheduler_state_dict"]
    assert sorted(ck_on) == sorted(list(ck_off) + ["ema_state_dict"]) and ck_on["ema_state_dict"]["updates"] == 3
    again = mod.run(init_lr=0.01, max_epochs=0, anno=anno, batch_size=4, save_model=str(tmp_path / "again_"), save_every=0,
                    use_graph=False, crop_size=64, c_size=64, seed=1, resume=res_on["checkpoints"][0], ema_decay=DECAY)
    capsys.readouterr()
    assert again["optimizer"].ema.updates() == 3
