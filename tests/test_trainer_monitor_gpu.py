"""Trainer(clip_grad_norm=, monitor=) on the GPU: clipping against an unclipped twin Trainer and ops.sgd_fused, the ring in
the eager / graph / split-graph / accumulation / RCCL forms of the step, the first non-finite gradient, the defaults, and
the flags of the training scripts."""
import math
import os
import re

import numpy as np
import pytest
import torch

from oracle import x3d_oracle as xo
from tests import step_ref
from x3dhip import synthetic

pytestmark = pytest.mark.gpu

CASE = "train_M_2x4x32_s1"          # the smallest fixture: its shape and its weights
LR = 0.05


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _fixture(golden_dir, dev):
    g = np.load(os.path.join(golden_dir, CASE + ".npz"))
    B, T, H, S = [int(v) for v in g["shape"]]
    sd = synthetic.procedural_state_dict(xo.state_template("M", 400, S), int(g["seed"][0]))
    x = synthetic.synthetic_clips(B, T, H, H, seed=int(g["seed"][1])).to(dev)
    y = synthetic.synthetic_labels(B, seed=int(g["seed"][1])).to(dev)
    return sd, S, x, y


def _trainer(sd, S, dev, **kw):
    import x3d
    from x3dhip.trainer import Trainer
    net = x3d.generate_model("M", n_classes=400, dropout=0.0, base_bn_splits=S)
    net.load_state_dict(sd)
    net.to(dev).train(True)
    return Trainer(net, lr=LR, **kw)


def _exact_norm(g):
    d = g.detach().cpu().numpy().astype(np.float64)
    return math.sqrt(math.fsum((d * d).tolist()))


def _ring_bytes(tr):
    torch.cuda.synchronize()
    return tr.monitor.ring.cpu(), tr.monitor.state.cpu()


def test_clipped_step_equals_the_scaled_gradient_through_sgd_fused(golden_dir):
    from x3dhip import ops
    dev = _dev()
    sd, S, x, y = _fixture(golden_dir, dev)
    twin = _trainer(sd, S, dev)
    twin._fwd_bwd(x, y)                                   # the unclipped gradient of the same step
    g = twin.fp.grad.clone()
    norm = _exact_norm(g)
    c = norm / 2                                          # clipping is active
    tr = _trainer(sd, S, dev, clip_grad_norm=c)
    assert tr.monitor.clipping
    tr.train_step(x, y)
    rec = tr.monitor.read()
    assert rec["step"].tolist() == [0] and rec["nonfinite"].tolist() == [0] and rec["first_bad"] == [None]
    print("recorded norm %.17g exact %.17g coef %.9g" % (rec["norm"][0], norm, rec["coef"][0]))
    assert abs(rec["norm"][0] - norm) <= 2 * np.spacing(norm)            # 2 fp64 ulp
    assert 0.49 < rec["coef"][0] < 0.51
    assert float(tr.monitor.last_norm()) == rec["norm"][0] and float(tr.monitor.last_coef()) == rec["coef"][0]
    # the twin applies the scaled gradient itself
    scaled = g * torch.tensor(rec["coef"][0], dtype=torch.float32, device=dev)
    assert torch.equal(tr.fp.grad, scaled)
    pg = twin.param_groups[0]
    ops.sgd_fused(twin.fp.flat, scaled, twin.fp.mom, pg["lr"], pg["momentum"], pg["weight_decay"], 1.0, first=True)
    torch.cuda.synchronize()
    assert torch.equal(tr.fp.flat, twin.fp.flat) and torch.equal(tr.fp.mom, twin.fp.mom)
    # per-tensor statistics by name, against the restatement on the gradient read back
    gn = g.cpu().numpy()
    names = [k for k, _ in tr.model.named_parameters()]
    assert list(rec["sumsq"]) == names and len(names) == 316
    for i in (0, 1, 157, 314, 315):
        o, k = tr.fp.offsets[i]
        assert rec["hash"][names[i]][0] == step_ref.tensor_hash(gn[o:o + k])
        want = step_ref.tensor_sumsq(gn[o:o + k])
        assert abs(rec["sumsq"][names[i]][0] - want) <= max(k - 1, 0) * 2.0 ** -53 * want


def test_a_huge_max_norm_changes_nothing(golden_dir):
    dev = _dev()
    sd, S, x, y = _fixture(golden_dir, dev)
    plain, big = _trainer(sd, S, dev), _trainer(sd, S, dev, clip_grad_norm=1e30)
    for _ in range(2):
        plain.train_step(x, y)
        big.train_step(x, y)
    torch.cuda.synchronize()
    assert torch.equal(plain.fp.flat, big.fp.flat) and torch.equal(plain.fp.mom, big.fp.mom)
    assert big.monitor.read()["coef"].tolist() == [1.0, 1.0]


def test_eager_graph_and_split_graph_give_identical_rings(golden_dir):
    dev = _dev()
    sd, S, x, y = _fixture(golden_dir, dev)
    rings = []
    for kw in (dict(), dict(use_graph=True), dict(use_graph=True, force_split=True)):
        tr = _trainer(sd, S, dev, clip_grad_norm=0.5, monitor=8, **kw)
        assert tr._overlap() == bool(kw.get("force_split"))
        for _ in range(4):
            tr.train_step(x, y)
        rings.append(_ring_bytes(tr) + (tr.fp.flat.clone(),))
        assert tr.monitor.read()["step"].tolist() == [0, 1, 2, 3]
    for ring, state, flat in rings[1:]:
        assert torch.equal(ring, rings[0][0]) and torch.equal(state, rings[0][1]) and torch.equal(flat, rings[0][2])


def test_accumulation_records_once_per_update_on_the_accumulated_buffer(golden_dir):
    dev = _dev()
    sd, S, x, y = _fixture(golden_dir, dev)
    tr = _trainer(sd, S, dev, num_steps_per_update=2, monitor=True)
    x2 = synthetic.synthetic_clips(*x.shape[:1], x.shape[2], x.shape[3], x.shape[4], seed=77).to(dev)
    for i in range(4):
        tr.train_step(x if i % 2 == 0 else x2, y)
        assert tr.stepped == (i % 2 == 1)
        assert tr.monitor.steps() == (i + 1) // 2
    rec = tr.monitor.read()
    assert rec["step"].tolist() == [0, 1] and rec["coef"].tolist() == [1.0, 1.0]
    acc = tr.accum.cpu().numpy()                          # the buffer the second update applied (monitoring leaves it alone)
    names = [k for k, _ in tr.model.named_parameters()]
    for i in (0, 100, 315):
        o, k = tr.fp.offsets[i]
        assert rec["hash"][names[i]][1] == step_ref.tensor_hash(acc[o:o + k])
    assert abs(rec["norm"][1] - _exact_norm(tr.accum)) <= 2 * np.spacing(rec["norm"][1])


def test_one_rank_rccl_group_matches_the_plain_path(golden_dir, monkeypatch):
    import torch.distributed as dist
    dev = _dev()
    sd, S, x, y = _fixture(golden_dir, dev)
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", "29537")
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    plain = _trainer(sd, S, dev, use_graph=True, clip_grad_norm=0.5)
    for _ in range(3):
        plain.train_step(x, y)
    want = _ring_bytes(plain)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        tr = _trainer(sd, S, dev, use_graph=True, clip_grad_norm=0.5, process_group=dist.group.WORLD, world_size=1,
                      force_split=True, force_collectives=True)
        assert tr.reducer.active and tr._overlap() and tr.monitor.inv_world == 1.0
        for _ in range(3):
            tr.train_step(x, y)
        got = _ring_bytes(tr)
        flat = tr.fp.flat.clone()
    finally:
        dist.destroy_process_group()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(flat, plain.fp.flat)


def test_first_nonfinite_names_the_step_and_the_tensor(golden_dir):
    dev = _dev()
    sd, S, x, y = _fixture(golden_dir, dev)
    tr = _trainer(sd, S, dev, monitor=True)
    names = [k for k, _ in tr.model.named_parameters()]
    which = 100
    o, k = tr.fp.offsets[which]
    for step in range(4):
        def hook(step=step):
            if step == 2:
                tr.fp.grad[o + k // 2] = float("nan")     # data, written into one tensor's slice of the flat gradient
        tr.train_step(x, y, pre_step=hook)
        if step < 2:
            assert tr.monitor.first_nonfinite() is None
    assert tr.monitor.first_nonfinite() == (2, names[which])
    rec = tr.monitor.read()
    assert rec["first_bad"][:3] == [None, None, names[which]] and rec["nonfinite"].tolist()[:3] == [0, 0, 1]
    assert rec["nonfinite_by_name"][names[which]][2] == 1 and np.isnan(rec["norm"][2])


def test_defaults_are_off(golden_dir):
    dev = _dev()
    sd, S, x, y = _fixture(golden_dir, dev)
    plain, mon = _trainer(sd, S, dev), _trainer(sd, S, dev, monitor=True, clip_grad_norm=1.0)
    assert not hasattr(plain, "monitor") and mon.monitor.R == 64
    for tr in (plain, mon):
        tr.train_step(x, y)
    a, b = plain.state_dict(), mon.state_dict()
    assert sorted(a) == sorted(b) == ["param_groups", "state"]
    assert sorted(a["param_groups"][0]) == sorted(b["param_groups"][0]) == sorted(
        ["lr", "momentum", "dampening", "weight_decay", "nesterov", "params"])
    assert sorted(a["state"]) == sorted(b["state"]) == list(range(316))
    assert all(list(v) == ["momentum_buffer"] for v in b["state"].values())


LOSS = re.compile(r" loss (\d+\.\d+) ")


def _kinetics_run(capsys, **kw):
    import train_x3d_kinetics_multigrid as tr
    torch.manual_seed(5)
    steps, _ = tr.run(init_lr=0.01, warmup_steps=2, max_epochs=1, batch_size=2, steps=0, max_steps_run=3,
                      iterations_per_epoch=9, save_every=0, use_graph=False, log_every=1, clip_size=32, **kw)
    assert steps == 3
    return [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith(" step ")]


def test_kinetics_flags(capsys):
    _dev()
    off = _kinetics_run(capsys)
    mon = _kinetics_run(capsys, monitor=16)
    both = _kinetics_run(capsys, clip_grad_norm=0.25, monitor=True)
    assert len(off) == len(mon) == len(both) == 3
    assert all(" gnorm " not in ln and " clip " not in ln and ln.endswith(" clips/s") for ln in off)
    assert all(re.search(r" gnorm \d\.\d{4}e[+-]\d+ clip 1\.0000$", ln) for ln in mon)
    assert all(re.search(r" gnorm \d\.\d{4}e[+-]\d+ clip [01]\.\d{4}$", ln) for ln in both)
    # observing changes nothing: the run without the flags prints the losses of the monitored one
    assert [LOSS.search(ln).group(1) for ln in off] == [LOSS.search(ln).group(1) for ln in mon]
    assert any(float(ln.rsplit(" ", 1)[1]) < 1.0 for ln in both)


def test_charades_script_flags(tmp_path, capsys):
    from tests import charades_ref as cr
    import train_x3d_charades as mod
    _dev()
    anno, _ = cr.load_fixture()
    lines = {}
    # a max_norm no gradient reaches: the coefficient is 1 and the run is the unflagged one bit for bit
    for name, kw in (("off", {}), ("on", dict(clip_grad_norm=1e30, monitor=True))):
        torch.manual_seed(5)
        res = mod.run(init_lr=0.01, max_epochs=1, anno=anno, batch_size=4, save_model=str(tmp_path / name), save_every=0,
                      use_graph=False, crop_size=64, c_size=64, dropout=0.5, seed=1, **kw)
        assert res["steps"] == 6
        lines[name] = [ln for ln in capsys.readouterr().out.splitlines() if " train steps: " in ln]
        assert hasattr(res["optimizer"], "monitor") == (name == "on")
    assert len(lines["off"]) == len(lines["on"]) > 0
    assert all(" gnorm " not in ln and " clip " not in ln for ln in lines["off"])
    assert all(re.search(r" mAP: \d\.\d{4} gnorm \d\.\d{4}e[+-]\d+ clip 1\.0000$", ln) for ln in lines["on"])
    # the run without the flags prints the losses (and mAPs) of the flagged one
    assert lines["off"] == [ln[:ln.index(" gnorm ")] for ln in lines["on"]]
