"""PreciseBN and Trainer.precise_bn on the GPU, X3D-M at 2x4x32^2 (the shape of train_M_2x4x32_s1) with batch 4 and one or two
splits: the momentum-1 pass; the pooled statistics against the fp64 oracle pooled in Fractions; nothing else moves; the
exchange for validation; a one-rank RCCL group; with the weight average; the long-cycle switch; bf16 storage; the defaults;
the flags of the training scripts."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import x3d_oracle as xo
from tests import parity, pbn_ref
from tests.test_trainer_guard_gpu import CASE, LR, _dev, _running
from x3dhip import stepops, synthetic
from x3dhip.weightema import running_stat_buffers

pytestmark = pytest.mark.gpu

B = 4
_CACHE = {}


def _setup(golden_dir, dev, S, clips=5):
    """(state dict for S splits, `clips` clips [4, 3, T, H, H], labels), made once per S and never changed."""
    key = (S, clips)
    if key not in _CACHE:
        g = np.load(os.path.join(golden_dir, CASE + ".npz"))
        _, T, H, _ = [int(v) for v in g["shape"]]
        sd = synthetic.procedural_state_dict(xo.state_template("M", 400, S), int(g["seed"][0]))
        xs = [synthetic.synthetic_clips(B, T, H, H, seed=int(g["seed"][1]) + 40 + i).to(dev) for i in range(clips)]
        y = synthetic.synthetic_labels(B, seed=int(g["seed"][1])).to(dev)
        _CACHE[key] = (sd, xs, y)
    return _CACHE[key]


def _model(sd, S, dev, dropout=0.0, **kw):
    import x3d
    net = x3d.generate_model("M", n_classes=400, dropout=dropout, base_bn_splits=S, **kw)
    net.load_state_dict(sd)
    return net.to(dev).train(True)


def _trainer(sd, S, dev, dropout=0.0, **kw):
    from x3dhip.trainer import Trainer
    torch.manual_seed(11)                                # the head's dropout stream starts from torch's seed
    return Trainer(_model(sd, S, dev, dropout), lr=LR, **kw)


def _pooled(pbn):
    """{state_dict name: the pooled statistics of that buffer} from the snapshot."""
    kt = pbn._kt
    return {n: kt.snap[int(o):int(o) + b.numel()].clone() for n, b, o in zip(pbn._names, kt.buffers, kt.table["offset"])}


def _bn_pairs(net, ctx):
    """(SubBatchNorm3d, the `save` tensor [2, S, C] of its forward finalize) for all 84 layers of a pass."""
    pairs = [(net.bn1, ctx.stem["save0"])]
    blocks = [blk for layer in (net.layer1, net.layer2, net.layer3, net.layer4) for blk in layer]
    assert len(blocks) == len(ctx.blocks)
    for blk, rec in zip(blocks, ctx.blocks):
        pairs += [(blk.bn1, rec["s1"]), (blk.bn2, rec["s2"]), (blk.bn3, rec["s3"])]
        if blk.downsample is not None:
            pairs.append((blk.downsample[1], rec["sd"]))
    pairs.append((net.bn5, ctx.head["save5"]))
    assert len(pairs) == 84
    return pairs


def _eval_logits(model, x):
    model.train(False)
    model.aggregate_sub_bn_stats()
    with torch.no_grad():
        out = model(x).clone()
    model.train(True)
    return out


# -- 1: the momentum-1 pass -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2])
def test_a_momentum_1_pass_leaves_the_cell_in_the_split_buffers(golden_dir, S):
    from x3dhip import engine
    from x3dhip.precisebn import PreciseBN
    dev = _dev()
    sd, xs, _ = _setup(golden_dir, dev, S)
    net = _model(sd, S, dev)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    ctx = engine.TrunkContext()
    with torch.no_grad():
        engine.trunk_forward(net, xs[0], True, ctx, bn_momentum=1.0)
    for bn, save in _bn_pairs(net, ctx):
        assert torch.equal(bn.split_bn.running_mean.view(S, -1).view(torch.int32), save[0].view(torch.int32))
        assert bool((bn.split_bn.running_var > 0).all())
    ctx2 = engine.TrunkContext()
    other = _model(sd, S, dev)
    with torch.no_grad():
        engine.trunk_forward(other, xs[0], True, ctx2)                          # the default is BN_MOMENTUM, as before
    want = 0.9 * before["bn5.split_bn.running_mean"].double() + 0.1 * ctx2.head["save5"][0].reshape(-1).double()
    assert torch.allclose(other.bn5.split_bn.running_mean.double(), want, rtol=1e-6, atol=1e-7)
    assert not torch.equal(other.bn5.split_bn.running_mean, net.bn5.split_bn.running_mean)
    if S == 1:                                           # K = 1, S = 1: the pooled values are the cell, bit for bit
        fresh = _model(sd, S, dev)
        pbn = PreciseBN(fresh).compute([xs[0]])
        assert (pbn.batches, pbn.cells) == (1, 1)
        got = _pooled(pbn)
        cell = {k: v for k, v in net.state_dict().items() if "split_bn.running_" in k}
        assert sorted(got) == sorted(cell) and len(got) == 168
        for k in got:
            assert torch.equal(got[k].view(torch.int32), cell[k].view(torch.int32)), k


# -- 2: against the oracle ---------------------------------------------------------------------------------------------------------
def test_three_batches_of_two_splits_against_the_fp64_oracle_pooled_in_fractions(golden_dir):
    from x3dhip.precisebn import PreciseBN
    dev = _dev()
    S, K = 2, 3
    sd, xs, _ = _setup(golden_dir, dev, S)
    pbn = PreciseBN(_model(sd, S, dev)).compute(xs[:K])
    assert (pbn.batches, pbn.cells) == (K, K * S)
    got = {k: v.cpu().numpy() for k, v in _pooled(pbn).items()}
    sd64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    for k in sd64:
        if "split_bn.running_" in k:
            sd64[k] = torch.zeros_like(sd64[k])          # new = 0.9 * 0 + 0.1 * cell: the cell is new / 0.1
    cells = {}
    for x in xs[:K]:
        new = {}
        with torch.no_grad():
            xo.trunk(x.cpu().double(), sd64, "M", S, True, new)
        for k, v in new.items():
            if "split_bn.running_" in k:
                cells.setdefault(k, []).append((v / xo.BN_MOMENTUM).numpy())
    assert sorted(cells) == sorted(got)
    worst = 0.0
    for mk in sorted(k for k in cells if k.endswith("running_mean")):
        vk = mk.replace("running_mean", "running_var")
        C = cells[mk][0].size // S
        mus = [a.reshape(S, C)[j] for a in cells[mk] for j in range(S)]       # the n = K * S cells of the layer
        vs = [a.reshape(S, C)[j] for a in cells[vk] for j in range(S)]
        want_m, want_v = np.empty(C), np.empty(C)
        for c in range(C):
            em, ev = pbn_ref.exact_pooled([m[c] for m in mus], [v[c] for v in vs])
            want_m[c], want_v[c] = float(em), float(ev)
        for j in range(S):                               # every split slot holds the pooled value
            em = parity.rel(got[mk].reshape(S, C)[j], want_m)
            ev = parity.rel(got[vk].reshape(S, C)[j], want_v)
            worst = max(worst, em, ev)
            assert em < parity.RTOL and ev < parity.RTOL, (mk, j, em, ev)
    print("worst relative error against the oracle: %.3e" % worst)


# -- 3: nothing else moves ---------------------------------------------------------------------------------------------------------
def _everything(tr):
    torch.cuda.synchronize()
    tr.model.aggregate_sub_bn_stats()
    out = dict(flat=tr.fp.flat.clone(), mom=tr.fp.mom.clone(), rng=tr.model._head_rng_state.clone(),
               pending=torch.tensor(tr.model._pending_tracked))
    out.update({k: v.clone() for k, v in tr.model.state_dict().items() if "bn." in k})      # split_bn.*, bn.*, the counters
    return out


def _assert_same(a, b):
    assert sorted(a) == sorted(b) and len(a) == 4 + 6 * 84
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("kw", [dict(), dict(use_graph=True), dict(use_graph=True, force_split=True)],
                         ids=["eager", "graph", "split"])
def test_compute_and_applied_leave_no_trace(golden_dir, kw):
    dev = _dev()
    S = 2
    sd, xs, y = _setup(golden_dir, dev, S)
    tr, twin = _trainer(sd, S, dev, dropout=0.5, **kw), _trainer(sd, S, dev, dropout=0.5, **kw)
    assert "precise_bn" not in vars(tr)
    for i in range(2):                                   # the second step replays what the first captured
        la, _ = tr.train_step(xs[i], y)
        lb, _ = twin.train_step(xs[i], y)
        assert torch.equal(la, lb)
    ptrs = [b.data_ptr() for _, b in running_stat_buffers(tr.model)]
    pbn = tr.precise_bn
    assert pbn is tr.precise_bn and "precise_bn" in vars(tr) and "precise_bn" not in vars(twin)
    assert pbn.compute(xs[2:4]) is pbn
    _assert_same(_everything(tr), _everything(twin))
    pooled = _pooled(pbn)
    with pbn.applied() as inside:
        assert inside is pbn
        now = {k: v for k, v in tr.model.state_dict().items() if "split_bn.running_" in k}
        assert all(torch.equal(now[k], pooled[k]) for k in pooled)
        assert [b.data_ptr() for _, b in running_stat_buffers(tr.model)] == ptrs                # no address moved
        _eval_logits(tr.model, xs[4])
    with pytest.raises(RuntimeError, match="inside"):
        with pbn.applied():
            raise RuntimeError("inside")
    _assert_same(_everything(tr), _everything(twin))
    assert all(torch.equal(v, pooled[k]) for k, v in _pooled(pbn).items())      # the pooled values wait in the snapshot
    for i in (2, 3):
        la, _ = tr.train_step(xs[i], y)
        lb, _ = twin.train_step(xs[i], y)
        assert torch.equal(la, lb)
    _assert_same(_everything(tr), _everything(twin))
    assert tr._overlap() == bool(kw.get("force_split"))


# -- 4: inside applied() -------------------------------------------------------------------------------------------------------------
def test_applied_scores_what_state_dict_holds(golden_dir):
    from x3dhip.precisebn import PreciseBN
    dev = _dev()
    S = 2
    sd, xs, _ = _setup(golden_dir, dev, S)
    net = _model(sd, S, dev)
    pbn = PreciseBN(net)
    with pytest.raises(RuntimeError, match="compute"):
        with pbn.applied():
            pass
    with pytest.raises(ValueError, match="no batches"):
        pbn.compute([])
    pbn.compute(xs[:3])
    psd = pbn.state_dict()
    assert sorted(psd) == ["batches", "cells", "model"] and (psd["batches"], psd["cells"]) == (3, 6)
    msd = net.state_dict()
    assert list(psd["model"]) == list(msd)
    for k in msd:
        if "running_" not in k:
            assert torch.equal(psd["model"][k], msd[k]), k
    live = _eval_logits(net, xs[3])
    with pbn.applied():
        got = _eval_logits(net, xs[3])
        inside = {k: v.clone() for k, v in net.state_dict().items()}
    for k in inside:
        assert torch.equal(inside[k], psd["model"][k]), k
    for name, mod in net.named_modules():                # S = 2, a power of two: bn.* are the pooled values bit for bit
        if getattr(mod, "split_bn", None) is not None:
            C = mod.num_features
            assert torch.equal(inside[name + ".bn.running_mean"], inside[name + ".split_bn.running_mean"][:C])
            assert torch.equal(inside[name + ".bn.running_var"], inside[name + ".split_bn.running_var"][C:])
    fresh = _model(psd["model"], S, dev)
    want = _eval_logits(fresh, xs[3])
    assert torch.equal(got, want) and not torch.equal(got, live)
    assert torch.equal(_eval_logits(net, xs[3]), live)   # outside again: the live statistics
    import x3dhip.precisebn as mod
    assert "power of two" in mod.__doc__ and "one fp32 ulp" in mod.__doc__


# -- 5: a process group ------------------------------------------------------------------------------------------------------------
def test_a_one_rank_rccl_group_gives_the_bits_of_no_group(golden_dir, monkeypatch):
    import torch.distributed as dist
    from x3dhip.precisebn import PreciseBN
    dev = _dev()
    S = 2
    sd, xs, _ = _setup(golden_dir, dev, S)
    alone = _pooled(PreciseBN(_model(sd, S, dev)).compute(xs[:2]))
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", "29547")
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        from x3dhip.trainer import Trainer
        tr = Trainer(_model(sd, S, dev), lr=LR, process_group=dist.group.WORLD, world_size=1)
        assert tr.precise_bn.pg is dist.group.WORLD
        group = _pooled(tr.precise_bn.compute(xs[:2]))
        assert tr.precise_bn.cells == 2 * S
    finally:
        dist.destroy_process_group()
    assert sorted(group) == sorted(alone) and all(torch.equal(group[k], alone[k]) for k in alone)


# -- 6: with the weight average ----------------------------------------------------------------------------------------------------
def test_compute_inside_ema_applied_uses_the_averaged_weights(golden_dir):
    from x3dhip.precisebn import PreciseBN
    dev = _dev()
    S = 2
    sd, xs, y = _setup(golden_dir, dev, S)
    tr = _trainer(sd, S, dev, ema_decay=0.9)
    for i in range(3):
        tr.train_step(xs[i], y)
    torch.cuda.synchronize()
    before = (tr.fp.flat.clone(), tr.ema.e.clone(), tr.ema.stats.clone(), _running(tr))
    with tr.ema.applied():
        got = _pooled(tr.precise_bn.compute(xs[3:5]))
    live = _pooled(PreciseBN(_model(tr.model.state_dict(), S, dev)).compute(xs[3:5]))
    avg = _pooled(PreciseBN(_model(tr.ema.state_dict()["model"], S, dev)).compute(xs[3:5]))
    assert all(torch.equal(got[k], avg[k]) for k in avg)
    assert any(not torch.equal(got[k], live[k]) for k in live)
    torch.cuda.synchronize()
    assert torch.equal(tr.fp.flat, before[0]) and torch.equal(tr.ema.e, before[1]) and torch.equal(tr.ema.stats, before[2])
    assert all(torch.equal(v, before[3][k]) for k, v in _running(tr).items())


# -- 7: the long-cycle switch --------------------------------------------------------------------------------------------------------
def test_after_a_long_cycle_switch_applied_raises_until_the_next_compute(golden_dir):
    dev = _dev()
    S = 1
    sd, xs, y = _setup(golden_dir, dev, S)
    tr = _trainer(sd, S, dev, use_graph=True)
    tr.train_step(xs[0], y)
    pbn = tr.precise_bn.compute(xs[1:2])
    with pbn.applied():
        pass
    assert tr.model.update_bn_splits_long_cycle(2) == 2
    tr.invalidate_graphs()
    for call in (pbn.applied().__enter__, pbn.state_dict):
        with pytest.raises(RuntimeError, match="long-cycle switch"):
            call()
    pbn.compute(xs[1:3])
    assert pbn.cells == 4
    with pbn.applied():
        assert all(v.numel() == 2 * sd[k].numel() and bool(torch.isfinite(v).all()) for k, v in _running(tr).items())
    with pytest.raises(ValueError, match="divisible"):
        tr.model.update_bn_splits_long_cycle(8)
        pbn.compute(xs[:1])                              # batch 4 over 8 splits
    fresh = {k: v for k, v in _running(tr).items()}
    assert all(bool((v == (0.0 if "mean" in k else 1.0)).all()) for k, v in fresh.items())        # ... and restored


# -- 8: bf16 storage -----------------------------------------------------------------------------------------------------------------
def test_bf16_storage(golden_dir):
    from x3dhip import engine
    from x3dhip.precisebn import PreciseBN
    dev = _dev()
    S = 2
    sd, xs, _ = _setup(golden_dir, dev, S)
    net = _model(sd, S, dev, act_dtype=torch.bfloat16)
    pbn = PreciseBN(net).compute(xs[:2])
    got = _pooled(pbn)
    fp32 = _pooled(PreciseBN(_model(sd, S, dev)).compute(xs[:2]))
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    assert any(not torch.equal(got[k], fp32[k]) for k in got)                   # the bf16 path really ran
    # the twin over two momentum-1 passes of the same model: the same bits
    live = [b.clone() for b in pbn._kt.buffers]
    hk = stepops.KeepTable([np.zeros(b.numel(), np.float32) for b in live])
    hp = stepops.PbnTable(hk, [S] * 84)
    acc = hp.new_acc()
    for x in xs[:2]:
        with torch.no_grad():
            engine.trunk_forward(net, x, True, None, bn_momentum=1.0)
        for h, b in zip(hk.buffers, pbn._kt.buffers):
            h[:] = b.cpu().numpy()
        stepops.pbn_accum_host(hp, acc)
    stepops.pbn_finish_host(hp, acc, 1, 2 * S, hk.snap)
    for (k, v), off, h in zip(got.items(), hk.table["offset"], hk.buffers):
        assert torch.equal(v.cpu().view(torch.int32), torch.from_numpy(hk.snap[int(off):int(off) + h.size]).view(torch.int32)), k
    with pbn.applied():
        assert bool(torch.isfinite(_eval_logits(net, xs[2])).all())


# -- the defaults --------------------------------------------------------------------------------------------------------------------
def test_defaults_are_off(golden_dir, monkeypatch):
    dev = _dev()
    S = 1
    sd, xs, y = _setup(golden_dir, dev, S)
    calls = dict(pbn_accum=0, pbn_finish=0)
    for name in calls:
        def wrap(name=name, real=getattr(stepops, name)):
            def f(*a, **k):
                calls[name] += 1
                return real(*a, **k)
            return f
        monkeypatch.setattr(stepops, name, wrap())
    plain, used = _trainer(sd, S, dev), _trainer(sd, S, dev)
    for i in range(2):
        plain.train_step(xs[i], y)
        used.train_step(xs[i], y)
    assert calls == dict(pbn_accum=0, pbn_finish=0) and "precise_bn" not in vars(plain) and "precise_bn" not in vars(used)
    with pytest.raises(AttributeError):
        plain.no_such_attribute
    assert not hasattr(plain, "ema") and not hasattr(plain, "monitor")
    used.precise_bn.compute(xs[2:4])
    assert calls == dict(pbn_accum=2, pbn_finish=1)
    a, b = plain.state_dict(), used.state_dict()
    assert sorted(a) == sorted(b) == ["param_groups", "state"] and a["param_groups"] == b["param_groups"]
    assert all(torch.equal(a["state"][i]["momentum_buffer"], b["state"][i]["momentum_buffer"]) for i in range(316))
    ma, mb = plain.model.state_dict(), used.model.state_dict()
    assert list(ma) == list(mb) and all(torch.equal(ma[k], mb[k]) for k in ma)


# -- 9: the scripts ------------------------------------------------------------------------------------------------------------------
def _kinetics_run(capsys, tmp_path, name, **kw):
    import train_x3d_kinetics_multigrid as tr
    torch.manual_seed(5)
    steps, _ = tr.run(init_lr=0.01, warmup_steps=2, max_epochs=1, batch_size=2, steps=0, max_steps_run=3,
                      iterations_per_epoch=9, save_every=3, save_model=str(tmp_path / name), use_graph=False, log_every=1,
                      clip_size=32, val_every=3, val_batches=1, val_batch_size=1, val_crops=2, **kw)
    assert steps == 3
    return capsys.readouterr().out.splitlines(), torch.load(str(tmp_path / (name + "000003.pt")), map_location="cpu")


def test_kinetics_script_precise_bn_flag(capsys, tmp_path):
    _dev()
    on, ck_on = _kinetics_run(capsys, tmp_path, "on_", ema_decay=0.9, precise_bn=2)
    off, ck_off = _kinetics_run(capsys, tmp_path, "off_", ema_decay=0.9)
    tail = r"val after step 3: Cls Loss: \d+\.\d{4} Acc: \d\.\d{4} \(1 videos\)$"
    order = [i for p in ("", "PBN ", "EMA ", "EMA PBN ") for i, ln in enumerate(on) if re.match("^ " + p + tail, ln)]
    assert len(order) == 4 and order == list(range(order[0], order[0] + 4))     # one of each, in this order
    strip = lambda lines: [re.sub(r"  \d+\.\d clips/s", "", ln) for ln in lines if "PBN" not in ln]      # noqa: E731
    assert strip(on) == strip(off) and not any("PBN" in ln for ln in off)       # the training-loss lines: the same bits
    assert sum(ln.startswith(" step ") for ln in off) == 3
    assert sorted(ck_on) == sorted(list(ck_off) + ["ema_precise_bn_state_dict", "precise_bn_state_dict"])
    assert "precise_bn_state_dict" not in ck_off and "ema_state_dict" in ck_off
    for key in ("precise_bn_state_dict", "ema_precise_bn_state_dict"):
        rec = ck_on[key]
        assert sorted(rec) == ["batches", "cells", "model"] and rec["batches"] == 2 and rec["cells"] % 2 == 0
        assert list(rec["model"]) == list(ck_on["model_state_dict"])
        assert all(bool(torch.isfinite(v).all()) for k, v in rec["model"].items() if "running_" in k)
    same = [k for k in ck_off["model_state_dict"] if not torch.equal(ck_on["model_state_dict"][k], ck_off["model_state_dict"][k])]
    assert same == []                                    # the model a run leaves is the same with and without the flag
    ea, eb = ck_on["ema_state_dict"]["model"], ck_off["ema_state_dict"]["model"]
    assert all(torch.equal(ea[k], eb[k]) for k in ea)


def test_charades_script_precise_bn_flag(tmp_path, capsys):
    from tests import charades_ref as cr
    import train_x3d_charades as mod
    _dev()
    anno, _ = cr.load_fixture()
    out = {}
    for name, kw in (("on", dict(ema_decay=0.9, precise_bn=2)), ("off", {})):
        torch.manual_seed(5)
        res = mod.run(init_lr=0.01, max_epochs=1, anno=anno, batch_size=4, save_model=str(tmp_path / (name + "_")),
                      save_every=6, use_graph=False, crop_size=64, c_size=64, dropout=0.5, seed=1, **kw)
        assert res["steps"] == 6 and len(res["checkpoints"]) == 1
        out[name] = (capsys.readouterr().out.splitlines(), res)
    (on, res_on), (off, res_off) = out["on"], out["off"]
    tail = r"Epoch:\d+ val Loc Cls Loss: \d+\.\d{4} Tot Loss: \d+\.\d{4} mAP: \d\.\d{4}$"
    order = [i for p in ("", "PBN ", "EMA ", "EMA PBN ") for i, ln in enumerate(on) if re.match("^ " + p + tail, ln)]
    assert len(order) == 4 and order[0] < order[1] < order[2] < order[3]
    assert [ln for ln in on if "EMA" not in ln and "PBN" not in ln] == off and not any("PBN" in ln for ln in off)
    assert "precise_bn" in vars(res_on["optimizer"]) and "precise_bn" not in vars(res_off["optimizer"])
    assert {"pbn_map", "pbn_loss", "ema_pbn_map", "ema_pbn_loss"} <= set(res_on["phases"][-1])
    assert "pbn_map" not in res_off["phases"][-1]
    # the checkpoint at step 6 was written during training, before the first 'val' phase: no record yet, and none by default
    ck_off = torch.load(res_off["checkpoints"][0], map_location="cpu")
    assert sorted(ck_off) == ["model_state_dict", "optimizer_state_dict", "scheduler_state_dict"]
    again = mod.run(init_lr=0.01, max_epochs=3, anno=anno, batch_size=4, save_model=str(tmp_path / "again_"), save_every=9,
                    use_graph=False, crop_size=64, c_size=64, seed=1, precise_bn=1)
    capsys.readouterr()
    ck = torch.load(again["checkpoints"][0], map_location="cpu")
    assert sorted(ck) == ["model_state_dict", "optimizer_state_dict", "precise_bn_state_dict", "scheduler_state_dict"]
    assert ck["precise_bn_state_dict"]["batches"] == 1
