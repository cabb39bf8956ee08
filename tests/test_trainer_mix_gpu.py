"""Trainer(objective="soft_ce") and the BatchMixer on the GPU: eager against the autograd path of model(x) with
F.cross_entropy on probabilities and torch.optim.SGD, one-hot targets against objective="ce", single graph and split graph
against eager bit for bit, gradient accumulation, dropout across replays, the refusals, the mixer writing into the graph's
static inputs, and a short training run with mixup, CutMix and label smoothing.  Same setup as tests/test_charades_gpu.py:
X3D-M, B = 2, T = 4, 64 x 64, here with the 400 Kinetics classes."""
import math
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import mix_cases as mc
from tests.test_charades_gpu import LR, MOM, WD, _assert_bitwise, _clips, _model, _per_tensor_rel, _trainer
from x3dhip import mixing, mixops

pytestmark = pytest.mark.gpu

NC = 400


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _labels(B, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, NC, size=(B, 1)))


def _soft(B, seed, lam=0.3, smoothing=0.1):
    """Soft targets [B, NC] as the mixer makes them (the twin on a hand-built plan): every row sums to 1."""
    y = _labels(B, seed).numpy()
    return torch.from_numpy(mixops.mix_targets_host(y, mc.make_plan(B, lam=lam), NC, smoothing))


def _net(dev, seed, dropout=0.0):
    return _model(dev, dropout=dropout, seed=seed, n_classes=NC)


# --------------------------------------------------------------------------- eager against autograd
def test_trainer_soft_ce_eager_equals_autograd_sgd():
    dev = _dev()
    x, y = _clips(2, seed=31).to(dev), _soft(2, 31).to(dev)
    a = _net(dev, 2)
    tr = _trainer(a, "soft_ce")
    loss, logits = tr.train_step(x, y)
    assert logits.shape == (2, NC, 1) and tr.last_losses is None
    b = _net(dev, 2)
    opt = torch.optim.SGD(b.parameters(), lr=LR, momentum=MOM, weight_decay=WD)
    opt.zero_grad()
    ref = F.cross_entropy(b(x).view(2, NC), y)
    ref.backward()
    opt.step()
    ref = ref.detach()
    torch.cuda.synchronize()
    print("soft_ce eager: loss %.9g autograd %.9g" % (float(loss), float(ref)))
    assert abs(float(loss) - float(ref)) <= 1e-6 * abs(float(ref))
    assert _per_tensor_rel(list(a.parameters()), list(b.parameters())) <= 1e-5


def test_one_hot_float_targets_equal_the_hard_label_objective():
    dev = _dev()
    x, y = _clips(2, seed=32).to(dev), _labels(2, 32).to(dev)
    onehot = F.one_hot(y.view(-1), NC).float()
    a, b = _net(dev, 3), _net(dev, 3)
    la, _ = _trainer(a, "soft_ce").train_step(x, onehot)
    lb, _ = _trainer(b, "ce").train_step(x, y)
    torch.cuda.synchronize()
    print("one-hot soft_ce %.9g ce %.9g, bits equal %s" % (float(la), float(lb), torch.equal(la.view(()), lb.view(()))))
    assert abs(float(la) - float(lb)) <= 1e-6 * abs(float(lb))
    assert _per_tensor_rel(list(a.parameters()), list(b.parameters())) <= 1e-5


# --------------------------------------------------------------------------- graphs
def _run(batches, dev, seed=5, dropout=0.0, **kw):
    net = _net(dev, seed, dropout)
    tr = _trainer(net, "soft_ce", **kw)
    out = []
    for x, y in batches:
        loss, _ = tr.train_step(x, y)
        out.append((loss.detach().clone(), None, tr.fp.grad.clone(), tr.fp.flat.clone()))
    torch.cuda.synchronize()
    return out, tr


def test_graph_and_split_graph_equal_eager_bitwise():
    dev = _dev()
    batches = [(_clips(2, seed=50 + i).to(dev), _soft(2, 50 + i, lam=[1.0, 0.75, 0.3][i]).to(dev)) for i in range(3)]
    eager, _ = _run(batches, dev)
    graph, tg = _run(batches, dev, use_graph=True)
    assert len(tg._graphs) == 1 and all(k[-2:] == ("soft_ce", (2, NC)) for k in tg._graphs)
    _assert_bitwise(eager, graph)
    split, ts = _run(batches, dev, use_graph=True, force_split=True)
    assert ts._overlap() and all(k[0] == "split" for k in ts._graphs)
    _assert_bitwise(eager, split)


def test_gradient_accumulation_equals_one_big_step():
    dev = _dev()
    xs = [_clips(2, seed=s).to(dev) for s in (71, 72)]
    ys = [_soft(2, s).to(dev) for s in (71, 72)]
    m1 = _net(dev, 6)
    t1 = _trainer(m1, "soft_ce", num_steps_per_update=2, use_graph=True)
    w_before = t1.fp.flat.clone()
    t1.train_step(xs[0], ys[0])
    assert not t1.stepped and torch.equal(t1.fp.flat, w_before)
    t1.train_step(xs[1], ys[1])
    assert t1.stepped
    m2 = _net(dev, 6)
    t2 = _trainer(m2, "soft_ce")
    t2._fwd_bwd(xs[0], ys[0])
    g0 = t2.fp.grad.clone()
    t2._fwd_bwd(xs[1], ys[1])
    g = 0.5 * (g0 + t2.fp.grad)
    expect = w_before - LR * (g + WD * w_before)
    torch.cuda.synchronize()
    assert ((t1.fp.flat - expect).norm() / (LR * g.norm())).item() < 1e-4


def test_dropout_draws_fresh_masks_per_replay():
    dev = _dev()
    x, y = _clips(2, seed=81).to(dev), _soft(2, 81).to(dev)
    mg, me = _net(dev, 7, dropout=0.5), _net(dev, 7, dropout=0.5)
    tg, te = _trainer(mg, "soft_ce", use_graph=True), _trainer(me, "soft_ce")
    tg.train_step(x, y)                                      # capture (+ warm-up) and the first replay
    torch.cuda.synchronize()
    rg = mg._head_rng(dev)
    losses = []
    for _ in range(2):
        te.fp.flat.copy_(tg.fp.flat)                         # fresh eager step from the same parameters and counter
        me._head_rng(dev).copy_(rg)
        ctr = int(rg[1])
        loss, _ = tg.train_step(x, y)
        torch.cuda.synchronize()
        assert int(rg[1]) == ctr + 1                         # one draw per step, as with "ce"
        le, _ = te._fwd_bwd(x, y)
        torch.cuda.synchronize()
        assert int(me._head_rng(dev)[1]) == ctr + 1
        assert torch.equal(te.fp.grad, tg.fp.grad)
        assert torch.equal(le.view(()), loss.view(()))
        losses.append(float(loss))
    assert losses[0] != losses[1]                            # same batch, different dropout masks


# --------------------------------------------------------------------------- refusals
def test_trainer_argument_errors_launch_nothing():
    dev = _dev()
    import x3d
    with pytest.raises(ValueError):
        _trainer(x3d.generate_model("M", n_classes=NC, dropout=0.0, base_bn_splits=1, task="loc"), "soft_ce")
    x = _clips(2, seed=91).to(dev)
    bad = [torch.zeros(2, 1, dtype=torch.int64, device=dev),             # hard labels
           torch.zeros(2, NC, dtype=torch.float64, device=dev),
           torch.zeros(2, NC + 1, device=dev),                           # wrong C
           torch.zeros(3, NC, device=dev),                               # wrong B
           torch.zeros(2, NC, 1, device=dev),
           torch.zeros(2, NC)]                                           # on the host
    net = _net(dev, 8, dropout=0.5)
    for use_graph in (False, True):
        tr = _trainer(net, "soft_ce", use_graph=use_graph)
        torch.cuda.synchronize()
        flat, rng, pending = tr.fp.flat.clone(), net._head_rng(dev).clone(), net._pending_tracked
        for y in bad:
            with pytest.raises(ValueError):
                tr.train_step(x, y)
        torch.cuda.synchronize()
        assert torch.equal(tr.fp.flat, flat) and torch.equal(net._head_rng(dev), rng)
        assert net._pending_tracked == pending and not tr._graphs


def test_default_trainer_and_script_are_untouched():
    dev = _dev()
    tr = _trainer(_net(dev, 9), "ce")
    assert tr.objective == "ce" and not [k for k in vars(tr) if "mix" in k or "soft" in k]
    assert tr._objective_key(torch.zeros(2, 1)) == ()
    import inspect
    import train_x3d_kinetics_multigrid as script
    sig = inspect.signature(script.run).parameters
    assert not script.mixing_on(**{k: sig[k].default for k in ("mixup", "cutmix", "mix_prob", "mix_switch_prob",
                                                               "label_smoothing")})


# --------------------------------------------------------------------------- the mixer and the graph's static inputs
def test_mixer_into_static_inputs_equals_fresh_tensors():
    dev = _dev()
    xs = [_clips(2, seed=60 + i).to(dev) for i in range(4)]
    ys = [_labels(2, 60 + i).to(dev) for i in range(4)]
    kw = dict(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, per_sample=True, seed=12)

    def run(static):
        net = _net(dev, 10)
        tr = _trainer(net, "soft_ce", use_graph=True)
        m = mixing.BatchMixer(NC, **kw)
        out, used = [], 0
        for x, y in zip(xs, ys):
            st = tr.static_inputs(x.shape) if static else None
            used += st is not None
            mx, soft = m(x, y, out=st)
            if st is not None:
                assert mx is st[0] and soft is st[1]
            loss, _ = tr.train_step(mx, soft)
            out.append((loss.detach().clone(), None, tr.fp.grad.clone(), tr.fp.flat.clone()))
        torch.cuda.synchronize()
        return out, used
    fresh, n0 = run(False)
    static, n1 = run(True)
    assert n0 == 0 and n1 == 3                                # from the second step on the graph's inputs exist
    _assert_bitwise(fresh, static)


# --------------------------------------------------------------------------- a short run
def test_mixup_cutmix_smoothing_smoke():
    """12 steps on four fixed batches, every step freshly mixed (mixup or CutMix, smoothing 0.1): the loss stays finite and
    goes down, by the rule of test_finetune_kinetics_model_on_multi_label_smoke."""
    import x3d
    dev = _dev()
    torch.manual_seed(0)
    net = x3d.generate_model("M", n_classes=NC, dropout=0.0, base_bn_splits=1).to(dev).train(True)
    from x3dhip.trainer import Trainer
    # the rate of every other test here (LR = 0.05): the 0.5 of the multi-label smoke suits a loss that is a mean over
    # B * 157 sigmoids, whose gradient per logit is 157 times smaller than a softmax row's
    tr = Trainer(net, lr=LR, momentum=0.9, objective="soft_ce", use_graph=True, weight_decay=1e-5)
    m = mixing.BatchMixer(NC, mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, seed=0)
    batches = [(_clips(4, seed=101 + i).to(dev), _labels(4, 101 + i).to(dev)) for i in range(4)]
    losses = []
    for k in range(12):
        x, y = batches[k % 4]
        mx, soft = m(x, y, out=tr.static_inputs(x.shape))
        loss, logits = tr.train_step(mx, soft)
        losses.append(float(loss))
    print("mix smoke losses", ["%.4f" % v for v in losses])
    assert logits.shape == (4, NC, 1)
    assert all(math.isfinite(v) for v in losses), losses
    assert losses[-1] < losses[0] and sum(losses[-3:]) < sum(losses[:3]), losses


# --------------------------------------------------------------------------- the script
def _script_run(capsys, tmp_path, name, **kw):
    import train_x3d_kinetics_multigrid as script
    torch.manual_seed(5)
    steps, _ = script.run(init_lr=0.01, warmup_steps=2, max_epochs=1, batch_size=2, steps=0, max_steps_run=4,
                          iterations_per_epoch=9, save_every=4, save_model=str(tmp_path / name), log_every=1, clip_size=32,
                          **kw)
    assert steps == 4
    return capsys.readouterr().out.splitlines(), torch.load(str(tmp_path / (name + "000004.pt")), map_location="cpu")


def test_kinetics_script_mixing_flags(capsys, tmp_path):
    """Four steps of the script's loop (captured graphs: the mixer writes into their static inputs from each shape's second
    step on) with the flags on, eagerly with the same flags, and without: one `mixing:` line when on and none when off, every
    loss finite, acc a fraction of the hard labels, the same checkpoint keys."""
    _dev()
    flags = dict(mixup=0.8, cutmix=1.0, label_smoothing=0.1)
    on, ck_on = _script_run(capsys, tmp_path, "on_", **flags)
    eager, _ = _script_run(capsys, tmp_path, "eager_", use_graph=False, **flags)
    off, ck_off = _script_run(capsys, tmp_path, "off_")
    want = "mixing: mixup alpha 0.8 cutmix alpha 1 prob 1 switch prob 0.5 label smoothing 0.1"
    assert on.count(want) == 1 and eager.count(want) == 1 and not any(ln.startswith("mixing") for ln in off)
    for lines in (on, eager, off):
        steps = [re.match(r"^ step \d+ long \d+ shape \(\d+,\d+,\d+\) loss (\S+) acc (\S+) lr", ln) for ln in lines]
        steps = [m for m in steps if m]
        assert len(steps) == 4
        assert all(math.isfinite(float(m.group(1))) and 0.0 <= float(m.group(2)) <= 1.0 for m in steps)
    strip = lambda lines: [re.sub(r"  \d+\.\d clips/s", "", ln) for ln in lines if ln.startswith(" step ")]      # noqa: E731
    assert strip(on) != strip(off) and strip(eager) != strip(off)
    assert sorted(ck_on) == sorted(ck_off)
    assert sorted(ck_on["optimizer_state_dict"]) == sorted(ck_off["optimizer_state_dict"])
