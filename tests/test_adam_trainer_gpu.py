"""Trainer(optimizer="adamw" | "lamb") on the GPU: every update of the eager / graph / split-graph / accumulation / guarded
forms of the step against x3dstep_adam_host and the x3dstep_lamb_*_host twins on the step's own inputs, bit for bit, and the
forms against each other; a poisoned batch under the guard; the weight average over the applied updates; the checkpoint round
trip, also into torch.optim.AdamW; the defaults."""
import copy
import re

import numpy as np
import pytest
import torch

from tests.test_trainer_guard_gpu import LR, _dev, _fixture, _running, _state, _trainer
from x3dhip import _steplib, stepops

pytestmark = pytest.mark.gpu

WD = 0.01
BETAS = (0.9, 0.999)
EPS = 1e-6
_EAGER = {}


class _Twin:
    """The host side of a run: the tables of the trainer's flat buffer, its scales and flags, a state and a ring."""

    def __init__(self, tr, max_norm=0.0):
        self.t = stepops.StepTables(stepops.segment_table([k for _, k in tr.fp.offsets]))
        self.hy = np.zeros(self.t.S, dtype=_steplib.HYPER_DT)
        self.hy["lr_scale"], self.hy["wd_scale"] = tr.hyper.lr_scale, tr.hyper.wd_scale
        self.mode = tr.adam.mode
        self.state = stepops.new_state()
        self.R = 4
        self.ws = stepops.aligned_bytes(self.t.workspace_bytes)
        self.ring = stepops.aligned_bytes(self.R * self.t.record_bytes)
        self.max_norm = max_norm
        self.updates = 0
        if self.mode == "lamb":
            self.adapt = tr.adam.adapt.copy()
            self.lws = stepops.aligned_bytes(stepops.lamb_workspace_bytes(self.t.nitems))
            self.wsumsq, self.rsumsq = np.zeros(self.t.S, np.float64), np.zeros(self.t.S, np.float64)
            self.trust = np.ones(self.t.S, np.float32)

    def update(self, w, g, m, v, guarded):
        """g: the gradient as it stood right before the update.  What the Trainer enqueues: measure (guarded), then the
        update as the next applied one."""
        w, m, v = w.copy(), m.copy(), v.copy()
        st = (self.state, self.ring, self.R) if guarded else (None, None, 0)
        if guarded:
            stepops.measure_host(g, self.t, self.ws, self.state, self.ring, self.R, self.max_norm, 1.0)
            count = 0
        else:
            self.updates += 1
            count = self.updates
        if self.mode == "lamb":
            stepops.lamb_moments_host(w, g, m, v, self.t, self.hy, *st, count, self.lws, BETAS, EPS, WD, 1.0)
            stepops.lamb_trust_host(self.t, self.hy, self.adapt, *st, count, self.lws, self.wsumsq, self.rsumsq, self.trust)
            stepops.lamb_apply_host(w, m, v, self.t, self.hy, self.trust, *st, count, LR, BETAS, EPS, WD)
        else:
            stepops.adam_host(w, g, m, v, self.t, self.hy, *st, count, LR, BETAS, EPS, WD, 1.0, self.mode == "adamw")
        return w, m, v


def _np(t):
    return t.detach().cpu().numpy().copy()


def _make(sd, S, dev, opt, **kw):
    return _trainer(sd, S, dev, optimizer=opt, betas=BETAS, adam_eps=EPS, weight_decay=WD, **kw)


def _follow(tr, clips, y, guarded=False, max_norm=0.0):
    """Run the clips; after each update fp.flat, fp.mom and the second moment must be the twins' on the gradient the step
    left in fp.grad (the accumulation buffer under accumulation) and on the buffers as they stood before the update."""
    twin = _Twin(tr, max_norm)
    seen, snap = [], {}

    def pre_step():
        torch.cuda.synchronize()
        snap["w"], snap["m"], snap["v"] = _np(tr.fp.flat), _np(tr.fp.mom), _np(tr.adam.exp_avg_sq)

    for x in clips:
        tr.train_step(x, y, pre_step=pre_step)
        if not tr.stepped:
            continue
        torch.cuda.synchronize()
        g = _np(tr.accum if tr.accum is not None else tr.fp.grad)
        w1, m1, v1 = twin.update(snap["w"], g, snap["m"], snap["v"], guarded)
        for name, got, want in (("w", tr.fp.flat, w1), ("m", tr.fp.mom, m1), ("v", tr.adam.exp_avg_sq, v1)):
            assert torch.equal(got.cpu().view(torch.int32), torch.from_numpy(want).view(torch.int32)), (name, len(seen))
        if twin.mode == "lamb":
            assert _np(tr.adam.wsumsq).tobytes() == twin.wsumsq.tobytes() and _np(tr.adam.rsumsq).tobytes() == twin.rsumsq.tobytes()
            assert torch.equal(tr.adam.trust.cpu(), torch.from_numpy(twin.trust))
        seen.append((snap["w"], g, snap["m"], snap["v"], w1, m1, v1))
    return seen, twin


def _eager(golden_dir, dev, opt):
    """(w, m, v) after three eager updates: computed once per optimizer, shared by the forms, never changed."""
    if opt not in _EAGER:
        sd, S, xs, bad, y = _fixture(golden_dir, dev)
        tr = _make(sd, S, dev, opt)
        seen, _ = _follow(tr, xs[:3], y)
        assert len(seen) == 3
        _EAGER[opt] = tuple(x.copy() for x in seen[2][4:])
    return _EAGER[opt]


@pytest.mark.parametrize("opt", ["adamw", "lamb"])
@pytest.mark.parametrize("form", ["eager", "graph", "split", "accum"])
def test_three_updates_are_the_twins_and_the_forms_agree(golden_dir, form, opt):
    dev = _dev()
    want = _eager(golden_dir, dev, opt)
    sd, S, xs, bad, y = _fixture(golden_dir, dev)
    kw = dict(eager={}, graph=dict(use_graph=True), split=dict(use_graph=True, force_split=True),
              accum=dict(num_steps_per_update=2))[form]
    tr = _make(sd, S, dev, opt, **kw)
    assert hasattr(tr, "hyper") and not hasattr(tr, "monitor") and tr.adam.mode == opt
    assert tr.param_groups[0]["betas"] == BETAS and tr.param_groups[0]["amsgrad"] is False
    # under accumulation every clip is fed twice: g / 2 + g / 2 is g, bit for bit
    clips = [x for x in xs[:3] for _ in range(2)] if form == "accum" else xs[:3]
    seen, _ = _follow(tr, clips, y)
    assert len(seen) == 3 and tr._overlap() == (form == "split")
    for got, ref in zip(seen[2][4:], want):
        assert got.tobytes() == ref.tobytes()
    assert np.all(np.isfinite(seen[2][4])) and not np.array_equal(seen[0][0], seen[2][4]) and tr.adam.step() == 3
    if opt == "lamb":
        got = tr.adam.read()
        one_d = [k for k, p in tr.model.named_parameters() if p.dim() <= 1]
        assert len(one_d) == 199 and all(got["trust"][k] == 1.0 for k in one_d)
        assert all(got["trust"][k] != 1.0 and got["wnorm"][k] > 0 and got["rnorm"][k] > 0
                   for k, p in tr.model.named_parameters() if p.dim() > 1)


@pytest.mark.parametrize("opt", ["adamw", "lamb"])
def test_a_poisoned_batch_under_the_guard_is_skipped_and_the_count_does_not_advance(golden_dir, opt):
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev)
    tr = _make(sd, S, dev, opt, skip_nonfinite=True, clip_grad_norm=0.5, use_graph=True)
    seen, twin = _follow(tr, [xs[0]], y, guarded=True, max_norm=0.5)
    before, v0 = _state(tr), tr.adam.exp_avg_sq.clone()
    tr.train_step(bad, y)
    after = _state(tr)
    assert all(torch.equal(after[k], before[k]) for k in before) and torch.equal(tr.adam.exp_avg_sq, v0)
    assert tr.monitor.state.cpu()[5:].tolist() == [1, 1, 1] and tr.adam.step() == 1
    # the twin sees the same three gradients; its state words give the third update k = 2, as the device's do
    stepops.measure_host(_np(tr.fp.grad), twin.t, twin.ws, twin.state, twin.ring, twin.R, 0.5, 1.0)
    w, m, v = _np(tr.fp.flat), _np(tr.fp.mom), _np(tr.adam.exp_avg_sq)
    if opt == "lamb":
        stepops.lamb_moments_host(w, _np(tr.fp.grad), m, v, twin.t, twin.hy, twin.state, twin.ring, twin.R, 0, twin.lws, BETAS,
                                  EPS, WD, 1.0)
        stepops.lamb_apply_host(w, m, v, twin.t, twin.hy, twin.trust, twin.state, twin.ring, twin.R, 0, LR, BETAS, EPS, WD)
    else:
        stepops.adam_host(w, _np(tr.fp.grad), m, v, twin.t, twin.hy, twin.state, twin.ring, twin.R, 0, LR, BETAS, EPS, WD, 1.0, 1)
    assert w.tobytes() == _np(tr.fp.flat).tobytes() and twin.state[5:].tolist() == [1, 1, 1]      # the twin skipped as well

    def pre_step():
        torch.cuda.synchronize()
        snap.update(w=_np(tr.fp.flat), m=_np(tr.fp.mom), v=_np(tr.adam.exp_avg_sq))

    snap = {}
    tr.train_step(xs[1], y, pre_step=pre_step)
    torch.cuda.synchronize()
    w1, m1, v1 = twin.update(snap["w"], _np(tr.fp.grad), snap["m"], snap["v"], True)
    assert w1.tobytes() == _np(tr.fp.flat).tobytes() and v1.tobytes() == _np(tr.adam.exp_avg_sq).tobytes()
    assert torch.equal(tr.monitor.state.cpu(), torch.from_numpy(twin.state)) and tr.adam.step() == 2
    assert tr.monitor.state.cpu()[5:].tolist() == [0, 1, 0] and not np.array_equal(w1, snap["w"])


def test_the_weight_average_takes_the_applied_updates_only(golden_dir):
    from tests.test_trainer_ema_gpu import DECAY, _average, _ema_stats, _iterate
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev)
    tr = _make(sd, S, dev, "adamw", ema_decay=DECAY, skip_nonfinite=True)
    start, hist = _iterate(tr), []
    for x in (xs[0], bad, xs[1]):
        tr.train_step(x, y)
        if x is not bad:
            hist.append(_iterate(tr))
    e, stats = _average(start, hist)
    torch.cuda.synchronize()
    assert torch.equal(tr.ema.e.cpu(), torch.from_numpy(e)) and tr.ema.updates() == 2 == tr.adam.step()
    got = _ema_stats(tr)
    assert all(torch.equal(got[k].cpu(), torch.from_numpy(stats[k])) for k in stats) and len(stats) == 168


def _to_cpu(d):
    return {k: (_to_cpu(v) if isinstance(v, dict) else v.cpu().clone() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


@pytest.mark.parametrize("opt,kw", [("adamw", {}), ("lamb", dict(skip_nonfinite=True))], ids=["adamw", "lamb-guarded"])
def test_checkpoint_round_trip(golden_dir, opt, kw):
    """Save at 2, resume in a new model and Trainer, and step 3 equals the uninterrupted run bit for bit."""
    import x3d
    from x3dhip.trainer import Trainer
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev)
    lamb = dict(lamb=dict(exempt=("fc2.weight",))) if opt == "lamb" else {}
    tr = _make(sd, S, dev, opt, **kw, **lamb)
    assert tr.state_dict()["state"] == {}
    for i in range(2):
        tr.train_step(xs[i], y)
    ck = dict(model=_to_cpu(tr.model.state_dict()), opt=_to_cpu(tr.state_dict()))
    assert sorted(ck["opt"]) == sorted(["optimizer", "param_groups", "state", "tensor_hyper"] + (["lamb"] if opt == "lamb" else []))
    assert ck["opt"]["optimizer"] == opt and sorted(ck["opt"]["state"][0]) == ["exp_avg", "exp_avg_sq", "step"]
    assert float(ck["opt"]["state"][315]["step"]) == 2.0 and ck["opt"]["param_groups"][0]["amsgrad"] is False
    tr.train_step(xs[2], y)
    net = x3d.generate_model("M", n_classes=400, dropout=0.0, base_bn_splits=S)
    net.load_state_dict(ck["model"])
    net.to(dev).train(True)
    again = Trainer(net, lr=LR, optimizer=opt, betas=BETAS, adam_eps=EPS, weight_decay=WD, **kw)
    again.load_state_dict(ck["opt"])
    assert again.adam.step() == 2
    if opt == "lamb":
        assert np.array_equal(again.adam.adapt, tr.adam.adapt) and int(again.adam.adapt.sum()) == 116
    again.train_step(xs[2], y)
    torch.cuda.synchronize()
    assert torch.equal(again.fp.flat, tr.fp.flat) and torch.equal(again.fp.mom, tr.fp.mom)
    assert torch.equal(again.adam.exp_avg_sq, tr.adam.exp_avg_sq) and again.adam.step() == 3
    # a checkpoint of another optimizer raises, either way; an SGD checkpoint into an SGD trainer loads as ever
    plain = _trainer(sd, S, dev)
    plain.train_step(xs[0], y)
    sgd_ck = _to_cpu(plain.state_dict())
    with pytest.raises(ValueError):
        again.load_state_dict(sgd_ck)
    with pytest.raises(ValueError):
        plain.load_state_dict(ck["opt"])
    other = _trainer(sd, S, dev)
    other.load_state_dict(sgd_ck)
    assert torch.equal(other.fp.mom, plain.fp.mom) and other.first is False


def test_the_adamw_checkpoint_loads_into_torch_and_one_more_step_agrees(golden_dir):
    """state_dict() after two updates into torch.optim.AdamW over the same shapes, in fp64 and in fp32; the third update's
    gradient is the trainer's own.  The bound is the host test's: four times torch's own fp32 distance from its fp64 run."""
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev)
    tr = _make(sd, S, dev, "adamw")
    for i in range(2):
        tr.train_step(xs[i], y)
    ck = _to_cpu(tr.state_dict())
    w2 = _np(tr.fp.flat)
    tr.train_step(xs[2], y)
    torch.cuda.synchronize()
    g, w3 = _np(tr.fp.grad), _np(tr.fp.flat)
    out = {}
    for dtype in (torch.float64, torch.float32):
        ps = [torch.tensor(w2[o:o + k], dtype=dtype).view(p.shape).requires_grad_() for (o, k), p in zip(tr.fp.offsets, tr.fp.params)]
        opt = torch.optim.AdamW(ps, lr=LR, foreach=False)
        opt.load_state_dict(copy.deepcopy(ck))           # torch keeps the 'step' tensors it is given and counts in them
        grp = opt.param_groups[0]
        assert grp["betas"] == BETAS and grp["eps"] == EPS and grp["weight_decay"] == WD and grp["amsgrad"] is False
        assert float(opt.state[ps[0]]["step"]) == 2.0 and opt.state[ps[5]]["exp_avg_sq"].dtype == dtype
        grp.update(lr=float(np.float32(LR)), betas=tuple(float(np.float32(b)) for b in BETAS), eps=float(np.float32(EPS)),
                   weight_decay=float(np.float32(WD)))
        for (o, k), p in zip(tr.fp.offsets, ps):
            p.grad = torch.tensor(g[o:o + k], dtype=dtype).view(p.shape)
        opt.step()
        out[dtype] = np.concatenate([p.detach().double().numpy().reshape(-1) for p in ps])
    d_ours = float(np.max(np.abs(w3.astype(np.float64) - out[torch.float64])))
    d_torch = float(np.max(np.abs(out[torch.float32] - out[torch.float64])))
    print("trainer %.3e, torch fp32 %.3e from torch fp64: ratio %.3f" % (d_ours, d_torch, d_ours / d_torch))
    assert 0.0 < d_ours <= 4.0 * d_torch


def test_the_defaults_are_off(golden_dir, monkeypatch):
    """Trainer() with the defaults: no `adam` attribute, the same state_dict() keys, not one launch of the feature, and over
    two updates the weights and the momentum ops.sgd_fused gives on the step's own inputs; the loss is that of a second
    default run, bit for bit."""
    from x3dhip import ops
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev)
    calls = []
    for name in ("adam", "lamb_moments", "lamb_trust", "lamb_apply"):
        monkeypatch.setattr(stepops, name, lambda *a, _n=name, **k: calls.append(_n))
    a, b = _trainer(sd, S, dev), _trainer(sd, S, dev)
    assert "adam" not in vars(a) and not hasattr(a, "hyper") and not hasattr(a, "monitor")
    assert sorted(a.param_groups[0]) == ["dampening", "lr", "momentum", "nesterov", "params", "weight_decay"]
    snap = {}

    def pre_step():
        snap.update(w=a.fp.flat.clone(), m=a.fp.mom.clone(), first=a.first)

    for i in range(2):
        la, _ = a.train_step(xs[i], y, pre_step=pre_step)
        lb, _ = b.train_step(xs[i], y)
        w, m = snap["w"], snap["m"]
        g0 = a.param_groups[0]
        ops.sgd_fused(w, a.fp.grad, m, g0["lr"], g0["momentum"], g0["weight_decay"], 1.0, first=snap["first"])
        torch.cuda.synchronize()
        assert torch.equal(w.view(torch.int32), a.fp.flat.view(torch.int32)) and torch.equal(m.view(torch.int32), a.fp.mom.view(torch.int32))
        assert torch.equal(la.view(torch.int32), lb.view(torch.int32)) and torch.equal(a.fp.flat, b.fp.flat)
    assert calls == [] and sorted(a.state_dict()) == ["param_groups", "state"]
    assert sorted(a.state_dict()["state"][0]) == ["momentum_buffer"]
    for kw in (dict(optimizer="adamw", nesterov=True), dict(optimizer="lamb", lars=0.001), dict(optimizer="rmsprop"),
               dict(lamb=dict(exempt_1d=False)), dict(optimizer="lamb", lamb=dict(eta=1.0)),
               dict(optimizer="lamb", lamb=dict(exempt=("no.such.parameter*",))), dict(optimizer="adamw", betas=(0.9, 1.0)),
               dict(optimizer="adamw", adam_eps=-1.0)):
        with pytest.raises(ValueError):
            _trainer(sd, S, dev, **kw)
    assert _running(a).keys() == _running(b).keys()


# -- the scripts ------------------------------------------------------------------------------------------------------------
LINE = re.compile(r"^optimizer (adamw|adam|lamb): betas \(0\.9, 0\.99\), eps 1e-06, (\d+) of 316 tensors exempt from decay"
                  r"(, 199 exempt from adaptation)?$")
TRUST = re.compile(r" trust [\d.e+-]+/[\d.e+-]+/[\d.e+-]+")


def test_kinetics_script_flags(capsys, tmp_path):
    import train_x3d_kinetics_multigrid as tr
    _dev()
    torch.manual_seed(5)
    steps, _ = tr.run(init_lr=0.001, warmup_steps=2, max_epochs=1, batch_size=2, steps=0, max_steps_run=3,
                      iterations_per_epoch=9, save_every=3, save_model=str(tmp_path / "on_"), use_graph=False, log_every=1,
                      clip_size=32, optimizer_name="lamb", betas=(0.9, 0.99), adam_eps=1e-6, wd_exempt_1d=True)
    assert steps == 3
    on = capsys.readouterr().out.splitlines()
    ck = torch.load(str(tmp_path / "on_000003.pt"), map_location="cpu")["optimizer_state_dict"]
    hit = [ln for ln in on if LINE.match(ln)]
    assert len(hit) == 1 and LINE.match(hit[0]).groups() == ("lamb", "199", ", 199 exempt from adaptation")
    steps_on = [ln for ln in on if ln.startswith(" step ")]
    assert on.index(hit[0]) < on.index(steps_on[0]) and len(steps_on) == 3 and all(TRUST.search(ln) for ln in steps_on)
    assert sorted(ck) == ["lamb", "optimizer", "param_groups", "state", "tensor_hyper"] and ck["optimizer"] == "lamb"
    assert float(ck["state"][0]["step"]) == 3.0 and ck["lamb"]["adapt"][ck["lamb"]["names"].index("bn1.weight")] == 0
    assert ck["param_groups"][0]["betas"] == (0.9, 0.99)


def test_charades_script_flags(tmp_path, capsys):
    from tests import charades_ref as cr
    import train_x3d_charades as mod
    _dev()
    anno, _ = cr.load_fixture()
    torch.manual_seed(5)
    res = mod.run(init_lr=0.001, max_epochs=1, anno=anno, batch_size=4, save_model=str(tmp_path / "on_"), save_every=3,
                  use_graph=False, crop_size=64, c_size=64, dropout=0.5, seed=1, optimizer_name="adamw", betas=(0.9, 0.99),
                  adam_eps=1e-6)
    on = capsys.readouterr().out.splitlines()
    assert res["steps"] == 6
    hit = [ln for ln in on if LINE.match(ln)]
    assert len(hit) == 1 and LINE.match(hit[0]).groups() == ("adamw", "0", None)
    assert not any(TRUST.search(ln) for ln in on)
    ck = torch.load(res["checkpoints"][0], map_location="cpu")
    assert sorted(ck["optimizer_state_dict"]) == ["optimizer", "param_groups", "state", "tensor_hyper"]
    again = mod.run(init_lr=0.001, max_epochs=0, anno=anno, batch_size=4, save_model=str(tmp_path / "again_"), save_every=0,
                    use_graph=False, crop_size=64, c_size=64, seed=1, resume=res["checkpoints"][0], optimizer_name="adamw",
                    betas=(0.9, 0.99), adam_eps=1e-6)
    capsys.readouterr()
    assert again["optimizer"].adam.step() == 3                        # restored from the checkpoint
    with pytest.raises(ValueError):
        mod.run(init_lr=0.001, max_epochs=0, anno=anno, batch_size=4, save_model=str(tmp_path / "sgd_"), save_every=0,
                use_graph=False, crop_size=64, c_size=64, seed=1, resume=res["checkpoints"][0])
