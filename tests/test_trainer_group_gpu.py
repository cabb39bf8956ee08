"""Trainer(tensor_hyper=, nesterov=) on the GPU: every update of the eager / graph / split-graph / accumulation / RCCL /
guarded forms of the step against x3dstep_apply_groups_host on the step's own inputs, bit for bit; three steps against
torch.optim.SGD with parameter groups in fp64; an exempt tensor; the weight average over the grouped iterates; the
checkpoint round trip; the defaults; the flags of the training scripts."""
import re

import numpy as np
import pytest
import torch

from tests import group_ref
from tests.test_trainer_guard_gpu import LR, _dev, _fixture, _state, _trainer
from x3dhip import _steplib, stepops
from x3dhip.hypergroups import recipe

pytestmark = pytest.mark.gpu

MU, WD = 0.9, 5e-5


def _grouped(sd, S, dev, **kw):
    import x3d
    probe = x3d.generate_model("M", n_classes=400, dropout=0.0, base_bn_splits=S)
    kw.setdefault("tensor_hyper", recipe(probe, wd_exempt_1d=True, head_lr_scale=10))
    kw.setdefault("nesterov", True)
    return _trainer(sd, S, dev, **kw)


class _Twin:
    """The host side of a run: the tables of the trainer's flat buffer, its scales, and (guarded) a state and a ring."""

    def __init__(self, tr, max_norm=0.0):
        self.t = stepops.StepTables(stepops.segment_table([k for _, k in tr.fp.offsets]))
        self.hy = np.zeros(self.t.S, dtype=_steplib.HYPER_DT)
        self.hy["lr_scale"], self.hy["wd_scale"] = tr.hyper.lr_scale, tr.hyper.wd_scale
        self.state = stepops.new_state()
        self.R = 4
        self.ws = stepops.aligned_bytes(self.t.workspace_bytes)
        self.ring = stepops.aligned_bytes(self.R * self.t.record_bytes)
        self.max_norm = max_norm

    def update(self, w, g, m, first, guarded, nesterov=True, wd=WD):
        w, m = w.copy(), m.copy()
        if guarded:
            stepops.measure_host(g, self.t, self.ws, self.state, self.ring, self.R, self.max_norm, 1.0)
        stepops.apply_groups_host(w, g, m, self.t, self.hy, self.state if guarded else None, self.ring if guarded else None,
                                  self.R, LR, MU, wd, 1.0, first, nesterov)
        return w, m


def _np(t):
    return t.detach().cpu().numpy().copy()


def _follow(tr, clips, y, guarded=False, max_norm=0.0):
    """Run the clips; before each update snapshot w and m (pre_step runs right before it), afterwards take the gradient the
    update read, and require w and m to be the twin's on those inputs.  Returns the per-update (w0, g, m0, w1, m1)."""
    twin = _Twin(tr, max_norm)
    seen, snap = [], {}

    def pre_step():
        torch.cuda.synchronize()
        snap["w"], snap["m"], snap["first"] = _np(tr.fp.flat), _np(tr.fp.mom), tr.first

    for x in clips:
        tr.train_step(x, y, pre_step=pre_step)
        if not tr.stepped:
            continue
        torch.cuda.synchronize()
        g = _np(tr.accum if tr.accum is not None else tr.fp.grad)
        w1, m1 = twin.update(snap["w"], g, snap["m"], snap["first"], guarded, bool(tr.param_groups[0]["nesterov"]))
        assert torch.equal(tr.fp.flat.cpu(), torch.from_numpy(w1)), "update %d" % len(seen)
        assert torch.equal(tr.fp.mom.cpu(), torch.from_numpy(m1)), "update %d" % len(seen)
        seen.append((snap["w"], g, snap["m"], w1, m1))
    return seen, twin


@pytest.mark.parametrize("kw", [dict(), dict(use_graph=True), dict(use_graph=True, force_split=True),
                                dict(use_graph=True, clip_grad_norm=0.5)],
                         ids=["eager", "graph", "split", "graph-clipped-unguarded"])
def test_three_steps_are_the_twins_on_the_steps_own_inputs(golden_dir, kw):
    """The last case has a monitor and no guard: `observe` scales the gradient in place and apply_groups(state=None) takes
    it from there, so the gradient read back after the step is the scaled one the update consumed."""
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev)
    tr = _grouped(sd, S, dev, **kw)
    assert tr.hyper.summary() == (199, 35584, 2) and tr.param_groups[0]["nesterov"] is True
    assert hasattr(tr, "monitor") == ("clip_grad_norm" in kw)
    seen, _ = _follow(tr, xs[:3], y)
    if "clip_grad_norm" in kw:
        assert all(0.0 < c < 1.0 for c in tr.monitor.read()["coef"]) and tr.monitor.state.cpu()[5:].tolist() == [0, 0, 0]
    assert len(seen) == 3 and tr._overlap() == bool(kw.get("force_split"))
    assert not np.array_equal(seen[0][0], seen[2][3]) and np.all(np.isfinite(seen[2][3]))


def test_accumulation_updates_once_per_two_micro_batches(golden_dir):
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev, clips=6)
    tr = _grouped(sd, S, dev, num_steps_per_update=2)
    seen, _ = _follow(tr, xs, y)
    assert len(seen) == 3


def test_one_rank_rccl_group(golden_dir, monkeypatch):
    import torch.distributed as dist
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev)
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", "29547")
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        tr = _grouped(sd, S, dev, use_graph=True, process_group=dist.group.WORLD, world_size=1, force_split=True,
                      force_collectives=True)
        seen, _ = _follow(tr, xs[:3], y)
        assert len(seen) == 3 and tr.reducer.active and tr._overlap()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("kw", [dict(), dict(use_graph=True)], ids=["eager", "graph"])
def test_clipped_and_guarded_a_nan_clip_is_skipped(golden_dir, kw):
    """clip_grad_norm and skip_nonfinite: measure, apply_groups(state), restore.  The second clip has a NaN pixel: the update
    is skipped, and the counters are those of the guarded update."""
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev)
    tr = _grouped(sd, S, dev, clip_grad_norm=0.5, skip_nonfinite=True, **kw)
    assert tr.hyper.tables is tr.monitor.tables, "the monitor's tables are shared"
    clips = [xs[0], bad, xs[1]]
    seen, twin = _follow(tr, clips, y, guarded=True, max_norm=0.5)
    assert len(seen) == 3
    w0, g, m0, w1, m1 = seen[1]
    assert not np.all(np.isfinite(g)) and np.array_equal(w0, w1) and np.array_equal(m0, m1)
    assert torch.equal(tr.monitor.state.cpu(), torch.from_numpy(twin.state))
    assert tr.monitor.state.cpu()[5:].tolist() == [0, 1, 0]
    assert int(tr.monitor.skipped()) == 1 and int(tr.monitor.skip_run()) == 0 and tr.monitor.first_nonfinite()[0] == 1
    coef = tr.monitor.read()["coef"]
    assert 0.0 < coef[0] < 1.0 and 0.0 < coef[2] < 1.0
    assert np.all(np.isfinite(seen[2][3]))


def test_three_steps_follow_torch_sgd_with_parameter_groups_in_fp64(golden_dir):
    """torch.optim.SGD(torch_param_groups(..), momentum, nesterov=True) in fp64, fed the trainer's own per-step gradients,
    within group_ref.TorchBound: the bound derived in tests/test_group_host.py (7 roundings of 2^-24 on the way to w', 4 on
    the way to m', relative to the sums of the absolute values of the terms, carried over the steps)."""
    import x3d
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev)
    tr = _grouped(sd, S, dev)
    seen, twin = _follow(tr, xs[:3], y)
    net = x3d.generate_model("M", n_classes=400, dropout=0.0, base_bn_splits=S)
    net.load_state_dict(sd)
    net.double()
    opt = torch.optim.SGD(tr.hyper.torch_param_groups(net, LR, WD), lr=LR, momentum=float(np.float32(MU)), nesterov=True)
    assert len(opt.param_groups) == 4                     # (1, 1), (1, 0), (10, 1), (10, 0)
    off = twin.t.seg_off
    lr_s, wd_s = group_ref.tensor_rule(LR, WD, twin.hy["lr_scale"], twin.hy["wd_scale"])
    lr_e, wd_e = group_ref.per_element(lr_s, off), group_ref.per_element(wd_s, off)
    params = [p for _, p in net.named_parameters()]
    flat64 = lambda: np.concatenate([p.detach().numpy().reshape(-1) for p in params])      # noqa: E731
    w64, m64 = flat64(), np.zeros(twin.t.n)
    assert np.array_equal(w64, seen[0][0].astype(np.float64))
    bound = group_ref.TorchBound(twin.t.n)
    for k, (w0, g, m0, w1, m1) in enumerate(seen):
        bw, bm = bound.step(w64, g, m64, 1.0, lr_e, wd_e, MU, 1.0, k == 0, True)
        for s, p in enumerate(params):
            p.grad = torch.from_numpy(g[int(off[s]):int(off[s + 1])].astype(np.float64)).view(p.shape)
        opt.step()
        w64 = flat64()
        m64 = np.concatenate([opt.state[p]["momentum_buffer"].numpy().reshape(-1) for p in params])
        ew, em = np.abs(w1.astype(np.float64) - w64), np.abs(m1.astype(np.float64) - m64)
        print("step %d: max err w %.3g (bound %.3g at it), m %.3g (bound %.3g at it)"
              % (k, ew.max(), bw[ew.argmax()], em.max(), bm[em.argmax()]))
        assert np.all(ew <= bw) and np.all(em <= bm)


def test_an_exempt_tensor_really_is_exempt(golden_dir):
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev)
    tr = _grouped(sd, S, dev, weight_decay=0.5, nesterov=False)
    names = [k for k, _ in tr.model.named_parameters()]
    before = _np(tr.fp.flat)
    tr.train_step(xs[0], y, pre_step=lambda: tr.fp.grad.zero_())
    torch.cuda.synchronize()
    after = _np(tr.fp.flat)
    for name in ("bn1.weight", "layer1.0.bn1.bias", "fc2.bias"):
        o, k = tr.fp.offsets[names.index(name)]
        assert before[o:o + k].tobytes() == after[o:o + k].tobytes(), name
    for name, shrink in (("conv1_s.weight", 1 - LR * 0.5), ("fc2.weight", 1 - 10 * LR * 0.5)):
        o, k = tr.fp.offsets[names.index(name)]
        b, a = before[o:o + k], after[o:o + k]
        nz = b != 0
        assert nz.any() and np.all(np.abs(a[nz]) < np.abs(b[nz]))
        assert np.allclose(a, b * np.float32(shrink), rtol=1e-5, atol=0)


def test_the_weight_average_follows_the_grouped_iterates(golden_dir):
    from tests.test_trainer_ema_gpu import DECAY, _average, _ema_stats, _iterate
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev)
    tr = _grouped(sd, S, dev, ema_decay=DECAY)
    start, hist = _iterate(tr), []
    plain = _trainer(sd, S, dev)
    for i in range(3):
        tr.train_step(xs[i], y)
        plain.train_step(xs[i], y)
        hist.append(_iterate(tr))
    e, stats = _average(start, hist)
    torch.cuda.synchronize()
    assert torch.equal(tr.ema.e.cpu(), torch.from_numpy(e)) and tr.ema.updates() == 3
    got = _ema_stats(tr)
    assert all(torch.equal(got[k].cpu(), torch.from_numpy(stats[k])) for k in stats) and len(stats) == 168
    assert not torch.equal(tr.fp.flat, plain.fp.flat), "the grouped iterates are not the plain ones"


def test_checkpoint_round_trip(golden_dir):
    """Save at 2, resume in a new model and Trainer, and step 3 equals the uninterrupted run bit for bit."""
    import x3d
    from x3dhip.trainer import Trainer
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev)
    tr = _grouped(sd, S, dev)
    tr.hyper.set("layer1.*", lr_scale=0.5)               # something the recipe alone does not give
    for i in range(2):
        tr.train_step(xs[i], y)
    to_cpu = lambda d: {k: (to_cpu(v) if isinstance(v, dict) else v.cpu().clone() if isinstance(v, torch.Tensor) else v)  # noqa: E731
                        for k, v in d.items()}
    ck = dict(model=to_cpu(tr.model.state_dict()), opt=to_cpu(tr.state_dict()))
    assert sorted(ck["opt"]) == ["param_groups", "state", "tensor_hyper"]
    assert sorted(ck["opt"]["tensor_hyper"]) == ["lr_scale", "names", "wd_scale"]
    assert ck["opt"]["param_groups"][0]["nesterov"] is True and len(ck["opt"]["param_groups"]) == 1
    tr.train_step(xs[2], y)
    net = x3d.generate_model("M", n_classes=400, dropout=0.0, base_bn_splits=S)
    net.load_state_dict(ck["model"])
    net.to(dev).train(True)
    again = Trainer(net, lr=LR, tensor_hyper={}, nesterov=True)
    assert again.hyper.summary() == (0, 0, 0)
    again.load_state_dict(ck["opt"])
    assert again.hyper.summary()[0] == 199 and np.array_equal(again.hyper.lr_scale, tr.hyper.lr_scale)
    assert torch.equal(again.hyper.hyper, tr.hyper.hyper)
    again.train_step(xs[2], y)
    torch.cuda.synchronize()
    assert torch.equal(again.fp.flat, tr.fp.flat) and torch.equal(again.fp.mom, tr.fp.mom)
    other = dict(ck["opt"], tensor_hyper=dict(ck["opt"]["tensor_hyper"], names=ck["opt"]["tensor_hyper"]["names"][::-1]))
    with pytest.raises(ValueError):
        again.load_state_dict(other)
    # a checkpoint without the key loads as before, and one with it into a Trainer without the feature
    old = {k: v for k, v in ck["opt"].items() if k != "tensor_hyper"}
    again.load_state_dict(old)
    plain = _trainer(sd, S, dev)
    plain.load_state_dict(ck["opt"])
    assert not hasattr(plain, "hyper")
    with pytest.raises(ValueError):
        _trainer(sd, S, dev, tensor_hyper={"no.such.parameter*": dict(lr_scale=2.0)})
    with pytest.raises(ValueError):
        _trainer(sd, S, dev, tensor_hyper={"fc2.*": dict(lr_scale=-1.0)})
    with pytest.raises(ValueError):
        _trainer(sd, S, dev, momentum=0.0, nesterov=True)


def test_defaults_are_off_and_all_ones_is_the_plain_update(golden_dir, monkeypatch):
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev)
    calls = []
    real = stepops.apply_groups
    monkeypatch.setattr(stepops, "apply_groups", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    plain = _trainer(sd, S, dev)
    same = _trainer(sd, S, dev, tensor_hyper=None, nesterov=False)
    ones = _trainer(sd, S, dev, tensor_hyper={})          # the feature on, every scale 1, no Nesterov
    assert "hyper" not in vars(plain) and not hasattr(same, "hyper") and hasattr(ones, "hyper")
    for i in range(2):
        plain.train_step(xs[i], y)
        same.train_step(xs[i], y)
    assert calls == []                                    # not one launch of the grouped update
    for i in range(2):
        ones.train_step(xs[i], y)
    assert len(calls) == 2
    a, b, c = _state(plain), _state(same), _state(ones)
    assert all(torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]) for k in a)
    sa, sb = plain.state_dict(), same.state_dict()
    assert sorted(sa) == sorted(sb) == ["param_groups", "state"] and sa["param_groups"] == sb["param_groups"]
    assert sa["param_groups"][0]["nesterov"] is False
    assert sorted(sa["param_groups"][0]) == sorted(["lr", "momentum", "dampening", "weight_decay", "nesterov", "params"])
    assert all(torch.equal(sa["state"][i]["momentum_buffer"], sb["state"][i]["momentum_buffer"]) for i in range(316))
    assert sorted(ones.state_dict()) == ["param_groups", "state", "tensor_hyper"]


# -- the scripts ------------------------------------------------------------------------------------------------------------
LINE = re.compile(r"^tensor hyper: 199 tensors \((\d+) elements\) exempt from weight decay, 2 tensors at a scaled learning "
                  r"rate, nesterov on$")


def test_kinetics_script_flags(capsys, tmp_path):
    import train_x3d_kinetics_multigrid as tr
    _dev()
    out = {}
    for name, kw in (("on", dict(wd_exempt_1d=True, head_lr_scale=10.0, nesterov=True)), ("off", {})):
        torch.manual_seed(5)
        steps, _ = tr.run(init_lr=0.01, warmup_steps=2, max_epochs=1, batch_size=2, steps=0, max_steps_run=3,
                          iterations_per_epoch=9, save_every=3, save_model=str(tmp_path / (name + "_")), use_graph=False,
                          log_every=1, clip_size=32, **kw)
        assert steps == 3
        out[name] = (capsys.readouterr().out.splitlines(), torch.load(str(tmp_path / (name + "_000003.pt")), map_location="cpu"))
    on, ck_on = out["on"]
    off, ck_off = out["off"]
    hit = [ln for ln in on if LINE.match(ln)]
    assert len(hit) == 1 and int(LINE.match(hit[0]).group(1)) == 35584
    assert on.index(hit[0]) < min(i for i, ln in enumerate(on) if ln.startswith(" step "))
    assert not any("tensor hyper" in ln for ln in off)
    assert [re.sub(r"[\d.e+-]+", "#", ln) for ln in on if ln is not hit[0]] == [re.sub(r"[\d.e+-]+", "#", ln) for ln in off]
    assert sorted(ck_on) == sorted(ck_off) == ["long_ind", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict"]
    assert sorted(ck_off["optimizer_state_dict"]) == ["param_groups", "state"]
    assert sorted(ck_on["optimizer_state_dict"]) == ["param_groups", "state", "tensor_hyper"]
    assert ck_on["optimizer_state_dict"]["param_groups"][0]["nesterov"] is True
    assert ck_off["optimizer_state_dict"]["param_groups"][0]["nesterov"] is False
    th = ck_on["optimizer_state_dict"]["tensor_hyper"]
    assert th["lr_scale"][th["names"].index("fc2.weight")] == 10.0 and th["wd_scale"][th["names"].index("bn1.weight")] == 0.0


@pytest.mark.parametrize("task", ["class", "loc"])
def test_charades_scripts_flags(tmp_path, capsys, task):
    from tests import charades_ref as cr
    import train_x3d_charades
    import train_x3d_charades_loc
    _dev()
    mod = train_x3d_charades if task == "class" else train_x3d_charades_loc
    anno, _ = cr.load_fixture()
    out = {}
    for name, kw in (("on", dict(wd_exempt_1d=True, head_lr_scale=10.0, nesterov=True)), ("off", {})):
        torch.manual_seed(5)
        res = mod.run(init_lr=0.01, max_epochs=1, anno=anno, batch_size=4, save_model=str(tmp_path / (name + "_")),
                      save_every=3, use_graph=False, crop_size=64, c_size=64, dropout=0.5, seed=1, **kw)
        assert res["steps"] == 6
        out[name] = (capsys.readouterr().out.splitlines(), torch.load(res["checkpoints"][0], map_location="cpu"), res)
    on, ck_on, res_on = out["on"]
    off, ck_off, res_off = out["off"]
    hit = [ln for ln in on if LINE.match(ln)]
    assert len(hit) == 1 and not any("tensor hyper" in ln for ln in off)
    assert on.index(hit[0]) < min(i for i, ln in enumerate(on) if " Epoch:" in ln)
    assert len(on) == len(off) + 1
    assert hasattr(res_on["optimizer"], "hyper") and not hasattr(res_off["optimizer"], "hyper")
    assert sorted(ck_on) == sorted(ck_off) == ["model_state_dict", "optimizer_state_dict", "scheduler_state_dict"]
    assert sorted(ck_off["optimizer_state_dict"]) == ["param_groups", "state"]
    assert sorted(ck_on["optimizer_state_dict"]) == ["param_groups", "state", "tensor_hyper"]
    th = ck_on["optimizer_state_dict"]["tensor_hyper"]
    assert th["lr_scale"][th["names"].index("fc2.bias")] == 10.0 and th["wd_scale"][th["names"].index("fc2.bias")] == 0.0
    again = mod.run(init_lr=0.01, max_epochs=0, anno=anno, batch_size=4, save_model=str(tmp_path / "again_"), save_every=0,
                    use_graph=False, crop_size=64, c_size=64, seed=1, resume=res_on["checkpoints"][0], nesterov=True)
    capsys.readouterr()
    # restored from the checkpoint, not from flags (fc2.bias has 157 elements here, not 400)
    assert again["optimizer"].hyper.summary() == (199, 35584 - 400 + 157, 2)
