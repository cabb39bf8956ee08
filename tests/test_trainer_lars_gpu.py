"""Trainer(lars=) on the GPU: every update of the eager / graph / split-graph / clipped / guarded / accumulation / RCCL forms of
the step against x3dstep_trust_host and x3dstep_apply_lars_host on the step's own inputs, bit for bit; three steps against a
LARS in plain torch, fp64; the exempt tensors; the weight average over the LARS iterates; the checkpoint round trip; the
defaults; the flags of the training scripts."""
import re

import numpy as np
import pytest
import torch

from tests import group_ref, lars_ref
from tests.test_trainer_guard_gpu import LR, _dev, _fixture, _state, _trainer
from x3dhip import _steplib, stepops

pytestmark = pytest.mark.gpu

MU, WD, ETA = 0.9, 5e-5, 0.001


class _Twin:
    """The host side of a run: the tables of the trainer's flat buffer, its scales and rates of trust, a state and a ring
    (the trust needs the record whether or not the update is guarded)."""

    def __init__(self, tr, max_norm=0.0):
        self.t = stepops.StepTables(stepops.segment_table([k for _, k in tr.fp.offsets]))
        self.hy = np.zeros(self.t.S, dtype=_steplib.HYPER_DT)
        self.hy["lr_scale"], self.hy["wd_scale"] = tr.hyper.lr_scale, tr.hyper.wd_scale
        self.eta = tr.lars.eta.copy()
        self.eps, self.clip = tr.lars.eps, tr.lars.clip
        self.state = stepops.new_state()
        self.R = 4
        self.ws = stepops.aligned_bytes(self.t.workspace_bytes)
        self.tws = stepops.aligned_bytes(stepops.trust_workspace_bytes(self.t.nitems))
        self.ring = stepops.aligned_bytes(self.R * self.t.record_bytes)
        self.wsumsq = np.zeros(self.t.S, np.float64)
        self.trust = np.zeros(self.t.S, np.float32)
        self.max_norm = max_norm

    def update(self, w, g, m, first, guarded, nesterov):
        """g: the gradient as it stood right before the update.  What the Trainer enqueues: measure (guarded) or observe
        (a monitor without the guard: the record, then the gradient scaled in place), trust, apply_lars.  Returns the
        gradient as the update left it as well."""
        w, g, m = w.copy(), g.copy(), m.copy()
        if guarded:
            stepops.measure_host(g, self.t, self.ws, self.state, self.ring, self.R, self.max_norm, 1.0)
        else:
            stepops.observe_host(g, self.t, self.ws, self.state, self.ring, self.R, self.max_norm, 1.0)
        stepops.trust_host(w, self.t, self.hy, self.eta, self.state, self.ring, self.R, self.tws, self.wsumsq, self.trust, LR,
                           WD, 1.0, self.eps, self.clip)
        stepops.apply_lars_host(w, g, m, self.t, self.hy, self.trust, self.state if guarded else None,
                                self.ring if guarded else None, self.R, LR, MU, WD, 1.0, first, nesterov)
        return w, m, g


def _np(t):
    return t.detach().cpu().numpy().copy()


def _follow(tr, clips, y, guarded=False, max_norm=0.0):
    """Run the clips; before each update snapshot w, m and the gradient (pre_step runs right before it, after the
    all-reduce), and require wsumsq, trust, w, m and the gradient afterwards to be the twins' on those inputs.  Returns the
    per-update (w0, g, m0, w1, m1, trust)."""
    twin = _Twin(tr, max_norm)
    seen, snap = [], {}

    def pre_step():
        torch.cuda.synchronize()
        snap["w"], snap["m"], snap["first"] = _np(tr.fp.flat), _np(tr.fp.mom), tr.first
        snap["g"] = _np(tr.accum if tr.accum is not None else tr.fp.grad)

    for x in clips:
        tr.train_step(x, y, pre_step=pre_step)
        if not tr.stepped:
            continue
        torch.cuda.synchronize()
        g = snap["g"]
        w1, m1, g1 = twin.update(snap["w"], g, snap["m"], snap["first"], guarded, bool(tr.param_groups[0]["nesterov"]))
        g_now = (tr.accum if tr.accum is not None else tr.fp.grad).cpu()
        assert torch.equal(g_now.view(torch.int32), torch.from_numpy(g1).view(torch.int32))      # bits: a NaN clip has NaNs
        assert _np(tr.lars.wsumsq).tobytes() == twin.wsumsq.tobytes(), "update %d" % len(seen)
        assert torch.equal(tr.lars.trust.cpu(), torch.from_numpy(twin.trust)), "update %d" % len(seen)
        assert torch.equal(tr.fp.flat.cpu(), torch.from_numpy(w1)), "update %d" % len(seen)
        assert torch.equal(tr.fp.mom.cpu(), torch.from_numpy(m1)), "update %d" % len(seen)
        seen.append((snap["w"], g, snap["m"], w1, m1, twin.trust.copy()))
    return seen, twin


@pytest.mark.parametrize("kw", [dict(), dict(use_graph=True), dict(use_graph=True, force_split=True)],
                         ids=["eager", "graph", "split"])
def test_three_steps_are_the_twins_on_the_steps_own_inputs(golden_dir, kw):
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev)
    tr = _trainer(sd, S, dev, lars=ETA, **kw)
    assert tr.lars.summary() == (117, 199) and hasattr(tr, "monitor") and hasattr(tr, "hyper")
    assert tr.lars.tables is tr.monitor.tables is tr.hyper.tables
    seen, _ = _follow(tr, xs[:3], y)
    assert len(seen) == 3 and tr._overlap() == bool(kw.get("force_split"))
    assert not np.array_equal(seen[0][0], seen[2][3]) and np.all(np.isfinite(seen[2][3]))
    assert tr.monitor.state.cpu()[5:].tolist() == [0, 0, 0]


def test_graph_clipped_and_unguarded(golden_dir):
    """A monitor with clipping and no guard: `observe` records the gradient and scales it in place, trust multiplies the
    recorded norm by the coefficient, and apply_lars(state=None) takes the scaled gradient from there."""
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev)
    tr = _trainer(sd, S, dev, lars=dict(eta=ETA, clip=True), nesterov=True, use_graph=True, clip_grad_norm=0.5)
    seen, twin = _follow(tr, xs[:3], y, max_norm=0.5)
    assert len(seen) == 3 and twin.clip is True
    assert all(0.0 < c < 1.0 for c in tr.monitor.read()["coef"]) and tr.monitor.state.cpu()[5:].tolist() == [0, 0, 0]
    assert torch.equal(tr.monitor.state.cpu(), torch.from_numpy(twin.state))


@pytest.mark.parametrize("kw", [dict(), dict(use_graph=True)], ids=["eager", "graph"])
def test_clipped_and_guarded_a_nan_clip_is_skipped(golden_dir, kw):
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev)
    tr = _trainer(sd, S, dev, lars=ETA, clip_grad_norm=0.5, skip_nonfinite=True, **kw)
    seen, twin = _follow(tr, [xs[0], bad, xs[1]], y, guarded=True, max_norm=0.5)
    assert len(seen) == 3
    w0, g, m0, w1, m1, trust = seen[1]
    assert not np.all(np.isfinite(g)) and np.array_equal(w0, w1) and np.array_equal(m0, m1)
    assert torch.equal(tr.monitor.state.cpu(), torch.from_numpy(twin.state))
    assert tr.monitor.state.cpu()[5:].tolist() == [0, 1, 0] and int(tr.monitor.skipped()) == 1
    coef = tr.monitor.read()["coef"]
    assert 0.0 < coef[0] < 1.0 and 0.0 < coef[2] < 1.0 and np.all(np.isfinite(seen[2][3]))


def test_accumulation_updates_once_per_two_micro_batches(golden_dir):
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev, clips=6)
    tr = _trainer(sd, S, dev, lars=ETA, num_steps_per_update=2)
    seen, _ = _follow(tr, xs, y)
    assert len(seen) == 3


def test_one_rank_rccl_group(golden_dir, monkeypatch):
    import torch.distributed as dist
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev)
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", "29548")
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        tr = _trainer(sd, S, dev, lars=ETA, use_graph=True, process_group=dist.group.WORLD, world_size=1, force_split=True,
                      force_collectives=True)
        seen, _ = _follow(tr, xs[:3], y)
        assert len(seen) == 3 and tr.reducer.active and tr._overlap()
    finally:
        dist.destroy_process_group()


def test_three_steps_follow_a_torch_lars_in_fp64_and_read_shows_the_exempt_tensors(golden_dir):
    """A LARS in plain torch, fp64 (norms by torch.linalg.vector_norm, p.grad = trust * (g + wd * w), torch.optim.SGD with
    weight_decay = 0), fed the trainer's own per-step gradients, within lars_ref.TorchBound (tests/test_lars_host.py)."""
    import x3d
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev)
    tr = _trainer(sd, S, dev, lars=ETA, nesterov=True)
    seen, twin = _follow(tr, xs[:3], y)
    got = tr.lars.read()
    names = [k for k, _ in tr.model.named_parameters()]
    one_d = [k for k, p in tr.model.named_parameters() if p.dim() <= 1]
    assert len(one_d) == 199 and all(got["trust"][k] == 1.0 for k in one_d)
    assert all(got["trust"][k] != 1.0 and 0.0 < got["trust"][k] < 10.0 for k in names if k not in set(one_d))
    assert all(got["wnorm"][k] > 0.0 for k in names)
    net = x3d.generate_model("M", n_classes=400, dropout=0.0, base_bn_splits=S)
    net.load_state_dict(sd)
    net.double()
    params = [p for _, p in net.named_parameters()]
    opt = torch.optim.SGD(params, lr=LR, momentum=float(np.float32(MU)), weight_decay=0.0, nesterov=True)
    off = twin.t.seg_off
    lr_s, wd_s = group_ref.tensor_rule(LR, WD, twin.hy["lr_scale"], twin.hy["wd_scale"])
    lr_e, wd_e = group_ref.per_element(lr_s, off), group_ref.per_element(wd_s, off)
    flat64 = lambda: np.concatenate([p.detach().numpy().reshape(-1) for p in params])      # noqa: E731
    w64, m64 = flat64(), np.zeros(twin.t.n)
    bound = lars_ref.TorchBound(twin.t.n)
    for k, (w0, g, m0, w1, m1, trust) in enumerate(seen):
        rs = np.ones(len(params))
        for s, p in enumerate(params):
            gt = torch.from_numpy(g[int(off[s]):int(off[s + 1])].astype(np.float64)).view(p.shape)
            a, b = float(torch.linalg.vector_norm(p.detach())), float(torch.linalg.vector_norm(gt))
            if twin.eta[s] > 0 and a > 0 and b > 0:
                rs[s] = float(twin.eta[s]) * a / (b + float(wd_s[s]) * a + float(np.float32(twin.eps)))
            p.grad = rs[s] * (gt + float(wd_s[s]) * p.detach())
        r = group_ref.per_element(rs, off)
        bw, bm = bound.step(w64, g, m64, 1.0, lr_e, wd_e, r, bound.ratio_slack(w64, off), MU, 1.0, k == 0, True)
        opt.step()
        w64 = flat64()
        m64 = np.concatenate([opt.state[p]["momentum_buffer"].numpy().reshape(-1) for p in params])
        ew, em = np.abs(w1.astype(np.float64) - w64), np.abs(m1.astype(np.float64) - m64)
        print("step %d: max err w %.3g (bound %.3g at it), m %.3g (bound %.3g at it)"
              % (k, ew.max(), bw[ew.argmax()], em.max(), bm[em.argmax()]))
        assert np.all(ew <= bw) and np.all(em <= bm)
        ref = tr.lars.torch_reference(torch.from_numpy(w0), torch.from_numpy(g), LR, WD, 1.0).numpy()
        assert np.all(np.abs(trust - ref) <= 2.0 ** -22 * ref)


def test_the_weight_average_follows_the_lars_iterates(golden_dir):
    from tests.test_trainer_ema_gpu import DECAY, _average, _ema_stats, _iterate
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev)
    tr = _trainer(sd, S, dev, lars=ETA, ema_decay=DECAY)
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
    assert not torch.equal(tr.fp.flat, plain.fp.flat), "the LARS iterates are not the plain ones"


def test_checkpoint_round_trip(golden_dir):
    """Save at 2, resume in a new model and Trainer, and step 3 equals the uninterrupted run bit for bit."""
    import x3d
    from x3dhip.trainer import Trainer
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev)
    tr = _trainer(sd, S, dev, lars=dict(eta=0.002, eps=1e-6, clip=True, exempt=("fc2.weight",)))
    assert tr.lars.summary() == (116, 200)
    tr.lars.set("layer1.*conv*", 0.004)                  # something the constructor alone does not give
    for i in range(2):
        tr.train_step(xs[i], y)
    to_cpu = lambda d: {k: (to_cpu(v) if isinstance(v, dict) else v.cpu().clone() if isinstance(v, torch.Tensor) else v)  # noqa: E731
                        for k, v in d.items()}
    ck = dict(model=to_cpu(tr.model.state_dict()), opt=to_cpu(tr.state_dict()))
    assert sorted(ck["opt"]) == ["lars", "param_groups", "state", "tensor_hyper"]
    assert sorted(ck["opt"]["lars"]) == ["clip", "eps", "eta", "names"]
    tr.train_step(xs[2], y)
    net = x3d.generate_model("M", n_classes=400, dropout=0.0, base_bn_splits=S)
    net.load_state_dict(ck["model"])
    net.to(dev).train(True)
    again = Trainer(net, lr=LR, lars=0.5)
    again.load_state_dict(ck["opt"])
    assert np.array_equal(again.lars.eta, tr.lars.eta) and torch.equal(again.lars.d_eta, tr.lars.d_eta)
    assert again.lars.eps == 1e-6 and again.lars.clip is True
    again.train_step(xs[2], y)
    torch.cuda.synchronize()
    assert torch.equal(again.fp.flat, tr.fp.flat) and torch.equal(again.fp.mom, tr.fp.mom)
    other = dict(ck["opt"], lars=dict(ck["opt"]["lars"], names=ck["opt"]["lars"]["names"][::-1]))
    with pytest.raises(ValueError):
        again.load_state_dict(other)
    # a checkpoint without the key loads as before, and one with it into a Trainer without the feature
    again.load_state_dict({k: v for k, v in ck["opt"].items() if k != "lars"})
    plain = _trainer(sd, S, dev)
    plain.load_state_dict(ck["opt"])
    assert not hasattr(plain, "lars")
    with pytest.raises(ValueError):
        _trainer(sd, S, dev, lars=dict(exempt=("no.such.parameter*",)))
    with pytest.raises(ValueError):
        _trainer(sd, S, dev, lars=-0.001)
    with pytest.raises(ValueError):
        _trainer(sd, S, dev, lars=dict(eta=0.001, trust=1.0))
    with pytest.raises(ValueError):
        tr.lars.set("no.such.parameter*", 0.1)


def test_defaults_are_off_and_every_eta_zero_is_the_grouped_update(golden_dir, monkeypatch):
    dev = _dev()
    sd, S, xs, bad, y = _fixture(golden_dir, dev)
    calls = []
    real_t, real_a = stepops.trust, stepops.apply_lars
    monkeypatch.setattr(stepops, "trust", lambda *a, **k: (calls.append("t"), real_t(*a, **k))[1])
    monkeypatch.setattr(stepops, "apply_lars", lambda *a, **k: (calls.append("a"), real_a(*a, **k))[1])
    plain = _trainer(sd, S, dev)
    grouped = _trainer(sd, S, dev, tensor_hyper={}, nesterov=True)
    assert "lars" not in vars(plain) and not hasattr(grouped, "lars") and not hasattr(plain, "monitor")
    for i in range(2):
        plain.train_step(xs[i], y)
        grouped.train_step(xs[i], y)
    assert calls == []                                    # not one launch of the feature
    zero = _trainer(sd, S, dev, lars=0.0, nesterov=True)   # the feature on, every tensor exempt
    assert zero.lars.summary() == (0, 316)
    for i in range(2):
        zero.train_step(xs[i], y)
    assert calls == ["t", "a", "t", "a"]
    a, b = _state(grouped), _state(zero)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert bool((zero.lars.trust == 1.0).all())
    assert sorted(plain.state_dict()) == ["param_groups", "state"]
    assert sorted(grouped.state_dict()) == ["param_groups", "state", "tensor_hyper"]
    assert sorted(zero.state_dict()) == ["lars", "param_groups", "state", "tensor_hyper"]


# -- the scripts ------------------------------------------------------------------------------------------------------------
LINE = re.compile(r"^lars: 117 tensors adapted, 199 exempt, eta 0\.001, eps 1e-08, clip (on|off)$")
TRUST = re.compile(r" trust [\d.e+-]+/[\d.e+-]+/[\d.e+-]+")


def test_kinetics_script_flags(capsys, tmp_path):
    import train_x3d_kinetics_multigrid as tr
    _dev()
    out = {}
    for name, kw in (("on", dict(lars=0.001, lars_clip=True)), ("off", {})):
        torch.manual_seed(5)
        steps, _ = tr.run(init_lr=0.01, warmup_steps=2, max_epochs=1, batch_size=2, steps=0, max_steps_run=3,
                          iterations_per_epoch=9, save_every=3, save_model=str(tmp_path / (name + "_")), use_graph=False,
                          log_every=1, clip_size=32, **kw)
        assert steps == 3
        out[name] = (capsys.readouterr().out.splitlines(), torch.load(str(tmp_path / (name + "_000003.pt")), map_location="cpu"))
    on, ck_on = out["on"]
    off, ck_off = out["off"]
    hit = [ln for ln in on if LINE.match(ln)]
    assert len(hit) == 1 and LINE.match(hit[0]).group(1) == "on"
    steps_on = [ln for ln in on if ln.startswith(" step ")]
    assert on.index(hit[0]) < on.index(steps_on[0]) and len(steps_on) == 3 and all(TRUST.search(ln) for ln in steps_on)
    assert not any(ln.startswith("lars:") or " trust " in ln for ln in off)
    assert sorted(ck_off["optimizer_state_dict"]) == ["param_groups", "state"]
    assert sorted(ck_on["optimizer_state_dict"]) == ["lars", "param_groups", "state", "tensor_hyper"]
    la = ck_on["optimizer_state_dict"]["lars"]
    assert la["clip"] is True and la["eta"][la["names"].index("bn1.weight")] == 0.0
    assert abs(la["eta"][la["names"].index("conv1_s.weight")] - 0.001) < 1e-9


@pytest.mark.parametrize("task", ["class", "loc"])
def test_charades_scripts_flags(tmp_path, capsys, task):
    from tests import charades_ref as cr
    import train_x3d_charades
    import train_x3d_charades_loc
    _dev()
    mod = train_x3d_charades if task == "class" else train_x3d_charades_loc
    anno, _ = cr.load_fixture()
    torch.manual_seed(5)
    res = mod.run(init_lr=0.01, max_epochs=1, anno=anno, batch_size=4, save_model=str(tmp_path / "on_"), save_every=3,
                  use_graph=False, crop_size=64, c_size=64, dropout=0.5, seed=1, lars=0.001)
    on = capsys.readouterr().out.splitlines()
    assert res["steps"] == 6
    hit = [ln for ln in on if LINE.match(ln)]
    assert len(hit) == 1 and LINE.match(hit[0]).group(1) == "off"
    train = [ln for ln in on if " Epoch:" in ln and " train " in ln]
    assert train and all(TRUST.search(ln) for ln in train) and on.index(hit[0]) < on.index(train[0])
    ck = torch.load(res["checkpoints"][0], map_location="cpu")
    assert sorted(ck["optimizer_state_dict"]) == ["lars", "param_groups", "state", "tensor_hyper"]
    again = mod.run(init_lr=0.01, max_epochs=0, anno=anno, batch_size=4, save_model=str(tmp_path / "again_"), save_every=0,
                    use_graph=False, crop_size=64, c_size=64, seed=1, resume=res["checkpoints"][0], lars=0.5)
    capsys.readouterr()
    assert again["optimizer"].lars.summary() == (117, 199)          # restored from the checkpoint, not from the flag
    assert abs(float(again["optimizer"].lars.eta.max()) - 0.001) < 1e-9
