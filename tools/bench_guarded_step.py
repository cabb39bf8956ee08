"""Timing of the guarded update (csrc_step/step.hip: x3dstep_measure, x3dstep_apply, x3dstep_keep; Trainer(skip_nonfinite=))
by the protocol of tools/bench_grad_monitor.py: a warm-up, then the median of `--rounds` alternating windows with the
slowest and the fastest window.  One JSON line, also written to profiles/guarded_step/bench.json, and
profiles/guarded_step/README.md from the same figures.

    python tools/bench_guarded_step.py [--out DIR] [--rounds N] [--steps K] [--bench-py NAME=FILE ...]

  update   (a) on the X3D-M flat buffers (316 tensors, 3.79 M elements), between two device events, us per call, alternating:
           the parent's path, observe(max_norm) + ops.sgd_fused (three launches and one), against measure + apply (two
           launches and one).  Every call of either path first copies the same gradient (norm 19.5, max_norm 1) into the flat
           buffer, since observe scales it in place; the copy alone is timed beside them.
  keep     (b) x3dstep_keep alone on the 168 running-statistics buffers of X3D-M: save, restore after a skip (copies back),
           restore after an applied update (every workgroup leaves)
  step     (c) the headline step (X3D-M, B 8, T 16, 224 x 224, use_graph) with skip_nonfinite off, on, and on with clipping,
           and for comparison the parent's clipped path (monitor + clip_grad_norm): four Trainers in one process,
           alternating window by window, ms per step
  --bench-py  files holding the JSON line of `bench.py --gpus 1`, named parent_1=..., parent_2=..., branch_1=..., branch_2=...
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "x3d-multigrid_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from tools.bench_grad_monitor import B, H, MAX_NORM, STEP_MAX_NORM, T, _holds, _row, _stats, step_windows  # noqa: E402

LR, MU, WD = 1e-4, 0.9, 5e-5


def _event_windows(versions, rounds, calls):
    import torch
    for fn in versions.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in versions}
    for _ in range(rounds):
        for k, fn in versions.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1e3 / calls)
    return {k: _stats(v, "us_per_call") for k, v in us.items()}


def update_windows(dev, rounds, calls=20):
    """(a) and (b)."""
    import torch
    import x3d
    from x3dhip import _steplib, ops, stepops
    from x3dhip.gradmonitor import GradMonitor
    from x3dhip.trainer import FlatParams
    torch.manual_seed(0)
    net = x3d.generate_model("M", n_classes=400).to(dev)
    fp = FlatParams(net)
    names = [k for k, _ in net.named_parameters()]
    g0 = torch.randn(fp.numel, device=dev) * 0.01
    w0 = fp.flat.clone()
    parent, guard = GradMonitor(fp, names, ring=64, max_norm=MAX_NORM), GradMonitor(fp, names, ring=64, max_norm=MAX_NORM)

    def parent_path():
        fp.grad.copy_(g0)
        parent.observe()
        ops.sgd_fused(fp.flat, fp.grad, fp.mom, LR, MU, WD, 1.0, first=False)

    def guarded_path():
        fp.grad.copy_(g0)
        guard.measure()
        stepops.apply(fp.flat, fp.grad, fp.mom, guard.tables, guard.state, guard.ring, guard.R, LR, MU, WD, 1.0, first=False)

    # the two paths give the same bits on the same inputs
    outs = []
    for fn in (parent_path, guarded_path):
        fp.flat.copy_(w0)
        fp.mom.zero_()
        fn()
        fn()
        outs.append((fp.flat.clone(), fp.mom.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert float(guard.last_coef()) == float(parent.last_coef()) < 1.0

    r = _event_windows({"refill_alone": lambda: fp.grad.copy_(g0), "observe_clip_then_sgd_fused": parent_path,
                        "measure_then_apply": guarded_path}, rounds, calls)
    assert int(guard.skipped()) == 0
    r["calls_per_window"], r["tensors"], r["elements"] = calls, len(names), fp.numel
    r["bar_fused_median_not_slower"] = (r["measure_then_apply"]["us_per_call"]
                                        <= r["observe_clip_then_sgd_fused"]["us_per_call"])

    bufs = []
    for mod in net.modules():
        sb = getattr(mod, "split_bn", None)
        if sb is not None:
            bufs += [sb.running_mean, sb.running_var]
    kt = stepops.KeepTable(bufs, dev)
    skip1, skip0 = guard.state.clone(), guard.state.clone()
    skip1[_steplib.S_SKIP], skip0[_steplib.S_SKIP] = 1, 0
    k = _event_windows({"save": lambda: stepops.keep(kt, skip0, _steplib.KEEP_SAVE),
                        "restore_after_a_skip": lambda: stepops.keep(kt, skip1, _steplib.KEEP_RESTORE),
                        "restore_after_an_applied_update": lambda: stepops.keep(kt, skip0, _steplib.KEEP_RESTORE)},
                       rounds, calls)
    k["buffers"], k["elements"], k["items"] = kt.nbuf, int(sum(b.numel() for b in bufs)), kt.nitems
    return r, k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guarded_step"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30, help="steps per timed window of the headline step")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bench-py", nargs="*", default=[], metavar="NAME=FILE")
    args = ap.parse_args()
    import torch
    from tools import stamp
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = {"metric": "guarded_step", "csrc_sha16": stamp.csrc_sha16(), "csrc_step_sha16": stamp.csrc_step_sha16(),
           "commit": stamp.commit(), "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "steps_per_window": args.steps, "shape": [B, T, H], "max_norm": MAX_NORM}
    res["update"], res["keep"] = update_windows(dev, args.rounds)
    variants = [("off", {}), ("skip", dict(skip_nonfinite=True)),
                ("skip_clip", dict(skip_nonfinite=True, clip_grad_norm=STEP_MAX_NORM)),
                ("monitor_clip", dict(monitor=True, clip_grad_norm=STEP_MAX_NORM))]
    res["step"], trainers = step_windows(dev, variants, args.rounds, args.steps, args.warmup)
    off = res["step"]["off"]
    for k in ("skip", "skip_clip", "monitor_clip"):
        res["step"][k]["cost_us_by_medians"] = 1e3 * (res["step"][k]["ms_per_step"] - off["ms_per_step"])
    res["step"]["skipped"] = {k: int(trainers[k].monitor.skipped()) for k in ("skip", "skip_clip")}
    res["step"]["last_coef_skip_clip"] = float(trainers["skip_clip"].monitor.last_coef())
    res["bench_py"] = {}
    for item in args.bench_py:
        name, path = item.split("=", 1)
        with open(path) as f:
            lines = [ln for ln in f.read().splitlines() if ln.startswith("{")]
        res["bench_py"][name] = json.loads(lines[-1])
    out = json.dumps(res, sort_keys=True)
    print(out)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench.json"), "w") as f:
        f.write(out + "\n")
    with open(os.path.join(args.out, "README.md"), "w") as f:
        f.write(readme(res))


def _bench_py_lines(bp):
    if not bp:
        return ["`bench.py` on the parent commit and on this tree was not run: unmeasured.", ""]
    any_run = bp[sorted(bp)[0]]
    lines = ["`python bench.py --gpus 1 --steps %s --warmup %s` with the defaults (guard off) on an export of the parent commit "
             "and on this tree, alternating, separate processes one after the other on one GPU:" % (
                 any_run.get("steps"), any_run.get("warmup")), "",
             "| run | ms per step |", "|---|---|"]
    for name in sorted(bp):
        r = bp[name]
        ms = r.get("ms_per_step", r.get("step_ms", r.get("value")))
        lines.append("| %s | %s |" % (name, "%.3f" % ms if isinstance(ms, (int, float)) else json.dumps(r, sort_keys=True)))
    return lines + [""]


def readme(res):
    """profiles/guarded_step/README.md from the figures of one run."""
    up, kp, st = res["update"], res["keep"], res["step"]
    a, b = up["observe_clip_then_sgd_fused"], up["measure_then_apply"]
    lines = ["# Guarded update: measure + apply against observe + sgd_fused, the keep launch, and the headline step", "",
             "Written by `tools/bench_guarded_step.py` on %s; `bench.json` beside this file holds every figure. A warm-up, then "
             "the median of %d alternating windows with the fastest and the slowest window in brackets. Sources: csrc_step %s, "
             "csrc %s." % (res["device"], res["rounds"], res["csrc_step_sha16"], res["csrc_sha16"]), "",
             "## (a) The update on the X3D-M flat buffers (%d tensors, %d elements), us per call" % (up["tensors"], up["elements"]),
             "", "Between two device events, %d calls per window, one process. `observe` scales the gradient in place, so every "
             "call of either path first copies the same gradient (norm 19.5) into the flat buffer; max_norm %g, so every call "
             "clips. The two paths were checked to leave the same bits in the parameters and the momentum." % (
                 up["calls_per_window"], res["max_norm"]), "",
             "| path (after the copy) | us per call |", "|---|---|",
             "| the copy alone | %s |" % _row(up["refill_alone"], "us_per_call", "%.1f"),
             "| parent: `observe(max_norm)` + `ops.sgd_fused` (3 + 1 launches) | %s |" % _row(a, "us_per_call", "%.1f"),
             "| `measure` + `apply` (2 + 1 launches) | %s |" % _row(b, "us_per_call", "%.1f"), "",
             "The expectation written before anything was measured: the fused path is no slower, since it saves one launch and "
             "one read and write of the gradient. By the medians: %s (%+.1f us, %+.1f %%)." % (
                 _holds(up["bar_fused_median_not_slower"]), b["us_per_call"] - a["us_per_call"],
                 100 * (b["us_per_call"] / a["us_per_call"] - 1)), "",
             "## (b) `keep` alone on the running statistics of X3D-M (%d buffers, %d elements, %d items), us per call" % (
                 kp["buffers"], kp["elements"], kp["items"]), "",
             "| launch | us per call |", "|---|---|",
             "| save | %s |" % _row(kp["save"], "us_per_call", "%.1f"),
             "| restore after a skipped update (copies back) | %s |" % _row(kp["restore_after_a_skip"], "us_per_call", "%.1f"),
             "| restore after an applied update (every workgroup leaves) | %s |" % _row(
                 kp["restore_after_an_applied_update"], "us_per_call", "%.1f"), "",
             "## (c) The headline step (X3D-M, B %d, T %d, %d x %d, use_graph), ms per step" % (
                 res["shape"][0], res["shape"][1], res["shape"][2], res["shape"][2]), "",
             "Four Trainers in one process, %d steps and a synchronise per window, host clock." % res["steps_per_window"], "",
             "| Trainer | ms per step | cost by the medians |", "|---|---|---|",
             "| defaults (guard off) | %s | |" % _row(st["off"], "ms_per_step", "%.3f"),
             "| `skip_nonfinite=True` | %s | %+.1f us |" % (_row(st["skip"], "ms_per_step", "%.3f"), st["skip"]["cost_us_by_medians"]),
             "| `skip_nonfinite=True, clip_grad_norm=%g` | %s | %+.1f us |" % (
                 STEP_MAX_NORM, _row(st["skip_clip"], "ms_per_step", "%.3f"), st["skip_clip"]["cost_us_by_medians"]),
             "| for comparison: `monitor=True, clip_grad_norm=%g` (the parent's clipped path) | %s | %+.1f us |" % (
                 STEP_MAX_NORM, _row(st["monitor_clip"], "ms_per_step", "%.3f"), st["monitor_clip"]["cost_us_by_medians"]),
             "", "The guard is a price, not a regression: it adds the two measuring launches and the two keep launches to a "
             "step that had none. No update was skipped in these windows (%s); the coefficient of the last clipped step was "
             "%.3g." % (json.dumps(st["skipped"], sort_keys=True), st["last_coef_skip_clip"]), "",
             "## The defaults against the parent commit", ""]
    lines += _bench_py_lines(res.get("bench_py"))
    lines += ["Nothing here is a share of any peak: these are achieved times of one process on one GPU.", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    main()
