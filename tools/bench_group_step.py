"""Timing of the grouped update (csrc_step/group.hip: x3dstep_apply_groups; Trainer(tensor_hyper=, nesterov=)) by the
protocol of tools/bench_guarded_step.py: a warm-up, then the median of `--rounds` alternating windows with the slowest and
the fastest window.  One JSON line, also written to profiles/group_step/bench.json, and profiles/group_step/README.md from
the same figures.

    python tools/bench_group_step.py [--out DIR] [--rounds N] [--steps K] [--bench-py NAME=FILE ...]

  update   (a) on the X3D-M flat buffers (316 tensors, 3.79 M elements), between two device events, us per call, alternating:
           measure + apply against measure + apply_groups(state), and ops.sgd_fused against apply_groups(state=None), each
           pair first checked to the same bits at all-ones scales; then both grouped forms with the recipe's scales and
           Nesterov, and torch.optim.SGD(foreach=True, nesterov=True) with the recipe's parameter groups on the 316 views.
           Every call first copies the same gradient into the flat buffer (the protocol of the guarded step's figures); the
           copy alone is timed beside them.
  step     (b) the headline step (X3D-M, B 8, T 16, 224 x 224, use_graph) with the defaults, with the recipe
           (wd_exempt_1d, head_lr_scale 10, nesterov), and the same two with skip_nonfinite: four Trainers in one process,
           alternating window by window, ms per step
  --bench-py  (c) files holding the JSON line of `bench.py --gpus 1`, named parent_1=..., parent_2=..., branch_1=..., branch_2=...
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "x3d-multigrid_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from tools.bench_grad_monitor import B, H, T, _row, _stats, step_windows  # noqa: E402
from tools.bench_guarded_step import _event_windows  # noqa: E402

LR, MU, WD = 1e-4, 0.9, 5e-5
HEAD_LR_SCALE = 10.0
# The kernel's resource usage, from the compiler's remarks (-Rpass-analysis=kernel-resource-usage, gfx950) at a batch of
# four 16-byte groups of w, g and m per lane.
RESOURCES = dict(vgprs=84, sgprs=40, scratch_bytes_per_lane=0, lds_bytes=0, occupancy_waves_per_simd=5, batch_groups=4)
# Written down before the first measurement.
EXPECTATION = ("apply_groups moves the bytes of x3dstep_apply (w, g and m read, w and m written: 75.9 MB) on a wave-per-item "
               "grid of about 2100 items instead of a flat grid, so it should take the same time as x3dstep_apply, within a "
               "few microseconds.")


def update_windows(dev, rounds, calls=20):
    """(a)"""
    import torch
    import x3d
    from x3dhip import _steplib, hypergroups, ops, stepops
    from x3dhip.gradmonitor import GradMonitor
    from x3dhip.trainer import FlatParams
    torch.manual_seed(0)
    net = x3d.generate_model("M", n_classes=400).to(dev)
    fp = FlatParams(net)
    names = [k for k, _ in net.named_parameters()]
    g0 = torch.randn(fp.numel, device=dev) * 0.01
    w0 = fp.flat.clone()
    mon = GradMonitor(fp, names, ring=64)
    ones = hypergroups.HyperTable(fp, names, monitor=mon)
    rec = hypergroups.HyperTable(fp, names, monitor=mon)
    rec.apply(hypergroups.recipe(net, wd_exempt_1d=True, head_lr_scale=HEAD_LR_SCALE))
    t = mon.tables

    def measure_apply():
        fp.grad.copy_(g0)
        mon.measure()
        stepops.apply(fp.flat, fp.grad, fp.mom, t, mon.state, mon.ring, mon.R, LR, MU, WD, 1.0, first=False)

    def measure_groups(table=ones, nesterov=False):
        fp.grad.copy_(g0)
        mon.measure()
        stepops.apply_groups(fp.flat, fp.grad, fp.mom, t, table.hyper, mon.state, mon.ring, mon.R, LR, MU, WD, 1.0, False,
                             nesterov)

    def sgd_fused():
        fp.grad.copy_(g0)
        ops.sgd_fused(fp.flat, fp.grad, fp.mom, LR, MU, WD, 1.0, first=False)

    def groups_free(table=ones, nesterov=False):
        fp.grad.copy_(g0)
        stepops.apply_groups(fp.flat, fp.grad, fp.mom, t, table.hyper, None, None, 0, LR, MU, WD, 1.0, False, nesterov)

    # at all-ones scales and without Nesterov every path gives the same bits on the same inputs
    outs = []
    for fn in (measure_apply, measure_groups, sgd_fused, groups_free):
        fp.flat.copy_(w0)
        fp.mom.zero_()
        fn()
        fn()
        outs.append((fp.flat.clone(), fp.mom.clone()))
    assert all(torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1]) for o in outs[1:])

    # torch.optim.SGD with the recipe's groups on the 316 views of the same flat buffers
    opt = torch.optim.SGD(rec.torch_param_groups(net, LR, WD), lr=LR, momentum=MU, nesterov=True, foreach=True)
    fp.grad.copy_(g0)
    opt.step()                                           # creates the momentum buffers

    def torch_sgd():
        fp.grad.copy_(g0)
        opt.step()

    r = _event_windows({
        "refill_alone": lambda: fp.grad.copy_(g0),
        "measure_then_apply": measure_apply,
        "measure_then_apply_groups_ones": measure_groups,
        "sgd_fused": sgd_fused,
        "apply_groups_ones_no_state": groups_free,
        "measure_then_apply_groups_recipe_nesterov": lambda: measure_groups(rec, True),
        "apply_groups_recipe_nesterov_no_state": lambda: groups_free(rec, True),
        "torch_sgd_foreach_recipe_groups_nesterov": torch_sgd,
    }, rounds, calls)
    assert int(mon.skipped()) == 0 and bool(torch.isfinite(fp.flat).all())
    r["calls_per_window"], r["tensors"], r["elements"], r["items"] = calls, len(names), fp.numel, t.nitems
    r["torch_param_groups"] = len(opt.param_groups)
    r["recipe"] = dict(zip(("exempt_tensors", "exempt_elements", "scaled_tensors"), rec.summary()))
    a, b = r["measure_then_apply"], r["measure_then_apply_groups_ones"]
    r["groups_minus_apply_us"] = b["us_per_call"] - a["us_per_call"]
    r["apply_window_spread_us"] = a["us_per_call_max"] - a["us_per_call_min"]
    r["free_minus_sgd_fused_us"] = r["apply_groups_ones_no_state"]["us_per_call"] - r["sgd_fused"]["us_per_call"]
    r["sgd_fused_window_spread_us"] = r["sgd_fused"]["us_per_call_max"] - r["sgd_fused"]["us_per_call_min"]
    r["short_tensors"] = sum(1 for _, k in fp.offsets if k < _steplib.ITEM)
    r["expectation_holds"] = bool(r["groups_minus_apply_us"] <= r["apply_window_spread_us"])      # not slower than apply's spread
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_step"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30, help="steps per timed window of the headline step")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bench-py", nargs="*", default=[], metavar="NAME=FILE")
    ap.add_argument("--readme-from", default=None, metavar="BENCH_JSON",
                    help="no GPU: write README.md into --out from the figures of an earlier run")
    args = ap.parse_args()
    if args.readme_from:
        with open(args.readme_from) as f:
            res = json.loads(f.read())
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "README.md"), "w") as f:
            f.write(readme(res))
        return
    import torch
    import x3d
    from tools import stamp
    from x3dhip import hypergroups
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = {"metric": "group_step", "csrc_sha16": stamp.csrc_sha16(), "csrc_step_sha16": stamp.csrc_step_sha16(),
           "commit": stamp.commit(), "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "steps_per_window": args.steps, "shape": [B, T, H], "resources": RESOURCES, "expectation": EXPECTATION,
           "head_lr_scale": HEAD_LR_SCALE}
    res["update"] = update_windows(dev, args.rounds)
    spec = hypergroups.recipe(x3d.generate_model("M", n_classes=400), wd_exempt_1d=True, head_lr_scale=HEAD_LR_SCALE)
    on = dict(tensor_hyper=spec, nesterov=True)
    variants = [("off", {}), ("recipe", on), ("skip", dict(skip_nonfinite=True)), ("skip_recipe", dict(on, skip_nonfinite=True))]
    res["step"], trainers = step_windows(dev, variants, args.rounds, args.steps, args.warmup)
    st = res["step"]
    st["recipe"]["cost_us_by_medians"] = 1e3 * (st["recipe"]["ms_per_step"] - st["off"]["ms_per_step"])
    st["skip_recipe"]["cost_us_by_medians"] = 1e3 * (st["skip_recipe"]["ms_per_step"] - st["skip"]["ms_per_step"])
    st["skipped"] = {k: int(trainers[k].monitor.skipped()) for k in ("skip", "skip_recipe")}
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


def _verdict(up):
    d, spread = up["groups_minus_apply_us"], up["apply_window_spread_us"]
    if up["expectation_holds"]:
        return ("The expectation held: by the medians `measure + apply_groups` differs from `measure + apply` by %+.1f us, which "
                "is not more than the %.1f us between the fastest and the slowest window of `measure + apply` itself."
                % (d, spread))
    return ("The expectation did NOT hold: by the medians `measure + apply_groups` is %+.1f us against `measure + apply`, more "
            "than the %.1f us between the fastest and the slowest window of `measure + apply` itself.  What differs from "
            "`x3dstep_apply`: %d items make %d workgroups of four waves where the flat kernel has full workgroups throughout; "
            "%d of the %d tensors are shorter than one item, so their waves run with most lanes idle; every wave reads its "
            "item and its tensor's scales before its first load of w, g or m.  At %d VGPRs and no scratch (%d waves per SIMD) "
            "the registers do not limit it."
            % (d, spread, up["items"], (up["items"] + 3) // 4, up.get("short_tensors", 0), up["tensors"],
               RESOURCES["vgprs"], RESOURCES["occupancy_waves_per_simd"]))


def _bench_lines(bp, batch):
    if not bp:
        return ["`bench.py` on the parent commit and on this tree was not run: unmeasured.", ""]
    any_run = bp[sorted(bp)[0]]
    lines = ["`python bench.py --gpus 1 --steps %s --warmup %s` with the defaults on an export of the parent commit and on this "
             "tree, alternating, separate processes one after the other on one GPU (ms per step from the printed clips/s at "
             "batch %d; the JSON line's own `ms_per_step` has two decimals):" % (any_run.get("steps"), any_run.get("warmup"), batch),
             "", "| run | clips/s | ms per step |", "|---|---|---|"]
    for name in sorted(bp):
        v = bp[name]["value"]
        lines.append("| %s | %.2f | %.4f |" % (name, v, 1e3 * batch / v))
    par = [1e3 * batch / bp[k]["value"] for k in sorted(bp) if k.startswith("parent")]
    bra = [1e3 * batch / bp[k]["value"] for k in sorted(bp) if k.startswith("branch")]
    if len(par) > 1 and bra:
        slower = max(bra) - max(par)
        lines += ["", "The parent's own runs lie %.4f ms apart (%.4f .. %.4f); this tree's runs are %.4f .. %.4f: %s."
                  % (max(par) - min(par), min(par), max(par), min(bra), max(bra),
                     "none is slower than the parent's slowest" if slower <= 0 else
                     "the slowest is %.4f ms slower than the parent's slowest" % slower)]
    return lines + [""]


def readme(res):
    """profiles/group_step/README.md from the figures of one run."""
    up, st, rs = res["update"], res["step"], res["resources"]
    row = lambda k: _row(up[k], "us_per_call", "%.1f")      # noqa: E731
    lines = ["# Grouped update: apply_groups against apply and sgd_fused, torch's parameter groups, and the headline step", "",
             "Written by `tools/bench_group_step.py` on %s; `bench.json` beside this file holds every figure. A warm-up, then "
             "the median of %d alternating windows with the fastest and the slowest window in brackets. Sources: csrc_step %s, "
             "csrc %s." % (res["device"], res["rounds"], res["csrc_step_sha16"], res["csrc_sha16"]), "",
             "The kernel (`x3dstep_apply_groups_kernel`, gfx950, from the compiler's resource-usage remarks): %d VGPRs, %d SGPRs, "
             "scratch %d bytes per lane, LDS %d bytes, %d waves per SIMD, at a batch of %d 16-byte groups of w, g and m per "
             "lane." % (rs["vgprs"], rs["sgprs"], rs["scratch_bytes_per_lane"], rs["lds_bytes"],
                        rs["occupancy_waves_per_simd"], rs["batch_groups"]), "",
             "The expectation, written down before anything was measured: " + res["expectation"], "",
             "## (a) The update on the X3D-M flat buffers (%d tensors, %d elements, %d items), us per call" % (
                 up["tensors"], up["elements"], up["items"]), "",
             "Between two device events, %d calls per window, one process. Every call first copies the same gradient into the "
             "flat buffer; the copy alone is timed beside them. At all-ones scales and without Nesterov the four paths of the "
             "first two pairs were checked to leave the same bits in the parameters and the momentum. The recipe: %d tensors "
             "(%d elements) exempt from decay, %d tensors at %g times the rate; torch gets the same as %d parameter groups."
             % (up["calls_per_window"], up["recipe"]["exempt_tensors"], up["recipe"]["exempt_elements"],
                up["recipe"]["scaled_tensors"], res["head_lr_scale"], up["torch_param_groups"]), "",
             "| path (after the copy) | us per call |", "|---|---|",
             "| the copy alone | %s |" % row("refill_alone"),
             "| `measure` + `apply` (2 + 1 launches) | %s |" % row("measure_then_apply"),
             "| `measure` + `apply_groups(state)`, all-ones scales | %s |" % row("measure_then_apply_groups_ones"),
             "| `measure` + `apply_groups(state)`, the recipe, Nesterov | %s |" % row("measure_then_apply_groups_recipe_nesterov"),
             "| `ops.sgd_fused` (1 launch) | %s |" % row("sgd_fused"),
             "| `apply_groups(state=None)`, all-ones scales | %s |" % row("apply_groups_ones_no_state"),
             "| `apply_groups(state=None)`, the recipe, Nesterov | %s |" % row("apply_groups_recipe_nesterov_no_state"),
             "| `torch.optim.SGD(foreach=True, nesterov=True)`, the recipe's groups on the 316 views | %s |" % row(
                 "torch_sgd_foreach_recipe_groups_nesterov"), "",
             _verdict(up), "",
             "Without a state: `apply_groups(state=None)` against `ops.sgd_fused` %+.1f us by the medians (the windows of "
             "`ops.sgd_fused` spread over %.1f us)." % (up["free_minus_sgd_fused_us"], up["sgd_fused_window_spread_us"]), "",
             "## (b) The headline step (X3D-M, B %d, T %d, %d x %d, use_graph), ms per step" % (
                 res["shape"][0], res["shape"][1], res["shape"][2], res["shape"][2]), "",
             "Four Trainers in one process, %d steps and a synchronise per window, host clock. The recipe: "
             "`tensor_hyper=recipe(model, wd_exempt_1d=True, head_lr_scale=%g), nesterov=True`." % (
                 res["steps_per_window"], res["head_lr_scale"]), "",
             "| Trainer | ms per step | the recipe's cost by the medians |", "|---|---|---|",
             "| defaults | %s | |" % _row(st["off"], "ms_per_step", "%.3f"),
             "| the recipe | %s | %+.1f us |" % (_row(st["recipe"], "ms_per_step", "%.3f"), st["recipe"]["cost_us_by_medians"]),
             "| `skip_nonfinite=True` | %s | |" % _row(st["skip"], "ms_per_step", "%.3f"),
             "| `skip_nonfinite=True` and the recipe | %s | %+.1f us |" % (
                 _row(st["skip_recipe"], "ms_per_step", "%.3f"), st["skip_recipe"]["cost_us_by_medians"]), "",
             "No update was skipped in these windows (%s)." % json.dumps(st["skipped"], sort_keys=True), "",
             "## (c) The defaults against the parent commit", "",
             "The default path has no new launch: `ops.sgd_fused` and `x3dstep_apply` are called as before.", ""]
    lines += _bench_lines(res.get("bench_py"), res["shape"][0])
    lines += ["Nothing here is a share of any peak: these are achieved times of one process on one GPU.", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    main()
