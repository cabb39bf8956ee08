"""Timing of the trust ratios (csrc_step/lars.hip: x3dstep_trust, x3dstep_apply_lars; Trainer(lars=)) by the protocol of
tools/bench_group_step.py: a warm-up, then the median of `--rounds` alternating windows with the slowest and the fastest
window.  One JSON line, also written to profiles/lars/bench.json, and profiles/lars/README.md from the same figures.

    python tools/bench_lars.py [--out DIR] [--rounds N] [--steps K] [--bench-py NAME=FILE ...]

  update   (a) on the X3D-M flat buffers (316 tensors, 3.79 M elements), between two device events, us per call, alternating:
           measure + apply_groups(state) against measure + trust + apply_lars(state), first checked to the same bits with every
           eta 0; the two trust launches alone; and a LARS in torch: two torch._foreach_norm passes over the 316 weight and
           gradient views, the ratios and torch.optim.SGD(foreach=True).  Every call first copies the same gradient into the
           flat buffer; the copy alone is timed beside them.
  step     (b) the headline step (X3D-M, B 8, T 16, 224 x 224, use_graph) with the defaults, with the recipe (wd_exempt_1d,
           head_lr_scale 10, nesterov) and with the recipe and lars: three Trainers in one process, alternating window by
           window, ms per step
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

from tools.bench_grad_monitor import B, H, T, _row, step_windows  # noqa: E402
from tools.bench_group_step import HEAD_LR_SCALE, LR, MU, WD, _bench_lines  # noqa: E402
from tools.bench_guarded_step import _event_windows  # noqa: E402

ETA, EPS = 0.001, 1e-8
# The kernels' resource usage, from the compiler's remarks (-Rpass-analysis=kernel-resource-usage, gfx950).
RESOURCES = {
    "x3dstep_trust_partials_kernel": dict(vgprs=20, sgprs=24, scratch_bytes_per_lane=0, lds_bytes=0, occupancy_waves_per_simd=8),
    "x3dstep_trust_finalize_kernel": dict(vgprs=52, sgprs=52, scratch_bytes_per_lane=0, lds_bytes=20480,
                                          occupancy_waves_per_simd=8),
    "x3dstep_apply_lars_kernel": dict(vgprs=88, sgprs=40, scratch_bytes_per_lane=0, lds_bytes=0, occupancy_waves_per_simd=5),
}
# Written down before the first measurement.
EXPECTATION = ("The partials launch of x3dstep_trust reads the same 15.2 MB as launch 1 of x3dstep_measure and does less work per "
               "element (no hash, no count), so the two trust launches should take no longer than the two measure launches; "
               "x3dstep_apply_lars moves the bytes of x3dstep_apply_groups and adds one multiply per element, so it should cost "
               "what x3dstep_apply_groups costs.")


def update_windows(dev, rounds, calls=20):
    """(a)"""
    import torch
    import x3d
    from x3dhip import hypergroups, stepops
    from x3dhip.gradmonitor import GradMonitor
    from x3dhip.lars import TrustTable
    from x3dhip.trainer import FlatParams
    torch.manual_seed(0)
    net = x3d.generate_model("M", n_classes=400).to(dev)
    fp = FlatParams(net)
    named = list(net.named_parameters())
    names = [k for k, _ in named]
    g0 = torch.randn(fp.numel, device=dev) * 0.01
    w0 = fp.flat.clone()
    mon = GradMonitor(fp, names, ring=64)
    hy = hypergroups.HyperTable(fp, names, monitor=mon)
    hy.apply(hypergroups.recipe(net, wd_exempt_1d=True, head_lr_scale=HEAD_LR_SCALE))
    one_d = [i for i, (_, p) in enumerate(named) if p.dim() <= 1]
    off = TrustTable(fp, names, mon, hy, eta=0.0, eps=EPS)
    on = TrustTable(fp, names, mon, hy, eta=ETA, eps=EPS)
    on.eta[one_d] = 0.0
    on.upload()
    t = mon.tables

    def measure_groups():
        fp.grad.copy_(g0)
        mon.measure()
        stepops.apply_groups(fp.flat, fp.grad, fp.mom, t, hy.hyper, mon.state, mon.ring, mon.R, LR, MU, WD, 1.0, False, True)

    def measure_lars(table=on):
        fp.grad.copy_(g0)
        mon.measure()
        table.compute(fp.flat, LR, WD, 1.0)
        stepops.apply_lars(fp.flat, fp.grad, fp.mom, t, hy.hyper, table.trust, mon.state, mon.ring, mon.R, LR, MU, WD, 1.0, False,
                           True)

    def measure_alone():
        fp.grad.copy_(g0)
        mon.measure()

    def measure_trust():
        fp.grad.copy_(g0)
        mon.measure()
        on.compute(fp.flat, LR, WD, 1.0)

    # with every eta 0 the LARS path leaves the bits of the grouped update
    outs = []
    for fn in (measure_groups, lambda: measure_lars(off)):
        fp.flat.copy_(w0)
        fp.mom.zero_()
        fn()
        fn()
        outs.append((fp.flat.clone(), fp.mom.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])

    # a LARS in torch on the 316 views of the same flat buffers: two norm passes, the ratios, the scaled gradients, SGD
    params = [p for _, p in named]
    eta_t = on.d_eta.clone()
    wd_t = torch.from_numpy(hy.wd_scale).to(dev) * WD
    opt = torch.optim.SGD(hy.torch_param_groups(net, LR, 0.0), lr=LR, momentum=MU, nesterov=True, foreach=True)
    fp.grad.copy_(g0)
    opt.step()                                           # creates the momentum buffers

    def torch_lars():
        fp.grad.copy_(g0)
        with torch.no_grad():
            a = torch.stack(torch._foreach_norm(params))
            b = torch.stack(torch._foreach_norm([p.grad for p in params]))
            r = eta_t * a / (b + wd_t * a + EPS)
            r = torch.where((eta_t > 0) & (a > 0) & (b > 0), r, torch.ones_like(r))
            grads = [p.grad for p in params]
            torch._foreach_add_(grads, torch._foreach_mul(params, list(wd_t.unbind())))
            torch._foreach_mul_(grads, list(r.unbind()))
        opt.step()

    r = _event_windows({
        "refill_alone": lambda: fp.grad.copy_(g0),
        "measure_alone": measure_alone,
        "measure_then_trust": measure_trust,
        "measure_then_apply_groups": measure_groups,
        "measure_then_trust_then_apply_lars": measure_lars,
        "torch_lars_foreach": torch_lars,
    }, rounds, calls)
    assert int(mon.skipped()) == 0 and bool(torch.isfinite(fp.flat).all())
    r["calls_per_window"], r["tensors"], r["elements"], r["items"] = calls, len(names), fp.numel, t.nitems
    r["adapted"], r["exempt"] = on.summary()
    us = lambda k: r[k]["us_per_call"]                   # noqa: E731
    r["trust_launches_us"] = us("measure_then_trust") - us("measure_alone")
    r["measure_launches_us"] = us("measure_alone") - us("refill_alone")
    r["lars_minus_groups_us"] = us("measure_then_trust_then_apply_lars") - us("measure_then_apply_groups")
    r["apply_lars_minus_apply_groups_us"] = r["lars_minus_groups_us"] - r["trust_launches_us"]
    g = r["measure_then_apply_groups"]
    r["groups_window_spread_us"] = g["us_per_call_max"] - g["us_per_call_min"]
    r["expectation_holds"] = bool(r["trust_launches_us"] <= r["measure_launches_us"]
                                  and r["apply_lars_minus_apply_groups_us"] <= r["groups_window_spread_us"])
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lars"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30, help="steps per timed window of the headline step")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bench-py", nargs="*", default=[], metavar="NAME=FILE")
    ap.add_argument("--readme-from", default=None, metavar="BENCH_JSON",
                    help="no GPU: write README.md into --out from the figures of an earlier run (and --bench-py files)")
    args = ap.parse_args()
    if args.readme_from:
        with open(args.readme_from) as f:
            res = json.loads(f.read())
    else:
        import torch
        import x3d
        from tools import stamp
        from x3dhip import hypergroups
        dev = torch.device("cuda:0")
        torch.cuda.set_device(dev)
        res = {"metric": "lars", "csrc_sha16": stamp.csrc_sha16(), "csrc_step_sha16": stamp.csrc_step_sha16(),
               "commit": stamp.commit(), "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
               "steps_per_window": args.steps, "shape": [B, T, H], "resources": RESOURCES, "expectation": EXPECTATION,
               "head_lr_scale": HEAD_LR_SCALE, "eta": ETA, "eps": EPS, "bench_py": {}}
        res["update"] = update_windows(dev, args.rounds)
        spec = hypergroups.recipe(x3d.generate_model("M", n_classes=400), wd_exempt_1d=True, head_lr_scale=HEAD_LR_SCALE)
        on = dict(tensor_hyper=spec, nesterov=True)
        variants = [("off", {}), ("recipe", on), ("recipe_lars", dict(on, lars=ETA))]
        res["step"], _ = step_windows(dev, variants, args.rounds, args.steps, args.warmup)
        st = res["step"]
        st["recipe_lars"]["cost_us_by_medians"] = 1e3 * (st["recipe_lars"]["ms_per_step"] - st["recipe"]["ms_per_step"])
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


def readme(res):
    """profiles/lars/README.md from the figures of one run."""
    up, st = res["update"], res["step"]
    row = lambda k: _row(up[k], "us_per_call", "%.1f")      # noqa: E731
    lines = ["# LARS trust ratios: trust + apply_lars against apply_groups, a LARS in torch, and the headline step", "",
             "Written by `tools/bench_lars.py` on %s; `bench.json` beside this file holds every figure. A warm-up, then the "
             "median of %d alternating windows with the fastest and the slowest window in brackets. Sources: csrc_step %s, "
             "csrc %s." % (res["device"], res["rounds"], res["csrc_step_sha16"], res["csrc_sha16"]), "",
             "The kernels (gfx950, from the compiler's resource-usage remarks):", "",
             "| kernel | VGPRs | SGPRs | scratch bytes per lane | LDS bytes | waves per SIMD |", "|---|---|---|---|---|---|"]
    for name in sorted(res["resources"]):
        rs = res["resources"][name]
        lines.append("| `%s` | %d | %d | %d | %d | %d |" % (name, rs["vgprs"], rs["sgprs"], rs["scratch_bytes_per_lane"],
                                                         rs["lds_bytes"], rs["occupancy_waves_per_simd"]))
    lines += ["", "The kernels that were there before keep their numbers: compiled from this tree, every kernel of step.hip, "
              "ema.hip, pbn.hip and group.hip reports the registers, scratch, LDS and occupancy it reported on the parent "
              "commit (`x3dstep_apply_groups_kernel`: 84 VGPRs, 40 SGPRs, no scratch, 5 waves per SIMD, as "
              "profiles/step_walks/ records), and the device code of the four files is the same instruction for instruction "
              "(`kernel_resources.txt` beside this file lists both).", "",
              "The expectation, written down before anything was measured: " + res["expectation"], "",
              "## (a) The update on the X3D-M flat buffers (%d tensors, %d elements, %d items), us per call" % (
                  up["tensors"], up["elements"], up["items"]), "",
              "Between two device events, %d calls per window, one process. Every call first copies the same gradient into the "
              "flat buffer; the copy alone is timed beside them. The scales are the recipe's (no decay on the %d tensors with "
              "ndim <= 1, fc2.* at %g times the rate), Nesterov on; eta %g on %d tensors and 0 on the others, eps %g. With "
              "every eta 0 the LARS path was first checked to leave the bits of the grouped update."
              % (up["calls_per_window"], up["exempt"], res["head_lr_scale"], res["eta"], up["adapted"], res["eps"]), "",
              "| path (after the copy) | us per call |", "|---|---|",
              "| the copy alone | %s |" % row("refill_alone"),
              "| `measure` (2 launches) | %s |" % row("measure_alone"),
              "| `measure` + `trust` (2 + 2 launches) | %s |" % row("measure_then_trust"),
              "| `measure` + `apply_groups(state)` | %s |" % row("measure_then_apply_groups"),
              "| `measure` + `trust` + `apply_lars(state)` | %s |" % row("measure_then_trust_then_apply_lars"),
              "| torch: two `_foreach_norm` passes, the ratios, `torch.optim.SGD(foreach=True, nesterov=True)` on the 316 "
              "views | %s |" % row("torch_lars_foreach"), "",
              "By the medians: the two trust launches cost %+.1f us (the two measure launches: %+.1f us); the whole LARS update "
              "costs %+.1f us more than the grouped update, of which %+.1f us are `apply_lars` against `apply_groups` (the "
              "windows of `measure` + `apply_groups` spread over %.1f us). The expectation about the trust launches %s; the one "
              "about `apply_lars` %s%s."
              % (up["trust_launches_us"], up["measure_launches_us"], up["lars_minus_groups_us"],
                 up["apply_lars_minus_apply_groups_us"], up["groups_window_spread_us"],
                 "held" if up["trust_launches_us"] <= up["measure_launches_us"] else "did NOT hold",
                 "held" if up["apply_lars_minus_apply_groups_us"] <= up["groups_window_spread_us"] else "did NOT hold",
                 "" if up["apply_lars_minus_apply_groups_us"] <= up["groups_window_spread_us"] else
                 ": it is slower by more than that spread (every wave reads its tensor's trust after its scales, before its first "
                 "load of w, g and m, and the kernel holds %d VGPRs against 84)" % res["resources"]["x3dstep_apply_lars_kernel"]["vgprs"]),
              "",
              "## (b) The headline step (X3D-M, B %d, T %d, %d x %d, use_graph), ms per step" % (
                  res["shape"][0], res["shape"][1], res["shape"][2], res["shape"][2]), "",
              "Three Trainers in one process, %d steps and a synchronise per window, host clock. The recipe: "
              "`tensor_hyper=recipe(model, wd_exempt_1d=True, head_lr_scale=%g), nesterov=True`; LARS: `lars=%g` on top of it "
              "(which brings the monitor's two launches with it)." % (res["steps_per_window"], res["head_lr_scale"], res["eta"]),
              "", "| Trainer | ms per step | the cost of lars by the medians |", "|---|---|---|",
              "| defaults | %s | |" % _row(st["off"], "ms_per_step", "%.3f"),
              "| the recipe | %s | |" % _row(st["recipe"], "ms_per_step", "%.3f"),
              "| the recipe and `lars` | %s | %+.1f us |" % (_row(st["recipe_lars"], "ms_per_step", "%.3f"),
                                                           st["recipe_lars"]["cost_us_by_medians"]), "",
              "## (c) The defaults against the parent commit", "",
              "The default path has no new launch: `ops.sgd_fused`, `x3dstep_apply` and `x3dstep_apply_groups` are called as "
              "before.", ""]
    lines += _bench_lines(res.get("bench_py"), res["shape"][0])
    lines += ["Nothing here is a share of any peak: these are achieved times of one process on one GPU.", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    main()
