"""Timing of the second-moment updates (csrc_step/adam.hip: x3dstep_adam, x3dstep_lamb_*; Trainer(optimizer=)) by the
protocol of tools/bench_lars.py: a warm-up, then the median of `--rounds` alternating windows with the slowest and the
fastest window, all in one process.  One JSON line, also written to profiles/adam/bench.json, and profiles/adam/README.md
from the same figures.

    python tools/bench_adam.py [--out DIR] [--rounds N] [--steps K] [--bench-py NAME=FILE ...]

  update   (a) on the X3D-M flat buffers (316 tensors, 3.79 M elements), between two device events, us per call, alternating:
           x3dstep_apply_groups against x3dstep_adam (AdamW, no state), torch.optim.AdamW(fused=True) and (foreach=True) on the
           316 views with the parameter groups hyper.torch_param_groups gives; the three LAMB launches against measure +
           trust + apply_lars.  Every call first copies the same gradient into the flat buffer; the copy alone is timed
           beside them.  The one bar: the slowest window of x3dstep_adam is faster than the fastest of torch's fused AdamW.
  step     (b) the headline step (X3D-M, B 8, T 16, 224 x 224, use_graph) with the defaults, with adamw and with lamb: three
           Trainers in one process, alternating window by window, ms per step
  --bench-py  (c) files holding the JSON line of `bench.py --gpus 1`, named parent_1=..., parent_2=..., branch_1=..., branch_2=...
  --ratios    the lines tests/test_adam_host.py prints (restatement against torch in fp64), copied into the README
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

BETAS, EPS, ETA = (0.9, 0.999), 1e-8, 0.001
# The kernels' resource usage, from the compiler's remarks (-Rpass-analysis=kernel-resource-usage, gfx950;
# profiles/adam/kernel_resources.txt).
RESOURCES = {
    "x3dstep_adam_kernel": dict(vgprs=116, sgprs=42, scratch_bytes_per_lane=0, lds_bytes=0, occupancy_waves_per_simd=4),
    "x3dstep_lamb_moments_kernel": dict(vgprs=82, sgprs=44, scratch_bytes_per_lane=0, lds_bytes=0, occupancy_waves_per_simd=5),
    "x3dstep_lamb_trust_kernel": dict(vgprs=50, sgprs=54, scratch_bytes_per_lane=0, lds_bytes=40960, occupancy_waves_per_simd=8),
    "x3dstep_lamb_apply_kernel": dict(vgprs=80, sgprs=44, scratch_bytes_per_lane=0, lds_bytes=0, occupancy_waves_per_simd=6),
}
# Written down before the first measurement.
EXPECTATION = ("From bytes alone: x3dstep_adam moves 7 streams of the 15 MB buffer (w, g, m, v in; w, m, v out) where "
               "x3dstep_apply_groups moves 5, so about 7/5 of the 20.8 us that profiles/group_step/ records for the latter.")


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
    mon = GradMonitor(fp, names, ring=64)
    hy = hypergroups.HyperTable(fp, names, monitor=mon)
    hy.apply(hypergroups.recipe(net, wd_exempt_1d=True, head_lr_scale=HEAD_LR_SCALE))
    one_d = [i for i, (_, p) in enumerate(named) if p.dim() <= 1]
    lars = TrustTable(fp, names, mon, hy, eta=ETA, eps=EPS)
    lars.eta[one_d] = 0.0
    lars.upload()
    t = mon.tables
    v = torch.zeros_like(fp.flat)
    adapt = torch.ones(len(names), dtype=torch.uint8, device=dev)
    adapt[one_d] = 0
    lws = torch.zeros(stepops.lamb_workspace_bytes(t.nitems), dtype=torch.uint8, device=dev)
    wss, rss = (torch.zeros(len(names), dtype=torch.float64, device=dev) for _ in range(2))
    trust = torch.ones(len(names), dtype=torch.float32, device=dev)

    def groups():
        fp.grad.copy_(g0)
        stepops.apply_groups(fp.flat, fp.grad, fp.mom, t, hy.hyper, None, None, 0, LR, MU, WD, 1.0, False, False)

    def adam():
        fp.grad.copy_(g0)
        stepops.adam(fp.flat, fp.grad, fp.mom, v, t, hy.hyper, None, None, 0, 5, LR, BETAS, EPS, WD, 1.0, True)

    def lamb():
        fp.grad.copy_(g0)
        stepops.lamb_moments(fp.flat, fp.grad, fp.mom, v, t, hy.hyper, None, None, 0, 5, lws, BETAS, EPS, WD, 1.0)
        stepops.lamb_trust(t, hy.hyper, adapt, None, None, 0, 5, lws, wss, rss, trust)
        stepops.lamb_apply(fp.flat, fp.mom, v, t, hy.hyper, trust, None, None, 0, 5, LR, BETAS, EPS, WD)

    def measure_lamb():
        fp.grad.copy_(g0)
        mon.measure()
        st = (mon.state, mon.ring, mon.R)
        stepops.lamb_moments(fp.flat, fp.grad, fp.mom, v, t, hy.hyper, *st, 0, lws, BETAS, EPS, WD, 1.0)
        stepops.lamb_trust(t, hy.hyper, adapt, *st, 0, lws, wss, rss, trust)
        stepops.lamb_apply(fp.flat, fp.mom, v, t, hy.hyper, trust, *st, 0, LR, BETAS, EPS, WD)

    def measure_lars():
        fp.grad.copy_(g0)
        mon.measure()
        lars.compute(fp.flat, LR, WD, 1.0)
        stepops.apply_lars(fp.flat, fp.grad, fp.mom, t, hy.hyper, lars.trust, mon.state, mon.ring, mon.R, LR, MU, WD, 1.0, False,
                           False)

    fns = {"refill_alone": lambda: fp.grad.copy_(g0), "apply_groups": groups, "adam": adam, "lamb_three_launches": lamb,
           "measure_then_lamb": measure_lamb, "measure_then_trust_then_apply_lars": measure_lars}
    errors = {}
    for key, kw in (("torch_adamw_fused", dict(fused=True)), ("torch_adamw_foreach", dict(foreach=True))):
        try:
            opt = torch.optim.AdamW(hy.torch_param_groups(net, LR, WD), lr=LR, betas=BETAS, eps=EPS, **kw)
            fp.grad.copy_(g0)
            opt.step()                                       # creates the state

            def torch_step(opt=opt):
                fp.grad.copy_(g0)
                opt.step()

            fns[key] = torch_step
        except Exception as e:                               # recorded: the bar then has nothing to be held against
            errors[key] = repr(e)
    r = _event_windows(fns, rounds, calls)
    assert bool(torch.isfinite(fp.flat).all()) and bool(torch.isfinite(v).all())
    r["errors"] = errors
    r["calls_per_window"], r["tensors"], r["elements"], r["items"] = calls, len(names), fp.numel, t.nitems
    us = lambda k: r[k]["us_per_call"]                       # noqa: E731
    r["adam_launch_us"] = us("adam") - us("refill_alone")
    r["apply_groups_launch_us"] = us("apply_groups") - us("refill_alone")
    r["adam_over_apply_groups"] = r["adam_launch_us"] / r["apply_groups_launch_us"]
    r["expectation_holds"] = bool(r["adam_over_apply_groups"] <= 7.0 / 5.0 * 1.1)
    r["lamb_launches_us"] = us("lamb_three_launches") - us("refill_alone")
    r["lamb_minus_lars_us"] = us("measure_then_lamb") - us("measure_then_trust_then_apply_lars")
    if "torch_adamw_fused" in r:
        r["bar_holds"] = bool(r["adam"]["us_per_call_max"] < r["torch_adamw_fused"]["us_per_call_min"])
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30, help="steps per timed window of the headline step")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bench-py", nargs="*", default=[], metavar="NAME=FILE")
    ap.add_argument("--ratios", default=None, metavar="FILE", help="the output of tests/test_adam_host.py -s -k follows")
    ap.add_argument("--readme-from", default=None, metavar="BENCH_JSON",
                    help="no GPU: write README.md into --out from the figures of an earlier run (and --bench-py files)")
    args = ap.parse_args()
    if args.readme_from:
        with open(args.readme_from) as f:
            res = json.loads(f.read())
    else:
        import torch
        from tools import stamp
        dev = torch.device("cuda:0")
        torch.cuda.set_device(dev)
        res = {"metric": "adam", "csrc_sha16": stamp.csrc_sha16(), "csrc_step_sha16": stamp.csrc_step_sha16(),
               "commit": stamp.commit(), "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
               "steps_per_window": args.steps, "shape": [B, T, H], "resources": RESOURCES, "expectation": EXPECTATION,
               "head_lr_scale": HEAD_LR_SCALE, "betas": list(BETAS), "eps": EPS, "bench_py": {}, "ratios": []}
        res["update"] = update_windows(dev, args.rounds)
        variants = [("off", {}), ("adamw", dict(optimizer="adamw", weight_decay=WD)), ("lamb", dict(optimizer="lamb", weight_decay=WD))]
        res["step"], _ = step_windows(dev, variants, args.rounds, args.steps, args.warmup)
        st = res["step"]
        for k in ("adamw", "lamb"):
            st[k]["cost_us_by_medians"] = 1e3 * (st[k]["ms_per_step"] - st["off"]["ms_per_step"])
    for item in args.bench_py:
        name, path = item.split("=", 1)
        with open(path) as f:
            lines = [ln for ln in f.read().splitlines() if ln.startswith("{")]
        res["bench_py"][name] = json.loads(lines[-1])
    if args.ratios:
        with open(args.ratios) as f:
            res["ratios"] = [ln.strip().lstrip(".") for ln in f.read().splitlines() if ": ratio " in ln or "of the powers" in ln]
    out = json.dumps(res, sort_keys=True)
    print(out)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench.json"), "w") as f:
        f.write(out + "\n")
    with open(os.path.join(args.out, "README.md"), "w") as f:
        f.write(readme(res))
    if res["update"].get("bar_holds") is False:
        sys.exit("the timing bar does not hold: x3dstep_adam's slowest window is not faster than torch's fused AdamW's fastest")


def readme(res):
    """profiles/adam/README.md from the figures of one run."""
    up, st = res["update"], res["step"]
    row = lambda k: _row(up[k], "us_per_call", "%.1f") if k in up else "not run: %s" % up["errors"].get(k)      # noqa: E731
    lines = ["# AdamW and LAMB: x3dstep_adam against apply_groups and torch's AdamW, LAMB against LARS, and the headline step", "",
             "Written by `tools/bench_adam.py` on %s; `bench.json` beside this file holds every figure. A warm-up, then the "
             "median of %d alternating windows with the fastest and the slowest window in brackets. Sources: csrc_step %s, "
             "csrc %s." % (res["device"], res["rounds"], res["csrc_step_sha16"], res["csrc_sha16"]), "",
             "The kernels (gfx950, from the compiler's resource-usage remarks, `kernel_resources.txt` beside this file):", "",
             "| kernel | VGPRs | SGPRs | scratch bytes per lane | LDS bytes | waves per SIMD |", "|---|---|---|---|---|---|"]
    for name in sorted(res["resources"]):
        rs = res["resources"][name]
        lines.append("| `%s` | %d | %d | %d | %d | %d |" % (name, rs["vgprs"], rs["sgprs"], rs["scratch_bytes_per_lane"],
                                                         rs["lds_bytes"], rs["occupancy_waves_per_simd"]))
    lines += ["", "`x3dstep_apply_groups_kernel` and `x3dstep_apply_lars_kernel` now instantiate the same walk (`rule_lane` of "
              "step_core.h) with the SGD rule and keep the registers, scratch and occupancy they had (84 and 88 VGPRs, no scratch, "
              "5 waves per SIMD). The compiler allocates some registers differently, orders two independent loads of the "
              "element-by-element path the other way round and emits three dword loads fewer, so the device code is close to "
              "but not the same instruction for instruction as it was. Their tests against the twins pass bit "
              "for bit, and (a) below times `apply_groups` at what profiles/group_step/ records.", "",
              "The expectation, written down before anything was measured: " + res["expectation"], "",
              "## (a) The update on the X3D-M flat buffers (%d tensors, %d elements, %d items), us per call" % (
                  up["tensors"], up["elements"], up["items"]), "",
              "Between two device events, %d calls per window, one process. Every call first copies the same gradient into the "
              "flat buffer; the copy alone is timed beside them. The scales are the recipe's (no decay on the tensors with "
              "ndim <= 1, fc2.* at %g times the rate); betas %s, eps %g; torch's AdamW runs on the 316 views of the same flat "
              "buffers with the parameter groups `hyper.torch_param_groups` gives."
              % (up["calls_per_window"], res["head_lr_scale"], tuple(res["betas"]), res["eps"]), "",
              "| path (after the copy) | us per call |", "|---|---|",
              "| the copy alone | %s |" % row("refill_alone"),
              "| `apply_groups` (no state) | %s |" % row("apply_groups"),
              "| `adam` (AdamW, no state) | %s |" % row("adam"),
              "| `torch.optim.AdamW(fused=True)` | %s |" % row("torch_adamw_fused"),
              "| `torch.optim.AdamW(foreach=True)` | %s |" % row("torch_adamw_foreach"),
              "| `lamb_moments` + `lamb_trust` + `lamb_apply` (no state) | %s |" % row("lamb_three_launches"),
              "| `measure` + the three LAMB launches (state) | %s |" % row("measure_then_lamb"),
              "| `measure` + `trust` + `apply_lars(state)` | %s |" % row("measure_then_trust_then_apply_lars"), "",
              "By the medians, after the copy: `x3dstep_adam` %.1f us, `x3dstep_apply_groups` %.1f us, a ratio of %.2f against "
              "the 1.40 expected from bytes alone: the expectation %s. The three LAMB launches %.1f us; after a `measure`, LAMB "
              "costs %+.1f us against LARS. The timing bar (the slowest window of `x3dstep_adam` faster than the fastest "
              "window of torch's fused AdamW): %s."
              % (up["adam_launch_us"], up["apply_groups_launch_us"], up["adam_over_apply_groups"],
                 "held (within a tenth)" if up["expectation_holds"] else "did NOT hold", up["lamb_launches_us"],
                 up["lamb_minus_lars_us"],
                 {True: "holds", False: "does NOT hold", None: "not measured (torch's fused AdamW did not run)"}[up.get("bar_holds")]),
              "",
              "## (b) The headline step (X3D-M, B %d, T %d, %d x %d, use_graph), ms per step" % (
                  res["shape"][0], res["shape"][1], res["shape"][2], res["shape"][2]), "",
              "Three Trainers in one process, %d steps and a synchronise per window, host clock." % res["steps_per_window"],
              "", "| Trainer | ms per step | against the defaults by the medians |", "|---|---|---|",
              "| defaults | %s | |" % _row(st["off"], "ms_per_step", "%.3f"),
              "| `optimizer=\"adamw\"` | %s | %+.1f us |" % (_row(st["adamw"], "ms_per_step", "%.3f"), st["adamw"]["cost_us_by_medians"]),
              "| `optimizer=\"lamb\"` | %s | %+.1f us |" % (_row(st["lamb"], "ms_per_step", "%.3f"), st["lamb"]["cost_us_by_medians"]),
              "", "## (c) The defaults against the parent commit", "",
              "The default path has no new launch: `ops.sgd_fused`, `x3dstep_apply`, `x3dstep_apply_groups` and "
              "`x3dstep_apply_lars` are called as before.", ""]
    lines += _bench_lines(res.get("bench_py"), res["shape"][0])
    if res.get("ratios"):
        lines += ["## The restatement against torch in fp64 (tests/test_adam_host.py, on the host)", "",
                  "Five updates on 16384 elements; the distance of the numpy restatement (which the twins and the kernels equal "
                  "bit for bit) from the fp64 run, beside the distance of the fp32 run of the same reference from it; the test "
                  "allows a ratio of 4.", ""] + ["    " + ln for ln in res["ratios"]] + [""]
    lines += ["Nothing here is a share of any peak: these are achieved times of one process on one GPU.", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    main()
