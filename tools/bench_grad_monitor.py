"""Timing of the gradient monitor (csrc_step/step.hip, x3dhip.gradmonitor) by the protocol of profiles/jpeg_index/: a
warm-up, then the median of `--rounds` alternating windows with the slowest and the fastest window.  One JSON line, also
written to profiles/grad_monitor/bench.json, and profiles/grad_monitor/README.md from the same figures.

    python tools/bench_grad_monitor.py [--out DIR] [--rounds N] [--steps K] [--parent-json FILE]
    python tools/bench_grad_monitor.py --off-only --json-out FILE     (also on a tree without the monitor: the parent commit)

  launches   on the X3D-M flat buffers (316 tensors, 3.79 M elements), between two device events, us per call, alternating:
             the monitor's launches (statistics only: two; statistics and clipping: three) and what a user can do without
             them, torch.nn.utils.clip_grad_norm_ on the 316 gradient views.  A clipped gradient has norm max_norm and
             the next call would leave it alone, so every timed call of every path first copies the same gradient (norm
             19.5, max_norm 1) into the flat buffer; the copy alone is timed beside them.
  step       the headline step (X3D-M, B 8, T 16, 224 x 224, use_graph) with the monitor off, on, and on with clipping: three
             Trainers in one process, alternating window by window, ms per step (host clock around K steps and a synchronise)
  --off-only the `off` windows alone through the same code, for a run on the parent commit; --parent-json reads its file
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "x3d-multigrid_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

B, T, H = 8, 16, 224
MAX_NORM = 1.0       # the gradient of the launch windows has norm 19.5: every call scales it by about 0.05
STEP_MAX_NORM = 1e-3


def _stats(v, key):
    return {key: statistics.median(v), key + "_min": min(v), key + "_max": max(v)}


def _trainer(dev, **kw):
    import torch
    import x3d
    from x3dhip.trainer import Trainer
    torch.manual_seed(0)
    net = x3d.generate_model("M", n_classes=400, dropout=0.5, base_bn_splits=max(1, B // 8)).to(dev).train(True)
    return Trainer(net, lr=0.05, use_graph=True, **kw)


def step_windows(dev, variants, rounds, steps, warmup):
    """ms per step of each Trainer variant, alternating window by window."""
    import torch
    from x3dhip import synthetic
    x = synthetic.synthetic_clips(B, T, H, H, seed=1234).to(dev)
    y = synthetic.synthetic_labels(B, seed=1234).to(dev)
    trainers, feeds = {}, {}
    for name, kw in variants:
        tr = trainers[name] = _trainer(dev, **kw)
        for _ in range(warmup):
            tr.step(x, y)
        st = tr.static_inputs(x.shape)          # the clips resident in the graph's own inputs: no copy in a timed step
        st[0].copy_(x)
        st[1].copy_(y)
        feeds[name] = st
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, _ in variants:
            tr, (xs, ys) = trainers[name], feeds[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.step(xs, ys)
            torch.cuda.synchronize()
            ms[name].append(1e3 * (time.perf_counter() - t0) / steps)
    return {k: _stats(v, "ms_per_step") for k, v in ms.items()}, trainers


def launch_windows(dev, rounds, calls=20):
    """us per call of the monitor's launches and of torch's clip_grad_norm_ on the X3D-M flat buffers."""
    import torch
    import x3d
    from x3dhip.gradmonitor import GradMonitor
    from x3dhip.trainer import FlatParams
    torch.manual_seed(0)
    net = x3d.generate_model("M", n_classes=400).to(dev)
    fp = FlatParams(net)
    names = [k for k, _ in net.named_parameters()]
    g0 = torch.randn(fp.numel, device=dev) * 0.01
    params = list(net.parameters())
    mon, clip = GradMonitor(fp, names, ring=64), GradMonitor(fp, names, ring=64, max_norm=MAX_NORM)
    # the same coefficient first: both paths on the same gradient
    fp.grad.copy_(g0)
    clip.observe()
    ours = fp.grad.clone()
    coef = float(clip.last_coef())
    fp.grad.copy_(g0)
    total = torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
    theirs_coef = MAX_NORM / (float(total) + 1e-6)
    assert abs(coef - theirs_coef) <= 1e-6 * theirs_coef, (coef, theirs_coef)
    assert torch.allclose(ours, fp.grad, rtol=1e-5, atol=0)

    def with_refill(fn):
        def call():
            fp.grad.copy_(g0)
            fn()
        return call

    versions = {"refill_alone": with_refill(lambda: None), "monitor_2_launches": with_refill(mon.observe),
                "monitor_clip_3_launches": with_refill(clip.observe),
                "torch_clip_grad_norm": with_refill(lambda: torch.nn.utils.clip_grad_norm_(params, MAX_NORM))}
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
    r = {k: _stats(v, "us_per_call") for k, v in us.items()}
    assert float(clip.last_coef()) == coef < 1.0  # still scaling at the end of the run, by the same coefficient
    r["calls_per_window"] = calls
    r["tensors"], r["elements"], r["items"] = len(names), fp.numel, mon.tables.nitems
    r["bar_slowest_faster_than_torch_fastest"] = (r["monitor_clip_3_launches"]["us_per_call_max"]
                                                  < r["torch_clip_grad_norm"]["us_per_call_min"])
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_monitor"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30, help="steps per timed window of the headline step")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--off-only", action="store_true", help="only the `off` windows of the headline step")
    ap.add_argument("--json-out", default=None, help="with --off-only: where the JSON line goes")
    ap.add_argument("--parent-json", default=None, help="the file an --off-only run on the parent commit wrote")
    ap.add_argument("--kernel-trace-json", default=None,
                    help="per-kernel times of a kernel trace taken in a run of its own: {command, kernels: {name: {us, ..}}}")
    args = ap.parse_args()
    import torch
    from tools import stamp
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = {"metric": "grad_monitor", "csrc_sha16": stamp.csrc_sha16(), "commit": stamp.commit(),
           "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "steps_per_window": args.steps,
           "shape": [B, T, H]}
    if args.off_only:
        res["step"], _ = step_windows(dev, [("off", {})], args.rounds, args.steps, args.warmup)
        out = json.dumps(res, sort_keys=True)
        print(out)
        if args.json_out:
            os.makedirs(os.path.dirname(os.path.abspath(args.json_out)), exist_ok=True)
            with open(args.json_out, "w") as f:
                f.write(out + "\n")
        return
    res["csrc_step_sha16"] = stamp.csrc_step_sha16()
    res["max_norm"] = MAX_NORM
    res["launches"] = launch_windows(dev, args.rounds)
    # a max_norm far below the gradient's norm: the scale launch does its work in every timed step
    variants = [("off", {}), ("monitor", dict(monitor=True)), ("monitor_clip", dict(monitor=True, clip_grad_norm=STEP_MAX_NORM))]
    res["step"], trainers = step_windows(dev, variants, args.rounds, args.steps, args.warmup)
    off = res["step"]["off"]
    for k in ("monitor", "monitor_clip"):
        res["step"][k]["cost_us_by_medians"] = 1e3 * (res["step"][k]["ms_per_step"] - off["ms_per_step"])
    res["step"]["last_coef_monitor_clip"] = float(trainers["monitor_clip"].monitor.last_coef())
    if args.parent_json:
        with open(args.parent_json) as f:
            parent = json.loads(f.read())
        res["parent"] = {"commit": parent.get("commit"), "csrc_sha16": parent["csrc_sha16"], "off": parent["step"]["off"]}
        p = parent["step"]["off"]
        res["parent"]["bar_off_median_within_parent_window"] = p["ms_per_step_min"] <= off["ms_per_step"] <= p["ms_per_step_max"]
    if args.kernel_trace_json:
        with open(args.kernel_trace_json) as f:
            res["kernel_trace"] = json.loads(f.read())
    out = json.dumps(res, sort_keys=True)
    print(out)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench.json"), "w") as f:
        f.write(out + "\n")
    with open(os.path.join(args.out, "README.md"), "w") as f:
        f.write(readme(res))


def _row(s, key, fmt):
    return (fmt + " (" + fmt + " .. " + fmt + ")") % (s[key], s[key + "_min"], s[key + "_max"])


def _holds(flag):
    return "holds" if flag else "DOES NOT HOLD"


def _trace_line(kt):
    """The per-kernel times of a kernel trace taken in a run of its own (--kernel-trace-json), or that there is none."""
    if not kt:
        return ("- How the time divides between the three kernels was not measured: no kernel trace was given "
                "(`--kernel-trace-json`).")
    k = kt["kernels"]
    return ("- A kernel trace in a run of its own (`kernel_trace.json`: %s) gives, by the medians, %.1f us for the partials "
            "kernel, %.1f us for the one-workgroup finalize kernel and %.1f us for the scale kernel. The finalize kernel is "
            "the largest part: its two ordered, compensated fp64 sums are one thread's work each, first the items of a "
            "tensor (432 for the largest), then the 316 tensors. Summing a large tensor's items in chunks by several "
            "threads would shorten it and is not built." % (
                kt["command"], k["x3dstep_partials_kernel"]["us"], k["x3dstep_finalize_kernel"]["us"],
                k["x3dstep_scale_kernel"]["us"]))


def readme(res):
    """profiles/grad_monitor/README.md from the figures of one run."""
    la, st = res["launches"], res["step"]
    lines = ["# Gradient monitor: the three launches against torch, and their price on the headline step", "",
             "Written by `tools/bench_grad_monitor.py` on %s; `bench.json` beside this file holds every figure. The protocol is "
             "that of `profiles/jpeg_index/`: a warm-up, then the median of %d alternating windows with the slowest and the "
             "fastest window in brackets. Sources: csrc_step %s, csrc %s." % (
                 res["device"], res["rounds"], res["csrc_step_sha16"], res["csrc_sha16"]), "",
             "## The launches on the X3D-M flat buffers (%d tensors, %d elements, %d items), us per call" % (
                 la["tensors"], la["elements"], la["items"]), "",
             "Between two device events, %d calls per window. A clipped gradient would be left alone by the next call, so every "
             "call of every path first copies the same gradient (norm 19.5) into the flat buffer; max_norm %g, so every call "
             "scales it." % (la["calls_per_window"], res["max_norm"]), "",
             "| path (after the copy) | us per call |", "|---|---|",
             "| the copy alone | %s |" % _row(la["refill_alone"], "us_per_call", "%.1f"),
             "| statistics and the record (2 launches) | %s |" % _row(la["monitor_2_launches"], "us_per_call", "%.1f"),
             "| statistics, the record and clipping (3 launches) | %s |" % _row(la["monitor_clip_3_launches"], "us_per_call", "%.1f"),
             "| `torch.nn.utils.clip_grad_norm_` on the 316 `.grad` views | %s |" % _row(la["torch_clip_grad_norm"], "us_per_call", "%.1f"),
             "", "The bar: the three launches' slowest window is faster than torch's fastest window: %s (%.1f us against %.1f us; "
             "%.1f x by the medians)." % (
                 _holds(la["bar_slowest_faster_than_torch_fastest"]), la["monitor_clip_3_launches"]["us_per_call_max"],
                 la["torch_clip_grad_norm"]["us_per_call_min"],
                 la["torch_clip_grad_norm"]["us_per_call"] / la["monitor_clip_3_launches"]["us_per_call"]), "",
             "## The headline step (X3D-M, B %d, T %d, %d x %d, use_graph), ms per step" % (
                 res["shape"][0], res["shape"][1], res["shape"][2], res["shape"][2]), "",
             "Three Trainers in one process, %d steps and a synchronise per window, host clock." % res["steps_per_window"], "",
             "| Trainer | ms per step | cost by the medians |", "|---|---|---|",
             "| defaults (monitor off) | %s | |" % _row(st["off"], "ms_per_step", "%.3f"),
             "| `monitor=True` | %s | %+.1f us |" % (_row(st["monitor"], "ms_per_step", "%.3f"), st["monitor"]["cost_us_by_medians"]),
             "| `monitor=True, clip_grad_norm=%g` | %s | %+.1f us |" % (
                 STEP_MAX_NORM, _row(st["monitor_clip"], "ms_per_step", "%.3f"), st["monitor_clip"]["cost_us_by_medians"]),
             "", "Turning the monitor on is a price, not a regression: there is no bar on it. The coefficient of the last "
             "clipped step was %.3g (below 1: the scale launch did its work)." % st["last_coef_monitor_clip"], ""]
    if "parent" in res:
        p = res["parent"]
        lines += ["The bar for the defaults: the `off` median lies within the minimum .. maximum of the parent commit%s run "
                  "the same way (`--off-only`, csrc %s): %s. Parent: %s ms; this tree: %s ms." % (
                      " " + p["commit"] if p.get("commit") else "", p["csrc_sha16"],
                      _holds(p["bar_off_median_within_parent_window"]), _row(p["off"], "ms_per_step", "%.3f"),
                      _row(st["off"], "ms_per_step", "%.3f")),
                  "The two are separate processes one after the other, and their windows are a few microseconds wide: this "
                  "tree's median is %+.2f %% from the parent's." % (
                      100 * (st["off"]["ms_per_step"] / p["off"]["ms_per_step"] - 1)), ""]
    else:
        lines += ["No parent-commit run was given (`--parent-json`): the bar for the defaults was not evaluated.", ""]
    net2 = la["monitor_2_launches"]["us_per_call"] - la["refill_alone"]["us_per_call"]
    net3 = la["monitor_clip_3_launches"]["us_per_call"] - la["refill_alone"]["us_per_call"]
    lines += ["## Reading the figures", "",
              "- Less the copy, the two launches take %.0f us and the three %.0f us; the same less the copy for torch: %.0f us. "
              "The expectation written before anything was measured was a launch-bound 10 to 20 us: the launches are not "
              "launch-bound." % (net2, net3, la["torch_clip_grad_norm"]["us_per_call"] - la["refill_alone"]["us_per_call"]),
              _trace_line(res.get("kernel_trace")),
              "- In the step the price is higher than between events: there the launches follow a graph replay and precede "
              "the SGD launch, and the host clock also sees their enqueue.",
              "- `bench_py_parent_*.json` / `bench_py_branch_*.json` beside this file, when present, are `bench.py --gpus 1 "
              "--steps 200 --warmup 20` on an export of the parent commit and on this tree, alternating, one after the other on one GPU.", "",
              "Nothing here is a share of any peak: these are achieved times of one process on one GPU.", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    main()
