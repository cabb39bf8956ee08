"""Timing of the weight average (csrc_step/ema.hip: x3dstep_ema, x3dstep_ema_keep, x3dstep_swap, x3dstep_swap_keep;
Trainer(ema_decay=)) by the protocol of tools/bench_grad_monitor.py: a warm-up, then the median of `--rounds` alternating
windows with the slowest and the fastest window.  One JSON line, also written to profiles/ema/bench.json, and
profiles/ema/README.md from the same figures.

    python tools/bench_ema.py [--out DIR] [--rounds N] [--steps K] [--bench-py NAME=FILE ...]

  update   (a) on the X3D-M buffers (316 parameter tensors, 3.79 M elements; 168 running-statistics buffers), between two
           device events, us per call, alternating: WeightEMA.update() (two launches) against what a user would write --
           torch._foreach_mul_ + torch._foreach_add_ over the 316 parameter views and the 168 buffers, and
           e.mul_(d).add_(w, alpha=1 - d) on the flat buffer alone; and each of the two launches alone
  swap     (b) the two exchange launches of WeightEMA.applied(), alone and as the pair
  step     (c) the headline step (X3D-M, B 8, T 16, 224 x 224, use_graph) with ema_decay off and on: two Trainers in one
           process, alternating window by window, ms per step
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

from tools.bench_grad_monitor import B, H, T, _row, step_windows  # noqa: E402
from tools.bench_guarded_step import _event_windows  # noqa: E402

DECAY = 0.9999


def update_windows(dev, rounds, calls=20):
    """(a) and (b)."""
    import torch
    import x3d
    from x3dhip import stepops
    from x3dhip.trainer import FlatParams
    from x3dhip.weightema import WeightEMA, running_stat_buffers
    torch.manual_seed(0)
    net = x3d.generate_model("M", n_classes=400).to(dev)
    fp = FlatParams(net)
    ema = WeightEMA(fp, net, DECAY, warmup=False)
    kt = ema._table()
    stats = [b for _, b in running_stat_buffers(net)]
    # the user's version: one averaged tensor per parameter view and per buffer
    e_views = [p.data.clone() for p in fp.params]
    e_stats = [b.clone() for b in stats]
    w_views = [p.data for p in fp.params]
    e_flat = fp.flat.clone()
    d = DECAY

    def foreach_path():
        torch._foreach_mul_(e_views, d)
        torch._foreach_add_(e_views, w_views, alpha=1 - d)
        torch._foreach_mul_(e_stats, d)
        torch._foreach_add_(e_stats, stats, alpha=1 - d)

    def flat_path():
        e_flat.mul_(d).add_(fp.flat, alpha=1 - d)

    count = [0]

    def flat_launch():
        count[0] += 1
        stepops.ema(ema.e, fp.flat, None, count[0], DECAY, False)

    def keep_launch():
        count[0] += 1
        stepops.ema_keep(kt, kt.snap, None, count[0], DECAY, False)

    r = _event_windows({"ema_update_two_launches": ema.update, "foreach_over_484_tensors": foreach_path,
                        "flat_torch_expression_weights_only": flat_path, "x3dstep_ema_alone": flat_launch,
                        "x3dstep_ema_keep_alone": keep_launch}, rounds, calls)
    r["calls_per_window"], r["tensors"], r["elements"] = calls, len(fp.params), fp.numel
    r["buffers"], r["buffer_elements"], r["items"] = kt.nbuf, int(sum(b.numel() for b in stats)), kt.nitems
    r["bytes_moved_flat"] = 12 * fp.numel                # two reads and one write of fp32
    gbs = r["bytes_moved_flat"] / (r["x3dstep_ema_alone"]["us_per_call"] * 1e-6) / 1e9
    r["flat_launch_achieved_GB_per_s"] = gbs

    def both_swaps():
        stepops.swap(fp.flat, ema.e)
        stepops.swap_keep(kt, kt.snap)

    s = _event_windows({"swap_flat": lambda: stepops.swap(fp.flat, ema.e), "swap_keep": lambda: stepops.swap_keep(kt, kt.snap),
                        "both_as_applied_enters": both_swaps}, rounds, calls)
    s["calls_per_window"] = calls
    return r, s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30, help="steps per timed window of the headline step")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bench-py", nargs="*", default=[], metavar="NAME=FILE")
    args = ap.parse_args()
    import torch
    from tools import stamp
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = {"metric": "weight_ema", "csrc_sha16": stamp.csrc_sha16(), "csrc_step_sha16": stamp.csrc_step_sha16(),
           "commit": stamp.commit(), "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "steps_per_window": args.steps, "shape": [B, T, H], "decay": DECAY}
    res["update"], res["swap"] = update_windows(dev, args.rounds)
    res["step"], trainers = step_windows(dev, [("off", {}), ("ema", dict(ema_decay=DECAY))], args.rounds, args.steps, args.warmup)
    res["step"]["ema"]["cost_us_by_medians"] = 1e3 * (res["step"]["ema"]["ms_per_step"] - res["step"]["off"]["ms_per_step"])
    res["step"]["updates"] = trainers["ema"].ema.updates()
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
    lines = ["`python bench.py --gpus 1 --steps %s --warmup %s` with the defaults (no average) on an export of the parent commit "
             "and on this tree, alternating, separate processes one after the other on one GPU:" % (
                 any_run.get("steps"), any_run.get("warmup")), "",
             "| run | ms per step |", "|---|---|"]
    for name in sorted(bp):
        r = bp[name]
        ms = r.get("ms_per_step", r.get("step_ms", r.get("value")))
        lines.append("| %s | %s |" % (name, "%.3f" % ms if isinstance(ms, (int, float)) else json.dumps(r, sort_keys=True)))
    return lines + [""]


def readme(res):
    """profiles/ema/README.md from the figures of one run."""
    up, sw, st = res["update"], res["swap"], res["step"]
    ours, flat = up["x3dstep_ema_alone"]["us_per_call"], up["flat_torch_expression_weights_only"]["us_per_call"]
    verdict = ("The flat launch is slower than the flat torch expression by the medians (%.1f against %.1f us): torch's two "
               "elementwise kernels each stream the buffer at the full rate, and this launch, one 16-byte group per lane and "
               "four per thread, does not make up in saved traffic (12 against 20 bytes per element) what it loses in rate."
               % (ours, flat)) if ours > flat else (
               "The flat launch is not slower than the flat torch expression by the medians (%.1f against %.1f us): one pass "
               "of 12 bytes per element against two passes of 20." % (ours, flat))
    lines = ["# Weight EMA: the two update launches against torch, the exchange, and their price on the headline step", "",
             "Written by `tools/bench_ema.py` on %s; `bench.json` beside this file holds every figure. A warm-up, then the median "
             "of %d alternating windows with the fastest and the slowest window in brackets. Sources: csrc_step %s, csrc %s."
             % (res["device"], res["rounds"], res["csrc_step_sha16"], res["csrc_sha16"]), "",
             "## (a) The update on the X3D-M buffers (%d tensors, %d elements; %d buffers, %d elements, %d items), us per call"
             % (up["tensors"], up["elements"], up["buffers"], up["buffer_elements"], up["items"]), "",
             "Between two device events, %d calls per window, one process, decay %g without warm-up." % (
                 up["calls_per_window"], res["decay"]), "",
             "| path | us per call |", "|---|---|",
             "| `WeightEMA.update()`: `x3dstep_ema` + `x3dstep_ema_keep` (2 launches) | %s |" % _row(
                 up["ema_update_two_launches"], "us_per_call", "%.1f"),
             "| `torch._foreach_mul_` + `_foreach_add_` over the %d views and the %d buffers | %s |" % (
                 up["tensors"], up["buffers"], _row(up["foreach_over_484_tensors"], "us_per_call", "%.1f")),
             "| `e.mul_(d).add_(w, alpha=1 - d)` on the flat buffer (weights only, no statistics) | %s |" % _row(
                 up["flat_torch_expression_weights_only"], "us_per_call", "%.1f"),
             "| `x3dstep_ema` alone | %s |" % _row(up["x3dstep_ema_alone"], "us_per_call", "%.1f"),
             "| `x3dstep_ema_keep` alone | %s |" % _row(up["x3dstep_ema_keep_alone"], "us_per_call", "%.1f"), "",
             "The flat launch moves %.1f MB (two reads and one write of fp32); over its median that is %.0f GB/s achieved, "
             "launch overhead included: an end-to-end figure of back-to-back calls, not a kernel's share of peak (no kernel "
             "trace was taken), and not an HBM rate either: both buffers together are 30 MB, which the 256 MB last-level cache "
             "holds from one call to the next. The estimate written before anything was measured was the order of the scale kernel's 10 us "
             "plus a launch." % (up["bytes_moved_flat"] / 1e6, up["flat_launch_achieved_GB_per_s"]), "", verdict, "",
             "## (b) The exchange of `WeightEMA.applied()`, us per call", "",
             "| launch | us per call |", "|---|---|",
             "| `x3dstep_swap` on the flat buffer | %s |" % _row(sw["swap_flat"], "us_per_call", "%.1f"),
             "| `x3dstep_swap_keep` on the statistics | %s |" % _row(sw["swap_keep"], "us_per_call", "%.1f"),
             "| both, as the block enters or leaves | %s |" % _row(sw["both_as_applied_enters"], "us_per_call", "%.1f"), "",
             "## (c) The headline step (X3D-M, B %d, T %d, %d x %d, use_graph), ms per step" % (
                 res["shape"][0], res["shape"][1], res["shape"][2], res["shape"][2]), "",
             "Two Trainers in one process, %d steps and a synchronise per window, host clock." % res["steps_per_window"], "",
             "| Trainer | ms per step | cost by the medians |", "|---|---|---|",
             "| defaults (no average) | %s | |" % _row(st["off"], "ms_per_step", "%.3f"),
             "| `ema_decay=%g` | %s | %+.1f us |" % (res["decay"], _row(st["ema"], "ms_per_step", "%.3f"),
                                                    st["ema"]["cost_us_by_medians"]), "",
             "The average is a price, not a regression: it adds two launches to a step that had none (%d updates were "
             "averaged in these windows)." % st["updates"], "",
             "## The defaults against the parent commit", ""]
    lines += _bench_py_lines(res.get("bench_py"))
    lines += ["Nothing here is a share of any peak: these are achieved times of one process on one GPU.", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    main()
