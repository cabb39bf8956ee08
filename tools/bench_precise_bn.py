"""Timing of the precise BN statistics (csrc_step/pbn.hip: x3dstep_pbn_accum, x3dstep_pbn_finish; x3dhip.precisebn) by the
protocol of tools/bench_ema.py: a warm-up, then the median of `--rounds` alternating windows with the slowest and the fastest
window.  One JSON line, also written to profiles/precise_bn/bench.json, and profiles/precise_bn/README.md from the same
figures.

    python tools/bench_precise_bn.py [--out DIR] [--rounds N] [--bench-py NAME=FILE ...]

  launches (a) on the X3D-M table (84 layers, 168 buffers), between two device events, us per call, alternating: each of the
           two launches against the torch expression of the same rule over the 168 buffers, layer by layer in fp64 (the
           streaming cell update for every split; the result into every split slot)
  compute  (b) PreciseBN.compute at K = 8 on the headline shape (X3D-M, B 8, T 16, 224 x 224) against K plain eval forwards
           of the same batches, ms per call, host clock around a synchronise
  --bench-py  files holding the JSON line of `bench.py --gpus 1`, named parent_1=..., parent_2=..., branch_1=..., branch_2=...:
           the headline step with the defaults against the parent commit, separate processes
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "x3d-multigrid_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from tools.bench_grad_monitor import B, H, T, _row, _stats  # noqa: E402
from tools.bench_guarded_step import _event_windows  # noqa: E402

K = 8


def launch_windows(dev, rounds, calls=20):
    """(a)."""
    import torch
    import x3d
    from x3dhip import _steplib, stepops
    from x3dhip.precisebn import PreciseBN
    torch.manual_seed(0)
    net = x3d.generate_model("M", n_classes=400).to(dev)
    S = net.bn1.num_splits
    pbn = PreciseBN(net)
    kt, pt = pbn._tables()
    for b in kt.buffers:
        b.copy_(torch.rand_like(b) + 0.5)
    acc, snap = pbn._acc, kt.snap
    stepops.pbn_accum(pt, acc)
    # the user's version: one fp64 accumulator set per layer
    layers = [(kt.buffers[2 * i].view(S, -1), kt.buffers[2 * i + 1].view(S, -1)) for i in range(pt.nlayers)]
    state = [dict(n=0.0, mean=torch.zeros(m.shape[1], dtype=torch.float64, device=dev),
                  m2=torch.zeros(m.shape[1], dtype=torch.float64, device=dev),
                  vsum=torch.zeros(m.shape[1], dtype=torch.float64, device=dev)) for m, _ in layers]
    outs = [(torch.empty_like(m), torch.empty_like(v)) for m, v in layers]

    def torch_accum():
        for (m, v), st in zip(layers, state):
            for j in range(S):
                mu = m[j].double()
                st["n"] += 1.0
                d = mu - st["mean"]
                st["mean"] = st["mean"] + d / st["n"]
                st["m2"] = st["m2"] + d * (mu - st["mean"])
                st["vsum"] = st["vsum"] + v[j].double()

    def torch_finish():
        for st, (om, ov) in zip(state, outs):
            om.copy_(st["mean"].float().expand_as(om))
            ov.copy_(((st["vsum"] + st["m2"]) / st["n"]).float().expand_as(ov))

    torch_accum()
    acc_one = acc.clone()                                # one pass: S cells per channel

    def ours_accum():
        stepops.pbn_accum(pt, acc)

    def ours_finish():
        stepops.pbn_finish(pt, acc_one, 1, S, snap)

    zero = torch.from_numpy(stepops.new_state()).to(dev)
    r = _event_windows({"x3dstep_pbn_accum": ours_accum, "torch_accum_84_layers": torch_accum,
                        "x3dstep_pbn_finish": ours_finish, "torch_finish_84_layers": torch_finish,
                        "x3dstep_keep_save": lambda: stepops.keep(kt, zero, _steplib.KEEP_SAVE)}, rounds, calls)
    r["calls_per_window"], r["layers"], r["buffers"], r["channels"], r["splits"] = calls, pt.nlayers, kt.nbuf, pt.channels, S
    r["work_items"], r["buffer_elements"] = pt.nwork, int(sum(b.numel() for b in kt.buffers))
    return r


def compute_windows(dev, rounds):
    """(b)."""
    import torch
    import x3d
    from x3dhip import synthetic
    from x3dhip.precisebn import PreciseBN
    torch.manual_seed(0)
    net = x3d.generate_model("M", n_classes=400).to(dev).train(True)
    xs = [synthetic.synthetic_clips(B, T, H, H, seed=1234 + i).to(dev) for i in range(K)]
    pbn = PreciseBN(net)

    def compute():
        pbn.compute(xs)

    def evals():
        net.train(False)
        with torch.no_grad():
            for x in xs:
                net(x)
        net.train(True)

    versions = {"precise_bn_compute": compute, "plain_eval_forwards": evals}
    for fn in versions.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in versions}
    for _ in range(rounds):
        for k, fn in versions.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append(1e3 * (time.perf_counter() - t0))
    r = {k: _stats(v, "ms_per_call") for k, v in ms.items()}
    r["batches"], r["splits"], r["cells"] = K, net.bn1.num_splits, pbn.cells
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "precise_bn"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--bench-py", nargs="*", default=[], metavar="NAME=FILE")
    args = ap.parse_args()
    import torch
    from tools import stamp
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = {"metric": "precise_bn", "csrc_sha16": stamp.csrc_sha16(), "csrc_step_sha16": stamp.csrc_step_sha16(),
           "commit": stamp.commit(), "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "shape": [B, T, H]}
    res["launches"] = launch_windows(dev, args.rounds)
    res["compute"] = compute_windows(dev, args.rounds)
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
    lines = ["`python bench.py --gpus 1 --steps %s --warmup %s` with the defaults on an export of the parent commit and on this "
             "tree, alternating, separate processes one after the other on one GPU:" % (any_run.get("steps"), any_run.get("warmup")),
             "", "| run | ms per step |", "|---|---|"]
    for name in sorted(bp):
        r = bp[name]
        ms = r.get("ms_per_step", r.get("step_ms", r.get("value")))
        lines.append("| %s | %s |" % (name, "%.3f" % ms if isinstance(ms, (int, float)) else json.dumps(r, sort_keys=True)))
    return lines + [""]


def readme(res):
    """profiles/precise_bn/README.md from the figures of one run."""
    la, co = res["launches"], res["compute"]
    extra = co["precise_bn_compute"]["ms_per_call"] - co["plain_eval_forwards"]["ms_per_call"]
    lines = ["# Precise BN statistics: the two launches against torch, and a K = %d pass against K eval forwards" % co["batches"], "",
             "Written by `tools/bench_precise_bn.py` on %s; `bench.json` beside this file holds every figure. A warm-up, then the "
             "median of %d alternating windows with the fastest and the slowest window in brackets. Sources: csrc_step %s, csrc %s."
             % (res["device"], res["rounds"], res["csrc_step_sha16"], res["csrc_sha16"]), "",
             "## (a) The launches on the X3D-M table (%d layers, %d buffers of %d elements, %d channels, %d splits, %d work items), "
             "us per call" % (la["layers"], la["buffers"], la["buffer_elements"], la["channels"], la["splits"], la["work_items"]), "",
             "Between two device events, %d calls per window, one process. The torch rows are the same rule written layer by "
             "layer in fp64: the streaming cell update for every split, and the result expanded into every split slot."
             % la["calls_per_window"], "",
             "| path | us per call |", "|---|---|",
             "| `x3dstep_pbn_accum` (1 launch) | %s |" % _row(la["x3dstep_pbn_accum"], "us_per_call", "%.1f"),
             "| the cell rule in torch over the %d layers | %s |" % (la["layers"], _row(la["torch_accum_84_layers"], "us_per_call", "%.1f")),
             "| `x3dstep_pbn_finish` (1 launch, one rank) | %s |" % _row(la["x3dstep_pbn_finish"], "us_per_call", "%.1f"),
             "| the result rule in torch over the %d layers | %s |" % (la["layers"], _row(la["torch_finish_84_layers"], "us_per_call", "%.1f")),
             "| `x3dstep_keep` (save), the launch the estimate named | %s |" % _row(la["x3dstep_keep_save"], "us_per_call", "%.1f"), "",
             "The estimate written before anything was measured was that each launch costs about what a keep launch costs "
             "(8.4 us in `profiles/guarded_step/`). These are end-to-end figures of back-to-back calls, launch overhead included; "
             "no kernel trace was taken.", "",
             "## (b) `PreciseBN.compute` at K = %d on the headline shape (X3D-M, B %d, T %d, %d x %d, %d splits, %d cells), ms per call"
             % (co["batches"], res["shape"][0], res["shape"][1], res["shape"][2], res["shape"][2], co["splits"], co["cells"]), "",
             "Host clock around a synchronise, one call per window.", "",
             "| path | ms per call |", "|---|---|",
             "| `PreciseBN.compute` (save, %d training-mode trunk passes + accum, swap, finish) | %s |" % (
                 co["batches"], _row(co["precise_bn_compute"], "ms_per_call", "%.2f")),
             "| %d plain eval forwards of the same batches | %s |" % (co["batches"], _row(co["plain_eval_forwards"], "ms_per_call", "%.2f")),
             "", "By the medians the pass takes %+.2f ms against the eval forwards. A training-mode trunk pass computes the batch "
             "statistics that an eval forward reads from memory; the eval forward also derives its coefficients from `bn.*` layer "
             "by layer and runs the head, which the pass leaves out." % extra, "",
             "## The defaults against the parent commit", ""]
    lines += _bench_py_lines(res.get("bench_py"))
    lines += ["With the defaults nothing of this feature runs in a training step: no attribute, not one launch.", "",
              "Nothing here is a share of any peak: these are achieved times of one process on one GPU.", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    main()
