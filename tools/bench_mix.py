"""Timing of batch mixing and the soft-target loss (csrc_mix/mix.hip; x3dhip.mixops, x3dhip.mixing, Trainer(objective="soft_ce"))
by the protocol of tools/bench_lars.py: a warm-up, then the median of `--rounds` alternating windows with the slowest and the
fastest window.  One JSON line, also written to profiles/mix/bench.json, and profiles/mix/README.md from the same figures.

    python tools/bench_mix.py [--out DIR] [--rounds N] [--steps K] [--bench-py NAME=FILE ...]

  clips    (a) the headline batch (8 clips of 3 x 16 x 224 x 224 floats, 77 MB), between two device events, us per call,
           alternating: mix_clips with a mixup plan against the torch expression x * lam + x[perm] * (1 - lam); mix_clips with a
           CutMix plan against a clone and the box assignment; mix_clips with the identity plan; copy_ of the same tensor.
           The achieved bytes/s of each from the bytes its rule has to move.
  loss     (b) mix_targets + soft_ce on [8, 400] against one_hot, smoothing, the mix and F.cross_entropy with its gradient
           in torch; soft_ce on one-hot targets against x3d_head_ce: the same bits or not.
  step     (c) the headline step (X3D-M, B 8, T 16, 224 x 224, use_graph) with the defaults against the same step with a
           BatchMixer(mixup 0.8, cutmix 1.0, smoothing 0.1) writing into the graph's static inputs and objective "soft_ce":
           two Trainers in one process, alternating window by window, ms per step
  --bench-py  (d) files holding the JSON line of `bench.py --gpus 1`, named parent_1=..., parent_2=..., branch_1=..., branch_2=...
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

from tools.bench_grad_monitor import B, H, T, _row, _stats, _trainer  # noqa: E402
from tools.bench_group_step import _bench_lines  # noqa: E402
from tools.bench_guarded_step import _event_windows  # noqa: E402

NC = 400
MIXUP, CUTMIX, SMOOTHING = 0.8, 1.0, 0.1
LAM = 0.7
BOX = (40, 170, 25, 150)                # y0, y1, x0, x1: 130 x 125 of 224 x 224 (x0 odd: no row of the box starts on a 16-byte group)
# The kernels' resource usage, from the compiler's remarks (-Rpass-analysis=kernel-resource-usage, gfx950).
RESOURCES = {
    "x3dmix_clips_kernel": dict(vgprs=60, sgprs=72, scratch_bytes_per_lane=0, lds_bytes=0, occupancy_waves_per_simd=8),
    "x3dmix_targets_kernel": dict(vgprs=6, sgprs=24, scratch_bytes_per_lane=0, lds_bytes=0, occupancy_waves_per_simd=8),
    "x3dmix_soft_ce_rows_kernel": dict(vgprs=31, sgprs=37, scratch_bytes_per_lane=0, lds_bytes=16, occupancy_waves_per_simd=8),
    "x3dmix_soft_ce_mean_kernel": dict(vgprs=14, sgprs=17, scratch_bytes_per_lane=0, lds_bytes=32, occupancy_waves_per_simd=8),
}
# Written down before the first measurement.
EXPECTATION = ("mix_clips moves 3 x 77 MB for mixup (read two clips, write one) in one launch where the torch expression makes "
               "four launches and moves about 10 x 77 MB (the gather, two products, the sum), so it should take well under half "
               "of torch's time and reach the bytes/s of copy_; CutMix reads the partner only where the box is, so it should "
               "cost about what a copy costs.  mix_targets + soft_ce are three small launches against about ten in torch.  "
               "The mixed step adds those launches and one pass over the batch to a step of about 23 ms.")


def clip_windows(dev, rounds, calls=10):
    """(a)"""
    import numpy as np
    import torch
    from x3dhip import mixops, synthetic
    x = synthetic.synthetic_clips(B, T, H, H, seed=1234).to(dev)
    out = torch.empty_like(x)
    perm = np.roll(np.arange(B), 1)
    plan_mix = mixops.identity_plan(B)
    plan_mix["partner"], plan_mix["lam"] = perm, LAM
    plan_cut = plan_mix.copy()
    plan_cut["y0"], plan_cut["y1"], plan_cut["x0"], plan_cut["x1"] = BOX
    d_id, d_mix, d_cut = (mixops.plan_to_device(p, dev) for p in (mixops.identity_plan(B), plan_mix, plan_cut))
    tperm = torch.from_numpy(perm).to(dev)
    y0, y1, x0, x1 = BOX

    def torch_mixup():
        return x * LAM + x[tperm] * (1.0 - LAM)

    def torch_cutmix():
        o = x.clone()
        o[..., y0:y1, x0:x1] = x[tperm][..., y0:y1, x0:x1]
        return o

    # the same values first: CutMix bit for bit, mixup within the roundings of the two expressions
    assert torch.equal(mixops.mix_clips(x, d_cut, out=out), torch_cutmix())
    assert float((mixops.mix_clips(x, d_mix, out=out) - torch_mixup()).abs().max()) <= 1e-6 * float(x.abs().max())
    assert torch.equal(mixops.mix_clips(x, d_id, out=out), x)
    r = _event_windows({
        "copy_": lambda: out.copy_(x),
        "mix_clips_identity": lambda: mixops.mix_clips(x, d_id, out=out),
        "mix_clips_mixup": lambda: mixops.mix_clips(x, d_mix, out=out),
        "torch_mixup": torch_mixup,
        "mix_clips_cutmix": lambda: mixops.mix_clips(x, d_cut, out=out),
        "torch_cutmix": torch_cutmix,
    }, rounds, calls)
    nbytes = x.numel() * 4
    box_share = (y1 - y0) * (x1 - x0) / float(H * H)
    moved = {"copy_": 2.0, "mix_clips_identity": 2.0, "mix_clips_mixup": 3.0, "mix_clips_cutmix": 2.0 + box_share}
    for k, f in moved.items():
        r[k]["bytes_moved"] = f * nbytes
        r[k]["tb_per_s"] = f * nbytes / (r[k]["us_per_call"] * 1e-6) / 1e12
    r["clip_bytes"], r["calls_per_window"], r["box_share"] = nbytes, calls, box_share
    r["mixup_not_slower_than_torch"] = bool(r["mix_clips_mixup"]["us_per_call_max"] <= r["torch_mixup"]["us_per_call_min"])
    r["cutmix_not_slower_than_torch"] = bool(r["mix_clips_cutmix"]["us_per_call_max"] <= r["torch_cutmix"]["us_per_call_min"])
    return r


def loss_windows(dev, rounds, calls=50):
    """(b)"""
    import numpy as np
    import torch
    import torch.nn.functional as F
    from x3dhip import mixops, ops
    g = torch.Generator().manual_seed(5)
    z = (4.0 * torch.randn(B, NC, generator=g)).to(dev)
    y = torch.randint(0, NC, (B,), generator=g).to(dev)
    perm = np.roll(np.arange(B), 1)
    plan = mixops.identity_plan(B)
    plan["partner"], plan["lam"] = perm, LAM
    dplan = mixops.plan_to_device(plan, dev)
    tperm = torch.from_numpy(perm).to(dev)
    off = SMOOTHING / NC
    on = 1.0 - SMOOTHING + off

    def ours():
        t = mixops.mix_targets(y, dplan, NC, SMOOTHING)
        return mixops.soft_ce(z, t)

    def in_torch():
        s = F.one_hot(y, NC).float() * (on - off) + off
        t = s * LAM + s[tperm] * (1.0 - LAM)
        zz = z.detach().requires_grad_(True)
        loss = F.cross_entropy(zz, t)
        (d,) = torch.autograd.grad(loss, zz)
        return loss, d

    (la, da), (lb, db) = ours(), in_torch()
    assert abs(float(la) - float(lb)) <= 2e-6 * abs(float(lb)) and float((da - db).abs().max()) <= 2e-6 * float(db.abs().max())
    r = _event_windows({"mix_targets_soft_ce": ours, "torch_one_hot_smooth_cross_entropy": in_torch}, rounds, calls)
    r["calls_per_window"] = calls
    onehot = F.one_hot(y, NC).float()
    ls, ds = mixops.soft_ce(z, onehot)
    lh, dh = ops.head_ce(z, y)
    r["one_hot_loss_bits_equal_head_ce"] = bool(torch.equal(ls, lh))
    r["one_hot_gradient_bits_equal_head_ce"] = bool(torch.equal(ds, dh))
    r["one_hot_gradient_max_abs_difference"] = float((ds - dh).abs().max())
    return r


def step_windows(dev, rounds, steps, warmup):
    """(c)"""
    import torch
    from x3dhip import synthetic
    from x3dhip.mixing import BatchMixer
    x = synthetic.synthetic_clips(B, T, H, H, seed=1234).to(dev)
    y = synthetic.synthetic_labels(B, seed=1234).to(dev)
    off, mix = _trainer(dev), _trainer(dev, objective="soft_ce")
    mixer = BatchMixer(NC, mixup_alpha=MIXUP, cutmix_alpha=CUTMIX, label_smoothing=SMOOTHING, seed=1234)

    def mixed_step():
        mix.step(*mixer(x, y, out=mix.static_inputs(x.shape)))

    for _ in range(warmup):
        off.step(x, y)
        mixed_step()
    sx, sy = off.static_inputs(x.shape)     # the clips resident in the graph's own inputs: no copy in a timed step
    sx.copy_(x)
    sy.copy_(y)
    fns = {"off": lambda: off.step(sx, sy), "mixup_cutmix_smoothing": mixed_step}
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            ms[k].append(1e3 * (time.perf_counter() - t0) / steps)
    r = {k: _stats(v, "ms_per_step") for k, v in ms.items()}
    r["mixup_cutmix_smoothing"]["cost_us_by_medians"] = 1e3 * (r["mixup_cutmix_smoothing"]["ms_per_step"] - r["off"]["ms_per_step"])
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mix"))
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
        from tools import stamp
        dev = torch.device("cuda:0")
        torch.cuda.set_device(dev)
        res = {"metric": "mix", "csrc_sha16": stamp.csrc_sha16(), "csrc_mix_sha16": stamp.csrc_mix_sha16(),
               "commit": stamp.commit(), "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
               "steps_per_window": args.steps, "shape": [B, T, H], "resources": RESOURCES, "expectation": EXPECTATION,
               "mixup": MIXUP, "cutmix": CUTMIX, "smoothing": SMOOTHING, "lam": LAM, "box": list(BOX), "bench_py": {}}
        res["clips"] = clip_windows(dev, args.rounds)
        res["loss"] = loss_windows(dev, args.rounds)
        res["step"] = step_windows(dev, args.rounds, args.steps, args.warmup)
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
    """profiles/mix/README.md from the figures of one run."""
    cl, lo, st = res["clips"], res["loss"], res["step"]
    row = lambda k: _row(cl[k], "us_per_call", "%.1f")      # noqa: E731
    tb = lambda k: "%.2f" % cl[k]["tb_per_s"]               # noqa: E731
    said = lambda flag: "holds" if flag else "DOES NOT HOLD"   # noqa: E731
    lines = ["# Batch mixing: mix_clips against torch, the soft-target loss, and the headline step", "",
             "Written by `tools/bench_mix.py` on %s; `bench.json` beside this file holds every figure. A warm-up, then the "
             "median of %d alternating windows with the fastest and the slowest window in brackets. Sources: csrc_mix %s, "
             "csrc %s." % (res["device"], res["rounds"], res["csrc_mix_sha16"], res["csrc_sha16"]), "",
             "The kernels (gfx950, from the compiler's resource-usage remarks):", "",
             "| kernel | VGPRs | SGPRs | scratch bytes per lane | LDS bytes | waves per SIMD |", "|---|---|---|---|---|---|"]
    for name in sorted(res["resources"]):
        rs = res["resources"][name]
        lines.append("| `%s` | %d | %d | %d | %d | %d |" % (name, rs["vgprs"], rs["sgprs"], rs["scratch_bytes_per_lane"],
                                                         rs["lds_bytes"], rs["occupancy_waves_per_simd"]))
    lines += ["", "The expectation, written down before anything was measured: " + res["expectation"], "",
              "## (a) The headline batch (%d clips of 3 x %d x %d x %d floats, %.1f MB), us per call" % (
                  res["shape"][0], res["shape"][1], res["shape"][2], res["shape"][2], cl["clip_bytes"] / 1e6), "",
              "Between two device events, %d calls per window, one process, every output into the same tensor. Mixup: lam %g, "
              "the partner the sample before. CutMix: the same partners, the box rows %d..%d, columns %d..%d (%.1f %% of the "
              "plane). `mix_clips` on the CutMix plan was first checked to give the bits of the torch assignment, on the mixup "
              "plan to agree with the torch expression within 1e-6 of the largest element (torch rounds both products, the "
              "kernel one product and a fused multiply-add). Bytes/s from the bytes the rule has to move: read one and write "
              "one for a copy, read two and write one for mixup, the box's share of a third pass for CutMix."
              % (cl["calls_per_window"], res["lam"], res["box"][0], res["box"][1], res["box"][2], res["box"][3],
                 100 * cl["box_share"]), "",
              "| path | us per call | TB/s |", "|---|---|---|",
              "| `out.copy_(x)` | %s | %s |" % (row("copy_"), tb("copy_")),
              "| `mix_clips`, the identity plan | %s | %s |" % (row("mix_clips_identity"), tb("mix_clips_identity")),
              "| `mix_clips`, mixup | %s | %s |" % (row("mix_clips_mixup"), tb("mix_clips_mixup")),
              "| torch: `x * lam + x[perm] * (1 - lam)` | %s | |" % row("torch_mixup"),
              "| `mix_clips`, CutMix | %s | %s |" % (row("mix_clips_cutmix"), tb("mix_clips_cutmix")),
              "| torch: `o = x.clone(); o[..., box] = x[perm][..., box]` | %s | |" % row("torch_cutmix"), "",
              "The bar -- the mixing launch's slowest window is not slower than the fastest window of the torch code it "
              "replaces -- %s for mixup (%.1f x by the medians) and %s for CutMix (%.1f x)."
              % (said(cl["mixup_not_slower_than_torch"]), cl["torch_mixup"]["us_per_call"] / cl["mix_clips_mixup"]["us_per_call"],
                 said(cl["cutmix_not_slower_than_torch"]),
                 cl["torch_cutmix"]["us_per_call"] / cl["mix_clips_cutmix"]["us_per_call"]), "",
              "## (b) Targets and loss on [%d, %d], us per call" % (res["shape"][0], NC), "",
              "%d calls per window. Ours: `mix_targets` and `soft_ce` (three launches). Torch: `one_hot`, the smoothing, the "
              "mix of the two label sets, `F.cross_entropy` on probabilities and its gradient by autograd. The two were first "
              "checked to agree within 2e-6." % lo["calls_per_window"], "",
              "| path | us per call |", "|---|---|",
              "| `mix_targets` + `soft_ce` | %s |" % _row(lo["mix_targets_soft_ce"], "us_per_call", "%.1f"),
              "| torch | %s |" % _row(lo["torch_one_hot_smooth_cross_entropy"], "us_per_call", "%.1f"), "",
              "`soft_ce` on exact one-hot targets against `x3d_head_ce` on the labels (recorded, not required: the compiler may "
              "contract the two gradient expressions differently, and `soft_ce` divides where `x3d_head_ce` multiplies by a "
              "reciprocal): the loss has %s, the gradient has %s (largest difference %.3g)."
              % ("the same bits" if lo["one_hot_loss_bits_equal_head_ce"] else "NOT the same bits",
                 "the same bits" if lo["one_hot_gradient_bits_equal_head_ce"] else "NOT the same bits",
                 lo["one_hot_gradient_max_abs_difference"]), "",
              "## (c) The headline step (X3D-M, B %d, T %d, %d x %d, use_graph), ms per step" % (
                  res["shape"][0], res["shape"][1], res["shape"][2], res["shape"][2]), "",
              "Two Trainers in one process, %d steps and a synchronise per window, host clock. The mixed step is what "
              "`--mixup %g --cutmix %g --label-smoothing %g` runs: the plan drawn on the host, its upload, `mix_clips` and "
              "`mix_targets` into the graph's static inputs, then the replay with `objective=\"soft_ce\"`. The step without "
              "keeps its clips resident in the static inputs, so the mixed step is also charged the pass over the batch that "
              "any input pipeline pays. (The expectation above had the step's length wrong: it is %.1f ms, not 23.)"
              % (res["steps_per_window"], res["mixup"], res["cutmix"], res["smoothing"], st["off"]["ms_per_step"]), "",
              "| Trainer | ms per step | the cost by the medians |", "|---|---|---|",
              "| defaults | %s | |" % _row(st["off"], "ms_per_step", "%.3f"),
              "| mixup, CutMix and smoothing | %s | %+.1f us |" % (_row(st["mixup_cutmix_smoothing"], "ms_per_step", "%.3f"),
                                                                  st["mixup_cutmix_smoothing"]["cost_us_by_medians"]), "",
              "## (d) The defaults against the parent commit", "",
              "The default path has no new launch: `objective=\"ce\"` calls `ops.head_ce` as before and nothing under `csrc/` "
              "changed.", ""]
    lines += _bench_lines(res.get("bench_py"), res["shape"][0])
    lines += ["Nothing here is a share of any peak: these are achieved times and rates of one process on one GPU.", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    main()
