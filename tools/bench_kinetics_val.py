"""Timing of the Kinetics validation phase and of the top-k meter's kernels (csrc_eval/topk.hip): one JSON line.

    python tools/bench_kinetics_val.py [--out FILE]

Every measurement runs in a child process of its own under `timeout -k 10` (a step that hangs ends there and the line
records it).  After warm-up each figure is the median of WINDOWS windows, with the minimum and the maximum:
  kernels   x3deval_cls_append_crops and x3deval_cls_value through x3dhip.evalops at b*n x K = 24 x 400 and 384 x 400
            (n = 3 crops), device events around CALLS calls per window: microseconds per call, launch cost included.
            value() runs over the CALLS * b rows of one window.
  phase     X3D-M in eval mode on BATCHES synthetic batches of [8, 3, 3, 16, 224, 224] per window, through
            train_x3d_kinetics_multigrid.validate (three float() reads per batch) and through validate_topk (the meter; one
            read at the end), alternating window by window; wall time of a window, host reads included: ms per batch
`--step NAME` runs one step in-process (what the children run)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "x3d-multigrid_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

STEPS = {"kernels": 120, "phase": 300}
WINDOWS = 9
CALLS = 200
BATCHES = 6


def _stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "windows": len(xs)}


def _window_us(fn, before):
    import torch
    before()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / CALLS


def run_kernels():
    import torch
    from x3dhip import evalops
    dev = torch.device("cuda", 0)
    K, n = 400, 3
    out = {}
    for b in (8, 128):
        g = torch.Generator(device="cuda").manual_seed(b)
        z = torch.randn((b * n, K), device=dev, generator=g) * 2
        y = torch.randint(0, K, (b,), device=dev, generator=g)
        cap = CALLS * b
        state, rows = evalops.ap_state(dev, cap), evalops.cls_rows(dev, cap)
        reset = lambda: evalops.ap_reset(state, cap)                                   # noqa: E731
        append = lambda: evalops.cls_append_crops(state, rows, z, y, n)                # noqa: E731
        value = lambda: evalops.cls_value(state, rows, K, 5)                           # noqa: E731
        _window_us(append, reset)
        name = "%dx%d" % (b * n, K)
        out["append_%s_us" % name] = _stats([_window_us(append, reset) for _ in range(WINDOWS)])
        t = value()[0].cpu()
        assert int(t[0]) == cap and int(t[3]) == CALLS, t
        out["value_%s_rows%d_us" % (name, cap)] = _stats([_window_us(value, lambda: None) for _ in range(WINDOWS)])
    return out


def run_phase():
    import torch
    import x3d as resnet_x3d
    import train_x3d_kinetics_multigrid as tk
    from kinetics_multigrid import device_batch
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    b, n, T, H = 8, 3, 16, 224
    model = resnet_x3d.generate_model(x3d_version="M", n_classes=400, n_input_channels=3, dropout=0.5, base_bn_splits=1)
    model.to(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    batches = []
    for _ in range(BATCHES):
        x, y = device_batch(b * n, T, H, 400, dev, gen)
        batches.append((x.view(b, n, 3, T, H, H), y.view(-1)[:b].contiguous()))

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn(model, batches)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / BATCHES, res

    window(tk.validate)
    window(tk.validate_topk)
    old, new = [], []
    for _ in range(WINDOWS):
        ms, (loss, acc, seen) = window(tk.validate)
        old.append(ms)
        ms, res = window(tk.validate_topk)
        new.append(ms)
    assert res["videos"] == seen, (res, seen)
    return {"validate_ms_per_batch": _stats(old), "validate_topk_ms_per_batch": _stats(new),
            "phase_shape": [b, n, 3, T, H, H], "batches_per_window": BATCHES,
            "cls_loss_validate": loss, "cls_loss_validate_topk": res["cls_loss"], "top1_validate": acc,
            "top1_validate_topk": res["top1"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if args.step:
        print("STEP " + json.dumps({"kernels": run_kernels, "phase": run_phase}[args.step]()))
        return
    from tools import stamp
    res = {"metric": "kinetics_val", "csrc_eval_sha16": stamp.csrc_eval_sha16(), "csrc_sha16": stamp.csrc_sha16(),
           "commit": stamp.commit(), "calls_per_window": CALLS}
    for step, limit in STEPS.items():
        p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step],
                           capture_output=True, text=True, stdin=subprocess.DEVNULL)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("STEP ")]
        if p.returncode != 0 or not line:
            res[step + "_error"] = "exit %d: %s" % (p.returncode, (p.stderr or p.stdout)[-400:])
            break                                           # nothing more on the GPU after a failed step
        res.update(json.loads(line[-1][5:]))
    out = json.dumps(res, sort_keys=True)
    print(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
