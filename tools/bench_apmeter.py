"""Timing of the device-resident APMeter (csrc_eval/apmeter.hip): one JSON line.

    python tools/bench_apmeter.py [--out FILE]

Every measurement runs in a child process of its own under `timeout -k 10` (a step that hangs ends there and the line
records it), timed with device events after warm-up:
  add_frames_us   APMeter.add_frames per call at the loc training shape (B 32, K 157, T 32, TL 160)
  add_logits_us   APMeter.add_logits per call at cls val (b 16, n_crops 10, K 157)
  value_630k_ms   value_device() at N = 630 000, K = 157
  value_1850_ms   value_device() at N = 1850, K = 157
  cpu_*_ms        the same AP on the same data by a CPU torch restatement (stable sort + cumsums per class)
`--step NAME` runs one step in-process (what the children run; also the target of a rocprofv3 trace)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "x3d-multigrid_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

STEPS = {"add_frames": 120, "add_logits": 120, "value_1850": 120, "value_630k": 300}


def _events(fn, warm, reps):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps                       # ms per call


def _filled(N, K, seed):
    import torch
    from apmeter import APMeter
    g = torch.Generator(device="cuda").manual_seed(seed)
    m = APMeter()
    s = torch.sigmoid(torch.randn((N, K), device="cuda", generator=g) * 2)
    y = (torch.rand((N, K), device="cuda", generator=g) < 0.05).float()
    m.add(s, y)
    return m, s, y


def _cpu_ap(s, y):
    """CPU restatement: per class a stable descending sort, then the unweighted AP (torch on the host)."""
    import torch
    s, y = s.cpu(), y.cpu()
    N = s.shape[0]
    rank = torch.arange(1, N + 1, dtype=torch.float64)
    t0 = time.perf_counter()
    ap = torch.zeros(s.shape[1], dtype=torch.float64)
    for k in range(s.shape[1]):
        order = torch.sort(s[:, k], descending=True, stable=True)[1]
        truth = y[order, k].double()
        tp = truth.cumsum(0)
        ap[k] = (tp / rank)[truth == 1].sum() / max(float(truth.sum()), 1.0)
    return (time.perf_counter() - t0) * 1e3, ap


def run_step(name):
    import torch
    from apmeter import APMeter
    torch.cuda.set_device(0)
    K = 157
    if name == "add_frames":
        B, T, TL = 32, 32, 160
        g = torch.Generator(device="cuda").manual_seed(1)
        z = torch.randn((B, K, T), device="cuda", generator=g)
        y = (torch.rand((B, K, TL), device="cuda", generator=g) < 0.05).float()
        masks = (torch.arange(TL, device="cuda")[None, :] < torch.randint(40, TL + 1, (B, 1), device="cuda")).float()
        m = APMeter()
        m.add_frames(z, y, masks)
        m.reserve(130 * B * TL)
        return {"add_frames_us": 1e3 * _events(lambda: m.add_frames(z, y, masks), 20, 100)}
    if name == "add_logits":
        b, n = 16, 10
        g = torch.Generator(device="cuda").manual_seed(2)
        z = torch.randn((b * n, K, 1), device="cuda", generator=g)
        y = (torch.rand((b, K), device="cuda", generator=g) < 0.05).float()
        m = APMeter()
        m.add_logits(z, y, n_crops=n)
        m.reserve(130 * b)
        return {"add_logits_us": 1e3 * _events(lambda: m.add_logits(z, y, n_crops=n), 20, 100)}
    N = {"value_1850": 1850, "value_630k": 630000}[name]
    m, s, y = _filled(N, K, 3)
    ms = _events(m.value_device, 2, 5 if N > 10000 else 50)
    cpu_ms, cpu_ap = _cpu_ap(s, y)
    gpu_ap = m.value().double()
    return {name + "_ms": ms, "cpu_" + name + "_ms": cpu_ms, name + "_max_abs_diff_vs_cpu": float((gpu_ap - cpu_ap).abs().max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if args.step:
        print("STEP " + json.dumps(run_step(args.step)))
        return
    from tools import stamp
    res = {"metric": "apmeter", "csrc_eval_sha16": stamp.csrc_eval_sha16(), "commit": stamp.commit(),
           "targets": {"value_630k_ms": 25.0, "value_1850_ms": 1.0, "add_frames_us": 20.0}}
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
