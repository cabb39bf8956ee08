"""Timing of the Kinetics clip input path through kinetics_multigrid.DeviceVideoKinetics alone (batch and val_batch), so
that the same file runs unchanged in a checkout of another commit.  One JSON line, also written to `--out` when given.

    python tools/bench_clip_input.py [--out FILE] [--rounds N] [--window SECONDS]

One process; each shape is warmed up, then timed in windows of at least `--window` seconds between two device events, host
work included (the random draws and the job tables are made on the host).  Reported: the median over the rounds, the
minimum and the maximum (the run-to-run spread).
  train   batch of B 8, T 16, 224 x 224 from 256 x 340 uint8 videos of 120 frames, into a preallocated `out=`
  val     val_batch of the same 8 videos, 3 temporal windows each: [8, 3, 3, 16, 224, 224]"""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "x3d-multigrid_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

B, N_FRAMES, H, W = 8, 120, 256, 340


def _window(fn, seconds):
    """ms per call over a window of at least `seconds` between two device events."""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps, total = 0, 0.0
    chunk = 4
    while total < seconds * 1e3:
        a.record()
        for _ in range(chunk):
            fn()
        b.record()
        torch.cuda.synchronize()
        total += a.elapsed_time(b)
        reps += chunk
        chunk = min(chunk * 2, 256)
    return total / reps


def _timed(fn, rounds, seconds):
    for _ in range(5):
        fn()
    v = [_window(fn, seconds) for _ in range(rounds)]
    return {"ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "spread_ms": max(v) - min(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0)
    args = ap.parse_args()
    import torch
    from kinetics_multigrid import DeviceVideoKinetics
    from tools import stamp
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    vids = [torch.randint(0, 256, (N_FRAMES, H, W, 3), dtype=torch.uint8, device=dev, generator=g) for _ in range(B)]
    ds = DeviceVideoKinetics(vids, list(range(B)), rng=random.Random(0))
    idx = list(range(B))
    out = torch.empty((B, 3, 16, 224, 224), dtype=torch.float32, device=dev)

    def train():
        return ds.batch(idx, 2, 3, out=out)          # iteration 2 of long-cycle state 3: the base shape, 16 x 224^2

    def val():
        return ds.val_batch(idx, crops=3)

    assert tuple(train()[0].shape) == (B, 3, 16, 224, 224) and tuple(val()[0].shape) == (B, 3, 3, 16, 224, 224)
    res = {"metric": "clip_input", "csrc_sha16": stamp.csrc_sha16(), "csrc_data_sha16": stamp.csrc_data_sha16(),
           "commit": stamp.commit(), "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "window_s": args.window, "train": _timed(train, args.rounds, args.window),
           "val": _timed(val, args.rounds, args.window)}
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
