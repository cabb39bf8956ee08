"""Timing of the Charades input path (csrc_data/ through charades.Charades).  One JSON line, also written to `--out` when given.

    python tools/bench_charades_input.py [--out FILE] [--rounds N] [--window SECONDS]

One process; each shape is warmed up, then timed in windows of at least `--window` seconds between two device events, host
work included (the job tables are built on the host).  Reported: the median over the rounds, the minimum and the maximum
(the run-to-run spread).
  train        B 32, 16 frames at stride 10, 224 x 224 from 256 x 340 frames, task 'loc' labels [32, 157, 160] + masks
  test_loc     B 16 whole videos at stride 10 (lengths: the fixture durations at 24 fps), zero-padded, labels + masks
  labels_kernel   x3ddata_charades_labels alone at the training shape, into preallocated outputs: bytes written / time,
                  as achieved bandwidth (not a share of any peak)
profiles/charades_input/ holds a run that also timed the same batches put together from what the tree offered before
this path (ClipPreprocessor on clip kernels of its own, dense host label arrays); that composition no longer exists."""
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

H, W, S, K = 256, 340, 224, 157


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
    return {"new_ms": statistics.median(v), "new_min_ms": min(v), "new_max_ms": max(v), "spread_ms": max(v) - min(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)      # profiles/charades_input/bench.json is a record: not overwritten by default
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0)
    args = ap.parse_args()
    import numpy as np
    import torch
    import charades
    from tools import stamp
    from x3dhip import dataops
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    with open(os.path.join(ROOT, "tests", "golden", "charades_anno.json")) as f:
        anno = json.load(f)
    g = torch.Generator(device=dev).manual_seed(0)
    videos = {v: torch.randint(0, 256, (int(round(24 * r["duration"])), H, W, 3), dtype=torch.uint8, device=dev, generator=g)
              for v, r in anno.items()}
    kw = dict(frames=80, gamma_tau=5, crop_size=S, c_size=S, task="loc")
    train = charades.Charades(anno, "training", videos, rng=random.Random(0), **kw)
    test = charades.Charades(anno, "testing", videos, crops=10, **kw)
    pick = random.Random(1)
    tr_idx = [pick.randrange(len(train)) for _ in range(32)]
    te_idx = [pick.randrange(len(test)) for _ in range(16)]
    params = [train.draw(i) for i in tr_idx]

    def train_new():
        return train.batch(tr_idx, params)

    def test_new():
        return test.test_batch(te_idx)

    res = {"metric": "charades_input", "csrc_data_sha16": stamp.csrc_data_sha16(), "commit": stamp.commit(),
           "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_s": args.window,
           "train": _timed(train_new, args.rounds, args.window),
           "test_loc": _timed(test_new, args.rounds, args.window)}
    res["test_loc"]["lengths"] = [test.data[i][2] for i in te_idx]

    jobs = [(i, p["start_f"] - 1, 160) for i, p in zip(tr_idx, params)]
    outs = [torch.empty(s, dtype=torch.float32, device=dev) for s in ((32, K, 160), (32, 160), (32, K))]
    tab = np.zeros(32, dtype=dataops.LABEL_JOB_DT)
    tab["video"], tab["start"], tab["n"] = [j[0] for j in jobs], [j[1] for j in jobs], [j[2] for j in jobs]
    jd = torch.from_numpy(tab.view(np.uint8)).to(dev)
    L = dataops._datalib.lib()
    t = train.table

    def kernel():
        dataops.check(L.x3ddata_charades_labels(t.off.data_ptr(), t.cls.data_ptr(), t.lo.data_ptr(), t.hi.data_ptr(), t.V,
                                                jd.data_ptr(), 32, K, 160, outs[0].data_ptr(), outs[1].data_ptr(),
                                                outs[2].data_ptr(), dataops.stream()))
    for _ in range(20):
        kernel()
    us = [1e3 * _window(kernel, args.window) for _ in range(args.rounds)]
    written = sum(o.numel() * 4 for o in outs)
    res["labels_kernel"] = {"us": statistics.median(us), "min_us": min(us), "max_us": max(us), "bytes_written": written,
                            "achieved_GBps": written / (statistics.median(us) * 1e-6) / 1e9,
                            "note": "launch included (back-to-back launches on one stream); bytes written / time"}
    out = json.dumps(res, sort_keys=True)
    print(out)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
