"""Timing of the Charades input path (csrc_data/ through charades.Charades) against the same batches put together from
what the tree offered before it: ClipPreprocessor once per sample plus torch copies into the padded batch, and dense host
label arrays sliced, padded and uploaded.  One JSON line, also written to profiles/charades_input/bench.json.

    python tools/bench_charades_input.py [--out FILE] [--rounds N] [--window SECONDS]

One process; per shape both versions are warmed up, then timed alternately (new, old, new, old, ...) in windows of at
least `--window` seconds between two device events, host work included (the job tables are built on the host in every
version).  The training shape has a third version, `old_batched`: the earlier ClipPreprocessor called once for the whole
batch, which it can take because all samples share T and the output size.  Reported per version: the median over the
rounds, the minimum and the maximum (the run-to-run spread).
  train        B 32, 16 frames at stride 10, 224 x 224 from 256 x 340 frames, task 'loc' labels [32, 157, 160] + masks
  test_loc     B 16 whole videos at stride 10 (lengths: the fixture durations at 24 fps), zero-padded, labels + masks
  labels_kernel   x3ddata_charades_labels alone at the training shape, into preallocated outputs: bytes written / time,
                  as achieved bandwidth (not a share of any peak)
Both versions are checked to give the same bits before anything is timed."""
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


def _alternate(versions, rounds, seconds):
    """versions: {name: fn}, "new" and "old" among them; timed in turn, round after round."""
    for fn in versions.values():
        for _ in range(5):
            fn()
    res = {k: [] for k in versions}
    for _ in range(rounds):
        for k, fn in versions.items():
            res[k].append(_window(fn, seconds))
    out = {}
    for k, v in res.items():
        out[k + "_ms"] = statistics.median(v)
        out[k + "_min_ms"], out[k + "_max_ms"] = min(v), max(v)
    spread = max(out[k + "_max_ms"] - out[k + "_min_ms"] for k in versions)
    out["spread_ms"] = spread
    for k in versions:
        if k != "new":
            out["new_not_slower_than_%s_beyond_spread" % k] = out["new_ms"] <= out[k + "_ms"] + spread
    return out


def _dense(ds):
    """What the reference keeps on the host: a dense float [157, n_frames] array per video (charades.py:91-97), here
    filled from the dataset's frame ranges."""
    import numpy as np
    off, cls, lo, hi = ds.table.host
    out = []
    for v, (_, _, nf) in enumerate(ds.data):
        lab = np.zeros((K, nf), np.float32)
        for a in range(off[v], off[v + 1]):
            lab[cls[a], lo[a]:hi[a]] = 1
        out.append(lab)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "charades_input", "bench.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0)
    args = ap.parse_args()
    import numpy as np
    import torch
    import charades
    from tools import stamp
    from x3dhip import dataops
    from x3dhip.clip_input import ClipPreprocessor, center_crop_box
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
    pre = ClipPreprocessor(dev, charades.CHARADES_MEAN, charades.CHARADES_STD)
    tr_dense, te_dense = _dense(train), _dense(test)
    pick = random.Random(1)
    tr_idx = [pick.randrange(len(train)) for _ in range(32)]
    te_idx = [pick.randrange(len(test)) for _ in range(16)]
    params = [train.draw(i) for i in tr_idx]

    def train_new():
        return train.batch(tr_idx, params)

    def train_old():
        batch = torch.empty((32, 3, 16, S, S), dtype=torch.float32, device=dev)
        labels = np.empty((32, K, 160), np.float32)
        for b, (i, p) in enumerate(zip(tr_idx, params)):
            first = p["start_f"] - 1
            q = dict(frame_idx=list(range(first, first + 160, 10)), x1=p["x1"], y1=p["y1"], crop=p["crop"], out=S,
                     flip=p["flip"])
            pre([(train.videos[i], q)], out=batch[b:b + 1])
            labels[b] = tr_dense[i][:, first:first + 160]
        return batch, torch.from_numpy(labels).to(dev), torch.ones((32, 160), dtype=torch.float32, device=dev)

    def train_old_batched():
        """The fairer baseline: all 32 samples share T and the output size, so the earlier ClipPreprocessor takes them in
        one call (still two allocations per sample inside it); labels as in train_old."""
        samples, labels = [], np.empty((32, K, 160), np.float32)
        for b, (i, p) in enumerate(zip(tr_idx, params)):
            first = p["start_f"] - 1
            samples.append((train.videos[i], dict(frame_idx=list(range(first, first + 160, 10)), x1=p["x1"], y1=p["y1"],
                                                  crop=p["crop"], out=S, flip=p["flip"])))
            labels[b] = tr_dense[i][:, first:first + 160]
        return pre(samples), torch.from_numpy(labels).to(dev), torch.ones((32, 160), dtype=torch.float32, device=dev)

    def test_new():
        return test.test_batch(te_idx)

    def test_old():
        nfs = [test.data[i][2] for i in te_idx]
        tmax, lmax = max(len(range(0, n, 10)) for n in nfs), max(nfs)
        batch = torch.zeros((16, 3, tmax, S, S), dtype=torch.float32, device=dev)
        labels = np.zeros((16, K, lmax), np.float32)
        masks = np.zeros((16, lmax), np.float32)
        for b, (i, n) in enumerate(zip(te_idx, nfs)):
            x1, y1, crop = center_crop_box(W, H)
            q = dict(frame_idx=list(range(0, n, 10)), x1=x1, y1=y1, crop=crop, out=S, flip=False)
            batch[b, :, :len(q["frame_idx"])] = pre([(test.videos[i], q)])[0]
            labels[b, :, :n] = te_dense[i]
            masks[b, :n] = 1
        return batch, torch.from_numpy(labels).to(dev), torch.from_numpy(masks).to(dev)

    for new, old in ((train_new, train_old), (train_new, train_old_batched), (test_new, test_old)):   # the same bits first
        for x, y in zip(new(), old()):
            assert torch.equal(x, y), (new.__name__, x.shape)
    res = {"metric": "charades_input", "csrc_data_sha16": stamp.csrc_data_sha16(), "commit": stamp.commit(),
           "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_s": args.window,
           "train": _alternate({"new": train_new, "old": train_old, "old_batched": train_old_batched}, args.rounds,
                               args.window),
           "test_loc": _alternate({"new": test_new, "old": test_old}, args.rounds, args.window)}
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
