"""Timing of the AP meter's segment marks and merge (csrc_eval/apmerge.hip): one JSON line.

    python tools/bench_apmeter_merge.py [--out FILE]

The size is the localisation validation's of profiles/apmeter/ -- 630 000 rows x 157 classes -- split into 8 shards whose
adds hold 300..1200 rows each (a batch of 16 videos of 20..75 labelled frames).  Every step runs in a child process of its
own under `timeout -k 10`; every figure is the median (with min and max) over WINDOWS windows of device-event time per
call, after warm-up:
  mark_us            x3deval_ap_mark per call (evalops.ap_mark: host check, one ctypes launch of one thread)
  merge_ms           x3deval_ap_merge on the stacked buffers: the plan and the copy kernel together
  merge_shards_ms    apmeter.merge_shards end to end: padding to the largest capacity, stacking, the two kernels
  clone_ms           clone() of an fp32 [157, N] and a uint8 [157, N] tensor: the same bytes moved, contiguous
  index_select_ms    the obvious alternative: a row permutation built on the host from the marks, then
                     torch.index_select along the row axis of the stacked buffers laid out [K, W * C] (the relayout that
                     needs is timed apart, index_select_relayout_ms)
  value_ms           value_device() of the merged meter
  gather_1rank_ms    apmeter.gather over a one-rank RCCL group (backend "nccl") of one rank's share, N / 8 rows: the bound
                     all-reduce with its read-back, five one-rank all-gathers and the merge -- what a one-GPU box can
                     time; the 8-rank all-gather over xGMI is not measured
`--step NAME` runs one step in-process (what the children run; `--step merge_kernels` is the target of a
rocprofv3 --kernel-trace --stats run that splits merge_ms into its two kernels)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "x3d-multigrid_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

STEPS = {"mark": 120, "merge": 400, "gather": 200}
WINDOWS = 7
N, K, W = 630000, 157, 8


def _windows(fn, warm, reps):
    """{"median", "min", "max"} of the per-call device time in ms over WINDOWS windows of `reps` calls."""
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(WINDOWS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / reps)
    times.sort()
    return {"median": times[len(times) // 2], "min": times[0], "max": times[-1]}


def _scaled(d, f):
    return {k: v * f for k, v in d.items()}


def _shards(count=W):
    """`count` segment-tracking meters of N / W rows each, and the segment lengths of each."""
    import numpy as np
    import torch
    from apmeter import APMeter
    rng = np.random.default_rng(5)
    g = torch.Generator(device="cuda").manual_seed(5)
    shards, lengths = [], []
    for r in range(count):
        m, mine, left = APMeter(track_segments=True), [], N // W
        while left > 0:
            n = min(left, int(rng.integers(300, 1201)))
            s = torch.sigmoid(torch.randn((n, K), device="cuda", generator=g) * 2)
            y = (torch.rand((n, K), device="cuda", generator=g) < 0.05).float()
            m.add(s, y)
            mine.append(n)
            left -= n
        shards.append(m)
        lengths.append(mine)
    return shards, lengths


def run_step(name):
    import torch
    import apmeter
    from x3dhip import evalops
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    if name == "mark":
        state = evalops.ap_state(dev, 1024)
        marks = evalops.ap_marks(dev, 1 << 20)               # room for every call below
        return {"mark_us": _scaled(_windows(lambda: evalops.ap_mark(state, marks), 50, 2000), 1e3)}
    if name == "gather":
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29644")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
        try:
            (m,), _ = _shards(1)
            res = {"gather_1rank_ms": _windows(lambda: apmeter.gather(m, dist.group.WORLD), 2, 5),
                   "gather_1rank_rows": apmeter.gather(m, dist.group.WORLD)._rows()}
        finally:
            dist.destroy_process_group()
        return res
    from tests import apmerge_ref
    shards, lengths = _shards()
    cap, nmarks = max(m._cap for m in shards), max(m._mcap for m in shards)
    parts = [apmeter._padded(m, K, False, cap, nmarks, dev) for m in shards]
    states, marks, scores, targets = [torch.stack([p[i] for p in parts]) for i in range(4)]
    dst = apmeter._merged(states, marks, scores, targets, None, N)
    ws = torch.empty(evalops.ap_merge_workspace_bytes(W, nmarks), dtype=torch.uint8, device=dev)

    def merge():
        evalops.ap_merge(states, marks, scores, targets, None, dst._state, dst._scores, dst._targets, None, ws)
    if name == "merge_kernels":
        _windows(merge, 2, 5)
        return {"segments": sum(len(l) for l in lengths)}
    res = {"rows": N, "classes": K, "shards": W, "segments": sum(len(l) for l in lengths), "shard_capacity": cap,
           "marks_per_shard": nmarks}
    res["merge_ms"] = _windows(merge, 2, 5)
    res["merge_shards_ms"] = _windows(lambda: apmeter.merge_shards(shards), 1, 3)
    a, b = dst._scores[:, :N].contiguous(), dst._targets[:, :N].contiguous()
    res["clone_ms"] = _windows(lambda: (a.clone(), b.clone()), 2, 5)
    res["bytes_read_and_written"] = 2 * (a.numel() * 4 + b.numel())
    idx = torch.from_numpy(apmerge_ref.gather_index(lengths, cap)).to(dev)
    flat_s = scores.permute(1, 0, 2).reshape(K, W * cap)
    flat_t = targets.permute(1, 0, 2).reshape(K, W * cap)
    res["index_select_ms"] = _windows(lambda: (flat_s.index_select(1, idx), flat_t.index_select(1, idx)), 2, 5)
    res["index_select_relayout_ms"] = _windows(
        lambda: (scores.permute(1, 0, 2).reshape(K, W * cap), targets.permute(1, 0, 2).reshape(K, W * cap)), 2, 5)
    merged = apmeter.merge_shards(shards)
    res["value_ms"] = _windows(merged.value_device, 2, 5)
    same = torch.equal(flat_s.index_select(1, idx).view(torch.int32), merged._scores[:, :N].view(torch.int32)) and \
        torch.equal(flat_t.index_select(1, idx), merged._targets[:, :N])
    res["merged_equals_index_select"] = bool(same) and merged._rows() == N
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS) + ["merge_kernels"])
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if args.step:
        print("STEP " + json.dumps(run_step(args.step)))
        return
    from tools import stamp
    res = {"metric": "apmeter_merge", "csrc_eval_sha16": stamp.csrc_eval_sha16(), "commit": stamp.commit(),
           "windows": WINDOWS}
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
