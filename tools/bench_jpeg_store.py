"""Timing of the frame store (x3dhip.jpegstore.FrameStore over csrc_jpeg/store.hip) against the device path it is built
on, by the protocol of profiles/jpeg_entropy/: the same 16 frames of 256 x 340 4:2:0 quality 75 repeated to 256
(tools/bench_jpeg_decode.py makes them), a torch.equal check against the host path before any timing, a warm-up, then the
median of `--rounds` alternating windows with minimum and maximum.  One JSON line, also written to
profiles/jpeg_store/bench.json, and profiles/jpeg_store/README.md from the same figures.

    python tools/bench_jpeg_store.py [--out DIR] [--rounds N] [--window S]

  add            FrameStore.add of the 256 frames into a fresh store (+ synchronise), frames/s at 1 and 2 threads
  decode         decode_into + synchronise for 128 and 256 frames, three ways, alternating window by window: the store;
                 JpegDecoder(entropy="device", threads=2) from bytes in memory; the same decoder from files on disk
                 through FrameFolder.read
  build_kernels  x3djpeg_store_build_jobs alone (its two launches) between two device events, us per batch
  resident       bytes per frame in the store (arena in use; tables; chunks as allocated) against the file and the decoded
                 frame
  replay         a captured plan(n, W, H).launch() replayed + synchronise against the same launch() made eagerly
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "x3d-multigrid_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

from tools import bench_jpeg_decode as bj  # noqa: E402

H, W = bj.H, bj.W


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_store"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window")
    args = ap.parse_args()
    import torch
    import frames as frames_mod
    from tools import stamp
    from x3dhip import _jpeglib, jpegops, jpegstore
    from x3dhip._lib import stream
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    distinct, encoder = bj.make_frames(args.distinct)
    files = [distinct[i % len(distinct)] for i in range(args.batch)]
    n = len(files)

    # the same bits first
    want = jpegops.JpegDecoder(dev, threads=16).decode(distinct)
    store = jpegstore.FrameStore(dev, threads=2)
    ids = store.add(files)
    for k, o in enumerate(store.decode(list(ids))):
        assert torch.equal(o, want[k % len(distinct)]), k
    res = {"metric": "jpeg_store", "csrc_jpeg_sha16": stamp.csrc_jpeg_sha16(), "csrc_sha16": stamp.csrc_sha16(),
           "commit": stamp.commit(), "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_s": args.window,
           "batch": n, "frame": [H, W], "subsampling": "4:2:0", "quality": 75, "encoder": encoder,
           "sub_bits": store.sub_bits, "mean_file_bytes": sum(len(d) for d in distinct) / len(distinct),
           "checked_against": "JpegDecoder(entropy='host'), torch.equal on every frame of the batch"}

    # (a) add
    res["add"] = {}
    for th in (1, 2):
        def add(th=th):
            s = jpegstore.FrameStore(dev, threads=th)
            s.add(files)
            torch.cuda.synchronize()
        add()
        v = [bj._rate(add, n, args.window) for _ in range(args.rounds)]
        res["add"]["threads_%d" % th] = bj._stats(v, "frames_per_s")

    # (b) decode_into, three ways, alternating
    tmp = tempfile.mkdtemp(prefix="jpeg_store_bench_")
    for i, d in enumerate(files):
        with open(os.path.join(tmp, frames_mod.FRAME_NAME.format(i + 1)), "wb") as f:
            f.write(d)
    folder = frames_mod.FrameFolder(tmp)
    dec = jpegops.JpegDecoder(dev, threads=2, entropy="device")
    res["decode"] = {}
    for m in sorted({n // 2, n}):
        dst = torch.empty((m, H, W, 3), dtype=torch.uint8, device=dev)
        idl, sub, rng = np.arange(m), files[:m], range(m)

        def from_store():
            store.decode_into(idl, dst)
            torch.cuda.synchronize()

        def from_memory():
            dec.decode_into(sub, dst)
            torch.cuda.synchronize()

        def from_files():
            dec.decode_into(folder.read(rng), dst)
            torch.cuda.synchronize()

        versions = {"store": from_store, "device_path_memory": from_memory, "device_path_files": from_files}
        for fn in versions.values():
            for _ in range(3):
                fn()
            assert torch.equal(dst[:len(distinct)], torch.stack(want)[:m])
        rates = {k: [] for k in versions}
        for _ in range(args.rounds):
            for k, fn in versions.items():
                rates[k].append(bj._rate(fn, m, args.window))
        r = {k: bj._stats(v, "frames_per_s") for k, v in rates.items()}
        s, mem, fil = r["store"], r["device_path_memory"], r["device_path_files"]
        r["store_over_memory_median"] = s["frames_per_s"] / mem["frames_per_s"]
        r["store_slowest_over_files_fastest"] = s["frames_per_s_min"] / fil["frames_per_s_max"]
        r["store_over_files_median"] = s["frames_per_s"] / fil["frames_per_s"]
        r["bar_median_not_below_memory"] = s["frames_per_s"] >= mem["frames_per_s"]
        r["bar_slowest_above_files_fastest"] = s["frames_per_s_min"] > fil["frames_per_s_max"]
        res["decode"]["frames_%d" % m] = r
    for name in os.listdir(tmp):
        os.remove(os.path.join(tmp, name))
    os.rmdir(tmp)

    # (c) the two build kernels alone, (e) a captured plan against eager
    L = _jpeglib.lib()
    res["build_kernels"], res["replay"] = {}, {}
    for m in sorted({n // 2, n}):
        b = store.plan(m, W, H)
        b.ids.copy_(torch.arange(m, dtype=torch.int32, device=dev))

        def build():
            _jpeglib.check(L.x3djpeg_store_build_jobs(*b._args, stream()))
        for _ in range(10):
            build()
        v = []
        for _ in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(50):
                build()
            e1.record()
            torch.cuda.synchronize()
            v.append(e0.elapsed_time(e1) * 1e3 / 50)
        res["build_kernels"]["frames_%d" % m] = dict(bj._stats(v, "us_per_batch"), job_bytes_written=m * (
            _jpeglib.SCAN_JOB_DT.itemsize + _jpeglib.FRAME_JOB_DT.itemsize))

        b.launch()
        torch.cuda.synchronize()
        assert torch.equal(b.dst[:len(distinct)], torch.stack(want)[:m]) and not b.status.any()
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                b.launch()
        torch.cuda.current_stream().wait_stream(side)

        def eager():
            b.launch()
            torch.cuda.synchronize()

        def replay():
            graph.replay()
            torch.cuda.synchronize()

        b.dst.zero_()
        replay()
        assert torch.equal(b.dst[:len(distinct)], torch.stack(want)[:m])
        versions = {"eager": eager, "replay": replay}
        for fn in versions.values():
            for _ in range(3):
                fn()
        rates = {k: [] for k in versions}
        for _ in range(args.rounds):
            for k, fn in versions.items():
                rates[k].append(bj._rate(fn, m, args.window))
        r = {k: bj._stats(v, "frames_per_s") for k, v in rates.items()}
        r["replay_over_eager_median"] = r["replay"]["frames_per_s"] / r["eager"]["frames_per_s"]
        res["replay"]["frames_%d" % m] = r

    # (d) resident bytes
    arena_used = sum(c[2] for c in store._chunks)
    res["resident"] = {"arena_bytes_per_frame": arena_used / n, "record_bytes_per_frame": _jpeglib.STORE_REC_DT.itemsize,
                       "header_entries": store.n_headers, "header_bytes": store.n_headers * _jpeglib.STORE_HEADER_DT.itemsize,
                       "bytes_resident_as_allocated": store.bytes_resident(), "chunk_bytes": store.chunk_bytes,
                       "file_bytes_per_frame": sum(len(d) for d in files) / n, "decoded_bytes_per_frame": H * W * 3}
    res["resident"]["arena_over_file"] = res["resident"]["arena_bytes_per_frame"] / res["resident"]["file_bytes_per_frame"]
    res["resident"]["decoded_over_arena"] = H * W * 3 / (res["resident"]["arena_bytes_per_frame"] + _jpeglib.STORE_REC_DT.itemsize)

    out = json.dumps(res, sort_keys=True)
    print(out)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench.json"), "w") as f:
        f.write(out + "\n")
    with open(os.path.join(args.out, "README.md"), "w") as f:
        f.write(readme(res))


def _row(s, key="frames_per_s", fmt="%.0f"):
    return (fmt + " (" + fmt + " .. " + fmt + ")") % (s[key], s[key + "_min"], s[key + "_max"])


def readme(res):
    """profiles/jpeg_store/README.md from the figures of one run."""
    lines = ["# Frame store: decode by frame id against the device path", "",
             "Written by `tools/bench_jpeg_store.py` on %s; `bench.json` beside this file holds every figure. The protocol is that "
             "of `profiles/jpeg_entropy/`: %d distinct frames of %d x %d 4:2:0 quality %d repeated to %d, `torch.equal` against "
             "the host path before any timing, a warm-up, then the median of %d alternating windows of %.1f s with the slowest "
             "and the fastest window in brackets. Sources: csrc_jpeg %s." % (
                 res["device"], 16, res["frame"][0], res["frame"][1], res["quality"], res["batch"], res["rounds"], res["window_s"],
                 res["csrc_jpeg_sha16"]), "",
             "## decode_into + synchronise, frames/s", "",
             "| frames | store | device path, bytes in memory (2 threads) | device path, files on disk (2 threads) |",
             "|---|---|---|---|"]
    for k, r in sorted(res["decode"].items(), key=lambda kv: int(kv[0].split("_")[1])):
        lines.append("| %s | %s | %s | %s |" % (k.split("_")[1], _row(r["store"]), _row(r["device_path_memory"]),
                                               _row(r["device_path_files"])))
    lines += ["", "The bar of the change, per batch size:", ""]
    for k, r in sorted(res["decode"].items(), key=lambda kv: int(kv[0].split("_")[1])):
        lines.append("- %s frames: the store's median is %.2f x the in-memory device path's median (the bar: at least 1: %s); its "
                     "slowest window is %.2f x the fastest window of the device path reading files (the bar: above 1: %s)." % (
                         k.split("_")[1], r["store_over_memory_median"], "holds" if r["bar_median_not_below_memory"] else "DOES NOT HOLD",
                         r["store_slowest_over_files_fastest"], "holds" if r["bar_slowest_above_files_fastest"] else "DOES NOT HOLD"))
    lines += ["", "The files of this run are small and were just written, so they come from the page cache: the row with files "
              "is the cost of open / read / close per frame, not of a disk.", "",
              "## add, frames/s (a fresh store, 256 frames, + synchronise)", ""]
    for k, r in sorted(res["add"].items()):
        lines.append("- %s: %s" % (k.replace("_", " "), _row(r)))
    lines += ["", "## The two build kernels alone (x3djpeg_store_build_jobs between device events), us per batch", ""]
    for k, r in sorted(res["build_kernels"].items(), key=lambda kv: int(kv[0].split("_")[1])):
        lines.append("- %s frames: %s for %d bytes of job tables" % (k.split("_")[1], _row(r, "us_per_batch", "%.1f"),
                                                                     r["job_bytes_written"]))
    lines += ["", "## A captured plan against the same launches made eagerly, frames/s (+ synchronise)", ""]
    for k, r in sorted(res["replay"].items(), key=lambda kv: int(kv[0].split("_")[1])):
        lines.append("- %s frames: replay %s, eager %s, replay / eager %.2f" % (k.split("_")[1], _row(r["replay"]), _row(r["eager"]),
                                                                                r["replay_over_eager_median"]))
    d = res["resident"]
    lines += ["", "## Resident bytes per frame", "",
              "- arena (prepared scan, padding, segment table): %.0f; record: %d; the %d header entr%s of the batch: %d bytes in all"
              % (d["arena_bytes_per_frame"], d["record_bytes_per_frame"], d["header_entries"],
                 "y" if d["header_entries"] == 1 else "ies", d["header_bytes"]),
              "- the file: %.0f (arena / file %.3f); the decoded frame: %d (%.1f x arena + record)"
              % (d["file_bytes_per_frame"], d["arena_over_file"], d["decoded_bytes_per_frame"], d["decoded_over_arena"]),
              "- as allocated, this store of %d frames holds %d bytes: chunks of %d bytes are allocated whole."
              % (res["batch"], d["bytes_resident_as_allocated"], d["chunk_bytes"]), "",
              "## Reading the figures", "",
              "- Per batch the store path uploads 28 bytes per request and launches; the time that is left is the kernels' "
              "(`profiles/jpeg_entropy/` has the three decoder kernels at 1.27 ms per 256 frames), which is why a replayed graph "
              "and the same launches made eagerly tie: there is no host work left for a graph to remove. What the graph gives "
              "is a decode that can sit inside a larger captured step and be replayed on other ids.",
              "- `add` is one pass over each file on the host and one copy per chunk touched, once per frame and not per step. "
              "Where two threads are slower than one, a batch of %d frames is too short a pass for the pool's hand-over to pay."
              % res["batch"],
              "- Nothing here is a share of any peak: these are achieved rates of one process on one GPU.", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    main()
