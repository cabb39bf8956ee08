"""Timing of the indexed Huffman decoder (csrc_jpeg/entropy_indexed.hip, FrameStore(index_bits=...)) against the
relaxation decoder and the frame store without an index, in one process, by the protocol of profiles/jpeg_entropy/ and
profiles/jpeg_store/: the same 16 frames of 256 x 340 4:2:0 quality 75 repeated to 128 and to 256
(tools/bench_jpeg_decode.py makes them), a torch.equal check against the host path before any timing, a warm-up, then the
median of `--rounds` alternating windows with minimum and maximum.  One JSON line, also written to
profiles/jpeg_index/bench.json, and profiles/jpeg_index/README.md from the same figures.

    python tools/bench_jpeg_index.py [--out DIR] [--rounds N] [--window S]

  kernel     the Huffman launch alone on built job tables between two device events, us per frame: the indexed kernel at
             index_bits 128, 256, 512, 1024 and the relaxation kernel at sub_bits 512, 1024, alternating
  decode     decode_into + synchronise for 128 and 256 frames: the store without an index and the indexed store at each
             granularity, in both tiers, alternating window by window
  add        FrameStore.add of the 256 frames into a fresh store (+ synchronise) with and without the index, frames/s
  index      index bytes per frame at each granularity against the arena bytes
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "x3d-multigrid_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

from tools import bench_jpeg_decode as bj  # noqa: E402

H, W = bj.H, bj.W
INDEX_BITS = (128, 256, 512, 1024)
SUB_BITS = (512, 1024)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_index"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window")
    args = ap.parse_args()
    import torch
    from tools import stamp
    from x3dhip import _jpeglib, jpegops, jpegstore
    from x3dhip._lib import stream
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    distinct, encoder = bj.make_frames(args.distinct)
    files = [distinct[i % len(distinct)] for i in range(args.batch)]
    n = len(files)
    sizes = sorted({n // 2, n})
    L = _jpeglib.lib()

    # the same bits first: every store of the run against the host path
    want = torch.stack(jpegops.JpegDecoder(dev, threads=16).decode(distinct))
    stores = {}
    for tier in jpegstore.TIERS:
        for sb in SUB_BITS:
            stores[tier, "relax_%d" % sb] = jpegstore.FrameStore(dev, threads=2, tier=tier, sub_bits=sb, chunk_bytes=16 << 20)
        for ib in INDEX_BITS:
            stores[tier, "indexed_%d" % ib] = jpegstore.FrameStore(dev, threads=2, tier=tier, index_bits=ib, chunk_bytes=16 << 20)
    for key, s in stores.items():
        ids = s.add(files)
        out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
        s.decode_into(list(ids), out)
        assert torch.equal(out.view(n // len(distinct), len(distinct), H, W, 3),
                           want.expand(n // len(distinct), -1, -1, -1, -1)), key
    plain = stores["device", "relax_1024"]
    res = {"metric": "jpeg_index", "csrc_jpeg_sha16": stamp.csrc_jpeg_sha16(), "csrc_sha16": stamp.csrc_sha16(),
           "commit": stamp.commit(), "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_s": args.window,
           "batch": n, "frame": [H, W], "subsampling": "4:2:0", "quality": 75, "encoder": encoder,
           "mean_file_bytes": sum(len(d) for d in distinct) / len(distinct),
           "index_bits_default": _jpeglib.INDEX_BITS_DEFAULT,
           "checked_against": "JpegDecoder(entropy='host'), torch.equal on every frame of every store of the run"}

    # (a) the Huffman launch alone, on job tables built once
    res["kernel"] = {}
    for m in sizes:
        kernels = {}
        for key in ["relax_%d" % sb for sb in SUB_BITS] + ["indexed_%d" % ib for ib in INDEX_BITS]:
            s = stores["device", key]
            b = s.plan(m, W, H)
            b.ids.copy_(torch.arange(m, dtype=torch.int32, device=dev))
            b.launch()
            torch.cuda.synchronize()
            assert not b.status.any() and torch.equal(b.dst[:len(distinct)], want[:m])
            if b.index_bits is None:
                def kern(b=b):
                    _jpeglib.check(L.x3djpeg_entropy_decode_batch(b.scan_jobs.data_ptr(), b.n, b.sub_bits, b.workspace.data_ptr(),
                                                                  b.ws_cap, b.status.data_ptr(), stream()))
            else:
                def kern(b=b):
                    _jpeglib.check(L.x3djpeg_entropy_decode_indexed(b.scan_jobs.data_ptr(), b.n, *b._index_args,
                                                                    b.status.data_ptr(), stream()))
            kernels[key] = (kern, b)
        for kern, _ in kernels.values():
            for _ in range(5):
                kern()
        torch.cuda.synchronize()
        v = {k: [] for k in kernels}
        for _ in range(args.rounds):
            for k, (kern, _) in kernels.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(20):
                    kern()
                e1.record()
                torch.cuda.synchronize()
                v[k].append(e0.elapsed_time(e1) * 1e3 / 20 / m)
        r = {k: bj._stats(t, "us_per_frame") for k, t in v.items()}
        for k, (_, b) in kernels.items():
            assert not b.status.any(), k
        best_i = min((k for k in r if k.startswith("indexed")), key=lambda k: r[k]["us_per_frame"])
        best_r = min((k for k in r if k.startswith("relax")), key=lambda k: r[k]["us_per_frame"])
        r["best_indexed"], r["best_relax"] = best_i, best_r
        r["relax_over_indexed_median"] = r[best_r]["us_per_frame"] / r[best_i]["us_per_frame"]
        r["bar_indexed_slowest_faster_than_relax_fastest"] = r[best_i]["us_per_frame_max"] < r[best_r]["us_per_frame_min"]
        res["kernel"]["frames_%d" % m] = r

    # (b) decode_into + synchronise, both tiers, alternating
    res["decode"] = {}
    for tier in jpegstore.TIERS:
        for m in sizes:
            dst = torch.empty((m, H, W, 3), dtype=torch.uint8, device=dev)
            idl = np.arange(m)
            versions = {}
            for key in ["relax_1024"] + ["indexed_%d" % ib for ib in INDEX_BITS]:
                def run(s=stores[tier, key]):
                    s.decode_into(idl, dst)
                    torch.cuda.synchronize()
                versions[key] = run
            for fn in versions.values():
                for _ in range(3):
                    fn()
                assert torch.equal(dst[:len(distinct)], want[:m])
            rates = {k: [] for k in versions}
            for _ in range(args.rounds):
                for k, fn in versions.items():
                    rates[k].append(bj._rate(fn, m, args.window))
            r = {k: bj._stats(v, "frames_per_s") for k, v in rates.items()}
            best = max((k for k in r if k.startswith("indexed")), key=lambda k: r[k]["frames_per_s"])
            r["best_indexed"] = best
            r["indexed_over_plain_median"] = r[best]["frames_per_s"] / r["relax_1024"]["frames_per_s"]
            r["bar_median_not_below_plain"] = r[best]["frames_per_s"] >= r["relax_1024"]["frames_per_s"]
            r["default_over_plain_median"] = (r["indexed_%d" % _jpeglib.INDEX_BITS_DEFAULT]["frames_per_s"]
                                              / r["relax_1024"]["frames_per_s"])
            res["decode"]["%s_frames_%d" % (tier, m)] = r

    # (c) add with and without the index
    res["add"] = {}
    versions = {}
    for key, kw in [("plain", {})] + [("indexed_%d" % ib, dict(index_bits=ib)) for ib in (128, 1024)]:
        def add(kw=kw):
            s = jpegstore.FrameStore(dev, threads=2, **kw)
            s.add(files)
            torch.cuda.synchronize()
        add()
        versions[key] = add
    rates = {k: [] for k in versions}
    for _ in range(args.rounds):
        for k, fn in versions.items():
            rates[k].append(bj._rate(fn, n, args.window))
    res["add"] = {k: bj._stats(v, "frames_per_s") for k, v in rates.items()}
    res["add"]["threads"] = 2

    # (d) bytes
    arena = sum(c[2] for c in plain._chunks) / n
    res["index"] = {"arena_bytes_per_frame": arena, "scan_bytes_per_frame": float(plain.scan_bytes.mean())}
    for ib in INDEX_BITS:
        s = stores["device", "indexed_%d" % ib]
        per = 8 * float(s.nentries.mean()) + _jpeglib.INDEX_REC_DT.itemsize
        res["index"]["index_bits_%d" % ib] = {"bytes_per_frame": per, "entries_per_frame": float(s.nentries.mean()),
                                              "over_scan_bytes": per / float(plain.scan_bytes.mean()),
                                              "bytes_index_as_allocated": s.bytes_index()}

    out = json.dumps(res, sort_keys=True)
    print(out)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench.json"), "w") as f:
        f.write(out + "\n")
    with open(os.path.join(args.out, "README.md"), "w") as f:
        f.write(readme(res))


def _row(s, key="frames_per_s", fmt="%.0f"):
    return (fmt + " (" + fmt + " .. " + fmt + ")") % (s[key], s[key + "_min"], s[key + "_max"])


def _holds(flag):
    return "holds" if flag else "DOES NOT HOLD"


def readme(res):
    """profiles/jpeg_index/README.md from the figures of one run."""
    keys = ["relax_%d" % sb for sb in SUB_BITS] + ["indexed_%d" % ib for ib in INDEX_BITS]
    lines = ["# Sync index: one-pass Huffman decoding against the relaxation decoder", "",
             "Written by `tools/bench_jpeg_index.py` on %s; `bench.json` beside this file holds every figure. The protocol is "
             "that of `profiles/jpeg_entropy/` and `profiles/jpeg_store/`: 16 distinct frames of %d x %d 4:2:0 quality %d "
             "repeated to %d, `torch.equal` against the host path for every store of the run before any timing, a warm-up, then "
             "the median of %d alternating windows with the slowest and the fastest window in brackets. The relaxation kernel "
             "and the store without an index are the parent commit's, run in the same process. Sources: csrc_jpeg %s." % (
                 res["device"], res["frame"][0], res["frame"][1], res["quality"], res["batch"], res["rounds"],
                 res["csrc_jpeg_sha16"]), "",
             "## The Huffman launch alone (between device events, 20 launches per window), us per frame", "",
             "| frames | " + " | ".join(k.replace("_", " ") for k in keys) + " |", "|---|" + "---|" * len(keys)]
    for k, r in sorted(res["kernel"].items(), key=lambda kv: int(kv[0].split("_")[1])):
        lines.append("| %s | %s |" % (k.split("_")[1], " | ".join(_row(r[q], "us_per_frame", "%.2f") for q in keys)))
    lines += ["", "The bar, per batch size: at its best granularity the indexed kernel's slowest window is faster than the "
              "relaxation kernel's fastest window at its better sub_bits.", ""]
    for k, r in sorted(res["kernel"].items(), key=lambda kv: int(kv[0].split("_")[1])):
        lines.append("- %s frames: %s at %.2f us (slowest %.2f) against %s at %.2f us (fastest %.2f), %.2f x by the medians: %s." % (
            k.split("_")[1], r["best_indexed"].replace("_", " "), r[r["best_indexed"]]["us_per_frame"],
            r[r["best_indexed"]]["us_per_frame_max"], r["best_relax"].replace("_", " "), r[r["best_relax"]]["us_per_frame"],
            r[r["best_relax"]]["us_per_frame_min"], r["relax_over_indexed_median"],
            _holds(r["bar_indexed_slowest_faster_than_relax_fastest"])))
    dkeys = ["relax_1024"] + ["indexed_%d" % ib for ib in INDEX_BITS]
    lines += ["", "## decode_into + synchronise, frames/s", "",
              "| tier, frames | store without an index (sub_bits 1024) | " + " | ".join(k.replace("_", " ") for k in dkeys[1:]) + " |",
              "|---|" + "---|" * len(dkeys)]
    for k, r in res["decode"].items():
        lines.append("| %s | %s |" % (k.replace("_frames_", ", "), " | ".join(_row(r[q]) for q in dkeys)))
    lines += ["", "The bar, per tier and batch size: the indexed store's median is at least the plain store's.", ""]
    for k, r in res["decode"].items():
        lines.append("- %s: %s, %.2f x the plain store by the medians: %s (index_bits %d, the default: %.2f x)." % (
            k.replace("_frames_", ", "), r["best_indexed"].replace("_", " "), r["indexed_over_plain_median"],
            _holds(r["bar_median_not_below_plain"]), res["index_bits_default"], r["default_over_plain_median"]))
    a = res["add"]
    lines += ["", "## add, frames/s (a fresh store, %d frames, %d threads, + synchronise)" % (res["batch"], a["threads"]), ""]
    for k in sorted(k for k in a if k != "threads"):
        lines.append("- %s: %s" % (k.replace("_", " "), _row(a[k])))
    d = res["index"]
    lines += ["", "## Index bytes per frame (arena %.0f, scan %.0f)" % (d["arena_bytes_per_frame"], d["scan_bytes_per_frame"]), ""]
    for ib in INDEX_BITS:
        e = d["index_bits_%d" % ib]
        lines.append("- index_bits %d: %.0f bytes (%.1f entries and the 16-byte record), %.1f %% of the scan bytes" % (
            ib, e["bytes_per_frame"], e["entries_per_frame"], 100 * e["over_scan_bytes"]))
    big = res["kernel"]["frames_%d" % res["batch"]]
    lines += ["", "## Reading the figures", "",
              "- The indexed kernel makes one pass over each scan where the relaxation kernel makes a speculative pass, its "
              "relaxation rounds, a counting sum and the write pass; the write pass is the same code (`decode_span<kWrite>`).",
              "- One workgroup of 256 workers decodes one frame, each worker a contiguous share of the subsequences one after "
              "the other, so a launch lasts as long as its slowest worker whatever the batch is, up to one workgroup per "
              "compute unit: %.0f us for %d frames and %.0f us for %d at %s. That is why the time per frame halves from the "
              "smaller batch to the larger one." % (
                  res["kernel"]["frames_%d" % (res["batch"] // 2)][big["best_indexed"]]["us_per_frame"] * (res["batch"] // 2),
                  res["batch"] // 2, big[big["best_indexed"]]["us_per_frame"] * res["batch"], res["batch"],
                  big["best_indexed"].replace("_", " ")),
              "- At index_bits 1024 a frame of this size has %.0f subsequences: more than half of the 256 workers have none, "
              "and the others have twice the bits of 512 each. Below 512 every worker has several subsequences and the work "
              "per worker no longer shrinks, while the entries read and compared grow: 512 is the fastest, and the "
              "default (`X3DJPEG_INDEX_BITS_DEFAULT` %d)." % (d["index_bits_1024"]["entries_per_frame"],
                                                             res["index_bits_default"]),
              "- `add` with an index costs one more Huffman pass per frame on the host (`x3djpeg_index_build`), whatever the "
              "granularity; it is paid once per stored frame, or in `tools/pack_frames.py --index-bits` without a GPU.",
              "- Nothing here is a share of any peak: these are achieved rates of one process on one GPU.", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    main()
