"""Timing of the two tiers of the frame store (x3dhip.jpegstore.FrameStore: arena in HBM, or in pinned host memory behind
csrc_jpeg/stage.hip) and of its pack files, by the protocol of profiles/jpeg_store/: 16 distinct frames of 256 x 340 4:2:0
quality 75 (tools/bench_jpeg_decode.py makes them) repeated to `--frames` frames, so that random ids do not sit in any
cache; a torch.equal check against the host path before any timing; a warm-up; then the median of `--rounds` alternating
windows with minimum and maximum.  One JSON line, also written to profiles/jpeg_tier/bench.json, and
profiles/jpeg_tier/README.md from the same figures.

    python tools/bench_jpeg_tier.py [--out DIR] [--rounds N] [--window S] [--frames N]

  decode   decode_into + synchronise of random ids, batches of 128 and 256, three ways, alternating window by window: the
           HBM tier; the host tier; JpegDecoder(entropy="device", threads=2) reading files from disk
  stage    x3djpeg_stage alone (its two launches) between two device events, us per batch, and staged bytes / time
  pack     FrameStore.save and FrameStore.load of the whole store, GB/s, both tiers
  pinned   pinned bytes per frame of the host tier
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "x3d-multigrid_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

from tools import bench_jpeg_decode as bj  # noqa: E402

H, W = bj.H, bj.W
HOST_LINK_GBS = 63.0        # PCIe Gen5 x16, the specification


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_tier"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=65536)
    ap.add_argument("--files", type=int, default=4096, help="files on disk the device path draws from")
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
    nd, n = len(distinct), args.frames
    want = torch.stack(jpegops.JpegDecoder(dev, threads=16).decode(distinct))
    tmp = tempfile.mkdtemp(prefix="jpeg_tier_bench_")
    pack_path = os.path.join(tmp, "frames.pack")

    # fill the HBM tier from the files, write it as a pack, read the pack into the host tier
    hbm = jpegstore.FrameStore(dev, threads=2)
    for lo in range(0, n, 1024):
        hbm.add([distinct[i % nd] for i in range(lo, min(n, lo + 1024))])
    res = {"metric": "jpeg_tier", "csrc_jpeg_sha16": stamp.csrc_jpeg_sha16(), "csrc_sha16": stamp.csrc_sha16(),
           "commit": stamp.commit(), "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_s": args.window,
           "frames": n, "distinct": nd, "frame": [H, W], "subsampling": "4:2:0", "quality": 75, "encoder": encoder,
           "sub_bits": hbm.sub_bits, "mean_file_bytes": sum(len(d) for d in distinct) / nd,
           "host_link_spec_gb_per_s": HOST_LINK_GBS,
           "checked_against": "JpegDecoder(entropy='host'), torch.equal on every frame of a random batch, each tier"}

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    res["pack"] = {}
    _, t = timed(lambda: hbm.save(pack_path))
    pack_bytes = os.path.getsize(pack_path)
    res["pack"]["bytes"] = pack_bytes
    res["pack"]["save_device_gb_per_s"] = pack_bytes / t / 1e9
    (host, _, _), t = timed(lambda: jpegstore.FrameStore.load(pack_path, dev, tier="host"))
    res["pack"]["load_host_gb_per_s"] = pack_bytes / t / 1e9
    _, t = timed(lambda: host.save(pack_path + ".host"))
    res["pack"]["save_host_gb_per_s"] = pack_bytes / t / 1e9
    os.remove(pack_path + ".host")
    (again, _, _), t = timed(lambda: jpegstore.FrameStore.load(pack_path, dev, tier="device"))
    res["pack"]["load_device_gb_per_s"] = pack_bytes / t / 1e9
    assert len(again) == len(host) == n
    del again
    os.remove(pack_path)
    res["pack"]["note"] = "the file was just written: reads come from the page cache, writes go to it"

    # the same bits first: a random batch from each tier
    rng = np.random.default_rng(2024)
    ids = rng.integers(0, n, 256)
    dst = torch.empty((256, H, W, 3), dtype=torch.uint8, device=dev)
    for store in (hbm, host):
        dst.zero_()
        store.decode_into(ids, dst)
        assert torch.equal(dst, want[torch.from_numpy(ids % nd).to(dev)])

    # files on disk for the device path
    for i in range(args.files):
        with open(os.path.join(tmp, frames_mod.FRAME_NAME.format(i + 1)), "wb") as f:
            f.write(distinct[i % nd])
    folder = frames_mod.FrameFolder(tmp)
    dec = jpegops.JpegDecoder(dev, threads=2, entropy="device")

    res["decode"] = {}
    for m in (128, 256):
        dst = torch.empty((m, H, W, 3), dtype=torch.uint8, device=dev)

        def from_hbm():
            hbm.decode_into(rng.integers(0, n, m), dst)
            torch.cuda.synchronize()

        def from_host():
            host.decode_into(rng.integers(0, n, m), dst)
            torch.cuda.synchronize()

        def from_files():
            dec.decode_into(folder.read(rng.integers(0, args.files, m).tolist()), dst)
            torch.cuda.synchronize()

        versions = {"hbm_tier": from_hbm, "host_tier": from_host, "device_path_files": from_files}
        for fn in versions.values():
            for _ in range(3):
                fn()
        rates = {k: [] for k in versions}
        for _ in range(args.rounds):
            for k, fn in versions.items():
                rates[k].append(bj._rate(fn, m, args.window))
        r = {k: bj._stats(v, "frames_per_s") for k, v in rates.items()}
        ht, fil = r["host_tier"], r["device_path_files"]
        spread = max(ht["frames_per_s_max"] - ht["frames_per_s_min"], fil["frames_per_s_max"] - fil["frames_per_s_min"])
        r["margin_frames_per_s"] = spread
        r["host_over_files_median"] = ht["frames_per_s"] / fil["frames_per_s"]
        r["host_over_hbm_median"] = ht["frames_per_s"] / r["hbm_tier"]["frames_per_s"]
        r["bar_host_median_not_below_files"] = ht["frames_per_s"] >= fil["frames_per_s"]
        r["bar_holds_by_more_than_the_margin"] = ht["frames_per_s"] - fil["frames_per_s"] > spread
        res["decode"]["frames_%d" % m] = r

    # the two stage launches alone
    L = _jpeglib.lib()
    res["stage"] = {}
    for m in (128, 256):
        b = host.plan(m, W, H)
        pick = rng.integers(0, n, (64, m)).astype(np.int32)
        picks = torch.from_numpy(pick).to(dev)
        staged = float(_jpeglib.stage_bytes(host.scan_bytes[pick], host.nseg[pick]).sum()) / len(pick)

        def stage(k):
            b.ids.copy_(picks[k % len(pick)])
            _jpeglib.check(L.x3djpeg_stage(*b._stage_args, stream()))
        for k in range(10):
            stage(k)
        v = []
        for _ in range(args.rounds):
            total = 0.0
            for k in range(50):
                b.ids.copy_(picks[k % len(pick)])
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _jpeglib.check(L.x3djpeg_stage(*b._stage_args, stream()))
                e1.record()
                torch.cuda.synchronize()
                total += e0.elapsed_time(e1)
            v.append(total * 1e3 / 50)
        s = bj._stats(v, "us_per_batch")
        res["stage"]["frames_%d" % m] = dict(s, staged_bytes=staged, gb_per_s=staged / s["us_per_batch"] / 1e3,
                                             share_of_spec=staged / s["us_per_batch"] / 1e3 / HOST_LINK_GBS)

    used = sum(c[2] for c in host._chunks)
    res["pinned"] = {"bytes_pinned": host.bytes_pinned(), "bytes_per_frame_as_allocated": host.bytes_pinned() / n,
                     "arena_bytes_per_frame": used / n, "chunk_bytes": host.chunk_bytes, "chunks": host.n_chunks,
                     "device_bytes_of_the_host_tier": host.bytes_resident(), "device_bytes_of_the_hbm_tier": hbm.bytes_resident()}
    for name in os.listdir(tmp):
        os.remove(os.path.join(tmp, name))
    os.rmdir(tmp)

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
    """profiles/jpeg_tier/README.md from the figures of one run."""
    by_n = lambda d: sorted(d.items(), key=lambda kv: int(kv[0].split("_")[1]))       # noqa: E731
    lines = ["# Frame store tiers: HBM, pinned host memory, and the files they replace", "",
             "Written by `tools/bench_jpeg_tier.py` on %s; `bench.json` beside this file holds every figure. The protocol is that "
             "of `profiles/jpeg_store/`: %d distinct frames of %d x %d 4:2:0 quality %d repeated to %d frames (%.2f GB of arena, "
             "so that random ids do not sit in any cache), `torch.equal` against the host path before any timing, a warm-up, "
             "then the median of %d alternating windows of %.1f s with the slowest and the fastest window in brackets. Every "
             "batch draws fresh random ids. Sources: csrc_jpeg %s." % (
                 res["device"], res["distinct"], res["frame"][0], res["frame"][1], res["quality"], res["frames"],
                 res["pinned"]["arena_bytes_per_frame"] * res["frames"] / 1e9, res["rounds"], res["window_s"],
                 res["csrc_jpeg_sha16"]), "",
             "## decode_into + synchronise, frames/s", "",
             "| frames | HBM tier | host tier | device path, files on disk (2 threads) |", "|---|---|---|---|"]
    for k, r in by_n(res["decode"]):
        lines.append("| %s | %s | %s | %s |" % (k.split("_")[1], _row(r["hbm_tier"]), _row(r["host_tier"]), _row(r["device_path_files"])))
    lines += ["", "The bar of the change: the host tier's median is at least the median of the device path reading files, the "
              "path it replaces for a dataset larger than HBM; the margin is the larger of the two max - min spreads.", ""]
    for k, r in by_n(res["decode"]):
        lines.append("- %s frames: host tier / files = %.2f (the bar: at least 1: %s; the difference %s the margin of %.0f "
                     "frames/s). Host tier / HBM tier = %.2f, reported without a bar." % (
                         k.split("_")[1], r["host_over_files_median"],
                         "holds" if r["bar_host_median_not_below_files"] else "DOES NOT HOLD",
                         "exceeds" if r["bar_holds_by_more_than_the_margin"] else "is within", r["margin_frames_per_s"],
                         r["host_over_hbm_median"]))
    lines += ["", "The files of this run are small and were just written, so they come from the page cache: that column is the "
              "cost of open / read / close and of the host's parse and un-stuffing per frame, not of a disk.", "",
              "## The two stage launches alone (x3djpeg_stage between device events), per batch", ""]
    for k, r in by_n(res["stage"]):
        lines.append("- %s frames: %s us for %.0f staged bytes: %.1f GB/s over the host link (its specification is %.0f GB/s; "
                     "this is a reported figure, not a share of a bound that anything is held to)" % (
                         k.split("_")[1], _row(r, "us_per_batch", "%.1f"), r["staged_bytes"], r["gb_per_s"],
                         res["host_link_spec_gb_per_s"]))
    p, d = res["pack"], res["pinned"]
    lines += ["", "## Pack files (%d bytes), GB/s" % p["bytes"], "",
              "- save: HBM tier %.2f, host tier %.2f" % (p["save_device_gb_per_s"], p["save_host_gb_per_s"]),
              "- load: into the HBM tier %.2f, into the host tier %.2f" % (p["load_device_gb_per_s"], p["load_host_gb_per_s"]),
              "- %s." % p["note"], "",
              "## Pinned bytes", "",
              "- %.0f pinned bytes per frame as allocated (%d chunks of %d bytes, allocated whole), %.0f in use per frame; the "
              "host tier keeps %d bytes on the device (record and header tables) where the HBM tier keeps %d."
              % (d["bytes_per_frame_as_allocated"], d["chunks"], d["chunk_bytes"], d["arena_bytes_per_frame"],
                 d["device_bytes_of_the_host_tier"], d["device_bytes_of_the_hbm_tier"]), "",
              "## What nobody had measured before this run", "",
              "- The gather rate over the host link (the stage section) and the host tier / HBM tier ratio (the bar section) are "
              "first measurements on this machine; the design was made without them.",
              "- The Kinetics-scale estimate of DESIGN.md section 6, row 12 -- about 240 k videos x about 300 frames x about 14 KB, "
              "roughly 1 TB for Kinetics-400 train, about 13 GB for the validation windows -- stays an estimate from the "
              "bytes per frame of this synthetic set: no real Kinetics tree was on the machine.",
              "- Nothing here is a share of any peak: these are achieved rates of one process on one GPU.", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    main()
