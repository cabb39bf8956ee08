"""Timing of the JPEG input path (csrc_jpeg/ through x3dhip.jpegops.JpegDecoder) on 256 x 340 4:2:0 quality-75 frames, the
size of the reference's Kinetics frame folders.  One JSON line, also written to profiles/jpeg_decode/bench.json.

    python tools/bench_jpeg_decode.py [--out FILE] [--rounds N] [--batch N]
    python tools/bench_jpeg_decode.py --entropy        (the rows below "--entropy", to profiles/jpeg_entropy/bench.json)

  host_stage   x3djpeg_parse + x3djpeg_entropy_decode of a batch into the pinned buffer, frames/s at 1, 4, 8, 16 threads
  kernels      x3djpeg_idct and x3djpeg_to_rgb alone on a resident batch, between two device events: us per frame and
               bytes moved / time (coefficients read + planes written; planes read + RGB written) -- achieved rates,
               not a share of any peak
  end_to_end   JpegDecoder.decode_into (host stage, copy, job table, two launches) + synchronise, 16 threads, frames/s
  pillow       Image.open(...).convert('RGB') in a pool of 16 threads into a pinned [n, H, W, 3] buffer + one upload +
               synchronise, on the same frames; null when Pillow is not importable where this runs
--entropy: the device Huffman decoder (JpegDecoder(entropy="device")) against the host one, same frames, same protocol:
  scan_prepare     x3djpeg_parse + x3djpeg_scan_prepare of a batch into the pinned buffer, frames/s at 1, 2, 16 threads
  entropy_kernel   x3djpeg_entropy_decode_batch alone on a resident batch between two device events, us per frame, with the
                   relaxation rounds the frames used; once per sub_bits of 256 .. 4096
  end_to_end       decode_into + synchronise for both paths at 2 and at 16 threads, the four alternating window by window;
                   and the device path at 2 threads once per sub_bits
  bytes_copied     host-to-device bytes per batch of either path (coefficients; scans and segment tables)
Every figure: warm-up first, then `--rounds` windows of at least `--window` seconds (end_to_end and pillow alternate);
median, minimum and maximum.

The frames are made here: a smooth colour field with edges and noise per frame, encoded by Pillow where it is importable
and otherwise by the small baseline encoder below (orthonormal DCT, the quantisation and Huffman tables of a committed
golden file).  One frame is checked against tests/jpeg_ref.py, all against Pillow where importable, before any timing."""
import argparse
import io
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "x3d-multigrid_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

H, W = 256, 340
STEP_FRAMES_PER_S = 1034 * 16          # what the headline training step consumes (1034 clips/s at T = 16)


def content(seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    base = np.stack([128 + 100 * np.sin(x / 23.0 + seed) * np.cos(y / 31.0),
                     128 + 110 * np.cos((x + y) / 40.0 + 0.5 * seed),
                     255.0 * (((x // 45 + y // 37 + seed) % 2) > 0)], axis=-1)
    return np.clip(base + rng.normal(0, 6.0, base.shape), 0, 255).astype(np.uint8)


def encode_baseline(rgb, template):
    """4:2:0 baseline JPEG of rgb [H, W, 3] with the tables and headers of `template` (a 4:2:0 file): its bytes up to the
    scan with the frame size patched, then this image's Huffman-coded scan."""
    from tests import jpeg_ref as jr
    info = jr.parse(template)
    h, w, _ = rgb.shape
    f = rgb.astype(np.float64)
    ycc = [0.299 * f[..., 0] + 0.587 * f[..., 1] + 0.114 * f[..., 2],
           128 - 0.168736 * f[..., 0] - 0.331264 * f[..., 1] + 0.5 * f[..., 2],
           128 + 0.5 * f[..., 0] - 0.418688 * f[..., 1] - 0.081312 * f[..., 2]]
    mh, mw = -(-h // 16) * 16, -(-w // 16) * 16
    ycc = [np.pad(p, ((0, mh - h), (0, mw - w)), mode="edge") for p in ycc]
    ycc[1:] = [p.reshape(mh // 2, 2, mw // 2, 2).mean(axis=(1, 3)) for p in ycc[1:]]
    k = np.arange(8)
    C = np.sqrt(0.25) * np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16)
    C[0] /= np.sqrt(2)
    quant = []
    for p, comp in zip(ycc, info["comps"]):
        b = (p - 128).reshape(p.shape[0] // 8, 8, p.shape[1] // 8, 8).transpose(0, 2, 1, 3)
        q = np.rint((C @ b @ C.T) / info["qt"][comp["tq"]].reshape(8, 8)).astype(np.int64)
        quant.append(q.reshape(q.shape[0], q.shape[1], 64)[..., jr.ZIGZAG])
    codes = {key: {s: (c, ln) for (ln, c), s in jr._codes(*v).items()} for key, v in info["huff"].items()}
    out, acc, nb = bytearray(), 0, 0
    pred = [0, 0, 0]

    def put(code, ln):
        nonlocal acc, nb
        acc = (acc << ln) | code
        nb += ln
        while nb >= 8:
            byte = (acc >> (nb - 8)) & 255
            out.append(byte)
            if byte == 255:
                out.append(0)
            nb -= 8
        acc &= (1 << nb) - 1

    def value(v):
        s = int(abs(v)).bit_length()
        return s, (v if v >= 0 else v + (1 << s) - 1)

    for my in range(mh // 16):
        for mx in range(mw // 16):
            for ci, comp in enumerate(info["comps"]):
                dc, ac = codes[(0, comp["td"])], codes[(1, comp["ta"])]
                n = 2 if ci == 0 else 1
                for by in range(n):
                    for bx in range(n):
                        z = quant[ci][my * n + by, mx * n + bx]
                        s, bits = value(int(z[0]) - pred[ci])
                        pred[ci] = int(z[0])
                        put(*dc[s])
                        if s:
                            put(bits, s)
                        run = 0
                        nz = np.flatnonzero(z[1:]) + 1
                        last = 0
                        for i in nz:
                            run = int(i) - last - 1
                            while run > 15:
                                put(*ac[0xF0])
                                run -= 16
                            s, bits = value(int(z[i]))
                            put(*ac[(run << 4) | s])
                            put(bits, s)
                            last = int(i)
                        if last != 63:
                            put(*ac[0])
    if nb:
        put((1 << (8 - nb)) - 1, 8 - nb)
    head = bytearray(template[:info["scan_off"]])
    i = head.index(b"\xff\xc0")
    head[i + 5:i + 9] = bytes([h >> 8, h & 255, w >> 8, w & 255])
    return bytes(head) + bytes(out) + b"\xff\xd9"


def make_frames(n):
    try:
        from PIL import Image
    except ImportError:
        Image = None
    from tests import jpeg_ref as jr
    template = jr.load_cases()["c420_37x53_q75"][0]
    out = []
    for s in range(n):
        img = content(s)
        if Image is not None:
            buf = io.BytesIO()
            Image.fromarray(img).save(buf, "JPEG", quality=75, subsampling=2)
            out.append(buf.getvalue())
        else:
            out.append(encode_baseline(img, template))
    return out, ("pillow" if Image is not None else "built-in baseline encoder")


def _rate(fn, n, window):
    """frames/s of fn (n frames per call, ending in a synchronise where it uses the device) over >= `window` seconds."""
    calls, t0 = 0, time.perf_counter()
    while True:
        fn()
        calls += 1
        dt = time.perf_counter() - t0
        if dt >= window:
            return n * calls / dt


def _stats(v, key):
    return {key: statistics.median(v), key + "_min": min(v), key + "_max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entropy", action="store_true", help="the device Huffman decoder against the host one")
    ap.add_argument("--out", default=None, help="default: profiles/jpeg_decode/bench.json, profiles/jpeg_entropy/bench.json "
                                                "with --entropy")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window of the host-side figures")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "jpeg_entropy" if args.entropy else "jpeg_decode", "bench.json")
    import torch
    from tests import jpeg_ref as jr
    from tools import stamp
    from x3dhip import _jpeglib, jpegops
    from x3dhip._lib import stream
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    distinct, encoder = make_frames(args.distinct)
    frames = [distinct[i % len(distinct)] for i in range(args.batch)]
    n = len(frames)
    try:
        from PIL import Image
    except ImportError:
        Image = None

    def pil_decode(data):
        return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))

    # the same bits first
    dec16 = jpegops.JpegDecoder(dev, threads=16)
    got = dec16.decode(distinct)
    assert np.array_equal(got[0].cpu().numpy(), jr.decode(distinct[0]))
    if Image is not None:
        for g, d in zip(got, distinct):
            assert np.array_equal(g.cpu().numpy(), pil_decode(d))
    res = {"metric": "jpeg_decode", "csrc_jpeg_sha16": stamp.csrc_jpeg_sha16(), "csrc_sha16": stamp.csrc_sha16(),
           "commit": stamp.commit(), "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_s": args.window, "batch": n,
           "frame": [H, W], "subsampling": "4:2:0", "quality": 75, "encoder": encoder,
           "mean_file_bytes": sum(len(d) for d in distinct) / len(distinct),
           "checked_against": "tests/jpeg_ref.py" + (" and Pillow" if Image is not None else "")}

    if args.entropy:
        entropy_rows(args, res, frames, distinct, got, dev)
        return finish(args, res)

    # host stage alone
    res["host_stage"] = {}
    for th in (1, 4, 8, 16):
        d = jpegops.JpegDecoder(dev, threads=th)
        d._host_stage(frames)
        v = [_rate(lambda: d._host_stage(frames), n, args.window) for _ in range(args.rounds)]
        res["host_stage"]["threads_%d" % th] = _stats(v, "frames_per_s")

    # the two kernels alone
    infos, coef_host, offs = dec16._host_stage(frames)
    total = int(offs[-1])
    coef = torch.empty(total, dtype=torch.int16, device=dev)
    coef.copy_(coef_host)
    planes = torch.empty(total, dtype=torch.uint8, device=dev)
    dst = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
    jobs = np.zeros(n, dtype=_jpeglib.FRAME_JOB_DT)
    jpegops.fill_jobs(jobs, infos)
    jobs["coef"] = coef.data_ptr() + 2 * offs[:-1]
    jobs["planes"] = planes.data_ptr() + offs[:-1]
    jobs["dst"] = dst.data_ptr() + np.arange(n) * (H * W * 3)
    jobs["dst_stride"] = 3 * W
    jd = torch.from_numpy(jobs.view(np.uint8)).to(dev)
    L = _jpeglib.lib()
    nblk = int(infos["nblocks"].max())

    def idct():
        _jpeglib.check(L.x3djpeg_idct(jd.data_ptr(), n, nblk, stream()))

    def to_rgb():
        _jpeglib.check(L.x3djpeg_to_rgb(jd.data_ptr(), n, W, H, stream()))

    moved = {"idct": 3 * total, "to_rgb": total + n * H * W * 3}
    res["kernels"] = {}
    for name, fn in (("idct", idct), ("to_rgb", to_rgb)):
        for _ in range(10):
            fn()
        v = []
        for _ in range(args.rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(50):
                fn()
            b.record()
            torch.cuda.synchronize()
            v.append(a.elapsed_time(b) * 1e3 / 50 / n)
        r = _stats(v, "us_per_frame")
        r["bytes_moved_per_batch"] = moved[name]
        r["achieved_GBps"] = moved[name] / (r["us_per_frame"] * n * 1e-6) / 1e9
        res["kernels"][name] = r
    assert torch.equal(dst[0], got[0])

    # end to end against Pillow + upload, alternating
    def e2e():
        dec16.decode_into(frames, dst)
        torch.cuda.synchronize()

    pinned = torch.empty((n, H, W, 3), dtype=torch.uint8).pin_memory()
    pin_np = pinned.numpy()
    pool = ThreadPoolExecutor(max_workers=16)

    def pil_one(i):
        pin_np[i] = pil_decode(frames[i])

    def pil():
        list(pool.map(pil_one, range(n)))
        dst.copy_(pinned, non_blocking=True)
        torch.cuda.synchronize()

    versions = {"end_to_end": e2e}
    if Image is not None:
        versions["pillow"] = pil
    for fn in versions.values():
        for _ in range(3):
            fn()
    rates = {k: [] for k in versions}
    for _ in range(args.rounds):
        for k, fn in versions.items():
            rates[k].append(_rate(fn, n, args.window))
    res["end_to_end"] = dict(_stats(rates["end_to_end"], "frames_per_s"), threads=16)
    res["pillow"] = dict(_stats(rates["pillow"], "frames_per_s"), threads=16) if Image is not None else None
    res["pillow_note"] = None if Image is not None else "Pillow is not importable where this ran: no all-host figure"
    e = res["end_to_end"]
    res["step_consumes_frames_per_s"] = STEP_FRAMES_PER_S
    res["end_to_end_over_step_rate"] = e["frames_per_s"] / STEP_FRAMES_PER_S
    host16 = res["host_stage"]["threads_16"]["frames_per_s"]
    kern_us = res["kernels"]["idct"]["us_per_frame"] + res["kernels"]["to_rgb"]["us_per_frame"]
    res["kernels_us_per_frame"] = kern_us
    res["host_stage_us_per_frame_16_threads"] = 1e6 / host16
    res["kernels_share_of_host_stage_time"] = kern_us / (1e6 / host16)
    if Image is not None:
        p = res["pillow"]
        spread = max(e["frames_per_s_max"] - e["frames_per_s_min"], p["frames_per_s_max"] - p["frames_per_s_min"])
        res["spread_frames_per_s"] = spread
        res["end_to_end_not_below_pillow_beyond_spread"] = e["frames_per_s"] >= p["frames_per_s"] - spread
    finish(args, res)


def entropy_rows(args, res, frames, distinct, got, dev):
    """The rows of --entropy into res.  got: the host path's decode of `distinct`."""
    import torch
    from x3dhip import _jpeglib, jpegops
    n = len(frames)
    res["metric"] = "jpeg_entropy"
    sweep = (256, 512, 1024, 2048, 4096)
    default = _jpeglib.SUB_BITS_DEFAULT
    res["sub_bits_default"] = default
    # the same bits first: every sub_bits of the sweep, frame by frame against the host path
    for sb in sweep:
        d = jpegops.JpegDecoder(dev, threads=16, entropy="device", sub_bits=sb)
        for g, o in zip(got, d.decode(distinct)):
            assert torch.equal(g, o), sb
    res["checked_against"] += ", device path equal to the host path at every sub_bits"

    res["scan_prepare"] = {}
    for th in (1, 2, 16):
        d = jpegops.JpegDecoder(dev, threads=th, entropy="device")
        d._prepare_stage(frames)
        v = [_rate(lambda: d._prepare_stage(frames), n, args.window) for _ in range(args.rounds)]
        res["scan_prepare"]["threads_%d" % th] = _stats(v, "frames_per_s")

    # the entropy kernel alone
    dst = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
    targets = [(dst.data_ptr() + i * H * W * 3, 3 * W) for i in range(n)]
    L = _jpeglib.lib()
    from x3dhip._lib import stream
    res["entropy_kernel"] = {}
    for sb in sweep:
        d = jpegops.JpegDecoder(dev, threads=16, entropy="device", sub_bits=sb)
        b = d._stage_device(frames, lambda infos: targets)

        def kern():
            _jpeglib.check(L.x3djpeg_entropy_decode_batch(b["scan_jobs"], n, sb, b["workspace"].data_ptr(),
                                                          b["workspace"].numel(), b["status"].data_ptr(), stream()))
        for _ in range(5):
            kern()
        v = []
        for _ in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                kern()
            e1.record()
            torch.cuda.synchronize()
            v.append(e0.elapsed_time(e1) * 1e3 / 20 / n)
        assert not b["status"].any()
        r = _stats(v, "us_per_frame")
        r["us_per_batch"] = r["us_per_frame"] * n
        head = b["workspace"].cpu().numpy().view(np.int32)
        # the first int32 of each frame's workspace: its rounds; the second: its subsequences
        ws_off = b["ws_off"] // 4
        r["rounds_max"], r["rounds_mean"] = int(head[ws_off].max()), float(head[ws_off].mean())
        r["subsequences_mean"] = float(head[ws_off + 1].mean())
        res["entropy_kernel"]["sub_bits_%d" % sb] = r

    # end to end, both paths at 2 and at 16 threads, alternating
    versions = {}
    for th in (2, 16):
        for ent in ("host", "device"):
            d = jpegops.JpegDecoder(dev, threads=th, entropy=ent)

            def fn(d=d):
                d.decode_into(frames, dst)
                torch.cuda.synchronize()
            versions["%s_threads_%d" % (ent, th)] = (fn, d)
    for fn, _ in versions.values():
        for _ in range(3):
            fn()
    rates = {k: [] for k in versions}
    for _ in range(args.rounds):
        for k, (fn, _) in versions.items():
            rates[k].append(_rate(fn, n, args.window))
    res["end_to_end"] = {k: _stats(v, "frames_per_s") for k, v in rates.items()}
    res["bytes_copied_per_batch"] = {ent: versions["%s_threads_2" % ent][1].last_bytes_copied for ent in ("host", "device")}
    assert torch.equal(dst[:len(distinct)], torch.stack(got))

    # the device path at 2 threads once per sub_bits, alternating
    sw = {}
    for sb in sweep:
        d = jpegops.JpegDecoder(dev, threads=2, entropy="device", sub_bits=sb)

        def fn(d=d):
            d.decode_into(frames, dst)
            torch.cuda.synchronize()
        fn()
        sw[sb] = fn
    rates = {sb: [] for sb in sweep}
    for _ in range(args.rounds):
        for sb, fn in sw.items():
            rates[sb].append(_rate(fn, n, args.window))
    res["end_to_end_device_2_threads_by_sub_bits"] = {"sub_bits_%d" % sb: _stats(v, "frames_per_s") for sb, v in rates.items()}

    e = res["end_to_end"]
    res["step_consumes_frames_per_s"] = STEP_FRAMES_PER_S
    for th in (2, 16):
        h, d = e["host_threads_%d" % th], e["device_threads_%d" % th]
        spread = max(h["frames_per_s_max"] - h["frames_per_s_min"], d["frames_per_s_max"] - d["frames_per_s_min"])
        res["threads_%d" % th] = {"spread_frames_per_s": spread, "device_over_host": d["frames_per_s"] / h["frames_per_s"],
                                  "device_not_below_host_beyond_spread": d["frames_per_s"] >= h["frames_per_s"] - spread,
                                  "device_over_step_rate": d["frames_per_s"] / STEP_FRAMES_PER_S,
                                  "host_over_step_rate": h["frames_per_s"] / STEP_FRAMES_PER_S}


def finish(args, res):
    out = json.dumps(res, sort_keys=True)
    print(out)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
