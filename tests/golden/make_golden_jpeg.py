"""Writes tests/golden/jpeg_cases.npz: small JPEG files (as uint8 arrays) with Pillow's decode of each, the fixtures of
tests/test_jpeg_host.py and tests/test_jpeg_gpu.py.  Needs Pillow only; run it again only to add a case.

    python tests/golden/make_golden_jpeg.py

Per case: jpg_<name> (the file's bytes) and rgb_<name> (Pillow's Image.open(...).convert('RGB'), uint8 [H, W, 3]); the
rejects have no rgb_ entry.  names lists the cases in order; pillow / libjpeg record the versions that decoded them.
"""
import io
import os

import numpy as np
from PIL import Image, features
import PIL

HERE = os.path.dirname(os.path.abspath(__file__))


def content(w, h, seed, sigma=12.0):
    """A smooth colour field with edges plus noise, uint8 [h, w, 3]."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([128 + 100 * np.sin(x / 5.0 + seed) * np.cos(y / 7.0),
                     128 + 110 * np.cos((x + y) / 6.0 + 0.5 * seed),
                     255.0 * (((x // 5 + y // 3) % 2) > 0)], axis=-1)
    return np.clip(base + rng.normal(0, sigma, base.shape), 0, 255).astype(np.uint8)


def frame(t, w=64, h=48):
    """Frame t of the moving pattern."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    a = 128 + 100 * np.sin((x + 3 * t) / 6.0) * np.cos((y - 2 * t) / 5.0)
    b = 128 + 100 * np.cos((x - y + 5 * t) / 9.0)
    c = 255.0 * (((x + 4 * t) // 8 + y // 8) % 2 > 0)
    rng = np.random.default_rng(100 + t)
    return np.clip(np.stack([a, b, c], axis=-1) + rng.normal(0, 4, (h, w, 3)), 0, 255).astype(np.uint8)


def encode(arr, mode="RGB", **kw):
    buf = io.BytesIO()
    Image.fromarray(arr, mode).save(buf, "JPEG", **kw)
    return buf.getvalue()


def pillow(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def main():
    S444, S422, S420 = 0, 1, 2
    cases = []

    def add(name, data, reject=False):
        cases.append((name, data, None if reject else pillow(data)))

    add("c444_8x8", encode(content(8, 8, 1), quality=92, subsampling=S444))
    add("c420_17x9", encode(content(17, 9, 2), quality=92, subsampling=S420))
    add("c420_9x17", encode(content(9, 17, 3), quality=92, subsampling=S420))
    add("c422_3x4", encode(content(3, 4, 4), quality=92, subsampling=S422))
    add("c422_4x3", encode(content(4, 3, 5), quality=92, subsampling=S422))
    add("c420_3x4", encode(content(3, 4, 6), quality=92, subsampling=S420))
    add("c420_4x3", encode(content(4, 3, 7), quality=92, subsampling=S420))
    add("c420_5x6", encode(content(5, 6, 8), quality=92, subsampling=S420))
    add("c422_33x70_q60", encode(content(33, 70, 9), quality=60, subsampling=S422))
    add("c420_37x53_q75", encode(content(37, 53, 10), quality=75, subsampling=S420))
    add("c420_50x50_q100_noise", encode(content(50, 50, 11, sigma=60.0), quality=100, subsampling=S420))
    add("c420_40x56_q1", encode(content(40, 56, 12), quality=1, subsampling=S420))
    add("c420_40x56_optimize", encode(content(40, 56, 13), quality=85, subsampling=S420, optimize=True))
    add("c420_64x48_restart", encode(content(64, 48, 14), quality=80, subsampling=S420, restart_marker_blocks=3))
    add("grey_30x44", encode(content(30, 44, 15)[..., 0], mode="L", quality=85))
    add("c420_120x90_q50", encode(content(120, 90, 16, sigma=3.0), quality=50, subsampling=S420))
    for t in range(12):
        add("vid_%02d" % t, encode(frame(t), quality=75, subsampling=S420))
    add("reject_progressive", encode(content(24, 16, 17), quality=80, progressive=True), reject=True)
    add("reject_cmyk", encode(np.concatenate([content(16, 16, 18), content(16, 16, 19)[..., :1]], axis=-1), mode="CMYK",
                              quality=80), reject=True)
    whole = encode(content(37, 53, 10), quality=75, subsampling=S420)
    add("reject_truncated", whole[:len(whole) - (len(whole) - whole.index(b"\xff\xda")) // 2], reject=True)

    out = {"names": np.array([c[0] for c in cases]), "pillow": np.array(PIL.__version__),
           "libjpeg": np.array(str(features.version("jpg")))}
    for name, data, rgb in cases:
        out["jpg_" + name] = np.frombuffer(data, np.uint8)
        if rgb is not None:
            out["rgb_" + name] = rgb
    path = os.path.join(HERE, "jpeg_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
