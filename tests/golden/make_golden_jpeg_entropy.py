"""Writes tests/golden/jpeg_entropy_cases.npz: JPEG files (as uint8 arrays) for the parallel Huffman decoder, the fixtures
of tests/test_jpeg_entropy_host.py and tests/test_jpeg_entropy_gpu.py.  Needs Pillow only; run it again only to add a case.

    python tests/golden/make_golden_jpeg_entropy.py

Per case jpg_<name> (the file's bytes); rgb_<name> (Pillow's decode) for the two small cases only: the others are compared
with the host decoder, which tests/test_jpeg_host.py pins to Pillow.  The cases are chosen for what they do to a decoder
that starts in the middle of the stream, and the properties they are chosen for are asserted here, so that another
Pillow cannot hollow them out:

    c420_340x256_q75        more subsequences than the workgroup has threads at the default sub_bits, stuffed bytes
    c420_340x256_q75_rows   the same image, a restart marker per MCU row (15 markers)
    c420_320x240_q5         nearly every block is DC + end-of-block
    c422_161x99_optimize    its own Huffman tables
    grey_200x150            one component
    flat_512x512            a strictly periodic stream, 32 bits per MCU: a decoder that started in a wrong state would
                            never leave it (here every multiple of 32 bits is an MCU boundary, so the guesses are right)
    c420_40x24_blocks1      a restart marker after every MCU: every segment shorter than a subsequence
    c444_48x40_q95_noise    long codes, 4:4:4
"""
import os

import numpy as np
import PIL
from PIL import features

from make_golden_jpeg import content, encode, pillow

HERE = os.path.dirname(os.path.abspath(__file__))
SUB_BITS = 1024          # X3DJPEG_SUB_BITS_DEFAULT
THREADS = 256            # the kernel's workgroup


def scan_stats(data):
    """(segment byte lengths after unstuffing, stuffed bytes, restart markers) of a baseline file with one scan."""
    i = data.index(b"\xff\xda")
    i += 2 + ((data[i + 2] << 8) | data[i + 3])
    segs, cur, stuffed, rst = [], 0, 0, 0
    while i < len(data):
        if data[i] != 0xFF:
            cur += 1
            i += 1
        elif data[i + 1] == 0x00:
            cur += 1
            stuffed += 1
            i += 2
        elif 0xD0 <= data[i + 1] <= 0xD7:
            segs.append(cur)
            cur, rst, i = 0, rst + 1, i + 2
        else:
            break
    segs.append(cur)
    return segs, stuffed, rst


def nsub(segs, sub_bits=SUB_BITS):
    return sum(max(1, -(-8 * n // sub_bits)) for n in segs)


def main():
    S444, S422, S420 = 0, 1, 2
    cases = []

    def add(name, data, rgb=False):
        cases.append((name, data, pillow(data) if rgb else None))
        return scan_stats(data)

    big = content(340, 256, 21, sigma=12.0)
    segs, stuffed, rst = add("c420_340x256_q75", encode(big, quality=75, subsampling=S420))
    assert len(segs) == 1 and rst == 0 and stuffed > 0 and nsub(segs) > THREADS, (segs, stuffed)
    segs, stuffed, rst = add("c420_340x256_q75_rows", encode(big, quality=75, subsampling=S420, restart_marker_rows=1))
    assert rst == 15 and len(segs) == 16 and stuffed > 0 and nsub(segs) > THREADS, (rst, stuffed)
    segs, stuffed, rst = add("c420_320x240_q5", encode(content(320, 240, 22, sigma=3.0), quality=5, subsampling=S420))
    assert rst == 0 and 8 * segs[0] < 24 * 6 * 300 and nsub(segs) >= 8, segs     # under 24 bits a block: 300 MCUs of 6
    segs, stuffed, rst = add("c422_161x99_optimize", encode(content(161, 99, 23), quality=85, subsampling=S422, optimize=True))
    assert rst == 0 and nsub(segs) >= 32, segs
    segs, stuffed, rst = add("grey_200x150", encode(content(200, 150, 24)[..., 0], mode="L", quality=85))
    assert rst == 0 and nsub(segs) >= 32, segs
    flat = np.full((512, 512, 3), 128, np.uint8)
    segs, stuffed, rst = add("flat_512x512", encode(flat, quality=75, subsampling=S420))
    assert rst == 0 and stuffed == 0 and segs[0] in (4096, 4097) and nsub(segs) >= 32, segs   # 32 bits per MCU
    segs, stuffed, rst = add("c420_40x24_blocks1", encode(content(40, 24, 25), quality=80, subsampling=S420,
                                                          restart_marker_blocks=1), rgb=True)
    assert rst == 5 and len(segs) == 6 and max(segs) * 8 <= SUB_BITS and nsub(segs) == 6, segs
    segs, stuffed, rst = add("c444_48x40_q95_noise", encode(content(48, 40, 26, sigma=60.0), quality=95, subsampling=S444),
                             rgb=True)
    assert rst == 0 and stuffed > 0 and nsub(segs) >= 32, (segs, stuffed)

    out = {"names": np.array([c[0] for c in cases]), "pillow": np.array(PIL.__version__),
           "libjpeg": np.array(str(features.version("jpg")))}
    for name, data, rgb in cases:
        out["jpg_" + name] = np.frombuffer(data, np.uint8)
        if rgb is not None:
            out["rgb_" + name] = rgb
        segs, stuffed, rst = scan_stats(data)
        print("%-24s %6d bytes  scan %6d  stuffed %4d  RST %3d  subsequences %4d" % (
            name, len(data), sum(segs), stuffed, rst, nsub(segs)))
    path = os.path.join(HERE, "jpeg_entropy_cases.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 200 * 1024, size
    print(path, size, "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
