"""What tests/test_jpeg_entropy_host.py and tests/test_jpeg_entropy_gpu.py share: the fixtures of the parallel Huffman
decoder (tests/golden/jpeg_entropy_cases.npz beside tests/golden/jpeg_cases.npz), a plain restatement of what
x3djpeg_scan_prepare does to a file, and the seeded damaged streams.  No test in here."""
import os

import numpy as np

from tests import jpeg_ref as jr

SUB_BITS = (32, 128, 1024)        # the smallest, one in between, X3DJPEG_SUB_BITS_DEFAULT
MUTATED = ("c420_64x48_restart", "c420_40x24_blocks1", "c444_48x40_q95_noise")
TRUNCATED = "c420_37x53_q75"


def load_entropy_cases():
    """{name: (jpeg bytes, Pillow's [H, W, 3] or None)} from tests/golden/jpeg_entropy_cases.npz, in file order."""
    z = np.load(os.path.join(jr.GOLDEN, "jpeg_entropy_cases.npz"))
    return {name: (z["jpg_" + name].tobytes(), z["rgb_" + name] if ("rgb_" + name) in z.files else None)
            for name in [str(n) for n in z["names"]]}


def good_cases():
    """{name: jpeg bytes}: every decodable case of both fixture files."""
    out = {k: v[0] for k, v in jr.load_cases().items() if v[1] is not None}
    out.update({k: v[0] for k, v in load_entropy_cases().items()})
    return out


def unstuff(data, scan_off, mcus, ri):
    """The entropy-coded data from scan_off on as x3djpeg_scan_prepare leaves it: (bytes without stuffing and restart
    markers, [(byte_off, byte_len, first_mcu, mcu_count)] per restart interval), or None where a restart marker that is due
    is missing.  Byte by byte, nothing shared with the library."""
    want = -(-mcus // ri) if ri else 1
    out, segs, pos = bytearray(), [], scan_off
    for s in range(want):
        start = len(out)
        while pos < len(data):
            if data[pos] != 0xFF:
                out.append(data[pos])
                pos += 1
            elif pos + 1 < len(data) and data[pos + 1] == 0x00:
                out.append(0xFF)
                pos += 2
            else:
                break
        segs.append((start, len(out) - start, s * ri, min(ri, mcus - s * ri) if ri else mcus))
        if s + 1 < want:
            while pos + 1 < len(data) and data[pos] == 0xFF and data[pos + 1] == 0xFF:
                pos += 1
            if data[pos:pos + 2] != bytes([0xFF, 0xD0 + (s & 7)]):
                return None
            pos += 2
    return bytes(out), segs


def scan_offset(data):
    i = data.index(b"\xff\xda")
    return i + 2 + ((data[i + 2] << 8) | data[i + 3])


def damaged(cases, per_case=200):
    """[(label, bytes)]: per_case single-byte changes inside the scan of each of MUTATED (seeded), and every truncation of
    TRUNCATED at 64-byte steps."""
    out = []
    for n, name in enumerate(MUTATED):
        data = cases[name]
        rng = np.random.default_rng(4100 + n)
        lo = scan_offset(data)
        for j in range(per_case):
            b = bytearray(data)
            at = int(rng.integers(lo, len(b) - 2))
            b[at] = (b[at] + int(rng.integers(1, 256))) & 255
            out.append(("%s/%d" % (name, j), bytes(b)))
    data = cases[TRUNCATED]
    out += [("%s[:%d]" % (TRUNCATED, n), data[:n]) for n in range(64, len(data), 64)]
    return out
