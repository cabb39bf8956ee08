"""Numpy restatement (int64) of baseline JPEG decoding as Pillow's bundled libjpeg-turbo does it: marker parsing, Huffman
decoding bit by bit, dequantisation, the "islow" integer IDCT, "fancy" chroma upsampling and the YCbCr -> RGB conversion.
The reference of the tests of libx3djpeg.so (include/x3djpeg.h); tests/test_jpeg_host.py pins it to Pillow bit for bit.

Slow and plain on purpose.  `track` (a dict) collects the largest |dequantised coefficient| and |IDCT intermediate|.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7,
                   14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46,
                   53, 60, 61, 54, 47, 55, 62, 63])          # zigzag position -> natural (row-major) position


class Unsupported(Exception):
    pass


class Corrupt(Exception):
    pass


def load_cases():
    """{name: (jpeg bytes, Pillow's [H, W, 3] or None for a reject)} from tests/golden/jpeg_cases.npz, in file order."""
    z = np.load(os.path.join(GOLDEN, "jpeg_cases.npz"))
    out = {}
    for name in [str(n) for n in z["names"]]:
        out[name] = (z["jpg_" + name].tobytes(), z["rgb_" + name] if ("rgb_" + name) in z.files else None)
    return out


def parse(data):
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise Corrupt("no SOI")
    pos = 2
    qt, huff, info = {}, {}, dict(restart_interval=0)
    adobe = None
    while True:
        if pos + 4 > len(data):
            raise Corrupt("ran out of markers")
        if data[pos] != 0xFF:
            raise Corrupt("marker expected")
        m = data[pos + 1]
        if m == 0xFF:
            pos += 1
            continue
        L = (data[pos + 2] << 8) | data[pos + 3]
        seg = data[pos + 4:pos + 2 + L]
        if L < 2 or len(seg) != L - 2:
            raise Corrupt("segment length")
        pos += 2 + L
        if m == 0xDB:
            i = 0
            while i < len(seg):
                pq, tq = seg[i] >> 4, seg[i] & 15
                i += 1
                if pq:
                    vals = [(seg[i + 2 * k] << 8) | seg[i + 2 * k + 1] for k in range(64)]
                    i += 128
                else:
                    vals = list(seg[i:i + 64])
                    i += 64
                t = np.zeros(64, np.int64)
                t[ZIGZAG] = vals
                qt[tq] = t
        elif m in (0xC0, 0xC1):
            if seg[0] != 8:
                raise Unsupported("12-bit samples")
            info["height"], info["width"] = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4]
            n = seg[5]
            if n not in (1, 3):
                raise Unsupported("%d components" % n)
            info["comps"] = [dict(id=seg[6 + 3 * c], h=seg[7 + 3 * c] >> 4, v=seg[7 + 3 * c] & 15, tq=seg[8 + 3 * c])
                             for c in range(n)]
        elif m == 0xC2:
            raise Unsupported("progressive")
        elif 0xC3 <= m <= 0xCF and m not in (0xC4, 0xC8):
            raise Unsupported("SOF%d" % (m - 0xC0))
        elif m == 0xC4:
            i = 0
            while i < len(seg):
                tc, th = seg[i] >> 4, seg[i] & 15
                bits = list(seg[i + 1:i + 17])
                n = sum(bits)
                huff[(tc, th)] = (bits, list(seg[i + 17:i + 17 + n]))
                i += 17 + n
        elif m == 0xDD:
            info["restart_interval"] = (seg[0] << 8) | seg[1]
        elif m == 0xEE and seg[:5] == b"Adobe" and len(seg) >= 12:
            adobe = seg[11]
        elif m == 0xDA:
            ns = seg[0]
            if "comps" not in info:
                raise Corrupt("SOS before SOF")
            if ns != len(info["comps"]):
                raise Unsupported("multi-scan")
            for c in range(ns):
                info["comps"][c]["td"], info["comps"][c]["ta"] = seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15
            break
    comps = info["comps"]
    if len(comps) == 1:
        comps[0]["h"] = comps[0]["v"] = 1
    elif adobe is not None and adobe != 1:
        raise Unsupported("Adobe transform %d" % adobe)
    elif (comps[0]["h"], comps[0]["v"]) not in ((1, 1), (2, 1), (2, 2)) or any((c["h"], c["v"]) != (1, 1) for c in comps[1:]):
        raise Unsupported("sampling factors")
    W, H = info["width"], info["height"]
    hmax, vmax = comps[0]["h"], comps[0]["v"]
    info["hmax"], info["vmax"] = hmax, vmax
    info["mcus_x"], info["mcus_y"] = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    for c in comps:
        c["blocks_w"], c["blocks_h"] = info["mcus_x"] * c["h"], info["mcus_y"] * c["v"]
        c["cw"], c["ch"] = -(-W * c["h"] // hmax), -(-H * c["v"] // vmax)
    info["qt"], info["huff"], info["scan_off"] = qt, huff, pos
    return info


class _Bits:
    def __init__(self, data, pos):
        self.d, self.p, self.acc, self.n = data, pos, 0, 0

    def bit(self):
        if self.n == 0:
            if self.p >= len(self.d):
                raise Corrupt("out of data")
            b = self.d[self.p]
            self.p += 1
            if b == 0xFF:
                if self.p >= len(self.d) or self.d[self.p] != 0:
                    raise Corrupt("marker inside the scan")
                self.p += 1
            self.acc, self.n = b, 8
        self.n -= 1
        return (self.acc >> self.n) & 1

    def bits(self, k):
        v = 0
        for _ in range(k):
            v = (v << 1) | self.bit()
        return v

    def restart(self, k):
        self.n = 0
        if self.d[self.p:self.p + 2] != bytes([0xFF, 0xD0 + (k & 7)]):
            raise Corrupt("restart marker expected")
        self.p += 2


def _codes(bits, vals):
    table, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            table[(ln, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return table


def _sym(br, table):
    code = 0
    for ln in range(1, 17):
        code = (code << 1) | br.bit()
        s = table.get((ln, code))
        if s is not None:
            return s
    raise Corrupt("bad Huffman code")


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def entropy_decode(data, info):
    """int16 coefficients in natural order, per component [blocks_h, blocks_w, 64]."""
    data = bytes(data)
    comps = info["comps"]
    out = [np.zeros((c["blocks_h"], c["blocks_w"], 64), np.int16) for c in comps]
    tabs = {k: _codes(*v) for k, v in info["huff"].items()}
    br = _Bits(data, info["scan_off"])
    pred = [0] * len(comps)
    ri, n = info["restart_interval"], 0
    for my in range(info["mcus_y"]):
        for mx in range(info["mcus_x"]):
            if ri and n and n % ri == 0:
                br.restart(n // ri - 1)
                pred = [0] * len(comps)
            n += 1
            for ci, c in enumerate(comps):
                dc, ac = tabs[(0, c["td"])], tabs[(1, c["ta"])]
                for by in range(c["v"]):
                    for bx in range(c["h"]):
                        blk = out[ci][my * c["v"] + by, mx * c["h"] + bx]
                        s = _sym(br, dc)
                        pred[ci] += _extend(br.bits(s), s)
                        blk[0] = pred[ci]
                        k = 1
                        while k < 64:
                            rs = _sym(br, ac)
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r != 15:
                                    break
                                k += 16
                                continue
                            k += r
                            if k > 63:
                                raise Corrupt("coefficient index past 63")
                            blk[ZIGZAG[k]] = _extend(br.bits(s), s)
                            k += 1
    return out


def _fix(x):
    return int(x * 8192 + 0.5)


F_0_298, F_0_390, F_0_541, F_0_765, F_0_899, F_1_175 = (_fix(x) for x in (0.298631336, 0.390180644, 0.541196100,
                                                                          0.765366865, 0.899976223, 1.175875602))
F_1_501, F_1_847, F_1_961, F_2_053, F_2_562, F_3_072 = (_fix(x) for x in (1.501321110, 1.847759065, 1.961570560,
                                                                          2.053119869, 2.562915447, 3.072711026))


def _pass(v, first, track):
    """One 1-D pass of jidctint.c over the second-to-last axis of v [..., 8, n] (int64)."""
    i0, i1, i2, i3, i4, i5, i6, i7 = (v[..., k, :] for k in range(8))
    z1 = (i2 + i6) * F_0_541
    t2 = z1 - i6 * F_1_847
    t3 = z1 + i2 * F_0_765
    t0 = (i0 + i4) * 8192
    t1 = (i0 - i4) * 8192
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o0, o1, o2, o3 = i7, i5, i3, i1
    z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
    z5 = (z3 + z4) * F_1_175
    o0, o1, o2, o3 = o0 * F_0_298, o1 * F_2_053, o2 * F_3_072, o3 * F_1_501
    z1, z2, z3, z4 = -z1 * F_0_899, -z2 * F_2_562, -z3 * F_1_961 + z5, -z4 * F_0_390 + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    sh = 11 if first else 18
    sums = [t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3]
    if track is not None:
        for a in (z5, t0, t1, t2, t3, o0, o1, o2, o3, *sums):
            track["idct"] = max(track.get("idct", 0), int(np.abs(a).max(initial=0)) + (1 << (sh - 1)))
    return np.stack([(s + (1 << (sh - 1))) >> sh for s in sums], axis=-2)


def idct_plane(coef, q, track=None):
    """coef int16 [bh, bw, 64] natural order, q [64] -> the uint8 plane [bh * 8, bw * 8]."""
    bh, bw, _ = coef.shape
    d = coef.astype(np.int64) * np.asarray(q, np.int64)
    if track is not None:
        track["dequant"] = max(track.get("dequant", 0), int(np.abs(d).max(initial=0)))
    d = d.reshape(bh, bw, 8, 8)
    ws = _pass(d, True, track)                                        # columns: along the row index
    out = _pass(ws.swapaxes(-1, -2), False, track).swapaxes(-1, -2)     # rows
    out = np.clip(out + 128, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(out.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8))


def upsample(c, hs, vs):
    """c int [ch, cw] (the component's true size) -> [ch * vs, cw * hs], libjpeg's fancy filter (plain replication when
    cw <= 2)."""
    c = c.astype(np.int64)
    ch, cw = c.shape
    if hs == 1 and vs == 1:
        return c
    if cw <= 2:
        return np.repeat(np.repeat(c, vs, axis=0), hs, axis=1)
    if vs == 1:
        prev = np.concatenate([c[:, :1], c[:, :-1]], axis=1)
        nxt = np.concatenate([c[:, 1:], c[:, -1:]], axis=1)
        out = np.empty((ch, cw * 2), np.int64)
        out[:, 0::2] = (3 * c + prev + 1) >> 2
        out[:, 1::2] = (3 * c + nxt + 2) >> 2
        return out
    up = np.concatenate([c[:1], c[:-1]], axis=0)
    dn = np.concatenate([c[1:], c[-1:]], axis=0)
    s = np.empty((ch * 2, cw), np.int64)
    s[0::2] = 3 * c + up
    s[1::2] = 3 * c + dn
    prev = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
    nxt = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
    out = np.empty((ch * 2, cw * 2), np.int64)
    out[:, 0::2] = (3 * s + prev + 8) >> 4
    out[:, 1::2] = (3 * s + nxt + 7) >> 4
    return out


def _g(x):
    return int(x * 65536 + 0.5)


def to_rgb(planes, W, H, hmax, vmax):
    """planes: uint8 arrays at least the component's true size (block padded planes are fine) -> uint8 [H, W, 3]."""
    y = planes[0][:H, :W].astype(np.int64)
    if len(planes) == 1:
        return np.stack([y, y, y], axis=-1).astype(np.uint8)
    cw, ch = -(-W // hmax), -(-H // vmax)
    cb = upsample(planes[1][:ch, :cw], hmax, vmax)[:H, :W] - 128
    cr = upsample(planes[2][:ch, :cw], hmax, vmax)[:H, :W] - 128
    r = y + ((_g(1.402) * cr + 32768) >> 16)
    b = y + ((_g(1.772) * cb + 32768) >> 16)
    g = y + ((-_g(0.34414) * cb - _g(0.71414) * cr + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def planes_of(data, track=None):
    info = parse(data)
    coefs = entropy_decode(data, info)
    return info, coefs, [idct_plane(k, info["qt"][c["tq"]], track) for k, c in zip(coefs, info["comps"])]


def decode(data, track=None):
    info, _, planes = planes_of(data, track)
    return to_rgb(planes, info["width"], info["height"], info["hmax"], info["vmax"])
