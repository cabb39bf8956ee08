"""What tests/test_jpeg_store_host.py and tests/test_jpeg_store_gpu.py share: a numpy restatement of the frame store's job
builder (x3djpeg_store_build_jobs / ..._host of include/x3djpeg.h) -- offsets by np.cumsum, fields by fill_jobs and
fill_scan_jobs -- the tables of a store built by hand in host memory, guarded buffers, and the request lists both files
run.  Nothing here goes through x3dhip.jpegstore or csrc_jpeg/store_core.h.  No test in here."""
import struct

import numpy as np

from tests import jpeg_entropy_cases as jc
from x3dhip import _jpeglib
from x3dhip._jpeglib import (FRAME_JOB_DT, INFO_DT, SCAN_JOB_DT, SCAN_PAD, STORE_DST_DT, STORE_HEADER_DT, STORE_REC_DT,
                             fill_scan_jobs)
from x3dhip.jpegops import fill_jobs

GUARD = 64          # bytes on either side of every output buffer
FILL = 0xA5


def aligned(nbytes, fill=0, guard=GUARD):
    """(whole, view): view is nbytes of uint8, 64-byte aligned, with `guard` bytes of FILL before and after it in whole."""
    whole = np.full(nbytes + 2 * guard + 64, FILL, np.uint8)
    at = guard + (-(whole.ctypes.data + guard) % 64)
    view = whole[at:at + nbytes]
    view[:] = fill
    return whole, view


def guards_intact(whole, view):
    at = view.ctypes.data - whole.ctypes.data
    return bool((whole[:at] == FILL).all() and (whole[at + view.size:] == FILL).all())


def workspace_bytes(scan_bytes, nseg, sub_bits):
    """x3djpeg_entropy_workspace_bytes, restated (csrc_jpeg/entropy_core.h: workspace_need)."""
    a16 = lambda v: (v + 15) & ~15                                          # noqa: E731
    nsub = np.asarray(scan_bytes, np.int64) * 8 // sub_bits + nseg
    return 16 + a16(4 * np.asarray(nseg, np.int64)) + a16(4 * nsub) + 2 * a16(8 * nsub) + a16(4 * nsub)


class Tables:
    """The three tables of a store over `files` (list of bytes), one record and one header per file, in host memory:
    recs, headers (numpy, 64-byte aligned), infos (INFO_DT per record), scan_bytes, nseg, and the arena that holds the
    prepared scans and segment tables."""

    def __init__(self, files):
        n = len(files)
        self.files, self.n = list(files), n
        self.infos = np.zeros(n, INFO_DT)
        parts, at, total = [], [], 0
        self.scan_bytes, self.nseg = np.zeros(n, np.int64), np.zeros(n, np.int64)
        for i, d in enumerate(files):
            rc, _, msg = _jpeglib.parse(d, self.infos[i:i + 1])
            assert rc == 0, msg
            rc, scan, segs, msg = _jpeglib.scan_prepare(d, self.infos[i:i + 1])
            assert rc == 0, msg
            self.scan_bytes[i], self.nseg[i] = scan.size - SCAN_PAD, segs.size
            for p in (scan.tobytes(), segs.tobytes()):
                total += -total % 16
                at.append(total)
                parts.append(p)
                total += len(p)
        self._arena_whole, self.arena = aligned(total)
        for a, p in zip(at, parts):
            self.arena[a:a + len(p)] = np.frombuffer(p, np.uint8)
        self._recs_whole, r = aligned(n * STORE_REC_DT.itemsize)
        self.recs = r.view(STORE_REC_DT)
        self.scan_at, self.seg_at = np.array(at[0::2], np.int64), np.array(at[1::2], np.int64)
        self.recs["scan"] = self.arena.ctypes.data + self.scan_at
        self.recs["segs"] = self.arena.ctypes.data + self.seg_at
        self.recs["scan_bytes"], self.recs["nseg"], self.recs["header"] = self.scan_bytes, self.nseg, np.arange(n)
        self._headers_whole, h = aligned(n * STORE_HEADER_DT.itemsize)
        self.headers = h.view(STORE_HEADER_DT)
        fill_jobs(self.headers["frame"], self.infos)
        fill_scan_jobs(self.headers["scan"], self.infos)


def restate(T, ids, dst, sub_bits, coef_base, planes_base, coef_cap=None, planes_cap=None, ws_cap=None,
            scan_base=None, seg_base=None):
    """The builder in numpy.  T: Tables (or anything with n, infos, scan_bytes, nseg, recs); ids: the requests; dst:
    STORE_DST_DT [n].  A capacity of None is the batch's own total.  Returns (scan jobs, frame jobs, plan int64 [3n + 2],
    build status).  scan_base / seg_base: per record, the addresses to expect (default: T.recs')."""
    ids = np.asarray(ids, np.int64)
    n = ids.size
    valid = (ids >= 0) & (ids < T.n)
    safe = np.where(valid, ids, 0)
    infos = T.infos[safe]
    counts = np.where(valid, infos["coef_count"], 0).astype(np.int64)
    ws = np.where(valid, workspace_bytes(T.scan_bytes[safe], T.nseg[safe], sub_bits), 0).astype(np.int64)
    coef_off = np.cumsum(counts) - counts
    ws_off = np.cumsum(ws) - ws
    coef_cap = int(counts.sum()) if coef_cap is None else coef_cap
    planes_cap = int(counts.sum()) if planes_cap is None else planes_cap
    ws_cap = int(ws.sum()) if ws_cap is None else ws_cap
    flags = np.where(valid, 0, _jpeglib.STORE_BAD_ID).astype(np.int64)
    flags |= np.where(valid & ((infos["width"] != dst["width"]) | (infos["height"] != dst["height"])), _jpeglib.STORE_BAD_SIZE, 0)
    flags |= np.where(valid & (coef_off + counts > min(coef_cap, planes_cap)), _jpeglib.STORE_NO_COEF, 0)
    flags |= np.where(valid & (ws_off + ws > ws_cap), _jpeglib.STORE_NO_WS, 0)
    fj = np.zeros(n, FRAME_JOB_DT)
    fill_jobs(fj, infos)
    fj["coef"] = coef_base + 2 * coef_off
    fj["planes"] = planes_base + coef_off
    fj["dst"], fj["dst_stride"] = dst["dst"], dst["dst_stride"]
    sj = np.zeros(n, SCAN_JOB_DT)
    fill_scan_jobs(sj, infos)
    sj["scan"] = (T.recs["scan"] if scan_base is None else scan_base)[safe]
    sj["segs"] = (T.recs["segs"] if seg_base is None else seg_base)[safe]
    sj["coef"] = fj["coef"]
    sj["ws_off"], sj["ws_bytes"] = ws_off, ws
    sj["scan_bytes"], sj["nseg"] = T.scan_bytes[safe], T.nseg[safe]
    fj[flags != 0] = np.zeros((), FRAME_JOB_DT)
    sj[flags != 0] = np.zeros((), SCAN_JOB_DT)
    plan = np.concatenate([coef_off, ws_off, flags, [counts.sum(), ws.sum()]]).astype(np.int64)
    return sj, fj, plan, int(np.bitwise_or.reduce(flags))


def dst_table(T, ids, base=0x7000000000, wider=()):
    """A destination table for the requests: frames one after the other from `base` on (addresses only: the builder never
    follows them); requests in `wider` ask for one pixel more than the frame has."""
    ids = np.asarray(ids, np.int64)
    ok = (ids >= 0) & (ids < T.n)
    info = T.infos[np.where(ok, ids, 0)]
    d = np.zeros(ids.size, STORE_DST_DT)
    d["width"], d["height"] = np.where(ok, info["width"], 8), np.where(ok, info["height"], 8)
    size = 3 * (d["width"].astype(np.int64) + 1) * d["height"]            # room for the wider ones: the same addresses
    d["dst"] = base + np.cumsum(size) - size
    for i in wider:
        d["width"][i] += 1
    d["dst_stride"] = 3 * d["width"].astype(np.int64)
    return d


def twin(T, ids, dst, sub_bits, coef_base, planes_base, coef_cap, planes_cap, ws_cap):
    """x3djpeg_store_build_jobs_host into guarded buffers pre-filled with 0x3C.  Returns (scan jobs, frame jobs, plan,
    build status); asserts the guards."""
    n = len(ids)
    idv = np.asarray(ids, np.int32).copy()
    bufs = [aligned(n * SCAN_JOB_DT.itemsize, 0x3C), aligned(n * FRAME_JOB_DT.itemsize, 0x3C), aligned(8 * (3 * n + 2), 0x3C),
            aligned(4, 0x3C)]
    dwhole, dv = aligned(dst.nbytes)
    dv[:] = dst.view(np.uint8).reshape(-1)
    rc = _jpeglib.lib().x3djpeg_store_build_jobs_host(
        T.recs.ctypes.data, T.n, T.headers.ctypes.data, len(T.headers), idv.ctypes.data, n, sub_bits, coef_base, coef_cap,
        planes_base, planes_cap, ws_cap, dv.ctypes.data, bufs[2][1].ctypes.data, bufs[0][1].ctypes.data,
        bufs[1][1].ctypes.data, bufs[3][1].ctypes.data)
    assert rc == 0, _jpeglib.last_error()
    for whole, view in bufs:
        assert guards_intact(whole, view), "guard overwritten"
    return (bufs[0][1].view(SCAN_JOB_DT).copy(), bufs[1][1].view(FRAME_JOB_DT).copy(), bufs[2][1].view(np.int64).copy(),
            int(bufs[3][1].view(np.int32)[0]))


# --------------------------------------------------------------------------- the request lists
def good_files():
    """Every good case of both fixture files, in their order: (names, files)."""
    g = jc.good_cases()
    return list(g), list(g.values())


def served_lists(n):
    """Request lists over a store of n frames that are served in full: in order, scrambled, with repeats, one alone."""
    rng = np.random.default_rng(611)
    return {"in_order": list(range(n)), "scrambled": [int(i) for i in rng.permutation(n)],
            "repeats": [int(i) for i in rng.integers(0, n, 2 * n)], "one": [n // 2]}


REFUSED_NAMES = ("c420_37x53_q75", "c420_64x48_restart", "c420_120x90_q50", "c420_40x24_blocks1", "vid_05")


def refused_lists(names):
    """The five-request lists with one thing wrong each: {label: (ids, wider, coef_short, ws_short, status bit, refused
    requests)}.  coef_short / ws_short: the request whose coefficients / workspace the capacity is one element short of
    (None: the capacity is the total) -- what comes after it does not fit either."""
    a, b, c, d, e = [names.index(k) for k in REFUSED_NAMES]
    B, n = _jpeglib, len(names)
    return {"id_minus_1": ([a, -1, c, d, e], (), None, None, B.STORE_BAD_ID, (1,)),
            "id_nrecs": ([a, b, c, n, e], (), None, None, B.STORE_BAD_ID, (3,)),
            "wider": ([a, b, c, d, e], (2,), None, None, B.STORE_BAD_SIZE, (2,)),
            "coef_short": ([a, b, c, d, e], (), 2, None, B.STORE_NO_COEF, (2, 3, 4)),
            "ws_short": ([a, b, c, d, e], (), None, 2, B.STORE_NO_WS, (2, 3, 4))}


def write_check_input(path, files, lists, sub_bits):
    """The input of tests/jpeg_store_check.cpp: the files, then per list n, sub_bits, coef_short, ws_short (-1: none),
    the expected build status and n pairs (id, extra width)."""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(files)))
        for b in files:
            f.write(struct.pack("<I", len(b)))
            f.write(b)
        f.write(struct.pack("<I", len(lists)))
        for ids, wider, coef_short, ws_short, status in lists:
            f.write(struct.pack("<iiiii", len(ids), sub_bits, -1 if coef_short is None else coef_short,
                                -1 if ws_short is None else ws_short, status))
            for i, v in enumerate(ids):
                f.write(struct.pack("<ii", v, 1 if i in wider else 0))
