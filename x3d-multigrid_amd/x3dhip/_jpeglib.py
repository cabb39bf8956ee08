"""ctypes binding of libx3djpeg.so (include/x3djpeg.h): the JPEG decoder (host parse + Huffman stage, the parallel
Huffman decoder on the device with its host-side scan preparation and CPU twin, IDCT and colour kernels, the frame store's
job builder and its CPU twin, the stage step of the store's host tier with its CPU twin, pinned memory).

Same discipline as _datalib.py: the library is mandatory, torch is imported before it is loaded, the ABI version and the
sizes of the mirrored structs are checked, and a failing entry point raises X3DHipError with the library's message.
"""
import ctypes
import os

import numpy as np

from ._lib import X3DHipError

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libx3djpeg.so")
ABI_VERSION = 2
SCAN_PAD = 16                # X3DJPEG_SCAN_PAD
SUB_BITS_DEFAULT = 1024      # X3DJPEG_SUB_BITS_DEFAULT
INDEX_BITS_DEFAULT = 512     # X3DJPEG_INDEX_BITS_DEFAULT
INDEX_MAX_BLOCKS = 1 << 22   # X3DJPEG_INDEX_MAX_BLOCKS

OK, EINVAL, ELAUNCH, EUNSUPPORTED, ECORRUPT, EINDEX = 0, -1, -2, -3, -4, -5

_P = ctypes.c_void_p
_I = ctypes.c_int
_Z = ctypes.c_size_t

# name -> (restype, argtypes).  Every symbol include/x3djpeg.h declares is listed here; tests/test_jpeg_host.py checks the
# two against each other and against the library's exports.
SIGNATURES = {
    "x3djpeg_abi_version": (_I, []),
    "x3djpeg_last_error": (ctypes.c_char_p, []),
    "x3djpeg_info_bytes": (_Z, []),
    "x3djpeg_frame_job_bytes": (_Z, []),
    "x3djpeg_scan_seg_bytes": (_Z, []),
    "x3djpeg_scan_job_bytes": (_Z, []),
    "x3djpeg_parse": (_I, [_P, _Z, _P]),
    "x3djpeg_entropy_decode": (_I, [_P, _Z, _P, _P, _Z]),
    "x3djpeg_scan_prepare": (_I, [_P, _Z, _P, _P, _Z, _P, _Z, _P, _P]),
    "x3djpeg_entropy_workspace_bytes": (_Z, [_Z, _Z, _I]),
    "x3djpeg_entropy_decode_parallel_host": (_I, [_P, _I, _I, _P, _Z, _P, _P]),
    "x3djpeg_entropy_decode_batch": (_I, [_P, _I, _I, _P, _Z, _P, _P]),
    "x3djpeg_idct": (_I, [_P, _I, _I, _P]),
    "x3djpeg_to_rgb": (_I, [_P, _I, _I, _I, _P]),
    "x3djpeg_decode_batch": (_I, [_P, _I, _I, _I, _I, _P]),
    "x3djpeg_store_header_bytes": (_Z, []),
    "x3djpeg_store_rec_bytes": (_Z, []),
    "x3djpeg_store_dst_bytes": (_Z, []),
    "x3djpeg_store_plan_bytes": (_Z, [_I]),
    "x3djpeg_store_build_jobs": (_I, [_P, _I, _P, _I, _P, _I, _I, _P, _Z, _P, _Z, _Z, _P, _P, _P, _P, _P, _P]),
    "x3djpeg_store_build_jobs_host": (_I, [_P, _I, _P, _I, _P, _I, _I, _P, _Z, _P, _Z, _Z, _P, _P, _P, _P, _P]),
    "x3djpeg_stage_bytes": (_Z, [_I, _I]),
    "x3djpeg_stage": (_I, [_P, _I, _P, _I, _Z, _P, _Z, _P, _P, _P, _P, _P]),
    "x3djpeg_stage_host": (_I, [_P, _I, _P, _I, _Z, _P, _Z, _P, _P, _P, _P]),
    "x3djpeg_pinned_alloc": (_I, [_Z, ctypes.POINTER(_P), ctypes.POINTER(_P)]),
    "x3djpeg_pinned_free": (_I, [_P]),
    "x3djpeg_index_rec_bytes": (_Z, []),
    "x3djpeg_index_count": (_Z, [_P, _Z, _I]),
    "x3djpeg_index_build": (_I, [_P, _Z, _P, _Z, _P, _I, _P, _Z, _P]),
    "x3djpeg_entropy_decode_indexed": (_I, [_P, _I, _P, _P, _I, _P, _Z, _I, _P, _P]),
    "x3djpeg_entropy_decode_indexed_host": (_I, [_P, _I, _P, _P, _I, _P, _Z, _I, _P]),
}

# X3DJpegInfo / X3DJpegFrameJob / X3DJpegScanSeg / X3DJpegScanJob of include/x3djpeg.h
INFO_DT = np.dtype([("width", "<i4"), ("height", "<i4"), ("ncomp", "<i4"), ("hmax", "<i4"), ("vmax", "<i4"),
                    ("mcus_x", "<i4"), ("mcus_y", "<i4"), ("restart_interval", "<i4"),
                    ("comp_h", "<i4", 3), ("comp_v", "<i4", 3), ("comp_tq", "<i4", 3), ("comp_td", "<i4", 3),
                    ("comp_ta", "<i4", 3), ("blocks_w", "<i4", 3), ("blocks_h", "<i4", 3), ("cw", "<i4", 3),
                    ("ch", "<i4", 3), ("block_start", "<i4", 3), ("nblocks", "<i4"),
                    ("coef_off", "<i8", 3), ("coef_count", "<i8"), ("scan_off", "<i8"),
                    ("qt", "<u2", (4, 64)), ("huff_bits", "u1", (8, 16)), ("huff_vals", "u1", (8, 256)),
                    ("qt_set", "u1", 4), ("huff_set", "u1", 8), ("pad", "u1", 4)], align=True)
FRAME_JOB_DT = np.dtype([("coef", "<u8"), ("planes", "<u8"), ("dst", "<u8"), ("dst_stride", "<i8"),
                         ("width", "<i4"), ("height", "<i4"), ("ncomp", "<i4"), ("hmax", "<i4"), ("vmax", "<i4"),
                         ("nblocks", "<i4"), ("blocks_w", "<i4", 3), ("blocks_h", "<i4", 3), ("cw", "<i4", 3),
                         ("ch", "<i4", 3), ("block_start", "<i4", 3), ("pad", "<i4", 3), ("qt", "<u2", (3, 64))])
SCAN_SEG_DT = np.dtype([("byte_off", "<u4"), ("byte_len", "<u4"), ("first_mcu", "<i4"), ("mcu_count", "<i4")])
SCAN_JOB_DT = np.dtype([("scan", "<u8"), ("segs", "<u8"), ("coef", "<u8"), ("coef_count", "<i8"), ("ws_off", "<i8"),
                        ("ws_bytes", "<i8"), ("scan_bytes", "<i4"), ("nseg", "<i4"), ("ncomp", "<i4"), ("mcus_x", "<i4"),
                        ("mcus_y", "<i4"), ("restart_interval", "<i4"), ("comp_h", "<i4", 3), ("comp_v", "<i4", 3),
                        ("comp_td", "<i4", 3), ("comp_ta", "<i4", 3), ("blocks_w", "<i4", 3), ("block_start", "<i4", 3),
                        ("huff_bits", "u1", (8, 16)), ("huff_vals", "u1", (8, 256))])
# X3DJpegStoreHeader / X3DJpegStoreRec / X3DJpegStoreDst of the frame store, and its constants
STORE_HEADER_DT = np.dtype([("frame", FRAME_JOB_DT), ("scan", SCAN_JOB_DT)])
STORE_REC_DT = np.dtype([("scan", "<u8"), ("segs", "<u8"), ("scan_bytes", "<i4"), ("nseg", "<i4"), ("header", "<i4"),
                         ("pad", "<i4")])
STORE_DST_DT = np.dtype([("dst", "<u8"), ("dst_stride", "<i8"), ("width", "<i4"), ("height", "<i4")])
STORE_BAD_ID, STORE_BAD_SIZE, STORE_NO_COEF, STORE_NO_WS = 1, 2, 4, 8
STORE_PLAN_THREADS, STORE_PLAN_CHUNK = 256, 1024
STAGE_BAD_ID, STAGE_NO_ROOM = 1, 2
# X3DJpegIndexRec of the sync index; an entry is two little-endian uint32 words (p, b | k << 3 | first block << 10)
INDEX_REC_DT = np.dtype([("first_entry", "<i8"), ("nentries", "<i4"), ("pad", "<i4")])
INDEX_ENTRY_BYTES = 8


def stage_bytes(scan_bytes, nseg):
    """x3djpeg_stage_bytes over numpy arrays: what a frame takes in a staging buffer."""
    return ((np.asarray(scan_bytes, np.int64) + SCAN_PAD + 15) & ~15) + np.asarray(nseg, np.int64) * SCAN_SEG_DT.itemsize

_lib = None


def lib():
    """Load (once) and return the ctypes handle; raises X3DHipError when unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise X3DHipError(
            "libx3djpeg.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C x3d-multigrid_amd/csrc_jpeg`). The JPEG input path has no fallback." % LIB_PATH)
    import torch  # noqa: F401  (its HIP runtime first: see _lib.lib)
    h = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(h, name)
        except AttributeError as e:
            raise X3DHipError("libx3djpeg.so lacks symbol %s (stale build?)" % name) from e
        fn.restype = res
        fn.argtypes = args
    v = h.x3djpeg_abi_version()
    if v != ABI_VERSION:
        raise X3DHipError("libx3djpeg.so ABI %d != expected %d" % (v, ABI_VERSION))
    if h.x3djpeg_info_bytes() != INFO_DT.itemsize or h.x3djpeg_frame_job_bytes() != FRAME_JOB_DT.itemsize:
        raise X3DHipError("libx3djpeg.so structs (%d, %d bytes) differ from the binding's (%d, %d)" % (
            h.x3djpeg_info_bytes(), h.x3djpeg_frame_job_bytes(), INFO_DT.itemsize, FRAME_JOB_DT.itemsize))
    if h.x3djpeg_scan_seg_bytes() != SCAN_SEG_DT.itemsize or h.x3djpeg_scan_job_bytes() != SCAN_JOB_DT.itemsize:
        raise X3DHipError("libx3djpeg.so scan structs (%d, %d bytes) differ from the binding's (%d, %d)" % (
            h.x3djpeg_scan_seg_bytes(), h.x3djpeg_scan_job_bytes(), SCAN_SEG_DT.itemsize, SCAN_JOB_DT.itemsize))
    if (h.x3djpeg_store_header_bytes() != STORE_HEADER_DT.itemsize or h.x3djpeg_store_rec_bytes() != STORE_REC_DT.itemsize
            or h.x3djpeg_store_dst_bytes() != STORE_DST_DT.itemsize):
        raise X3DHipError("libx3djpeg.so store structs (%d, %d, %d bytes) differ from the binding's (%d, %d, %d)" % (
            h.x3djpeg_store_header_bytes(), h.x3djpeg_store_rec_bytes(), h.x3djpeg_store_dst_bytes(),
            STORE_HEADER_DT.itemsize, STORE_REC_DT.itemsize, STORE_DST_DT.itemsize))
    if h.x3djpeg_index_rec_bytes() != INDEX_REC_DT.itemsize:
        raise X3DHipError("libx3djpeg.so index record (%d bytes) differs from the binding's (%d)" % (
            h.x3djpeg_index_rec_bytes(), INDEX_REC_DT.itemsize))
    _lib = h
    return h


def last_error():
    return lib().x3djpeg_last_error().decode("utf-8", "replace")


def check(rc):
    if rc != 0:
        raise X3DHipError("libx3djpeg: error %d: %s" % (rc, last_error()))


def parse(data, info=None):
    """x3djpeg_parse on a bytes object.  Returns (rc, info record, message); info is a 1-element INFO_DT array."""
    if info is None:
        info = np.zeros(1, dtype=INFO_DT)
    rc = lib().x3djpeg_parse(data, len(data), info.ctypes.data)
    return rc, info, (last_error() if rc else "")


def entropy_decode(data, info, coef_ptr, coef_bytes):
    """x3djpeg_entropy_decode into the int16 buffer at coef_ptr.  Returns (rc, message)."""
    rc = lib().x3djpeg_entropy_decode(data, len(data), info.ctypes.data, coef_ptr, coef_bytes)
    return rc, (last_error() if rc else "")


def segments_of(info):
    """Restart intervals of a parsed frame (INFO_DT record): the entries x3djpeg_scan_prepare writes."""
    ri, mcus = int(info["restart_interval"]), int(info["mcus_x"]) * int(info["mcus_y"])
    return -(-mcus // ri) if ri else 1


def scan_prepare(data, info):
    """x3djpeg_scan_prepare into fresh arrays.  Returns (rc, uint8 scan with its padding, SCAN_SEG_DT segments, message)."""
    i = info[0] if info.shape else info
    cap = len(data) - int(i["scan_off"]) + SCAN_PAD
    scan = np.zeros(max(cap, SCAN_PAD), np.uint8)
    segs = np.zeros(segments_of(i), SCAN_SEG_DT)
    out = np.zeros(2, np.uint64)
    rc = lib().x3djpeg_scan_prepare(data, len(data), info.ctypes.data, scan.ctypes.data, scan.size, segs.ctypes.data,
                                    segs.size, out.ctypes.data, out.ctypes.data + 8)
    if rc:
        return rc, None, None, last_error()
    assert int(out[1]) == segs.size
    return 0, scan[:int(out[0]) + SCAN_PAD], segs, ""


_SCAN_JOB_FIELDS = ("coef_count", "ncomp", "mcus_x", "mcus_y", "restart_interval", "comp_h", "comp_v", "comp_td", "comp_ta",
                    "blocks_w", "block_start", "huff_bits", "huff_vals")


def fill_scan_jobs(jobs, infos):
    """The fields of X3DJpegScanJob that come from X3DJpegInfo (everything but the pointers, sizes and workspace)."""
    for f in _SCAN_JOB_FIELDS:
        jobs[f] = infos[f]


def workspace_bytes(scan_bytes, nseg, sub_bits):
    n = lib().x3djpeg_entropy_workspace_bytes(int(scan_bytes), int(nseg), int(sub_bits))
    if n == 0:
        raise X3DHipError("libx3djpeg: sub_bits %r is not a multiple of 32, or the scan is too large" % (sub_bits,))
    return n


def entropy_decode_parallel_host(data, info, coef_ptr, sub_bits=SUB_BITS_DEFAULT):
    """Prepare + x3djpeg_entropy_decode_parallel_host of one frame into the int16 buffer at coef_ptr (coef_count elements).
    Returns (rc of prepare or the frame's status, relaxation rounds, subsequences, message)."""
    rc, scan, segs, msg = scan_prepare(data, info)
    if rc:
        return rc, 0, 0, msg
    job = np.zeros(1, SCAN_JOB_DT)
    fill_scan_jobs(job, info)
    ws = np.zeros(workspace_bytes(scan.size - SCAN_PAD, segs.size, sub_bits) // 8 + 2, np.uint64)
    base = (ws.ctypes.data + 15) & ~15
    job["scan"], job["segs"], job["coef"] = scan.ctypes.data, segs.ctypes.data, coef_ptr
    job["scan_bytes"], job["nseg"] = scan.size - SCAN_PAD, segs.size
    job["ws_off"], job["ws_bytes"] = 0, ws.nbytes - 16
    status, rounds = np.zeros(1, np.int32), np.zeros(1, np.int32)
    check(lib().x3djpeg_entropy_decode_parallel_host(job.ctypes.data, 1, sub_bits, base, ws.nbytes - 16,
                                                     status.ctypes.data, rounds.ctypes.data))
    head = np.frombuffer((ctypes.c_int32 * 2).from_address(base), np.int32)
    return int(status[0]), int(rounds[0]), int(head[1]), ""


def index_count(segs, index_bits):
    """x3djpeg_index_count of a SCAN_SEG_DT array: entries of the frame's sync index (0: index_bits is not taken)."""
    segs = np.ascontiguousarray(segs, SCAN_SEG_DT)
    return int(lib().x3djpeg_index_count(segs.ctypes.data, segs.size, int(index_bits)))


def index_build(scan, segs, info, index_bits):
    """x3djpeg_index_build of one prepared scan (uint8 with its padding, SCAN_SEG_DT segments, INFO_DT record).  Returns
    (rc, uint32 [n, 2] entries or None, message)."""
    segs = np.ascontiguousarray(segs, SCAN_SEG_DT)
    cap = index_count(segs, index_bits)
    entries = np.zeros(max(cap, 1), np.uint64)
    n = np.zeros(1, np.uint64)
    rc = lib().x3djpeg_index_build(scan.ctypes.data, scan.size - SCAN_PAD, segs.ctypes.data, segs.size, info.ctypes.data,
                                   int(index_bits), entries.ctypes.data, cap, n.ctypes.data)
    if rc:
        return rc, None, last_error()
    assert int(n[0]) == cap
    return 0, entries[:cap].view("<u4").reshape(cap, 2), ""
