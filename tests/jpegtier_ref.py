"""What tests/test_jpeg_tier_host.py and tests/test_jpeg_tier_gpu.py share: a numpy restatement of the stage plan of the
frame store's host tier (x3djpeg_stage / x3djpeg_stage_host of include/x3djpeg.h) -- offsets by np.cumsum, flags, staged
records and ids -- the twin's call into guarded buffers, and the request lists both files run.  Nothing here goes through
x3dhip.jpegstore or csrc_jpeg/stage_core.h.  No test in here."""
import json
import os
import struct

import numpy as np

from tests import jpegstore_ref as sr
from x3dhip import _jpeglib
from x3dhip._jpeglib import SCAN_PAD, STORE_REC_DT

NS = (1, 2, 257, 1025, 2051)        # one pass, two passes, a third pass with a carry and a partial tail


def a16(v):
    return (np.asarray(v, np.int64) + 15) & ~15


def frame_bytes(scan_bytes, nseg):
    """x3djpeg_stage_bytes, restated: the scan and its padding rounded up to 16, then 16 bytes per segment."""
    return a16(np.asarray(scan_bytes, np.int64) + SCAN_PAD) + 16 * np.asarray(nseg, np.int64)


def restate(recs, ids, cap=None, max_frame=None, staging_base=0):
    """The stage plan in numpy.  recs: STORE_REC_DT array; ids: the requests; cap: the staging capacity (None: the total);
    max_frame: max_frame_bytes (None: the largest frame of recs).  Returns (staged recs, staged ids int32, offsets int64
    [n + 1], status)."""
    ids = np.asarray(ids, np.int64)
    n = ids.size
    valid = (ids >= 0) & (ids < len(recs))
    r = recs[np.where(valid, ids, 0)]
    size = frame_bytes(r["scan_bytes"], r["nseg"])
    max_frame = int(frame_bytes(recs["scan_bytes"], recs["nseg"]).max()) if max_frame is None else max_frame
    flags = np.where(valid, 0, _jpeglib.STAGE_BAD_ID)
    flags = np.where(valid & (size > max_frame), _jpeglib.STAGE_NO_ROOM, flags)
    asked = np.where(flags == 0, size, 0)
    off = np.cumsum(asked) - asked
    cap = int(asked.sum()) if cap is None else cap
    flags = np.where((flags == 0) & (off + asked > cap), _jpeglib.STAGE_NO_ROOM, flags)
    served = flags == 0
    staged = np.where(served, asked, 0)
    offsets = np.concatenate([np.cumsum(staged) - staged, [staged.sum()]]).astype(np.int64)
    # a request without room is followed by none that is served: the served ones lie without a gap
    assert np.array_equal(offsets[:-1][served], off[served])
    out = np.zeros(n, STORE_REC_DT)
    out["scan"] = np.where(served, staging_base + off, 0)
    out["segs"] = np.where(served, staging_base + off + a16(r["scan_bytes"].astype(np.int64) + SCAN_PAD), 0)
    for f in ("scan_bytes", "nseg", "header"):
        out[f] = np.where(served, r[f], 0)
    return out, np.where(served, np.arange(n), -1).astype(np.int32), offsets, int(np.bitwise_or.reduce(flags))


def twin(recs, ids, cap, max_frame, room=None):
    """x3djpeg_stage_host into guarded buffers pre-filled with 0x3C.  recs must be 16-byte aligned host memory.  room: the
    bytes of the staging buffer (default cap).  Returns (staged recs, staged ids, offsets, status, staging); asserts the
    guards."""
    n = len(ids)
    idv = np.asarray(ids, np.int32).copy()
    room = cap if room is None else room
    bufs = [sr.aligned(n * STORE_REC_DT.itemsize, 0x3C), sr.aligned(4 * n, 0x3C), sr.aligned(8 * (n + 1), 0x3C),
            sr.aligned(4, 0x3C), sr.aligned(max(room, 16), 0x3C)]
    rc = _jpeglib.lib().x3djpeg_stage_host(recs.ctypes.data, len(recs), idv.ctypes.data, n, max_frame, bufs[4][1].ctypes.data,
                                           cap, bufs[0][1].ctypes.data, bufs[1][1].ctypes.data, bufs[2][1].ctypes.data,
                                           bufs[3][1].ctypes.data)
    assert rc == 0, _jpeglib.last_error()
    for whole, view in bufs:
        assert sr.guards_intact(whole, view), "guard overwritten"
    return (bufs[0][1].view(STORE_REC_DT), bufs[1][1].view(np.int32), bufs[2][1].view(np.int64),
            int(bufs[3][1].view(np.int32)[0]), bufs[4][1])


def source_bytes(read, recs, i):
    """What request for frame i must leave in the staging buffer: read(address, nbytes) -> uint8 array gives arena bytes."""
    sb, ns = int(recs["scan_bytes"][i]), int(recs["nseg"][i])
    out = np.zeros(int(frame_bytes(sb, ns)), np.uint8)
    out[:sb + SCAN_PAD] = read(int(recs["scan"][i]), sb + SCAN_PAD)
    out[int(a16(sb + SCAN_PAD)):] = read(int(recs["segs"][i]), 16 * ns)
    return out


def lists(nrecs, seed=612):
    """Request lists over nrecs frames: the four orders of jpegstore_ref.served_lists, each frame alone, and random ids at
    every n of NS."""
    rng = np.random.default_rng(seed)
    out = dict(sr.served_lists(nrecs))
    for i in range(nrecs):
        out["alone_%d" % i] = [i]
    for n in NS:
        out["n_%d" % n] = [int(i) for i in rng.integers(0, nrecs, n)]
    return out


def write_check_input(path, files, runs):
    """The input of tests/jpeg_tier_check.cpp: the files, then per run n, the request the capacity is one byte short of
    (-1: the capacity is the total), the expected stage status and the n ids."""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(files)))
        for b in files:
            f.write(struct.pack("<I", len(b)))
            f.write(b)
        f.write(struct.pack("<I", len(runs)))
        for ids, short, status in runs:
            f.write(struct.pack("<iii", len(ids), -1 if short is None else short, status))
            f.write(np.asarray(ids, "<i4").tobytes())


# --------------------------------------------------------------------------- a small Kinetics tree
TREE = (("class a", "vidA", 24, 64, 80), ("class b", "vidB", 40, 80, 64), ("class a", "vidC", 31, 80, 64),
        ("class c", "vidD", 27, 64, 80))                   # label, video id, frames, width, height
TREE_LABELS = ["c0", "class a", "c2", "class b", "class c"]
MIN_FRAMES = 16     # the listing skips folders of 81 frames or fewer: the tests lower frames.MIN_FRAMES to this


def write_tree(tmp, subset, tree=TREE, name=None):
    """The reference's layout for `subset` ('train' or 'validate') under tmp/name: the videos of `tree` (four of two sizes),
    smooth moving gradients written with Pillow (baseline, 4:2:0, quality 75).  Returns (root, annotation path, labels
    path)."""
    from PIL import Image
    root = os.path.join(str(tmp), name or subset)
    anno = {}
    for v, (label, vid, n, w, h) in enumerate(tree):
        name = vid + "_000000_000010" if subset == "train" else vid
        path = os.path.join(root, label.replace(" ", "_"), name)
        os.makedirs(path)
        y, x = np.mgrid[0:h, 0:w]
        for t in range(n):
            rgb = np.stack([(x * 3 + 5 * t + 40 * v) % 256, (y * 2 + 3 * t) % 256, ((x + y) * 2 + 7 * t) % 256], axis=2)
            Image.fromarray(rgb.astype(np.uint8)).save(os.path.join(path, "frame_%05d.jpg" % (t + 1)), quality=75)
        anno[vid] = {"subset": subset, "annotations": {"label": label, "segment": [0, 10]}}
    anno["other"] = {"subset": "testing"}
    anno_path, labels_path = os.path.join(str(tmp), (name or subset) + ".json"), os.path.join(str(tmp), "labels.txt")
    with open(anno_path, "w") as f:
        json.dump(anno, f)
    with open(labels_path, "w") as f:
        f.write("\n".join(TREE_LABELS) + "\n")
    return root, anno_path, labels_path
