"""The host tier and the pack files of the frame store, checks that need no GPU: x3djpeg_stage_host (the stage kernels' code,
run serially) against the numpy restatement of tests/jpegtier_ref.py byte for byte inside guard bytes; the refusals; the
staged tables taken through the job builder's twin and decoded on the CPU; the same lists once more in a stand-alone program
built with the address and undefined-behaviour sanitisers; the C ABI; FrameStore.save / load on a store kept in host
memory, with the files load must refuse; jpegops.HostStages, through which a store is filled, on its own without a GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import jpegstore_ref as sr
from tests import jpegtier_ref as tr
from tests.test_jpeg_store_host import HostMemory
from x3dhip import _jpeglib
from x3dhip._jpeglib import SCAN_PAD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES, FILES = sr.good_files()
SUB_BITS = 128
_T = {}


def _lib():
    if not os.path.exists(_jpeglib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _jpeglib.lib()


def _tables():
    if "t" not in _T:
        _lib()
        _T["t"] = sr.Tables(FILES)
    return _T["t"]


def _reader(T):
    base = T.arena.ctypes.data
    return lambda addr, nbytes: T.arena[addr - base:addr - base + nbytes]


def _check_staging(T, ids, got, read=None, recs=None):
    """The staged bytes of every served request are its source's with zero tails, and nothing else was written."""
    srecs, sids, offsets, status, staging = got
    read, recs = read or _reader(T), T.recs if recs is None else recs
    total = int(offsets[-1])
    for k, i in enumerate(ids):
        if sids[k] < 0:
            continue
        want = tr.source_bytes(read, recs, i)
        at = int(offsets[k])
        assert staging[at:at + want.size].tobytes() == want.tobytes(), (k, i)
    assert (staging[total:] == 0x3C).all()                  # no byte at or after the total


def _stage(T, ids, short=None, max_frame=None):
    """The twin and the restatement on one list; short: the request whose end the capacity is one byte short of."""
    size = tr.frame_bytes(T.recs["scan_bytes"], T.recs["nseg"])
    max_frame = int(size.max()) if max_frame is None else max_frame
    ok = [i for i in ids if 0 <= i < T.n]
    total = int(size[ok].sum())
    cap = total if short is None else int(size[[i for i in ids[:short + 1] if 0 <= i < T.n]].sum()) - 1
    got = tr.twin(T.recs, ids, cap, max_frame, room=total)
    want = tr.restate(T.recs, ids, cap, max_frame, staging_base=got[4].ctypes.data)
    assert got[0].tobytes() == want[0].tobytes(), "staged records"
    assert got[1].tobytes() == want[1].tobytes(), "staged ids"
    assert got[2].tobytes() == want[2].tobytes(), "offsets"
    assert got[3] == want[3], "status"
    return got


# --------------------------------------------------------------------------- 1. the twin against the restatement
@pytest.mark.parametrize("label", sorted(tr.lists(len(FILES))))
def test_twin_equals_the_restatement(label):
    T = _tables()
    ids = tr.lists(T.n)[label]
    got = _stage(T, ids)
    assert got[3] == 0 and (got[1] == np.arange(len(ids))).all()
    assert int(got[2][-1]) == sum(_lib().x3djpeg_stage_bytes(int(T.scan_bytes[i]), int(T.nseg[i])) for i in ids)
    _check_staging(T, ids, got)
    if label == "in_order":                                 # the round-up tails are there to be zeroed
        assert ((T.scan_bytes + SCAN_PAD) % 16 != 0).any() and T.nseg.max() > 1


def test_stage_bytes_is_the_arena_size_of_a_frame():
    h = _lib()
    for sb, ns in ((0, 1), (1, 1), (15, 3), (16, 1), (17, 2), (13852, 1), ((1 << 27) - 1, 4)):
        assert h.x3djpeg_stage_bytes(sb, ns) == int(tr.frame_bytes(sb, ns)) == ((sb + SCAN_PAD + 15) // 16) * 16 + 16 * ns
    assert h.x3djpeg_stage_bytes(-1, 1) == 0 and h.x3djpeg_stage_bytes(5, -1) == 0


# --------------------------------------------------------------------------- 2. refusals
def _five():
    return [NAMES.index(k) for k in sr.REFUSED_NAMES]


@pytest.mark.parametrize("label", ["id_minus_1", "id_nrecs", "cap_short", "frame_beyond_max"])
def test_a_request_that_cannot_be_staged_takes_no_bytes(label):
    T = _tables()
    ids, short, max_frame, bit, refused = list(_five()), None, None, _jpeglib.STAGE_BAD_ID, 1
    if label == "id_minus_1":
        ids[1] = -1
    elif label == "id_nrecs":
        ids[3], refused = T.n, 3
    elif label == "cap_short":
        short, bit, refused = 4, _jpeglib.STAGE_NO_ROOM, 4    # one byte short of the total: exactly the last one
    else:
        size = tr.frame_bytes(T.recs["scan_bytes"], T.recs["nseg"])[ids]
        refused, bit = int(np.argmax(size)), _jpeglib.STAGE_NO_ROOM
        max_frame = int(size.max()) - 16
        assert (size[np.arange(5) != refused] <= max_frame).all()
    got = _stage(T, ids, short, max_frame)
    clean_ids = list(_five())
    clean = _stage(T, clean_ids)
    srecs, sids, offsets, status, staging = got
    assert status == bit and [k for k in range(5) if sids[k] < 0] == [refused]
    assert not srecs[refused:refused + 1].view(np.uint8).any()
    _check_staging(T, ids, got)
    size = np.diff(clean[2])
    assert int(offsets[-1]) == int(clean[2][-1]) - int(size[refused])          # nothing of its bytes
    for k in range(5):
        if k < refused:                                     # every other request is as before; later ones move up
            assert offsets[k] == clean[2][k] and srecs[k].tobytes()[16:] == clean[0][k].tobytes()[16:]
        elif k > refused:
            assert offsets[k] == clean[2][k] - size[refused]
    # the builder answers the refused request with BAD_ID and a zero pair, and serves the others
    jobs = _build(T, got, ids)
    assert jobs[3] == _jpeglib.STORE_BAD_ID and not jobs[0][refused:refused + 1].view(np.uint8).any()
    assert not jobs[1][refused:refused + 1].view(np.uint8).any()
    assert all(jobs[0][k]["scan"] == srecs[k]["scan"] for k in range(5) if k != refused)


def _build(T, got, ids, coef_base=0x5000000000, planes_base=0x6000000000, sub_bits=SUB_BITS):
    """x3djpeg_store_build_jobs_host on the staged tables."""
    S = type("S", (), dict(recs=got[0], n=len(ids), headers=T.headers))
    safe = [i if 0 <= i < T.n else 0 for i in ids]
    dst = sr.dst_table(T, safe)
    counts = T.infos["coef_count"][safe].astype(np.int64)
    ws = sr.workspace_bytes(T.scan_bytes[safe], T.nseg[safe], sub_bits)
    return sr.twin(S, got[1], dst, sub_bits, coef_base, planes_base, int(counts.sum()), int(counts.sum()), int(ws.sum()))


# --------------------------------------------------------------------------- 3. end to end on the CPU
def _decode_staged(T, ids, got, sub_bits=SUB_BITS, recs_of=None):
    n = len(ids)
    counts = T.infos["coef_count"][ids].astype(np.int64)
    total = int(counts.sum())
    ws_total = int(sr.workspace_bytes(T.scan_bytes[ids], T.nseg[ids], sub_bits).sum())
    cwhole, coef = sr.aligned(2 * total, 0x5A)
    wwhole, ws = sr.aligned(ws_total)
    pwhole, planes = sr.aligned(total)
    sj, fj, plan, status = _build(T, got, ids, coef.ctypes.data, planes.ctypes.data, sub_bits)
    assert status == 0
    st = np.full(n, 77, np.int32)
    sjc = np.ascontiguousarray(sj)
    _jpeglib.check(_lib().x3djpeg_entropy_decode_parallel_host(sjc.ctypes.data, n, sub_bits, ws.ctypes.data, ws_total,
                                                               st.ctypes.data, None))
    assert not st.any() and sr.guards_intact(cwhole, coef) and sr.guards_intact(wwhole, ws)
    got16 = coef.view(np.int16)
    for k, i in enumerate(ids):
        want = np.zeros(int(counts[k]), np.int16)
        rc, _ = _jpeglib.entropy_decode(FILES[i], T.infos[i:i + 1], want.ctypes.data, want.nbytes)
        assert rc == 0 and np.array_equal(got16[plan[k]:plan[k] + counts[k]], want), NAMES[i]


def test_the_staged_tables_decode_to_the_host_decoders_coefficients():
    T = _tables()
    ids = sr.served_lists(T.n)["scrambled"]
    _decode_staged(T, ids, _stage(T, ids))


# --------------------------------------------------------------------------- 4. the sanitised stand-alone program
def test_the_same_lists_in_a_sanitised_stand_alone_program(tmp_path):
    """host.cpp, scan.cpp, store_host.cpp, stage_host.cpp and the core headers compiled with -fsanitize=address,undefined into
    a program of their own, run as a child process; nothing sanitised is loaded into this interpreter."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    L = tr.lists(len(FILES))
    runs = [(ids, None, 0) for ids in L.values()]
    five = _five()
    runs += [(five[:1] + [-1] + five[2:], None, _jpeglib.STAGE_BAD_ID), (five[:3] + [len(FILES)] + five[4:], None, _jpeglib.STAGE_BAD_ID),
             (five, 4, _jpeglib.STAGE_NO_ROOM), (five, 2, _jpeglib.STAGE_NO_ROOM)]
    exe = str(tmp_path / "jpeg_tier_check")
    src = os.path.join(ROOT, "x3d-multigrid_amd", "csrc_jpeg")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "jpeg_tier_check.cpp")]
    cmd += [os.path.join(src, k) for k in ("host.cpp", "scan.cpp", "store_host.cpp", "stage_host.cpp")] + ["-o", exe]
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True)
    path = str(tmp_path / "runs.bin")
    tr.write_check_input(path, FILES, runs)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "frames" and int(last[1]) == len(FILES) and int(last[3]) == len(runs) and int(last[-1]) == 0
    assert int(last[5]) == sum(len(ids) for ids in L.values()) + 4 + 4 + 4 + 2 and int(last[7]) == 1 + 1 + 1 + 3


# --------------------------------------------------------------------------- 5. ABI
def test_stage_symbols_constants_and_argument_checks():
    h = _lib()
    assert _jpeglib.ABI_VERSION == 2 and h.x3djpeg_abi_version() == 2
    src = open(os.path.join(ROOT, "include", "x3djpeg.h")).read()
    for name, value in (("BAD_ID", _jpeglib.STAGE_BAD_ID), ("NO_ROOM", _jpeglib.STAGE_NO_ROOM)):
        assert re.search(r"#define X3DJPEG_STAGE_%s %d\b" % (name, value), src), name
    dev, host = _jpeglib.SIGNATURES["x3djpeg_stage"], _jpeglib.SIGNATURES["x3djpeg_stage_host"]
    assert dev[1][:-1] == host[1] and len(dev[1]) == 12
    T = _tables()
    ids = np.zeros(1, np.int32)
    out = [sr.aligned(k)[1] for k in (1 << 16, 32, 4, 16, 4)]
    args = [T.recs.ctypes.data, T.n, ids.ctypes.data, 1, 1 << 16, out[0].ctypes.data, 1 << 16, out[1].ctypes.data,
            out[2].ctypes.data, out[3].ctypes.data, out[4].ctypes.data]
    assert h.x3djpeg_stage_host(*args) == 0
    for at, bad in ((0, None), (2, None), (5, None), (7, None), (8, None), (9, None), (10, None), (1, 0), (3, 0), (3, 65536),
                    (4, 0), (4, 1 << 41), (5, out[0].ctypes.data + 8)):
        a = list(args)
        a[at] = bad
        assert h.x3djpeg_stage_host(*a) == _jpeglib.EINVAL, (at, bad)
        assert h.x3djpeg_stage(*a, None) == _jpeglib.EINVAL, (at, bad)
    assert b"argument check failed" in h.x3djpeg_last_error()


# --------------------------------------------------------------------------- 6. the host stages on their own
def test_host_stages_prepare_in_plain_host_memory_without_a_gpu(monkeypatch):
    """jpegops.HostStages is what FrameStore.add prepares frames with, and tools/pack_frames.py runs it on machines
    without a GPU: it is no JpegDecoder, touches neither torch.cuda nor pinned memory, and its staging buffer holds, per
    frame, the scan and the segment table x3djpeg_scan_prepare gives for that frame alone (sr.Tables)."""
    import torch
    from x3dhip import jpegops
    T = _tables()

    def refuse(*a, **kw):
        raise AssertionError("the host stages reached for the GPU")
    for name in ("init", "_lazy_init", "is_available", "device_count", "current_device", "set_device", "device",
                 "synchronize", "current_stream", "Event", "Stream"):
        monkeypatch.setattr(torch.cuda, name, refuse)
    monkeypatch.setattr(torch.Tensor, "pin_memory", refuse)
    stages = jpegops.HostStages(3, SUB_BITS)
    assert issubclass(jpegops.JpegDecoder, jpegops.HostStages) and not isinstance(stages, jpegops.JpegDecoder)
    assert stages.threads == 3 and stages.sub_bits == SUB_BITS and jpegops.HostStages(99, None).threads == 16
    infos, staged, scan_at, seg_at, scan_bytes, nseg, ws = stages._prepare_stage(FILES)
    monkeypatch.undo()
    assert staged.device.type == "cpu" and staged.dtype == torch.uint8 and not staged.is_pinned()
    assert not stages._staging(1).is_pinned() and stages._staging(1).data_ptr() == staged.data_ptr()     # reused
    assert infos.tobytes() == T.infos.tobytes()
    assert np.array_equal(scan_bytes, T.scan_bytes) and np.array_equal(nseg, T.nseg)
    assert np.array_equal(ws, sr.workspace_bytes(T.scan_bytes, T.nseg, SUB_BITS))
    got = staged.numpy()
    for i in range(len(FILES)):
        nb, sb = int(scan_bytes[i]) + SCAN_PAD, int(nseg[i]) * _jpeglib.SCAN_SEG_DT.itemsize
        assert got[scan_at[i]:scan_at[i] + nb].tobytes() == T.arena[T.scan_at[i]:T.scan_at[i] + nb].tobytes(), NAMES[i]
        assert got[seg_at[i]:seg_at[i] + sb].tobytes() == T.arena[T.seg_at[i]:T.seg_at[i] + sb].tobytes(), NAMES[i]
    with pytest.raises(ValueError, match="sub_bits must be a multiple of 32"):
        jpegops.HostStages(2, 48)


# --------------------------------------------------------------------------- 7. pack files on host memory
def _store(files=FILES, **kw):
    from x3dhip import jpegstore
    _lib()
    mem = HostMemory()
    store = jpegstore.FrameStore("cpu", memory=mem, **kw)
    if files:
        store.add(files)
    return store, mem


def _mem_reader(mem):
    spans = [(v.ctypes.data, v) for _, v in mem.blocks]

    def read(addr, nbytes):
        for base, v in spans:
            if base <= addr and addr + nbytes <= base + v.size:
                return v[addr - base:addr - base + nbytes]
        raise AssertionError("address outside the store's memory")
    return read


def _store_tables(store):
    """A store's tables as the stage twin wants them: 16-byte aligned copies."""
    n = len(store)
    _, rv = sr.aligned(n * _jpeglib.STORE_REC_DT.itemsize)
    rv[:] = store._recs.host[:n].view(np.uint8).reshape(-1)
    _, hv = sr.aligned(store.n_headers * _jpeglib.STORE_HEADER_DT.itemsize)
    hv[:] = store._headers.host[:store.n_headers].view(np.uint8).reshape(-1)
    return rv.view(_jpeglib.STORE_REC_DT), hv.view(_jpeglib.STORE_HEADER_DT)


def _same_frames(store, mem, files, sub_bits):
    """Stage and decode every frame of `store` on the CPU: the coefficients are the files'."""
    recs, heads = _store_tables(store)
    n = len(store)
    infos = np.concatenate([_jpeglib.parse(f)[1] for f in files])
    T = type("S", (), dict(n=n, recs=recs, headers=heads, infos=infos, scan_bytes=store.scan_bytes.astype(np.int64),
                           nseg=store.nseg.astype(np.int64)))
    ids = list(range(n))
    size = tr.frame_bytes(T.scan_bytes, T.nseg)
    got = tr.twin(recs, ids, int(size.sum()), int(size.max()))
    want = tr.restate(recs, ids, None, None, staging_base=got[4].ctypes.data)
    assert got[0].tobytes() == want[0].tobytes() and got[2].tobytes() == want[2].tobytes() and got[3] == 0
    _check_staging(T, ids, got, _mem_reader(mem), recs)
    S = type("S", (), dict(recs=got[0], n=n, headers=heads))
    counts = infos["coef_count"].astype(np.int64)
    ws = store.ws_need.astype(np.int64)
    assert np.array_equal(ws, sr.workspace_bytes(T.scan_bytes, T.nseg, sub_bits))
    _, coef = sr.aligned(2 * int(counts.sum()))
    _, planes = sr.aligned(int(counts.sum()))
    _, wsb = sr.aligned(int(ws.sum()))
    sj, fj, plan, status = sr.twin(S, got[1], sr.dst_table(T, ids), sub_bits, coef.ctypes.data, planes.ctypes.data,
                                   int(counts.sum()), int(counts.sum()), int(ws.sum()))
    assert status == 0
    st = np.full(n, 77, np.int32)
    sjc = np.ascontiguousarray(sj)
    _jpeglib.check(_lib().x3djpeg_entropy_decode_parallel_host(sjc.ctypes.data, n, sub_bits, wsb.ctypes.data, int(ws.sum()),
                                                               st.ctypes.data, None))
    assert not st.any()
    for k in range(n):
        want16 = np.zeros(int(counts[k]), np.int16)
        rc, _ = _jpeglib.entropy_decode(files[k], infos[k:k + 1], want16.ctypes.data, want16.nbytes)
        assert rc == 0 and np.array_equal(coef.view(np.int16)[plan[k]:plan[k] + counts[k]], want16), k


def _load(path, **kw):
    from x3dhip import jpegstore
    mem = HostMemory()
    store, meta, id_map = jpegstore.FrameStore.load(path, "cpu", memory=mem, **kw)
    return store, mem, meta, id_map


def test_pack_round_trip_gives_the_same_frames(tmp_path):
    store, mem = _store(chunk_bytes=8192, sub_bits=32)
    assert store.n_chunks >= 3
    path = str(tmp_path / "all.pack")
    meta = {"videos": [{"name": "a", "label": 3, "first": 0, "frames": len(FILES)}], "note": "café"}
    store.save(path, meta)
    got, gmem, gmeta, id_map = _load(path, chunk_bytes=8192)
    assert gmeta == meta and id_map == [range(0, len(FILES))] and len(got) == len(FILES) and got.sub_bits == 32
    assert got.n_headers == store.n_headers and got.n_chunks == store.n_chunks
    for f in ("width", "height", "nblocks", "scan_bytes", "nseg", "coef_count", "ws_need"):
        assert np.array_equal(getattr(got, f), getattr(store, f)), f
    assert np.array_equal(got._recs.host["header"][:len(got)], store._recs.host["header"][:len(store)])
    _same_frames(got, gmem, FILES, 32)
    # sub_bits 32 at save, 1024 at load: the workspace needs are those of 1024; another chunk size places them anew
    got, gmem, _, _ = _load(path, sub_bits=1024, chunk_bytes=1 << 20)
    assert got.sub_bits == 1024 and got.n_chunks == 1
    _same_frames(got, gmem, FILES, 1024)
    # a loaded store takes more frames, and finds the headers it knows
    heads = got.n_headers
    assert got.add(FILES[:3]) == range(len(FILES), len(FILES) + 3) and got.n_headers == heads
    _same_frames(got, gmem, FILES + FILES[:3], 1024)
    # an empty store is a pack too
    empty, _ = _store(files=())
    empty.save(str(tmp_path / "empty.pack"))
    got, _, gmeta, id_map = _load(str(tmp_path / "empty.pack"))
    assert len(got) == 0 and gmeta is None and id_map == [range(0, 0)]


def test_ranges_skip_reorder_and_repeat(tmp_path):
    store, mem = _store(chunk_bytes=8192)
    path = str(tmp_path / "all.pack")
    store.save(path)
    n = len(FILES)
    ranges = [range(n - 4, n), range(5, 9), range(0, 2), range(5, 9), range(3, 3)]
    got, gmem, _, id_map = _load(path, ranges=ranges, chunk_bytes=8192)
    assert id_map == [range(0, 4), range(4, 8), range(8, 10), range(10, 14), range(14, 14)] and len(got) == 14
    picked = [FILES[i] for r in ranges for i in r]
    _same_frames(got, gmem, picked, got.sub_bits)
    for bad in ([range(0, n + 1)], [range(-1, 2)], [range(0, 4, 2)]):
        with pytest.raises(ValueError):
            _load(path, ranges=bad)


def test_load_refuses_a_damaged_pack(tmp_path):
    from x3dhip import jpegstore
    store, mem = _store(chunk_bytes=8192)
    assert store.n_chunks >= 3
    path = str(tmp_path / "good.pack")
    store.save(path, {"k": 1})
    good = open(path, "rb").read()
    _load(path)
    head = jpegstore.PACK_HEAD
    fields = list(head.unpack(good[:head.size]))
    frames_at = head.size + fields[6] * jpegstore.STORE_HEADER_DT.itemsize
    ft = np.frombuffer(good[frames_at:frames_at + fields[5] * jpegstore.PACK_FRAME_DT.itemsize], jpegstore.PACK_FRAME_DT)

    def with_head(at, value):
        f = list(fields)
        f[at] = value
        return head.pack(*f) + good[head.size:]

    def with_frame(i, name, value):
        t = ft.copy()
        t[name][i] = value
        return good[:frames_at] + t.tobytes() + good[frames_at + t.nbytes:]

    bad = {"magic": with_head(0, b"X3DJPACX"), "version": with_head(1, 2), "header entry": with_head(2, fields[2] + 16),
           "frame entry": with_head(3, 40), "frames": with_head(5, fields[5] + 1), "frames less": with_head(5, fields[5] - 1),
           "headers": with_head(6, fields[6] + 1), "arena offset": with_head(7, fields[7] + 16),
           "arena bytes": with_head(8, fields[8] + 16), "meta bytes": with_head(9, fields[9] - 1),
           "offset past the end": with_frame(7, "offset", len(good)), "offset before the arena": with_frame(0, "offset", 16),
           "offset unaligned": with_frame(3, "offset", int(ft["offset"][3]) + 1),
           "last frame one piece on": with_frame(len(ft) - 1, "offset", int(ft["offset"][-1]) + 16),
           "length": with_frame(2, "length", int(ft["length"][2]) + 16), "header index": with_frame(4, "header", fields[6]),
           "header index below": with_frame(4, "header", -1), "width": with_frame(1, "width", int(ft["width"][1]) + 1),
           "scan bytes": with_frame(1, "scan_bytes", -5), "meta": good[:-1] + b"\xff", "empty": b"", "short head": good[:40]}
    for step in range(0, len(good), 4096):                  # truncation at every 4 KB boundary
        bad["cut at %d" % step] = good[:step]
    bad["one byte short"] = good[:-1]
    bad["one byte long"] = good + b" "
    p = str(tmp_path / "bad.pack")
    for label, data in bad.items():
        with open(p, "wb") as f:
            f.write(data)
        for kw in (dict(), dict(ranges=[range(0, 1)])):
            with pytest.raises(ValueError):
                _load(p, **kw)
            assert label
    # a damaged scan is not the loader's business: it loads, and fails alone at decode time (the decoder's own checks)
    at = int(ft["offset"][5]) + 40
    with open(p, "wb") as f:
        f.write(good[:at] + bytes(b ^ 0xFF for b in good[at:at + 64]) + good[at + 64:])
    got, _, _, _ = _load(p)
    assert len(got) == len(FILES)


# --------------------------------------------------------------------------- 7. the packing tool, without a GPU
def test_pack_frames_packs_a_folder_tree_whole_and_as_validation_windows(tmp_path, monkeypatch, capsys):
    import frames
    from tools import pack_frames
    from x3dhip import jpegstore
    _lib()
    monkeypatch.setattr(frames, "MIN_FRAMES", tr.MIN_FRAMES)
    root, anno, labels = tr.write_tree(tmp_path, "validate")
    whole, windows = str(tmp_path / "whole.pack"), str(tmp_path / "windows.pack")
    pack_frames.main(["--root", root, "--anno", anno, "--labels", labels, "--subset", "validate", "--out", whole, "--threads", "2"])
    pack_frames.main(["--root", root, "--anno", anno, "--labels", labels, "--subset", "validate", "--out", windows,
                      "--val-windows", "3", "--sample-duration", "10", "--gamma-tau", "2", "--threads", "2"])
    out = capsys.readouterr().out.splitlines()
    assert out[0].startswith(whole + ": 4 videos, %d frames" % sum(t[2] for t in tr.TREE)) and out[1].startswith(windows + ": 4 videos")
    entries = frames.list_annotation(root, anno, labels, "validate")
    assert [e[1] for e in entries] == [1, 3, 1, 4]
    for path, win in ((whole, None), (windows, dict(gamma_tau=2, sample_duration=10, crops=3))):
        store, mem, meta, id_map = _load(path)
        assert meta["subset"] == "validate" and meta["windows"] == win and len(meta["videos"]) == 4
        assert jpegstore.FrameStore.read_meta(path) == meta
        files, at = [], 0
        for v, (folder, label), t in zip(meta["videos"], entries, tr.TREE):
            index = list(range(t[2])) if win is None else frames.val_window_frames(t[2], **win)
            assert (v["name"], v["label"], v["first"], v["frames"], v["n_frames"]) == (
                t[0].replace(" ", "_") + "/" + t[1], label, at, len(index), t[2])
            assert v["index"] == (None if win is None else index)
            assert (store.width[at], store.height[at]) == (t[3], t[4])
            files += folder.read(index)
            at += len(index)
        assert len(store) == at and (win is None or at < sum(t[2] for t in tr.TREE))
        if win is not None:
            assert all(len(v["index"]) <= 15 for v in meta["videos"])        # 3 windows of 5 frames
        _same_frames(store, mem, files, store.sub_bits)
