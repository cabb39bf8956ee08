"""The frame store of libx3djpeg.so, checks that need no GPU: x3djpeg_store_build_jobs_host (the kernels' code, run serially)
against the numpy restatement of tests/jpegstore_ref.py byte for byte, padding included and inside guard bytes; the
refusals; the built scan jobs decoded on the CPU; the same request lists once more in a stand-alone program built with the
address and undefined-behaviour sanitisers; the C ABI; and the host logic of x3dhip.jpegstore.FrameStore (header
deduplication, chunking, an add() that fails) on a store kept in host memory."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import jpeg_entropy_cases as jc
from tests import jpeg_ref as jr
from tests import jpegstore_ref as sr
from x3dhip import _jpeglib
from x3dhip._lib import X3DHipError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES, FILES = sr.good_files()
COEF_BASE, PLANES_BASE = 0x5000000000, 0x6000000000       # addresses only: the builder never follows them
_T = {}


def _lib():
    if not os.path.exists(_jpeglib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _jpeglib.lib()


def _tables():
    """The hand-built tables over every good case, once."""
    if "t" not in _T:
        _lib()
        _T["t"] = sr.Tables(FILES)
    return _T["t"]


def _same(got, want, label):
    for g, w, what in zip(got[:3], want[:3], ("scan jobs", "frame jobs", "plan")):
        assert g.tobytes() == w.tobytes(), (label, what)
    assert got[3] == want[3], (label, "build status")


# --------------------------------------------------------------------------- 1. the twin against the restatement
@pytest.mark.parametrize("sub_bits", jc.SUB_BITS)
@pytest.mark.parametrize("order", ["in_order", "scrambled", "repeats", "one"])
def test_twin_equals_the_restatement(order, sub_bits):
    T = _tables()
    ids = sr.served_lists(T.n)[order]
    dst = sr.dst_table(T, ids)
    want = sr.restate(T, ids, dst, sub_bits, COEF_BASE, PLANES_BASE)
    total, ws_total = int(want[2][-2]), int(want[2][-1])
    got = sr.twin(T, ids, dst, sub_bits, COEF_BASE, PLANES_BASE, total, total, ws_total)
    _same(got, want, order)
    assert got[3] == 0 and not got[2][2 * len(ids):3 * len(ids)].any()
    # the sizes the restatement works with are the library's
    assert ws_total == sum(_jpeglib.workspace_bytes(T.scan_bytes[i], T.nseg[i], sub_bits) for i in ids)
    assert {int(i) for i in T.infos["ncomp"]} == {1, 3} and T.nseg.max() > 1 and len({tuple(i) for i in T.infos["comp_h"]}) >= 2


# --------------------------------------------------------------------------- 2. refusals
def _refused_run(label, sub_bits=128):
    T = _tables()
    ids, wider, coef_short, ws_short, bit, refused = sr.refused_lists(NAMES)[label]
    clean_ids = [i if 0 <= i < T.n else 0 for i in ids]
    clean = sr.restate(T, clean_ids, sr.dst_table(T, clean_ids), sub_bits, COEF_BASE, PLANES_BASE)
    plan = sr.restate(T, ids, sr.dst_table(T, ids), sub_bits, COEF_BASE, PLANES_BASE)[2]
    n = len(ids)
    counts = np.diff(np.concatenate([plan[:n], plan[3 * n:3 * n + 1]]))
    ws = np.diff(np.concatenate([plan[n:2 * n], plan[3 * n + 1:]]))
    coef_cap = int(plan[3 * n]) if coef_short is None else int(plan[coef_short] + counts[coef_short] - 1)
    ws_cap = int(plan[3 * n + 1]) if ws_short is None else int(plan[n + ws_short] + ws[ws_short] - 1)
    dst = sr.dst_table(T, ids, wider=wider)
    return T, ids, dst, (coef_cap, coef_cap, ws_cap), bit, refused, clean


@pytest.mark.parametrize("label", ["id_minus_1", "id_nrecs", "wider", "coef_short", "ws_short"])
def test_a_request_that_cannot_be_served_gets_the_refused_pair_and_the_status_bit(label):
    sub_bits = 128
    T, ids, dst, caps, bit, refused, clean = _refused_run(label, sub_bits)
    got = sr.twin(T, ids, dst, sub_bits, COEF_BASE, PLANES_BASE, *caps)
    _same(got, sr.restate(T, ids, dst, sub_bits, COEF_BASE, PLANES_BASE, *caps), label)
    sj, fj, plan, status = got
    n = len(ids)
    assert status == bit
    assert [i for i in range(n) if plan[2 * n + i]] == list(refused) and all(plan[2 * n + i] == bit for i in refused)
    for i in range(n):
        if i in refused:                                    # every byte zero: null scan / segs / coef, no blocks, no pixels
            assert not sj[i:i + 1].view(np.uint8).any() and not fj[i:i + 1].view(np.uint8).any(), (label, i)
        elif label.startswith("id_"):                       # a bad id takes no room: what follows moves up, nothing else
            pass
        else:                                               # byte-identical to the run in which nothing is refused
            assert sj[i].tobytes() == clean[0][i].tobytes() and fj[i].tobytes() == clean[1][i].tobytes(), (label, i)
    if not label.startswith("id_"):                         # refusing moves nobody else's range
        assert np.array_equal(plan[:2 * n], clean[2][:2 * n]) and np.array_equal(plan[3 * n:], clean[2][3 * n:])
    else:
        bad = refused[0]
        assert np.array_equal(plan[:bad + 1], clean[2][:bad + 1])
        for i in range(bad):
            assert sj[i].tobytes() == clean[0][i].tobytes() and fj[i].tobytes() == clean[1][i].tobytes(), (label, i)
        for i in range(bad + 1, n):                         # the same jobs, at the offsets the restatement gives
            same = [f for f in _jpeglib.SCAN_JOB_DT.names if f not in ("coef", "ws_off")]
            assert all(np.array_equal(sj[i][f], clean[0][i][f]) for f in same), (label, i)


# --------------------------------------------------------------------------- 3. end to end on the CPU
@pytest.mark.parametrize("sub_bits", jc.SUB_BITS)
def test_the_twins_scan_jobs_decode_to_the_host_decoders_coefficients(sub_bits):
    T = _tables()
    ids = sr.served_lists(T.n)["scrambled"]
    n = len(ids)
    counts = T.infos["coef_count"][ids].astype(np.int64)
    total = int(counts.sum())
    ws_total = int(sr.workspace_bytes(T.scan_bytes[ids], T.nseg[ids], sub_bits).sum())
    cwhole, coef = sr.aligned(2 * total, 0x5A)
    wwhole, ws = sr.aligned(ws_total)
    pwhole, planes = sr.aligned(total)
    sj, fj, plan, status = sr.twin(T, ids, sr.dst_table(T, ids), sub_bits, coef.ctypes.data, planes.ctypes.data, total, total,
                                   ws_total)
    assert status == 0
    st = np.full(n, 77, np.int32)
    sjc = np.ascontiguousarray(sj)
    _jpeglib.check(_lib().x3djpeg_entropy_decode_parallel_host(sjc.ctypes.data, n, sub_bits, ws.ctypes.data, ws_total,
                                                               st.ctypes.data, None))
    assert not st.any()
    assert sr.guards_intact(cwhole, coef) and sr.guards_intact(wwhole, ws)
    got = coef.view(np.int16)
    for k, i in enumerate(ids):
        want = np.zeros(int(counts[k]), np.int16)
        rc, _ = _jpeglib.entropy_decode(FILES[i], T.infos[i:i + 1], want.ctypes.data, want.nbytes)
        assert rc == 0 and np.array_equal(got[plan[k]:plan[k] + counts[k]], want), (NAMES[i], sub_bits)


# --------------------------------------------------------------------------- 4. the sanitised stand-alone program
def test_the_same_lists_in_a_sanitised_stand_alone_program(tmp_path):
    """host.cpp, scan.cpp, store_host.cpp and the two core headers compiled with -fsanitize=address,undefined into a program
    of their own, run as a child process on the lists of the tests above; nothing sanitised is loaded into this
    interpreter."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    lists = [(ids, (), None, None, 0) for ids in sr.served_lists(len(FILES)).values()]
    lists += [v[:5] for v in sr.refused_lists(NAMES).values()]
    exe = str(tmp_path / "jpeg_store_check")
    src = os.path.join(ROOT, "x3d-multigrid_amd", "csrc_jpeg")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "jpeg_store_check.cpp"),
           os.path.join(src, "host.cpp"), os.path.join(src, "scan.cpp"), os.path.join(src, "store_host.cpp"), "-o", exe]
    # the sanitisers' runtimes linked into the program itself where the compiler ships them so (gcc needs to be told)
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True)
    served = refused = 0
    for sub_bits in jc.SUB_BITS:
        path = str(tmp_path / ("lists_%d.bin" % sub_bits))
        sr.write_check_input(path, FILES, lists, sub_bits)
        r = subprocess.run([exe, path], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        last = r.stdout.strip().splitlines()[-1].split()
        assert last[0] == "frames" and int(last[1]) == len(FILES) and int(last[3]) == len(lists) and int(last[-1]) == 0
        served, refused = served + int(last[5]), refused + int(last[7])
    assert served == 3 * (4 * len(FILES) + 1 + 4 + 4 + 4 + 2 + 2) and refused == 3 * (1 + 1 + 1 + 3 + 3)


# --------------------------------------------------------------------------- 5. ABI
def test_store_symbols_structs_and_argument_checks():
    h = _lib()
    assert _jpeglib.ABI_VERSION == 2 and h.x3djpeg_abi_version() == 2
    assert h.x3djpeg_store_header_bytes() == _jpeglib.STORE_HEADER_DT.itemsize == 512 + _jpeglib.SCAN_JOB_DT.itemsize
    assert _jpeglib.STORE_HEADER_DT.itemsize % 16 == 0
    assert h.x3djpeg_store_rec_bytes() == _jpeglib.STORE_REC_DT.itemsize == 32
    assert h.x3djpeg_store_dst_bytes() == _jpeglib.STORE_DST_DT.itemsize == 24
    assert h.x3djpeg_store_plan_bytes(5) == 8 * 17 and h.x3djpeg_store_plan_bytes(0) == 0
    src = open(os.path.join(ROOT, "include", "x3djpeg.h")).read()
    for name, value in (("BAD_ID", _jpeglib.STORE_BAD_ID), ("BAD_SIZE", _jpeglib.STORE_BAD_SIZE),
                        ("NO_COEF", _jpeglib.STORE_NO_COEF), ("NO_WS", _jpeglib.STORE_NO_WS), ("PLAN_THREADS", _jpeglib.STORE_PLAN_THREADS),
                        ("PLAN_CHUNK", _jpeglib.STORE_PLAN_CHUNK)):
        assert re.search(r"#define X3DJPEG_STORE_%s %d\b" % (name, value), src), name
    assert re.search(r"#define X3DJPEG_ABI_VERSION 2\b", src)
    body = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(x3djpeg_store_[a-z0-9_]+)\s*\(", body))
    assert declared == {k for k in _jpeglib.SIGNATURES if k.startswith("x3djpeg_store_")} and len(declared) == 6
    # the argument lists of the two builders differ by the stream alone
    dev, host = _jpeglib.SIGNATURES["x3djpeg_store_build_jobs"], _jpeglib.SIGNATURES["x3djpeg_store_build_jobs_host"]
    assert dev[1][:-1] == host[1] and len(dev[1]) == 18
    nulls = (None, 1, None, 1, None, 1, 1024, None, 0, None, 0, 0, None, None, None, None, None)
    assert h.x3djpeg_store_build_jobs_host(*nulls) == _jpeglib.EINVAL and b"x3djpeg_store_build_jobs_host" in h.x3djpeg_last_error()
    assert h.x3djpeg_store_build_jobs(*nulls, None) == _jpeglib.EINVAL and b"argument check failed" in h.x3djpeg_last_error()
    # one null, a bad count, a bad sub_bits: each refused before anything is read
    T = _tables()
    ids = np.zeros(1, np.int32)
    dst = sr.dst_table(T, [0])
    out = [np.zeros(n, np.uint8) for n in (_jpeglib.SCAN_JOB_DT.itemsize, 512, 40, 4)]
    args = [T.recs.ctypes.data, T.n, T.headers.ctypes.data, T.n, ids.ctypes.data, 1, 1024, COEF_BASE, 1 << 20, PLANES_BASE,
            1 << 20, 1 << 20, dst.ctypes.data, out[2].ctypes.data, out[0].ctypes.data, out[1].ctypes.data, out[3].ctypes.data]
    assert h.x3djpeg_store_build_jobs_host(*args) == 0
    for at, bad in ((0, None), (2, None), (4, None), (12, None), (13, None), (14, None), (15, None), (16, None), (5, 0),
                    (5, 65536), (6, 48), (1, 0), (3, 0)):
        a = list(args)
        a[at] = bad
        assert h.x3djpeg_store_build_jobs_host(*a) == _jpeglib.EINVAL, (at, bad)
        assert h.x3djpeg_store_build_jobs(*a, None) == _jpeglib.EINVAL, (at, bad)


# --------------------------------------------------------------------------- 6. the host logic of FrameStore
class HostMemory:
    """x3dhip.jpegstore.TorchMemory's three methods over numpy arrays."""

    def __init__(self):
        self.blocks = []

    def alloc(self, nbytes):
        whole, view = sr.aligned(int(nbytes))
        self.blocks.append((whole, view))
        return view

    def write(self, buf, off, host):
        buf[off:off + host.size] = host

    def ptr(self, buf):
        return buf.ctypes.data


def _store(**kw):
    from x3dhip import jpegstore
    _lib()
    mem = HostMemory()
    return jpegstore.FrameStore("cpu", memory=mem, **kw), mem


def _check_against_the_files(store, mem, files, ids):
    """Every frame of the store lies whole inside one block of its memory, and its bytes there are what
    x3djpeg_scan_prepare gives for its file."""
    scan_at, seg_at = store.addresses()
    spans = [(v.ctypes.data, v.ctypes.data + v.size, v) for _, v in mem.blocks]
    for i, data in zip(ids, files):
        rc, info, _ = _jpeglib.parse(data)
        rc, scan, segs, _ = _jpeglib.scan_prepare(data, info)
        lo, hi = int(scan_at[i]), int(seg_at[i]) + segs.nbytes
        home = [s for s in spans if s[0] <= lo and hi <= s[1]]
        assert len(home) == 1 and lo % 16 == 0 and int(seg_at[i]) % 16 == 0, i
        base, _, v = home[0]
        assert v[lo - base:lo - base + scan.size].tobytes() == scan.tobytes(), i
        assert v[int(seg_at[i]) - base:hi - base].tobytes() == segs.tobytes(), i
        assert int(seg_at[i]) >= lo + scan.size
        assert (store.scan_bytes[i], store.nseg[i]) == (scan.size - _jpeglib.SCAN_PAD, segs.size)
        assert (store.width[i], store.height[i], store.coef_count[i], store.nblocks[i]) == (
            info["width"][0], info["height"][0], info["coef_count"][0], info["nblocks"][0])


def test_frame_store_deduplicates_headers_by_their_bytes():
    g = dict(zip(NAMES, FILES))
    store, mem = _store()
    assert len(store) == 0 and store.n_headers == 0
    assert store.add([g["vid_00"], g["vid_00"]]) == range(0, 2) and store.n_headers == 1
    assert store.add([g["vid_03"]]) == range(2, 3) and store.n_headers == 1          # a video's frames share their header
    q1, q75 = _jpeglib.parse(g["c420_40x56_q1"])[1], _jpeglib.parse(g["c420_40x56_optimize"])[1]
    assert not np.array_equal(q1["qt"], q75["qt"]) and (q1["width"], q1["height"]) == (q75["width"], q75["height"])
    store.add([g["c420_40x56_q1"], g["c420_40x56_optimize"], g["c420_40x56_q1"]])      # same size, another quality
    assert store.n_headers == 3 and len(store) == 6
    store.add([g["vid_07"], g["c420_40x56_q1"]])                                         # known ones, from an earlier add
    assert store.n_headers == 3 and len(store) == 8
    heads = store._recs.host["header"][:8].tolist()
    assert heads == [0, 0, 0, 1, 2, 1, 0, 1]
    _check_against_the_files(store, mem, [g[k] for k in ("vid_00", "vid_00", "vid_03", "c420_40x56_q1", "c420_40x56_optimize",
                                                         "c420_40x56_q1", "vid_07", "c420_40x56_q1")], range(8))
    assert store.add([]) == range(8, 8)


def test_frame_store_never_splits_a_frame_and_never_moves_one():
    chunk = 8192
    store, mem = _store(chunk_bytes=chunk, sub_bits=128)
    seen, before = [], None
    for lo in range(0, len(FILES), 5):
        part = FILES[lo:lo + 5]
        ids = store.add(part)
        assert ids == range(lo, lo + len(part))
        seen += part
        scan_at, seg_at = store.addresses()
        if before is not None:                              # growth of the arena and of the tables moves no frame
            assert np.array_equal(scan_at[:len(before[0])], before[0]) and np.array_equal(seg_at[:len(before[1])], before[1])
        before = (scan_at, seg_at)
    _check_against_the_files(store, mem, seen, range(len(seen)))
    assert store.n_chunks >= 4
    big = [i for i, f in enumerate(FILES) if len(f) > chunk]                 # larger than a chunk: a chunk of its own
    assert big and all(store._chunks[store._mirror["chunk"][i]][1] >= len(FILES[i]) - 1024 for i in big)
    assert store.bytes_resident() == sum(c[1] for c in store._chunks) + store._recs.nbytes + store._headers.nbytes
    assert store._headers.n > 8                                              # the header table has grown too
    # the tables the store wrote are the ones the builder reads: its twin on them gives the restatement's jobs
    n = len(store)
    T = type("S", (), dict(n=n, infos=np.concatenate([_jpeglib.parse(f)[1] for f in FILES]), scan_bytes=store.scan_bytes,
                           nseg=store.nseg, recs=store._recs.host[:n], headers=store._headers.host[:store.n_headers]))
    ids = sr.served_lists(n)["scrambled"]
    dst = sr.dst_table(T, ids)
    want = sr.restate(T, ids, dst, 128, COEF_BASE, PLANES_BASE)
    rwhole, rv = sr.aligned(T.recs.nbytes)
    hwhole, hv = sr.aligned(T.headers.nbytes)
    rv[:], hv[:] = T.recs.view(np.uint8).reshape(-1), T.headers.view(np.uint8).reshape(-1)
    T.recs, T.headers = rv.view(_jpeglib.STORE_REC_DT), hv.view(_jpeglib.STORE_HEADER_DT)
    got = sr.twin(T, ids, dst, 128, COEF_BASE, PLANES_BASE, int(want[2][-2]), int(want[2][-2]), int(want[2][-1]))
    _same(got, want, "store tables")
    assert np.array_equal(store.ws_need, sr.workspace_bytes(store.scan_bytes, store.nseg, 128))


def test_add_leaves_the_store_as_it_was_when_a_file_is_refused():
    rejects = {k: v[0] for k, v in jr.load_cases().items() if v[1] is None}
    store, mem = _store(chunk_bytes=4096)
    store.add(FILES[:7])

    def state():
        return (len(store), store.n_headers, store.n_chunks, store.bytes_resident(), [c[2] for c in store._chunks],
                store._recs.host[:len(store)].tobytes(), [v.tobytes() for _, v in mem.blocks])

    before = state()
    with pytest.raises(X3DHipError, match=r"frame 2 of the batch.*progressive"):
        store.add([FILES[8], FILES[9], rejects["reject_progressive"], FILES[10]])
    assert state() == before
    with pytest.raises(X3DHipError, match=r"frame 0 of the batch"):
        store.add([rejects["reject_truncated"][:200]])
    assert state() == before
    assert store.add(FILES[8:11]) == range(7, 10)
    _check_against_the_files(store, mem, FILES[:7] + FILES[8:11], range(10))
    for bad in (dict(sub_bits=48), dict(chunk_bytes=100), dict(chunk_bytes=0)):
        with pytest.raises(ValueError):
            _store(**bad)
    from x3dhip import jpegstore
    with pytest.raises(ValueError):
        jpegstore.FrameStore("cpu")                          # a store of its own memory lives on a GPU
