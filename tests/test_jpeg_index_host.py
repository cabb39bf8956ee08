"""The sync index of libx3djpeg.so, checks that need no GPU: x3djpeg_index_build against the plain restatement of
tests/jpegindex_ref.py byte for byte at three granularities; x3djpeg_entropy_decode_indexed_host (the indexed kernel's
code, run serially) against the host decoder x3djpeg_entropy_decode bit for bit; detection of every single-bit change of
the entries and of wrong records and ids, for the damaged frame alone; a stale index (the good file's, on a damaged scan)
never gives status 0 with other coefficients than the relaxation decoder's; the same lists once more in a stand-alone
program built with the address and undefined-behaviour sanitisers; the sidecar of a pack file; the C ABI."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import jpeg_entropy_cases as jc
from tests import jpegindex_ref as ir
from tests import jpegstore_ref as sr
from tests import jpegtier_ref as tr
from tests.test_jpeg_store_host import HostMemory
from x3dhip import _jpeglib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOOD = jc.good_cases()
INDEX_BITS = (32, 128, 1024)      # the smallest, one in between, the largest the measurements cover
GUARD = 32                        # int16 elements on either side of a coefficient buffer
NEW = ("x3djpeg_index_rec_bytes", "x3djpeg_index_count", "x3djpeg_index_build", "x3djpeg_entropy_decode_indexed",
       "x3djpeg_entropy_decode_indexed_host")
_C = {}


def _lib():
    if not os.path.exists(_jpeglib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _jpeglib.lib()


class Frame:
    """One file prepared for the device path, with the host decoder's coefficients; index(bits): its entries."""

    def __init__(self, data):
        _lib()
        self.data = data
        rc, self.info, msg = _jpeglib.parse(data)
        assert rc == 0, msg
        rc, self.scan, self.segs, msg = _jpeglib.scan_prepare(data, self.info)
        assert rc == 0, msg
        self.count = int(self.info["coef_count"][0])
        self.want = np.zeros(self.count, np.int16)
        self.host_rc, _ = _jpeglib.entropy_decode(data, self.info, self.want.ctypes.data, self.want.nbytes)
        self._index = {}

    def index(self, bits):
        if bits not in self._index:
            rc, e, msg = _jpeglib.index_build(self.scan, self.segs, self.info, bits)
            assert rc == 0, msg
            self._index[bits] = e
        return self._index[bits]


def _frame(name):
    if name not in _C:
        _C[name] = Frame(GOOD[name])
    return _C[name]


def _tables(frames, bits):
    """(INDEX_REC_DT [n], uint32 [total, 2]) of a list of Frames: the index tables of a store that holds them in order."""
    recs = np.zeros(len(frames), _jpeglib.INDEX_REC_DT)
    parts = [f.index(bits) for f in frames]
    recs["nentries"] = [len(p) for p in parts]
    recs["first_entry"] = np.cumsum(recs["nentries"]) - recs["nentries"]
    return recs, np.ascontiguousarray(np.concatenate(parts))


def _decode(jobs, ids, recs, entries, bits, nrecs=None):
    """x3djpeg_entropy_decode_indexed_host on jobs (Frames) with the frame ids `ids` into guarded buffers.  Returns
    (status [n], [coefficients]); the guards are checked."""
    n = len(jobs)
    sj = np.zeros(n, _jpeglib.SCAN_JOB_DT)
    bufs = []
    for k, f in enumerate(jobs):
        _jpeglib.fill_scan_jobs(sj[k:k + 1], f.info)
        buf = np.full(f.count + 2 * GUARD, 0x5A5A, np.int16)
        bufs.append(buf)
        sj["scan"][k], sj["segs"][k], sj["coef"][k] = f.scan.ctypes.data, f.segs.ctypes.data, buf.ctypes.data + 2 * GUARD
        sj["scan_bytes"][k], sj["nseg"][k] = f.scan.size - _jpeglib.SCAN_PAD, f.segs.size
    ids = np.ascontiguousarray(ids, np.int32)
    recs, entries = np.ascontiguousarray(recs), np.ascontiguousarray(entries, np.uint32)
    status = np.full(n, 77, np.int32)
    _jpeglib.check(_lib().x3djpeg_entropy_decode_indexed_host(
        sj.ctypes.data, n, ids.ctypes.data, recs.ctypes.data, len(recs) if nrecs is None else nrecs, entries.ctypes.data,
        len(entries), bits, status.ctypes.data))
    for f, buf in zip(jobs, bufs):
        assert np.all(buf[:GUARD] == 0x5A5A) and np.all(buf[GUARD + f.count:] == 0x5A5A), "guard overwritten"
    return status, [buf[GUARD:GUARD + f.count] for f, buf in zip(jobs, bufs)]


# --------------------------------------------------------------------------- 1. the rule
@pytest.mark.parametrize("bits", INDEX_BITS)
def test_the_indexer_equals_the_restatement(bits):
    empty = 0
    for name, data in GOOD.items():
        f = _frame(name)
        st, segs = ir.states(data, bits)
        want = ir.pack(st)
        got = f.index(bits)
        assert got.dtype == np.uint32 and got.tobytes() == want.tobytes(), (name, bits)
        assert _jpeglib.index_count(f.segs, bits) == ir.nsub(segs, bits) == len(want), (name, bits)
        # entries that repeat the one before: a subsequence in which no symbol starts, or one after the segment's last block
        empty += sum(a == b for a, b in zip(st[1:], st[:-1]))
    print(bits, "entries that repeat the one before:", empty)
    assert _jpeglib.index_count(_frame("vid_00").segs, 48) == 0 and _jpeglib.index_count(_frame("vid_00").segs, 0) == 0


def test_the_indexer_refuses_what_it_cannot_index():
    h, f = _lib(), _frame("c420_64x48_restart")
    cap = _jpeglib.index_count(f.segs, 128)
    out, n = np.zeros(cap, np.uint64), np.zeros(1, np.uint64)
    args = [f.scan.ctypes.data, f.scan.size - _jpeglib.SCAN_PAD, f.segs.ctypes.data, f.segs.size, f.info.ctypes.data, 128,
            out.ctypes.data, cap, n.ctypes.data]
    assert h.x3djpeg_index_build(*args) == 0 and int(n[0]) == cap
    for at, bad in ((0, None), (2, None), (4, None), (6, None), (8, None), (5, 48), (5, 0), (7, cap - 1), (3, f.segs.size - 1)):
        a = list(args)
        a[at] = bad
        assert h.x3djpeg_index_build(*a) == _jpeglib.EINVAL, (at, bad)
    # a segment of 2^22 blocks: the entry has 22 bits for the block.  1366 x 1366 MCUs of 4:2:0 without restarts.
    big = f.info.copy()
    big["mcus_x"], big["mcus_y"], big["restart_interval"] = 1366, 1366, 0
    big["blocks_w"][0], big["blocks_h"][0] = [2732, 1366, 1366], [2732, 1366, 1366]
    big["block_start"][0] = [0, 2732 * 2732, 2732 * 2732 + 1366 * 1366]
    big["coef_count"] = 64 * (2732 * 2732 + 2 * 1366 * 1366)
    seg = np.zeros(1, _jpeglib.SCAN_SEG_DT)
    seg["byte_len"], seg["mcu_count"] = 64, 1366 * 1366
    assert 6 * 1366 * 1366 >= _jpeglib.INDEX_MAX_BLOCKS
    rc = h.x3djpeg_index_build(f.scan.ctypes.data, 64, seg.ctypes.data, 1, big.ctypes.data, 128, out.ctypes.data, cap, n.ctypes.data)
    assert rc == _jpeglib.EUNSUPPORTED and b"segment 0" in h.x3djpeg_last_error() and b"sync index" in h.x3djpeg_last_error()
    # a scan the host decoder refuses is refused by the indexer, as corrupt
    refused = 0
    for label, data in jc.damaged(GOOD)[:200]:
        rc, info, _ = _jpeglib.parse(data)
        if rc:
            continue
        prc, scan, segs, _ = _jpeglib.scan_prepare(data, info)
        want = np.zeros(int(info["coef_count"][0]), np.int16)
        hrc, _ = _jpeglib.entropy_decode(data, info, want.ctypes.data, want.nbytes)
        if prc:
            assert hrc == _jpeglib.ECORRUPT, label
            continue
        irc, e, _ = _jpeglib.index_build(scan, segs, info, 128)
        assert irc == hrc and irc in (0, _jpeglib.ECORRUPT), (label, irc, hrc)
        refused += irc != 0
    assert refused > 0


# --------------------------------------------------------------------------- 2. the indexed decoder's twin
@pytest.mark.parametrize("bits", INDEX_BITS)
def test_the_indexed_twin_equals_the_host_decoder(bits):
    """Every good case in one batch -- restart per MCU (many segments of one subsequence), one component, own tables,
    quality-95 noise, the training-sized frame with more subsequences than the kernel has workers -- then a shuffled
    batch with repeats over the same tables."""
    names = list(GOOD)
    for must in ("c420_40x24_blocks1", "grey_200x150", "c422_161x99_optimize", "c444_48x40_q95_noise", "c420_340x256_q75"):
        assert must in names
    frames = [_frame(k) for k in names]
    assert all(f.host_rc == 0 for f in frames)
    recs, entries = _tables(frames, bits)
    assert bits != 1024 or recs["nentries"][names.index("c420_340x256_q75")] > 256
    status, got = _decode(frames, np.arange(len(frames)), recs, entries, bits)
    assert not status.any(), dict(zip(names, status))
    for f, g, name in zip(frames, got, names):
        assert np.array_equal(g, f.want), (name, bits)
    ids = np.random.default_rng(77).integers(0, len(frames), 48)
    assert len(set(ids.tolist())) < len(ids)
    status, got = _decode([frames[i] for i in ids], ids, recs, entries, bits)
    assert not status.any()
    for i, g in zip(ids, got):
        assert np.array_equal(g, frames[i].want), (names[i], bits)


# --------------------------------------------------------------------------- 3. detection
DETECT_BITS = 128


def _detect_batch():
    frames = [_frame(k) for k in jc.MUTATED]
    recs, entries = _tables(frames, DETECT_BITS)
    return frames, recs, entries


@pytest.mark.parametrize("which", range(len(jc.MUTATED)))
def test_every_single_bit_flip_of_the_entries_is_an_index_error_for_that_frame_alone(which):
    frames, recs, entries = _detect_batch()
    lo, n = int(recs["first_entry"][which]), int(recs["nentries"][which])
    rng = np.random.default_rng(5200 + which)
    first_of_segment = 0
    for _ in range(300):
        e, word, bit = int(rng.integers(lo, lo + n)), int(rng.integers(0, 2)), int(rng.integers(0, 32))
        bad = entries.copy()
        bad[e, word] ^= np.uint32(1 << bit)
        first_of_segment += int(entries[e, 0] == 0 and entries[e, 1] == 0)
        status, got = _decode(frames, [0, 1, 2], recs, bad, DETECT_BITS)
        want = [0, 0, 0]
        want[which] = _jpeglib.EINDEX
        assert status.tolist() == want, (jc.MUTATED[which], e - lo, word, bit, status)
        for k in range(3):
            assert k == which or np.array_equal(got[k], frames[k].want)
    assert first_of_segment > 0 or jc.MUTATED[which] == "c444_48x40_q95_noise"     # entry 0 of a segment is checked too


def test_a_wrong_record_or_id_is_refused_for_that_frame_alone():
    frames, recs, entries = _detect_batch()
    total = len(entries)

    def run(which, ids=(0, 1, 2), want=_jpeglib.EINVAL, **fields):
        r = recs.copy()
        for name, value in fields.items():
            r[name][which] = value
        status, got = _decode(frames, list(ids), r, entries, DETECT_BITS)
        assert status[which] == want and not status[[k for k in range(3) if k != which]].any(), (which, fields, ids, status)
        for k in range(3):
            assert k == which or np.array_equal(got[k], frames[k].want)

    n1 = int(recs["nentries"][1])
    run(1, nentries=n1 + 1)
    run(1, nentries=n1 - 1)
    run(1, nentries=0)
    run(1, nentries=-n1)
    run(2, nentries=int(recs["nentries"][2]) + 1)            # the last frame's: beyond the entry array
    run(1, first_entry=total - n1 + 1)                       # ends beyond the entry array
    run(1, first_entry=-1)
    run(1, first_entry=1 << 40)
    run(0, ids=(-1, 1, 2))
    run(2, ids=(0, 1, 3))
    run(1, ids=(0, -(1 << 31), 2))
    # a first_entry that stays inside the array names other entries: an index error (the start state, or a hand-over)
    run(1, first_entry=int(recs["first_entry"][1]) + 1, want=_jpeglib.EINDEX)
    run(1, first_entry=int(recs["first_entry"][1]) - 1, want=_jpeglib.EINDEX)
    # another frame's id with as many entries would pass the counts: its entries are not this scan's
    twin = [_frame("vid_00"), _frame("vid_02")]
    r2, e2 = _tables(twin, 1024)
    if r2["nentries"][0] == r2["nentries"][1]:
        status, _ = _decode(twin, [1, 1], r2, e2, 1024)
        assert status.tolist() == [_jpeglib.EINDEX, 0]
    # the granularity the index was not built with
    status, _ = _decode(frames, [0, 1, 2], recs, entries, 256)
    assert (status != 0).all()


def test_a_stale_index_never_gives_status_zero_with_other_coefficients():
    """The 600 seeded scan-byte changes of jpeg_entropy_cases.damaged, each decoded with the index of the file it was made
    from.  Most are caught (a hand-over that no longer matches, counts that no longer fit, a code the host decoder refuses
    too); a change that leaves every hand-over as it was -- inside the extra bits of a coefficient -- decodes with status
    0, and then to exactly what the relaxation decoder makes of the changed scan."""
    seen = {}
    good = {name: _frame(name) for name in jc.MUTATED}
    assert all(not _decode([f], [0], *_tables([f], DETECT_BITS), DETECT_BITS)[0].any() for f in good.values())
    for label, data in jc.damaged(GOOD)[:600]:
        name = label.split("/")[0]
        assert name in jc.MUTATED
        rc, info, _ = _jpeglib.parse(data)
        if rc:
            continue
        try:
            f = Frame(data)
        except AssertionError:                                # the change made a marker of the byte: nothing to decode
            continue
        recs, entries = _tables([good[name]], DETECT_BITS)
        status, got = _decode([f], [0], recs, entries, DETECT_BITS)
        seen[int(status[0])] = seen.get(int(status[0]), 0) + 1
        if status[0] == 0:
            ref = np.full(f.count + 2 * GUARD, 0x5A5A, np.int16)
            st, _, _, _ = _jpeglib.entropy_decode_parallel_host(data, f.info, ref.ctypes.data + 2 * GUARD, DETECT_BITS)
            assert st == 0 and np.array_equal(got[0], ref[GUARD:GUARD + f.count]), label
            assert f.host_rc == 0 and np.array_equal(got[0], f.want), label
    print(seen)
    assert seen.get(_jpeglib.EINDEX, 0) > 0 and set(seen) <= {0, _jpeglib.EINDEX, _jpeglib.EINVAL, _jpeglib.ECORRUPT}


# --------------------------------------------------------------------------- 4. the sanitised stand-alone program
def test_the_same_lists_in_a_sanitised_stand_alone_program(tmp_path):
    """host.cpp, scan.cpp, index_host.cpp and the core headers compiled with -fsanitize=address,undefined into a program of
    their own, run as a child process on every good case and every damaged stream; nothing sanitised is loaded into this
    interpreter."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    names = list(GOOD)
    blobs = [(-1, GOOD[k]) for k in names]
    for label, data in jc.damaged(GOOD):
        base = label.split("/")[0].split("[")[0]
        blobs.append((names.index(base), data))
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(blobs)))
        for base, b in blobs:
            f.write(struct.pack("<iI", base, len(b)))
            f.write(b)
    src = os.path.join(ROOT, "x3d-multigrid_amd", "csrc_jpeg")
    exe = str(tmp_path / "jpeg_index_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "jpeg_index_check.cpp")]
    cmd += [os.path.join(src, k) for k in ("host.cpp", "scan.cpp", "index_host.cpp")] + ["-o", exe]
    # the sanitisers' runtimes linked into the program itself where the compiler ships them so (gcc needs to be told)
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "cases" and int(last[1]) == len(blobs) and int(last[-1]) == 0, r.stdout[-500:]
    assert int(last[3]) == 3 * len(GOOD) == int(last[5]) and int(last[7]) > 3 * 500 and int(last[9]) > 0


# --------------------------------------------------------------------------- 5. FrameStore and the sidecar of a pack
NAMES, FILES = sr.good_files()
STORE_BITS = 128


def _store(files=FILES, **kw):
    from x3dhip import jpegstore
    _lib()
    mem = HostMemory()
    store = jpegstore.FrameStore("cpu", memory=mem, **kw)
    if files:
        store.add(files)
    return store, mem


def _load(path, **kw):
    from x3dhip import jpegstore
    store, meta, id_map = jpegstore.FrameStore.load(path, "cpu", memory=HostMemory(), **kw)
    return store, meta, id_map


def _index_is_the_files(store, files, bits):
    """The store's index tables are what the restatement gives for the files, frame by frame, and decode them."""
    n = len(files)
    assert store.index_bits == bits and len(store) == n
    recs = store._index_recs.host[:n]
    entries = store._entries.host[:store._entries.n].view("<u4").reshape(-1, 2)
    want = [_jpeglib.index_build(*_jpeglib.scan_prepare(f, _jpeglib.parse(f)[1])[1:3], _jpeglib.parse(f)[1], bits)[1] for f in files]
    assert np.array_equal(store.nentries, [len(w) for w in want]) and np.array_equal(recs["nentries"], store.nentries)
    assert np.array_equal(recs["first_entry"], np.cumsum(store.nentries) - store.nentries) and not recs["pad"].any()
    assert store._entries.n == int(store.nentries.sum()) and entries.tobytes() == np.concatenate(want).tobytes()
    # decoded straight from the store's own memory
    heads = store._headers.host[store._recs.host["header"][:n]]["scan"]
    sj = np.ascontiguousarray(heads).copy()
    r = store._recs.host[:n]
    sj["scan"], sj["segs"], sj["scan_bytes"], sj["nseg"] = r["scan"], r["segs"], r["scan_bytes"], r["nseg"]
    coef = [np.zeros(int(c), np.int16) for c in store.coef_count]
    sj["coef"] = [c.ctypes.data for c in coef]
    status = np.full(n, 77, np.int32)
    ids = np.arange(n, dtype=np.int32)
    _jpeglib.check(_lib().x3djpeg_entropy_decode_indexed_host(sj.ctypes.data, n, ids.ctypes.data, recs.ctypes.data, n,
                                                              entries.ctypes.data, len(entries), bits, status.ctypes.data))
    assert not status.any()
    for k, f in enumerate(files):
        info = _jpeglib.parse(f)[1]
        want16 = np.zeros(int(info["coef_count"][0]), np.int16)
        assert _jpeglib.entropy_decode(f, info, want16.ctypes.data, want16.nbytes)[0] == 0 and np.array_equal(coef[k], want16), k


def test_an_indexed_store_builds_grows_and_counts_its_index():
    from x3dhip import jpegstore
    from x3dhip._lib import X3DHipError
    plain, _ = _store()
    assert plain.index_bits is None and plain.bytes_index() == 0 and not plain.nentries.any()
    store, _ = _store(files=FILES[:5], index_bits=32, threads=3)      # 32: enough entries to outgrow the first buffer
    first = store._entries.dev
    assert store._entries.n <= (1 << 14) and store.add(FILES[5:]) == range(5, len(FILES))
    _index_is_the_files(store, FILES, 32)
    # the entry array grew into a new buffer (a planned batch keeps the old one), and the store counts what it holds
    assert store._entries.n > (1 << 14) and store._entries.dev is not first
    assert store.bytes_index() == store._entries.nbytes + store._index_recs.nbytes >= 8 * store._entries.n + 16 * len(store)
    assert store.bytes_resident() - store.bytes_index() == plain.bytes_resident()
    assert jpegstore.FrameStore("cpu", memory=HostMemory(), index_bits=True).index_bits == _jpeglib.INDEX_BITS_DEFAULT
    for bad in (48, 16, 0, 1 << 21):
        with pytest.raises(ValueError, match="index_bits"):
            jpegstore.FrameStore("cpu", memory=HostMemory(), index_bits=bad)
    # a file the indexer refuses: add names it and stores nothing.  The scan's last byte cut off: headers and scan
    # preparation pass, the last block does not decode.
    cut = FILES[3][:-40]
    assert _jpeglib.parse(cut)[0] == 0
    before = (len(store), store._entries.n, store._index_recs.n, store.n_chunks)
    with pytest.raises(X3DHipError, match="JPEG frame 1 of the batch.*corrupt"):
        store.add([FILES[0], cut, FILES[1]])
    assert (len(store), store._entries.n, store._index_recs.n, store.n_chunks) == before
    from x3dhip.jpegops import status_text
    assert "index" in status_text(_jpeglib.EINDEX) and "index" not in status_text(_jpeglib.ECORRUPT)


def test_pack_and_sidecar_round_trip(tmp_path):
    from x3dhip import jpegstore
    store, _ = _store(chunk_bytes=8192, index_bits=STORE_BITS)
    plain, _ = _store(chunk_bytes=8192)
    assert store.n_chunks >= 3
    path, ppath = str(tmp_path / "indexed.pack"), str(tmp_path / "plain.pack")
    store.save(path, {"k": 1})
    plain.save(ppath, {"k": 1})
    # the pack of an indexed store is the pack of a store without one, byte for byte; only the indexed one has a sidecar
    assert open(path, "rb").read() == open(ppath, "rb").read()
    assert os.path.exists(path + ".idx") and not os.path.exists(ppath + ".idx")
    assert jpegstore.PACK_VERSION == 1 and jpegstore.INDEX_SUFFIX == ".idx"
    side = os.path.getsize(path + ".idx")
    assert side == ((jpegstore.INDEX_HEAD.size + 4 * len(FILES) + 7) & ~7) + 8 * int(store.nentries.sum())
    got, meta, id_map = _load(path, chunk_bytes=1 << 20)
    assert meta == {"k": 1} and id_map == [range(len(FILES))]
    _index_is_the_files(got, FILES, STORE_BITS)
    # index=False ignores the sidecar; an int builds the index while loading, at that granularity; a pack without a
    # sidecar loads as ever
    assert _load(path, index=False)[0].index_bits is None and _load(ppath)[0].index_bits is None
    _index_is_the_files(_load(path, index=1024, chunk_bytes=8192)[0], FILES, 1024)
    _index_is_the_files(_load(ppath, index=32)[0], FILES, 32)
    assert _load(ppath, index=True)[0].index_bits == _jpeglib.INDEX_BITS_DEFAULT
    # a loaded store takes more frames
    got.add(FILES[:3])
    _index_is_the_files(got, FILES + FILES[:3], STORE_BITS)
    # ranges: only the shard's entries, in the order asked for
    n = len(FILES)
    ranges = [range(n - 4, n), range(5, 9), range(0, 2), range(5, 9), range(3, 3)]
    got, _, id_map = _load(path, ranges=ranges, chunk_bytes=8192)
    assert id_map == [range(0, 4), range(4, 8), range(8, 10), range(10, 14), range(14, 14)]
    _index_is_the_files(got, [FILES[i] for r in ranges for i in r], STORE_BITS)
    empty, _ = _store(files=(), index_bits=STORE_BITS)
    empty.save(str(tmp_path / "empty.pack"))
    got, _, _ = _load(str(tmp_path / "empty.pack"))
    assert len(got) == 0 and got.index_bits == STORE_BITS


def test_load_refuses_a_damaged_sidecar(tmp_path):
    from x3dhip import jpegstore
    store, _ = _store(chunk_bytes=8192, index_bits=STORE_BITS)
    path = str(tmp_path / "good.pack")
    store.save(path)
    good = open(path + ".idx", "rb").read()
    _load(path)
    head = jpegstore.INDEX_HEAD
    fields = list(head.unpack(good[:head.size]))
    assert fields[:3] == [b"X3DJPIDX", 1, STORE_BITS] and fields[3] == len(FILES) and fields[5] == int(store.nentries.sum())
    counts = np.frombuffer(good[head.size:head.size + 4 * len(FILES)], "<u4")
    assert np.array_equal(counts, store.nentries)

    def with_head(at, value):
        f = list(fields)
        f[at] = value
        return head.pack(*f) + good[head.size:]

    def with_count(i, value):
        c = counts.copy()
        c[i] = value
        return good[:head.size] + c.tobytes() + good[head.size + c.nbytes:]

    bad = {"magic": with_head(0, b"X3DJPIDY"), "version": with_head(1, 2), "version 0": with_head(1, 0),
           "index_bits another": with_head(2, 2 * STORE_BITS), "index_bits finer": with_head(2, STORE_BITS // 2),
           "index_bits odd": with_head(2, 48), "index_bits 0": with_head(2, 0),
           "frames": with_head(3, fields[3] + 1), "frames less": with_head(3, fields[3] - 1),
           "arena bytes": with_head(4, fields[4] + 16), "entries": with_head(5, fields[5] + 1),
           "entries less": with_head(5, fields[5] - 1), "a count": with_count(2, int(counts[2]) + 1),
           "two counts": with_count(4, int(counts[4]) + 1)[:head.size + 20] + with_count(5, int(counts[5]) - 1)[head.size + 20:],
           "a count of zero": with_count(0, 0), "empty": b"", "short head": good[:20]}
    for step in range(0, len(good), 4096):                  # truncation at every 4 KB boundary
        bad["cut at %d" % step] = good[:step]
    bad["one byte short"] = good[:-1]
    bad["one byte long"] = good + b" "
    for label, data in bad.items():
        with open(path + ".idx", "wb") as f:
            f.write(data)
        for kw in (dict(), dict(ranges=[range(0, 1)])):
            with pytest.raises(ValueError):
                _load(path, **kw)
            assert label
        assert _load(path, index=False)[0].index_bits is None           # the pack itself is fine
    # the sidecar of another pack with as many frames: its arena is another
    other, _ = _store(files=FILES[::-1], chunk_bytes=8192, index_bits=STORE_BITS)
    other.save(str(tmp_path / "other.pack"))
    with open(path + ".idx", "wb") as f:
        f.write(open(str(tmp_path / "other.pack") + ".idx", "rb").read())
    if os.path.getsize(str(tmp_path / "other.pack")) == os.path.getsize(path):
        with pytest.raises(ValueError):                     # the counts are checked against the segment tables
            _load(path)
    # damaged entries are not the loader's business: they load, and the decoder reports them
    with open(path + ".idx", "wb") as f:
        f.write(good[:-8] + bytes(b ^ 0xFF for b in good[-8:]))
    assert _load(path)[0].index_bits == STORE_BITS


def test_pack_frames_writes_the_sidecar_without_a_gpu(tmp_path, monkeypatch, capsys):
    import frames
    from tools import pack_frames
    _lib()
    monkeypatch.setattr(frames, "MIN_FRAMES", tr.MIN_FRAMES)
    root, anno, labels = tr.write_tree(tmp_path, "validate")
    plain, indexed, default = (str(tmp_path / k) for k in ("plain.pack", "indexed.pack", "default.pack"))
    common = ["--root", root, "--anno", anno, "--labels", labels, "--subset", "validate", "--threads", "2"]
    pack_frames.main(common + ["--out", plain])
    pack_frames.main(common + ["--out", indexed, "--index-bits", "256"])
    pack_frames.main(common + ["--index-bits", "--out", default])
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 5 and out[2].startswith(indexed + ".idx: ") and out[4].startswith(default + ".idx: ")
    assert open(plain, "rb").read() == open(indexed, "rb").read() == open(default, "rb").read()
    assert not os.path.exists(plain + ".idx")
    entries = frames.list_annotation(root, anno, labels, "validate")
    files = [f for (folder, _), t in zip(entries, tr.TREE) for f in folder.read(list(range(t[2])))]
    _index_is_the_files(_load(indexed)[0], files, 256)
    _index_is_the_files(_load(default)[0], files, _jpeglib.INDEX_BITS_DEFAULT)


def test_the_option_reaches_the_stores_of_the_datasets(monkeypatch):
    import frames
    from x3dhip import jpegstore
    seen = []
    real = jpegstore.FrameStore

    class Spy(real):
        def __init__(self, device, **kw):
            seen.append(kw)
            raise RuntimeError("seen")

        @classmethod
        def load(cls, path, device, **kw):
            seen.append(kw)
            raise RuntimeError("seen")

        @classmethod
        def read_meta(cls, path):
            return {"videos": [dict(first=0, frames=2)]}

    monkeypatch.setattr(jpegstore, "FrameStore", Spy)
    monkeypatch.setattr(frames, "list_annotation", lambda *a: [("folder", 0)])
    for call, key in ((lambda **kw: frames.StoredKinetics.from_annotation("R", "A", "L", "train", **kw), "index_bits"),
                      (lambda **kw: frames.StoredKinetics.from_pack("P", **kw), "index"),
                      (lambda **kw: frames.charades_videos("R", {}, "cuda:0", resident="compressed", **kw), "index_bits")):
        for given in (dict(), dict(index_bits=256)):
            with pytest.raises(RuntimeError, match="seen"):
                call(**given)
            assert seen[-1][key] == given.get("index_bits"), (key, given)
    src = os.path.join(ROOT, "x3d-multigrid_amd")
    for script in ("train_x3d_charades.py", "train_x3d_kinetics_multigrid.py", "score_x3d_kinetics_store.py"):
        text = open(os.path.join(src, script)).read()
        assert "'--index-bits', type=int, nargs='?', const=True, default=None" in text and "index_bits=args.index_bits" in text
    assert "_cls.main(run" in open(os.path.join(src, "train_x3d_charades_loc.py")).read()     # the same parser


# --------------------------------------------------------------------------- 6. ABI
def test_index_symbols_structs_and_argument_checks():
    h = _lib()
    assert _jpeglib.ABI_VERSION == 2 and h.x3djpeg_abi_version() == 2
    assert h.x3djpeg_index_rec_bytes() == _jpeglib.INDEX_REC_DT.itemsize == 16
    assert _jpeglib.EINDEX == -5
    src = open(os.path.join(ROOT, "include", "x3djpeg.h")).read()
    assert re.search(r"#define X3DJPEG_ABI_VERSION 2\b", src) and re.search(r"#define X3DJPEG_EINDEX \(-5\)", src)
    assert re.search(r"#define X3DJPEG_INDEX_BITS_DEFAULT %d\b" % _jpeglib.INDEX_BITS_DEFAULT, src)
    assert re.search(r"#define X3DJPEG_INDEX_MAX_BLOCKS \(1 << 22\)", src) and _jpeglib.INDEX_MAX_BLOCKS == 1 << 22
    body = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(x3djpeg_[a-z0-9_]+)\s*\(", body))
    for name in NEW:
        assert name in declared and name in _jpeglib.SIGNATURES and hasattr(h, name), name
        assert not name.startswith("x3djpeg_store_")
    assert len([k for k in _jpeglib.SIGNATURES if k.startswith("x3djpeg_store_")]) == 6
    dev, host = _jpeglib.SIGNATURES["x3djpeg_entropy_decode_indexed"], _jpeglib.SIGNATURES["x3djpeg_entropy_decode_indexed_host"]
    assert dev[1][:-1] == host[1] and len(dev[1]) == 10
    # one null, a bad count, a bad granularity, an unaligned table: each refused before anything is read or launched
    f = _frame("vid_00")
    recs, entries = _tables([f], 128)
    sj = np.zeros(1, _jpeglib.SCAN_JOB_DT)
    ids, status = np.zeros(1, np.int32), np.zeros(1, np.int32)
    args = [sj.ctypes.data, 1, ids.ctypes.data, recs.ctypes.data, 1, entries.ctypes.data, len(entries), 128, status.ctypes.data]
    assert h.x3djpeg_entropy_decode_indexed_host(*args) == 0 and status[0] == _jpeglib.EINVAL       # a job of zeros
    for at, bad in ((0, None), (2, None), (3, None), (5, None), (8, None), (1, 0), (4, 0), (7, 48), (7, 0), (7, 1 << 21),
                    (5, entries.ctypes.data + 4), (3, recs.ctypes.data + 4)):
        a = list(args)
        a[at] = bad
        assert h.x3djpeg_entropy_decode_indexed_host(*a) == _jpeglib.EINVAL, (at, bad)
        assert h.x3djpeg_entropy_decode_indexed(*a, None) == _jpeglib.EINVAL, (at, bad)
    assert b"argument check failed" in h.x3djpeg_last_error()
    assert h.x3djpeg_entropy_decode_indexed(*(args[:1] + [65536] + args[2:]), None) == _jpeglib.EINVAL
