"""The frame store on the GPU (x3djpeg_store_build_jobs, x3dhip.jpegstore.FrameStore, frames.StoredVideo): the job tables
the two kernels build equal the CPU twin's byte for byte, across the plan kernel's workgroup and chunk sizes; pixels equal
JpegDecoder(entropy="host") and Pillow's goldens for every good case at three subsequence lengths, alone and mixed, with
the guards around the coefficient buffer intact; a store that grows keeps decoding what it held; refused requests (only
lists the sanitised CPU run of tests/test_jpeg_store_host.py has been through) fail alone and leave their destination
untouched; a captured plan replays on other frames; Charades over stored videos gives the batches it gives over decoded
ones, bit for bit, and so does the training script."""
import json
import os
import random
import re
import sys

import numpy as np
import pytest
import torch

import frames
from tests import jpeg_entropy_cases as jc
from tests import jpeg_ref as jr
from tests import jpegstore_ref as sr
from x3dhip import _jpeglib, jpegops, jpegstore
from x3dhip._jpeglib import FRAME_JOB_DT, SCAN_JOB_DT, STORE_DST_DT
from x3dhip._lib import X3DHipError, stream

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NAMES, FILES = sr.good_files()
GOLD = {k: v[1] for k, v in list(jr.load_cases().items()) + list(jc.load_entropy_cases().items()) if v[1] is not None}
GUARD = 64          # int16 elements on either side of the coefficient buffer, bytes on either side of the job tables
_WANT = {}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _want():
    """JpegDecoder(entropy='host') on every good case, once: {name: uint8 [H, W, 3]}."""
    if not _WANT:
        outs = jpegops.JpegDecoder(DEV, threads=4).decode(FILES)
        _WANT.update(zip(NAMES, outs))
        for k, g in GOLD.items():
            if k in _WANT:
                assert torch.equal(_WANT[k], _t(g)), k
    return _WANT


class _View:
    """What jpegstore_ref.restate and twin ask of a store's tables, from a FrameStore's host copies."""

    def __init__(self, store, files):
        n = len(store)
        self.n, self.scan_bytes, self.nseg = n, store.scan_bytes.astype(np.int64), store.nseg.astype(np.int64)
        self.infos = np.concatenate([_jpeglib.parse(f)[1] for f in files])
        self._keep = [sr.aligned(store._recs.host[:n].nbytes), sr.aligned(store._headers.host[:store.n_headers].nbytes)]
        self._keep[0][1][:] = store._recs.host[:n].view(np.uint8).reshape(-1)
        self._keep[1][1][:] = store._headers.host[:store.n_headers].view(np.uint8).reshape(-1)
        self.recs = self._keep[0][1].view(_jpeglib.STORE_REC_DT)
        self.headers = self._keep[1][1].view(_jpeglib.STORE_HEADER_DT)


def _build(store, ids, dst, coef_cap, ws_cap, decode=False, max_blocks=0, max_w=0, max_h=0):
    """x3djpeg_store_build_jobs alone on the store's device tables (then, for decode=True, the three launches of the device
    path) with guards around the job tables, the plan and the coefficient buffer.  ids: any int32 values; dst:
    STORE_DST_DT [n].  Returns a dict of numpy / tensors; asserts the guards."""
    n = len(ids)
    sjb, fjb = n * SCAN_JOB_DT.itemsize, n * FRAME_JOB_DT.itemsize
    tables = torch.full((GUARD + sjb + GUARD + fjb + GUARD + 8 * (3 * n + 2) + GUARD,), 0x3C, dtype=torch.uint8, device=DEV)
    sj_at, fj_at, plan_at = GUARD, 2 * GUARD + sjb, 3 * GUARD + sjb + fjb
    coef = torch.full((coef_cap + 2 * GUARD,), 0x5A5A, dtype=torch.int16, device=DEV)
    planes = torch.zeros(max(coef_cap, 1), dtype=torch.uint8, device=DEV)
    ws = torch.zeros(max(ws_cap, 16), dtype=torch.uint8, device=DEV)
    status = torch.full((n + 1,), 77, dtype=torch.int32, device=DEV)
    idt, dt = _t(np.asarray(ids, np.int32)), _t(dst.view(np.uint8).reshape(-1))
    L, mem, base = _jpeglib.lib(), store.memory, tables.data_ptr()
    coef_ptr = coef.data_ptr() + 2 * GUARD
    _jpeglib.check(L.x3djpeg_store_build_jobs(
        mem.ptr(store._recs.dev), len(store), mem.ptr(store._headers.dev), store.n_headers, idt.data_ptr(), n, store.sub_bits,
        coef_ptr, coef_cap, planes.data_ptr(), coef_cap, ws_cap, dt.data_ptr(), base + plan_at, base + sj_at, base + fj_at,
        status.data_ptr() + 4 * n, stream()))
    if decode:
        _jpeglib.check(L.x3djpeg_entropy_decode_batch(base + sj_at, n, store.sub_bits, ws.data_ptr(), ws_cap, status.data_ptr(),
                                                      stream()))
        _jpeglib.check(L.x3djpeg_decode_batch(base + fj_at, n, max_blocks, max_w, max_h, stream()))
    torch.cuda.synchronize()
    host = tables.cpu().numpy()
    for lo, hi in ((0, sj_at), (sj_at + sjb, fj_at), (fj_at + fjb, plan_at), (plan_at + 8 * (3 * n + 2), host.size)):
        assert (host[lo:hi] == 0x3C).all(), "guard of the job tables overwritten"
    assert bool((coef[:GUARD] == 0x5A5A).all()) and bool((coef[GUARD + coef_cap:] == 0x5A5A).all()), "coefficient guard overwritten"
    st = status.cpu().numpy()
    return dict(sj=host[sj_at:sj_at + sjb].view(SCAN_JOB_DT), fj=host[fj_at:fj_at + fjb].view(FRAME_JOB_DT),
                plan=host[plan_at:plan_at + 8 * (3 * n + 2)].view(np.int64), build_status=int(st[n]), status=st[:n],
                coef_ptr=coef_ptr, planes_ptr=planes.data_ptr())


# --------------------------------------------------------------------------- 7. job tables
SMALL = ["c420_40x24_blocks1", "c444_8x8", "c420_40x24_blocks1", "grey_30x44"]


@pytest.fixture(scope="module")
def small():
    files = [FILES[NAMES.index(k)] for k in SMALL]
    store = jpegstore.FrameStore(DEV, chunk_bytes=1 << 16, sub_bits=128)
    store.add(files)
    return store, _View(store, files)


@pytest.mark.parametrize("n", [1, 2, _jpeglib.STORE_PLAN_THREADS + 1, _jpeglib.STORE_PLAN_CHUNK + 1,
                               2 * _jpeglib.STORE_PLAN_CHUNK + 3])
def test_job_tables_equal_the_cpu_twin(small, n):
    """The 40 x 24 fixture repeated (ids 0 and 2), with two other small frames mixed in from n = 257 on so that the sums the
    carry takes across a pass differ from request to request."""
    store, T = small
    ids = [0] if n == 1 else [2, 2] if n == 2 else [(0, 1, 2, 3, 0, 0, 3)[i % 7] for i in range(n)]
    dst = sr.dst_table(T, ids)
    counts = T.infos["coef_count"][ids].astype(np.int64)
    coef_cap, ws_cap = int(counts.sum()), int(sr.workspace_bytes(T.scan_bytes[ids], T.nseg[ids], 128).sum())
    got = _build(store, ids, dst, coef_cap, ws_cap)
    want = sr.twin(T, ids, dst, 128, got["coef_ptr"], got["planes_ptr"], coef_cap, coef_cap, ws_cap)
    for key, w in zip(("sj", "fj", "plan"), want[:3]):
        g = torch.from_numpy(got[key].view(np.uint8).copy())
        assert torch.equal(g, torch.from_numpy(w.view(np.uint8).reshape(-1).copy())), (n, key)
    assert got["build_status"] == want[3] == 0
    # pointer fields as offsets from their bases: into the coefficient buffer, the planes, the arena
    assert np.array_equal(got["sj"]["coef"] - np.uint64(got["coef_ptr"]), (2 * np.cumsum(counts) - 2 * counts).astype(np.uint64))
    assert np.array_equal(got["fj"]["planes"] - np.uint64(got["planes_ptr"]), (np.cumsum(counts) - counts).astype(np.uint64))
    scan_at, seg_at = store.addresses(ids)
    assert np.array_equal(got["sj"]["scan"], scan_at) and np.array_equal(got["sj"]["segs"], seg_at)
    if n > _jpeglib.STORE_PLAN_CHUNK:
        assert got["plan"][_jpeglib.STORE_PLAN_CHUNK] == counts[:_jpeglib.STORE_PLAN_CHUNK].sum()      # across the carry


# --------------------------------------------------------------------------- 8. pixels
@pytest.fixture(scope="module", params=jc.SUB_BITS)
def full(request):
    store = jpegstore.FrameStore(DEV, sub_bits=request.param, threads=2)
    assert store.add(FILES) == range(len(FILES)) and store.sub_bits == request.param
    return store


def test_every_case_alone_equals_the_host_path_and_pillow(full):
    want = _want()
    for i, k in enumerate(NAMES):
        (got,) = full.decode([i])
        assert got.dtype == torch.uint8 and torch.equal(got, want[k]), (k, full.sub_bits)
        if k in GOLD:
            assert torch.equal(got, _t(GOLD[k])), k
    assert not full.last_batch.status.any() and int(full.last_batch.build_status) == 0


def test_one_mixed_scrambled_batch_equals_the_host_path_inside_the_guards(full):
    want = _want()
    ids = sr.served_lists(len(FILES))["scrambled"] + [3, 3]
    outs = full.decode(ids)
    for i, o in zip(ids, outs):
        assert torch.equal(o, want[NAMES[i]]), (NAMES[i], full.sub_bits)
    # the same batch through the entry points, the coefficient buffer between guards and of exactly the size asked for
    T = _View(full, FILES)
    w, h = full.width[ids].astype(np.int64), full.height[ids].astype(np.int64)
    at = np.cumsum(3 * w * h) - 3 * w * h
    flat = torch.full((int((3 * w * h).sum()) + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    dst = np.zeros(len(ids), STORE_DST_DT)
    dst["dst"], dst["dst_stride"], dst["width"], dst["height"] = flat.data_ptr() + GUARD + at, 3 * w, w, h
    got = _build(full, ids, dst, int(full.coef_count[ids].sum()), int(full.ws_need[ids].sum()), decode=True,
                 max_blocks=int(full.nblocks[ids].max()), max_w=int(w.max()), max_h=int(h.max()))
    assert got["build_status"] == 0 and not got["status"].any()
    assert bool((flat[:GUARD] == 0xA5).all()) and bool((flat[-GUARD:] == 0xA5).all())
    for k, i in enumerate(ids):
        o = flat[GUARD + at[k]:GUARD + at[k] + 3 * w[k] * h[k]].view(int(h[k]), int(w[k]), 3)
        assert torch.equal(o, want[NAMES[i]]), (NAMES[i], full.sub_bits)
    assert np.array_equal(full.ws_need, sr.workspace_bytes(full.scan_bytes, full.nseg, full.sub_bits))
    assert T.n == len(FILES)


def test_decode_into_takes_strided_slots_and_checks_its_arguments(full):
    want = _want()
    vid = [NAMES.index("vid_%02d" % t) for t in (7, 0, 7, 11)]
    H, W, _ = want["vid_00"].shape
    pitch = 3 * W + 16
    raw = torch.full((6, H, pitch), 0xA5, dtype=torch.uint8, device=DEV)       # guard frame, four slots, guard frame
    dst = raw.as_strided((4, H, W, 3), (H * pitch, pitch, 3, 1), H * pitch)
    assert full.decode_into(vid, dst) is dst
    for k, i in enumerate(vid):
        assert torch.equal(dst[k], want[NAMES[i]]), k
    assert bool((raw[0] == 0xA5).all()) and bool((raw[5] == 0xA5).all()) and bool((raw[1:5, :, 3 * W:] == 0xA5).all())
    # the Python layer refuses a bad id or a frame of another size before anything is launched
    full.last_batch = None
    for bad in ([-1], [len(full)], [0, len(full) + 5], []):
        with pytest.raises(ValueError):
            full.decode(bad)
    with pytest.raises(ValueError, match=r"frame 1 is"):
        full.decode_into([vid[0], NAMES.index("c444_8x8"), vid[1], vid[2]], dst)
    with pytest.raises(ValueError):
        full.decode_into(vid[:3], dst)
    assert full.last_batch is None and bool((raw[0] == 0xA5).all())
    assert full.bytes_resident() >= sum(int(s) for s in full.scan_bytes) and len(full) == len(FILES)


# --------------------------------------------------------------------------- 9. growth
def test_a_store_that_grows_keeps_decoding_what_it_held():
    want = _want()
    small = [i for i, f in enumerate(FILES) if len(f) < 4000]
    store = jpegstore.FrameStore(DEV, chunk_bytes=4096, sub_bits=128)
    held, chunks = [], []
    for lo in range(0, len(small), 6):
        part = small[lo:lo + 6]
        ids = store.add([FILES[i] for i in part])
        assert ids == range(len(held), len(held) + len(part))
        held += part
        chunks.append(store.n_chunks)
        order = list(range(len(held)))[::-1]                # frames added before and after every growth so far
        for i, o in zip(order, store.decode(order)):
            assert torch.equal(o, want[NAMES[held[i]]]), (lo, NAMES[held[i]])
    assert chunks[-1] >= 4 and len(set(chunks)) >= 3 and len(held) > 24
    lo, hi = store.addresses()
    for c in range(store.n_chunks):                         # no frame is split: each lies inside its own chunk
        base = store.memory.ptr(store._chunks[c][0])
        mine = np.flatnonzero(store._mirror["chunk"][:len(store)] == c)
        assert mine.size and (lo[mine] >= base).all() and (hi[mine] + 16 * store.nseg[mine] <= base + store._chunks[c][1]).all()


# --------------------------------------------------------------------------- 10. refusals on the device
@pytest.mark.parametrize("label", ["id_minus_1", "id_nrecs", "wider", "coef_short", "ws_short"])
def test_a_refused_request_fails_alone_and_leaves_its_destination_untouched(label):
    """The five-request lists of tests/test_jpeg_store_host.py, which its sanitised stand-alone program has been through."""
    want = _want()
    store = jpegstore.FrameStore(DEV, sub_bits=128)
    store.add(FILES)
    T = _View(store, FILES)
    ids, wider, coef_short, ws_short, bit, refused = sr.refused_lists(NAMES)[label]
    n = len(ids)
    plan = sr.restate(T, ids, sr.dst_table(T, ids), 128, 0, 0)[2]
    counts = np.diff(np.concatenate([plan[:n], plan[3 * n:3 * n + 1]]))
    ws = np.diff(np.concatenate([plan[n:2 * n], plan[3 * n + 1:]]))
    coef_cap = int(plan[3 * n]) if coef_short is None else int(plan[coef_short] + counts[coef_short] - 1)
    ws_cap = int(plan[3 * n + 1]) if ws_short is None else int(plan[n + ws_short] + ws[ws_short] - 1)
    dst = sr.dst_table(T, ids, base=0, wider=wider)
    room = int(dst["dst"][-1] + 3 * (dst["width"][-1] + 1) * dst["height"][-1])
    out = torch.full((room,), 0xA5, dtype=torch.uint8, device=DEV)
    dst["dst"] += np.uint64(out.data_ptr())
    ok = [i for i in ids if 0 <= i < T.n]
    got = _build(store, ids, dst, coef_cap, ws_cap, decode=True, max_blocks=int(store.nblocks[ok].max()),
                 max_w=int(store.width[ok].max()) + 1, max_h=int(store.height[ok].max()))
    assert got["build_status"] == bit
    assert [i for i in range(n) if got["plan"][2 * n + i]] == list(refused)
    edges = [int(p) - out.data_ptr() for p in dst["dst"]] + [room]
    for k in range(n):
        mine = out[edges[k]:edges[k + 1]]
        if k in refused:
            assert got["status"][k] == _jpeglib.EINVAL and bool((mine == 0xA5).all()), (label, k)
            assert not got["sj"][k:k + 1].view(np.uint8).any() and not got["fj"][k:k + 1].view(np.uint8).any()
        else:
            w = want[NAMES[ids[k]]]
            assert got["status"][k] == 0 and torch.equal(mine[:w.numel()].view(w.shape), w), (label, k)
            assert bool((mine[w.numel():] == 0xA5).all())
    # the Python layer: a refusal found on the device is an error naming the frame, and check=False leaves it in last_batch
    if label == "wider":
        b = store.plan(3, 37, 53)
        b.ids.copy_(_t(np.array([ids[0], ids[0], ids[1]], np.int32)))          # the last one is 64 x 48
        b.dst.fill_(0xA5)
        b.launch()
        torch.cuda.synchronize()
        assert b.status.cpu().tolist() == [0, 0, _jpeglib.EINVAL] and int(b.build_status) & _jpeglib.STORE_BAD_SIZE
        assert torch.equal(b.dst[0], want[NAMES[ids[0]]]) and torch.equal(b.dst[1], b.dst[0]) and bool((b.dst[2] == 0xA5).all())
        with pytest.raises(X3DHipError, match=r"frame 2 of the batch.*another size"):
            b.raise_for_status()


# --------------------------------------------------------------------------- 11. capture
def test_a_captured_plan_replays_on_other_frames():
    want = _want()
    store = jpegstore.FrameStore(DEV)
    store.add(FILES)
    vid = [NAMES.index("vid_%02d" % t) for t in range(12)]
    H, W, _ = want["vid_00"].shape
    first = vid[:5]
    eager = torch.stack(store.decode(first))
    b = store.plan(5, W, H)
    assert b.ids.dtype == torch.int32 and tuple(b.dst.shape) == (5, H, W, 3)
    assert b.ids.cpu().tolist() == [NAMES.index("c420_64x48_restart")] * 5       # the first stored frame of 64 x 48
    b.ids.copy_(_t(np.array(first, np.int32)))
    b.launch()
    torch.cuda.synchronize()
    assert torch.equal(b.dst, eager) and not b.status.any()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            b.launch()
    torch.cuda.current_stream().wait_stream(s)
    for pick in (first, [vid[11], vid[6], vid[6], vid[9], vid[5]], first[::-1]):
        b.ids.copy_(_t(np.array(pick, np.int32)))
        b.dst.fill_(0xA5)
        b.coef.fill_(0x5A5A)
        b.status.fill_(77)
        graph.replay()
        torch.cuda.synchronize()
        assert not b.status.any() and int(b.build_status) == 0
        assert torch.equal(b.dst, torch.stack(store.decode(pick))), pick
        for k, i in enumerate(pick):
            assert torch.equal(b.dst[k], want[NAMES[i]]), (pick, k)
    # frames added after the plan was made are outside it; the plan still serves what it knew
    more = store.add([FILES[vid[3]]] * 1500)                 # the record table grows past its first capacity
    b.ids.copy_(_t(np.array([vid[1], more[0], vid[2], vid[3], more[-1]], np.int32)))
    b.dst.fill_(0xA5)
    graph.replay()
    torch.cuda.synchronize()
    assert b.status.cpu().tolist() == [0, _jpeglib.EINVAL, 0, 0, _jpeglib.EINVAL] and int(b.build_status) == _jpeglib.STORE_BAD_ID
    assert torch.equal(b.dst[2], want["vid_02"]) and bool((b.dst[1] == 0xA5).all()) and bool((b.dst[4] == 0xA5).all())
    assert torch.equal(store.decode([more[-1]])[0], want["vid_03"])
    with pytest.raises(ValueError):
        store.plan(2, 7, 7)


# --------------------------------------------------------------------------- 12. Charades
LENGTHS = {"AAAAA": (200, 32, 24), "BBBBB": (170, 24, 32), "CCCCC": (187, 32, 24)}       # frames, width, height


def _anno(subsets):
    out = {}
    for (vid, (n, _, _)), subset in zip(LENGTHS.items(), subsets):
        dur = n / 24.0
        out[vid] = dict(subset=subset, duration=dur, actions=[[3, 0.5, dur / 2], [11, dur / 3, dur - 0.4], [156, 1.0, 1.7]])
    return out


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    Image = pytest.importorskip("PIL.Image")
    root = tmp_path_factory.mktemp("charades_frames")
    rng = np.random.default_rng(12)
    for vid, (n, w, h) in LENGTHS.items():
        os.makedirs(str(root / vid))
        y, x = np.mgrid[0:h, 0:w]
        tint = rng.integers(0, 255, 3)
        for t in range(n):
            img = np.stack([(x * 5 + t * 3 + tint[0]) % 256, (y * 7 + t + tint[1]) % 256,
                            ((x + y) * 3 + 2 * t + tint[2]) % 256], -1)
            img = (img + rng.integers(0, 24, img.shape)) % 256
            name = (frames.FRAME_NAME if vid != "BBBBB" else vid + "-{:06d}.jpg").format(t + 1)
            Image.fromarray(img.astype(np.uint8)).save(str(root / vid / name), quality=80)
    return str(root)


@pytest.fixture(scope="module")
def both(folders):
    anno = _anno(["training"] * 3)
    dec = frames.charades_videos(folders, anno, DEV, threads=2)
    sto = frames.charades_videos(folders, anno, DEV, threads=2, resident="compressed", chunk_bytes=1 << 16)
    return dec, sto


def test_stored_videos_are_the_decoded_ones_in_a_fraction_of_the_bytes(both):
    dec, sto = both
    assert list(dec) == list(sto) == list(LENGTHS)
    store = sto["AAAAA"].store
    assert all(isinstance(v, frames.StoredVideo) and v.store is store for v in sto.values())
    for vid, (n, w, h) in LENGTHS.items():
        assert tuple(sto[vid].shape) == tuple(dec[vid].shape) == (n, h, w, 3)
        idx = [0, n - 1, 5, 5, n // 2]
        assert torch.equal(sto[vid].frames(idx), dec[vid][idx])
    with pytest.raises(ValueError):
        sto["BBBBB"].frames([170])
    decoded = sum(v.numel() for v in dec.values())
    assert len(store) == sum(v[0] for v in LENGTHS.values()) and store.n_headers == 2 and store.n_chunks >= 2
    assert store.bytes_resident() < decoded / 2, (store.bytes_resident(), decoded)
    with pytest.raises(ValueError):
        frames.charades_videos("nowhere", {}, DEV, resident="hbm")


@pytest.mark.parametrize("task", ["class", "loc"])
def test_charades_batches_over_stored_videos_equal_those_over_decoded_ones(both, task):
    from charades import Charades
    dec, sto = both
    kw = dict(task=task, frames=80, gamma_tau=2, crop_size=20, c_size=20, scales=(0.8, 0.9))
    train = [Charades(_anno(["training"] * 3), "training", v, rng=random.Random(4), **kw) for v in (dec, sto)]
    assert len(train[0]) == len(train[1]) == 3 and train[0].data == train[1].data
    idx = [2, 0, 1, 0]
    params = [train[0].draw(i) for i in idx]
    a, b = train[0].batch(idx, params=params), train[1].batch(idx, params=params)
    assert len(a) == len(b) == (2 if task == "class" else 3) and tuple(a[0].shape) == (4, 3, 40, 20, 20)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and torch.equal(x, y)
    assert float(a[0].abs().sum()) > 0
    train[0].rng, train[1].rng = random.Random(9), random.Random(9)    # and with draws of their own
    a, b = train[0].batch([1, 2]), train[1].batch([1, 2])
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    test = [Charades(_anno(["testing"] * 3), "testing", v, crops=10, **kw) for v in (dec, sto)]
    if task == "class":                                     # 50, 43 and 47 strided frames: step 1, 0 and 0
        from charades import testing_windows
        assert [testing_windows(len(range(0, n, 4)), 40, 10)[0] for n, _, _ in LENGTHS.values()] == [1, 0, 0]
    a, b = test[0].test_batch([0, 1, 2]), test[1].test_batch([0, 1, 2])
    assert len(a) == len(b) == (2 if task == "class" else 3)
    assert tuple(a[0].shape) == ((3, 10, 3, 40, 20, 20) if task == "class" else (3, 3, 50, 20, 20))
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and torch.equal(x, y)
    if task == "loc":                                       # the shorter videos are padded, clips and masks
        assert tuple(a[2].shape) == (3, 200) and a[2][1].sum() == 170 and not a[0][1, :, 43:].any()
    a, b = test[0].test_batch([1]), test[1].test_batch([1])
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# --------------------------------------------------------------------------- 13. the script
def test_the_script_trains_and_validates_the_same_either_way(folders, tmp_path, monkeypatch, capsys):
    import train_x3d_charades
    anno = str(tmp_path / "charades.json")
    with open(anno, "w") as f:
        json.dump(_anno(["training", "training", "testing"]), f)
    printed = {}
    for resident in ("decoded", "compressed"):
        monkeypatch.setattr(sys, "argv", ["train_x3d_charades.py", "--anno", anno, "--frames-root", folders, "--epochs", "2",
                                          "--batch", "2", "--size", "64", "--no-graph", "--save-every", "0",
                                          "--save", str(tmp_path / "ck_"), "--resident", resident])
        torch.manual_seed(5)
        capsys.readouterr()
        train_x3d_charades.main(train_x3d_charades.run, str(tmp_path / "ck_"))
        printed[resident] = [ln for ln in capsys.readouterr().out.splitlines() if "Loss" in ln]
    lines = printed["decoded"]
    assert len(lines) == 3 and [("train" in ln) for ln in lines] == [True, True, False] and " val " in lines[2]
    assert [re.search(r"steps: (\d+)", ln).group(1) for ln in lines[:2]] == ["1", "2"]
    assert all(re.search(r"mAP: ", ln) for ln in lines)
    assert printed["compressed"] == lines
