"""The sync index on the GPU (x3djpeg_entropy_decode_indexed, FrameStore(index_bits=...)): coefficients equal the host
decoder's at three granularities and three batch sizes; pixels equal a store without an index, JpegDecoder(entropy="host")
and Pillow's goldens in both tiers; a damaged index -- only cases the CPU twin has passed first -- is reported for its
frame alone, with the neighbours right and the guards around the coefficient buffer intact; a captured plan replays on
other ids; the index arena grows; a pack and its sidecar go from one tier into the other; StoredKinetics and the Charades
script give the same with and without the index."""
import json
import random
import re
import sys

import numpy as np
import pytest
import torch

import frames
from tests import jpeg_entropy_cases as jc
from tests import jpegtier_ref as tr
from tests.test_jpeg_index_host import GOOD, GUARD, _decode, _frame, _tables
from tests.test_jpeg_store_gpu import FILES, GOLD, NAMES, _anno, _t, _want, folders  # noqa: F401
from x3dhip import _jpeglib, jpegstore
from x3dhip._lib import stream

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
EINVAL, EINDEX = _jpeglib.EINVAL, _jpeglib.EINDEX


def _indexed(jobs, ids, recs, entries, bits):
    """x3djpeg_entropy_decode_indexed on jobs (Frames of the host tests) with frame ids `ids`: the scans, segment tables,
    job table, index tables and one coefficient buffer with a guard before and after every frame's range, all on the
    device.  Returns (status [n], [int16 coefficients]) on the host; the guards are checked."""
    n = len(jobs)
    uniq = {id(f): f for f in jobs}
    where = {}
    for key, f in uniq.items():
        blob = np.concatenate([f.scan, np.zeros(-f.scan.size % 16, np.uint8), f.segs.view(np.uint8).reshape(-1)])
        dev = _t(blob)
        where[key] = (dev, dev.data_ptr(), dev.data_ptr() + f.scan.size + (-f.scan.size % 16))
    at = np.cumsum([0] + [f.count + GUARD for f in jobs]) + GUARD
    coef = torch.full((int(at[-1]),), 0x5A5A, dtype=torch.int16, device=DEV)
    sj = np.zeros(n, _jpeglib.SCAN_JOB_DT)
    for k, f in enumerate(jobs):
        _jpeglib.fill_scan_jobs(sj[k:k + 1], f.info)
        _, sj["scan"][k], sj["segs"][k] = where[id(f)]
        sj["coef"][k] = coef.data_ptr() + 2 * int(at[k])
        sj["scan_bytes"][k], sj["nseg"][k] = f.scan.size - _jpeglib.SCAN_PAD, f.segs.size
    d_sj, d_ids = _t(sj.view(np.uint8).reshape(-1)), _t(np.asarray(ids, np.int32))
    d_recs, d_ent = _t(recs.view(np.uint8).reshape(-1)), _t(np.ascontiguousarray(entries, np.uint32).reshape(-1))
    status = torch.full((n,), 77, dtype=torch.int32, device=DEV)
    _jpeglib.check(_jpeglib.lib().x3djpeg_entropy_decode_indexed(
        d_sj.data_ptr(), n, d_ids.data_ptr(), d_recs.data_ptr(), len(recs), d_ent.data_ptr(), len(entries), bits,
        status.data_ptr(), stream()))
    torch.cuda.synchronize()
    host = coef.cpu().numpy()
    keep = np.ones(host.size, bool)
    for k, f in enumerate(jobs):
        keep[at[k]:at[k] + f.count] = False
    assert (host[keep] == 0x5A5A).all(), "coefficient guard overwritten"
    return status.cpu().numpy(), [host[at[k]:at[k] + f.count] for k, f in enumerate(jobs)]


# --------------------------------------------------------------------------- 1. coefficients
@pytest.mark.parametrize("n", [1, 2, 257])
@pytest.mark.parametrize("bits", [32, 128, 1024])
def test_coefficients_equal_the_host_decoder(bits, n):
    names = list(GOOD)
    table = [_frame(k) for k in names]
    recs, entries = _tables(table, bits)
    # n = 1: the training-sized frame (more subsequences than workers at every granularity); otherwise every case in turn
    ids = [names.index("c420_340x256_q75")] if n == 1 else [(7 * k + 3) % len(names) for k in range(n)]
    status, got = _indexed([table[i] for i in ids], ids, recs, entries, bits)
    assert not status.any(), [(names[i], s) for i, s in zip(ids, status) if s]
    for i, g in zip(ids, got):
        assert np.array_equal(g, table[i].want), (names[i], bits)


# --------------------------------------------------------------------------- 2. pixels
@pytest.fixture(scope="module", params=[("device", 32), ("device", 1024), ("host", 128)], ids=lambda p: "%s-%d" % p)
def stores(request):
    tier, bits = request.param
    plain = jpegstore.FrameStore(DEV, threads=2, tier=tier)
    indexed = jpegstore.FrameStore(DEV, threads=2, tier=tier, index_bits=bits)
    assert plain.add(FILES) == indexed.add(FILES) == range(len(FILES))
    assert indexed.index_bits == bits and indexed.tier == tier and plain.index_bits is None
    return plain, indexed


def test_pixels_equal_a_store_without_an_index_the_host_path_and_pillow(stores):
    plain, indexed = stores
    want = _want()
    for i, k in enumerate(NAMES):
        (got,) = indexed.decode([i])
        assert torch.equal(got, want[k]) and torch.equal(got, plain.decode([i])[0]), (k, indexed.index_bits)
        if k in GOLD:
            assert torch.equal(got, _t(GOLD[k])), k
    ids = [(5 * k + 1) % len(FILES) for k in range(40)]
    for a, b, i in zip(indexed.decode(ids), plain.decode(ids), ids):
        assert torch.equal(a, b) and torch.equal(a, want[NAMES[i]]), NAMES[i]
    assert not indexed.last_batch.status.any() and int(indexed.last_batch.build_status) == 0
    assert indexed.bytes_index() > 0 and indexed.bytes_resident() == plain.bytes_resident() + indexed.bytes_index()
    assert (indexed.bytes_pinned() > 0) == (indexed.tier == "host")


# --------------------------------------------------------------------------- 3. a damaged index
def test_a_damaged_index_is_reported_for_its_frame_alone_inside_the_guards():
    """Every case is run through the CPU twin first (the same code, serially, inside guards of its own) and reaches the
    GPU only with the status the twin gave: nothing here is meant to fault."""
    bits = 128
    jobs = [_frame(k) for k in jc.MUTATED]
    recs, entries = _tables(jobs, bits)
    lo, n1 = int(recs["first_entry"][1]), int(recs["nentries"][1])
    rng = np.random.default_rng(88)
    cases = []
    for _ in range(6):                                       # a handful of flipped entries of the middle frame
        bad = entries.copy()
        bad[int(rng.integers(lo, lo + n1)), int(rng.integers(0, 2))] ^= np.uint32(1 << int(rng.integers(0, 32)))
        cases.append((recs, bad, [0, 1, 2], [0, EINDEX, 0]))
    bad = entries.copy()
    bad[lo] = (0, 1)                                         # entry 0 of a segment that is not the start state
    cases.append((recs, bad, [0, 1, 2], [0, EINDEX, 0]))
    wrong = recs.copy()
    wrong["nentries"][1] += 1                                # one wrong record
    cases.append((wrong, entries, [0, 1, 2], [0, EINVAL, 0]))
    wrong = recs.copy()
    wrong["first_entry"][1] = len(entries) - n1 + 1
    cases.append((wrong, entries, [0, 1, 2], [0, EINVAL, 0]))
    cases.append((recs, entries, [0, -1, 2], [0, EINVAL, 0]))
    cases.append((recs, entries, [0, 3, 2], [0, EINVAL, 0]))
    for r, e, ids, want in cases:
        status, _ = _decode(jobs, ids, r, e, bits)            # the CPU twin, guards checked
        assert status.tolist() == want
        status, got = _indexed(jobs, ids, r, e, bits)
        assert status.tolist() == want
        for k in (0, 2):
            assert np.array_equal(got[k], jobs[k].want)


def test_a_store_reports_an_index_that_is_not_its_scans():
    from x3dhip._lib import X3DHipError
    store = jpegstore.FrameStore(DEV, threads=2, index_bits=128)
    store.add(FILES)
    i = NAMES.index("c420_40x24_blocks1")
    e = int(store._index_recs.host["first_entry"][i]) + 1
    word = store._entries.host[e:e + 1].copy()
    word ^= np.uint64(1 << 3)
    # the CPU twin first, on the store's own tables with this change
    n, changed = len(store), store._entries.host[:store._entries.n].copy()
    changed[e] = word[0]
    jobs = [_frame(NAMES[k]) for k in (0, i, 2)]
    status, _ = _decode(jobs, [0, i, 2], store._index_recs.host[:n].copy(), changed.view("<u4").reshape(-1, 2), 128)
    assert status.tolist() == [0, EINDEX, 0]
    store.memory.write(store._entries.dev, 8 * e, word.view(np.uint8))
    with pytest.raises(X3DHipError, match="JPEG frame 1 of the batch.*sync index"):
        store.decode([0, i, 2])
    assert store.last_batch.status.cpu().tolist() == [0, EINDEX, 0]
    want = _want()
    outs = store.decode([0, i, 2], check=False)
    assert torch.equal(outs[0], want[NAMES[0]]) and torch.equal(outs[2], want[NAMES[2]])


# --------------------------------------------------------------------------- 4. capture, growth
@pytest.mark.parametrize("tier", ["device", "host"])
def test_a_captured_plan_of_an_indexed_store_replays_on_other_ids(tier):
    want = _want()
    store = jpegstore.FrameStore(DEV, tier=tier, index_bits=128)
    store.add(FILES)
    vid = [NAMES.index("vid_%02d" % t) for t in range(12)]
    H, W, _ = want["vid_00"].shape
    b = store.plan(5, W, H)
    assert b.index_bits == 128
    first = vid[:5]
    b.ids.copy_(_t(np.array(first, np.int32)))
    b.launch()
    torch.cuda.synchronize()
    assert not b.status.any() and torch.equal(b.dst, torch.stack([want[NAMES[i]] for i in first]))
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
        for k, i in enumerate(pick):
            assert torch.equal(b.dst[k], want[NAMES[i]]), (pick, k)
    # an id outside the store as the plan knew it: refused for that request alone
    b.ids.copy_(_t(np.array([vid[1], len(FILES), vid[2], -1, vid[3]], np.int32)))
    b.dst.fill_(0xA5)
    graph.replay()
    torch.cuda.synchronize()
    assert b.status.cpu().tolist() == [0, EINVAL, 0, EINVAL, 0]
    assert torch.equal(b.dst[2], want["vid_02"]) and bool((b.dst[1] == 0xA5).all()) and bool((b.dst[3] == 0xA5).all())


def test_the_index_arena_grows_and_keeps_decoding_what_it_held():
    want = _want()
    store = jpegstore.FrameStore(DEV, threads=2, index_bits=32, chunk_bytes=1 << 16)
    store.add(FILES[:4])
    first = store._entries.dev
    held = store.plan(2, int(store.width[1]), int(store.height[1]))
    held.ids.copy_(_t(np.array([1, 1], np.int32)))
    for lo in range(4, len(FILES), 7):
        store.add(FILES[lo:lo + 7])
    more = store.add([FILES[NAMES.index("vid_03")]] * 1500)  # the record tables grow past their first capacity
    assert store._entries.dev is not first and store._entries.n > 1 << 14 and len(store) > 1024
    assert store.bytes_index() >= 8 * store._entries.n + 16 * len(store)
    ids = list(range(len(FILES))) + [more[0], more[-1]]
    for i, o in zip(ids, store.decode(ids)):
        assert torch.equal(o, want[NAMES[i] if i < len(FILES) else "vid_03"]), i
    held.launch()                                           # the batch planned before: on the tables it was given
    torch.cuda.synchronize()
    assert not held.status.any() and torch.equal(held.dst[0], want[NAMES[1]]) and torch.equal(held.dst[1], want[NAMES[1]])


# --------------------------------------------------------------------------- 5. packs
@pytest.mark.parametrize("src,dst", [("device", "host"), ("host", "device")])
def test_a_pack_and_its_sidecar_go_from_one_tier_into_the_other(tmp_path, src, dst):
    want = _want()
    store = jpegstore.FrameStore(DEV, threads=2, tier=src, index_bits=256, chunk_bytes=1 << 16)
    store.add(FILES)
    path = str(tmp_path / "frames.pack")
    store.save(path, {"from": src})
    got, meta, id_map = jpegstore.FrameStore.load(path, DEV, tier=dst, chunk_bytes=1 << 17)
    assert meta == {"from": src} and got.tier == dst and got.index_bits == 256 and len(got) == len(FILES)
    assert np.array_equal(got.nentries, store.nentries)
    assert got._entries.host[:got._entries.n].tobytes() == store._entries.host[:store._entries.n].tobytes()
    for i, o in enumerate(got.decode(list(range(len(FILES))))):
        assert torch.equal(o, want[NAMES[i]]), NAMES[i]
    part, _, id_map = jpegstore.FrameStore.load(path, DEV, tier=dst, ranges=[range(20, 24), range(2, 5)])
    assert id_map == [range(0, 4), range(4, 7)] and part.index_bits == 256
    for i, o in zip([20, 21, 22, 23, 2, 3, 4], part.decode(list(range(7)))):
        assert torch.equal(o, want[NAMES[i]]), NAMES[i]
    built, _, _ = jpegstore.FrameStore.load(path, DEV, tier=dst, index=64)
    assert built.index_bits == 64 and torch.equal(built.decode([7])[0], want[NAMES[7]])
    assert jpegstore.FrameStore.load(path, DEV, tier=dst, index=False)[0].index_bits is None


# --------------------------------------------------------------------------- 6. datasets and the script
KW = dict(sample_duration=10, gamma_tau=2, crop_size=32, x3d_version="M")


@pytest.mark.parametrize("tier", ["device", "host"])
def test_stored_kinetics_batches_equal_with_and_without_the_index(tmp_path, monkeypatch, tier):
    from tools import pack_frames
    monkeypatch.setattr(frames, "MIN_FRAMES", tr.MIN_FRAMES)
    root, anno, labels = tr.write_tree(tmp_path, "train")
    pack = str(tmp_path / "train.pack")
    pack_frames.pack(root, anno, labels, "train", pack, threads=2, index_bits=512)
    mk = dict(tier=tier, device=DEV, chunk_bytes=64 << 10, **KW)
    a = frames.StoredKinetics.from_annotation(root, anno, labels, "train", threads=2, rng=random.Random(99), **mk)
    b = frames.StoredKinetics.from_annotation(root, anno, labels, "train", threads=2, rng=random.Random(99), index_bits=128, **mk)
    c = frames.StoredKinetics.from_pack(pack, rng=random.Random(99), **mk)            # the sidecar, without a flag
    d = frames.StoredKinetics.from_pack(pack, rng=random.Random(99), index_bits=64, **mk)
    assert [x.store.index_bits for x in (a, b, c, d)] == [None, 128, 512, 64]
    for picks, iteration, long_state in (([0, 1, 2, 3], 0, 3), ([3, 3, 0], 1, 3), ([2, 0, 1], 1, 0)):
        ca, ya, la, sa = a.batch(picks, iteration, long_state)
        for other in (b, c, d):
            co, yo, lo, so = other.batch(picks, iteration, long_state)
            assert torch.equal(ca, co) and torch.equal(ya, yo) and la == lo and sa == so, other.store.index_bits
    va, ya = a.val_batch([0, 1, 2, 3], crops=3)
    for other in (b, c, d):
        vo, yo = other.val_batch([0, 1, 2, 3], crops=3)
        assert torch.equal(va, vo) and torch.equal(ya, yo)


def test_the_script_trains_and_validates_the_same_with_and_without_the_index(folders, tmp_path, monkeypatch, capsys):  # noqa: F811
    import train_x3d_charades
    anno = str(tmp_path / "charades.json")
    with open(anno, "w") as f:
        json.dump(_anno(["training", "training", "testing"]), f)
    printed, seen = {}, []
    real = frames.charades_videos
    monkeypatch.setattr(frames, "charades_videos", lambda *a, **kw: seen.append(real(*a, **kw)) or seen[-1])
    for label, extra in (("plain", []), ("indexed", ["--index-bits", "256"]), ("default", ["--index-bits"])):
        monkeypatch.setattr(sys, "argv", ["train_x3d_charades.py", "--anno", anno, "--frames-root", folders, "--epochs", "2",
                                          "--batch", "2", "--size", "64", "--no-graph", "--save-every", "0",
                                          "--save", str(tmp_path / "ck_"), "--resident", "compressed"] + extra)
        torch.manual_seed(5)
        capsys.readouterr()
        train_x3d_charades.main(train_x3d_charades.run, str(tmp_path / "ck_"))
        printed[label] = [ln for ln in capsys.readouterr().out.splitlines() if "Loss" in ln]
    lines = printed["plain"]
    assert len(lines) == 3 and all(re.search(r"mAP: ", ln) for ln in lines) and " val " in lines[2]
    assert printed["indexed"] == lines and printed["default"] == lines
    assert [next(iter(v.values())).store.index_bits for v in seen] == [None, 256, _jpeglib.INDEX_BITS_DEFAULT]
