"""The host tier and the pack files of the frame store on the GPU (x3djpeg_stage, x3djpeg_pinned_alloc, x3dhip.jpegstore):
the tables and the staged bytes the two stage kernels give equal the CPU twin's, across the plan kernel's passes, with
nothing written past the total; pixels of a host-tier store equal the device tier's, JpegDecoder(entropy="host") and
Pillow's goldens; refused requests (only lists the sanitised CPU run of tests/test_jpeg_tier_host.py has been through)
fail alone and leave their destination untouched; a captured plan replays on other frames; packs saved from one tier load
into the other; frames.StoredKinetics gives FolderKinetics' batches bit for bit from either tier, filled from folders or
from a pack, the training script prints the same losses whichever way its frames are resident, and the store scoring script
gives the files script's figures.  Pinned allocations
stay below 16 MB."""
import random

import numpy as np
import pytest
import torch

import frames
from tests import jpeg_entropy_cases as jc
from tests import jpeg_ref as jr
from tests import jpegstore_ref as sr
from tests import jpegtier_ref as tr
from tests.test_jpeg_store_gpu import LENGTHS, _anno, folders          # noqa: F401  (the Charades frame folders, a fixture)
from x3dhip import _jpeglib, jpegops, jpegstore
from x3dhip._jpeglib import STORE_REC_DT
from x3dhip._lib import X3DHipError, stream

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NAMES, FILES = sr.good_files()
GOLD = {k: v[1] for k, v in list(jr.load_cases().items()) + list(jc.load_entropy_cases().items()) if v[1] is not None}
GUARD = 64
_WANT = {}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _want():
    """JpegDecoder(entropy='host') on every good case, once, checked against Pillow's goldens: {name: uint8 [H, W, 3]}."""
    if not _WANT:
        outs = jpegops.JpegDecoder(DEV, threads=4).decode(FILES)
        _WANT.update(zip(NAMES, outs))
        assert any(k in _WANT for k in GOLD)
        for k, g in GOLD.items():
            if k in _WANT:
                assert torch.equal(_WANT[k], _t(g)), k
    return _WANT


def _host_store(chunk_bytes=64 << 10, **kw):
    store = jpegstore.FrameStore(DEV, tier="host", chunk_bytes=chunk_bytes, **kw)
    store.add(FILES)
    return store


def _aligned_recs(store):
    n = len(store)
    keep = sr.aligned(n * STORE_REC_DT.itemsize)
    keep[1][:] = store._recs.host[:n].view(np.uint8).reshape(-1)
    return keep, keep[1].view(STORE_REC_DT)


def _arena_reader(store):
    """read(device-visible address, nbytes) over the pinned chunks of a host-tier store, through their host views."""
    spans = [(c[0].dev, c[0].view) for c in store._chunks]

    def read(addr, nbytes):
        for base, v in spans:
            if base <= addr and addr + nbytes <= base + v.size:
                return v[addr - base:addr - base + nbytes]
        raise AssertionError("address outside the store's chunks")
    return read


def _stage(store, ids, cap, max_frame, room):
    """x3djpeg_stage alone on the store's device record table, every output between guards of 0x3C.  Returns numpy
    (staged recs, staged ids, offsets, status, staging, staging address); asserts the guards."""
    n = len(ids)
    sizes = [n * STORE_REC_DT.itemsize, 4 * n, 8 * (n + 1), 4, max(room, 16)]
    at, total = [], GUARD
    for s in sizes:
        at.append(total)
        total += (s + 15) // 16 * 16 + GUARD
    buf = torch.full((total,), 0x3C, dtype=torch.uint8, device=DEV)
    idt = _t(np.asarray(ids, np.int32))
    base = buf.data_ptr()
    assert base % 16 == 0
    _jpeglib.check(_jpeglib.lib().x3djpeg_stage(store.memory.ptr(store._recs.dev), len(store), idt.data_ptr(), n, max_frame,
                                                base + at[4], cap, base + at[0], base + at[1], base + at[2], base + at[3],
                                                stream()))
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    out, covered = [], np.zeros(total, bool)
    for a, s in zip(at, sizes):
        out.append(host[a:a + s])
        covered[a:a + s] = True
    assert (host[~covered] == 0x3C).all(), "guard overwritten"
    return (out[0].view(STORE_REC_DT), out[1].view(np.int32), out[2].view(np.int64), int(out[3].view(np.int32)[0]), out[4],
            base + at[4])


def _relative(recs, base):
    """Staged records with their addresses relative to the staging buffer (0 stays 0)."""
    r = recs.copy()
    for f in ("scan", "segs"):
        r[f] = np.where(recs[f] != 0, recs[f] - np.uint64(base), 0)
    return r


# --------------------------------------------------------------------------- 1. stage tables and bytes
@pytest.fixture(scope="module", params=[64 << 10, 16 << 10])
def host_store(request):
    store = _host_store(request.param, sub_bits=128)
    assert store.n_chunks >= 3 and store.bytes_pinned() <= 16 << 20
    if request.param == 16 << 10:                           # a frame larger than a chunk has a chunk of its own
        assert any(c[1] > request.param for c in store._chunks)
    return store


@pytest.mark.parametrize("n", tr.NS)
def test_stage_tables_and_bytes_equal_the_cpu_twin(host_store, n):
    store = host_store
    ids = tr.lists(len(store))["n_%d" % n]
    keep, recs = _aligned_recs(store)
    size = tr.frame_bytes(recs["scan_bytes"], recs["nseg"])
    total, max_frame = int(size[ids].sum()), int(size.max())
    assert total <= 16 << 20
    got = _stage(store, ids, total, max_frame, total + 4096)
    # the twin cannot follow device-visible addresses: it runs on host copies of the same frames
    T = sr.Tables(FILES)
    T.recs["header"] = recs["header"]                       # the store shares equal headers; Tables has one per frame
    twin = tr.twin(T.recs, ids, total, max_frame, room=total + 4096)
    assert got[3] == twin[3] == 0
    assert torch.equal(torch.from_numpy(got[1].copy()), torch.from_numpy(twin[1].copy()))
    assert torch.equal(torch.from_numpy(got[2].copy()), torch.from_numpy(twin[2].copy()))
    a, b = _relative(got[0], got[5]), _relative(twin[0], twin[4].ctypes.data)
    assert a.tobytes() == b.tobytes()
    want = tr.restate(recs, ids, total, max_frame, staging_base=got[5])
    assert got[0].tobytes() == want[0].tobytes() and got[2].tobytes() == want[2].tobytes()
    # staged bytes: the source's, tails zero, as the twin's; nothing at or after the total
    assert torch.equal(torch.from_numpy(got[4][:total].copy()), torch.from_numpy(twin[4][:total].copy()))
    read = _arena_reader(store)
    for k in sorted(set(range(0, n, max(1, n // 40))) | {n - 1}):
        w = tr.source_bytes(read, recs, ids[k])
        o = int(got[2][k])
        assert got[4][o:o + w.size].tobytes() == w.tobytes(), k
    assert (got[4][total:] == 0x3C).all()


# --------------------------------------------------------------------------- 2. pixels
def test_host_tier_pixels_equal_the_device_tier_the_host_path_and_pillow(host_store):
    want = _want()
    dev = jpegstore.FrameStore(DEV, sub_bits=128)
    dev.add(FILES)
    order = sr.served_lists(len(FILES))["scrambled"]
    a, b = host_store.decode(order), dev.decode(order)      # every size and subsampling in one mixed call
    for k, i in enumerate(order):
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], want[NAMES[i]]), NAMES[i]
        if NAMES[i] in GOLD:
            assert torch.equal(a[k], _t(GOLD[NAMES[i]])), NAMES[i]
    assert len({tuple(x.shape) for x in a}) >= 5
    vid = [NAMES.index("vid_%02d" % t) for t in (3, 0, 7, 3)]
    H, W, _ = want["vid_00"].shape
    dst = torch.full((4, H, W, 3), 0xA5, dtype=torch.uint8, device=DEV)
    assert host_store.decode_into(vid, dst) is dst
    assert torch.equal(dst, torch.stack([want[NAMES[i]] for i in vid]))
    assert int(host_store.last_batch.stage_status) == 0 and host_store.last_batch.staged
    # what the tiers hold where
    arena = sum(c[1] for c in dev._chunks)
    assert dev.bytes_pinned() == 0 and dev.bytes_resident() == arena + dev._recs.nbytes + dev._headers.nbytes
    assert host_store.bytes_pinned() == sum(c[1] for c in host_store._chunks) >= sum(c[2] for c in host_store._chunks)
    assert host_store.bytes_resident() == host_store._recs.nbytes + host_store._headers.nbytes


# --------------------------------------------------------------------------- 3. refusals
@pytest.mark.parametrize("label", ["id_minus_1", "id_nrecs", "cap_short"])
def test_a_request_the_stage_refuses_fails_alone_and_leaves_its_destination_untouched(host_store, label):
    want = _want()
    store = host_store
    five = [NAMES.index(k) for k in sr.REFUSED_NAMES]
    ids, refused, bit = list(five), 1, _jpeglib.STAGE_BAD_ID
    if label == "id_minus_1":
        ids[1] = -1
    elif label == "id_nrecs":
        ids[3], refused = len(store), 3
    else:
        refused, bit = 4, _jpeglib.STAGE_NO_ROOM
    safe = np.array([i if 0 <= i < len(store) else five[k] for k, i in enumerate(ids)])
    m = store._mirror[safe]
    w, h = m["width"].astype(np.int64), m["height"].astype(np.int64)
    at = np.concatenate([[0], np.cumsum(3 * w * h)])
    flat = torch.full((int(at[-1]),), 0xA5, dtype=torch.uint8, device=DEV)
    table = np.zeros(5, _jpeglib.STORE_DST_DT)
    table["dst"], table["dst_stride"], table["width"], table["height"] = flat.data_ptr() + at[:-1], 3 * w, w, h
    size = tr.frame_bytes(m["scan_bytes"], m["nseg"])
    served = np.array([0 <= i < len(store) for i in ids])
    cap = int(size[served].sum()) - (1 if label == "cap_short" else 0)
    with torch.cuda.device(DEV):
        b = jpegstore.Batch(store, 5, int(m["coef_count"].sum()), int(m["ws_need"].sum()), int(m["nblocks"].max()),
                            int(w.max()), int(h.max()), _t(np.asarray(ids, np.int32)), _t(table.view(np.uint8).reshape(-1)),
                            stage_cap=cap, max_frame_bytes=int(size.max()))
        b.staging.fill_(0x3C)
        b.launch()
    torch.cuda.synchronize()
    assert int(b.stage_status) == bit and int(b.build_status) == _jpeglib.STORE_BAD_ID
    assert b.staged_ids.cpu().tolist() == [-1 if k == refused else k for k in range(5)]
    assert b.status.cpu().tolist() == [_jpeglib.EINVAL if k == refused else 0 for k in range(5)]
    total = int(b.offsets[-1])
    assert total == int(size[served].sum()) - (int(size[4]) if label == "cap_short" else 0)
    assert bool((b.staging[total:] == 0x3C).all())          # nothing of the refused request's bytes
    for k in range(5):
        got = flat[int(at[k]):int(at[k + 1])]
        if k == refused:
            assert bool((got == 0xA5).all()), label
        else:
            assert torch.equal(got.view(int(h[k]), int(w[k]), 3), want[NAMES[ids[k]]]), (label, k)
    with pytest.raises(X3DHipError, match="the stage refused the request"):
        b.raise_for_status()


# --------------------------------------------------------------------------- 4. graph capture
def test_a_captured_host_tier_plan_replays_on_other_frames(host_store):
    want = _want()
    store = host_store
    vid = [NAMES.index("vid_%02d" % t) for t in range(12)]
    H, W, _ = want["vid_00"].shape
    b = store.plan(8, W, H)
    sel = np.flatnonzero((store.width == W) & (store.height == H))
    assert b.staged and b.stage_cap == 8 * int(tr.frame_bytes(store.scan_bytes[sel], store.nseg[sel]).max())
    first = vid[:8]
    b.ids.copy_(_t(np.array(first, np.int32)))
    b.launch()
    torch.cuda.synchronize()
    assert torch.equal(b.dst, torch.stack([want[NAMES[i]] for i in first])) and not b.status.any()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):             # one stream, no parallel branches
            b.launch()
    torch.cuda.current_stream().wait_stream(s)
    for pick in ([vid[11], vid[6], vid[6], vid[9], vid[5], vid[0], vid[10], vid[2]], first[::-1]):
        b.ids.copy_(_t(np.array(pick, np.int32)))
        b.dst.fill_(0xA5)
        b.staging.fill_(0x3C)
        b.status.fill_(77)
        graph.replay()
        torch.cuda.synchronize()
        assert not b.status.any() and int(b.build_status) == 0 and int(b.stage_status) == 0
        assert torch.equal(b.dst, torch.stack([want[NAMES[i]] for i in pick])), pick
    # an id outside the store, written into the captured batch: refused on the device, alone
    b.ids.copy_(_t(np.array(first[:3] + [len(store)] + first[4:], np.int32)))
    b.dst.fill_(0xA5)
    graph.replay()
    torch.cuda.synchronize()
    assert int(b.stage_status) == _jpeglib.STAGE_BAD_ID and bool((b.dst[3] == 0xA5).all())
    assert torch.equal(b.dst[4], want[NAMES[first[4]]]) and torch.equal(b.dst[2], want[NAMES[first[2]]])


# --------------------------------------------------------------------------- 5. packs on the GPU
@pytest.mark.parametrize("src,dst", [("device", "host"), ("host", "device")])
def test_a_pack_saved_from_one_tier_loads_into_the_other(tmp_path, src, dst):
    want = _want()
    a = jpegstore.FrameStore(DEV, tier=src, chunk_bytes=64 << 10)
    a.add(FILES)
    path = str(tmp_path / "frames.pack")
    a.save(path, {"from": src})
    b, meta, id_map = jpegstore.FrameStore.load(path, DEV, tier=dst, chunk_bytes=32 << 10)
    assert meta == {"from": src} and id_map == [range(0, len(FILES))] and b.tier == dst and b.n_chunks > a.n_chunks
    order = sr.served_lists(len(FILES))["scrambled"]
    for k, (x, y) in enumerate(zip(a.decode(order), b.decode(order))):
        assert torch.equal(x, y) and torch.equal(x, want[NAMES[order[k]]]), NAMES[order[k]]
    arena = sum(c[1] for c in b._chunks)
    tables = b._recs.nbytes + b._headers.nbytes
    assert (b.bytes_resident(), b.bytes_pinned()) == ((tables, arena) if dst == "host" else (tables + arena, 0))
    assert arena <= 16 << 20
    # a shard: two ranges of the saved ids, in another order
    n = len(FILES)
    c, _, id_map = jpegstore.FrameStore.load(path, DEV, tier=dst, ranges=[range(n - 5, n), range(2, 6)])
    assert id_map == [range(0, 5), range(5, 9)]
    picked = list(range(n - 5, n)) + list(range(2, 6))
    for k, x in enumerate(c.decode(range(9))):
        assert torch.equal(x, want[NAMES[picked[k]]]), k


def test_a_pinned_allocation_that_fails_leaves_the_store_as_it_was(monkeypatch):
    store = jpegstore.FrameStore(DEV, tier="host", chunk_bytes=64 << 10)
    store.add(FILES[:4])
    before = (len(store), store.n_chunks, store.n_headers, store.bytes_pinned(), store._recs.host[:4].tobytes())

    def refuse(self, nbytes):
        raise X3DHipError("libx3djpeg: error -2: x3djpeg_pinned_alloc: %d bytes of pinned host memory: out of memory" % nbytes)
    monkeypatch.setattr(jpegstore.PinnedMemory, "alloc", refuse)
    with pytest.raises(X3DHipError, match="bytes of pinned host memory"):
        store.add(FILES)                                    # needs further chunks
    monkeypatch.undo()
    assert before == (len(store), store.n_chunks, store.n_headers, store.bytes_pinned(), store._recs.host[:4].tobytes())
    assert torch.equal(store.decode([2])[0], _want()[NAMES[2]])
    h = _jpeglib.lib()
    assert h.x3djpeg_pinned_alloc(0, None, None) == _jpeglib.EINVAL and h.x3djpeg_pinned_free(None) == _jpeglib.EINVAL


# --------------------------------------------------------------------------- 6. datasets
KW = dict(sample_duration=10, gamma_tau=2, crop_size=32, x3d_version="M")


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from tools import pack_frames
    tmp = tmp_path_factory.mktemp("kinetics_tree")
    mp = pytest.MonkeyPatch()
    mp.setattr(frames, "MIN_FRAMES", tr.MIN_FRAMES)
    root, anno, labels = tr.write_tree(tmp, "train")
    vroot, vanno, _ = tr.write_tree(tmp, "validate")
    packs = dict(train=str(tmp / "train.pack"), val=str(tmp / "val.pack"), windows=str(tmp / "windows.pack"))
    pack_frames.pack(root, anno, labels, "train", packs["train"], threads=2)
    pack_frames.pack(vroot, vanno, labels, "validate", packs["val"], threads=2)
    pack_frames.pack(vroot, vanno, labels, "validate", packs["windows"], val_windows=3, sample_duration=10, gamma_tau=2, threads=2)
    # for the training script, whose validation windows span 80 frames: two videos of 82
    lroot, lanno, _ = tr.write_tree(tmp, "validate", [t[:2] + (82,) + t[3:] for t in tr.TREE[:2]], "validate_long")
    packs["val_long"] = str(tmp / "val_long.pack")
    pack_frames.pack(lroot, lanno, labels, "validate", packs["val_long"], val_windows=3, threads=2)
    yield dict(train=(root, anno, labels), val=(vroot, vanno, labels), val_long=(lroot, lanno, labels), packs=packs)
    mp.undo()


@pytest.mark.parametrize("tier", ["device", "host"])
@pytest.mark.parametrize("source", ["annotation", "pack"])
def test_stored_kinetics_batches_equal_folder_kinetics(tree, source, tier):
    root, anno, labels = tree["train"]
    a = frames.FolderKinetics.from_annotation(root, anno, labels, "train", rng=random.Random(99), device=DEV, threads=2, **KW)
    if source == "annotation":
        b = frames.StoredKinetics.from_annotation(root, anno, labels, "train", tier=tier, device=DEV, threads=2,
                                                  chunk_bytes=64 << 10, rng=random.Random(99), **KW)
    else:
        b = frames.StoredKinetics.from_pack(tree["packs"]["train"], DEV, tier=tier, chunk_bytes=64 << 10,
                                            rng=random.Random(99), **KW)
    assert len(a) == len(b) == 4 and list(a.labels) == list(b.labels) == [1, 3, 1, 4] and b.store.tier == tier
    assert [v.shape for v in a.videos] == [v.shape for v in b.videos] and b.store.bytes_pinned() <= 16 << 20
    assert (b.store.bytes_pinned() > 0) == (tier == "host")
    for picks, iteration, long_state in (([0, 1, 2, 3], 0, 3), ([3, 3, 0], 1, 3), ([1, 2], 2, 2), ([2, 0, 1], 1, 0)):
        ca, ya, la, sa = a.batch(picks, iteration, long_state)      # two frame sizes in one batch
        cb, yb, lb, sb = b.batch(picks, iteration, long_state)
        assert ca.shape == cb.shape and torch.equal(ca, cb), (picks, iteration, long_state)
        assert torch.equal(ya, yb) and la == lb and sa == sb
    va, ya = a.val_batch([0, 1, 2, 3], crops=3)
    vb, yb = b.val_batch([0, 1, 2, 3], crops=3)
    assert tuple(va.shape) == (4, 3, 3, 5, 32, 32) and torch.equal(va, vb) and torch.equal(ya, yb)
    if source == "pack":                                    # a rank's shard: videos 1 and 3
        c = frames.StoredKinetics.from_pack(tree["packs"]["train"], DEV, tier=tier, rank=1, world=2, **KW)
        assert len(c) == 2 and list(c.labels) == [3, 4]
        vc, yc = c.val_batch([0, 1], crops=3)
        assert torch.equal(vc, va[[1, 3]]) and yc.tolist() == [3, 4]


@pytest.mark.parametrize("tier", ["device", "host"])
def test_a_validation_window_pack_serves_kinetics_batches_and_refuses_other_frames(tree, tier):
    import kinetics
    vroot, vanno, labels = tree["val"]
    want = kinetics.Kinetics(vroot, vanno, labels, "validate", sample_duration=10, gamma_tau=2, crops=3, crop_size=32,
                             device=DEV, threads=2)
    ds = frames.StoredKinetics.from_pack(tree["packs"]["windows"], DEV, tier=tier, sample_duration=10, gamma_tau=2, crop_size=32)
    assert len(ds.store) < sum(t[2] for t in tr.TREE) // 2 and all(isinstance(v, frames.WindowedVideo) for v in ds.videos)
    got = kinetics.Kinetics.from_dataset(ds, crops=3)
    for (ca, ya), (cb, yb) in zip(want.batches(3), got.batches(3)):
        assert torch.equal(ca, cb) and torch.equal(ya, yb)
    assert len(list(got.batches(3))) == 2
    # each rank its own shard of the pack
    mine = frames.StoredKinetics.from_pack(tree["packs"]["windows"], DEV, tier=tier, rank=1, world=2, sample_duration=10,
                                           gamma_tau=2, crop_size=32)
    shard = kinetics.Kinetics.from_dataset(mine, crops=3, sharded=(1, 2))
    (ca, ya), = list(want.batches(4, rank=1, world=2))
    (cb, yb), = list(shard.batches(4, rank=1, world=2))
    assert torch.equal(ca, cb) and torch.equal(ya, yb)
    with pytest.raises(ValueError, match="shard of rank 1 of 2"):
        shard.shard(0, 2)
    # other windows draw frames the pack does not hold
    assert set(frames.val_window_frames(40, 2, 10, 4)) - set(frames.val_window_frames(40, 2, 10, 3)) == {10, 12, 24, 26}
    with pytest.raises(ValueError, match=r"frame 10 of video class_b/vidB is not in the pack \(it holds 15 of its 40 frames\)"):
        ds.val_batch([0, 1], crops=4)
    with pytest.raises(ValueError, match=r"frame 39 of video class_b/vidB is not in the pack"):
        ds.videos[1].frames([0, 39])
    assert tuple(ds.videos[1].frames([0, 36]).shape) == (2, 64, 80, 3)


@pytest.fixture(scope="module")
def kinds(tree):
    """The four training videos of the tree three ways: (labels, decoded tensors, FolderVideos on one decoder,
    StoredVideos in one store)."""
    entries = frames.list_annotation(*tree["train"], "train")
    dec = jpegops.JpegDecoder(DEV, threads=2)
    store = jpegstore.FrameStore(DEV, threads=2, chunk_bytes=64 << 10)
    decoded = [frames.decode_folder(f, DEV, decoder=dec) for f, _ in entries]
    folder = [frames.FolderVideo(f, dec) for f, _ in entries]
    stored = [frames.StoredVideo(store, frames.add_folder(store, f)) for f, _ in entries]
    assert [v.shape[1:3] for v in decoded] == [(t[4], t[3]) for t in tr.TREE]
    return [label for _, label in entries], decoded, folder, stored


@pytest.mark.parametrize("mix", ["sfdf", "dsfs", "fdsd"])
def test_one_batch_across_decoded_folder_and_stored_videos(kinds, mix):
    """A plain DeviceVideoKinetics whose videos are of all three kinds (d: decoded tensor, f: FolderVideo, s: StoredVideo;
    videos 0 and 3 are 64 x 80, 1 and 2 are 80 x 64, so the letters put both sizes into one source or one size into two
    sources) gives the all-decoded dataset's batches bit for bit: the groups of gather_frames and the slots after them."""
    from kinetics_multigrid import DeviceVideoKinetics
    labels, decoded, folder, stored = kinds
    of = dict(d=decoded, f=folder, s=stored)
    videos = [of[k][i] for i, k in enumerate(mix)]
    assert {type(v) for v in videos} == {torch.Tensor, frames.FolderVideo, frames.StoredVideo}
    a = DeviceVideoKinetics(decoded, labels, rng=random.Random(5), **KW)
    b = DeviceVideoKinetics(videos, labels, rng=random.Random(5), **KW)
    for picks, iteration, long_state in (([0, 1, 2, 3], 0, 3), ([3, 1, 1, 0, 2], 1, 2)):
        ca, ya, la, sa = a.batch(picks, iteration, long_state)
        cb, yb, lb, sb = b.batch(picks, iteration, long_state)
        assert ca.shape == cb.shape and torch.equal(ca, cb), (picks, iteration, long_state)
        assert torch.equal(ya, yb) and la == lb and sa == sb
    va, ya = a.val_batch([0, 1, 2, 3], crops=3)
    vb, yb = b.val_batch([0, 1, 2, 3], crops=3)
    assert tuple(va.shape) == (4, 3, 3, 5, 32, 32) and torch.equal(va, vb) and torch.equal(ya, yb)
    assert float(va.abs().sum()) > 0 and not torch.equal(va[0], va[3])
    assert all(videos[i] is v for i, v in enumerate(b.videos))             # the dataset's videos stay what they were


def test_gather_frames_gives_every_sample_its_own_frames(kinds):
    """Interleaved samples [A, B, A, B] of two sources of one frame size (a store holding videos 1 and 2, a decoder reading
    their folders): two decode_into calls, and every sample gets exactly its frame_idx, in its order, repeats included."""
    _, decoded, folder, stored = kinds
    picks = [(stored[1], [3, 0, 7, 7]), (folder[1], [5, 39, 1]), (stored[2], [30]), (folder[2], [10, 9, 0, 2, 2]),
             (decoded[1], [4, 6])]
    assert len({v.shape[1:] for v, _ in picks}) == 1
    want = [v.frames(idx) if frames.is_lazy(v) else v for v, idx in picks]
    calls = []
    for src in (stored[1].source, folder[1].source):
        real = src.decode_into
        src.decode_into = lambda requests, dst, real=real: calls.append(len(requests)) or real(requests, dst)
    samples = [dict(frames=v, frame_idx=list(idx), tag=k) for k, (v, idx) in enumerate(picks)]
    try:
        frames.gather_frames(samples)
    finally:
        del stored[1].source.decode_into, folder[1].source.decode_into
    assert calls == [5, 8]                                                  # one call per source, over all its samples
    for k, (s, (v, idx)) in enumerate(zip(samples, picks)):
        assert s["tag"] == k and torch.equal(s["frames"], want[k]), k
        if frames.is_lazy(v):
            assert list(s["frame_idx"]) == list(range(len(idx))) and torch.equal(s["frames"], decoded[1 + (k > 1)][idx]), k
        else:
            assert s["frames"] is v and s["frame_idx"] == idx              # a decoded video passes through untouched
    with pytest.raises(ValueError, match="frame index outside the video"):
        frames.gather_frames([dict(frames=folder[1], frame_idx=[40])])
    with pytest.raises(ValueError, match="frame 40 outside the 40 frames"):
        folder[1].frames([40])
    # neither a tensor nor a lazy video: left as it is, and refused by the clip kernels' own check
    from kinetics_multigrid import DeviceVideoKinetics
    bad = type("V", (), dict(shape=tuple(decoded[0].shape), device=DEV))()
    assert not frames.is_lazy(bad) and frames.gather_frames is __import__("x3dhip.clip_input").clip_input.gather_frames
    with pytest.raises(ValueError, match="frames must be contiguous uint8 tensors"):
        DeviceVideoKinetics([bad], [0], **KW).val_batch([0], crops=3)


@pytest.mark.parametrize("task", ["class", "loc"])
def test_charades_batches_over_folder_videos_equal_those_over_decoded_ones(folders, task):    # noqa: F811
    """Charades over frames.FolderVideo (files read and decoded per batch), on the folders of test_jpeg_store_gpu's
    Charades test: batch and test_batch equal the decoded videos' bit for bit."""
    import os
    from charades import Charades
    dec = frames.charades_videos(folders, _anno(["training"] * 3), DEV, threads=2)
    decoder = jpegops.JpegDecoder(DEV, threads=2)
    lazy = {}
    for vid in LENGTHS:
        path = os.path.join(folders, vid)
        name = frames.FRAME_NAME if os.path.exists(os.path.join(path, frames.FRAME_NAME.format(1))) else vid + "-{:06d}.jpg"
        lazy[vid] = frames.FolderVideo(frames.FrameFolder(path, name), decoder)
        assert tuple(lazy[vid].shape) == tuple(dec[vid].shape) and frames.is_lazy(lazy[vid]) and not frames.is_lazy(dec[vid])
    kw = dict(task=task, frames=80, gamma_tau=2, crop_size=20, c_size=20, scales=(0.8, 0.9))
    train = [Charades(_anno(["training"] * 3), "training", v, rng=random.Random(4), **kw) for v in (dec, lazy)]
    assert len(train[0]) == len(train[1]) == 3 and train[0].data == train[1].data
    idx = [2, 0, 1, 0]
    params = [train[0].draw(i) for i in idx]
    a, b = train[0].batch(idx, params=params), train[1].batch(idx, params=params)
    assert len(a) == len(b) == (2 if task == "class" else 3) and tuple(a[0].shape) == (4, 3, 40, 20, 20)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and torch.equal(x, y)
    assert float(a[0].abs().sum()) > 0
    train[0].rng, train[1].rng = random.Random(9), random.Random(9)    # and with draws of their own
    for x, y in zip(train[0].batch([1, 2]), train[1].batch([1, 2])):
        assert torch.equal(x, y)
    test = [Charades(_anno(["testing"] * 3), "testing", v, crops=10, **kw) for v in (dec, lazy)]
    a, b = test[0].test_batch([0, 1, 2]), test[1].test_batch([0, 1, 2])
    assert len(a) == len(b) == (2 if task == "class" else 3)
    assert tuple(a[0].shape) == ((3, 10, 3, 40, 20, 20) if task == "class" else (3, 3, 50, 20, 20))
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and torch.equal(x, y)
    for x, y in zip(test[0].test_batch([1]), test[1].test_batch([1])):
        assert torch.equal(x, y)
    with pytest.raises(ValueError, match="frames must be contiguous uint8 tensors on a CUDA"):
        Charades(_anno(["training"] * 3), "training", dict(dec, AAAAA=dec["AAAAA"].cpu()), **kw)


# --------------------------------------------------------------------------- 7. the scripts
def test_the_script_prints_the_same_losses_however_the_frames_are_resident(tree, capsys):
    import train_x3d_kinetics_multigrid as tk
    root, anno, labels = tree["train"]
    vroot, vanno, _ = tree["val_long"]
    ways = {"files": (dict(), dict()),
            "hbm": (dict(resident="hbm"), dict(resident="hbm")),
            "host": (dict(resident="host"), dict(resident="host")),
            "pack": (dict(resident="host", pack=tree["packs"]["train"]), dict(resident="hbm", pack=tree["packs"]["val_long"]))}
    seen = {}
    for way, (t, v) in ways.items():
        train = t if "pack" in t else dict(t, root=root, anno=anno, labels=labels, threads=2)
        val = v if "pack" in v else dict(v, root=vroot, anno=vanno, labels=labels, threads=2)
        torch.manual_seed(7)
        steps, _ = tk.run(batch_size=2, max_steps_run=3, iterations_per_epoch=40, max_epochs=3, val_every=3, use_graph=False,
                          save_every=0, clip_size=32, log_every=1, frames_root=train, val_frames=val)
        assert steps == 3
        out = capsys.readouterr().out.splitlines()
        losses = [ln.split(" lr ")[0] for ln in out if ln.startswith(" step ")]
        vals = [ln for ln in out if ln.startswith(" val after step ")]
        assert len(losses) == 3 and len(vals) == 1 and "(2 videos)" in vals[0] and "Top5:" in vals[0], out
        seen[way] = (losses, vals)
    assert seen["hbm"] == seen["files"] and seen["host"] == seen["files"] and seen["pack"] == seen["files"]


def test_the_store_scoring_script_gives_what_the_files_script_gives(tree, tmp_path, capsys):
    import json
    import score_x3d_kinetics_store as stored
    import test_x3d_kinetics as script
    import train_x3d_kinetics_multigrid as tk
    vroot, vanno, labels = tree["val_long"]
    prefix = str(tmp_path / "ck_")
    tk.run(batch_size=2, max_steps_run=1, iterations_per_epoch=40, max_epochs=3, use_graph=False, save_every=1,
           save_model=prefix, clip_size=32, log_every=1)
    ckpt = prefix + "000001.pt"
    want = script.main(["--load", ckpt, "--frames-root", vroot, "--anno", vanno, "--labels", labels, "--batch", "2",
                        "--decode-threads", "2"])
    capsys.readouterr()
    for way in (["--resident", "hbm", "--pack", tree["packs"]["val_long"]],
                ["--resident", "host", "--frames-root", vroot, "--anno", vanno, "--labels", labels, "--decode-threads", "2"]):
        got = stored.main(["--load", ckpt, "--batch", "2"] + way)
        out = capsys.readouterr().out.splitlines()
        rec = json.loads(out[-1])
        assert any(ln.startswith(" Cls Loss: ") for ln in out) and rec["checkpoint"] == ckpt
        for k in ("videos", "top1", "top5", "cls_loss", "loss_per_video"):
            assert got[k] == want[k] == rec[k] and want["videos"] == 2, (way[1], k)
