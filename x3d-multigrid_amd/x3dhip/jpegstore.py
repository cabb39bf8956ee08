"""JPEG frames resident in HBM in compressed form, decoded by frame id: the frame store of include/x3djpeg.h.

JpegDecoder(entropy="device") does, for every frame of every batch, work that does not depend on the batch: it reads and
parses the file, strips the byte stuffing (x3djpeg_scan_prepare), builds two job structs in numpy and uploads all of it.
A FrameStore does that once per frame, in add(): the prepared scan and its segment table go into arena chunks on the
device (about the size of the file; a chunk is never moved or resized once written, so every address stays valid for the
life of the store), the part of the headers the jobs need into a header table (one entry per distinct header: the frames
of a video share theirs), and one 32-byte record per frame into a record table.  A batch is then a list of frame ids:
only the ids and the destination table are uploaded, x3djpeg_store_build_jobs builds both job tables on the device in two
launches, and the three launches of the device path (x3djpeg_entropy_decode_batch, x3djpeg_decode_batch) run on them
untouched -- bit for bit what JpegDecoder gives.  Because the job tables are built on the device from a device tensor of
ids, a whole batch (plan) can be captured in a graph and replayed on other frames by writing their ids into that tensor.

    store = FrameStore("cuda:0")
    ids = store.add(files)                       # range of frame ids; files: list of bytes
    frames = store.decode_into(ids, dst)         # dst: uint8 [n, H, W, 3]
    batch = store.plan(64, 340, 256)             # static buffers: batch.ids, batch.dst; batch.launch() is capturable

There is no fallback: a file the decoder does not take raises X3DHipError in add() and the store is left as it was.

Two tiers.  tier="device" (the default) is the above.  With tier="host" the arena chunks lie in pinned host memory the GPU
reads over the host link (PinnedMemory), for a dataset larger than HBM; the record and header tables stay on the device.
A batch of such a store owns a small staging buffer in HBM: x3djpeg_stage gathers the frames the batch draws into it (two
more launches, ids still read on the device, still capturable), and the builder and the decoders run on the staged copy.

Pack files.  store.save(path, meta) writes the whole store -- header table, per-frame fields, arena bytes, a JSON blob the
caller owns -- as one file of data, without addresses; FrameStore.load(path, device, tier=...) reads it back with bulk
reads (all of it or ranges of its frames) instead of opening, parsing and un-stuffing every JPEG file again.

Sync index.  FrameStore(..., index_bits=N) also keeps, per frame, the decoder state at the start of every N-bit
subsequence of its scan (x3djpeg_index_build, on the host threads of add()): 8 bytes per N bits of scan, always in device
memory, in both tiers.  A batch of such a store runs x3djpeg_entropy_decode_indexed in place of
x3djpeg_entropy_decode_batch: one pass over the scan instead of a speculative pass and its relaxation rounds, every
hand-over between subsequences compared with the index, so an index that is not the scan's reports X3DJPEG_EINDEX and
never wrong pixels.  save() of an indexed store writes the pack as ever and the index beside it (path + ".idx").
"""
import ctypes
import json
import os
import struct

import numpy as np
import torch

from . import _jpeglib
from ._jpeglib import (FRAME_JOB_DT, INDEX_REC_DT, INFO_DT, SCAN_JOB_DT, SCAN_PAD, SCAN_SEG_DT, STORE_DST_DT,
                       STORE_HEADER_DT, STORE_REC_DT, stage_bytes)
from ._lib import X3DHipError, stream
from .jpegops import HostStages, check_dst, check_sub_bits, fill_jobs, status_text

MIRROR_DT = np.dtype([("width", "<i4"), ("height", "<i4"), ("nblocks", "<i4"), ("scan_bytes", "<i4"), ("nseg", "<i4"),
                      ("chunk", "<i4"), ("coef_count", "<i8"), ("ws_need", "<i8"), ("nentries", "<i4")])
_REASONS = ((_jpeglib.STORE_BAD_ID, "a frame id outside the store"),
            (_jpeglib.STORE_BAD_SIZE, "a frame of another size than its destination"),
            (_jpeglib.STORE_NO_COEF, "coefficients beyond the buffer"), (_jpeglib.STORE_NO_WS, "workspace beyond the buffer"))
_STAGE_REASONS = ((_jpeglib.STAGE_BAD_ID, "a frame id outside the store"),
                  (_jpeglib.STAGE_NO_ROOM, "a frame beyond the staging buffer"))
TIERS = ("device", "host")

# A pack file, little-endian: PACK_HEAD, the header table (STORE_HEADER_DT [nheaders]), the frame table (PACK_FRAME_DT
# [nframes]), zeros up to a multiple of 16, the arena bytes (per frame its scan, padded to 16, then its segment table: what
# x3djpeg_stage_bytes counts), the JSON meta blob.  `offset` is a file offset.
PACK_MAGIC, PACK_VERSION = b"X3DJPACK", 1
PACK_HEAD = struct.Struct("<8sIIIIQQQQQ")       # magic, version, header entry bytes, frame entry bytes, sub_bits at save,
#                                                 nframes, nheaders, arena offset, arena bytes, meta bytes
PACK_FRAME_DT = np.dtype([("offset", "<u8"), ("length", "<u8"), ("scan_bytes", "<i4"), ("nseg", "<i4"), ("header", "<i4"),
                          ("width", "<i4"), ("height", "<i4"), ("nblocks", "<i4"), ("coef_count", "<i8")])

# The sidecar of a pack (path + ".idx"), little-endian: INDEX_HEAD, the entry count of every frame (uint32 [nframes]),
# zeros up to a multiple of 8, the entries of all frames in frame order (8 bytes each).
INDEX_SUFFIX, INDEX_MAGIC, INDEX_VERSION = ".idx", b"X3DJPIDX", 1
INDEX_HEAD = struct.Struct("<8sIIQQQ")          # magic, version, index_bits, nframes and arena bytes of the pack it
#                                                 belongs to, entries in all


def check_index_bits(index_bits):
    """The granularity of a sync index as an int (True: the library's default), None for no index, or ValueError."""
    if index_bits is None or index_bits is False:
        return None
    bits = _jpeglib.INDEX_BITS_DEFAULT if index_bits is True else int(index_bits)
    if bits < 32 or bits % 32 or bits > 1 << 20:
        raise ValueError("index_bits must be a multiple of 32 in 32 .. 2^20 (got %r)" % (index_bits,))
    return bits


def store_headers(infos):
    """STORE_HEADER_DT entries of parsed frames (INFO_DT array): the two job structs with the per-request fields zero."""
    h = np.zeros(len(infos), STORE_HEADER_DT)
    fill_jobs(h["frame"], infos)
    _jpeglib.fill_scan_jobs(h["scan"], infos)
    return h


class TorchMemory:
    """Where a store keeps its data: uint8 tensors on a device.  (The tests put a store into host memory through an object
    with the same three methods, to run the CPU twin of the job builder on it.)"""

    def __init__(self, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("FrameStore needs a GPU device (got %s)" % self.device)

    def alloc(self, nbytes):
        return torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)

    def write(self, buf, off, host):
        """host: contiguous numpy uint8."""
        if host.size:
            buf[off:off + host.size].copy_(torch.from_numpy(host))

    def ptr(self, buf):
        return buf.data_ptr()

    def read(self, buf, off, nbytes):
        return buf[off:off + nbytes].cpu().numpy()


class _PinnedBuffer:
    """One x3djpeg_pinned_alloc: `view` is the host's numpy view of it, `dev` the address the runtime gives the device."""

    def __init__(self, nbytes):
        host, dev = ctypes.c_void_p(), ctypes.c_void_p()
        self._host = None
        _jpeglib.check(_jpeglib.lib().x3djpeg_pinned_alloc(int(nbytes), ctypes.byref(host), ctypes.byref(dev)))
        self._host, self.dev, self.nbytes = host.value, dev.value, int(nbytes)
        self.view = np.ctypeslib.as_array((ctypes.c_uint8 * self.nbytes).from_address(self._host))

    def __del__(self):
        host, self._host = getattr(self, "_host", None), None
        if host is not None:
            self.view = None
            try:
                _jpeglib.lib().x3djpeg_pinned_free(host)
            except Exception:                               # the interpreter is shutting down: the process frees it
                pass


class PinnedMemory:
    """Where a host-tier store keeps its arena: mapped, portable pinned host memory.  The same three methods as
    TorchMemory; ptr is the device-visible address, write a plain host copy.  host_view lets load() read a file straight
    into a chunk."""

    def alloc(self, nbytes):
        return _PinnedBuffer(nbytes)

    def write(self, buf, off, host):
        buf.view[off:off + host.size] = host

    def ptr(self, buf):
        return buf.dev

    def read(self, buf, off, nbytes):
        return buf.view[off:off + nbytes]

    def host_view(self, buf):
        return buf.view


def _read(memory, buf, off, nbytes):
    """nbytes of a chunk as numpy uint8 (a memory object without read keeps numpy arrays)."""
    if hasattr(memory, "read"):
        return memory.read(buf, off, nbytes)
    return np.asarray(buf[off:off + nbytes])


class NumpyMemory:
    """The same three methods over plain host memory: a store that is only filled and saved (tools/pack_frames.py), or
    read by the CPU twins, needs no GPU."""

    def alloc(self, nbytes):
        whole = np.zeros(int(nbytes) + 64, np.uint8)
        at = -whole.ctypes.data % 64
        return whole[at:at + int(nbytes)]

    def write(self, buf, off, host):
        buf[off:off + host.size] = host

    def ptr(self, buf):
        return buf.ctypes.data

    def read(self, buf, off, nbytes):
        return buf[off:off + nbytes]

    def host_view(self, buf):
        return buf


class _Table:
    """A table on the device with its host copy, grown by doubling.  Growth writes a new buffer and leaves the old one to
    whoever still holds it (a planned batch)."""

    def __init__(self, memory, dtype, capacity):
        self.memory, self.host, self.n = memory, np.zeros(capacity, dtype), 0
        self.dev = memory.alloc(self.host.nbytes)

    def append(self, rows):
        lo, hi = self.n, self.n + len(rows)
        if hi > len(self.host):
            host = np.zeros(max(hi, 2 * len(self.host)), self.host.dtype)
            host[:lo] = self.host[:lo]
            host[lo:hi] = rows
            dev = self.memory.alloc(host.nbytes)
            self.memory.write(dev, 0, host[:hi].view(np.uint8).reshape(-1))
            self.host, self.dev = host, dev
        else:
            self.host[lo:hi] = rows
            size = self.host.dtype.itemsize
            self.memory.write(self.dev, lo * size, self.host[lo:hi].view(np.uint8).reshape(-1))
        self.n = hi

    @property
    def nbytes(self):
        return self.host.nbytes


class Batch:
    """The buffers and the five launches of one batch of `n` requests.  ids (int32 [n]) and dsts (the destination table)
    are on the device; launch() reads them there, so a captured launch() decodes whatever ids hold when it is replayed.
    status: int32 [n], per frame 0 or a negative X3DJPEG_E*; build_status: int32 [1], the OR of the X3DJPEG_STORE_* bits
    of the requests the builder refused (a refused frame reports X3DJPEG_EINVAL and its destination is not written)."""

    def __init__(self, store, n, coef_cap, ws_cap, max_blocks, max_w, max_h, ids, dsts, dst=None, stage_cap=None,
                 max_frame_bytes=0):
        mem, self.n, self.sub_bits = store.memory, int(n), store.sub_bits
        self.max_blocks, self.max_w, self.max_h = int(max_blocks), int(max_w), int(max_h)
        self.coef_cap, self.ws_cap = int(coef_cap), int(ws_cap)
        dev = store.device
        self.ids, self.dsts, self.dst = ids, dsts, dst
        self.coef = torch.empty(self.coef_cap, dtype=torch.int16, device=dev)
        self.planes = torch.empty(self.coef_cap, dtype=torch.uint8, device=dev)
        self.workspace = torch.empty(self.ws_cap, dtype=torch.uint8, device=dev)
        self.scan_jobs = torch.empty(self.n * SCAN_JOB_DT.itemsize, dtype=torch.uint8, device=dev)
        self.frame_jobs = torch.empty(self.n * FRAME_JOB_DT.itemsize, dtype=torch.uint8, device=dev)
        self.plan = torch.empty(3 * self.n + 2, dtype=torch.int64, device=dev)
        self.staged = stage_cap is not None
        self._status = torch.empty(self.n + (2 if self.staged else 1), dtype=torch.int32, device=dev)
        self.status, self.build_status = self._status[:self.n], self._status[self.n:self.n + 1]
        # the tables as they are now: a later add() may move them, and leaves these to this batch
        self._recs, self._headers = store._recs.dev, store._headers.dev
        self.nrecs, self.nheaders = store._recs.n, store._headers.n
        recs_ptr, nrecs, ids_ptr = mem.ptr(self._recs), self.nrecs, ids.data_ptr()
        self._stage_args = None
        if self.staged:
            # the host tier: the frames are gathered into `staging` first, and the builder is given the staged tables
            self._chunks = list(store._chunks)              # the arena this batch reads lives as long as the batch
            self.stage_cap, self.max_frame_bytes = int(stage_cap), int(max_frame_bytes)
            self.staging = torch.empty(max(self.stage_cap, 16), dtype=torch.uint8, device=dev)
            self.staged_recs = torch.empty(self.n * STORE_REC_DT.itemsize, dtype=torch.uint8, device=dev)
            self.staged_ids = torch.empty(self.n, dtype=torch.int32, device=dev)
            self.offsets = torch.empty(self.n + 1, dtype=torch.int64, device=dev)
            self.stage_status = self._status[self.n + 1:]
            self._stage_args = (recs_ptr, nrecs, ids_ptr, self.n, self.max_frame_bytes, self.staging.data_ptr(),
                                self.stage_cap, self.staged_recs.data_ptr(), self.staged_ids.data_ptr(),
                                self.offsets.data_ptr(), self.stage_status.data_ptr())
            recs_ptr, nrecs, ids_ptr = self.staged_recs.data_ptr(), self.n, self.staged_ids.data_ptr()
        # an indexed store: the index tables as they are now, and the ids as the caller wrote them (not the staged ones)
        self.index_bits, self._index_args = store.index_bits, None
        if self.index_bits is not None:
            self._index_recs, self._entries = store._index_recs.dev, store._entries.dev
            self._index_args = (ids.data_ptr(), mem.ptr(self._index_recs), store._index_recs.n, mem.ptr(self._entries),
                                store._entries.n, self.index_bits)
        self._args = (recs_ptr, nrecs, mem.ptr(self._headers), self.nheaders, ids_ptr, self.n,
                      self.sub_bits, self.coef.data_ptr(), self.coef_cap, self.planes.data_ptr(), self.coef_cap, self.ws_cap,
                      dsts.data_ptr(), self.plan.data_ptr(), self.scan_jobs.data_ptr(), self.frame_jobs.data_ptr(),
                      self.build_status.data_ptr())

    def launch(self):
        """x3djpeg_store_build_jobs (two launches), x3djpeg_entropy_decode_batch (x3djpeg_entropy_decode_indexed for an
        indexed store), x3djpeg_decode_batch (two) on the current stream, after x3djpeg_stage (two) for a host-tier store,
        and nothing else: no allocation, no copy, no synchronisation."""
        L, s = _jpeglib.lib(), stream()
        if self._stage_args is not None:
            _jpeglib.check(L.x3djpeg_stage(*self._stage_args, s))
        _jpeglib.check(L.x3djpeg_store_build_jobs(*self._args, s))
        if self._index_args is not None:
            _jpeglib.check(L.x3djpeg_entropy_decode_indexed(self.scan_jobs.data_ptr(), self.n, *self._index_args,
                                                            self.status.data_ptr(), s))
        else:
            _jpeglib.check(L.x3djpeg_entropy_decode_batch(self.scan_jobs.data_ptr(), self.n, self.sub_bits,
                                                          self.workspace.data_ptr(), self.ws_cap, self.status.data_ptr(), s))
        _jpeglib.check(L.x3djpeg_decode_batch(self.frame_jobs.data_ptr(), self.n, self.max_blocks, self.max_w, self.max_h, s))

    def raise_for_status(self):
        """One read of the status words (a synchronisation); X3DHipError naming the first frame that failed."""
        st = self._status.cpu().numpy()
        bad = np.flatnonzero(st[:self.n])
        staged = int(st[self.n + 1]) if self.staged else 0
        what = "the stage refused the request (%s)" if staged else "the job builder refused the request (%s)"
        if st[self.n] or staged or bad.size:
            why = [text for bit, text in _STAGE_REASONS if staged & bit]
            why = why or [text for bit, text in _REASONS if st[self.n] & bit]   # a request the stage refused reads as a bad id
            i = int(bad[0]) if bad.size else -1
            raise X3DHipError("JPEG frame %d of the batch: libx3djpeg error %d: %s" % (
                i, int(st[i]) if bad.size else _jpeglib.EINVAL,
                what % ", ".join(why) if why else status_text(st[i])))


class FrameStore:
    """device: where the frames live.  chunk_bytes: the size of an arena chunk (None: 64 MiB; a frame larger than that gets
    a chunk of its own).  sub_bits: the subsequence length of the device Huffman decoder (None: the library's default),
    fixed for the store since the workspace a frame needs depends on it.  threads: host threads of add() (a
    jpegops.HostStages: no device is involved in filling).  check=False skips the read of
    the status words after decode / decode_into and leaves the batch in last_batch.  memory: see TorchMemory.  tier:
    "device" keeps the arena chunks where the tables are; "host" keeps them in pinned host memory (PinnedMemory) and
    decodes through a staging buffer per batch.  A `memory` given by the caller holds tables and chunks alike.
    index_bits: None for the relaxation decoder; a multiple of 32 (True: the library's default) keeps a sync index of
    that granularity for every frame, in device memory in both tiers, and decodes through it (the workspace is still
    sized for sub_bits: the indexed decoder does not use it)."""

    def __init__(self, device, chunk_bytes=None, sub_bits=None, threads=2, check=True, memory=None, tier="device",
                 index_bits=None):
        if tier not in TIERS:
            raise ValueError("tier must be one of %s (got %r)" % (", ".join(TIERS), tier))
        self.tier = tier
        self.memory = memory if memory is not None else TorchMemory(device)
        self.arena_memory = PinnedMemory() if tier == "host" and memory is None else self.memory
        self.device = torch.device(device)
        self.sub_bits = check_sub_bits(sub_bits)
        self.chunk_bytes = 64 << 20 if chunk_bytes is None else int(chunk_bytes)
        if self.chunk_bytes < 16 or self.chunk_bytes % 16:
            raise ValueError("chunk_bytes must be a positive multiple of 16 (got %r)" % (chunk_bytes,))
        self.check = bool(check)
        self.last_batch = None
        self._stages = HostStages(threads, self.sub_bits)
        self._chunks = []            # [buffer, bytes, bytes used]
        self._recs = _Table(self.memory, STORE_REC_DT, 1024)
        self._headers = _Table(self.memory, STORE_HEADER_DT, 8)
        self._header_index = {}      # header bytes -> index
        self._mirror = np.zeros(1024, MIRROR_DT)
        self.index_bits = check_index_bits(index_bits)
        if self.index_bits is not None:
            self._index_recs = _Table(self.memory, INDEX_REC_DT, 1024)
            self._entries = _Table(self.memory, np.dtype("<u8"), 1 << 14)

    def __len__(self):
        return self._recs.n

    def _field(name):                                       # noqa: N805  (the host mirror, one numpy array per field)
        return property(lambda self: self._mirror[name][:self._recs.n])

    width, height, nblocks = _field("width"), _field("height"), _field("nblocks")
    scan_bytes, nseg, coef_count, ws_need = _field("scan_bytes"), _field("nseg"), _field("coef_count"), _field("ws_need")
    nentries = _field("nentries")                           # of the frame's sync index; 0 in a store without one
    del _field

    @property
    def n_headers(self):
        return self._headers.n

    @property
    def n_chunks(self):
        return len(self._chunks)

    def addresses(self, ids=None):
        """(scan address, segment table address) per frame, as the record table holds them."""
        r = self._recs.host[:self._recs.n] if ids is None else self._recs.host[:self._recs.n][np.asarray(ids)]
        return r["scan"].copy(), r["segs"].copy()

    def bytes_resident(self):
        """Device bytes the store holds: the header table, the record table and the sync index, and in the device tier
        the arena chunks in full."""
        chunks = 0 if self.tier == "host" else sum(c[1] for c in self._chunks)
        return chunks + self._recs.nbytes + self._headers.nbytes + self.bytes_index()

    def bytes_index(self):
        """Device bytes of the sync index: its record table and its entry array as allocated; 0 without an index."""
        return 0 if self.index_bits is None else self._index_recs.nbytes + self._entries.nbytes

    def bytes_pinned(self):
        """Pinned host bytes the store holds: the arena chunks of the host tier in full."""
        return sum(c[1] for c in self._chunks) if self.tier == "host" else 0

    # ------------------------------------------------------------------ filling
    def add(self, files):
        """files: list of bytes, one JPEG file each.  Returns the range of their frame ids.  X3DHipError naming the first
        file the decoder does not take; nothing is stored then."""
        files = [f if isinstance(f, bytes) else bytes(f) for f in files]
        n, first = len(files), self._recs.n
        if n == 0:
            return range(first, first)
        infos, staged, scan_at, seg_at, scan_bytes, nseg, ws_need = self._stages._prepare_stage(files)
        if int(scan_bytes.max()) >= 1 << 31 or first + n >= 1 << 31:
            raise ValueError("the store holds fewer than 2^31 frames of fewer than 2^31 scan bytes")
        base = staged.data_ptr()
        entries = self._build_index(infos, base + scan_at[:-1], scan_bytes, base + seg_at[:-1], nseg)
        staged = staged.numpy()
        seg_len = nseg.astype(np.int64) * SCAN_SEG_DT.itemsize
        scan_len = (scan_bytes + SCAN_PAD + 15) & ~15
        size = scan_len + seg_len                           # a frame in the arena: its scan, padded, then its segment table
        chunk_of, off_of, chunks = self._place(size)
        # headers: equal to the previous frame's, or looked up by their bytes
        heads = store_headers(infos)
        hv = heads.view(np.uint8).reshape(n, -1)
        fresh = np.ones(n, bool)
        fresh[1:] = (hv[1:] != hv[:-1]).any(axis=1)
        index, added = dict(), []
        which = np.zeros(int(fresh.sum()), np.int64)
        for j, i in enumerate(np.flatnonzero(fresh)):
            key = hv[i].tobytes()
            h = self._header_index.get(key, index.get(key))
            if h is None:
                h = index[key] = self._headers.n + len(added)
                added.append(i)
            which[j] = h
        header_of = which[np.cumsum(fresh) - 1]
        # the arena: one packed host buffer per chunk touched, one copy each
        for c in np.unique(chunk_of):
            sel = np.flatnonzero(chunk_of == c)
            lo, hi = int(off_of[sel[0]]), int(off_of[sel[-1]] + size[sel[-1]])
            pack = np.zeros(hi - lo, np.uint8)
            for i in sel:
                o = int(off_of[i]) - lo
                nb = int(scan_bytes[i]) + SCAN_PAD
                pack[o:o + nb] = staged[scan_at[i]:scan_at[i] + nb]
                o += int(scan_len[i])
                pack[o:o + seg_len[i]] = staged[seg_at[i]:seg_at[i] + seg_len[i]]
            self.arena_memory.write(chunks[c][0], lo, pack)
            chunks[c][2] = hi
        self._commit(chunks, chunk_of, off_of, scan_bytes, nseg, header_of, heads[added], index,
                     {f: infos[f] for f in ("width", "height", "nblocks", "coef_count")}, ws_need, entries)
        return range(first, first + n)

    def _build_index(self, infos, scan_ptr, scan_bytes, seg_ptr, nseg):
        """The sync index of n prepared frames on the host threads: (entries per frame, uint64 entries of all of them in
        order), or None for a store without an index.  infos: INFO_DT [n]; the rest one entry per frame, host addresses.
        X3DHipError naming the first frame the indexer refuses."""
        if self.index_bits is None:
            return None
        L, bits, n = _jpeglib.lib(), self.index_bits, len(infos)
        scan_p, seg_p = [int(v) for v in scan_ptr], [int(v) for v in seg_ptr]
        scan_b, nseg_l = [int(v) for v in scan_bytes], [int(v) for v in nseg]
        count = np.array([L.x3djpeg_index_count(seg_p[i], nseg_l[i], bits) for i in range(n)], np.int64)
        at = np.concatenate([[0], np.cumsum(count)])
        out = np.zeros(int(at[-1]), np.uint64)
        wrote = np.zeros(n, np.uint64)
        info_ptr, info_size, out_ptr, wrote_ptr = infos.ctypes.data, INFO_DT.itemsize, out.ctypes.data, wrote.ctypes.data
        at_l, count_l, fail = at.tolist(), count.tolist(), self._stages._fail

        def build(lo, hi):
            res = []
            for i in range(lo, hi):
                rc = L.x3djpeg_index_build(scan_p[i], scan_b[i], seg_p[i], nseg_l[i], info_ptr + i * info_size, bits,
                                           out_ptr + 8 * at_l[i], count_l[i], wrote_ptr + 8 * i)
                res.append(fail(i, rc) if rc else None)
            return res

        for msg in self._stages._chunks(build, n):
            if msg:
                raise X3DHipError(msg)
        assert np.array_equal(wrote.astype(np.int64), count)
        return count, out

    def _place(self, size):
        """Placement of frames of `size` bytes each: in order, a new chunk when the next frame does not fit.  Returns
        (chunk per frame, offset in it per frame, the chunk list to be).  Chunks are allocated, nothing of the store is
        touched: a failed allocation leaves it as it was."""
        ends = np.cumsum(size)
        n = len(size)
        chunk_of, off_of = np.zeros(n, np.int64), np.zeros(n, np.int64)
        new_chunks, at = [], 0
        cur = len(self._chunks) - 1
        room = self._chunks[cur][1] - self._chunks[cur][2] if cur >= 0 else 0
        used0 = self._chunks[cur][2] if cur >= 0 else 0
        while at < n:
            before = int(ends[at - 1]) if at else 0
            k = int(np.searchsorted(ends, before + room, side="right"))       # frames [at, k) fit
            if k > at:
                chunk_of[at:k] = cur
                off_of[at:k] = used0 + ends[at:k] - size[at:k] - before
                placed = int(ends[k - 1]) - before
                room, used0, at = room - placed, used0 + placed, k
                continue
            cap = max(self.chunk_bytes, int(size[at]))
            new_chunks.append([self.arena_memory.alloc(cap), cap, 0])
            cur, room, used0 = len(self._chunks) + len(new_chunks) - 1, cap, 0
        return chunk_of, off_of, [list(c) for c in self._chunks] + new_chunks

    def _commit(self, chunks, chunk_of, off_of, scan_bytes, nseg, header_of, new_headers, new_index, fields, ws_need,
                entries=None):
        """The arena is written: the records, the new headers, the mirror and (entries: what _build_index gave) the sync
        index of n more frames."""
        n, first = len(chunk_of), self._recs.n
        scan_len = (np.asarray(scan_bytes, np.int64) + SCAN_PAD + 15) & ~15
        base = np.array([self.arena_memory.ptr(chunks[c][0]) for c in chunk_of], np.uint64)
        recs = np.zeros(n, STORE_REC_DT)
        recs["scan"] = base + off_of.astype(np.uint64)
        recs["segs"] = recs["scan"] + scan_len.astype(np.uint64)
        recs["scan_bytes"], recs["nseg"], recs["header"] = scan_bytes, nseg, header_of
        self._chunks = chunks
        if len(new_headers):
            self._headers.append(new_headers)
            self._header_index.update(new_index)
        self._recs.append(recs)
        if first + n > len(self._mirror):
            grown = np.zeros(max(first + n, 2 * len(self._mirror)), MIRROR_DT)
            grown[:first] = self._mirror[:first]
            self._mirror = grown
        m = self._mirror[first:first + n]
        for f, v in fields.items():
            m[f] = v
        m["scan_bytes"], m["nseg"], m["ws_need"], m["chunk"] = scan_bytes, nseg, ws_need, chunk_of
        if entries is not None:
            count, words = entries
            irecs = np.zeros(n, INDEX_REC_DT)
            irecs["first_entry"] = self._entries.n + np.cumsum(count) - count
            irecs["nentries"] = m["nentries"] = count
            self._entries.append(words)
            self._index_recs.append(irecs)

    # ------------------------------------------------------------------ decoding
    def _ids(self, ids):
        ids = np.asarray(ids if not isinstance(ids, range) else np.arange(ids.start, ids.stop, ids.step), dtype=np.int64)
        if ids.ndim != 1 or ids.size < 1 or ids.size > 65535:
            raise ValueError("a batch holds 1 .. 65535 frames (got %s)" % (ids.shape,))
        bad = np.flatnonzero((ids < 0) | (ids >= len(self)))
        if bad.size:
            raise ValueError("frame id %d (request %d) outside the %d frames of the store" % (ids[bad[0]], bad[0], len(self)))
        return ids

    def _run(self, ids, dst_ptr, dst_stride, width, height, check):
        """ids: checked; dst_ptr, dst_stride, width, height: one entry per request (numpy)."""
        n = ids.size
        m = self._mirror[ids]
        table = np.zeros(n, STORE_DST_DT)                   # one upload: 28 bytes per request, table then ids
        table["dst"], table["dst_stride"], table["width"], table["height"] = dst_ptr, dst_stride, width, height
        blob = np.concatenate([table.view(np.uint8).reshape(-1), ids.astype(np.int32).view(np.uint8)])
        with torch.cuda.device(self.device):
            up = torch.from_numpy(blob).to(self.device)
            b = Batch(self, n, int(m["coef_count"].sum()), int(m["ws_need"].sum()), int(m["nblocks"].max()),
                      int(m["width"].max()), int(m["height"].max()), up[table.nbytes:].view(torch.int32), up[:table.nbytes],
                      **self._stage_sizes(m, None))
            b.launch()
        self.last_batch = b
        if self.check if check is None else check:
            b.raise_for_status()
        return b

    def _stage_sizes(self, m, n):
        """The staging buffer of a batch over the frames m (mirror rows): their exact sum (n None), or n times the largest
        (a planned batch).  Nothing for the device tier."""
        if self.tier != "host":
            return {}
        size = stage_bytes(m["scan_bytes"], m["nseg"])
        largest = int(size.max())
        return dict(stage_cap=int(size.sum()) if n is None else n * largest, max_frame_bytes=largest)

    def decode_into(self, ids, dst, check=None):
        """ids: n frame ids of frames of one size; dst: uint8 [n, H, W, 3] on the device, unit stride over the channels, 3
        over x, any row stride >= 3 * W and any frame stride.  ValueError for an id outside the store or a frame whose size
        is not dst's, before anything is launched."""
        ids = self._ids(ids)
        n = ids.size
        H, W = check_dst(dst, n, self.device)
        w, h = self._mirror["width"][ids], self._mirror["height"][ids]
        bad = np.flatnonzero((w != W) | (h != H))
        if bad.size:
            i = int(bad[0])
            raise ValueError("frame %d is %d x %d, dst holds %d x %d frames" % (i, w[i], h[i], W, H))
        ptr = dst.data_ptr() + np.arange(n, dtype=np.int64) * dst.stride(0)
        self._run(ids, ptr.astype(np.uint64), dst.stride(1), W, H, check)
        return dst

    def decode(self, ids, check=None):
        """A list of uint8 [H, W, 3] tensors on the device, one per id; the frames may differ in size."""
        ids = self._ids(ids)
        w, h = self._mirror["width"][ids].astype(np.int64), self._mirror["height"][ids].astype(np.int64)
        at = np.concatenate([[0], np.cumsum(3 * w * h)])
        flat = torch.empty(int(at[-1]), dtype=torch.uint8, device=self.device)
        self._run(ids, (flat.data_ptr() + at[:-1]).astype(np.uint64), 3 * w, w, h, check)
        return [flat[a:e].view(int(y), int(x), 3) for a, e, y, x in zip(at[:-1].tolist(), at[1:].tolist(), h.tolist(), w.tolist())]

    def plan(self, n, width, height):
        """A reusable batch of n frames of width x height: static tensors ids (int32 [n], every entry the first stored
        frame of that size) and dst (uint8 [n, height, width, 3]), buffers sized for the largest frame of that size the
        store holds now.  batch.launch() decodes the frames ids name into dst; an id outside the store as it is now, or of
        a frame of another size, is refused on the device (batch.status, batch.build_status); it keeps its place in the buffers,
        which are sized for frames of this size, so requests after a larger frame may be refused for lack of room too."""
        n = int(n)
        if n < 1 or n > 65535:
            raise ValueError("a batch holds 1 .. 65535 frames (got %d)" % n)
        m = self._mirror[:len(self)]
        sel = np.flatnonzero((m["width"] == width) & (m["height"] == height))
        if not sel.size:
            raise ValueError("the store holds no frame of %d x %d" % (width, height))
        m = m[sel]
        with torch.cuda.device(self.device):
            dst = torch.empty((n, height, width, 3), dtype=torch.uint8, device=self.device)
            table = np.zeros(n, STORE_DST_DT)
            table["dst"] = (dst.data_ptr() + np.arange(n, dtype=np.int64) * dst.stride(0)).astype(np.uint64)
            table["dst_stride"], table["width"], table["height"] = 3 * width, width, height
            dsts = torch.from_numpy(table.view(np.uint8).reshape(-1)).to(self.device)
            ids = torch.full((n,), int(sel[0]), dtype=torch.int32, device=self.device)
            return Batch(self, n, n * int(m["coef_count"].max()), n * int(m["ws_need"].max()), int(m["nblocks"].max()),
                         width, height, ids, dsts, dst, **self._stage_sizes(m, n))

    # ------------------------------------------------------------------ pack files
    def save(self, path, meta=None):
        """Writes the store as one pack file (see PACK_HEAD): data only, no address.  meta: anything json.dumps takes; it
        comes back from load()."""
        n, nh = len(self), self._headers.n
        blob = json.dumps(meta).encode("utf-8")
        m = self._mirror[:n]
        recs = self._recs.host[:n]
        size = stage_bytes(m["scan_bytes"], m["nseg"])
        tables = PACK_HEAD.size + nh * STORE_HEADER_DT.itemsize + n * PACK_FRAME_DT.itemsize
        arena_at = (tables + 15) & ~15
        used = np.array([c[2] for c in self._chunks], np.int64)
        chunk_at = arena_at + np.cumsum(used) - used        # a chunk's used part holds its frames in order without a gap
        base = np.array([self.arena_memory.ptr(c[0]) for c in self._chunks], np.uint64)
        ft = np.zeros(n, PACK_FRAME_DT)
        if n:
            ft["offset"] = chunk_at[m["chunk"]].astype(np.uint64) + (recs["scan"] - base[m["chunk"]])
        ft["length"] = size
        for f in ("scan_bytes", "nseg", "width", "height", "nblocks", "coef_count"):
            ft[f] = m[f]
        ft["header"] = recs["header"]
        with open(path, "wb") as f:
            f.write(PACK_HEAD.pack(PACK_MAGIC, PACK_VERSION, STORE_HEADER_DT.itemsize, PACK_FRAME_DT.itemsize, self.sub_bits,
                                   n, nh, arena_at, int(used.sum()), len(blob)))
            f.write(self._headers.host[:nh].tobytes())
            f.write(ft.tobytes())
            f.write(b"\0" * (arena_at - tables))
            for c in self._chunks:
                step = 64 << 20
                for lo in range(0, c[2], step):
                    f.write(memoryview(np.ascontiguousarray(_read(self.arena_memory, c[0], lo, min(step, c[2] - lo)))))
            f.write(blob)
        if self.index_bits is not None:
            total = self._entries.n
            with open(path + INDEX_SUFFIX, "wb") as f:
                f.write(INDEX_HEAD.pack(INDEX_MAGIC, INDEX_VERSION, self.index_bits, n, int(used.sum()), total))
                f.write(m["nentries"].astype("<u4").tobytes())
                f.write(b"\0" * (-(INDEX_HEAD.size + 4 * n) % 8))
                f.write(self._entries.host[:total].tobytes())

    @staticmethod
    def _read_index_tables(f, path, nframes, arena_bytes, scan_bytes, nseg):
        """(index_bits, entry count per frame, file offset of the entries) of an open sidecar, checked against the pack it
        is read with (its frame count and arena bytes, and per frame the bounds its sizes put on the count); ValueError
        for any defect."""
        def bad(why):
            return ValueError("%s is not the sync index of this pack in a form this version reads: %s" % (path, why))
        file_bytes = os.fstat(f.fileno()).st_size
        head = f.read(INDEX_HEAD.size)
        if len(head) < INDEX_HEAD.size:
            raise bad("%d bytes, shorter than its head" % file_bytes)
        magic, version, bits, n, arena, total = INDEX_HEAD.unpack(head)
        if magic != INDEX_MAGIC:
            raise bad("magic %r" % magic)
        if version != INDEX_VERSION:
            raise bad("format version %d, not %d" % (version, INDEX_VERSION))
        if bits < 32 or bits % 32 or bits > 1 << 20:
            raise bad("index_bits %d" % bits)
        if n != nframes or arena != arena_bytes:
            raise bad("made for a pack of %d frames and %d arena bytes, not %d and %d" % (n, arena, nframes, arena_bytes))
        at = (INDEX_HEAD.size + 4 * n + 7) & ~7
        if total >= 1 << 59 or at + 8 * total != file_bytes:
            raise bad("its counts (%d frames, %d entries) do not give its %d bytes" % (n, total, file_bytes))
        count = np.frombuffer(f.read(4 * n), "<u4").astype(np.int64)
        if len(count) != n or int(count.sum()) != total:
            raise bad("the frames' entry counts do not sum to its %d entries" % total)
        # a segment has ceil(bits / index_bits) entries, at least one: what the sizes alone say (the decoder checks the rest)
        most = np.asarray(scan_bytes, np.int64) * 8 // bits + np.asarray(nseg, np.int64)
        wrong = (count < np.asarray(nseg, np.int64)) | (count > most)
        if wrong.any():
            i = int(np.flatnonzero(wrong)[0])
            raise bad("frame %d: %d entries for %d scan bytes in %d segments" % (i, count[i], scan_bytes[i], nseg[i]))
        return bits, count, at

    @staticmethod
    def _read_pack_tables(f, path):
        """(sub_bits at save, header table, frame table, meta) of an open pack file; ValueError for any defect."""
        def bad(why):
            return ValueError("%s is not a frame pack this version reads: %s" % (path, why))
        file_bytes = os.fstat(f.fileno()).st_size
        head = f.read(PACK_HEAD.size)
        if len(head) < PACK_HEAD.size:
            raise bad("%d bytes, shorter than its head" % file_bytes)
        magic, version, hbytes, fbytes, sub_bits, n, nh, arena_at, arena_bytes, meta_bytes = PACK_HEAD.unpack(head)
        if magic != PACK_MAGIC:
            raise bad("magic %r" % magic)
        if version != PACK_VERSION:
            raise bad("format version %d, not %d" % (version, PACK_VERSION))
        if hbytes != STORE_HEADER_DT.itemsize or fbytes != PACK_FRAME_DT.itemsize:
            raise bad("entries of %d and %d bytes, not %d and %d" % (hbytes, fbytes, STORE_HEADER_DT.itemsize,
                                                                     PACK_FRAME_DT.itemsize))
        if n >= 1 << 31 or nh >= 1 << 31 or (n and not nh):
            raise bad("%d frames with %d headers" % (n, nh))
        tables = PACK_HEAD.size + nh * hbytes + n * fbytes
        if arena_at != (tables + 15) & ~15 or arena_at + arena_bytes + meta_bytes != file_bytes:
            raise bad("its counts (%d frames, %d headers, %d arena bytes at %d, %d meta bytes) do not give its %d bytes" % (
                n, nh, arena_bytes, arena_at, meta_bytes, file_bytes))
        heads = np.frombuffer(f.read(nh * hbytes), STORE_HEADER_DT)
        ft = np.frombuffer(f.read(n * fbytes), PACK_FRAME_DT)
        if len(heads) != nh or len(ft) != n:
            raise bad("shorter than its tables")
        if n:
            off, length = ft["offset"].astype(np.int64), ft["length"].astype(np.int64)
            wrong = ((ft["scan_bytes"] < 0) | (ft["nseg"] < 1) | (length != stage_bytes(ft["scan_bytes"], ft["nseg"]))
                     | (off < arena_at) | (off % 16 != 0) | (off + length > arena_at + arena_bytes) | (off + length < off))
            if wrong.any():
                i = int(np.flatnonzero(wrong)[0])
                raise bad("frame %d: %d bytes at %d, outside the arena [%d, %d) or not what its sizes give" % (
                    i, length[i], off[i], arena_at, arena_at + arena_bytes))
            wrong = (ft["header"] < 0) | (ft["header"] >= nh)
            if wrong.any():
                i = int(np.flatnonzero(wrong)[0])
                raise bad("frame %d: header %d of %d" % (i, ft["header"][i], nh))
            h = heads[ft["header"]]
            wrong = ((h["frame"]["width"] != ft["width"]) | (h["frame"]["height"] != ft["height"])
                     | (h["frame"]["nblocks"] != ft["nblocks"]) | (h["scan"]["coef_count"] != ft["coef_count"])
                     | (ft["coef_count"] != ft["nblocks"].astype(np.int64) * 64) | (ft["nblocks"] < 1) | (ft["width"] < 1)
                     | (ft["height"] < 1))
            if wrong.any():
                i = int(np.flatnonzero(wrong)[0])
                raise bad("frame %d: its sizes are not its header's" % i)
        f.seek(arena_at + arena_bytes)
        try:
            meta = json.loads(f.read(meta_bytes).decode("utf-8"))
        except ValueError as e:
            raise bad("meta: %s" % e)
        return sub_bits, heads, ft, meta

    @classmethod
    def read_meta(cls, path):
        """The meta blob of a pack file, after the same checks of its tables as load() makes; no frame is read."""
        with open(path, "rb") as f:
            return cls._read_pack_tables(f, path)[3]

    @classmethod
    def load(cls, path, device, tier="device", sub_bits=None, ranges=None, memory=None, index=None, **kw):
        """Reads a pack file.  Returns (store, meta, id_map).  ranges: a list of ranges of saved frame ids (None: all of
        them); only those frames are read, placed as add() places frames, and id_map is the list of the ranges of their
        new ids, one per entry of `ranges`.  sub_bits: None takes the one the pack was saved with.  The host tier reads
        straight into each chunk's host view, the device tier through one staging buffer per chunk.  ValueError, before
        any store exists, for a file that is not a whole pack of this version.  index: None uses the pack's sync index
        (path + ".idx") if that file is there -- only the entries of the frames read are read -- and gives a store
        without an index otherwise; False ignores the file; an int (True: the library's default) builds the index of that
        granularity from the scans as they are read.  A sidecar that is not this pack's whole index is a ValueError too."""
        with open(path, "rb") as f:
            saved_bits, heads, ft, meta = cls._read_pack_tables(f, path)
            f.seek(0)
            arena_bytes = PACK_HEAD.unpack(f.read(PACK_HEAD.size))[8]
            if ranges is None:
                ranges = [range(len(ft))]
            ranges = [r if isinstance(r, range) else range(*r) for r in ranges]
            for r in ranges:
                if r.step != 1 or (len(r) and (r.start < 0 or r.stop > len(ft))):
                    raise ValueError("range %r outside the %d frames of %s (or not of step 1)" % (r, len(ft), path))
            sel = np.concatenate([np.arange(r.start, r.stop, dtype=np.int64) for r in ranges] + [np.zeros(0, np.int64)])
            side = None                                     # (entry count per frame read, their entries)
            if index is None and os.path.exists(path + INDEX_SUFFIX):
                with open(path + INDEX_SUFFIX, "rb") as g:
                    index_bits, count, ent_at = cls._read_index_tables(g, path + INDEX_SUFFIX, len(ft), arena_bytes,
                                                                       ft["scan_bytes"], ft["nseg"])
                    first = np.cumsum(count) - count
                    words = np.zeros(int(count[sel].sum()), np.uint64)
                    o = 0
                    for r in ranges:                        # the frames of a range follow each other in the sidecar
                        nb = int(count[r.start:r.stop].sum()) if len(r) else 0
                        if nb:
                            g.seek(ent_at + 8 * int(first[r.start]))
                            if g.readinto(memoryview(words)[o:o + nb]) != 8 * nb:
                                raise ValueError("%s ends inside frame %d" % (path + INDEX_SUFFIX, r.start))
                        o += nb
                    side = (count[sel], words)
            else:
                index_bits = check_index_bits(index)
            store = cls(device, sub_bits=saved_bits if sub_bits is None else sub_bits, memory=memory, tier=tier,
                        index_bits=index_bits, **kw)
            n = sel.size
            at = np.cumsum([0] + [len(r) for r in ranges])
            id_map = [range(int(a), int(b)) for a, b in zip(at[:-1], at[1:])]
            if len(heads):
                store._headers.append(heads)
                store._header_index = {heads[i:i + 1].tobytes(): i for i in range(len(heads) - 1, -1, -1)}
            if n == 0:
                return store, meta, id_map
            t = ft[sel]
            size, src = t["length"].astype(np.int64), t["offset"].astype(np.int64)
            chunk_of, off_of, chunks = store._place(size)
            mem = store.arena_memory
            L, built = _jpeglib.lib(), []
            scan_len = (t["scan_bytes"].astype(np.int64) + SCAN_PAD + 15) & ~15
            if index_bits is not None and side is None:
                infos = np.zeros(n, INFO_DT)                # what the indexer reads of an info is what a scan job holds
                _jpeglib.fill_scan_jobs(infos, heads[t["header"]]["scan"])
            for c in np.unique(chunk_of):
                idx = np.flatnonzero(chunk_of == c)
                lo, hi = int(off_of[idx[0]]), int(off_of[idx[-1]] + size[idx[-1]])
                view = mem.host_view(chunks[c][0])[lo:hi] if hasattr(mem, "host_view") else np.empty(hi - lo, np.uint8)
                # runs of frames that follow each other in the file: one read each
                cut = np.flatnonzero(src[idx[1:]] != src[idx[:-1]] + size[idx[:-1]]) + 1
                for run in np.split(idx, cut):
                    a = int(off_of[run[0]]) - lo
                    nb = int(size[run].sum())
                    f.seek(int(src[run[0]]))
                    if f.readinto(memoryview(view)[a:a + nb]) != nb:
                        raise ValueError("%s ends inside frame %d" % (path, sel[run[0]]))
                if index_bits is not None:
                    scan_ptr = view.ctypes.data + off_of[idx] - lo
                    if side is None:
                        built.append(store._build_index(infos[idx], scan_ptr, t["scan_bytes"][idx], scan_ptr + scan_len[idx],
                                                        t["nseg"][idx]))
                    else:                                   # the counts against the segment tables themselves
                        for i, sp in zip(idx.tolist(), (scan_ptr + scan_len[idx]).tolist()):
                            if L.x3djpeg_index_count(sp, int(t["nseg"][i]), index_bits) != side[0][i]:
                                raise ValueError("%s is not the sync index of this pack: frame %d has %d entries at "
                                                 "index_bits %d" % (path + INDEX_SUFFIX, sel[i], side[0][i], index_bits))
                if not hasattr(mem, "host_view"):
                    mem.write(chunks[c][0], lo, view)
                chunks[c][2] = hi
        uniq, inv = np.unique(np.stack([t["scan_bytes"], t["nseg"]], axis=1), axis=0, return_inverse=True)
        ws = np.array([_jpeglib.workspace_bytes(a, b, store.sub_bits) for a, b in uniq.tolist()], np.int64)
        store._commit(chunks, chunk_of, off_of, t["scan_bytes"], t["nseg"], t["header"], heads[:0], {},
                      {f: t[f] for f in ("width", "height", "nblocks", "coef_count")}, ws[inv.reshape(-1)],
                      side if side is not None else
                      (np.concatenate([b[0] for b in built]), np.concatenate([b[1] for b in built])) if built else None)
        return store, meta, id_map
