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
"""
import numpy as np
import torch

from . import _jpeglib
from ._jpeglib import (FRAME_JOB_DT, SCAN_JOB_DT, SCAN_PAD, SCAN_SEG_DT, STORE_DST_DT, STORE_HEADER_DT, STORE_REC_DT,
                       SUB_BITS_DEFAULT)
from ._lib import X3DHipError, stream
from .jpegops import JpegDecoder, fill_jobs

MIRROR_DT = np.dtype([("width", "<i4"), ("height", "<i4"), ("nblocks", "<i4"), ("scan_bytes", "<i4"), ("nseg", "<i4"),
                      ("chunk", "<i4"), ("coef_count", "<i8"), ("ws_need", "<i8")])
_REASONS = ((_jpeglib.STORE_BAD_ID, "a frame id outside the store"),
            (_jpeglib.STORE_BAD_SIZE, "a frame of another size than its destination"),
            (_jpeglib.STORE_NO_COEF, "coefficients beyond the buffer"), (_jpeglib.STORE_NO_WS, "workspace beyond the buffer"))


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


class _HostStages(JpegDecoder):
    """JpegDecoder's parse and prepare stages on their own: the thread pool and the staging buffer, no device."""

    def __init__(self, threads, sub_bits):
        from concurrent.futures import ThreadPoolExecutor
        self.sub_bits = sub_bits
        self.threads = max(1, min(16, int(threads)))
        self._pool = ThreadPoolExecutor(max_workers=self.threads) if self.threads > 1 else None
        self._bytes = None

    def _staging(self, total):                              # read by add() before it returns: plain memory will do
        if self._bytes is None or self._bytes.numel() < total:
            self._bytes = torch.empty(max(total, 1 << 16), dtype=torch.uint8)
        self._pinned_bytes = self._bytes
        return self._bytes


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

    def __init__(self, store, n, coef_cap, ws_cap, max_blocks, max_w, max_h, ids, dsts, dst=None):
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
        self._status = torch.empty(self.n + 1, dtype=torch.int32, device=dev)
        self.status, self.build_status = self._status[:self.n], self._status[self.n:]
        # the tables as they are now: a later add() may move them, and leaves these to this batch
        self._recs, self._headers = store._recs.dev, store._headers.dev
        self.nrecs, self.nheaders = store._recs.n, store._headers.n
        self._args = (mem.ptr(self._recs), self.nrecs, mem.ptr(self._headers), self.nheaders, ids.data_ptr(), self.n,
                      self.sub_bits, self.coef.data_ptr(), self.coef_cap, self.planes.data_ptr(), self.coef_cap, self.ws_cap,
                      dsts.data_ptr(), self.plan.data_ptr(), self.scan_jobs.data_ptr(), self.frame_jobs.data_ptr(),
                      self.build_status.data_ptr())

    def launch(self):
        """x3djpeg_store_build_jobs (two launches), x3djpeg_entropy_decode_batch, x3djpeg_decode_batch (two) on the current
        stream, and nothing else: no allocation, no copy, no synchronisation."""
        L, s = _jpeglib.lib(), stream()
        _jpeglib.check(L.x3djpeg_store_build_jobs(*self._args, s))
        _jpeglib.check(L.x3djpeg_entropy_decode_batch(self.scan_jobs.data_ptr(), self.n, self.sub_bits,
                                                      self.workspace.data_ptr(), self.ws_cap, self.status.data_ptr(), s))
        _jpeglib.check(L.x3djpeg_decode_batch(self.frame_jobs.data_ptr(), self.n, self.max_blocks, self.max_w, self.max_h, s))

    def raise_for_status(self):
        """One read of the status words (a synchronisation); X3DHipError naming the first frame that failed."""
        st = self._status.cpu().numpy()
        bad = np.flatnonzero(st[:self.n])
        if st[self.n] or bad.size:
            why = [text for bit, text in _REASONS if st[self.n] & bit]
            i = int(bad[0]) if bad.size else -1
            raise X3DHipError("JPEG frame %d of the batch: libx3djpeg error %d: %s" % (
                i, int(st[i]) if bad.size else _jpeglib.EINVAL,
                "the job builder refused the request (%s)" % ", ".join(why) if why else
                "corrupt JPEG: the device Huffman decoder refused the scan" if st[i] == _jpeglib.ECORRUPT else
                "the scan job does not fit its sizes or its workspace"))


class FrameStore:
    """device: where the frames live.  chunk_bytes: the size of an arena chunk (a frame larger than that gets a chunk of
    its own).  sub_bits: the subsequence length of the device Huffman decoder (None: the library's default), fixed for the
    store since the workspace a frame needs depends on it.  threads: host threads of add().  check=False skips the read of
    the status words after decode / decode_into and leaves the batch in last_batch.  memory: see TorchMemory."""

    def __init__(self, device, chunk_bytes=64 << 20, sub_bits=None, threads=2, check=True, memory=None):
        self.memory = memory if memory is not None else TorchMemory(device)
        self.device = torch.device(device)
        self.sub_bits = SUB_BITS_DEFAULT if sub_bits is None else int(sub_bits)
        if self.sub_bits < 32 or self.sub_bits % 32 or self.sub_bits > 1 << 20:
            raise ValueError("sub_bits must be a multiple of 32 in 32 .. 2^20 (got %r)" % (sub_bits,))
        self.chunk_bytes = int(chunk_bytes)
        if self.chunk_bytes < 16 or self.chunk_bytes % 16:
            raise ValueError("chunk_bytes must be a positive multiple of 16 (got %r)" % (chunk_bytes,))
        self.check = bool(check)
        self.last_batch = None
        _jpeglib.lib()
        self._stages = _HostStages(threads, self.sub_bits)
        self._chunks = []            # [buffer, bytes, bytes used]
        self._recs = _Table(self.memory, STORE_REC_DT, 1024)
        self._headers = _Table(self.memory, STORE_HEADER_DT, 8)
        self._header_index = {}      # header bytes -> index
        self._mirror = np.zeros(1024, MIRROR_DT)

    def __len__(self):
        return self._recs.n

    def _field(name):                                       # noqa: N805  (the host mirror, one numpy array per field)
        return property(lambda self: self._mirror[name][:self._recs.n])

    width, height, nblocks = _field("width"), _field("height"), _field("nblocks")
    scan_bytes, nseg, coef_count, ws_need = _field("scan_bytes"), _field("nseg"), _field("coef_count"), _field("ws_need")
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
        """Device bytes the store holds: the arena chunks in full, the header table and the record table."""
        return sum(c[1] for c in self._chunks) + self._recs.nbytes + self._headers.nbytes

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
        staged = staged.numpy()
        seg_len = nseg.astype(np.int64) * SCAN_SEG_DT.itemsize
        scan_len = (scan_bytes + SCAN_PAD + 15) & ~15
        size = scan_len + seg_len                           # a frame in the arena: its scan, padded, then its segment table
        # placement: frames in order, a new chunk when the next frame does not fit.  Chunks are allocated, nothing of the
        # store is touched until everything is in place.
        ends = np.cumsum(size)
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
            new_chunks.append([self.memory.alloc(cap), cap, 0])
            cur, room, used0 = len(self._chunks) + len(new_chunks) - 1, cap, 0
        chunks = self._chunks + new_chunks
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
            self.memory.write(chunks[c][0], lo, pack)
            chunks[c][2] = hi
        base = np.array([self.memory.ptr(chunks[c][0]) for c in chunk_of], np.uint64)
        recs = np.zeros(n, STORE_REC_DT)
        recs["scan"] = base + off_of.astype(np.uint64)
        recs["segs"] = recs["scan"] + scan_len.astype(np.uint64)
        recs["scan_bytes"], recs["nseg"], recs["header"] = scan_bytes, nseg, header_of
        # commit
        self._chunks = chunks
        if added:
            self._headers.append(heads[added])
            self._header_index.update(index)
        self._recs.append(recs)
        if first + n > len(self._mirror):
            grown = np.zeros(max(first + n, 2 * len(self._mirror)), MIRROR_DT)
            grown[:first] = self._mirror[:first]
            self._mirror = grown
        m = self._mirror[first:first + n]
        for f in ("width", "height", "nblocks", "coef_count"):
            m[f] = infos[f]
        m["scan_bytes"], m["nseg"], m["ws_need"], m["chunk"] = scan_bytes, nseg, ws_need, chunk_of
        return range(first, first + n)

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
                      int(m["width"].max()), int(m["height"].max()), up[table.nbytes:].view(torch.int32), up[:table.nbytes])
            b.launch()
        self.last_batch = b
        if self.check if check is None else check:
            b.raise_for_status()
        return b

    def decode_into(self, ids, dst, check=None):
        """ids: n frame ids of frames of one size; dst: uint8 [n, H, W, 3] on the device, unit stride over the channels, 3
        over x, any row stride >= 3 * W and any frame stride.  ValueError for an id outside the store or a frame whose size
        is not dst's, before anything is launched."""
        ids = self._ids(ids)
        if (not isinstance(dst, torch.Tensor) or dst.device != self.device or dst.dtype != torch.uint8 or dst.dim() != 4
                or dst.shape[3] != 3 or dst.shape[0] != ids.size):
            raise ValueError("dst must be a uint8 tensor [%d, H, W, 3] on %s" % (ids.size, self.device))
        n, H, W, _ = dst.shape
        if dst.stride(3) != 1 or dst.stride(2) != 3 or dst.stride(1) < 3 * W or dst.stride(0) < 0:
            raise ValueError("dst needs strides (any, >= 3 * W, 3, 1), got %s" % (tuple(dst.stride()),))
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
                         width, height, ids, dsts, dst)
