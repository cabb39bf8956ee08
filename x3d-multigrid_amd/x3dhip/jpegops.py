"""JPEG frames -> uint8 [H, W, 3] tensors in HBM over the C ABI of include/x3djpeg.h, bit-exact with Pillow.

The serial stage (headers, Huffman decoding) runs on the host in a thread pool (ctypes releases the GIL) into one reused
pinned coefficient buffer; one asynchronous copy, one job table and two kernel launches per batch go on the current
stream, whatever the number of frames and however they differ in size or subsampling.  There is no fallback: a frame the
library does not take raises X3DHipError and nothing is launched for its batch.

entropy="device" moves the Huffman decoding to the GPU as well: the thread pool only parses the headers and strips the
byte stuffing and restart markers (x3djpeg_scan_prepare) into a reused pinned byte buffer, the copy carries the
entropy-coded bytes instead of the coefficients (about 1/18 of them), and one more launch
(x3djpeg_entropy_decode_batch, one workgroup per frame) fills the coefficient buffer the two kernels read, bit for bit
what the host decoder writes.  A damaged scan is then found on the device: the per-frame status is read back once per
batch, after the launches.

HostStages holds the part of this that needs no device (the pool, the header parse, the scan preparation into plain host
memory): jpegstore.FrameStore fills itself through one, and JpegDecoder is a HostStages whose staging buffer is pinned.
check_dst, check_sub_bits and status_text are the argument checks and the status wording the decoder and the store share.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _jpeglib
from ._jpeglib import FRAME_JOB_DT, INFO_DT, SCAN_JOB_DT, SCAN_PAD, SCAN_SEG_DT, SUB_BITS_DEFAULT
from ._lib import X3DHipError, stream

_JOB_FIELDS = ("width", "height", "ncomp", "hmax", "vmax", "nblocks", "blocks_w", "blocks_h", "cw", "ch", "block_start")


def fill_jobs(jobs, infos):
    """The fields of X3DJpegFrameJob that come from X3DJpegInfo (everything but the four pointers / strides)."""
    for f in _JOB_FIELDS:
        jobs[f] = infos[f]
    tq = infos["comp_tq"]
    jobs["qt"] = np.take_along_axis(infos["qt"], tq[:, :, None].astype(np.int64), axis=1)


def frame_jobs(infos, offs, coef, planes, targets):
    """The X3DJpegFrameJob table of a batch: frame i's coefficients and planes at element offs[i] of the device buffers
    coef (int16) and planes (uint8), its destination targets[i] = (data_ptr, row stride in bytes)."""
    jobs = np.zeros(len(infos), dtype=FRAME_JOB_DT)
    fill_jobs(jobs, infos)
    jobs["coef"] = coef.data_ptr() + 2 * offs[:-1]
    jobs["planes"] = planes.data_ptr() + offs[:-1]
    jobs["dst"] = [t[0] for t in targets]
    jobs["dst_stride"] = [t[1] for t in targets]
    return jobs


def check_sub_bits(sub_bits):
    """The subsequence length of the device Huffman decoder as an int (None: the library's default), or ValueError."""
    bits = SUB_BITS_DEFAULT if sub_bits is None else int(sub_bits)
    if bits < 32 or bits % 32 or bits > 1 << 20:
        raise ValueError("sub_bits must be a multiple of 32 in 32 .. 2^20 (got %r)" % (sub_bits,))
    return bits


def check_dst(dst, n, device):
    """decode_into's destination: uint8 [n, H, W, 3] on `device`, unit stride over the channels, 3 over x, any row stride
    >= 3 * W and any frame stride.  Returns (H, W), or ValueError."""
    if (not isinstance(dst, torch.Tensor) or dst.device != device or dst.dtype != torch.uint8 or dst.dim() != 4
            or dst.shape[3] != 3 or dst.shape[0] != n):
        raise ValueError("dst must be a uint8 tensor [%d, H, W, 3] on %s" % (n, device))
    _, H, W, _ = dst.shape
    if dst.stride(3) != 1 or dst.stride(2) != 3 or dst.stride(1) < 3 * W or dst.stride(0) < 0:
        raise ValueError("dst needs strides (any, >= 3 * W, 3, 1), got %s" % (tuple(dst.stride()),))
    return H, W


def status_text(rc):
    """What a nonzero per-frame status of the device Huffman decoder says."""
    if rc == _jpeglib.ECORRUPT:
        return "corrupt JPEG: the device Huffman decoder refused the scan"
    if rc == _jpeglib.EINDEX:
        return "the sync index does not describe the scan it was used with"
    return "the scan job does not fit its sizes or its workspace"


def read_header(data):
    """(width, height) of a JPEG file from its headers, without decoding; X3DHipError if the decoder does not take it."""
    rc, info, msg = _jpeglib.parse(bytes(data))
    if rc:
        raise X3DHipError("libx3djpeg: error %d: %s" % (rc, msg))
    return int(info["width"][0]), int(info["height"][0])


class HostStages:
    """The host work on a batch of files that needs no device: the thread pool, the header parse and the scan preparation
    for the device Huffman decoder, into a reused staging buffer of plain host memory.  A FrameStore fills itself through
    one; JpegDecoder is built on it.  threads is never sized from the machine's core count."""

    def __init__(self, threads, sub_bits):
        self.sub_bits = check_sub_bits(sub_bits)
        self.threads = max(1, min(16, int(threads)))
        _jpeglib.lib()
        self._pool = ThreadPoolExecutor(max_workers=self.threads) if self.threads > 1 else None
        self._buffers = {}          # dtype -> reused host buffer: scans and segment tables (uint8), coefficients (int16)

    def _chunks(self, fn, n):
        """fn(lo, hi) over [0, n) cut into one contiguous range per thread; the results in order.  A range per thread,
        not a task per frame: the pool's bookkeeping holds the GIL, the library calls do not."""
        k = min(self.threads, n)
        cuts = [n * t // k for t in range(k + 1)]
        if self._pool is None or k == 1:
            return fn(0, n)
        return [r for part in self._pool.map(fn, cuts[:-1], cuts[1:]) for r in part]

    @staticmethod
    def _fail(i, rc):                                       # on the thread that made the call: the message is thread-local
        return "JPEG frame %d of the batch: libx3djpeg error %d: %s" % (i, rc, _jpeglib.last_error())

    def _parse_stage(self, frames):
        """Headers of all frames -> infos.  Raises X3DHipError naming the first frame that fails."""
        n = len(frames)
        L = _jpeglib.lib()
        infos = np.zeros(n, dtype=INFO_DT)
        info_ptr, info_size = infos.ctypes.data, INFO_DT.itemsize
        fail = self._fail

        def parse(lo, hi):
            out = []
            for i in range(lo, hi):
                rc = L.x3djpeg_parse(frames[i], len(frames[i]), info_ptr + i * info_size)
                out.append(fail(i, rc) if rc else None)
            return out

        for msg in self._chunks(parse, n):
            if msg:
                raise X3DHipError(msg)
        return infos

    def _alloc(self, n, dtype):
        return torch.empty(n, dtype=dtype)

    def _staging(self, total, dtype=torch.uint8):
        """The reused host buffer of `dtype`, at least `total` elements: its user has read it before the next call."""
        buf = self._buffers.get(dtype)
        if buf is None or buf.numel() < total:
            buf = self._buffers[dtype] = self._alloc(max(total, 1 << 16), dtype)
        return buf

    def _prepare_stage(self, frames):
        """Headers and scan preparation of all frames for the device decoder.  Returns (infos, uint8 host tensor: per
        frame its unstuffed scan with padding, then per frame its segment table; byte offsets of the scans, of the tables;
        scan bytes, segments and workspace bytes per frame).  Raises X3DHipError naming the first frame that fails."""
        n = len(frames)
        L = _jpeglib.lib()
        infos = self._parse_stage(frames)
        info_ptr, info_size = infos.ctypes.data, INFO_DT.itemsize
        fail, sub_bits = self._fail, self.sub_bits
        lens = np.array([len(f) for f in frames], dtype=np.int64)
        cap = (lens - infos["scan_off"] + SCAN_PAD + 15) & ~15
        mcus, ri = infos["mcus_x"].astype(np.int64) * infos["mcus_y"], infos["restart_interval"].astype(np.int64)
        nseg = np.where(ri > 0, -(-mcus // np.maximum(ri, 1)), 1)
        scan_at = np.concatenate([[0], np.cumsum(cap)])
        seg_at = scan_at[-1] + np.concatenate([[0], np.cumsum(nseg * SCAN_SEG_DT.itemsize)])
        total = int(seg_at[-1])
        staging = self._staging(total)
        base = staging.data_ptr()
        written = np.zeros((n, 2), dtype=np.uint64)         # scan bytes, segments
        ws = np.zeros(n, dtype=np.int64)
        out_ptr = written.ctypes.data
        scan_p, seg_p = (base + scan_at[:-1]).tolist(), (base + seg_at[:-1]).tolist()
        cap_l, nseg_l = cap.tolist(), nseg.tolist()

        def prepare(lo, hi):
            out = []
            for i in range(lo, hi):
                rc = L.x3djpeg_scan_prepare(frames[i], len(frames[i]), info_ptr + i * info_size, scan_p[i], cap_l[i],
                                            seg_p[i], nseg_l[i], out_ptr + 16 * i, out_ptr + 16 * i + 8)
                if rc == 0:
                    ws[i] = L.x3djpeg_entropy_workspace_bytes(int(written[i, 0]), nseg_l[i], sub_bits)
                out.append(fail(i, rc) if rc else None)
            return out

        for msg in self._chunks(prepare, n):
            if msg:
                raise X3DHipError(msg)
        return infos, staging[:total], scan_at, seg_at, written[:, 0].astype(np.int64), nseg, ws


class JpegDecoder(HostStages):
    """entropy: "host" (Huffman decoding in the thread pool) or "device" (on the GPU).  For "device": sub_bits is the
    length of a subsequence in bits, a multiple of 32 (None: the library's default); check=False skips the read of the
    per-frame status after a batch and leaves it, an int32 tensor on the device, in last_status."""

    def __init__(self, device, threads=8, entropy="host", sub_bits=None, check=True):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("JpegDecoder needs a GPU device (got %s)" % self.device)
        if entropy not in ("host", "device"):
            raise ValueError("entropy must be 'host' or 'device' (got %r)" % (entropy,))
        self.entropy = entropy
        super().__init__(threads, sub_bits)
        self.check = bool(check)
        self.last_status = None
        self.last_bytes_copied = 0  # of the last batch's host-to-device copy of coefficients or scan bytes
        self._copied = None         # event after the last H2D copy out of a staging buffer

    def _alloc(self, n, dtype):
        return torch.empty(n, dtype=dtype).pin_memory()

    def _staging(self, total, dtype=torch.uint8):
        """Pinned, and only once the previous batch's copy has left it."""
        if self._copied is not None:
            self._copied.synchronize()
        return super()._staging(total, dtype)

    def _host_stage(self, frames):
        """Headers and Huffman decoding of all frames.  Returns (infos, pinned int16 tensor holding the coefficients of
        the frames back to back, element offsets).  Raises X3DHipError naming the first frame that fails."""
        n = len(frames)
        L = _jpeglib.lib()
        infos = self._parse_stage(frames)
        info_ptr, info_size = infos.ctypes.data, INFO_DT.itemsize
        fail = self._fail
        counts = infos["coef_count"].astype(np.int64)
        offs = np.concatenate([[0], np.cumsum(counts)])
        total = int(offs[-1])
        pinned = self._staging(total, torch.int16)
        base = pinned.data_ptr()
        at, size = (base + 2 * offs[:-1]).tolist(), (2 * counts).tolist()

        def decode(lo, hi):
            out = []
            for i in range(lo, hi):
                rc = L.x3djpeg_entropy_decode(frames[i], len(frames[i]), info_ptr + i * info_size, at[i], size[i])
                out.append(fail(i, rc) if rc else None)
            return out

        for msg in self._chunks(decode, n):
            if msg:
                raise X3DHipError(msg)
        return infos, pinned[:total], offs

    def _stage_device(self, frames, dsts):
        """Everything of a device-path batch short of the launches: the host work, the copy of the scan bytes, the
        buffers and both job tables.  Returns a dict: n, sub_bits, scan_jobs / frame_jobs (device pointers), workspace,
        status, coef (tensors), ws_off (each frame's byte offset in the workspace), max_blocks, max_w, max_h, keep (tensors
        the launches read)."""
        n = len(frames)
        infos, host_bytes, scan_at, seg_at, scan_bytes, nseg, ws_need = self._prepare_stage(frames)
        targets = dsts(infos)
        counts = infos["coef_count"].astype(np.int64)
        offs = np.concatenate([[0], np.cumsum(counts)])
        total = int(offs[-1])
        ws_off = np.concatenate([[0], np.cumsum(ws_need)])
        with torch.cuda.device(self.device):
            dev_bytes = torch.empty(host_bytes.numel(), dtype=torch.uint8, device=self.device)
            dev_bytes.copy_(host_bytes, non_blocking=True)
            self._copied = torch.cuda.Event()
            self._copied.record()
            self.last_bytes_copied = int(host_bytes.numel())
            coef = torch.empty(total, dtype=torch.int16, device=self.device)
            planes = torch.empty(total, dtype=torch.uint8, device=self.device)
            workspace = torch.empty(int(ws_off[-1]), dtype=torch.uint8, device=self.device)
            status = torch.empty(n, dtype=torch.int32, device=self.device)
            jobs = frame_jobs(infos, offs, coef, planes, targets)
            sj = np.zeros(n, dtype=SCAN_JOB_DT)
            _jpeglib.fill_scan_jobs(sj, infos)
            sj["scan"] = dev_bytes.data_ptr() + scan_at[:-1]
            sj["segs"] = dev_bytes.data_ptr() + seg_at[:-1]
            sj["coef"] = jobs["coef"]
            sj["ws_off"], sj["ws_bytes"] = ws_off[:-1], ws_need
            sj["scan_bytes"], sj["nseg"] = scan_bytes, nseg
            jd = torch.from_numpy(np.concatenate([jobs.view(np.uint8), sj.view(np.uint8)])).to(self.device)
        return dict(n=n, sub_bits=self.sub_bits, frame_jobs=jd.data_ptr(), scan_jobs=jd.data_ptr() + jobs.nbytes,
                    workspace=workspace, ws_off=ws_off[:-1], status=status, coef=coef, max_blocks=int(infos["nblocks"].max()),
                    max_w=int(infos["width"].max()), max_h=int(infos["height"].max()),
                    keep=(dev_bytes, coef, planes, workspace, status, jd))

    @staticmethod
    def launch_device(b):
        """The three launches of a staged device-path batch on the current stream (capturable: nothing else happens)."""
        L = _jpeglib.lib()
        _jpeglib.check(L.x3djpeg_entropy_decode_batch(b["scan_jobs"], b["n"], b["sub_bits"], b["workspace"].data_ptr(),
                                                      b["workspace"].numel(), b["status"].data_ptr(), stream()))
        _jpeglib.check(L.x3djpeg_decode_batch(b["frame_jobs"], b["n"], b["max_blocks"], b["max_w"], b["max_h"], stream()))

    def _run_device(self, frames, dsts):
        b = self._stage_device(frames, dsts)
        with torch.cuda.device(self.device):
            self.launch_device(b)
            cur = torch.cuda.current_stream()
            for t in b["keep"]:
                t.record_stream(cur)
            self.last_status = b["status"]
            if self.check:
                st = b["status"].cpu().numpy()              # the one synchronisation of the batch
                bad = np.flatnonzero(st)
                if bad.size:
                    i = int(bad[0])
                    raise X3DHipError("JPEG frame %d of the batch: libx3djpeg error %d: %s" % (
                        i, int(st[i]), status_text(st[i])))

    def _run(self, frames, dsts):
        """dsts(infos) -> per frame (data_ptr, row stride in bytes, tensor to keep alive), called after the host stage
        succeeded for every frame."""
        frames = [f if isinstance(f, bytes) else bytes(f) for f in frames]
        n = len(frames)
        if n < 1 or n > 65535:
            raise ValueError("a batch holds 1 .. 65535 frames (got %d)" % n)
        if self.entropy == "device":
            return self._run_device(frames, dsts)
        infos, coef_host, offs = self._host_stage(frames)
        targets = dsts(infos)
        total = int(offs[-1])
        with torch.cuda.device(self.device):
            coef = torch.empty(total, dtype=torch.int16, device=self.device)
            coef.copy_(coef_host, non_blocking=True)
            self.last_bytes_copied = 2 * total
            self._copied = torch.cuda.Event()
            self._copied.record()
            planes = torch.empty(total, dtype=torch.uint8, device=self.device)
            jobs = frame_jobs(infos, offs, coef, planes, targets)
            jd = torch.from_numpy(jobs.view(np.uint8)).to(self.device)
            _jpeglib.check(_jpeglib.lib().x3djpeg_decode_batch(
                jd.data_ptr(), n, int(infos["nblocks"].max()), int(infos["width"].max()), int(infos["height"].max()),
                stream()))
            cur = torch.cuda.current_stream()
            for t in (coef, planes, jd):
                t.record_stream(cur)

    def decode(self, frames, out=None):
        """frames: list of bytes.  Returns a list of uint8 [H, W, 3] tensors on the device; out: tensors to write into
        (contiguous, of each frame's size)."""
        res = []

        def dsts(infos):
            t = []
            for i in range(len(infos)):
                H, W = int(infos["height"][i]), int(infos["width"][i])
                if out is not None:
                    o = out[i]
                    if (not isinstance(o, torch.Tensor) or o.device != self.device or o.dtype != torch.uint8
                            or tuple(o.shape) != (H, W, 3) or not o.is_contiguous()):
                        raise ValueError("out[%d] must be a contiguous uint8 tensor (%d, %d, 3) on %s" % (i, H, W, self.device))
                else:
                    o = torch.empty((H, W, 3), dtype=torch.uint8, device=self.device)
                res.append(o)
                t.append((o.data_ptr(), 3 * W))
            return t

        if out is not None and len(out) != len(frames):
            raise ValueError("out must hold one tensor per frame")
        self._run(frames, dsts)
        return res

    def decode_into(self, frames, dst):
        """frames: n files of one size; dst: uint8 [n, H, W, 3] on the device, unit stride over the channels, 3 over x, any
        row stride >= 3 * W and any frame stride.  ValueError when a frame's size is not dst's."""
        n = len(frames)
        H, W = check_dst(dst, n, self.device)

        def dsts(infos):
            for i in range(n):
                if int(infos["height"][i]) != H or int(infos["width"][i]) != W:
                    raise ValueError("frame %d is %d x %d, dst holds %d x %d frames" % (
                        i, int(infos["width"][i]), int(infos["height"][i]), W, H))
            p, s0 = dst.data_ptr(), dst.stride(0)
            return [(p + i * s0, dst.stride(1)) for i in range(n)]

        self._run(frames, dsts)
        return dst
