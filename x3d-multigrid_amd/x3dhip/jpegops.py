"""JPEG frames -> uint8 [H, W, 3] tensors in HBM over the C ABI of include/x3djpeg.h, bit-exact with Pillow.

The serial stage (headers, Huffman decoding) runs on the host in a thread pool (ctypes releases the GIL) into one reused
pinned coefficient buffer; one asynchronous copy, one job table and two kernel launches per batch go on the current
stream, whatever the number of frames and however they differ in size or subsampling.  There is no fallback: a frame the
library does not take raises X3DHipError and nothing is launched for its batch.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _jpeglib
from ._jpeglib import FRAME_JOB_DT, INFO_DT
from ._lib import X3DHipError, stream

_JOB_FIELDS = ("width", "height", "ncomp", "hmax", "vmax", "nblocks", "blocks_w", "blocks_h", "cw", "ch", "block_start")


def fill_jobs(jobs, infos):
    """The fields of X3DJpegFrameJob that come from X3DJpegInfo (everything but the four pointers / strides)."""
    for f in _JOB_FIELDS:
        jobs[f] = infos[f]
    tq = infos["comp_tq"]
    jobs["qt"] = np.take_along_axis(infos["qt"], tq[:, :, None].astype(np.int64), axis=1)


def read_header(data):
    """(width, height) of a JPEG file from its headers, without decoding; X3DHipError if the decoder does not take it."""
    rc, info, msg = _jpeglib.parse(bytes(data))
    if rc:
        raise X3DHipError("libx3djpeg: error %d: %s" % (rc, msg))
    return int(info["width"][0]), int(info["height"][0])


class JpegDecoder:
    def __init__(self, device, threads=8):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("JpegDecoder needs a GPU device (got %s)" % self.device)
        self.threads = max(1, min(16, int(threads)))       # never sized from the machine's core count
        _jpeglib.lib()
        self._pool = ThreadPoolExecutor(max_workers=self.threads) if self.threads > 1 else None
        self._pinned = None
        self._copied = None         # event after the last H2D copy out of the pinned buffer

    def _chunks(self, fn, n):
        """fn(lo, hi) over [0, n) cut into one contiguous range per thread; the results in order.  A range per thread,
        not a task per frame: the pool's bookkeeping holds the GIL, the library calls do not."""
        k = min(self.threads, n)
        cuts = [n * t // k for t in range(k + 1)]
        if self._pool is None or k == 1:
            return fn(0, n)
        return [r for part in self._pool.map(fn, cuts[:-1], cuts[1:]) for r in part]

    def _host_stage(self, frames):
        """Headers and Huffman decoding of all frames.  Returns (infos, pinned int16 tensor holding the coefficients of
        the frames back to back, element offsets).  Raises X3DHipError naming the first frame that fails."""
        n = len(frames)
        L = _jpeglib.lib()
        infos = np.zeros(n, dtype=INFO_DT)
        info_ptr, info_size = infos.ctypes.data, INFO_DT.itemsize

        def fail(i, rc):                                    # on the thread that made the call: the message is thread-local
            return "JPEG frame %d of the batch: libx3djpeg error %d: %s" % (i, rc, _jpeglib.last_error())

        def parse(lo, hi):
            out = []
            for i in range(lo, hi):
                rc = L.x3djpeg_parse(frames[i], len(frames[i]), info_ptr + i * info_size)
                out.append(fail(i, rc) if rc else None)
            return out

        for msg in self._chunks(parse, n):
            if msg:
                raise X3DHipError(msg)
        counts = infos["coef_count"].astype(np.int64)
        offs = np.concatenate([[0], np.cumsum(counts)])
        total = int(offs[-1])
        if self._copied is not None:
            self._copied.synchronize()                      # the previous batch's copy has left the pinned buffer
        if self._pinned is None or self._pinned.numel() < total:
            self._pinned = torch.empty(max(total, 1 << 16), dtype=torch.int16).pin_memory()
        base = self._pinned.data_ptr()
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
        return infos, self._pinned[:total], offs

    def _run(self, frames, dsts):
        """dsts(infos) -> per frame (data_ptr, row stride in bytes, tensor to keep alive), called after the host stage
        succeeded for every frame."""
        frames = [f if isinstance(f, bytes) else bytes(f) for f in frames]
        n = len(frames)
        if n < 1 or n > 65535:
            raise ValueError("a batch holds 1 .. 65535 frames (got %d)" % n)
        infos, coef_host, offs = self._host_stage(frames)
        targets = dsts(infos)
        total = int(offs[-1])
        with torch.cuda.device(self.device):
            coef = torch.empty(total, dtype=torch.int16, device=self.device)
            coef.copy_(coef_host, non_blocking=True)
            self._copied = torch.cuda.Event()
            self._copied.record()
            planes = torch.empty(total, dtype=torch.uint8, device=self.device)
            jobs = np.zeros(n, dtype=FRAME_JOB_DT)
            fill_jobs(jobs, infos)
            jobs["coef"] = coef.data_ptr() + 2 * offs[:-1]
            jobs["planes"] = planes.data_ptr() + offs[:-1]
            jobs["dst"] = [t[0] for t in targets]
            jobs["dst_stride"] = [t[1] for t in targets]
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
        if (not isinstance(dst, torch.Tensor) or dst.device != self.device or dst.dtype != torch.uint8 or dst.dim() != 4
                or dst.shape[3] != 3 or dst.shape[0] != len(frames)):
            raise ValueError("dst must be a uint8 tensor [%d, H, W, 3] on %s" % (len(frames), self.device))
        n, H, W, _ = dst.shape
        if dst.stride(3) != 1 or dst.stride(2) != 3 or dst.stride(1) < 3 * W or dst.stride(0) < 0:
            raise ValueError("dst needs strides (any, >= 3 * W, 3, 1), got %s" % (tuple(dst.stride()),))

        def dsts(infos):
            for i in range(n):
                if int(infos["height"][i]) != H or int(infos["width"][i]) != W:
                    raise ValueError("frame %d is %d x %d, dst holds %d x %d frames" % (
                        i, int(infos["width"][i]), int(infos["height"][i]), W, H))
            p, s0 = dst.data_ptr(), dst.stride(0)
            return [(p + i * s0, dst.stride(1)) for i in range(n)]

        self._run(frames, dsts)
        return dst
