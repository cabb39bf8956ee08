"""Tensor-level wrappers over the step C ABI (include/x3dstep.h), in the style of evalops.py and dataops.py.

Sizes, dtypes and devices are checked here, on the host, before anything is launched.  Every launch goes to the current
stream.  There is no fallback: `observe` on a CPU tensor raises; `observe_host` is the library's CPU twin on numpy arrays
(the tests' second implementation of the same arithmetic, never a substitute on the training path).
"""
import numpy as np
import torch

from . import _steplib
from ._lib import ptr, stream
from ._steplib import HEADER_DT, ITEM_DT, STATE_WORDS, check


def _np_ptr(a):
    return a.ctypes.data


def segment_table(lengths):
    """seg_off int64 [S + 1] of tensors with these element counts, in order."""
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if lengths.size < 1 or np.any(lengths < 1):
        raise ValueError("segment_table: needs at least one tensor and at least one element in each")
    return np.concatenate([np.zeros(1, np.int64), np.cumsum(lengths)])


def build_items(seg_off):
    """(items [nitems] ITEM_DT, seg_item int32 [S + 1]) of a segment table: x3dstep_build_items."""
    seg_off = np.ascontiguousarray(seg_off, dtype=np.int64)
    if seg_off.ndim != 1 or seg_off.size < 2:
        raise ValueError("build_items: seg_off must be a flat array of S + 1 >= 2 offsets")
    S = seg_off.size - 1
    L = _steplib.lib()
    n = check(L.x3dstep_item_count(_np_ptr(seg_off), S))
    items = np.zeros(n, dtype=ITEM_DT)
    seg_item = np.zeros(S + 1, dtype=np.int32)
    got = check(L.x3dstep_build_items(_np_ptr(seg_off), S, _np_ptr(items), n, _np_ptr(seg_item)))
    assert got == n
    return items, seg_item


def record_bytes(S):
    b = _steplib.lib().x3dstep_record_bytes(int(S))
    if b == 0:
        raise ValueError("record_bytes: S = %d outside 1 .. %d" % (S, _steplib.MAX_SEGMENTS))
    return int(b)


def workspace_bytes(nitems):
    b = _steplib.lib().x3dstep_workspace_bytes(int(nitems))
    if b == 0:
        raise ValueError("workspace_bytes: %d items outside 1 .. %d" % (nitems, _steplib.MAX_ITEMS))
    return int(b)


def new_state():
    """The state before the first step: counter 0, no bad step, no bad tensor."""
    st = np.zeros(STATE_WORDS, dtype=np.int64)
    st[_steplib.S_BAD_STEP] = st[_steplib.S_BAD_SEG] = -1
    return st


class StepTables:
    """The tables of one flat buffer: the segment table, its items and seg_item on the host, and (device given) on the
    device as int64 / uint8 / int32 tensors."""

    def __init__(self, seg_off, device=None):
        self.seg_off = np.ascontiguousarray(seg_off, dtype=np.int64)
        self.items, self.seg_item = build_items(self.seg_off)
        self.S = self.seg_off.size - 1
        self.n = int(self.seg_off[-1])
        self.nitems = int(self.items.size)
        self.record_bytes = record_bytes(self.S)
        self.workspace_bytes = workspace_bytes(self.nitems)
        self.device = None if device is None else torch.device(device)
        if self.device is not None:
            self.d_seg_off = torch.from_numpy(self.seg_off).to(self.device)
            self.d_items = torch.from_numpy(self.items.view(np.uint8).copy()).to(self.device)
            self.d_seg_item = torch.from_numpy(self.seg_item).to(self.device)


def observe(g, tables, workspace, state, ring, R, max_norm=0.0, inv_world=1.0):
    """The three launches on the current stream (two when max_norm <= 0): statistics of g into slot state[0] mod R of
    `ring`, then g *= the coefficient.  g float32 [n]; workspace / ring uint8; state int64 [STATE_WORDS]; all on the
    tables' device."""
    dev = tables.device
    if dev is None or dev.type != "cuda":
        raise ValueError("observe: the tables are not on a GPU (observe_host is the CPU twin)")
    if g.device != dev or g.dtype != torch.float32 or g.dim() != 1 or not g.is_contiguous() or g.numel() != tables.n:
        raise ValueError("observe: g must be a contiguous float32 [%d] on %s" % (tables.n, dev))
    if state.device != dev or state.dtype != torch.int64 or state.numel() != STATE_WORDS or not state.is_contiguous():
        raise ValueError("observe: state must be int64 [%d] on %s" % (STATE_WORDS, dev))
    R = int(R)
    for name, t, need in (("workspace", workspace, tables.workspace_bytes), ("ring", ring, R * tables.record_bytes)):
        if t.device != dev or t.dtype != torch.uint8 or not t.is_contiguous() or t.numel() < need or R < 1:
            raise ValueError("observe: %s must be a contiguous uint8 tensor of at least %d bytes on %s" % (name, need, dev))
    check(_steplib.lib().x3dstep_observe(ptr(g), tables.n, ptr(tables.d_seg_off), tables.S, ptr(tables.d_items),
                                         ptr(tables.d_seg_item), tables.nitems, ptr(workspace), ptr(state), ptr(ring), R,
                                         float(max_norm), float(inv_world), stream()))


def observe_host(g, tables, workspace, state, ring, R, max_norm=0.0, inv_world=1.0):
    """The CPU twin on numpy arrays (g float32 [n] is scaled in place; state int64; workspace / ring uint8)."""
    R = int(R)
    if g.dtype != np.float32 or g.ndim != 1 or g.size != tables.n or not g.flags.c_contiguous or not g.flags.writeable:
        raise ValueError("observe_host: g must be a writeable contiguous float32 [%d]" % tables.n)
    if state.dtype != np.int64 or state.size != STATE_WORDS or not state.flags.c_contiguous:
        raise ValueError("observe_host: state must be int64 [%d]" % STATE_WORDS)
    for name, a, need in (("workspace", workspace, tables.workspace_bytes), ("ring", ring, R * tables.record_bytes)):
        if a.dtype != np.uint8 or not a.flags.c_contiguous or a.size < need or R < 1:
            raise ValueError("observe_host: %s must be a contiguous uint8 array of at least %d bytes" % (name, need))
    check(_steplib.lib().x3dstep_observe_host(_np_ptr(g), tables.n, _np_ptr(tables.seg_off), tables.S,
                                              _np_ptr(tables.items), _np_ptr(tables.seg_item), tables.nitems,
                                              _np_ptr(workspace), _np_ptr(state), _np_ptr(ring), R, float(max_norm),
                                              float(inv_world)))


def aligned_bytes(nbytes, align=16):
    """A zeroed uint8 numpy array of nbytes whose address is a multiple of `align` (the tables of the twin are 8-byte
    aligned, g 16-byte aligned for the vector loads)."""
    raw = np.zeros(nbytes + align, dtype=np.uint8)
    off = (-raw.ctypes.data) % align
    return raw[off:off + nbytes]


def parse_record(rec, S):
    """One record (uint8 [record_bytes]) -> (header (a HEADER_DT scalar), sumsq f8 [S], hash u8 [S], nonfinite i4 [S])."""
    rec = np.ascontiguousarray(rec, dtype=np.uint8)
    hb = HEADER_DT.itemsize
    head = rec[:hb].view(HEADER_DT)[0]
    sumsq = rec[hb:hb + 8 * S].view("<f8")
    hsh = rec[hb + 8 * S:hb + 16 * S].view("<u8")
    nf = rec[hb + 16 * S:hb + 20 * S].view("<i4")
    return head, sumsq, hsh, nf


def ring_steps(state, R):
    """The steps whose records the ring still holds, oldest first, and their slots."""
    count = int(state[_steplib.S_STEP])
    steps = list(range(max(0, count - int(R)), count))
    return steps, [s % int(R) for s in steps]
