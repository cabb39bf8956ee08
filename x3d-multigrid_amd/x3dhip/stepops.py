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


def _need_flat(who, name, t, n, dev):
    """`t` must be a contiguous float32 [n] tensor on `dev`."""
    if not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == torch.float32 and t.dim() == 1
            and t.is_contiguous() and t.numel() == n):
        raise ValueError("%s: %s must be a contiguous float32 [%d] on %s" % (who, name, n, dev))


def _need_flat_np(who, name, a, n, writeable=False):
    """... and the numpy form: a contiguous float32 [n] array, writeable where the twin stores to it."""
    if not (isinstance(a, np.ndarray) and a.dtype == np.float32 and a.ndim == 1 and a.size == n and a.flags.c_contiguous
            and (a.flags.writeable or not writeable)):
        raise ValueError("%s: %s must be a %scontiguous float32 [%d]" % (who, name, "writeable " if writeable else "", n))


def _need_state(who, state, dev, optional=False):
    """`state` must be the contiguous int64 [STATE_WORDS] tensor on `dev` (optional: or None)."""
    if state is None and optional:
        return
    if (not isinstance(state, torch.Tensor) or state.device != dev or state.dtype != torch.int64
            or state.numel() != STATE_WORDS or not state.is_contiguous()):
        raise ValueError("%s: state must be int64 [%d] on %s%s" % (who, STATE_WORDS, dev, ", or None" if optional else ""))


def _state_ptr_np(who, state, optional=False):
    """... and the numpy form, which gives the address (None for no state)."""
    if state is None and optional:
        return None
    if (not isinstance(state, np.ndarray) or state.dtype != np.int64 or state.size != STATE_WORDS
            or not state.flags.c_contiguous):
        raise ValueError("%s: state must be int64 [%d]%s" % (who, STATE_WORDS, ", or None" if optional else ""))
    return _np_ptr(state)


def _on_gpu(who, dev, what="tables are"):
    if dev is None or dev.type != "cuda":
        raise ValueError("%s: the %s not on a GPU (%s_host is the CPU twin)" % (who, what, who))
    return dev


def _check_device(who, g, tables, workspace, state, ring, R):
    dev = _on_gpu(who, tables.device)
    _need_flat(who, "g", g, tables.n, dev)
    _need_state(who, state, dev)
    for name, t, need in (("workspace", workspace, tables.workspace_bytes), ("ring", ring, R * tables.record_bytes)):
        if t is None:
            continue
        if t.device != dev or t.dtype != torch.uint8 or not t.is_contiguous() or t.numel() < need or R < 1:
            raise ValueError("%s: %s must be a contiguous uint8 tensor of at least %d bytes on %s" % (who, name, need, dev))


def _check_host(who, g, tables, workspace, state, ring, R, writeable=True):
    _need_flat_np(who, "g", g, tables.n, writeable)
    _state_ptr_np(who, state)
    for name, a, need in (("workspace", workspace, tables.workspace_bytes), ("ring", ring, R * tables.record_bytes)):
        if a is None:
            continue
        if a.dtype != np.uint8 or not a.flags.c_contiguous or a.size < need or R < 1:
            raise ValueError("%s: %s must be a contiguous uint8 array of at least %d bytes" % (who, name, need))


def observe(g, tables, workspace, state, ring, R, max_norm=0.0, inv_world=1.0):
    """The three launches on the current stream (two when max_norm <= 0): statistics of g into slot state[0] mod R of
    `ring`, then g *= the coefficient.  g float32 [n]; workspace / ring uint8; state int64 [STATE_WORDS]; all on the
    tables' device."""
    R = int(R)
    _check_device("observe", g, tables, workspace, state, ring, R)
    check(_steplib.lib().x3dstep_observe(ptr(g), tables.n, ptr(tables.d_seg_off), tables.S, ptr(tables.d_items),
                                         ptr(tables.d_seg_item), tables.nitems, ptr(workspace), ptr(state), ptr(ring), R,
                                         float(max_norm), float(inv_world), stream()))


def measure(g, tables, workspace, state, ring, R, max_norm=0.0, inv_world=1.0):
    """The first two launches of `observe`: the record, the norm and the coefficient for max_norm; g is only read."""
    R = int(R)
    _check_device("measure", g, tables, workspace, state, ring, R)
    check(_steplib.lib().x3dstep_measure(ptr(g), tables.n, ptr(tables.d_seg_off), tables.S, ptr(tables.d_items),
                                         ptr(tables.d_seg_item), tables.nitems, ptr(workspace), ptr(state), ptr(ring), R,
                                         float(max_norm), float(inv_world), stream()))


def observe_host(g, tables, workspace, state, ring, R, max_norm=0.0, inv_world=1.0):
    """The CPU twin on numpy arrays (g float32 [n] is scaled in place; state int64; workspace / ring uint8)."""
    R = int(R)
    _check_host("observe_host", g, tables, workspace, state, ring, R)
    check(_steplib.lib().x3dstep_observe_host(_np_ptr(g), tables.n, _np_ptr(tables.seg_off), tables.S,
                                              _np_ptr(tables.items), _np_ptr(tables.seg_item), tables.nitems,
                                              _np_ptr(workspace), _np_ptr(state), _np_ptr(ring), R, float(max_norm),
                                              float(inv_world)))


def measure_host(g, tables, workspace, state, ring, R, max_norm=0.0, inv_world=1.0):
    """The CPU twin of `measure` (g is only read)."""
    R = int(R)
    _check_host("measure_host", g, tables, workspace, state, ring, R, writeable=False)
    check(_steplib.lib().x3dstep_measure_host(_np_ptr(g), tables.n, _np_ptr(tables.seg_off), tables.S,
                                              _np_ptr(tables.items), _np_ptr(tables.seg_item), tables.nitems,
                                              _np_ptr(workspace), _np_ptr(state), _np_ptr(ring), R, float(max_norm),
                                              float(inv_world)))


def apply(w, g, m, tables, state, ring, R, lr, momentum=0.9, weight_decay=5e-5, grad_scale=1.0, first=False):
    """The guarded update, one launch on the current stream after `measure` on the same state and ring: nothing is stored
    to w, g or m when the measured gradient had a non-finite element; otherwise ops.sgd_fused's arithmetic on g times the
    measured coefficient (g itself is left unscaled).  Counts the skips in state[S_SKIP / S_SKIPPED / S_RUN]."""
    R = int(R)
    _check_device("apply", g, tables, None, state, ring, R)
    for name, t in (("w", w), ("m", m)):
        _need_flat("apply", name, t, tables.n, g.device)
    check(_steplib.lib().x3dstep_apply(ptr(w), ptr(g), ptr(m), tables.n, ptr(state), ptr(ring), R, tables.S, float(lr),
                                       float(momentum), float(weight_decay), float(grad_scale), 1 if first else 0, stream()))


def apply_host(w, g, m, tables, state, ring, R, lr, momentum=0.9, weight_decay=5e-5, grad_scale=1.0, first=False):
    """The CPU twin of `apply` on numpy arrays (w and m are updated in place)."""
    R = int(R)
    _check_host("apply_host", g, tables, None, state, ring, R, writeable=False)
    for name, a in (("w", w), ("m", m)):
        _need_flat_np("apply_host", name, a, tables.n, writeable=True)
    check(_steplib.lib().x3dstep_apply_host(_np_ptr(w), _np_ptr(g), _np_ptr(m), tables.n, _np_ptr(state), _np_ptr(ring), R,
                                            tables.S, float(lr), float(momentum), float(weight_decay), float(grad_scale),
                                            1 if first else 0))


def _group_flags(who, momentum, first, nesterov):
    if first not in (0, 1, False, True) or nesterov not in (0, 1, False, True):
        raise ValueError("%s: first and nesterov must be 0 or 1 (got %r, %r)" % (who, first, nesterov))
    if nesterov and not float(momentum) > 0.0:
        raise ValueError("%s: nesterov needs momentum > 0 (got %r)" % (who, momentum))
    return int(first), int(nesterov)


def apply_groups(w, g, m, tables, hyper, state, ring, R, lr, momentum=0.9, weight_decay=5e-5, grad_scale=1.0, first=False,
                 nesterov=False):
    """The grouped update, one launch on the current stream: `apply` with tensor s at the rate lr * hyper[s, 0] and the
    decay weight_decay * hyper[s, 1], and Nesterov momentum when asked (include/x3dstep.h).  hyper: float32 [S, 2] on the
    tables' device (X3DStepHyper [S]: lr_scale, wd_scale).  state: the monitor's int64 [STATE_WORDS] after `measure` on the
    same state and ring, or None: the unguarded form, which reads no state (ring and R are then ignored), takes the
    coefficient 1 and always applies."""
    R = int(R)
    dev = _on_gpu("apply_groups", tables.device)
    for name, t in (("w", w), ("g", g), ("m", m)):
        _need_flat("apply_groups", name, t, tables.n, dev)
    if (not isinstance(hyper, torch.Tensor) or hyper.device != dev or hyper.dtype != torch.float32
            or tuple(hyper.shape) != (tables.S, 2) or not hyper.is_contiguous()):
        raise ValueError("apply_groups: hyper must be a contiguous float32 [%d, 2] on %s" % (tables.S, dev))
    if state is not None:
        _check_device("apply_groups", g, tables, None, state, ring, R)
    first, nesterov = _group_flags("apply_groups", momentum, first, nesterov)
    check(_steplib.lib().x3dstep_apply_groups(ptr(w), ptr(g), ptr(m), tables.n, ptr(tables.d_items), tables.nitems,
                                              ptr(hyper), tables.S, None if state is None else ptr(state),
                                              None if state is None else ptr(ring), R if state is not None else 0,
                                              float(lr), float(momentum), float(weight_decay), float(grad_scale), first,
                                              nesterov, stream()))


def apply_groups_host(w, g, m, tables, hyper, state, ring, R, lr, momentum=0.9, weight_decay=5e-5, grad_scale=1.0,
                      first=False, nesterov=False):
    """The CPU twin of `apply_groups` on numpy arrays (w and m are updated in place; hyper: HYPER_DT [S] or float32
    [S, 2]; state int64 [STATE_WORDS] or None)."""
    R = int(R)
    for name, a, wr in (("w", w, True), ("g", g, False), ("m", m, True)):
        _need_flat_np("apply_groups_host", name, a, tables.n, wr)
    if hyper.dtype == _steplib.HYPER_DT:
        ok = hyper.ndim == 1 and hyper.size == tables.S
    else:
        ok = hyper.dtype == np.float32 and hyper.shape == (tables.S, 2)
    if not ok or not hyper.flags.c_contiguous:
        raise ValueError("apply_groups_host: hyper must be a contiguous HYPER_DT [%d] or float32 [%d, 2]"
                         % (tables.S, tables.S))
    if state is not None:
        _check_host("apply_groups_host", g, tables, None, state, ring, R, writeable=False)
    first, nesterov = _group_flags("apply_groups_host", momentum, first, nesterov)
    check(_steplib.lib().x3dstep_apply_groups_host(_np_ptr(w), _np_ptr(g), _np_ptr(m), tables.n, _np_ptr(tables.items),
                                                   tables.nitems, _np_ptr(hyper), tables.S,
                                                   None if state is None else _np_ptr(state),
                                                   None if state is None else _np_ptr(ring), R if state is not None else 0,
                                                   float(lr), float(momentum), float(weight_decay), float(grad_scale), first,
                                                   nesterov))


def trust_workspace_bytes(nitems):
    b = _steplib.lib().x3dstep_trust_workspace_bytes(int(nitems))
    if b == 0:
        raise ValueError("trust_workspace_bytes: %d items outside 1 .. %d" % (nitems, _steplib.MAX_ITEMS))
    return int(b)


def _need_hyper(who, hyper, S, dev):
    if (not isinstance(hyper, torch.Tensor) or hyper.device != dev or hyper.dtype != torch.float32
            or tuple(hyper.shape) != (S, 2) or not hyper.is_contiguous()):
        raise ValueError("%s: hyper must be a contiguous float32 [%d, 2] on %s" % (who, S, dev))


def _need_hyper_np(who, hyper, S):
    if hyper.dtype == _steplib.HYPER_DT:
        ok = hyper.ndim == 1 and hyper.size == S
    else:
        ok = hyper.dtype == np.float32 and hyper.shape == (S, 2)
    if not ok or not hyper.flags.c_contiguous:
        raise ValueError("%s: hyper must be a contiguous HYPER_DT [%d] or float32 [%d, 2]" % (who, S, S))


def _need_vec(who, name, t, dtype, k, dev):
    if not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == dtype and t.dim() == 1 and t.is_contiguous()
            and t.numel() == k):
        raise ValueError("%s: %s must be a contiguous %s [%d] on %s" % (who, name, dtype, k, dev))


def _need_vec_np(who, name, a, dtype, k, writeable=False):
    if not (isinstance(a, np.ndarray) and a.dtype == dtype and a.ndim == 1 and a.size == k and a.flags.c_contiguous
            and (a.flags.writeable or not writeable)):
        raise ValueError("%s: %s must be a contiguous %s [%d]" % (who, name, np.dtype(dtype).name, k))


def _trust_args(who, eps, clip):
    eps = float(eps)
    if not (np.isfinite(eps) and eps >= 0.0) or clip not in (0, 1, False, True):
        raise ValueError("%s: eps must be finite and >= 0 and clip 0 or 1 (got %r, %r)" % (who, eps, clip))
    return eps, int(clip)


def trust(w, tables, hyper, eta, state, ring, R, workspace, wsumsq, trust_out, lr, weight_decay=5e-5, grad_scale=1.0,
          eps=1e-8, clip=False):
    """The LARS trust ratios, two launches on the current stream after `measure` / `observe` on the same state and ring:
    wsumsq[s] (float64 [S]) the sum of squares of tensor s of w, as `measure` would record it on w, and trust_out[s]
    (float32 [S]) = eta[s] |w_s| / (|g_s| + wd_s |w_s| + eps), with `clip` min(that / lr_s, 1); exactly 1 where eta[s] is 0,
    a norm is 0 or the gradient was not finite (include/x3dstep.h).  eta: float32 [S]; hyper: float32 [S, 2]; workspace:
    uint8, trust_workspace_bytes(nitems); all on the tables' device.  w, the state and the ring are only read."""
    R = int(R)
    dev = _on_gpu("trust", tables.device)
    _check_device("trust", w, tables, None, state, ring, R)
    _need_hyper("trust", hyper, tables.S, dev)
    _need_vec("trust", "eta", eta, torch.float32, tables.S, dev)
    _need_vec("trust", "wsumsq", wsumsq, torch.float64, tables.S, dev)
    _need_vec("trust", "trust_out", trust_out, torch.float32, tables.S, dev)
    need = trust_workspace_bytes(tables.nitems)
    if (not isinstance(workspace, torch.Tensor) or workspace.device != dev or workspace.dtype != torch.uint8
            or not workspace.is_contiguous() or workspace.numel() < need):
        raise ValueError("trust: workspace must be a contiguous uint8 tensor of at least %d bytes on %s" % (need, dev))
    eps, clip = _trust_args("trust", eps, clip)
    check(_steplib.lib().x3dstep_trust(ptr(w), tables.n, ptr(tables.d_items), ptr(tables.d_seg_item), tables.nitems,
                                       ptr(hyper), ptr(eta), tables.S, ptr(state), ptr(ring), R, ptr(workspace), ptr(wsumsq),
                                       ptr(trust_out), float(lr), float(weight_decay), float(grad_scale), eps, clip, stream()))


def trust_host(w, tables, hyper, eta, state, ring, R, workspace, wsumsq, trust_out, lr, weight_decay=5e-5, grad_scale=1.0,
               eps=1e-8, clip=False):
    """The CPU twin of `trust` on numpy arrays (wsumsq float64 [S] and trust_out float32 [S] are written)."""
    R = int(R)
    _check_host("trust_host", w, tables, None, state, ring, R, writeable=False)
    _need_hyper_np("trust_host", hyper, tables.S)
    _need_vec_np("trust_host", "eta", eta, np.float32, tables.S)
    _need_vec_np("trust_host", "wsumsq", wsumsq, np.float64, tables.S, True)
    _need_vec_np("trust_host", "trust_out", trust_out, np.float32, tables.S, True)
    need = trust_workspace_bytes(tables.nitems)
    if workspace.dtype != np.uint8 or not workspace.flags.c_contiguous or workspace.size < need:
        raise ValueError("trust_host: workspace must be a contiguous uint8 array of at least %d bytes" % need)
    check(_steplib.lib().x3dstep_trust_host(_np_ptr(w), tables.n, _np_ptr(tables.items), _np_ptr(tables.seg_item),
                                            tables.nitems, _np_ptr(hyper), _np_ptr(eta), tables.S, _np_ptr(state),
                                            _np_ptr(ring), R, _np_ptr(workspace), _np_ptr(wsumsq), _np_ptr(trust_out),
                                            float(lr), float(weight_decay), float(grad_scale), float(eps), int(clip)))


def apply_lars(w, g, m, tables, hyper, trust_in, state, ring, R, lr, momentum=0.9, weight_decay=5e-5, grad_scale=1.0,
               first=False, nesterov=False):
    """`apply_groups` with the decayed gradient of tensor s multiplied by trust_in[s] (float32 [S] on the tables' device,
    what `trust` wrote) before the momentum; every trust 1: the bits of `apply_groups` (include/x3dstep.h)."""
    R = int(R)
    dev = _on_gpu("apply_lars", tables.device)
    for name, t in (("w", w), ("g", g), ("m", m)):
        _need_flat("apply_lars", name, t, tables.n, dev)
    _need_hyper("apply_lars", hyper, tables.S, dev)
    _need_vec("apply_lars", "trust_in", trust_in, torch.float32, tables.S, dev)
    if state is not None:
        _check_device("apply_lars", g, tables, None, state, ring, R)
    first, nesterov = _group_flags("apply_lars", momentum, first, nesterov)
    check(_steplib.lib().x3dstep_apply_lars(ptr(w), ptr(g), ptr(m), tables.n, ptr(tables.d_items), tables.nitems,
                                            ptr(hyper), ptr(trust_in), tables.S, None if state is None else ptr(state),
                                            None if state is None else ptr(ring), R if state is not None else 0,
                                            float(lr), float(momentum), float(weight_decay), float(grad_scale), first,
                                            nesterov, stream()))


def apply_lars_host(w, g, m, tables, hyper, trust_in, state, ring, R, lr, momentum=0.9, weight_decay=5e-5, grad_scale=1.0,
                    first=False, nesterov=False):
    """The CPU twin of `apply_lars` on numpy arrays (w and m are updated in place)."""
    R = int(R)
    for name, a, wr in (("w", w, True), ("g", g, False), ("m", m, True)):
        _need_flat_np("apply_lars_host", name, a, tables.n, wr)
    _need_hyper_np("apply_lars_host", hyper, tables.S)
    _need_vec_np("apply_lars_host", "trust_in", trust_in, np.float32, tables.S)
    if state is not None:
        _check_host("apply_lars_host", g, tables, None, state, ring, R, writeable=False)
    first, nesterov = _group_flags("apply_lars_host", momentum, first, nesterov)
    check(_steplib.lib().x3dstep_apply_lars_host(_np_ptr(w), _np_ptr(g), _np_ptr(m), tables.n, _np_ptr(tables.items),
                                                 tables.nitems, _np_ptr(hyper), _np_ptr(trust_in), tables.S,
                                                 None if state is None else _np_ptr(state),
                                                 None if state is None else _np_ptr(ring), R if state is not None else 0,
                                                 float(lr), float(momentum), float(weight_decay), float(grad_scale), first,
                                                 nesterov))


def lamb_workspace_bytes(nitems):
    b = _steplib.lib().x3dstep_lamb_workspace_bytes(int(nitems))
    if b == 0:
        raise ValueError("lamb_workspace_bytes: %d items outside 1 .. %d" % (nitems, _steplib.MAX_ITEMS))
    return int(b)


def _adam_args(who, betas, eps, decoupled=1):
    b1, b2 = (float(b) for b in betas)
    eps = float(eps)
    if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
        raise ValueError("%s: betas must lie in [0, 1) (got %r)" % (who, (b1, b2)))
    if not (np.isfinite(eps) and eps >= 0.0) or decoupled not in (0, 1, False, True):
        raise ValueError("%s: eps must be finite and >= 0 and decoupled 0 or 1 (got %r, %r)" % (who, eps, decoupled))
    return b1, b2, eps, int(decoupled)


def _state_args(state, ring, R):
    """(state, ring, R) as the C ABI takes them from torch tensors: nulls and 0 for the unguarded form."""
    if state is None:
        return None, None, 0
    return ptr(state), ptr(ring), int(R)


def _state_args_np(state, ring, R):
    if state is None:
        return None, None, 0
    return _np_ptr(state), _np_ptr(ring), int(R)


def _need_bytes(who, name, t, need, dev):
    if (not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != torch.uint8 or not t.is_contiguous()
            or t.numel() < need):
        raise ValueError("%s: %s must be a contiguous uint8 tensor of at least %d bytes on %s" % (who, name, need, dev))


def _need_bytes_np(who, name, a, need):
    if not isinstance(a, np.ndarray) or a.dtype != np.uint8 or not a.flags.c_contiguous or a.size < need:
        raise ValueError("%s: %s must be a contiguous uint8 array of at least %d bytes" % (who, name, need))


def adam(w, g, m, v, tables, hyper, state, ring, R, count, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
         grad_scale=1.0, decoupled=True):
    """Adam (decoupled=False: weight decay as an L2 term of the gradient) or AdamW (decoupled=True), one launch on the
    current stream: torch.optim.Adam / AdamW's single-tensor arithmetic with tensor s at the rate lr * hyper[s, 0] and the
    decay weight_decay * hyper[s, 1] (include/x3dstep.h).  m: exp_avg, v: exp_avg_sq, float32 [n] like w and g.  state: the
    monitor's int64 [STATE_WORDS] after `measure` on the same state and ring (the guarded form: the clipping coefficient
    is applied, a non-finite step stores nothing and is counted), or None.  The bias correction is that of update
    k = count + (state: the updates applied so far, this one included); without a state count is k itself."""
    dev = _on_gpu("adam", tables.device)
    for name, t in (("w", w), ("g", g), ("m", m), ("v", v)):
        _need_flat("adam", name, t, tables.n, dev)
    _need_hyper("adam", hyper, tables.S, dev)
    if state is not None:
        _check_device("adam", g, tables, None, state, ring, int(R))
    b1, b2, eps, decoupled = _adam_args("adam", betas, eps, decoupled)
    check(_steplib.lib().x3dstep_adam(ptr(w), ptr(g), ptr(m), ptr(v), tables.n, ptr(tables.d_items), tables.nitems,
                                      ptr(hyper), tables.S, *_state_args(state, ring, R), int(count), float(lr), b1, b2, eps,
                                      float(weight_decay), float(grad_scale), decoupled, stream()))


def adam_host(w, g, m, v, tables, hyper, state, ring, R, count, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
              grad_scale=1.0, decoupled=True):
    """The CPU twin of `adam` on numpy arrays (w, m and v are updated in place).  The scalars go to the library as they
    are: it is the twin that refuses them."""
    for name, a, wr in (("w", w, True), ("g", g, False), ("m", m, True), ("v", v, True)):
        _need_flat_np("adam_host", name, a, tables.n, wr)
    _need_hyper_np("adam_host", hyper, tables.S)
    if state is not None:
        _check_host("adam_host", g, tables, None, state, ring, int(R), writeable=False)
    check(_steplib.lib().x3dstep_adam_host(_np_ptr(w), _np_ptr(g), _np_ptr(m), _np_ptr(v), tables.n, _np_ptr(tables.items),
                                           tables.nitems, _np_ptr(hyper), tables.S, *_state_args_np(state, ring, R),
                                           int(count), float(lr), float(betas[0]), float(betas[1]), float(eps),
                                           float(weight_decay), float(grad_scale), int(decoupled)))


def lamb_moments(w, g, m, v, tables, hyper, state, ring, R, count, workspace, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0,
                 grad_scale=1.0):
    """Launch 1 of LAMB on the current stream: the new moments into m and v and, per item, the fp64 sums of squares of the
    direction r and of w into workspace (uint8, lamb_workspace_bytes(nitems)).  w and g are only read."""
    dev = _on_gpu("lamb_moments", tables.device)
    for name, t in (("w", w), ("g", g), ("m", m), ("v", v)):
        _need_flat("lamb_moments", name, t, tables.n, dev)
    _need_hyper("lamb_moments", hyper, tables.S, dev)
    _need_bytes("lamb_moments", "workspace", workspace, lamb_workspace_bytes(tables.nitems), dev)
    if state is not None:
        _check_device("lamb_moments", g, tables, None, state, ring, int(R))
    b1, b2, eps, _ = _adam_args("lamb_moments", betas, eps)
    check(_steplib.lib().x3dstep_lamb_moments(ptr(w), ptr(g), ptr(m), ptr(v), tables.n, ptr(tables.d_items), tables.nitems,
                                              ptr(hyper), tables.S, *_state_args(state, ring, R), int(count), b1, b2, eps,
                                              float(weight_decay), float(grad_scale), ptr(workspace), stream()))


def lamb_moments_host(w, g, m, v, tables, hyper, state, ring, R, count, workspace, betas=(0.9, 0.999), eps=1e-6,
                      weight_decay=0.0, grad_scale=1.0):
    """The CPU twin of `lamb_moments` on numpy arrays (m, v and the workspace are written)."""
    for name, a, wr in (("w", w, False), ("g", g, False), ("m", m, True), ("v", v, True)):
        _need_flat_np("lamb_moments_host", name, a, tables.n, wr)
    _need_hyper_np("lamb_moments_host", hyper, tables.S)
    _need_bytes_np("lamb_moments_host", "workspace", workspace, lamb_workspace_bytes(tables.nitems))
    if state is not None:
        _check_host("lamb_moments_host", g, tables, None, state, ring, int(R), writeable=False)
    check(_steplib.lib().x3dstep_lamb_moments_host(_np_ptr(w), _np_ptr(g), _np_ptr(m), _np_ptr(v), tables.n,
                                                   _np_ptr(tables.items), tables.nitems, _np_ptr(hyper), tables.S,
                                                   *_state_args_np(state, ring, R), int(count), float(betas[0]),
                                                   float(betas[1]), float(eps), float(weight_decay), float(grad_scale),
                                                   _np_ptr(workspace)))


def lamb_trust(tables, hyper, adapt, state, ring, R, count, workspace, wsumsq, rsumsq, trust_out):
    """Launch 2 of LAMB: per tensor wsumsq[s] and rsumsq[s] (float64 [S]: the sums of squares of the weights and of the
    direction, as `measure` would record them) and trust_out[s] (float32 [S]) = |w_s| / |r_s|; exactly 1 where adapt[s]
    (uint8 [S]) is 0, a norm is 0 or the gradient was not finite."""
    dev = _on_gpu("lamb_trust", tables.device)
    _need_hyper("lamb_trust", hyper, tables.S, dev)
    _need_vec("lamb_trust", "adapt", adapt, torch.uint8, tables.S, dev)
    _need_vec("lamb_trust", "wsumsq", wsumsq, torch.float64, tables.S, dev)
    _need_vec("lamb_trust", "rsumsq", rsumsq, torch.float64, tables.S, dev)
    _need_vec("lamb_trust", "trust_out", trust_out, torch.float32, tables.S, dev)
    _need_bytes("lamb_trust", "workspace", workspace, lamb_workspace_bytes(tables.nitems), dev)
    if state is not None:
        _need_state("lamb_trust", state, dev)
        _need_bytes("lamb_trust", "ring", ring, int(R) * tables.record_bytes, dev)
    check(_steplib.lib().x3dstep_lamb_trust(ptr(tables.d_seg_item), tables.nitems, ptr(hyper), ptr(adapt), tables.S,
                                            *_state_args(state, ring, R), int(count), ptr(workspace), ptr(wsumsq),
                                            ptr(rsumsq), ptr(trust_out), stream()))


def lamb_trust_host(tables, hyper, adapt, state, ring, R, count, workspace, wsumsq, rsumsq, trust_out, seg_item=None):
    """The CPU twin of `lamb_trust` on numpy arrays (seg_item: another table than the tables' own, for the tests)."""
    _need_hyper_np("lamb_trust_host", hyper, tables.S)
    _need_vec_np("lamb_trust_host", "adapt", adapt, np.uint8, tables.S)
    _need_vec_np("lamb_trust_host", "wsumsq", wsumsq, np.float64, tables.S, True)
    _need_vec_np("lamb_trust_host", "rsumsq", rsumsq, np.float64, tables.S, True)
    _need_vec_np("lamb_trust_host", "trust_out", trust_out, np.float32, tables.S, True)
    _need_bytes_np("lamb_trust_host", "workspace", workspace, lamb_workspace_bytes(tables.nitems))
    if state is not None:
        _state_ptr_np("lamb_trust_host", state)
        _need_bytes_np("lamb_trust_host", "ring", ring, int(R) * tables.record_bytes)
    si = tables.seg_item if seg_item is None else np.ascontiguousarray(seg_item, dtype=np.int32)
    check(_steplib.lib().x3dstep_lamb_trust_host(_np_ptr(si), tables.nitems, _np_ptr(hyper), _np_ptr(adapt), tables.S,
                                                 *_state_args_np(state, ring, R), int(count), _np_ptr(workspace),
                                                 _np_ptr(wsumsq), _np_ptr(rsumsq), _np_ptr(trust_out)))


def lamb_apply(w, m, v, tables, hyper, trust_in, state, ring, R, count, lr, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0):
    """Launch 3 of LAMB: w <- w - (lr_s * trust_in[s]) * r with r recomputed from the stored moments; counts the skips
    in the state as `apply` does.  m and v are only read."""
    dev = _on_gpu("lamb_apply", tables.device)
    for name, t in (("w", w), ("m", m), ("v", v)):
        _need_flat("lamb_apply", name, t, tables.n, dev)
    _need_hyper("lamb_apply", hyper, tables.S, dev)
    _need_vec("lamb_apply", "trust_in", trust_in, torch.float32, tables.S, dev)
    if state is not None:
        _check_device("lamb_apply", w, tables, None, state, ring, int(R))
    b1, b2, eps, _ = _adam_args("lamb_apply", betas, eps)
    check(_steplib.lib().x3dstep_lamb_apply(ptr(w), ptr(m), ptr(v), tables.n, ptr(tables.d_items), tables.nitems, ptr(hyper),
                                            ptr(trust_in), tables.S, *_state_args(state, ring, R), int(count), float(lr), b1,
                                            b2, eps, float(weight_decay), stream()))


def lamb_apply_host(w, m, v, tables, hyper, trust_in, state, ring, R, count, lr, betas=(0.9, 0.999), eps=1e-6,
                    weight_decay=0.0):
    """The CPU twin of `lamb_apply` on numpy arrays (w is updated in place)."""
    for name, a, wr in (("w", w, True), ("m", m, False), ("v", v, False)):
        _need_flat_np("lamb_apply_host", name, a, tables.n, wr)
    _need_hyper_np("lamb_apply_host", hyper, tables.S)
    _need_vec_np("lamb_apply_host", "trust_in", trust_in, np.float32, tables.S)
    if state is not None:
        _check_host("lamb_apply_host", w, tables, None, state, ring, int(R), writeable=False)
    check(_steplib.lib().x3dstep_lamb_apply_host(_np_ptr(w), _np_ptr(m), _np_ptr(v), tables.n, _np_ptr(tables.items),
                                                 tables.nitems, _np_ptr(hyper), _np_ptr(trust_in), tables.S,
                                                 *_state_args_np(state, ring, R), int(count), float(lr), float(betas[0]),
                                                 float(betas[1]), float(eps), float(weight_decay)))


class KeepTable:
    """The table `keep` takes for a list of small float32 buffers: where each lies in the snapshot (every buffer starts on
    a multiple of four elements, so that a 16-byte aligned buffer is copied in 16-byte groups), the item table of the
    snapshot (the cut of build_items) and the snapshot itself.

    buffers: contiguous float32 torch tensors on one GPU, which the table keeps alive -- or, for the CPU twin, numpy arrays
    (`device` None)."""

    def __init__(self, buffers, device=None):
        self.buffers = list(buffers)
        if not self.buffers:
            raise ValueError("KeepTable: no buffers")
        self.device = None if device is None else torch.device(device)
        lens, addrs = [], []
        for b in self.buffers:
            if self.device is None:
                ok = (isinstance(b, np.ndarray) and b.dtype == np.float32 and b.ndim == 1 and b.flags.c_contiguous
                      and b.flags.writeable and b.size >= 1)
                addr = b.ctypes.data if ok else 0
                k = b.size if ok else 0
            else:
                ok = (b.device == self.device and b.dtype == torch.float32 and b.is_contiguous() and b.numel() >= 1)
                addr = b.data_ptr() if ok else 0
                k = b.numel() if ok else 0
            if not ok:
                raise ValueError("KeepTable: every buffer must be a non-empty contiguous float32 %s"
                                 % ("array" if self.device is None else "tensor on %s" % self.device))
            lens.append(k)
            addrs.append(addr)
        padded = [(k + 3) // 4 * 4 for k in lens]
        self.seg_off = segment_table(padded)
        self.items, _ = build_items(self.seg_off)
        self.table = np.zeros(len(lens), dtype=_steplib.KEEP_DT)
        self.table["addr"], self.table["offset"], self.table["len"] = addrs, self.seg_off[:-1], lens
        self.nbuf, self.nitems, self.snap_n = len(lens), int(self.items.size), int(self.seg_off[-1])
        if self.device is None:
            self.snap = aligned_bytes(4 * self.snap_n).view(np.float32)
        else:
            self.snap = torch.zeros(self.snap_n, dtype=torch.float32, device=self.device)
            self.d_table = torch.from_numpy(self.table.view(np.uint8).copy()).to(self.device)
            self.d_items = torch.from_numpy(self.items.view(np.uint8).copy()).to(self.device)


def keep(kt, state, mode):
    """One launch on the current stream: mode KEEP_SAVE copies the table's buffers into its snapshot; KEEP_RESTORE copies
    them back when state[S_SKIP] == 1 (the latest `apply` skipped) and does nothing otherwise."""
    _need_state("keep", state, _on_gpu("keep", kt.device, "table is"))
    if mode not in (_steplib.KEEP_SAVE, _steplib.KEEP_RESTORE):
        raise ValueError("keep: mode must be KEEP_SAVE or KEEP_RESTORE (got %r)" % (mode,))
    check(_steplib.lib().x3dstep_keep(ptr(kt.d_table), kt.nbuf, ptr(kt.d_items), kt.nitems, ptr(kt.snap), kt.snap_n,
                                      ptr(state), int(mode), stream()))


def keep_host(kt, state, mode):
    """The CPU twin of `keep` (a KeepTable of numpy arrays; state int64 [STATE_WORDS])."""
    if kt.device is not None:
        raise ValueError("keep_host: the table is on a GPU")
    check(_steplib.lib().x3dstep_keep_host(_np_ptr(kt.table), kt.nbuf, _np_ptr(kt.items), kt.nitems, _np_ptr(kt.snap),
                                           kt.snap_n, _state_ptr_np("keep_host", state), int(mode)))


def _check_decay(who, decay):
    decay = float(decay)
    if not 0.0 <= decay < 1.0:
        raise ValueError("%s: decay must lie in [0, 1) (got %r)" % (who, decay))
    return decay


def _check_flat_pair(who, a, b, dev):
    for t in (a, b):
        _need_flat(who, "each of the two buffers", t, a.numel(), dev)
    if a.numel() < 1:
        raise ValueError("%s: the buffers are empty" % who)


def _check_keep_device(who, kt, snap):
    dev = _on_gpu(who, kt.device, "table is")
    _need_flat(who, "the snapshot", snap, kt.snap_n, dev)
    return dev


def _check_keep_host(who, kt, snap):
    if kt.device is not None:
        raise ValueError("%s: the table is on a GPU" % who)
    _need_flat_np(who, "the snapshot", snap, kt.snap_n)


def ema(e, w, state, count, decay, warmup=True):
    """One launch on the current stream: e <- d * e + (1 - d) * w for update k = count + (state: the updates applied so far),
    d = min(decay, (1 + k) / (10 + k)) with `warmup`; nothing is stored when the latest `apply` skipped (include/x3dstep.h).
    state: the monitor's int64 [STATE_WORDS], or None (count is then the number of updates, this one included)."""
    dev = e.device
    if dev.type != "cuda":
        raise ValueError("ema: e is not on a GPU (ema_host is the CPU twin)")
    _check_flat_pair("ema", e, w, dev)
    _need_state("ema", state, dev, optional=True)
    check(_steplib.lib().x3dstep_ema(ptr(e), ptr(w), e.numel(), None if state is None else ptr(state), int(count),
                                     _check_decay("ema", decay), 1 if warmup else 0, stream()))


def ema_host(e, w, state, count, decay, warmup=True):
    """The CPU twin of `ema` on numpy arrays (e is updated in place)."""
    for name, a in (("e", e), ("w", w)):
        _need_flat_np("ema_host", name, a, np.size(e))
    check(_steplib.lib().x3dstep_ema_host(_np_ptr(e), _np_ptr(w), e.size, _state_ptr_np("ema_host", state, optional=True),
                                          int(count), float(decay), 1 if warmup else 0))


def ema_keep(kt, esnap, state, count, decay, warmup=True):
    """One launch: the rule of `ema` over the table's live buffers, into `esnap` (float32 [kt.snap_n], laid out as the
    table's own snapshot; the padding past a buffer's length is left alone)."""
    dev = _check_keep_device("ema_keep", kt, esnap)
    _need_state("ema_keep", state, dev, optional=True)
    check(_steplib.lib().x3dstep_ema_keep(ptr(kt.d_table), kt.nbuf, ptr(kt.d_items), kt.nitems, ptr(esnap), kt.snap_n,
                                          None if state is None else ptr(state), int(count),
                                          _check_decay("ema_keep", decay), 1 if warmup else 0, stream()))


def ema_keep_host(kt, esnap, state, count, decay, warmup=True):
    """The CPU twin of `ema_keep` (a KeepTable of numpy arrays)."""
    _check_keep_host("ema_keep_host", kt, esnap)
    check(_steplib.lib().x3dstep_ema_keep_host(_np_ptr(kt.table), kt.nbuf, _np_ptr(kt.items), kt.nitems, _np_ptr(esnap),
                                               kt.snap_n, _state_ptr_np("ema_keep_host", state, optional=True), int(count),
                                               float(decay), 1 if warmup else 0))


def swap(a, b):
    """One launch: exchange two flat float32 buffers in place, bit for bit."""
    dev = a.device
    if dev.type != "cuda":
        raise ValueError("swap: a is not on a GPU (swap_host is the CPU twin)")
    _check_flat_pair("swap", a, b, dev)
    check(_steplib.lib().x3dstep_swap(ptr(a), ptr(b), a.numel(), stream()))


def swap_host(a, b):
    """The CPU twin of `swap`."""
    for name, x in (("a", a), ("b", b)):
        _need_flat_np("swap_host", name, x, np.size(a), writeable=True)
    check(_steplib.lib().x3dstep_swap_host(_np_ptr(a), _np_ptr(b), a.size))


def swap_keep(kt, snap):
    """One launch: exchange the table's live buffers with their ranges of `snap`, in place and bit for bit."""
    _check_keep_device("swap_keep", kt, snap)
    check(_steplib.lib().x3dstep_swap_keep(ptr(kt.d_table), kt.nbuf, ptr(kt.d_items), kt.nitems, ptr(snap), kt.snap_n,
                                           stream()))


def swap_keep_host(kt, snap):
    """The CPU twin of `swap_keep`."""
    _check_keep_host("swap_keep_host", kt, snap)
    check(_steplib.lib().x3dstep_swap_keep_host(_np_ptr(kt.table), kt.nbuf, _np_ptr(kt.items), kt.nitems, _np_ptr(snap),
                                                kt.snap_n))


class PbnTable:
    """The tables `pbn_accum` / `pbn_finish` take, built by the library from a KeepTable whose buffers come in pairs
    (split_bn.running_mean, split_bn.running_var) and the number of splits of each pair: the layer table (where the live
    buffers are, where they lie in the keep table's snapshot, C, S and the layer's first channel in the accumulator array)
    and the work table (runs of at most PBN_RUN channels).  `channels`: the accumulator array has 4 * channels doubles."""

    def __init__(self, kt, splits):
        splits = np.ascontiguousarray(splits, dtype=np.int32).reshape(-1)
        if kt.nbuf != 2 * splits.size or splits.size < 1:
            raise ValueError("PbnTable: %d buffers for %d layers (a mean and a variance buffer each)" % (kt.nbuf, splits.size))
        L = _steplib.lib()
        assert L.x3dstep_pbn_layer_bytes() == _steplib.PBN_LAYER_DT.itemsize
        self.kt, self.device, self.snap_n = kt, kt.device, kt.snap_n
        self.nlayers = int(splits.size)
        self.layers = np.zeros(self.nlayers, dtype=_steplib.PBN_LAYER_DT)
        self.channels = int(check(L.x3dstep_pbn_build_layers(_np_ptr(kt.table), kt.nbuf, _np_ptr(splits), self.nlayers,
                                                             _np_ptr(self.layers))))
        n = check(L.x3dstep_pbn_work_count(_np_ptr(self.layers), self.nlayers))
        self.work = np.zeros(n, dtype=ITEM_DT)
        assert check(L.x3dstep_pbn_build_work(_np_ptr(self.layers), self.nlayers, _np_ptr(self.work), n)) == n
        self.nwork = int(n)
        if self.device is not None:
            self.d_layers = torch.from_numpy(self.layers.view(np.uint8).copy()).to(self.device)
            self.d_work = torch.from_numpy(self.work.view(np.uint8).copy()).to(self.device)

    def new_acc(self, W=1):
        """Zeroed accumulators of W ranks: float64 [W * 4 * channels] (a torch tensor on the table's device, or numpy)."""
        n = int(W) * _steplib.PBN_ACC_DOUBLES * self.channels
        if self.device is None:
            return aligned_bytes(8 * n).view(np.float64)
        return torch.zeros(n, dtype=torch.float64, device=self.device)


def _check_pbn_device(who, pt, acc, W):
    dev = _on_gpu(who, pt.device, "table is")
    need = int(W) * _steplib.PBN_ACC_DOUBLES * pt.channels
    if (not isinstance(acc, torch.Tensor) or acc.device != dev or acc.dtype != torch.float64 or acc.dim() != 1
            or not acc.is_contiguous() or acc.numel() != need or W < 1):
        raise ValueError("%s: the accumulators must be a contiguous float64 [%d] on %s" % (who, need, dev))
    return dev


def _check_pbn_host(who, pt, acc, W):
    if pt.device is not None:
        raise ValueError("%s: the table is on a GPU" % who)
    need = int(W) * _steplib.PBN_ACC_DOUBLES * pt.channels
    if acc.dtype != np.float64 or acc.ndim != 1 or acc.size != need or not acc.flags.c_contiguous or W < 1:
        raise ValueError("%s: the accumulators must be a contiguous float64 [%d]" % (who, need))


def pbn_accum(pt, acc):
    """One launch on the current stream: one cell update per split for every channel, from the table's live buffers (which
    a forward pass with BN momentum 1 just wrote) into acc (float64 [4 * channels]: {n, mean, m2, vsum} per channel)."""
    _check_pbn_device("pbn_accum", pt, acc, 1)
    check(_steplib.lib().x3dstep_pbn_accum(ptr(pt.d_layers), pt.nlayers, ptr(pt.d_work), pt.nwork, ptr(acc), stream()))


def pbn_accum_host(pt, acc):
    """The CPU twin of `pbn_accum` (a PbnTable over a KeepTable of numpy arrays)."""
    _check_pbn_host("pbn_accum_host", pt, acc, 1)
    check(_steplib.lib().x3dstep_pbn_accum_host(_np_ptr(pt.layers), pt.nlayers, _np_ptr(pt.work), pt.nwork, _np_ptr(acc)))


def pbn_finish(pt, acc_all, W, expect_n, snap):
    """One launch: the W accumulators of every channel (acc_all float64 [W * 4 * channels], rank after rank) merged in rank
    order, the pooled mean and variance written into all S slots of the layer's buffers in `snap` (float32 [snap_n], laid
    out as the keep table's snapshot; the padding is left alone); NaN where the merged count is not expect_n."""
    dev = _check_pbn_device("pbn_finish", pt, acc_all, W)
    _need_flat("pbn_finish", "the snapshot", snap, pt.snap_n, dev)
    check(_steplib.lib().x3dstep_pbn_finish(ptr(pt.d_layers), pt.nlayers, ptr(pt.d_work), pt.nwork, ptr(acc_all), int(W),
                                            int(expect_n), ptr(snap), pt.snap_n, stream()))


def pbn_finish_host(pt, acc_all, W, expect_n, snap):
    """The CPU twin of `pbn_finish`."""
    _check_pbn_host("pbn_finish_host", pt, acc_all, W)
    _need_flat_np("pbn_finish_host", "the snapshot", snap, pt.snap_n)
    check(_steplib.lib().x3dstep_pbn_finish_host(_np_ptr(pt.layers), pt.nlayers, _np_ptr(pt.work), pt.nwork, _np_ptr(acc_all),
                                                 int(W), int(expect_n), _np_ptr(snap), pt.snap_n))


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
