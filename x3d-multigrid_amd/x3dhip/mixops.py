"""Tensor-level wrappers over the mixing C ABI (include/x3dmix.h), in the style of stepops.py and dataops.py.

Sizes, dtypes and devices are checked here, on the host, before anything is launched: a bad call raises ValueError and
launches nothing.  Every launch goes to the current stream; none allocates inside the library or synchronises, so each may
be captured into a graph.  There is no fallback: a CPU tensor raises; the `*_host` functions are the library's CPU twins on
numpy arrays (the tests' second implementation of the same arithmetic, never a substitute on the training path).
"""
import numpy as np
import torch

from . import _mixlib, ops
from ._lib import ptr, stream
from ._mixlib import SAMPLE_BYTES, SAMPLE_DT, check


def _np_ptr(a):
    return a.ctypes.data


def identity_plan(B):
    """The plan that mixes nothing: every sample its own partner, lam = 1, an empty box."""
    plan = np.zeros(int(B), dtype=SAMPLE_DT)
    plan["partner"] = np.arange(int(B), dtype=np.int32)
    plan["lam"] = np.float32(1.0)
    return plan


def plan_to_device(plan, device):
    """A host plan (SAMPLE_DT [B]) as the uint8 [B, 32] device tensor the kernels read (a blocking copy: tests and tools; the
    BatchMixer uploads from a pinned buffer)."""
    plan = np.ascontiguousarray(plan, dtype=SAMPLE_DT)
    return torch.from_numpy(plan.view(np.uint8).reshape(-1, SAMPLE_BYTES).copy()).to(device)


def _clip_geometry(who, x):
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() < 4 or x.numel() == 0:
        raise ValueError("%s: clips must be a float32 tensor [B, planes.., H, W] of at least 4 dimensions" % who)
    if not x.is_cuda or not x.is_contiguous():
        raise ValueError("%s: clips must be contiguous on a CUDA(HIP) device (the mixing path has no CPU fallback)" % who)
    B, H, W = int(x.shape[0]), int(x.shape[-2]), int(x.shape[-1])
    planes = x[0].numel() // (H * W)
    if planes * H * W >= 1 << 31:
        raise ValueError("%s: a clip of %d elements (2^31 or more)" % (who, planes * H * W))
    return B, planes, H, W


def _need_plan(who, plan, B, dev):
    if (not isinstance(plan, torch.Tensor) or plan.dtype != torch.uint8 or plan.device != dev or not plan.is_contiguous()
            or plan.numel() != B * SAMPLE_BYTES or plan.data_ptr() % 4):
        raise ValueError("%s: plan must be a contiguous uint8 [%d, %d] on %s" % (who, B, SAMPLE_BYTES, dev))


def mix_clips(x, plan, out=None):
    """out[b] = the mix of x[b] and x[partner_b] by plan entry b (mixup, CutMix or a copy: include/x3dmix.h).  x: float32
    clips [B, 3, T, H, W] (any [B, .., H, W]); plan: the device plan; out: a tensor of x's shape that shares no memory with x
    (the Trainer's static graph input), or None for a fresh one.  One launch."""
    B, planes, H, W = _clip_geometry("mix_clips", x)
    _need_plan("mix_clips", plan, B, x.device)
    if out is None:
        out = ops._f(tuple(x.shape), x)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != x.device
          or tuple(out.shape) != tuple(x.shape) or not out.is_contiguous()):
        raise ValueError("mix_clips: out must be a contiguous float32 %s on %s" % (tuple(x.shape), x.device))
    nbytes = x.numel() * 4
    if x.data_ptr() < out.data_ptr() + nbytes and out.data_ptr() < x.data_ptr() + nbytes:
        raise ValueError("mix_clips: x and out overlap (the mix is out of place)")
    check(_mixlib.lib().x3dmix_clips(ptr(x), ptr(out), ptr(plan), B, planes, H, W, stream()))
    return out


def mix_targets(labels, plan, n_classes, smoothing=0.0, out=None):
    """Soft targets float32 [B, n_classes] of int64 labels [B] (or [B, 1]) under the plan: lam of the sample's own smoothed
    one-hot and 1 - lam of its partner's (timm's smoothing rule).  One launch."""
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64 or labels.numel() == 0:
        raise ValueError("mix_targets: labels must be an int64 tensor [B] or [B, 1]")
    if labels.dim() not in (1, 2) or (labels.dim() == 2 and labels.shape[1] != 1):
        raise ValueError("mix_targets: labels must be [B] or [B, 1] (got %s)" % (tuple(labels.shape),))
    if not labels.is_cuda or not labels.is_contiguous():
        raise ValueError("mix_targets: labels must be contiguous on a CUDA(HIP) device")
    B, C = int(labels.shape[0]), int(n_classes)
    if C < 1:
        raise ValueError("mix_targets: n_classes = %d" % C)
    smoothing = float(smoothing)
    if not 0.0 <= smoothing < 1.0:
        raise ValueError("mix_targets: smoothing %r outside [0, 1)" % smoothing)
    _need_plan("mix_targets", plan, B, labels.device)
    if out is None:
        out = ops._f((B, C), labels)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != labels.device
          or tuple(out.shape) != (B, C) or not out.is_contiguous()):
        raise ValueError("mix_targets: out must be a contiguous float32 %s on %s" % ((B, C), labels.device))
    check(_mixlib.lib().x3dmix_targets(ptr(labels), ptr(plan), B, C, smoothing, ptr(out), stream()))
    return out


def soft_ce(logits, targets, grad_scale=1.0, rng=None):
    """Mean softmax cross entropy of logits [R, C] against float32 soft targets [R, C] (F.cross_entropy(logits, probabilities)):
    (loss [1], dlogits [R, C] = grad_scale * d loss / d logits).  rng: the head's dropout state, advanced by one (as head_ce
    does).  Two launches."""
    if not isinstance(logits, torch.Tensor) or not isinstance(targets, torch.Tensor):
        raise ValueError("soft_ce: logits and targets must be tensors")
    if logits.dtype != torch.float32 or targets.dtype != torch.float32:
        raise ValueError("soft_ce: logits and targets must be float32 (got %s, %s)" % (logits.dtype, targets.dtype))
    if logits.dim() != 2 or tuple(targets.shape) != tuple(logits.shape) or logits.numel() == 0:
        raise ValueError("soft_ce: logits [R, C] and targets of the same shape (got %s, %s)"
                         % (tuple(logits.shape), tuple(targets.shape)))
    if targets.device != logits.device:
        raise ValueError("soft_ce: logits and targets on different devices")
    if not logits.is_cuda or not logits.is_contiguous() or not targets.is_contiguous():
        raise ValueError("soft_ce: logits and targets must be contiguous on a CUDA(HIP) device")
    if rng is not None and (not isinstance(rng, torch.Tensor) or rng.device != logits.device or rng.numel() != 2
                            or rng.element_size() != 8 or not rng.is_contiguous()):
        raise ValueError("soft_ce: rng must be the head's 64-bit {seed, counter} pair on %s" % logits.device)
    grad_scale = float(grad_scale)
    if not np.isfinite(grad_scale):
        raise ValueError("soft_ce: grad_scale %r is not finite" % grad_scale)
    R, C = logits.shape
    loss, dlog, sc = ops._f((1,), logits), ops._f((R, C), logits), ops._f((R,), logits)
    check(_mixlib.lib().x3dmix_soft_ce(ptr(logits), ptr(targets), ptr(loss), ptr(dlog), ptr(sc), R, C, grad_scale, ptr(rng),
                                       stream()))
    return loss, dlog


# -- the CPU twins on numpy arrays ---------------------------------------------------------------------------------------------
def _np_plan(who, plan, B):
    if not isinstance(plan, np.ndarray) or plan.dtype != SAMPLE_DT or plan.shape != (B,) or not plan.flags.c_contiguous:
        raise ValueError("%s: plan must be a contiguous SAMPLE_DT [%d] array" % (who, B))


def mix_clips_host(x, plan, out=None):
    if not isinstance(x, np.ndarray) or x.dtype != np.float32 or x.ndim < 4 or x.size == 0 or not x.flags.c_contiguous:
        raise ValueError("mix_clips_host: clips must be a contiguous float32 array [B, planes.., H, W]")
    B, H, W = x.shape[0], x.shape[-2], x.shape[-1]
    planes = x[0].size // (H * W)
    _np_plan("mix_clips_host", plan, B)
    if out is None:
        out = np.empty_like(x)
    elif (not isinstance(out, np.ndarray) or out.dtype != np.float32 or out.shape != x.shape or not out.flags.c_contiguous
          or not out.flags.writeable):
        raise ValueError("mix_clips_host: out must be a writeable contiguous float32 %s" % (x.shape,))
    check(_mixlib.lib().x3dmix_clips_host(_np_ptr(x), _np_ptr(out), _np_ptr(plan), B, planes, H, W))
    return out


def mix_targets_host(labels, plan, n_classes, smoothing=0.0):
    labels = np.ascontiguousarray(labels, dtype=np.int64).reshape(-1)
    B, C = labels.size, int(n_classes)
    _np_plan("mix_targets_host", plan, B)
    out = np.empty((B, C), dtype=np.float32)
    check(_mixlib.lib().x3dmix_targets_host(_np_ptr(labels), _np_ptr(plan), B, C, float(smoothing), _np_ptr(out)))
    return out


def soft_ce_host(logits, targets, grad_scale=1.0, rng=None):
    """(loss float32 [1], dlogits float32 [R, C]) of the twin; rng: a uint64 [2] array, advanced in place."""
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    targets = np.ascontiguousarray(targets, dtype=np.float32)
    if logits.ndim != 2 or targets.shape != logits.shape or logits.size == 0:
        raise ValueError("soft_ce_host: logits [R, C] and targets of the same shape")
    if rng is not None and (not isinstance(rng, np.ndarray) or rng.dtype != np.uint64 or rng.shape != (2,)):
        raise ValueError("soft_ce_host: rng must be a uint64 [2] array")
    R, C = logits.shape
    loss, dlog, sc = np.empty(1, np.float32), np.empty((R, C), np.float32), np.empty(R, np.float32)
    check(_mixlib.lib().x3dmix_soft_ce_host(_np_ptr(logits), _np_ptr(targets), _np_ptr(loss), _np_ptr(dlog), _np_ptr(sc), R, C,
                                            float(grad_scale), None if rng is None else _np_ptr(rng)))
    return loss, dlog
