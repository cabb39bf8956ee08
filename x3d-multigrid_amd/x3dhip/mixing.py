"""BatchMixer: mixup, CutMix and label smoothing between a batch and Trainer(objective="soft_ce").

The plan of a batch -- every sample's partner, its weight lam and, for CutMix, its box -- is drawn on the HOST from a numpy
Generator the mixer owns, so nothing is read back from the device and no call synchronises; it is written into a pinned
buffer and uploaded with a non-blocking copy.  The kernels of libx3dmix (mixops.py) then mix the clips in one launch and
build the soft targets in another.  The rules are timm's Mixup: lam ~ Beta(alpha, alpha), the box of rand_bbox (no margin,
edges clipped to the plane, lam corrected to the area that was really cut), smoothing on both labels before they are mixed.

Not here: mixing of Charades labels ("bce" / "loc"), mixing uint8 frames before normalisation, Beta draws on the device, the
generator in a checkpoint (a resumed run restarts it from its seed), boxes that cut in time (a box covers every frame and
channel).
"""
import numpy as np
import torch

from . import mixops
from ._mixlib import SAMPLE_BYTES, SAMPLE_DT

_RING = 4       # pinned staging buffers in rotation: a buffer is written again only after the copy out of it has finished


class BatchMixer:
    def __init__(self, n_classes, mixup_alpha=0.0, cutmix_alpha=0.0, prob=1.0, switch_prob=0.5, label_smoothing=0.0,
                 per_sample=False, seed=0):
        """n_classes: the width of the soft targets.  mixup_alpha / cutmix_alpha: the Beta parameter of each mode, 0 turns
        the mode off; with both positive a batch (per_sample: a sample) is CutMix with probability switch_prob, else mixup.
        prob: the probability that a batch (a sample) is mixed at all.  label_smoothing: timm's epsilon.  per_sample: one
        lam (mode, box) per sample instead of one per batch; the partners are one permutation of the batch either way.
        seed: of the mixer's own generator (the training script passes seed + rank)."""
        self.n_classes = int(n_classes)
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.prob, self.switch_prob = float(prob), float(switch_prob)
        self.label_smoothing = float(label_smoothing)
        self.per_sample = bool(per_sample)
        if self.n_classes < 1:
            raise ValueError("BatchMixer: n_classes = %d" % self.n_classes)
        if not (self.mixup_alpha >= 0.0 and self.cutmix_alpha >= 0.0 and np.isfinite(self.mixup_alpha + self.cutmix_alpha)):
            raise ValueError("BatchMixer: mixup_alpha and cutmix_alpha must be finite and >= 0 (got %r, %r)"
                             % (mixup_alpha, cutmix_alpha))
        if not (0.0 <= self.prob <= 1.0 and 0.0 <= self.switch_prob <= 1.0):
            raise ValueError("BatchMixer: prob and switch_prob must lie in [0, 1] (got %r, %r)" % (prob, switch_prob))
        if not 0.0 <= self.label_smoothing < 1.0:
            raise ValueError("BatchMixer: label_smoothing %r outside [0, 1)" % label_smoothing)
        self.seed = int(seed)
        self.rng = np.random.default_rng(self.seed)
        self.last_plan = None
        self._pinned, self._events, self._slot, self._dev_plan = {}, {}, 0, {}

    @property
    def mixes(self):
        """False when both alphas are 0: the clips pass through untouched, only the targets are built."""
        return self.mixup_alpha > 0.0 or self.cutmix_alpha > 0.0

    # -- the plan, on the host ---------------------------------------------------------------------------------------------
    def _draw_one(self, H, W):
        """(lam fp32, y0, y1, x0, x1) of one draw; an empty box with lam = 1 is the identity."""
        r = self.rng
        if not self.mixes or r.random() >= self.prob:
            return np.float32(1.0), 0, 0, 0, 0
        if self.mixup_alpha > 0.0 and self.cutmix_alpha > 0.0:
            cut = r.random() < self.switch_prob
        else:
            cut = self.cutmix_alpha > 0.0
        alpha = self.cutmix_alpha if cut else self.mixup_alpha
        lam = float(r.beta(alpha, alpha))
        if not cut:
            return np.float32(lam), 0, 0, 0, 0
        ratio = np.sqrt(1.0 - lam)
        cut_h, cut_w = int(H * ratio), int(W * ratio)
        cy, cx = int(r.integers(0, H)), int(r.integers(0, W))
        y0, y1 = min(max(cy - cut_h // 2, 0), H), min(max(cy + cut_h // 2, 0), H)
        x0, x1 = min(max(cx - cut_w // 2, 0), W), min(max(cx + cut_w // 2, 0), W)
        if y0 >= y1 or x0 >= x1:
            return np.float32(1.0), 0, 0, 0, 0
        return np.float32(1.0 - float((y1 - y0) * (x1 - x0)) / float(H * W)), y0, y1, x0, x1

    def draw(self, B, H, W):
        """The plan of the next batch of B clips with H x W planes: a SAMPLE_DT [B] array."""
        B, H, W = int(B), int(H), int(W)
        if B < 1 or H < 1 or W < 1:
            raise ValueError("BatchMixer.draw: B, H, W = %d, %d, %d must be positive" % (B, H, W))
        plan = mixops.identity_plan(B)
        if not self.mixes:
            return plan
        plan["partner"] = self.rng.permutation(B).astype(np.int32)
        if self.per_sample:
            for b in range(B):
                plan["lam"][b], plan["y0"][b], plan["y1"][b], plan["x0"][b], plan["x1"][b] = self._draw_one(H, W)
        else:
            plan["lam"], plan["y0"], plan["y1"], plan["x0"], plan["x1"] = self._draw_one(H, W)
        return plan

    # -- the upload ----------------------------------------------------------------------------------------------------------
    def _upload(self, plan, device):
        B = plan.shape[0]
        key = (device, B)
        if key not in self._pinned:
            self._pinned[key] = [torch.empty(B * SAMPLE_BYTES, dtype=torch.uint8).pin_memory() for _ in range(_RING)]
            self._events[key] = [None] * _RING
            self._dev_plan[key] = [torch.empty((B, SAMPLE_BYTES), dtype=torch.uint8, device=device) for _ in range(_RING)]
        slot, self._slot = self._slot % _RING, self._slot + 1
        ev = self._events[key][slot]
        if ev is not None:
            ev.synchronize()        # the copy issued _RING batches ago: long finished; waits for that copy alone
        host = self._pinned[key][slot]
        host.numpy()[:] = plan.view(np.uint8)
        dev = self._dev_plan[key][slot]
        dev.copy_(host.view(B, SAMPLE_BYTES), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._events[key][slot] = ev
        return dev

    # -- the call ------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _check(x, y):
        if not isinstance(x, torch.Tensor) or x.dim() < 4 or not x.is_cuda:
            raise ValueError("BatchMixer: clips must be a tensor [B, .., H, W] on a CUDA(HIP) device")
        if not isinstance(y, torch.Tensor) or y.dtype != torch.int64 or y.device != x.device or y.shape[0] != x.shape[0]:
            raise ValueError("BatchMixer: labels must be int64 [B] or [B, 1] on the clips' device")

    def __call__(self, x, y, out=None, plan=None):
        """(mixed clips, soft targets float32 [B, n_classes]) of clips x float32 [B, 3, T, H, W] and labels y int64 [B] or
        [B, 1] on x's device.  out=(sx, sy): written into these tensors (the Trainer's static_inputs) and returned.  With
        both alphas 0 no clip kernel is launched: x is returned as it is (copied into sx when one is given).  plan: a host
        plan to use in the place of a drawn one (tests).  `last_plan` is the host copy of the plan that was used."""
        self._check(x, y)
        sx, sy = out if out is not None else (None, None)
        B, H, W = int(x.shape[0]), int(x.shape[-2]), int(x.shape[-1])
        if plan is None:
            plan = self.draw(B, H, W)
        else:
            plan = np.ascontiguousarray(plan, dtype=SAMPLE_DT)
            if plan.shape != (B,):
                raise ValueError("BatchMixer: a plan of %s entries for %d clips" % (plan.shape, B))
        self.last_plan = plan
        dplan = self._upload(plan, x.device)
        targets = mixops.mix_targets(y.contiguous(), dplan, self.n_classes, self.label_smoothing, out=sy)
        if not self.mixes:
            if sx is not None and sx.data_ptr() != x.data_ptr():
                sx.copy_(x)
                return sx, targets
            return x, targets
        return mixops.mix_clips(x.contiguous().float(), dplan, out=sx), targets
