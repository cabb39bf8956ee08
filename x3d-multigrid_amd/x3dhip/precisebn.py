"""PreciseBN: the BatchNorm statistics recomputed over K training batches under exactly the weights to be scored, pooled
over batches, splits and ranks on the device (include/x3dstep.h: x3dstep_pbn_accum, x3dstep_pbn_finish; DESIGN.md section 6
row 17), and exchanged with the live statistics in place for validation (x3dstep_swap_keep), so that no address a captured
graph holds moves.

A cell is one split of one batch on one rank.  A training-mode trunk pass with BN momentum 1.0 leaves each cell's mean and
unbiased variance in split_bn.running_mean / running_var (csrc/bn.hip computes (1 - m) * old + m * new in fp64: with m = 1 and
a finite `old` that is `new` rounded once); one launch per batch folds them into an fp64 accumulator per channel.  Over
n = K * S * W cells the pooled statistics are the reference's aggregation rule (x3d.py:27-45, SubBatchNorm3d.aggregate_stats)
applied to all n cells instead of S:

    mean = sum(mu) / n        var = sum(v) / n + sum((mu - mean)^2) / n

which, unlike a mean of variances, keeps the between-cell term.  Every split slot of a layer receives the same pooled
value, so model.aggregate_sub_bn_stats() inside `applied()` gives bn.running_* equal to the pooled values bit for bit when
the number of splits is a power of two (every shipped configuration: base 4 x {8, 4, 2, 1}) and within one fp32 ulp
otherwise (the sum of S equal values divided by S is then rounded).

Only the trunk runs: the head's dropout RNG, the model's pending num_batches_tracked count and every parameter stay as
they are; no backward pass, no graph capture.  The statistics are derived data: nothing loads them on resume.
"""
import contextlib

import torch

from . import _steplib, stepops
from .weightema import running_stat_buffers


class PreciseBN:
    def __init__(self, model, process_group=None):
        """model: an x3d.ResNet on a GPU; process_group: the ranks whose cells are pooled (None: this process alone)."""
        self.model, self.pg = model, process_group
        self._kt = self._pt = self._acc = None
        self._version = None          # model._bn_version the tables were built for
        self._computed = None         # ... and the one the snapshot's statistics belong to
        self.batches = self.cells = 0

    def _tables(self):
        """The keep table over the 168 running-statistics buffers, its snapshot and a zero state of its own, the layer
        and work tables over it and the accumulators; rebuilt when the long-cycle switch re-created the buffers."""
        ver = self.model._bn_version
        if self._kt is None or self._version != ver:
            named = running_stat_buffers(self.model)
            dev = named[0][1].device
            if dev.type != "cuda":
                raise ValueError("PreciseBN: the model is on %s; the statistics' kernels need a GPU" % dev)
            splits = [m.num_splits for m in self.model.modules() if getattr(m, "split_bn", None) is not None]
            self._kt = stepops.KeepTable([b for _, b in named], dev)
            self._pt = stepops.PbnTable(self._kt, splits)
            self._acc = self._pt.new_acc()
            self._state = torch.from_numpy(stepops.new_state()).to(dev)
            self._names = [k for k, _ in named]
            self._version, self._computed = ver, None
        return self._kt, self._pt

    def _gather(self, acc):
        """(the accumulators of every rank, rank after rank; the number of ranks): one all-gather, on the device over RCCL
        (backend "nccl"), staged through the host for any other backend."""
        if self.pg is None:
            return acc, 1
        import torch.distributed as dist
        world = dist.get_world_size(self.pg)
        cdev = acc.device if dist.get_backend(self.pg) == "nccl" else torch.device("cpu")
        src = acc.to(cdev)
        out = torch.empty((world,) + tuple(src.shape), dtype=src.dtype, device=cdev)
        dist.all_gather(list(out.unbind(0)), src, group=self.pg)
        return out.to(acc.device).view(-1), world

    def compute(self, batches):
        """batches: an iterable of float [N, 3, T, H, W] tensors on the model's GPU, N divisible by the current number of
        splits, the same number of batches on every rank.  Afterwards the live statistics are what they were, and the
        pooled statistics wait in this object's snapshot for `applied()`.  Returns self."""
        from . import engine
        kt, pt = self._tables()
        model = self.model
        S = model.bn1.num_splits
        stepops.keep(kt, self._state, _steplib.KEEP_SAVE)
        self._acc.zero_()
        K = 0
        try:
            with torch.no_grad():
                for x in batches:
                    engine.trunk_forward(model, x.contiguous().float(), True, None, bn_momentum=1.0)
                    stepops.pbn_accum(pt, self._acc)
                    K += 1
        finally:
            stepops.swap_keep(kt, kt.snap)       # the live buffers are the saved ones again
        if K < 1:
            raise ValueError("PreciseBN.compute: no batches")
        acc_all, W = self._gather(self._acc)
        stepops.pbn_finish(pt, acc_all, W, K * S * W, kt.snap)
        self.batches, self.cells, self._computed = K, K * S * W, self._version
        return self

    def _check_current(self, who):
        if self._computed is None or self._computed != self.model._bn_version:
            raise RuntimeError("PreciseBN.%s: no statistics for the model's current split-BN buffers (compute() was never "
                               "called, or a long-cycle switch re-created them since): call compute() first" % who)

    @contextlib.contextmanager
    def applied(self):
        """Inside the block the model's split_bn.running_* hold the pooled statistics (exchanged in place by one launch);
        on the way out, an exception included, they are exchanged back.  Call model.aggregate_sub_bn_stats() inside the
        block before evaluating, as the validators do.  No training step inside."""
        self._check_current("applied")
        kt = self._kt
        stepops.swap_keep(kt, kt.snap)
        try:
            yield self
        finally:
            stepops.swap_keep(kt, kt.snap)

    def state_dict(self):
        """{'batches', 'cells', 'model'}; 'model' in the layout of model.state_dict(): split_bn.running_* hold the pooled
        statistics and bn.running_* their aggregation (SubBatchNorm3d.aggregate_stats' expression); every other key as the
        live model has it."""
        self._check_current("state_dict")
        kt = self._kt
        sd = {k: v.detach().clone() for k, v in self.model.state_dict().items()}
        pooled = {}
        for name, b, off in zip(self._names, kt.buffers, kt.table["offset"]):
            pooled[name] = sd[name] = kt.snap[int(off):int(off) + b.numel()].view(b.shape).clone()
        for name, mod in self.model.named_modules():
            if getattr(mod, "split_bn", None) is None:
                continue
            prefix = name + "." if name else ""
            S = mod.num_splits
            mu = pooled[prefix + "split_bn.running_mean"].view(S, -1)
            var = pooled[prefix + "split_bn.running_var"].view(S, -1)
            mean = mu.sum(0) / S
            sd[prefix + "bn.running_mean"] = mean
            sd[prefix + "bn.running_var"] = var.sum(0) / S + ((mu - mean) ** 2).sum(0) / S
        return {'batches': self.batches, 'cells': self.cells, 'model': sd}
