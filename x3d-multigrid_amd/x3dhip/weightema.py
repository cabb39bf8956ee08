"""WeightEMA: an exponential moving average of the flat parameter buffer and of every split_bn.running_mean / running_var,
kept on the device by two launches per update (include/x3dstep.h: x3dstep_ema, x3dstep_ema_keep),
and exchanged with the live values in place for validation (x3dstep_swap, x3dstep_swap_keep), so that no address a captured
graph holds moves.

The decay warms up as min(decay, (1 + k) / (10 + k)), k the number of updates averaged so far.  With a monitor
(Trainer(clip_grad_norm= / monitor= / skip_nonfinite=)) k is derived on the device from the monitor's state: an update that
stepops.apply skipped is not averaged and does not count.  Without one the host counts.

An unguarded non-finite update poisons the average for good: NaN and Inf propagate through e <- d * e + (1 - d) * w as the
arithmetic gives them, and a NaN in e never leaves it.  Train with skip_nonfinite=True to keep such updates out of both
the weights and the average.

The average is not optimizer state: it is in no Trainer.state_dict(); state_dict() here is its own.
"""
import contextlib

import torch

from . import _steplib, stepops


def running_stat_buffers(model):
    """[(name, tensor)] of split_bn.running_mean / running_var of every SubBatchNorm3d, in module order: the buffers a
    forward pass in training mode overwrites (Trainer._keep_table walks the same list)."""
    out = []
    for name, mod in model.named_modules():
        sb = getattr(mod, "split_bn", None)
        if sb is not None:
            prefix = name + "." if name else ""
            out += [(prefix + "split_bn.running_mean", sb.running_mean), (prefix + "split_bn.running_var", sb.running_var)]
    return out


class WeightEMA:
    def __init__(self, fp, model, decay, warmup=True, monitor=None):
        """fp: trainer.FlatParams of `model`; decay in [0, 1); warmup: min(decay, (1 + k) / (10 + k)); monitor: the
        Trainer's gradmonitor.GradMonitor or None.  The average starts as a copy of the weights and statistics as they are
        now (one host read of the monitor's counters)."""
        decay = float(decay)
        if not 0.0 <= decay < 1.0:
            raise ValueError("WeightEMA: decay must lie in [0, 1) (got %r)" % decay)
        if fp.flat.device.type != "cuda":
            raise ValueError("WeightEMA: the flat parameters are on %s; the average's kernels need a GPU" % fp.flat.device)
        self.fp, self.model, self.monitor = fp, model, monitor
        self.decay, self.warmup = decay, bool(warmup)
        self.names = [k for k, _ in model.named_parameters()]
        if len(self.names) != len(fp.offsets):
            raise ValueError("WeightEMA: %d parameters for %d tensors of the flat buffer" % (len(self.names), len(fp.offsets)))
        self.e = fp.flat.clone()
        self._n = 0                          # updates counted on the host (no monitor)
        self._kt = self._kt_old = None
        self._version = None
        base = -self._applied()
        self._woff = self._soff = base       # k = offset + updates applied so far
        self._table()

    # -- counts -------------------------------------------------------------------------------------------------------------
    def _applied(self):
        """Updates applied so far: the monitor's S_STEP - S_SKIPPED (a host read: synchronises), or the host's count."""
        if self.monitor is None:
            return self._n
        st = self.monitor.state.cpu()
        return int(st[_steplib.S_STEP]) - int(st[_steplib.S_SKIPPED])

    def updates(self):
        """Updates averaged into the weights so far (synchronises when there is a monitor)."""
        return self._woff + self._applied()

    def stat_updates(self):
        """Updates averaged into the running statistics since they were last re-created (the long-cycle switch)."""
        self._table()
        return self._soff + self._applied()

    # -- the statistics' table --------------------------------------------------------------------------------------------------
    def _table(self):
        """The keep table over the running statistics; its snapshot is the averaged statistics.  Rebuilt when the long-cycle
        switch re-created the buffers: the average restarts as a copy of the fresh buffers and its k at 1 (one host read of
        the applied-update count, at a switch that already invalidates every graph).  The table before stays referenced
        until the next rebuild: every launch that names it was enqueued on this stream before the first on the new one."""
        ver = self.model._bn_version
        if self._kt is None or self._version != ver:
            named = running_stat_buffers(self.model)
            kt = stepops.KeepTable([b for _, b in named], self.e.device)
            for b, off in zip(kt.buffers, kt.table["offset"]):
                kt.snap[int(off):int(off) + b.numel()].copy_(b)
            if self._kt is not None:
                self._soff = -self._applied()
            self._kt_old, self._kt, self._version = self._kt, kt, ver
            self.stat_names = [k for k, _ in named]
        return self._kt

    def sync_layout(self):
        """Before the forward pass of an update: notice a long-cycle switch while the fresh statistics are still fresh."""
        self._table()

    @property
    def stats(self):
        """The averaged statistics: float32 [snap_n], buffer b at table['offset'][b] (every start a multiple of four)."""
        return self._table().snap

    # -- the two launches -------------------------------------------------------------------------------------------------------
    def update(self):
        """Average the weights and the statistics as they are now: two launches on the current stream, no sync."""
        kt = self._table()
        if self.monitor is None:
            self._n += 1
            state, applied = None, self._n
        else:
            state, applied = self.monitor.state, 0
        stepops.ema(self.e, self.fp.flat, state, self._woff + applied, self.decay, self.warmup)
        stepops.ema_keep(kt, kt.snap, state, self._soff + applied, self.decay, self.warmup)

    def _swap(self):
        kt = self._table()
        stepops.swap(self.fp.flat, self.e)
        stepops.swap_keep(kt, kt.snap)

    @contextlib.contextmanager
    def applied(self):
        """Inside the block the model holds the averaged weights and statistics (exchanged in place by two launches: the
        flat buffer and every running-statistics buffer keep their addresses); on the way out, an exception included, they
        are exchanged back.  Call model.aggregate_sub_bn_stats() inside the block before evaluating, as the validators do:
        the aggregated bn.* then belong to the average until the next aggregation outside.  No training step inside."""
        self._swap()
        try:
            yield self
        finally:
            self._swap()

    # -- state ------------------------------------------------------------------------------------------------------------------
    def state_dict(self):
        """{'decay', 'warmup', 'updates', 'stat_updates', 'model'}; 'model' in the layout of model.state_dict(): parameters
        and split-BN running statistics averaged, every other key as the live model has it (load it with
        model.load_state_dict to score the average)."""
        kt = self._table()
        sd = {k: v.detach().clone() for k, v in self.model.state_dict().items()}
        for name, (o, n) in zip(self.names, self.fp.offsets):
            sd[name] = self.e[o:o + n].view(sd[name].shape).clone()
        for name, b, off in zip(self.stat_names, kt.buffers, kt.table["offset"]):
            sd[name] = kt.snap[int(off):int(off) + b.numel()].view(b.shape).clone()
        return {'decay': self.decay, 'warmup': self.warmup, 'updates': self.updates(), 'stat_updates': self.stat_updates(),
                'model': sd}

    def load_state_dict(self, sd):
        """Restores the averages and their counts (decay and warmup stay what the constructor was given).  The statistics
        must have the live model's layout (the same long-cycle split)."""
        kt = self._table()
        msd = sd['model']
        for name, (o, n) in zip(self.names, self.fp.offsets):
            if name not in msd or msd[name].numel() != n:
                raise ValueError("WeightEMA.load_state_dict: parameter %s is missing or has another size" % name)
        for name, b in zip(self.stat_names, kt.buffers):
            if name not in msd or msd[name].numel() != b.numel():
                raise ValueError("WeightEMA.load_state_dict: statistics %s are missing or have another size (another "
                                 "long-cycle split?)" % name)
        dev = self.e.device
        for name, (o, n) in zip(self.names, self.fp.offsets):
            self.e[o:o + n].copy_(msd[name].reshape(-1).to(dev, torch.float32))
        for name, b, off in zip(self.stat_names, kt.buffers, kt.table["offset"]):
            kt.snap[int(off):int(off) + b.numel()].copy_(msd[name].reshape(-1).to(dev, torch.float32))
        applied = self._applied()
        self._woff = int(sd['updates']) - applied
        self._soff = int(sd['stat_updates']) - applied
