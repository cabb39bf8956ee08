"""GradMonitor: per-tensor statistics of the flat gradient recorded in a device-resident ring, and clipping by the global
norm, between the all-reduce and the fused SGD kernel (include/x3dstep.h).

`observe` enqueues three launches (two without clipping) on the current stream and never synchronises; `read`,
`first_nonfinite` and `.item()` on `last_norm()` are where the host waits.  The ring is diagnostics, not optimizer state:
it is in no state_dict.
"""
import numpy as np
import torch

from . import _steplib, stepops


class SkippedRunError(RuntimeError):
    """Too many updates in a row were skipped for a non-finite gradient (GradMonitor.skip_report)."""


class GradMonitor:
    def __init__(self, flat_params, names, ring=64, max_norm=None, inv_world=1.0):
        """flat_params: trainer.FlatParams (its .grad is observed unless observe() is given another buffer of the same
        layout); names: one per tensor, in the order of flat_params.offsets; ring: records kept; max_norm: clip the global
        norm to it (None / <= 0: statistics only); inv_world: 1 / world, what the SGD kernel multiplies the summed
        gradient by -- the norm is that of the gradient the update applies."""
        names = list(names)
        if len(names) != len(flat_params.offsets):
            raise ValueError("GradMonitor: %d names for %d tensors" % (len(names), len(flat_params.offsets)))
        if len(set(names)) != len(names):
            raise ValueError("GradMonitor: the names must differ")
        ring = int(ring)
        if ring < 1:
            raise ValueError("GradMonitor: ring must hold at least one record (got %d)" % ring)
        dev = flat_params.grad.device
        if dev.type != "cuda":
            raise ValueError("GradMonitor: the flat gradient is on %s; the monitor's kernels need a GPU" % dev)
        at = 0
        for (o, k) in flat_params.offsets:
            if o != at:
                raise ValueError("GradMonitor: the tensors must cover the flat buffer in order")
            at += k
        self.fp = flat_params
        self.names = names
        self.R = ring
        self.max_norm = 0.0 if max_norm is None else float(max_norm)
        self.inv_world = float(inv_world)
        self.tables = stepops.StepTables(stepops.segment_table([k for _, k in flat_params.offsets]), dev)
        self.workspace = torch.zeros(self.tables.workspace_bytes, dtype=torch.uint8, device=dev)
        self.ring = torch.zeros(ring * self.tables.record_bytes, dtype=torch.uint8, device=dev)
        self.state = torch.from_numpy(stepops.new_state()).to(dev)

    @property
    def clipping(self):
        return self.max_norm > 0.0

    def observe(self, grad=None):
        """Record the statistics of `grad` (default: the flat gradient) and, with max_norm, scale it in place."""
        stepops.observe(self.fp.grad if grad is None else grad, self.tables, self.workspace, self.state, self.ring, self.R,
                        self.max_norm, self.inv_world)

    def measure(self, grad=None):
        """Record the statistics of `grad` and the coefficient for max_norm, as `observe` does, and leave the gradient as it
        is: the two launches before stepops.apply, which reads the decision and the coefficient from the state."""
        stepops.measure(self.fp.grad if grad is None else grad, self.tables, self.workspace, self.state, self.ring, self.R,
                        self.max_norm, self.inv_world)

    def skipped(self):
        """Updates stepops.apply skipped so far: an int64 device scalar (a view of the state, no copy, no sync)."""
        return self.state[_steplib.S_SKIPPED]

    def skip_run(self):
        """Updates skipped in a row, 0 after an applied one: an int64 device scalar (a view of the state, no sync)."""
        return self.state[_steplib.S_RUN]

    def skip_report(self, max_skip_run=None):
        """Where a training loop already waits for the loss (synchronises): the number of skipped updates, after
        raising SkippedRunError when `max_skip_run` updates in a row were skipped."""
        st = self.state.cpu().numpy()
        run = int(st[_steplib.S_RUN])
        if max_skip_run is not None and max_skip_run > 0 and run >= max_skip_run:
            bad = self.first_nonfinite()
            raise SkippedRunError("%d updates in a row were skipped for a non-finite gradient (limit %d); the first "
                                  "non-finite gradient was at step %d in parameter %s"
                                  % (run, max_skip_run, bad[0], bad[1]))
        return int(st[_steplib.S_SKIPPED])

    def last_norm(self):
        """The norm of the latest observed step: a float64 device scalar (a view of the state, no copy, no sync)."""
        return self.state.view(torch.float64)[_steplib.S_NORM]

    def last_coef(self):
        """The coefficient of the latest observed step: a float32 device scalar (1 while clipping is off)."""
        return self.state.view(torch.float32)[2 * _steplib.S_COEF]

    def steps(self):
        """Steps observed so far (synchronises)."""
        return int(self.state[_steplib.S_STEP].item())

    def first_nonfinite(self):
        """(step, parameter name) of the first non-finite gradient element seen, or None (synchronises)."""
        st = self.state.cpu().numpy()
        if st[_steplib.S_BAD_STEP] < 0:
            return None
        return int(st[_steplib.S_BAD_STEP]), self.names[int(st[_steplib.S_BAD_SEG])]

    def read(self):
        """The records still in the ring, oldest first (synchronises): a dict of host arrays over those K steps --
        "step" int64 [K], "total" / "norm" float64 [K], "coef" float32 [K], "nonfinite" int32 [K], "first_bad" (a list of
        K names or None) and, keyed by parameter name, "sumsq" (float64 [K] each), "hash" (uint64 [K] each) and
        "nonfinite_by_name" (int32 [K] each)."""
        st = self.state.cpu().numpy()
        raw = self.ring.cpu().numpy().reshape(self.R, self.tables.record_bytes)
        steps, slots = stepops.ring_steps(st, self.R)
        S, K = self.tables.S, len(steps)
        heads = np.zeros(K, dtype=_steplib.HEADER_DT)
        sumsq, hsh, nf = np.zeros((K, S), np.float64), np.zeros((K, S), np.uint64), np.zeros((K, S), np.int32)
        for i, slot in enumerate(slots):
            heads[i], sumsq[i], hsh[i], nf[i] = stepops.parse_record(raw[slot], S)
        assert list(heads["step"]) == steps, "the ring's records do not carry the steps the counter implies"
        return {
            "step": heads["step"].copy(), "total": heads["total"].copy(), "norm": heads["norm"].copy(),
            "coef": heads["coef"].copy(), "nonfinite": heads["nonfinite"].copy(),
            "first_bad": [None if b < 0 else self.names[b] for b in heads["first_bad"]],
            "sumsq": {k: sumsq[:, i].copy() for i, k in enumerate(self.names)},
            "hash": {k: hsh[:, i].copy() for i, k in enumerate(self.names)},
            "nonfinite_by_name": {k: nf[:, i].copy() for i, k in enumerate(self.names)},
        }
