"""Second-moment state for the fused update: Adam with L2, AdamW and LAMB on the flat buffers (include/x3dstep.h; DESIGN.md
section 6).  `fp.mom` is exp_avg; the second flat buffer, exp_avg_sq, is allocated here and only here, with the betas, eps,
the mode and the host's part of the update count -- and for LAMB the workspace of the partial sums, the per-tensor sums of
squares of the weights and of the direction, the trust ratios and the adaptation flags.

The count of applied updates that the bias correction needs lives where the guard decides: with skip_nonfinite the kernels
form it from the monitor's state words (steps measured minus steps skipped) plus the offset `count` kept here, so a skipped
update does not advance it and nothing is read back; without the guard every update is applied and the host counts them.
Nothing here synchronises except `read`, `step` and the checkpoint functions.
"""
import fnmatch

import numpy as np
import torch

from . import _steplib, stepops

MODES = ("adamw", "adam", "lamb")


def describe(trainer, model):
    """The one line the training scripts print before training when an adaptive optimizer is on."""
    a = trainer.adam
    hy = trainer.hyper
    no_decay = int(np.count_nonzero(hy.wd_scale == 0))
    line = "optimizer %s: betas (%g, %g), eps %g, %d of %d tensors exempt from decay" % (
        a.mode, a.betas[0], a.betas[1], a.eps, no_decay, len(a.names))
    if a.mode == "lamb":
        line += ", %d exempt from adaptation" % int(np.count_nonzero(a.adapt == 0))
    return line


def log_field(trainer):
    """`trust MIN/MEDIAN/MAX` over the adapted tensors for the log line (synchronises, where the line already does)."""
    a = trainer.adam
    on = a.adapt != 0
    if not on.any():
        return "trust -/-/-"
    v = a.trust.cpu().numpy()[on]
    return "trust %.3g/%.3g/%.3g" % (float(v.min()), float(np.median(v)), float(v.max()))


class AdamState:
    def __init__(self, fp, names, hyper, monitor=None, mode="adamw", betas=(0.9, 0.999), eps=1e-8, guarded=False):
        """fp: trainer.FlatParams; names: one per tensor, in the order of fp.offsets; hyper: the hypergroups.HyperTable of
        the same buffer; monitor: the gradmonitor.GradMonitor, needed when `guarded` (the update then reads its state and
        ring)."""
        if mode not in MODES:
            raise ValueError("AdamState: mode must be one of %s (got %r)" % (MODES, mode))
        names = list(names)
        if len(names) != len(fp.offsets) or len(set(names)) != len(names):
            raise ValueError("AdamState: needs one distinct name per tensor (%d names, %d tensors)" % (len(names), len(fp.offsets)))
        if hyper is None or (guarded and monitor is None):
            raise ValueError("AdamState: needs the hyper table of the flat buffer, and the gradient monitor when guarded")
        b1, b2, eps, _ = stepops._adam_args("AdamState", betas, eps)
        self.fp, self.names, self.hyper, self.monitor = fp, names, hyper, monitor
        self.mode, self.betas, self.eps, self.guarded = mode, (b1, b2), eps, bool(guarded)
        self.decoupled = mode != "adam"
        self.tables = hyper.tables
        self.device = fp.flat.device
        self.count = 0            # guarded: the offset added to the device's count; unguarded: the updates applied so far
        self.exp_avg_sq = torch.zeros_like(fp.flat)
        if mode == "lamb":
            S = len(names)
            self.adapt = np.ones(S, dtype=np.uint8)
            self.d_adapt = torch.from_numpy(self.adapt.copy()).to(self.device)
            self.workspace = torch.zeros(stepops.lamb_workspace_bytes(self.tables.nitems), dtype=torch.uint8, device=self.device)
            self.wsumsq = torch.zeros(S, dtype=torch.float64, device=self.device)
            self.rsumsq = torch.zeros(S, dtype=torch.float64, device=self.device)
            self.trust = torch.ones(S, dtype=torch.float32, device=self.device)

    # -- LAMB's adaptation flags ----------------------------------------------------------------------------------------
    def upload(self):
        """Copy the host flags to the device tensor (one copy; call it outside any graph capture)."""
        self.d_adapt.copy_(torch.from_numpy(self.adapt))

    def exempt(self, pattern):
        """Exempt every parameter whose name matches the fnmatch `pattern` from the adaptation (a trust of exactly 1).
        Returns the number of tensors matched; raises when it matches nothing.  Call upload() afterwards."""
        hit = [i for i, k in enumerate(self.names) if fnmatch.fnmatchcase(k, pattern)]
        if not hit:
            raise ValueError("AdamState: pattern %r matches no parameter" % (pattern,))
        self.adapt[hit] = 0
        return len(hit)

    # -- the update -------------------------------------------------------------------------------------------------------
    def update(self, w, g, m, lr, weight_decay, grad_scale):
        """The update's launches on the current stream: one for adamw / adam, three for lamb.  Guarded: after the monitor's
        measure of this step."""
        mon, t, hy = self.monitor, self.tables, self.hyper.hyper
        if self.guarded:
            st, count = (mon.state, mon.ring, mon.R), self.count
        else:
            self.count += 1
            st, count = (None, None, 0), self.count
        if self.mode != "lamb":
            stepops.adam(w, g, m, self.exp_avg_sq, t, hy, *st, count, lr, self.betas, self.eps, weight_decay, grad_scale,
                         self.decoupled)
            return
        v = self.exp_avg_sq
        stepops.lamb_moments(w, g, m, v, t, hy, *st, count, self.workspace, self.betas, self.eps, weight_decay, grad_scale)
        stepops.lamb_trust(t, hy, self.d_adapt, *st, count, self.workspace, self.wsumsq, self.rsumsq, self.trust)
        stepops.lamb_apply(w, m, v, t, hy, self.trust, *st, count, lr, self.betas, self.eps, weight_decay)

    def step(self):
        """The number of applied updates (guarded: one host read of the monitor's state)."""
        if not self.guarded:
            return self.count
        st = self.monitor.state.cpu()
        return self.count + int(st[_steplib.S_STEP]) - int(st[_steplib.S_SKIPPED])

    def read(self):
        """Host arrays keyed by parameter name (synchronises; for logging and tests), LAMB only: {"trust": {name: float32},
        "wnorm": {name: float64}, "rnorm": {name: float64}} of the latest applied update."""
        if self.mode != "lamb":
            raise ValueError("AdamState.read: %s has no trust ratios" % self.mode)
        tr = self.trust.cpu().numpy()
        wn, rn = np.sqrt(self.wsumsq.cpu().numpy()), np.sqrt(self.rsumsq.cpu().numpy())
        return {"trust": {k: tr[i] for i, k in enumerate(self.names)}, "wnorm": {k: wn[i] for i, k in enumerate(self.names)},
                "rnorm": {k: rn[i] for i, k in enumerate(self.names)}}

    # -- checkpoints (torch.optim.AdamW's layout) -------------------------------------------------------------------------------
    def state_entries(self):
        """{i: {'step', 'exp_avg', 'exp_avg_sq'}} per parameter, empty before the first applied update."""
        step = self.step()
        if step < 1:
            return {}
        fp = self.fp
        out = {}
        for i, (o, k) in enumerate(fp.offsets):
            shape = fp.params[i].shape
            out[i] = {'step': torch.tensor(float(step)), 'exp_avg': fp.mom[o:o + k].view(shape).clone(),
                      'exp_avg_sq': self.exp_avg_sq[o:o + k].view(shape).clone()}
        return out

    def load_state_entries(self, st):
        """Restores both moments and sets `count` so that the next update's k continues from the checkpoint's step."""
        fp = self.fp
        step = 0
        for i, (o, k) in enumerate(fp.offsets):
            ent = st.get(i, st.get(str(i)))
            if ent is None:
                if st:
                    raise ValueError("AdamState: the checkpoint has no state for parameter %d" % i)
                continue
            fp.mom[o:o + k].copy_(ent['exp_avg'].reshape(-1).to(self.device))
            self.exp_avg_sq[o:o + k].copy_(ent['exp_avg_sq'].reshape(-1).to(self.device))
            step = int(float(ent['step']))
        if not st:
            fp.mom.zero_()
            self.exp_avg_sq.zero_()
        self.count = step
        if self.guarded:
            s = self.monitor.state.cpu()
            self.count = step - (int(s[_steplib.S_STEP]) - int(s[_steplib.S_SKIPPED]))

    def lamb_state_dict(self):
        return {"names": list(self.names), "adapt": [int(v) for v in self.adapt]}

    def load_lamb_state_dict(self, sd):
        if list(sd["names"]) != self.names:
            raise ValueError("AdamState: the checkpoint's parameter names differ from the model's")
        adapt = [int(v) for v in sd["adapt"]]
        if len(adapt) != len(self.names) or any(v not in (0, 1) for v in adapt):
            raise ValueError("AdamState: the checkpoint's adapt must hold one 0 or 1 per tensor")
        self.adapt[:] = adapt
        self.upload()
