"""Layer-wise adaptive rate scaling (LARS, You et al. 2017) for the fused update: a rate of trust `eta` for every parameter
tensor of the flat buffer, held on the host by parameter name and mirrored in one device tensor, and the device tensors
stepops.trust writes every step -- the sum of squares of every tensor's weights and its trust ratio
eta |w| / (|g| + wd |w| + eps) -- which stepops.apply_lars reads (include/x3dstep.h).

The gradient's norms come from the monitor's record of the step, the scales from the HyperTable; nothing here
synchronises except `read`.  The table is changed on the host, between steps, and copied to the device outside every
graph; the launches read it from device memory.
"""
import fnmatch

import numpy as np
import torch

from . import stepops


def describe(trainer):
    """The one line the training scripts print before training when the feature is on."""
    t = trainer.lars
    adapted, exempt = t.summary()
    return "lars: %d tensors adapted, %d exempt, eta %g, eps %g, clip %s" % (adapted, exempt, t.base_eta, t.eps,
                                                                            "on" if t.clip else "off")


def log_field(trainer):
    """`trust MIN/MEDIAN/MAX` over the adapted tensors for the log line (synchronises, where the line already does)."""
    t = trainer.lars
    on = t.eta > 0
    if not on.any():
        return "trust -/-/-"
    v = t.trust.cpu().numpy()[on]
    return "trust %.3g/%.3g/%.3g" % (float(v.min()), float(np.median(v)), float(v.max()))


def _eta(v):
    v = float(v)
    if not (np.isfinite(v) and v >= 0.0 and v <= float(np.finfo(np.float32).max)):
        raise ValueError("eta must be finite and >= 0 (got %r)" % (v,))
    return np.float32(v)


class TrustTable:
    def __init__(self, fp, names, monitor, hyper, eta=0.001, eps=1e-8, clip=False):
        """fp: trainer.FlatParams; names: one per tensor, in the order of fp.offsets; monitor: the gradmonitor.GradMonitor
        over the same buffer, whose record gives the gradient's sums of squares; hyper: the hypergroups.HyperTable, whose
        scales the trust rule reads.  Every tensor starts at the rate `eta`."""
        names = list(names)
        if len(names) != len(fp.offsets) or len(set(names)) != len(names):
            raise ValueError("TrustTable: needs one distinct name per tensor (%d names, %d tensors)"
                             % (len(names), len(fp.offsets)))
        if monitor is None or hyper is None:
            raise ValueError("TrustTable: needs the gradient monitor and the hyper table of the same flat buffer")
        self.fp, self.names, self.monitor, self.hyper = fp, names, monitor, hyper
        self.device = fp.grad.device
        self.tables = monitor.tables
        self.base_eta = float(_eta(eta))
        self.eps = float(eps)
        self.clip = bool(clip)
        if not (np.isfinite(self.eps) and self.eps >= 0.0):
            raise ValueError("TrustTable: eps must be finite and >= 0 (got %r)" % (eps,))
        S = len(names)
        self.eta = np.full(S, self.base_eta, dtype=np.float32)
        self.d_eta = torch.from_numpy(self.eta.copy()).to(self.device)
        self.wsumsq = torch.zeros(S, dtype=torch.float64, device=self.device)
        self.trust = torch.ones(S, dtype=torch.float32, device=self.device)
        self.workspace = torch.zeros(stepops.trust_workspace_bytes(self.tables.nitems), dtype=torch.uint8, device=self.device)

    def upload(self):
        """Copy the host rates to the device tensor (one copy; call it outside any graph capture)."""
        self.d_eta.copy_(torch.from_numpy(self.eta))

    def _set(self, pattern, eta):
        hit = [i for i, k in enumerate(self.names) if fnmatch.fnmatchcase(k, pattern)]
        if not hit:
            raise ValueError("TrustTable: pattern %r matches no parameter" % (pattern,))
        self.eta[hit] = _eta(eta)
        return hit

    def set(self, pattern, eta):
        """Give every parameter whose name matches the fnmatch `pattern` this rate of trust (0: exempt, a trust of exactly
        1) and copy the table to the device.  Returns the number of tensors matched; raises when it matches nothing."""
        hit = self._set(pattern, eta)
        self.upload()
        return len(hit)

    def apply(self, spec):
        """A dict of pattern -> eta, applied in order; one copy to the device."""
        for pattern, eta in spec.items():
            self._set(pattern, eta)
        self.upload()

    def compute(self, w, lr, weight_decay, grad_scale):
        """The two launches of stepops.trust on the current stream, after the monitor's measure / observe of this step."""
        mon = self.monitor
        stepops.trust(w, self.tables, self.hyper.hyper, self.d_eta, mon.state, mon.ring, mon.R, self.workspace, self.wsumsq,
                      self.trust, lr, weight_decay, grad_scale, self.eps, self.clip)

    def read(self):
        """Host arrays keyed by parameter name (synchronises; for logging and tests): {"trust": {name: float32},
        "wnorm": {name: float64}} of the latest step."""
        tr = self.trust.cpu().numpy()
        wn = np.sqrt(self.wsumsq.cpu().numpy())
        return {"trust": {k: tr[i] for i, k in enumerate(self.names)}, "wnorm": {k: wn[i] for i, k in enumerate(self.names)}}

    def summary(self):
        """(tensors adapted, tensors exempt)."""
        adapted = int(np.count_nonzero(self.eta > 0))
        return adapted, len(self.names) - adapted

    def torch_reference(self, w, g, lr, weight_decay, grad_scale, coef=1.0):
        """The trust ratios in plain torch, fp64, from flat w and g (any device): a [S] float64 tensor.  For comparison
        only: two norms per tensor and a host loop, never on the training path."""
        hy = np.stack([self.hyper.lr_scale, self.hyper.wd_scale], axis=1)
        out = torch.ones(len(self.names), dtype=torch.float64)
        for i, (o, k) in enumerate(self.fp.offsets):
            a = float(torch.linalg.vector_norm(w[o:o + k].double()))
            b = float(torch.linalg.vector_norm(g[o:o + k].double())) * float(np.float32(grad_scale)) * float(np.float32(coef))
            if not (self.eta[i] > 0 and a > 0 and b > 0 and np.isfinite(a) and np.isfinite(b)):
                continue
            wd_s = float(np.float32(weight_decay) * hy[i, 1])
            lr_s = float(np.float32(lr) * hy[i, 0])
            r = float(self.eta[i]) * a / (b + wd_s * a + float(np.float32(self.eps)))
            if self.clip:
                r = min(r / lr_s, 1.0) if lr_s > 0 else 1.0
            out[i] = r
        return out

    def state_dict(self):
        return {"names": list(self.names), "eta": [float(v) for v in self.eta], "eps": self.eps, "clip": self.clip}

    def load_state_dict(self, sd):
        if list(sd["names"]) != self.names:
            raise ValueError("TrustTable: the checkpoint's parameter names differ from the model's")
        eta = [_eta(v) for v in sd["eta"]]
        if len(eta) != len(self.names):
            raise ValueError("TrustTable: the checkpoint holds %d rates for %d tensors" % (len(eta), len(self.names)))
        eps = float(sd["eps"])
        if not (np.isfinite(eps) and eps >= 0.0):
            raise ValueError("TrustTable: the checkpoint's eps must be finite and >= 0 (got %r)" % (eps,))
        self.eta[:] = eta
        self.eps, self.clip = eps, bool(sd["clip"])
        self.upload()
