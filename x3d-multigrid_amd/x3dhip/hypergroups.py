"""Per-tensor hyper-parameters of the fused update: a learning-rate scale and a weight-decay scale for every parameter
tensor of the flat buffer, held on the host by parameter name and mirrored in one device tensor of X3DStepHyper that
stepops.apply_groups reads (include/x3dstep.h).

The scales multiply the one base `lr` and `weight_decay` of Trainer.param_groups[0], which schedules and warm-ups keep
driving.  The table is changed on the host, between steps, and copied to the device outside every graph; the update
launch reads it from device memory, so a captured graph that holds the launch sees the new values.
"""
import fnmatch

import numpy as np
import torch

from . import stepops


def recipe(model, wd_exempt_1d=False, head_lr_scale=1.0):
    """The two common cases as a dict of pattern -> dict(lr_scale= / wd_scale=), in the order Trainer(tensor_hyper=)
    applies it: every parameter with ndim <= 1 (BatchNorm scale and shift, biases) exempt from weight decay, and the
    classifier fc2.* at head_lr_scale times the base rate."""
    out = {}
    if wd_exempt_1d:
        for name, p in model.named_parameters():
            if p.dim() <= 1:
                out[name] = dict(wd_scale=0.0)
    if float(head_lr_scale) != 1.0:
        out["fc2.*"] = dict(lr_scale=float(head_lr_scale))
    return out


def describe(trainer):
    """The one line the training scripts print before training when the feature is on."""
    exempt, elements, scaled = trainer.hyper.summary()
    return ("tensor hyper: %d tensors (%d elements) exempt from weight decay, %d tensors at a scaled learning rate, "
            "nesterov %s" % (exempt, elements, scaled, "on" if trainer.param_groups[0]["nesterov"] else "off"))


def _scale(who, v):
    v = float(v)
    if not (np.isfinite(v) and v >= 0.0 and v <= float(np.finfo(np.float32).max)):
        raise ValueError("%s must be finite and >= 0 (got %r)" % (who, v))
    return np.float32(v)


class HyperTable:
    def __init__(self, fp, names, monitor=None):
        """fp: trainer.FlatParams; names: one per tensor, in the order of fp.offsets (named_parameters()); monitor: a
        gradmonitor.GradMonitor over the same buffer, whose item table is then shared."""
        names = list(names)
        if len(names) != len(fp.offsets) or len(set(names)) != len(names):
            raise ValueError("HyperTable: needs one distinct name per tensor (%d names, %d tensors)"
                             % (len(names), len(fp.offsets)))
        self.fp = fp
        self.names = names
        self.device = fp.grad.device
        self.lr_scale = np.ones(len(names), dtype=np.float32)
        self.wd_scale = np.ones(len(names), dtype=np.float32)
        self.hyper = torch.ones(len(names), 2, dtype=torch.float32, device=self.device)
        self._tables = None if monitor is None else monitor.tables

    @property
    def tables(self):
        """The StepTables of the flat buffer: the monitor's when there is one, else built once on first use."""
        if self._tables is None:
            self._tables = stepops.StepTables(stepops.segment_table([k for _, k in self.fp.offsets]), self.device)
        return self._tables

    def upload(self):
        """Copy the host arrays to the device tensor (one copy; call it outside any graph capture)."""
        self.hyper.copy_(torch.from_numpy(np.stack([self.lr_scale, self.wd_scale], axis=1)))

    def _set(self, pattern, lr_scale, wd_scale):
        hit = [i for i, k in enumerate(self.names) if fnmatch.fnmatchcase(k, pattern)]
        if not hit:
            raise ValueError("HyperTable: pattern %r matches no parameter" % (pattern,))
        if lr_scale is not None:
            self.lr_scale[hit] = _scale("lr_scale", lr_scale)
        if wd_scale is not None:
            self.wd_scale[hit] = _scale("wd_scale", wd_scale)
        return hit

    def set(self, pattern, lr_scale=None, wd_scale=None):
        """Give every parameter whose name matches the fnmatch `pattern` these scales (None: left as it is) and copy the
        table to the device.  Returns the number of tensors matched; raises when the pattern matches nothing."""
        hit = self._set(pattern, lr_scale, wd_scale)
        self.upload()
        return len(hit)

    def apply(self, spec):
        """A dict of pattern -> dict(lr_scale= / wd_scale=), applied in order (recipe() gives one); one copy to the device."""
        for pattern, kw in spec.items():
            extra = set(kw) - {"lr_scale", "wd_scale"}
            if extra:
                raise ValueError("HyperTable: pattern %r: unknown keys %s" % (pattern, sorted(extra)))
            self._set(pattern, kw.get("lr_scale"), kw.get("wd_scale"))
        self.upload()

    def summary(self):
        """(tensors exempt from decay, their elements, tensors at a scaled rate)."""
        exempt = [i for i in range(len(self.names)) if self.wd_scale[i] == 0.0]
        scaled = [i for i in range(len(self.names)) if self.lr_scale[i] != 1.0]
        return len(exempt), int(sum(self.fp.offsets[i][1] for i in exempt)), len(scaled)

    def torch_param_groups(self, model, lr, weight_decay):
        """The list of dicts that makes torch.optim.SGD(groups, momentum=, nesterov=) do the same on `model`: one group per
        distinct pair of scales, its lr and weight_decay the fp32 products the kernel's tensor rule forms, as Python
        floats.  model.named_parameters() must give the table's names."""
        named = list(model.named_parameters())
        if [k for k, _ in named] != self.names:
            raise ValueError("torch_param_groups: the model's parameter names are not the table's")
        groups = {}
        for (_, p), ls, ws in zip(named, self.lr_scale, self.wd_scale):
            groups.setdefault((float(ls), float(ws)), []).append(p)
        return [dict(params=ps, lr=float(np.float32(lr) * np.float32(ls)),
                     weight_decay=float(np.float32(weight_decay) * np.float32(ws))) for (ls, ws), ps in groups.items()]

    def state_dict(self):
        return {"names": list(self.names), "lr_scale": [float(v) for v in self.lr_scale],
                "wd_scale": [float(v) for v in self.wd_scale]}

    def load_state_dict(self, sd):
        if list(sd["names"]) != self.names:
            raise ValueError("HyperTable: the checkpoint's parameter names differ from the model's")
        lr = [_scale("lr_scale", v) for v in sd["lr_scale"]]
        wd = [_scale("wd_scale", v) for v in sd["wd_scale"]]
        if len(lr) != len(self.names) or len(wd) != len(self.names):
            raise ValueError("HyperTable: the checkpoint holds %d / %d scales for %d tensors" % (len(lr), len(wd), len(self.names)))
        self.lr_scale[:] = lr
        self.wd_scale[:] = wd
        self.upload()
