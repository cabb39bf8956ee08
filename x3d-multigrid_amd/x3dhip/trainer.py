"""Training-step driver: flat parameter/gradient/momentum buffers, fused SGD, data-parallel
gradient all-reduce (RCCL via torch.distributed) and optional hipGraph capture of the step.

Replaces, for the hot path, what the reference does with ``nn.DataParallel`` + ``optim.SGD``
(train_x3d_kinetics_multigrid.py:177,183,244-279): one process per GPU, each rank runs the
same shape on its share of the batch, gradients are summed with one bucketed all-reduce of
the flat buffer (15.18 MB fp32 for X3D-M) and divided by the world size inside the fused SGD
kernel; BN statistics stay local to the rank (DataParallel semantics).

Objectives: "ce" (Kinetics, single-label cross entropy), "bce" (Charades multi-label BCEWithLogits,
train_x3d_charades.py:177-182) and "loc" (Charades per-frame cls + loc BCE, train_x3d_charades_loc.py:168-189).
"""
import weakref

import torch
import torch.nn.functional as F

from . import ops

# every live Trainer of the process: captured graphs hold raw pointers into the process-wide finalize scratch (ops.scratch),
# so a retired scratch block may only be released when NO trainer holds a graph any more
_TRAINERS = weakref.WeakSet()


class FlatParams:
    """Re-homes every parameter of ``model`` into one contiguous fp32 buffer (and gives each a
    .grad view into a second one), in ``named_parameters()`` order."""

    def __init__(self, model):
        params = [p for _, p in model.named_parameters()]
        self.params = params
        n = sum(p.numel() for p in params)
        dev = params[0].device
        self.flat = torch.empty(n, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(n, dtype=torch.float32, device=dev)
        self.mom = torch.zeros(n, dtype=torch.float32, device=dev)
        self.offsets = []
        o = 0
        for p in params:
            k = p.numel()
            self.flat[o:o + k].copy_(p.data.reshape(-1))
            p.data = self.flat[o:o + k].view(p.shape)
            p.grad = self.grad[o:o + k].view(p.shape)
            self.offsets.append((o, k))
            o += k
        self.numel = n

    def head_first_buckets(self, model, nbuckets=2):
        """Bucket boundaries (element ranges of the flat buffer) in reverse-autograd order:
        the head (fc1+fc2, 45 % of the bytes) is ready first, then layer4/3, then the rest."""
        names = [k for k, _ in model.named_parameters()]
        cut = None
        for i, k in enumerate(names):
            if k.startswith("layer3."):
                cut = self.offsets[i][0]
                break
        if cut is None or nbuckets < 2:
            return [(0, self.numel)]
        return [(cut, self.numel), (0, cut)]   # late layers + head first, early layers last


class GradReducer:
    """Data-parallel gradient exchange: sum the flat gradient over the ranks of ``pg`` with one
    all-reduce per bucket (RCCL on GPUs -- backend "nccl" is RCCL on ROCm; gloo in the CPU
    tests).  Buckets go out in reverse-autograd order on a side stream so that, when the
    backward pass is split around them, the early buckets travel over xGMI while the remaining
    backward kernels run.  The division by the world size happens in the fused SGD kernel."""

    def __init__(self, flat_grad, buckets, world_size, process_group=None, force_collectives=False):
        self.flat_grad, self.buckets, self.world, self.pg = flat_grad, buckets, world_size, process_group
        # force_collectives: issue the all-reduces on a one-rank group too (a sum over one rank is the identity) -- how
        # the RCCL path (backend "nccl") is exercised on a single-GPU box (tests/test_train_gpu.py)
        self.force_collectives = bool(force_collectives)
        self.active = world_size > 1 or (process_group is not None and self.force_collectives)
        self.stream = torch.cuda.Stream() if (self.active and flat_grad.is_cuda) else None

    def buffers_like(self):
        return list(self.buckets)

    def reduce(self):
        if not self.active:
            return
        import torch.distributed as dist
        if self.stream is None:                       # CPU tensors (gloo)
            for (a, b) in self.buckets:
                dist.all_reduce(self.flat_grad[a:b], op=dist.ReduceOp.SUM, group=self.pg)
            return
        cur = torch.cuda.current_stream()
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            for (a, b) in self.buckets:
                dist.all_reduce(self.flat_grad[a:b], op=dist.ReduceOp.SUM, group=self.pg)
        cur.wait_stream(self.stream)

    def start_bucket(self, i):
        """Enqueue the all-reduce of bucket i behind everything on the current stream WITHOUT making the current
        stream wait for it: the caller keeps launching backward kernels (x3dhip.trainer: the early layers) while
        the bucket travels over xGMI.  finish() joins."""
        if not self.active:
            return
        import torch.distributed as dist
        a, b = self.buckets[i]
        if self.stream is None:
            dist.all_reduce(self.flat_grad[a:b], op=dist.ReduceOp.SUM, group=self.pg)
            return
        self.stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.stream):
            dist.all_reduce(self.flat_grad[a:b], op=dist.ReduceOp.SUM, group=self.pg)

    def finish(self):
        if self.active and self.stream is not None:
            torch.cuda.current_stream().wait_stream(self.stream)


class Trainer:
    """Optimizer-like object (``param_groups``, ``state_dict`` in torch.optim.SGD's format) that
    owns the whole training step."""

    OBJECTIVES = ("ce", "bce", "loc", "soft_ce")

    def __init__(self, model, lr, momentum=0.9, weight_decay=5e-5, process_group=None, world_size=1,
                 use_graph=False, num_steps_per_update=1, overlap=True, force_split=False, force_collectives=False,
                 objective="ce", clip_grad_norm=None, monitor=False, skip_nonfinite=False, ema_decay=None,
                 ema_warmup=True, tensor_hyper=None, nesterov=False, lars=None, optimizer="sgd", betas=(0.9, 0.999),
                 adam_eps=1e-8, lamb=None):
        """overlap: multi-rank steps are captured as two graphs around the first gradient bucket (False: single graph,
        all-reduce after the whole backward); force_split: the two-graph form on a single rank too (tests);
        force_collectives: all-reduce on a one-rank process group (the single-GPU RCCL test).  Round 4: constructor
        arguments -- nothing in this module reads the environment.

        objective: the loss the step trains with --
          "ce"  (default): mean cross entropy, labels int64 [B] / [B, 1] (train_x3d_kinetics_multigrid.py:189,259);
          "bce": task 'class', mean BCEWithLogits over [B, n_classes], labels float [B, n_classes] (multi-hot or soft
                 targets in [0, 1]; train_x3d_charades.py:177-182);
          "loc": task 'loc', (cls_loss + loc_loss) / 2 of charades_losses.charades_loc_loss on the per-frame logits,
                 labels float [B, n_classes, TL] at any TL (train_x3d_charades_loc.py:168-189); `last_losses` holds
                 (cls_loss, loc_loss) of the latest step as device tensors.
          "soft_ce": task 'class', mean softmax cross entropy against soft targets, labels float [B, n_classes]
                 (F.cross_entropy(logits, probabilities); what mixing.BatchMixer makes of int64 labels under mixup, CutMix
                 and label smoothing): the "ce" head with mixops.soft_ce in the place of ops.head_ce.
        The loss returned by train_step is the micro-batch objective; num_steps_per_update divides the gradient only.

        clip_grad_norm / monitor: either creates a gradmonitor.GradMonitor (`self.monitor`) that records per-tensor
        statistics of the gradient every update, after the all-reduce and `pre_step` and right before the SGD kernel, and,
        with clip_grad_norm = c, scales the gradient by min(1, c / (norm + 1e-6)) (torch.nn.utils.clip_grad_norm_; the norm
        is that of the all-reduced gradient / world, so every rank computes the same coefficient).  monitor: True (a ring of
        64 records) or the ring's size.  Both off (the default): no attribute, not one extra launch.  The ring is
        diagnostics, not optimizer state: state_dict() is the same either way.

        skip_nonfinite: drop an update whose gradient (after the all-reduce and `pre_step`) has a NaN or an Inf, decided and
        carried out on the device with no host sync.  Implies a monitor (a ring of 64 unless monitor= says otherwise).  The
        update becomes monitor.measure (two launches) and stepops.apply (one launch: the clipping multiply and the SGD
        arithmetic of ops.sgd_fused, bit for bit, or no store at all), in every form of the step (eager, graph, split
        graph, accumulation, data parallel: every rank measures the same all-reduced gradient and decides alike).  A
        skipped update leaves the parameters, the momentum and every split_bn.running_mean / running_var as they were
        before the step: the running statistics are saved by one launch before the forward pass of the update's first
        micro-batch and put back by one launch after `apply` (each rank its own).  num_batches_tracked is not rolled
        back: it counts forward passes, skipped ones included, and nothing reads it (the BN momentum is the fixed 0.1).
        `first` stays a host value: when the very first update is skipped, the next one runs with first=False on a
        momentum buffer of zeros, which gives the same values (fmaf(mu, 0, g) == g) and can differ only in the sign of a
        zero.  monitor.skipped() / skip_run() count on the device.  The snapshot and the counters are not optimizer state:
        state_dict() is unchanged.  Off (the default): not one launch is added.

        ema_decay / ema_warmup: ema_decay = d in [0, 1) creates a weightema.WeightEMA (`self.ema`): an exponential moving
        average of the flat parameters and of every split_bn.running_mean / running_var, updated by two launches after the
        SGD kernel (on the guarded path: after `apply` and the restore), outside every graph, in every form of the step
        (under accumulation on the updating call only; under data parallelism every rank averages the same weights, so
        the averaged weights are the same bits on every rank, and each rank averages its own statistics).  ema_warmup: the
        decay of update k is min(d, (1 + k) / (10 + k)).  With skip_nonfinite a skipped update leaves the average and its
        count untouched; without the guard a non-finite update poisons the average for good.  `with trainer.ema.applied():`
        exchanges the average with the live weights and statistics in place for validation.  The average is not part of
        state_dict(): trainer.ema.state_dict() is its own.  None (the default): no attribute, not one launch.

        `trainer.precise_bn` is a precisebn.PreciseBN over this model and process group, made on first use:
        `trainer.precise_bn.compute(batches)` recomputes the BN statistics over K training batches under the weights as they
        are (inside `ema.applied()`: the averaged ones), pooled over batches, splits and ranks, and
        `with trainer.precise_bn.applied():` exchanges them with the live statistics for validation.  Until it is first
        used there is no attribute (`'precise_bn' in vars(trainer)`; `hasattr` would make it) and not one launch, and
        state_dict() is the same either way.

        tensor_hyper / nesterov: per-tensor hyper-parameters of the update.  tensor_hyper is a dict of fnmatch pattern over
        the named_parameters() names -> dict(lr_scale= / wd_scale=), applied in order (hypergroups.recipe(model,
        wd_exempt_1d=True, head_lr_scale=10) gives the usual one: no weight decay on BatchNorm scale / shift and biases,
        the classifier at a multiple of the base rate); a pattern that matches nothing raises.  nesterov=True is Nesterov
        momentum (torch.optim.SGD's form).  Either creates a hypergroups.HyperTable (`self.hyper`) and turns the update into
        one launch of stepops.apply_groups, which reads the scales of every tensor from a device table: with skip_nonfinite
        in the place of stepops.apply (measure, apply_groups, restore), without it in the place of ops.sgd_fused after the
        monitor's observe, if there is one.  Same order as ever: after the all-reduce and `pre_step`, outside every
        captured graph, on the updating call only under accumulation, grad_scale = 1 / world; data parallel: every rank
        holds the same table, no collective is added.  param_groups stays the single base dict (its 'nesterov' key tells),
        so schedules that drive trainer.lr keep working on the base rate; state_dict() gains a top-level 'tensor_hyper'
        ({'names', 'lr_scale', 'wd_scale'}), which load_state_dict restores (ValueError on other names; a checkpoint
        without the key loads as before).  lr_scale = 0 is arithmetic, not a freeze: the momentum still moves and no
        backward pass is skipped.  Both at their defaults: no attribute, no launch, the update kernels called as before.

        lars: layer-wise adaptive rate scaling (You et al. 2017).  A float (the rate of trust eta) or dict(eta=0.001,
        eps=1e-8, clip=False, exempt_1d=True, exempt=()): every tensor's decayed gradient is multiplied by its trust ratio
        eta |w| / (|g| + wd_s |w| + eps) before the momentum (clip=True: min(ratio / lr_s, 1), apex's LARC clipping mode).
        Every parameter with ndim <= 1 gets eta = 0 -- a trust of exactly 1 -- unless exempt_1d=False; `exempt` holds
        further fnmatch patterns (one that matches nothing raises).  Creates a lars.TrustTable (`self.lars`).  The
        gradient's norms are read from the monitor's record and the scales from the hyper table, so lars implies a monitor
        (as skip_nonfinite does) and a HyperTable (as nesterov does).  The update stays one sequence: measure or observe,
        stepops.trust (two launches: the weights' sums of squares, the ratios), stepops.apply_lars in the place of
        stepops.apply_groups, the restore; with skip_nonfinite the update reads the state and the ring, without it they
        are not passed, exactly as for apply_groups.  Same place as ever: outside every captured graph, `lr` a host value,
        on the updating call only under accumulation; data parallel: every rank computes the same ratios from the same
        weights and the same all-reduced gradient, no collective is added.  state_dict() gains a top-level 'lars'
        ({'names', 'eta', 'eps', 'clip'}), which load_state_dict restores.  None (the default): no attribute, not one
        launch, the same checkpoint keys.

        optimizer / betas / adam_eps / lamb: optimizer = "sgd" (the default: everything above), "adamw" (decoupled weight
        decay, torch.optim.AdamW), "adam" (weight decay as an L2 term, torch.optim.Adam) or "lamb" (You et al. 2020: the
        AdamW direction scaled per tensor by |w| / |direction|).  Anything but "sgd" creates an adamw.AdamState
        (`self.adam`), which holds the second-moment flat buffer (fp.mom is exp_avg), and implies a HyperTable as nesterov
        does; the monitor is created only where clip_grad_norm, monitor or skip_nonfinite ask for one.  The update stays
        one sequence: measure or observe, stepops.adam (one launch) or the three LAMB launches (moments and partial sums,
        per-tensor sums and ratios, the step), the restore; with skip_nonfinite the update reads the state and the ring --
        the clipping coefficient, the skip, and the count of applied updates for the bias correction, which a skipped update
        does not advance -- without it the host counts the updates.  `momentum` is not used.  lamb: None or dict(
        exempt_1d=True, exempt=()): every parameter with ndim <= 1 is exempt from the adaptation (a trust of exactly 1)
        unless exempt_1d=False; `exempt` holds further fnmatch patterns (one that matches nothing raises).  nesterov=True or
        lars= with an adaptive optimizer raises ValueError.  Same place as ever: after the all-reduce and `pre_step`, outside
        every captured graph, on the updating call only under accumulation, grad_scale = 1 / world, no collective added.
        state_dict() takes torch.optim.AdamW's layout: state[i] = {'step', 'exp_avg', 'exp_avg_sq'} ('step' is the count of
        applied updates: reading it is the one host read, at checkpoint time only), param_groups[0] gains 'betas', 'eps' and
        'amsgrad': False, a top-level 'optimizer' holds the name and, for lamb, 'lamb' the names and the adaptation flags;
        load_state_dict restores the buffers and continues the count, and raises on a checkpoint of another optimizer.
        "sgd": no attribute, no allocation, not one launch, the same checkpoint keys.

        The Trainer re-homes the model's parameters into flat buffers (FlatParams) when it is constructed: a fine-tune
        that swaps the classifier calls model.replace_logits(n) BEFORE constructing the Trainer -- a head replaced
        afterwards is not part of the flat buffers and would not be trained."""
        if objective not in self.OBJECTIVES:
            raise ValueError("objective must be one of %s (got %r)" % (self.OBJECTIVES, objective))
        task = getattr(model, "task", "class")
        if (objective in ("bce", "soft_ce") and task != "class") or (objective == "loc" and task != "loc"):
            raise ValueError("objective %r needs a model with task %r (got task %r)"
                             % (objective, "loc" if objective == "loc" else "class", task))
        self.objective = objective
        self.last_losses = None
        self.model = model
        self.overlap, self.force_split = bool(overlap), bool(force_split)
        self.fp = FlatParams(model)
        # gradient accumulation (train_x3d_kinetics_multigrid.py:119,267-273): every train_step is one micro-batch with
        # loss / num_steps_per_update; the parameters move on every num_steps_per_update-th call
        self.num_steps_per_update = int(num_steps_per_update)
        self._micro = 0
        self.accum = torch.zeros_like(self.fp.grad) if self.num_steps_per_update > 1 else None
        self._acc_reducer = None
        self.stepped = False
        self.param_groups = [dict(lr=lr, momentum=momentum, dampening=0, weight_decay=weight_decay,
                                  nesterov=bool(nesterov), params=list(range(len(self.fp.params))))]
        self.pg = process_group
        self.world = world_size
        self.first = True
        self.use_graph = use_graph
        self._graphs = {}
        _TRAINERS.add(self)
        model._direct_grads = True      # engine writes parameter gradients straight into fp.grad
        self.reducer = GradReducer(self.fp.grad, self.fp.head_first_buckets(model), world_size, process_group,
                                   force_collectives=force_collectives)
        self.skip_nonfinite = bool(skip_nonfinite)
        self._keep = self._keep_old = None
        if clip_grad_norm is not None or monitor or self.skip_nonfinite or lars is not None:
            from .gradmonitor import GradMonitor
            ring = 64 if (monitor is True or not monitor) else int(monitor)
            self.monitor = GradMonitor(self.fp, [k for k, _ in model.named_parameters()], ring=ring,
                                       max_norm=clip_grad_norm, inv_world=1.0 / world_size)
        if optimizer not in ("sgd", "adamw", "adam", "lamb"):
            raise ValueError("optimizer must be one of 'sgd', 'adamw', 'adam', 'lamb' (got %r)" % (optimizer,))
        adaptive = optimizer != "sgd"
        if adaptive and (nesterov or lars is not None):
            raise ValueError("nesterov and lars belong to SGD: optimizer %r takes neither" % (optimizer,))
        if lamb is not None and optimizer != "lamb":
            raise ValueError("lamb= needs optimizer='lamb' (got %r)" % (optimizer,))
        if tensor_hyper is not None or nesterov or lars is not None or adaptive:
            from .hypergroups import HyperTable
            if nesterov and not float(momentum) > 0.0:
                raise ValueError("nesterov needs momentum > 0 (got %r)" % (momentum,))
            self.hyper = HyperTable(self.fp, [k for k, _ in model.named_parameters()], monitor=getattr(self, "monitor", None))
            if tensor_hyper:
                self.hyper.apply(tensor_hyper)
        if lars is not None:
            from .lars import TrustTable
            cfg = dict(eta=0.001, eps=1e-8, clip=False, exempt_1d=True, exempt=())
            if isinstance(lars, dict):
                extra = set(lars) - set(cfg)
                if extra:
                    raise ValueError("lars: unknown keys %s" % sorted(extra))
                cfg.update(lars)
            else:
                cfg["eta"] = float(lars)
            named = list(model.named_parameters())
            self.lars = TrustTable(self.fp, [k for k, _ in named], self.monitor, self.hyper, eta=cfg["eta"], eps=cfg["eps"],
                                   clip=cfg["clip"])
            if cfg["exempt_1d"]:
                self.lars.eta[[i for i, (_, p) in enumerate(named) if p.dim() <= 1]] = 0.0
            for pattern in cfg["exempt"]:
                self.lars._set(pattern, 0.0)
            self.lars.upload()
        if adaptive:
            from .adamw import AdamState
            named = list(model.named_parameters())
            self.adam = AdamState(self.fp, [k for k, _ in named], self.hyper, monitor=getattr(self, "monitor", None),
                                  mode=optimizer, betas=betas, eps=adam_eps, guarded=self.skip_nonfinite)
            self.param_groups[0].update(betas=self.adam.betas, eps=self.adam.eps, amsgrad=False)
            if optimizer == "lamb":
                cfg = dict(exempt_1d=True, exempt=())
                extra = set(lamb or {}) - set(cfg)
                if extra:
                    raise ValueError("lamb: unknown keys %s" % sorted(extra))
                cfg.update(lamb or {})
                if cfg["exempt_1d"]:
                    self.adam.adapt[[i for i, (_, p) in enumerate(named) if p.dim() <= 1]] = 0
                for pattern in cfg["exempt"]:
                    self.adam.exempt(pattern)
                self.adam.upload()
        if ema_decay is not None:
            from .weightema import WeightEMA
            self.ema = WeightEMA(self.fp, model, ema_decay, warmup=ema_warmup, monitor=getattr(self, "monitor", None))

    def __getattr__(self, name):
        # only reached when the attribute is missing: precise_bn is made on first use
        if name == "precise_bn":
            from .precisebn import PreciseBN
            self.precise_bn = PreciseBN(self.model, self.pg)
            return self.precise_bn
        raise AttributeError("%s object has no attribute %r" % (type(self).__name__, name))

    @property
    def lr(self):
        return self.param_groups[0]['lr']

    @lr.setter
    def lr(self, v):
        self.param_groups[0]['lr'] = v

    # -- pieces ---------------------------------------------------------------------------
    def _head_loss_bwd(self, pooled, y):
        """fc1 / ReLU / dropout / fc2, the objective's loss and their backward on the pooled rows [N, C5] (task 'loc':
        pooled [N, C5, T], per-frame rows), straight into the flat gradient views (x3d.py:333-343, train...:259-271):
        HIP kernels only, no autograd."""
        model = self.model
        p = float(model.dropout.p)
        rng = model._head_rng(pooled.device) if p > 0 else None
        w1 = model.fc1.weight
        w1v = w1.data.view(w1.shape[0], -1)
        outs = (w1.grad.view(w1.shape[0], -1), model.fc2.weight.grad, model.fc2.bias.grad)
        if self.objective == "loc":
            # per-frame rows in the order of x3d.ResNet.forward (row = b * T + t: the same dropout mask as model(x))
            B, C5, T = pooled.shape
            rows = pooled.permute(0, 2, 1).reshape(B * T, C5).contiguous()
            hd, logits = ops.head_fwd(rows, w1v, model.fc2.weight.data, model.fc2.bias.data, p, rng)
            if rng is not None:
                ops.head_advance_rng(rng)
            lg = logits.view(B, T, -1).permute(0, 2, 1).contiguous()                 # [B, n_classes, T]
            # (cls + loc) / 2 of train_x3d_charades_loc.py:185; the 1 / num_steps_per_update is the accumulation's
            losses, dlg = ops.loc_losses(lg, y.contiguous(), grad_scale=0.5)
            dlog = dlg.permute(0, 2, 1).contiguous().view(B * T, -1)
            drows, _, _, _ = ops.head_bwd(dlog, hd, rows, w1v, model.fc2.weight.data, p, outs=outs)
            dpooled = drows.view(B, T, C5).permute(0, 2, 1).contiguous()
            self.last_losses = (losses[0], losses[1])
            return (losses[0] + losses[1]) * 0.5, lg, dpooled
        hd, logits = ops.head_fwd(pooled, w1v, model.fc2.weight.data, model.fc2.bias.data, p, rng)
        if self.objective == "bce":
            loss, dlog = ops.head_bce(logits, y.contiguous(), 1.0, rng)
        elif self.objective == "soft_ce":
            from . import mixops
            loss, dlog = mixops.soft_ce(logits, y.contiguous(), 1.0, rng)
        else:
            loss, dlog = ops.head_ce(logits, y.reshape(-1).contiguous(), rng)
        dpooled, _, _, _ = ops.head_bwd(dlog, hd, pooled, w1v, model.fc2.weight.data, p, outs=outs)
        return loss.view(()), logits.unsqueeze(2), dpooled

    def _check_labels(self, x, y):
        """Labels of the "bce" / "soft_ce" / "loc" objectives, checked on the host before anything is launched ("ce" keeps its
        behaviour: its labels are checked by the kernels' wrappers)."""
        if self.objective == "ce":
            return
        model = self.model
        if not model.training:
            raise ValueError("objective %r trains: call model.train() first" % self.objective)
        if not isinstance(y, torch.Tensor) or y.dtype != torch.float32:
            raise ValueError("objective %r needs float32 labels (got %s)"
                             % (self.objective, getattr(y, "dtype", type(y).__name__)))
        B, C = x.shape[0], model.fc2.out_features
        if self.objective in ("bce", "soft_ce"):
            if tuple(y.shape) != (B, C):
                raise ValueError("objective %r needs labels [B, n_classes] = %s (got %s)"
                                 % (self.objective, (B, C), tuple(y.shape)))
        elif y.dim() != 3 or tuple(y.shape[:2]) != (B, C) or y.shape[2] < 1:
            raise ValueError("objective 'loc' needs labels [B, n_classes, TL] with B, n_classes = %s (got %s)"
                             % ((B, C), tuple(y.shape)))
        if y.device != x.device:
            raise ValueError("labels on %s, clips on %s" % (y.device, x.device))

    def _fwd_head(self, x, y):
        """Zero the gradients, trunk forward, head + loss + head backward: everything of a step before the trunk's
        backward.  Returns (loss, logits) and what engine.trunk_backward takes: the context, dpooled and a fresh sink."""
        from . import engine
        self.fp.grad.zero_()
        tctx = engine.TrunkContext()
        with torch.no_grad():
            pooled = engine.trunk_forward(self.model, x.contiguous().float(), True, tctx)
            loss, logits, dpooled = self._head_loss_bwd(pooled, y)                               # x3d.py:333-339
        return loss, logits, tctx, dpooled, engine._GradSink(True)

    def _fwd_bwd(self, x, y):
        from . import engine
        model = self.model
        if self.objective == "ce" and (getattr(model, "task", "class") != "class" or not model.training or not x.is_cuda):
            self.fp.grad.zero_()                # generic path through autograd (per-frame head, eval)
            logits = model(x)
            loss = F.cross_entropy(logits, y)
            loss.backward()
            return loss.detach(), logits.detach()
        loss, logits, tctx, dpooled, sink = self._fwd_head(x, y)
        model._pending_tracked += 1             # (the split form counts the step in _graphed_split)
        with torch.no_grad():
            engine.trunk_backward(model, tctx, dpooled, sink)
        return loss, logits

    def _allreduce(self):
        self.reducer.reduce()

    def _keep_table(self):
        """The keep table over split_bn.running_mean / running_var of every SubBatchNorm3d, rebuilt when the long-cycle
        switch re-created those buffers.  The table before stays referenced until the next rebuild: every launch that
        names it was enqueued on this stream before the first launch on the new one."""
        from . import stepops
        ver = self.model._bn_version
        if self._keep is None or self._keep_version != ver:
            from .weightema import running_stat_buffers
            self._keep_old = self._keep
            self._keep = stepops.KeepTable([b for _, b in running_stat_buffers(self.model)], self.fp.grad.device)
            self._keep_version = ver
        return self._keep

    def _keep_save(self):
        """Before the forward pass of an update's first micro-batch, outside every graph: the running statistics as they
        are now, whoever wrote them last."""
        ema = getattr(self, "ema", None)
        if ema is not None:
            ema.sync_layout()                # a long-cycle switch: the average restarts from the statistics while fresh
        if self.skip_nonfinite:
            from . import _steplib, stepops
            stepops.keep(self._keep_table(), self.monitor.state, _steplib.KEEP_SAVE)

    def _sgd(self, grad=None):
        self._update(grad)
        ema = getattr(self, "ema", None)
        if ema is not None:
            ema.update()                     # two launches; a skipped update is left out on the device

    def _update(self, grad=None):
        """One sequence whatever the configuration: measure or observe, the update, the restore."""
        mon = getattr(self, "monitor", None)
        hy = getattr(self, "hyper", None)
        la = getattr(self, "lars", None)
        ad = getattr(self, "adam", None)
        g = self.param_groups[0]
        guarded = self.skip_nonfinite
        w, gr, m = self.fp.flat, self.fp.grad if grad is None else grad, self.fp.mom
        arith = (g['lr'], g['momentum'], g['weight_decay'], 1.0 / self.world)
        if guarded or hy is not None:
            from . import _steplib, stepops
        if guarded:
            mon.measure(grad)                # the decision and the coefficient stay on the device
        elif mon is not None:                # statistics (and clipping) of exactly what the update is about to apply
            mon.observe(grad)                # scales the gradient in place
        if ad is not None:                   # Adam, AdamW or LAMB: both moments, the count from the state when guarded
            ad.update(w, gr, m, g['lr'], g['weight_decay'], 1.0 / self.world)
        elif la is not None:                 # trust ratios: the weights' norms, the ratios, the update that takes them
            la.compute(w, g['lr'], g['weight_decay'], 1.0 / self.world)
            stepops.apply_lars(w, gr, m, hy.tables, hy.hyper, la.trust, mon.state if guarded else None,
                               mon.ring if guarded else None, mon.R if guarded else 0, *arith, first=self.first,
                               nesterov=bool(g['nesterov']))
        elif hy is not None:                 # per-tensor scales and / or Nesterov: one launch that knows the tensors
            stepops.apply_groups(w, gr, m, hy.tables, hy.hyper, mon.state if guarded else None,
                                 mon.ring if guarded else None, mon.R if guarded else 0, *arith, first=self.first,
                                 nesterov=bool(g['nesterov']))
        elif guarded:
            stepops.apply(w, gr, m, mon.tables, mon.state, mon.ring, mon.R, *arith, first=self.first)
        else:
            ops.sgd_fused(w, gr, m, *arith, first=self.first)
        if guarded:
            stepops.keep(self._keep_table(), mon.state, _steplib.KEEP_RESTORE)
        self.first = False

    # -- public -----------------------------------------------------------------------------
    def step(self, x, y):
        """One optimizer step on clips x[B,3,T,H,W], labels y (objective "ce": [B, 1] int64; "bce" / "soft_ce": float [B, n_classes];
        "loc": float [B, n_classes, TL]).  Returns (loss, logits)."""
        return self.train_step(x, y)

    def train_step(self, x, y, pre_step=None):
        """forward + CE + backward (+ all-reduce) + SGD.  ``pre_step`` runs after backward and
        before the parameter update (where the reference calls lr_warmup, train...:274).  With num_steps_per_update = K > 1
        every call is one micro-batch: its gradient / K is added to the accumulation buffer, and only the K-th call
        all-reduces, runs ``pre_step`` and updates the parameters (``self.stepped`` tells which kind of call it was)."""
        self._check_labels(x, y)
        if self.num_steps_per_update > 1:
            return self._train_step_accum(x, y, pre_step)
        self.stepped = True
        self._keep_save()
        if self.use_graph and self._overlap():
            loss, logits = self._graphed_split(x, y)        # all-reduce issued inside, overlapped with the early layers
        else:
            if self.use_graph:
                loss, logits = self._graphed_fwd_bwd(x, y)
            else:
                loss, logits = self._fwd_bwd(x, y)
            self._allreduce()
        if pre_step is not None:
            pre_step()
        self._sgd()                          # outside any graph: lr / first-step flag are host values
        return loss, logits

    @staticmethod
    def _feed(ent, x, y):
        """Hand a batch to a captured graph: copied into the graph's static input tensors -- unless the caller already wrote
        it there (`static_inputs`): a device-side input pipeline (kinetics_multigrid.DeviceVideoKinetics(out=...)) or a
        benchmark that keeps its synthetic clips resident fills the static buffers directly and no copy is made."""
        if x.data_ptr() != ent["x"].data_ptr():
            ent["x"].copy_(x)
        if y.data_ptr() != ent["y"].data_ptr():
            ent["y"].copy_(y)

    def static_inputs(self, x_shape):
        """(clips, labels) tensors the captured graph(s) of this clip shape read, or None before the first step of that
        shape: write the next batch into them and pass them to train_step to skip the input copy."""
        shp = tuple(x_shape)
        for key, ent in self._graphs.items():
            if (key[0] == "split" and key[1] == shp) or key[0] == shp:
                return ent["x"], ent["y"]
        return None

    MAX_GRAPHS = 6      # shapes of one long cycle: 2-3 (cycle_batch_sampler.py:98-111); each graph pins its activations

    def _lookup(self, key):
        """Graph cache: entries captured under an older split-BN layout point at split_bn buffers that
        update_bn_splits_long_cycle has since re-created (x3d.py:298-303) -- they are dropped as soon as the version moves,
        so a long-cycle switch releases their private pools (all activations of a step) instead of stranding them; the
        cache is also bounded (least recently used first)."""
        ver = self.model._bn_version
        if getattr(self, "_graphs_version", ver) != ver and self._graphs:
            self.invalidate_graphs()
        self._graphs_version = ver
        ent = self._graphs.pop(key, None)
        if ent is not None:
            self._graphs[key] = ent             # most recently used last
        return ent

    def _store(self, key, ent):
        while len(self._graphs) >= self.MAX_GRAPHS:
            self._graphs.pop(next(iter(self._graphs)))
        self._graphs[key] = ent

    def _train_step_accum(self, x, y, pre_step):
        K = self.num_steps_per_update
        if self._micro == 0:
            self._keep_save()
        loss, logits = self._graphed_fwd_bwd(x, y) if self.use_graph else self._fwd_bwd(x, y)
        ops.grad_accumulate(self.accum, self.fp.grad, 1.0 / K, first=self._micro == 0)
        self._micro += 1
        self.stepped = self._micro == K
        if self.stepped:
            self._micro = 0
            if self.reducer.active:
                # one exchange per optimizer step, on the accumulated gradient (no overlap with a backward pass here)
                if self._acc_reducer is None:
                    self._acc_reducer = GradReducer(self.accum, self.reducer.buffers_like(), self.world, self.pg,
                                                    force_collectives=self.reducer.force_collectives)
                self._acc_reducer.reduce()
            if pre_step is not None:
                pre_step()
            self._sgd(self.accum)
        return loss, logits

    def _objective_key(self, y):
        """Graph-cache key suffix: the "ce" key is unchanged; the other objectives add the label shape (TL of "loc" may
        change between batches of one clip shape)."""
        return () if self.objective == "ce" else (self.objective, tuple(y.shape))

    def _replayed(self, ent):
        if "losses" in ent:
            self.last_losses = ent["losses"]

    def _graphed_fwd_bwd(self, x, y):
        key = (tuple(x.shape), self.model._bn_version, self.model.training) + self._objective_key(y)
        ent = self._lookup(key)
        if ent is None:
            ent = self._capture(x, y, self._fwd_bwd)
            self._store(key, ent)
        self._feed(ent, x, y)
        ent["fb"].replay()
        self._replayed(ent)
        self.model._pending_tracked += 1     # the replayed forward advanced every split-BN once
        return ent["loss"], ent["logits"]

    # -- data parallel: backward captured as two graphs around the first gradient bucket ---------
    def _overlap(self):
        """Split capture is used for multi-rank runs (Trainer(overlap=False) disables it; force_split=True enables it on a
        single rank for tests), task 'class', with the two-bucket layout."""
        if not self.overlap or len(self.reducer.buckets) != 2:
            return False
        if self.objective == "ce" and getattr(self.model, "task", "class") != "class":
            return False
        if not self.model.training:
            return False
        return self.world > 1 or self.force_split

    def _fwd_bwd_late(self, x, y):
        """Graph A: zero grads, forward, loss, head backward, trunk backward of conv5 / layer4 / layer3."""
        from . import engine
        loss, logits, tctx, dpooled, sink = self._fwd_head(x, y)
        with torch.no_grad():
            state = engine.trunk_backward(self.model, tctx, dpooled, sink, part="late")
        return loss, logits, tctx, sink, state

    def _bwd_early(self, tctx, sink, state):
        """Graph B: trunk backward of layer2 / layer1 / stem."""
        from . import engine
        engine.trunk_backward(self.model, tctx, None, sink, part="early", state=state)

    def _graphed_split(self, x, y):
        key = ("split", tuple(x.shape), self.model._bn_version) + self._objective_key(y)
        ent = self._lookup(key)
        if ent is None:
            ent = self._capture(x, y, self._fwd_bwd_late, self._bwd_early)
            self._store(key, ent)
        self._feed(ent, x, y)
        ent["ga"].replay()
        self.reducer.start_bucket(0)          # head + layer4 + layer3 gradients: on the wire while graph B runs
        ent["gb"].replay()
        self._replayed(ent)
        self.reducer.start_bucket(1)
        self.reducer.finish()
        self.model._pending_tracked += 1
        return ent["loss"], ent["logits"]

    def invalidate_graphs(self):
        """Captured graphs hold pointers to split_bn buffers: drop them when those are re-created
        (update_bn_splits_long_cycle) or when parameters are re-homed.  Called from the long-cycle switch
        (train_x3d_kinetics_multigrid.run) and, as a safety net, by the cache lookup when the BN version moved."""
        self._graphs.clear()
        if not any(t._graphs for t in _TRAINERS):
            # retired finalize-scratch blocks are shared by every graph of the process: freed only when none is left
            ops.release_retired_scratch()
        if torch.cuda.is_available():
            # hand the dropped graphs' private pools (all activations of a step per captured shape) back to the device.  This
            # synchronises the device -- at a long-cycle switch, i.e. 13 times over the whole schedule (every rank switches
            # at the same step: the sampler is deterministic in the step counter, cycle_batch_sampler.py:76-93)
            torch.cuda.empty_cache()

    def _capture(self, x, y, body, tail=None):
        """Capture a step on clones of (x, y).  body(x, y) -> (loss, logits, *keep) becomes one graph (entry key "fb").
        With `tail` (the split form) body becomes graph "ga" and tail(*keep) graph "gb" in the same pool: the caller
        starts the first gradient bucket between their replays."""
        split = tail is not None
        # thread-local capture: the process group's watchdog thread may touch the HIP runtime while we capture
        mode = "thread_local" if (split or self.world > 1) else "global"
        sx, sy = x.clone(), y.clone()
        # the warm-up and the capture run real steps: state that a step mutates is restored afterwards
        bn_state = {k: v.clone() for k, v in self.model.state_dict().items() if "running_" in k}
        pending = self.model._pending_tracked      # (state_dict() above flushed it: 0)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):                                  # allocator / lazy-init warm-up, eager
                keep = body(sx, sy)[2:]
                if split:
                    tail(*keep)
        torch.cuda.current_stream().wait_stream(s)
        ga = torch.cuda.CUDAGraph()
        with torch.cuda.graph(ga, capture_error_mode=mode):
            loss, logits, *keep = body(sx, sy)
        ent = dict(x=sx, y=sy, loss=loss, logits=logits)
        if split:
            gb = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gb, pool=ga.pool(), capture_error_mode=mode):
                tail(*keep)
            ent.update(ga=ga, gb=gb, keep=tuple(keep))
        else:
            ent["fb"] = ga
        self.model._pending_tracked = pending
        sd = self.model.state_dict()
        for k, v in bn_state.items():
            sd[k].copy_(v)
        if self.objective == "loc":
            ent["losses"] = self.last_losses      # written by the captured head: the replays refresh them
        return ent

    # -- torch.optim.SGD-compatible state (reference checkpoints, train...:185-187,286-291) ---
    def state_dict(self):
        state = {}
        ad = getattr(self, "adam", None)
        if ad is not None:
            state = ad.state_entries()
        elif not self.first:
            for i, (o, k) in enumerate(self.fp.offsets):
                state[i] = {'momentum_buffer': self.fp.mom[o:o + k].view(self.fp.params[i].shape).clone()}
        sd = {'state': state, 'param_groups': [dict(self.param_groups[0])]}
        hy = getattr(self, "hyper", None)
        if hy is not None:
            sd['tensor_hyper'] = hy.state_dict()
        la = getattr(self, "lars", None)
        if la is not None:
            sd['lars'] = la.state_dict()
        if ad is not None:
            sd['optimizer'] = ad.mode
            if ad.mode == "lamb":
                sd['lamb'] = ad.lamb_state_dict()
        return sd

    def load_state_dict(self, sd):
        ad = getattr(self, "adam", None)
        mine, theirs = "sgd" if ad is None else ad.mode, sd.get('optimizer', 'sgd')
        if mine != theirs:
            raise ValueError("load_state_dict: a checkpoint of optimizer %r into a trainer with optimizer %r" % (theirs, mine))
        g = sd['param_groups'][0]
        for k in ('lr', 'momentum', 'weight_decay'):
            if k in g:
                self.param_groups[0][k] = g[k]
        hy = getattr(self, "hyper", None)
        if hy is not None and sd.get('tensor_hyper') is not None:
            hy.load_state_dict(sd['tensor_hyper'])
        la = getattr(self, "lars", None)
        if la is not None and sd.get('lars') is not None:
            la.load_state_dict(sd['lars'])
        st = sd.get('state', {})
        if ad is not None:
            if ad.mode == "lamb" and sd.get('lamb') is not None:
                ad.load_lamb_state_dict(sd['lamb'])
            ad.load_state_entries(st)
            self.first = False
            return
        if st:
            for i, (o, k) in enumerate(self.fp.offsets):
                buf = st.get(i, st.get(str(i)))
                if buf is not None and buf.get('momentum_buffer') is not None:
                    self.fp.mom[o:o + k].copy_(buf['momentum_buffer'].reshape(-1).to(self.fp.mom.device))
            self.first = False
