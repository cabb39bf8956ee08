"""The loop the two Charades scripts share (train_x3d_charades.py:53-215, train_x3d_charades_loc.py:54-221): fine-tuning a
Kinetics model on a `charades.Charades` dataset, phases 2 * ['train'] + ['val'], training mAP from the logits
`Trainer.train_step` returns, validation through charades_eval, ReduceLROnPlateau stepped with the validation phase's
tot_loss, the reference's checkpoint record and print lines.

What differs (MI355X-first): batches are made on the device by charades.Charades (no DataLoader, no workers), the losses
are summed on the device and read where the reference prints them, the meters never leave the GPU, and one process drives
one GPU.

Several GPUs (the reference wraps the model in nn.DataParallel, GPUS = 2): one rank per GPU, run(process_group=, rank=,
world=).  Every rank shuffles with the shared seed and forms the same global batches; rank r takes the r-th contiguous
chunk of each (DataParallel's scatter) and the Trainer averages the gradients over the ranks.  Every rank draws the
augmentation parameters of the WHOLE global batch in order and uses its own slice, so the shared `rng` is consumed exactly
as by one process.  A global batch is cut to a multiple of `world`: at most world - 1 samples at the tail of an epoch are
dropped (none for world = 1, whose loop is untouched).  The training mAP is one mAP over every rank's rows in the
reference's row order (apmeter.gather), the printed losses are the mean over the ranks.  Validation: the model's buffers
are broadcast from rank 0 first -- the reference's semantics, where replica 0's BatchNorm statistics are the module's --
then rank r scores the whole batches r, r + world, ... and every rank gets the metric of the whole set
(charades_eval.validate_*(process_group=)), so ReduceLROnPlateau takes the same step everywhere.  Rank 0 alone prints and
saves.
"""
import math
import os
import random

import torch

import x3d as resnet_x3d
import apmeter
import charades_eval
from apmeter import APMeter
from charades import Charades, CHARADES_MEAN, CHARADES_STD


class ReduceLROnPlateau:
    """torch.optim.lr_scheduler.ReduceLROnPlateau restated for anything with `param_groups` (torch's class type-checks
    for a real Optimizer, and the Trainer is not one -- the reason MultiStepLR is restated in the Kinetics script).
    Semantics of torch's class for threshold_mode='rel', cooldown, min_lr and eps as given; the attributes carry torch's
    names, so `state_dict()` loads into torch's class and torch's into this one."""

    def __init__(self, optimizer, mode='min', factor=0.1, patience=10, threshold=1e-4, threshold_mode='rel', cooldown=0,
                 min_lr=0, eps=1e-8):
        if factor >= 1.0:
            raise ValueError("Factor should be < 1.0.")
        if mode not in ('min', 'max'):
            raise ValueError("mode " + str(mode) + " is unknown!")
        if threshold_mode not in ('rel', 'abs'):
            raise ValueError("threshold mode " + str(threshold_mode) + " is unknown!")
        self.factor = factor
        self.optimizer = optimizer
        if isinstance(min_lr, (list, tuple)):
            if len(min_lr) != len(optimizer.param_groups):
                raise ValueError("expected %d min_lrs, got %d" % (len(optimizer.param_groups), len(min_lr)))
            self.default_min_lr = None
            self.min_lrs = list(min_lr)
        else:
            self.default_min_lr = min_lr
            self.min_lrs = [min_lr] * len(optimizer.param_groups)
        self.patience = patience
        self.cooldown = cooldown
        self.eps = eps
        self.last_epoch = 0
        self._last_lr = [g['lr'] for g in optimizer.param_groups]
        self.mode_worse = math.inf if mode == 'min' else -math.inf
        self.mode = mode
        self.threshold = threshold
        self.threshold_mode = threshold_mode
        self.best = self.mode_worse
        self.cooldown_counter = 0
        self.num_bad_epochs = 0

    def _is_better(self, a, best):
        if self.mode == 'min' and self.threshold_mode == 'rel':
            return a < best * (1.0 - self.threshold)
        if self.mode == 'min':
            return a < best - self.threshold
        if self.threshold_mode == 'rel':
            return a > best * (self.threshold + 1.0)
        return a > best + self.threshold

    @property
    def in_cooldown(self):
        return self.cooldown_counter > 0

    def step(self, metrics):
        current = float(metrics)
        self.last_epoch += 1
        if self._is_better(current, self.best):
            self.best = current
            self.num_bad_epochs = 0
        else:
            self.num_bad_epochs += 1
        if self.in_cooldown:
            self.cooldown_counter -= 1
            self.num_bad_epochs = 0
        if self.num_bad_epochs > self.patience:
            for i, g in enumerate(self.optimizer.param_groups):
                old_lr = float(g['lr'])
                new_lr = max(old_lr * self.factor, self.min_lrs[i])
                if old_lr - new_lr > self.eps:
                    g['lr'] = new_lr
            self.cooldown_counter = self.cooldown
            self.num_bad_epochs = 0
        self._last_lr = [g['lr'] for g in self.optimizer.param_groups]

    def get_last_lr(self):
        return self._last_lr

    def state_dict(self):
        return {k: v for k, v in self.__dict__.items() if k != 'optimizer'}

    def load_state_dict(self, sd):
        self.__dict__.update(sd)
        self.mode_worse = math.inf if self.mode == 'min' else -math.inf


def synthetic_videos(anno, device, height=36, width=48, seed=0, fps=24):
    """{video id: uint8 [round(fps * duration), height, width, 3]} of noise on `device` for every video of an annotation
    dict (the scripts run on what is already in HBM; frames.charades_videos puts real frame folders there)."""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    out = {}
    for vid, rec in anno.items():
        n = int(round(fps * rec['duration']))
        out[vid] = torch.randint(0, 256, (n, height, width, 3), dtype=torch.uint8, device=device, generator=g)
    return out


def _batches(n, batch_size, order=None):
    order = list(range(n)) if order is None else order
    return [order[i:i + batch_size] for i in range(0, n, batch_size)]


def _global_batches(n, batch_size, order, world):
    """The global batches of an epoch, each cut to a multiple of `world` (an empty remainder is no batch)."""
    out = []
    for idx in _batches(n, batch_size, order):
        idx = idx[:len(idx) // world * world]
        if idx:
            out.append(idx)
    return out


def _rank_chunk(idx, rank, world):
    """The rank's contiguous chunk of a global batch (DataParallel's scatter); len(idx) is a multiple of world."""
    per = len(idx) // world
    return idx[rank * per:(rank + 1) * per]


def _rank_share(draw, idx, rank, world):
    """(indices, params) of the rank's chunk of a global batch: draw(i) is called for EVERY sample of the global batch, in
    order, as one process does (the draws consume a shared random.Random), and the rank keeps its own slice."""
    params = [draw(i) for i in idx]
    return _rank_chunk(idx, rank, world), _rank_chunk(params, rank, world)


def _broadcast(tensors, process_group):
    """In-place broadcast of `tensors` from the group's rank 0, one collective per dtype (staged through the host when
    the backend is not RCCL)."""
    import torch.distributed as dist
    src = dist.get_global_rank(process_group, 0)
    nccl = dist.get_backend(process_group) == "nccl"
    by_dtype = {}
    for t in tensors:
        by_dtype.setdefault(t.dtype, []).append(t)
    for group in by_dtype.values():
        flat = torch.cat([t.detach().reshape(-1) for t in group])
        wire = flat if nccl else flat.cpu()
        dist.broadcast(wire, src, group=process_group)
        flat = wire.to(flat.device)
        o = 0
        with torch.no_grad():
            for t in group:
                t.copy_(flat[o:o + t.numel()].view_as(t))
                o += t.numel()


def _rank_mean(values, process_group, world):
    """The mean over the ranks of a list of device scalars, as floats (one all-reduce; one synchronisation)."""
    import torch.distributed as dist
    v = torch.stack([x.reshape(()) for x in values])
    wire = v if dist.get_backend(process_group) == "nccl" else v.cpu()
    dist.all_reduce(wire, op=dist.ReduceOp.SUM, group=process_group)
    return [float(x) / world for x in wire.cpu()]


def _save_ckpt(model, optimizer, lr_sched, save_model, steps, pbn_ckpt=None):
    """The reference's checkpoint record (train_x3d_charades.py:203-207); with a weight average (Trainer(ema_decay=)) also
    'ema_state_dict'; pbn_ckpt: the precise-BN records of the latest 'val' phase."""
    ckpt = {'model_state_dict': model.state_dict(), 'optimizer_state_dict': optimizer.state_dict(),
            'scheduler_state_dict': lr_sched.state_dict()}
    if getattr(optimizer, 'ema', None) is not None:
        ckpt['ema_state_dict'] = optimizer.ema.state_dict()
    ckpt.update(pbn_ckpt or {})
    os.makedirs(os.path.dirname(save_model) or '.', exist_ok=True)
    path = save_model + str(steps).zfill(6) + '.pt'
    torch.save(ckpt, path)
    return path


def run(task, anno, videos, init_lr, max_epochs, batch_size, save_model, x3d_version='M', load_ckpt=None, resume=None,
        save_every=1000, use_graph=True, num_steps_per_update=1, crop_size=None, c_size=224, dropout=0.5, seed=0,
        device=None, process_group=None, rank=0, world=1, base_bn_splits=1, clip_grad_norm=None, monitor=False,
        skip_nonfinite=False, max_skip_run=8, ema_decay=None, ema_warmup=True, precise_bn=None, wd_exempt_1d=False,
        head_lr_scale=1.0, nesterov=False, lars=None, lars_clip=False, lars_eps=1e-8, optimizer_name='sgd', betas=(0.9, 0.999),
        adam_eps=1e-8):
    """One shared body of the two scripts' run().  task 'class': objective 'bce', validate_cls; task 'loc': objective
    'loc', validate_loc.  anno: the annotation file or its dict; videos: {id: uint8 CUDA tensor [n, H, W, 3]}.
    load_ckpt: a Kinetics checkpoint loaded before replace_logits(157); resume: a checkpoint of this loop (model,
    optimizer and scheduler state).  crop_size / c_size: the testing and training output sizes (default: the version's
    table and the reference's hard-coded 224).  Returns a dict: 'steps', 'epochs', 'phases' (one record per phase),
    'checkpoints', 'lr'.  process_group / rank / world: data parallel over that group, one rank per GPU (see the
    module docstring; batch_size is the GLOBAL batch and must be a multiple of world).  base_bn_splits: the BatchNorm
    splits of a training batch (a single process with `world` splits normalises as `world` ranks do).
    clip_grad_norm / monitor: Trainer(clip_grad_norm=, monitor=); with either, the training log line gains `gnorm` and
    `clip` (of the latest update) and rank 0 reports the first non-finite gradient when the run ends, also on an exception.
    skip_nonfinite / max_skip_run: Trainer(skip_nonfinite=True) drops an update whose gradient has a NaN or an Inf; the log
    line gains `skipped N`, and when max_skip_run updates in a row were skipped the run stops with
    gradmonitor.SkippedRunError, which names the first non-finite gradient (checked where the losses are read).
    ema_decay / ema_warmup: Trainer(ema_decay=, ema_warmup=) keeps an exponential moving average of the weights and the
    split-BN running statistics on the GPU.  Every 'val' phase is then run a second time inside `optimizer.ema.applied()`
    -- the broadcast of rank 0's buffers and the aggregation of the statistics included, so that every rank's averaged
    statistics are rank 0's afterwards, as the live ones are; the live statistics are aggregated again after the block --
    and printed with the prefix EMA (the phase record gains
    'ema_map' and 'ema_loss'; the learning-rate schedule follows the live loss alone).  Checkpoints gain
    'ema_state_dict', which `resume` restores when it is there (otherwise the average starts from the loaded weights).
    precise_bn: K -- before every 'val' phase the BN statistics are recomputed over K training batches under the weights as
    they are (x3dhip.precisebn: pooled over batches, splits and ranks on the GPU) and the phase is run once more with them
    (line prefixed PBN, the record gains 'pbn_map' and 'pbn_loss'); with ema_decay the same inside
    `optimizer.ema.applied()` (prefix EMA PBN, 'ema_pbn_map' and 'ema_pbn_loss').  The K batches are drawn with a generator
    of their own: the training draws and every printed training loss are the same bits with and without it.  Checkpoints
    gain 'precise_bn_state_dict' (and 'ema_precise_bn_state_dict') once a 'val' phase has run; nothing loads them: they are
    derived data, recomputed at the next validation.
    wd_exempt_1d / head_lr_scale / nesterov: Trainer(tensor_hyper=hypergroups.recipe(model, wd_exempt_1d, head_lr_scale),
    nesterov=) -- no weight decay on the parameters with ndim <= 1, the fresh 157-way fc2.* at a multiple of the base rate
    (which ReduceLROnPlateau keeps driving), Nesterov momentum.  With any of them rank 0 prints one line before training
    (tensors and elements exempt from decay, tensors at a scaled rate) and 'optimizer_state_dict' gains 'tensor_hyper',
    which `resume` restores.
    lars / lars_clip / lars_eps: Trainer(lars=dict(eta=lars, clip=lars_clip, eps=lars_eps)) -- layer-wise adaptive rate
    scaling, the parameters with ndim <= 1 exempt.  It implies the monitor and the hyper table, so their lines and fields
    appear too; rank 0 prints one more line before training (tensors adapted and exempt, eta, eps, clip), the training log
    line gains `trust MIN/MEDIAN/MAX` over the adapted tensors, and 'optimizer_state_dict' gains 'lars', which `resume`
    restores.
    optimizer_name / betas / adam_eps: Trainer(optimizer=, betas=, adam_eps=) -- 'adamw', 'adam' or 'lamb' in the place of SGD
    on the same flat buffers (x3dhip/adamw.py).  Rank 0 prints one more line before training (the optimizer, betas, eps, the
    tensors exempt from decay and, for lamb, from adaptation), with lamb the log line gains `trust MIN/MEDIAN/MAX`, and the
    optimizer's state in a checkpoint takes torch.optim.AdamW's layout with a top-level 'optimizer'."""
    from x3dhip import adamw as adammod
    from x3dhip import hypergroups
    from x3dhip import lars as larsmod
    from x3dhip.trainer import Trainer
    loc = task == 'loc'
    ddp = process_group is not None and world > 1
    if ddp and batch_size % world != 0:
        raise ValueError("global batch %d is not divisible by the world size %d" % (batch_size, world))
    say = print if rank == 0 else (lambda *a, **k: None)
    frames = 80                                                                  # DOUBLED INSIDE DATASET
    table_crop = {'S': 160, 'M': 224, 'XL': 312}[x3d_version]
    resize_size = {'S': [180., 225.], 'M': [256., 256.], 'XL': [360., 450.]}[x3d_version]
    gamma_tau = {'S': 6, 'M': 5, 'XL': 5}[x3d_version]                           # DOUBLED INSIDE DATASET
    crop_size = table_crop if crop_size is None else crop_size
    rng = random.Random(seed)
    steps = epochs = 0

    common = dict(task=task, frames=frames, gamma_tau=gamma_tau, crop_size=crop_size, c_size=c_size,
                  scales=[table_crop / i for i in resize_size], mean=CHARADES_MEAN, std=CHARADES_STD, rng=rng)
    dataset = Charades(anno, 'training', videos, crops=1, **common)
    val_dataset = Charades(anno, 'testing', videos, crops=10, **common)
    dev = dataset.device
    if device is not None and torch.device(device) != dev and torch.device(device) != torch.device(dev.type):
        raise ValueError("device %s was asked for, but the videos are on %s" % (device, dev))
    torch.cuda.set_device(dev)
    iterations_per_epoch = max(1, len(dataset) // batch_size)
    max_steps = iterations_per_epoch * max_epochs
    say('train', len(dataset), 'val', len(val_dataset))
    say('Total iterations:', max_steps, 'Total epochs:', max_epochs)
    say('datasets created')

    kw = dict(task='loc') if loc else {}
    x3d = resnet_x3d.generate_model(x3d_version=x3d_version, n_classes=400, n_input_channels=3, dropout=dropout,
                                    base_bn_splits=base_bn_splits, **kw)
    if load_ckpt is not None:
        x3d.load_state_dict(torch.load(load_ckpt, map_location='cpu')['model_state_dict'])
    x3d.replace_logits(157)                      # before the Trainer: FlatParams flattens the head it finds
    ck = None
    if resume is not None:
        ck = torch.load(resume, map_location='cpu')
        x3d.load_state_dict(ck['model_state_dict'])
    x3d.to(dev)
    if ddp:                                      # one model on every rank, the random 157-way head included
        x3d._flush_tracked()
        _broadcast(list(x3d.parameters()) + list(x3d.buffers()), process_group)
    say('model loaded')

    lr = init_lr
    say('INIT LR: %f' % lr)
    optimizer = Trainer(x3d, lr=lr, momentum=0.9, weight_decay=1e-5, objective='loc' if loc else 'bce',
                        use_graph=use_graph, num_steps_per_update=num_steps_per_update,
                        clip_grad_norm=clip_grad_norm, monitor=monitor, skip_nonfinite=skip_nonfinite,
                        ema_decay=ema_decay, ema_warmup=ema_warmup,
                        tensor_hyper=hypergroups.recipe(x3d, wd_exempt_1d, head_lr_scale) or None, nesterov=nesterov,
                        lars=None if lars is None else dict(eta=lars, clip=lars_clip, eps=lars_eps),
                        **(dict(optimizer=optimizer_name, betas=tuple(betas), adam_eps=adam_eps)
                           if optimizer_name != 'sgd' else {}),
                        **(dict(process_group=process_group, world_size=world) if ddp else {}))
    if hasattr(optimizer, 'hyper'):
        say(hypergroups.describe(optimizer))
    if lars is not None:
        say(larsmod.describe(optimizer))
    if optimizer_name != 'sgd':
        say(adammod.describe(optimizer, x3d))
    mon = getattr(optimizer, 'monitor', None)
    ema = getattr(optimizer, 'ema', None)
    lr_sched = ReduceLROnPlateau(optimizer, mode='min', patience=2, factor=0.1)
    if ck is not None:
        optimizer.load_state_dict(ck['optimizer_state_dict'])
        lr_sched.load_state_dict(ck['scheduler_state_dict'])
        if ema is not None and 'ema_state_dict' in ck:
            ema.load_state_dict(ck['ema_state_dict'])

    val_apm = APMeter(track_segments=ddp)
    tr_apm = APMeter(track_segments=ddp)
    pbn_rng = random.Random(seed + 7919)         # the precise-BN batches never touch the training draws
    pbn_ckpt = {}

    def pbn_batches():
        """precise_bn training batches of the global batch size, every rank its chunk, drawn with pbn_rng alone (the
        same on every rank, as `rng` is)."""
        for _ in range(precise_bn):
            own, dataset.rng = dataset.rng, pbn_rng
            try:
                idx = [pbn_rng.randrange(len(dataset)) for _ in range(batch_size)]
                if ddp:
                    mine, params = _rank_share(dataset.draw, idx, rank, world)
                    data = dataset.batch(mine, params=params)
                else:
                    data = dataset.batch(idx)
            finally:
                dataset.rng = own
            yield data[0]

    def pbn_phase(vb, key, prefix, tag):
        """The 'val' phase once more on precise BN statistics of the weights as they are.  No broadcast of rank 0's
        buffers here: after the all-gather inside compute() every rank holds the same pooled statistics."""
        pbn = optimizer.precise_bn.compute(pbn_batches())
        with pbn.applied():
            gen = (val_dataset.test_batch(idx) for idx in (vb[rank::world] if ddp else vb))
            res = (charades_eval.validate_loc if loc else charades_eval.validate_cls)(
                x3d, gen, val_apm, **(dict(process_group=process_group) if ddp else {}))
        pbn_ckpt[key] = pbn.state_dict()         # derived data: saved, never loaded
        x3d.aggregate_sub_bn_stats()             # bn.* belong to the statistics outside the block again
        val_apm.reset()
        if loc:
            say(' {} Epoch:{} {} Loc Loss: {:.4f} Cls Loss: {:.4f} Tot Loss: {:.4f} mAP: {:.4f}'.format(
                prefix, epochs, phase, res['loc_loss'], res['cls_loss'], res['loss'], res['map']))
        else:
            say(' {} Epoch:{} {} Loc Cls Loss: {:.4f} Tot Loss: {:.4f} mAP: {:.4f}'.format(
                prefix, epochs, phase, res['cls_loss'], res['loss'], res['map']))
        phases[-1].update({tag + 'map': res['map'], tag + 'loss': res['loss'] * len(vb) / num_steps_per_update})
    phases, checkpoints = [], []
    s_times = max(1, iterations_per_epoch // 2)
    zero = torch.zeros((), device=dev)
    try:
        while epochs < max_epochs:
            say('Step {} Epoch {}'.format(steps, epochs))
            say('-' * 10)
            for phase in 2 * ['train'] + ['val']:
                say(phase)
                if phase == 'train':
                    x3d.train(True)
                    epochs += 1
                    tot_loss, tot_loc_loss, tot_cls_loss = zero.clone(), zero.clone(), zero.clone()
                    order = list(range(len(dataset)))
                    rng.shuffle(order)
                    rec = dict(phase=phase, epoch=epochs, maps=[], losses=[])
                    for idx in _global_batches(len(dataset), batch_size, order, world if ddp else 1):
                        if ddp:
                            own, params = _rank_share(dataset.draw, idx, rank, world)
                            data = dataset.batch(own, params=params)
                        else:
                            data = dataset.batch(idx)
                        loss, logits = optimizer.train_step(data[0], data[1])
                        if loc:
                            tr_apm.add_frames(logits, data[1], data[2])
                            tot_cls_loss += optimizer.last_losses[0].view(())
                            tot_loc_loss += optimizer.last_losses[1].view(())
                        else:
                            tr_apm.add_logits(logits, data[1])
                            tot_cls_loss += loss.detach().view(())
                        tot_loss += loss.detach().view(()) / num_steps_per_update
                        if not optimizer.stepped:
                            continue
                        steps += 1
                        if steps % s_times == 0:
                            if ddp:
                                tr_map = float(apmeter.gather(tr_apm, process_group).value().mean())
                                tot_loss, tot_loc_loss, tot_cls_loss = _rank_mean(
                                    [tot_loss, tot_loc_loss, tot_cls_loss], process_group, world)
                            else:
                                tr_map = float(tr_apm.value().mean())
                            tr_apm.reset()
                            n = s_times * num_steps_per_update
                            gline = '' if mon is None else ' gnorm {:.4e} clip {:.4f}'.format(float(mon.last_norm()),
                                                                                              float(mon.last_coef()))
                            if skip_nonfinite:
                                gline += ' skipped {}'.format(mon.skip_report(max_skip_run))
                            if lars is not None:
                                gline += ' ' + larsmod.log_field(optimizer)
                            if optimizer_name == 'lamb':
                                gline += ' ' + adammod.log_field(optimizer)
                            if loc:
                                say(' Epoch:{} {} steps: {} Loc Loss: {:.4f} Cls Loss: {:.4f} Tot Loss: {:.4f} mAP: {:.4f}{}'
                                      .format(epochs, phase, steps, float(tot_loc_loss) / n, float(tot_cls_loss) / n,
                                              float(tot_loss) / s_times, tr_map, gline))
                            else:
                                say(' Epoch:{} {} steps: {} Cls Loss: {:.4f} Tot Loss: {:.4f} mAP: {:.4f}{}'.format(
                                    epochs, phase, steps, float(tot_cls_loss) / n, float(tot_loss) / s_times, tr_map, gline))
                            rec['maps'].append(tr_map)
                            rec['losses'].append(float(tot_loss) / s_times)
                            tot_loss, tot_loc_loss, tot_cls_loss = zero.clone(), zero.clone(), zero.clone()
                        if save_every and steps % save_every == 0 and rank == 0:
                            checkpoints.append(_save_ckpt(x3d, optimizer, lr_sched, save_model, steps, pbn_ckpt))
                    rec['steps'] = steps
                    phases.append(rec)
                else:
                    vb = _batches(len(val_dataset), max(1, batch_size // 2))
                    if ddp:                          # replica 0's running statistics are the module's
                        x3d._flush_tracked()         # num_batches_tracked is advanced lazily: bring every rank's
                        _broadcast(list(x3d.buffers()), process_group)      # buffers up to date before they are replaced
                    gen = (val_dataset.test_batch(idx) for idx in (vb[rank::world] if ddp else vb))
                    res = (charades_eval.validate_loc if loc else charades_eval.validate_cls)(
                        x3d, gen, val_apm, **(dict(process_group=process_group) if ddp else {}))
                    num_iter = len(vb)
                    tot_loss = res['loss'] * num_iter / num_steps_per_update
                    val_map = res['map']
                    lr_sched.step(tot_loss)
                    val_apm.reset()
                    if loc:
                        say(' Epoch:{} {} Loc Loss: {:.4f} Cls Loss: {:.4f} Tot Loss: {:.4f} mAP: {:.4f}'.format(
                            epochs, phase, res['loc_loss'], res['cls_loss'], (tot_loss * num_steps_per_update) / num_iter,
                            val_map))
                    else:
                        say(' Epoch:{} {} Loc Cls Loss: {:.4f} Tot Loss: {:.4f} mAP: {:.4f}'.format(
                            epochs, phase, res['cls_loss'], (tot_loss * num_steps_per_update) / num_iter, val_map))
                    phases.append(dict(phase=phase, epoch=epochs, map=val_map, loss=tot_loss, rows=res['rows'],
                                       lr=optimizer.param_groups[0]['lr'], steps=steps))
                    if precise_bn:
                        pbn_phase(vb, 'precise_bn_state_dict', 'PBN', 'pbn_')
                    if ema is not None:
                        with ema.applied():              # the same phase on the averaged weights and statistics
                            if ddp:
                                _broadcast(list(x3d.buffers()), process_group)
                            gen = (val_dataset.test_batch(idx) for idx in (vb[rank::world] if ddp else vb))
                            res = (charades_eval.validate_loc if loc else charades_eval.validate_cls)(
                                x3d, gen, val_apm, **(dict(process_group=process_group) if ddp else {}))
                        x3d.aggregate_sub_bn_stats()     # bn.* belong to the live statistics again
                        val_apm.reset()
                        if loc:
                            say(' EMA Epoch:{} {} Loc Loss: {:.4f} Cls Loss: {:.4f} Tot Loss: {:.4f} mAP: {:.4f}'.format(
                                epochs, phase, res['loc_loss'], res['cls_loss'], res['loss'], res['map']))
                        else:
                            say(' EMA Epoch:{} {} Loc Cls Loss: {:.4f} Tot Loss: {:.4f} mAP: {:.4f}'.format(
                                epochs, phase, res['cls_loss'], res['loss'], res['map']))
                        phases[-1].update(ema_map=res['map'], ema_loss=res['loss'] * num_iter / num_steps_per_update)
                        if precise_bn:
                            with ema.applied():          # the statistics of the averaged weights
                                pbn_phase(vb, 'ema_precise_bn_state_dict', 'EMA PBN', 'ema_pbn_')
    finally:
        torch.cuda.synchronize()
        bad = mon.first_nonfinite() if mon is not None else None
        if bad is not None:
            say(' first non-finite gradient: step {} parameter {}'.format(*bad))
    return dict(steps=steps, epochs=epochs, phases=phases, checkpoints=checkpoints, lr=optimizer.param_groups[0]['lr'],
                scheduler=lr_sched, optimizer=optimizer, model=x3d)
