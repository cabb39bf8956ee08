"""Multigrid training entry point for X3D on MI355X -- mirror of the reference's
``train_x3d_kinetics_multigrid.py`` for the hot path (constants :49-61, setup_data :64-105,
run :108-296, lr_warmup :300-305, print_stats :308-315).

What is the same: the module constants and their meaning, the long-cycle switch (BN splits
re-created, LR scaled by LONG_CYCLE on (re)start / last cycle and LONG_CYCLE_LR_SCALE otherwise),
warm-up towards the *scaled* LR, MultiStepLR milestones with the second-to-last moved to the
middle of the last phase, SGD(momentum .9, wd 5e-5 on every parameter), CE on logits[B,C,1],
checkpoints {'model_state_dict','optimizer_state_dict','scheduler_state_dict','long_ind'}
every 4000 steps with split-BN re-shaping before load.

What differs (MI355X-first): one process per GPU (``torch.distributed`` over RCCL) instead of
nn.DataParallel -- BATCH is split evenly over ranks, gradients are all-reduced as one flat
buffer and averaged in the fused SGD kernel; BN statistics stay rank-local exactly as
DataParallel replicas' do.  Clips are synthetic NCTHW tensors generated in HBM (``--synthetic``,
the default) or, with ``--frames-root/--anno/--labels``, come from the reference's folders of JPEG
frames: read on the host, decoded on the GPU (frames.FolderKinetics); the per-step (B,T,H,W) comes
from the same schedule arithmetic as the reference's sampler + dataset.

    python train_x3d_kinetics_multigrid.py -gpu 0 --steps 60 --iters-per-epoch 40 --max-epochs 3
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 \
        train_x3d_kinetics_multigrid.py --steps 200
    python train_x3d_kinetics_multigrid.py -gpu 0 --frames-root data/kinetics/frames \
        --anno data/kinetics/kinetics_train.json --labels data/kinetics/labels.txt
"""
import argparse
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import x3d as resnet_x3d  # noqa: E402
import cycle_batch_sampler as cbs  # noqa: E402
from kinetics_multigrid import device_batch  # noqa: E402

KINETICS_DATASET_SIZE = {'train': 220000, 'val': 17500}

BS = 8
BS_UPSCALE = 16  # CHANGE WITH GPU AVAILABILITY
INIT_LR = (1.6 / 1024) * (BS * BS_UPSCALE)
SCHEDULE_SCALE = 4
EPOCHS = (60000 * 1024 * 1.5) / 220000

LONG_CYCLE = [8, 4, 2, 1]
LONG_CYCLE_LR_SCALE = [8, 0.5, 0.5, 0.5]
GPUS = 4
BASE_BS_PER_GPU = BS * BS_UPSCALE // GPUS  # FOR SPLIT BN
CONST_BN_SIZE = 8

X3D_VERSION = 'M'  # ['S', 'M', 'XL']


def lr_schedule_milestones(num_iterations):
    """schedule[1:] with the second-to-last entry moved to the midpoint of the last phase."""
    schedule = [int(f * num_iterations) for f in (0, 0.4, 0.65, 0.85, 1)]
    milestones = list(schedule)
    milestones[-2] = (milestones[-2] + milestones[-1]) // 2
    return schedule, milestones[1:]


def setup_data(batch_size, num_steps_per_update, epochs, iterations_per_epoch, cur_iterations, crop_size,
               resize_size, num_frames, gamma_tau):
    """Returns (step-shape generator, None, lr milestones).  The generator yields
    (global_batch, long_ind, (T, H)) per optimizer step -- what the reference's
    CycleBatchSampler + DataLoader + Kinetics.__getitem__ chain produces."""
    num_iterations = int(epochs * iterations_per_epoch)
    schedule, milestones = lr_schedule_milestones(num_iterations)
    ms = cbs.MultigridSchedule(batch_size, schedule, cur_iterations, LONG_CYCLE)

    def shapes():
        for n, long_ind, task in ms.steps():
            yield n, long_ind, cbs.step_clip_shape(long_ind, task, num_frames, gamma_tau)

    return shapes(), None, milestones


def lr_warmup(init_lr, cur_steps, warmup_steps, opt):
    start_after = 1
    if start_after < cur_steps < warmup_steps:
        lr_scale = min(1., float(cur_steps + 1) / warmup_steps)
        for pg in opt.param_groups:
            pg['lr'] = lr_scale * init_lr


class MultiStepLR:
    """Chainable MultiStepLR (torch.optim.lr_scheduler.MultiStepLR semantics, train...:184):
    each ``step()`` multiplies the current lr by gamma when the new epoch is a milestone."""

    def __init__(self, opt, milestones, gamma=0.1, last_epoch=0):
        self.opt, self.milestones, self.gamma, self.last_epoch = opt, list(milestones), gamma, last_epoch

    def step(self):
        self.last_epoch += 1
        k = self.milestones.count(self.last_epoch)
        if k:
            for pg in self.opt.param_groups:
                pg['lr'] *= self.gamma ** k

    def state_dict(self):
        return {'milestones': {m: self.milestones.count(m) for m in self.milestones}, 'gamma': self.gamma,
                'last_epoch': self.last_epoch}

    def load_state_dict(self, sd):
        self.last_epoch = sd['last_epoch']
        self.gamma = sd.get('gamma', self.gamma)


def print_stats(long_ind, batch_size, stats, gamma_tau, bn_splits, lr):
    bs = batch_size * LONG_CYCLE[long_ind]
    if long_ind in [0, 1]:
        print(' ***** LR {} Frames {}/{} BS ({},{}) W/H ({},{}) BN_splits {} long_ind {} *****'.format(
            lr, stats[0], gamma_tau, bs * 2, bs, stats[2], stats[3], bn_splits, long_ind), flush=True)
    else:
        print(' ***** LR {} Frames {}/{} BS ({},{},{}) W/H ({},{},{}) BN_splits {} long_ind {} *****'.format(
            lr, stats[0], gamma_tau, bs * 4, bs * 2, bs, stats[1], stats[2], stats[3], bn_splits, long_ind), flush=True)


def validate(model, batches):
    """Validation phase of the reference loop (train_x3d_kinetics_multigrid.py:203-206, 239-266, 288-292):
    eval mode, `aggregate_sub_bn_stats()` first, no gradients; every batch is [b, n, 3, T, H, W] with n temporal crops
    per video, run as b*n clips; prediction = argmax of the crop-averaged SOFTMAX, loss = cross entropy of the
    crop-averaged LOGITS against the label.  Returns (mean loss per batch, top-1 accuracy, videos seen).
    The model is left in eval mode (the caller switches back with model.train(True), as the reference does)."""
    import torch.nn.functional as F
    model.train(False)
    model.aggregate_sub_bn_stats()
    tot_cls_loss, tot_corr, tot_dat, num_iter = 0.0, 0.0, 0, 0
    with torch.no_grad():
        for inputs, labels in batches:
            num_iter += 1
            b, n, c, t, h, w = inputs.shape
            logits = model(inputs.view(b * n, c, t, h, w))                 # [b*n, classes, 1]
            logits = logits.view(b, n, logits.shape[1], 1)
            logits_sm = torch.mean(F.softmax(logits, dim=2), 1)
            logits = torch.mean(logits, 1)
            preds = torch.max(logits_sm, 1)[1]                             # [b, 1]
            labels = labels.view(b, 1)
            tot_cls_loss += float(F.cross_entropy(logits, labels))
            tot_corr += float(torch.sum(preds == labels))
            tot_dat += b
    return tot_cls_loss / max(num_iter, 1), tot_corr / max(tot_dat, 1), tot_dat


def validate_topk(model, batches, meter=None, process_group=None):
    """The same validation phase scored by the device-resident topkmeter.TopKMeter: eval mode,
    `aggregate_sub_bn_stats()` first, no gradients, one `add_logits` per batch and no host synchronisation inside the
    loop.  Returns the meter's value() dict ("videos", "top1", "top5", "cls_loss", "loss_per_video", "class_acc",
    "mean_class_acc"); with a process_group every rank scores its own batches and the raw totals are summed over the
    ranks (topkmeter.reduce_totals), so every rank returns the figures of the whole set.  The model is left in eval
    mode."""
    import topkmeter
    meter = topkmeter.TopKMeter() if meter is None else meter
    model.train(False)
    model.aggregate_sub_bn_stats()
    with torch.no_grad():
        for inputs, labels in batches:
            b, n, c, t, h, w = inputs.shape
            meter.add_logits(model(inputs.view(b * n, c, t, h, w)), labels, n_crops=n)
    if process_group is not None:
        return topkmeter.reduce_totals(meter.totals(check=False), process_group)     # a failed meter: all ranks raise
    return meter.value()


def val_line(res):
    """The reference's validation line (train_x3d_kinetics_multigrid.py:294) extended with top-5."""
    return 'Cls Loss: {:.4f} Acc: {:.4f} Top5: {:.4f} ({} videos)'.format(res['cls_loss'], res['top1'], res['top5'],
                                                                          res['videos'])


def _save_ckpt(model, optimizer, lr_sched, long_ind, save_model, steps, pbn_ckpt=None):
    """The reference's checkpoint record (train_x3d_kinetics_multigrid.py:286-291); with a weight average
    (Trainer(ema_decay=)) also 'ema_state_dict'; pbn_ckpt: the precise-BN records of the latest validation."""
    ckpt = {'model_state_dict': model.state_dict(), 'optimizer_state_dict': optimizer.state_dict(),
            'scheduler_state_dict': lr_sched.state_dict(), 'long_ind': long_ind}
    if getattr(optimizer, 'ema', None) is not None:
        ckpt['ema_state_dict'] = optimizer.ema.state_dict()
    ckpt.update(pbn_ckpt or {})
    os.makedirs(os.path.dirname(save_model) or '.', exist_ok=True)
    torch.save(ckpt, save_model + str(steps).zfill(6) + '.pt')


TIERS = {'hbm': 'device', 'host': 'host'}       # --resident -> the tier of x3dhip.jpegstore.FrameStore


def stored_dataset(frames_mod, resident, pack, kw, subset, rank, world, common):
    """frames.StoredKinetics for --resident hbm / host: from a pack file (each rank its own shard, videos rank, rank +
    world, ...), or filled from the frame folders."""
    if resident not in TIERS:
        raise ValueError("resident must be 'files', 'hbm' or 'host' (got %r)" % (resident,))
    kw = dict(kw)
    kw.pop('entropy', None)                      # a store decodes on the GPU, Huffman stage included
    threads, index_bits = kw.pop('threads', 8), kw.pop('index_bits', None)
    if pack is not None:
        return frames_mod.StoredKinetics.from_pack(pack, tier=TIERS[resident], rank=rank, world=world,
                                                   index_bits=index_bits, **common)
    return frames_mod.StoredKinetics.from_annotation(kw.pop('root'), kw.pop('anno'), kw.pop('labels'), kw.pop('subset', subset),
                                                     tier=TIERS[resident], threads=threads, rank=rank, world=world,
                                                     index_bits=index_bits, **common, **kw)


def mixing_on(mixup=0.0, cutmix=0.0, mix_prob=None, mix_switch_prob=None, label_smoothing=0.0):
    """Does any of the mixing arguments of `run` ask for the soft-target objective."""
    return bool(mixup > 0 or cutmix > 0 or label_smoothing > 0 or mix_prob is not None or mix_switch_prob is not None)


def run(init_lr=INIT_LR, warmup_steps=8000, max_epochs=120, batch_size=BS * BS_UPSCALE, steps=0, max_steps_run=None,
        iterations_per_epoch=None, load_ckpt=None, save_model='models/x3d_multigrid_kinetics_rgb_sgd_',
        save_every=4000, use_graph=True, x3d_version=X3D_VERSION, log_every=20, val_every=None, val_batches=2,
        val_batch_size=2, val_crops=3, num_steps_per_update=1, clip_size=None, act_dtype=torch.float32,
        frames_root=None, val_frames=None, clip_grad_norm=None, monitor=False, skip_nonfinite=False, max_skip_run=8,
        ema_decay=None, ema_warmup=True, precise_bn=None, wd_exempt_1d=False, head_lr_scale=1.0, nesterov=False,
        lars=None, lars_clip=False, lars_eps=1e-8, optimizer_name='sgd', betas=(0.9, 0.999), adam_eps=1e-8,
        mixup=0.0, cutmix=0.0, mix_prob=None, mix_switch_prob=None, label_smoothing=0.0):
    """The reference's training loop (train_x3d_kinetics_multigrid.py:157-292) on synthetic clips, or on folders of JPEG
    frames: frames_root is a dict(root=, anno=, labels=[, subset='train', threads=8, entropy='host']) for
    frames.FolderKinetics.from_annotation, or a ready frames.FolderKinetics (its own crop size then sets the clip
    sizes); each step's samples are drawn by a sampler seeded per rank, its clips come from FolderKinetics.batch.  val_every: run the
    validation phase (`validate`, the reference does it after every 4 training epochs, :195) every that many steps on
    `val_batches` synthetic batches of [val_batch_size, val_crops, 3, T, H, W]; or, with val_frames -- a
    dict(root=, anno=, labels=[, subset='validate', threads=8, entropy='host']) for kinetics.Kinetics, or a ready instance -- on the
    frame folders of the validation set: every video once, val_crops temporal windows each, in batches of val_batch_size,
    sharded over the ranks and scored by `validate_topk` (top-1, top-5 and the loss, reduced over the ranks).
    num_steps_per_update: gradient accumulation over that many micro-batches per optimizer step (train...:119,267-273;
    the schedule then counts iterations and lr_schedule is divided by it, :130).  clip_size overrides the crop size of
    the shape table (tests: the default batch arithmetic at a tiny resolution).
    clip_grad_norm / monitor: Trainer(clip_grad_norm=, monitor=) -- clip the global gradient norm; record per-tensor
    gradient statistics in a device ring (True or the ring's size).  With either, the log line gains `gnorm` and `clip`, and
    rank 0 reports the first non-finite gradient (step, parameter) when the run ends, also when it ends in an exception.
    skip_nonfinite: Trainer(skip_nonfinite=True) -- an update whose gradient has a NaN or an Inf is dropped on the GPU; the
    log line gains `skipped N`, and when max_skip_run updates in a row were skipped the run stops with
    gradmonitor.SkippedRunError, which names the first non-finite gradient (checked where the loss is read).
    ema_decay / ema_warmup: Trainer(ema_decay=, ema_warmup=) -- an exponential moving average of the weights and the split-BN
    running statistics on the GPU.  Every validation is then run a second time inside `optimizer.ema.applied()` (the
    aggregation of the statistics included; the live ones are aggregated again afterwards, so that bn.* in a checkpoint are
    the live model's) and printed with the prefix EMA; checkpoints gain 'ema_state_dict', which
    load_ckpt restores when it is there (otherwise the average starts from the loaded weights).
    precise_bn: K -- before every validation the BN statistics are recomputed over K training batches at the current long
    cycle's base shape under the weights as they are (x3dhip.precisebn: pooled over batches, splits and ranks on the GPU), and
    the validation is run once more with them, printed with the prefix PBN; with ema_decay the same inside
    `optimizer.ema.applied()`: the statistics of the averaged weights, prefix EMA PBN.  The K batches come from a generator
    of their own, so the training draws -- and every printed training loss -- are the same bits with and without it.
    Checkpoints gain 'precise_bn_state_dict' (and 'ema_precise_bn_state_dict'); nothing loads them: they are derived data,
    recomputed at the next validation.
    wd_exempt_1d / head_lr_scale / nesterov: Trainer(tensor_hyper=hypergroups.recipe(model, wd_exempt_1d, head_lr_scale),
    nesterov=) -- no weight decay on the parameters with ndim <= 1, fc2.* at a multiple of the base rate, Nesterov momentum;
    the schedule keeps driving the base rate.  With any of them rank 0 prints one line before training (tensors and elements
    exempt from decay, tensors at a scaled rate) and the optimizer's state in a checkpoint gains 'tensor_hyper'.
    lars / lars_clip / lars_eps: Trainer(lars=dict(eta=lars, clip=lars_clip, eps=lars_eps)) -- layer-wise adaptive rate
    scaling: every tensor's update times its trust ratio eta |w| / (|g| + wd |w| + eps), the parameters with ndim <= 1
    exempt; lars_clip: min(ratio / lr, 1).  It implies the monitor and the hyper table, so their lines and fields appear
    too; rank 0 prints one more line before training (tensors adapted and exempt, eta, eps, clip), the log line gains
    `trust MIN/MEDIAN/MAX` over the adapted tensors, and the optimizer's state in a checkpoint gains 'lars'.
    optimizer_name / betas / adam_eps: Trainer(optimizer=, betas=, adam_eps=) -- 'adamw', 'adam' or 'lamb' in the place of SGD
    on the same flat buffers (x3dhip/adamw.py).  Rank 0 prints one more line before training (the optimizer, betas, eps, the
    tensors exempt from decay and, for lamb, from adaptation), with lamb the log line gains `trust MIN/MEDIAN/MAX`, and the
    optimizer's state in a checkpoint takes torch.optim.AdamW's layout with a top-level 'optimizer'.
    mixup / cutmix / mix_prob / mix_switch_prob / label_smoothing: any of them (an alpha or a smoothing above 0, or one of the
    probabilities given) trains with Trainer(objective="soft_ce") and puts a mixing.BatchMixer, seeded 1234 + rank, between
    every batch (synthetic or from frames) and train_step: the clips are mixed by one launch, straight into the graph's
    static input once it exists, and the labels become soft targets [B, 400].  Rank 0 prints one line before training; the
    log line's acc stays against each sample's own hard label.  The mixer's generator is not in a checkpoint: a resumed run
    restarts it from its seed.  With none of them the lines, the checkpoint keys and the bits are as before."""
    from x3dhip import hypergroups
    from x3dhip import adamw as adammod
    from x3dhip import lars as larsmod
    from x3dhip.trainer import Trainer
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    pg = None
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        pg = dist.group.WORLD

    frames = 80
    crop_size = {'S': 160, 'M': 224, 'XL': 312, 'L': 312}[x3d_version]
    resize_size = {'S': [180., 225.], 'M': [256., 256.], 'XL': [360., 450.], 'L': [360., 450.]}[x3d_version]
    gamma_tau = {'S': 6, 'M': 5, 'XL': 5, 'L': 5}[x3d_version]
    st_steps = load_steps = steps
    if batch_size % world != 0:
        raise ValueError("global batch %d is not divisible by the world size %d" % (batch_size, world))
    if iterations_per_epoch is None:
        iterations_per_epoch = KINETICS_DATASET_SIZE['train'] // batch_size
    last_long = -2

    shapes, _, lr_schedule = setup_data(batch_size, num_steps_per_update, max_epochs, iterations_per_epoch,
                                        steps * num_steps_per_update, crop_size, resize_size, frames, gamma_tau)
    lr_schedule = [i // num_steps_per_update for i in lr_schedule]          # train...:130
    total_steps = lr_schedule[-1]
    if rank == 0:
        print('Total iterations:', lr_schedule[-1] * num_steps_per_update, 'Total steps:', lr_schedule[-1])

    base_per_gpu = batch_size // world
    base_splits = max(1, base_per_gpu // CONST_BN_SIZE)
    # act_dtype=torch.bfloat16: mixed-storage mode (bf16 storage of the wide bottleneck tensors, fp32 arithmetic; not in the
    # reference, BASELINE config 5)
    model = resnet_x3d.generate_model(x3d_version=x3d_version, n_classes=400, n_input_channels=3, dropout=0.5,
                                      base_bn_splits=base_splits, act_dtype=act_dtype)
    ck = None
    if load_ckpt is not None:
        ck = torch.load(load_ckpt, map_location='cpu')
        cur_long_ind = ck['long_ind']
        model.update_bn_splits_long_cycle(LONG_CYCLE[cur_long_ind])   # split_bn buffers are [C*S]
        model.load_state_dict(ck['model_state_dict'])
        last_long = cur_long_ind
    model.to(dev).train(True)

    lr = init_lr
    optimizer = Trainer(model, lr=lr, momentum=0.9, weight_decay=5e-5, process_group=pg, world_size=world,
                        use_graph=use_graph, num_steps_per_update=num_steps_per_update, clip_grad_norm=clip_grad_norm,
                        monitor=monitor, skip_nonfinite=skip_nonfinite, ema_decay=ema_decay, ema_warmup=ema_warmup,
                        tensor_hyper=hypergroups.recipe(model, wd_exempt_1d, head_lr_scale) or None, nesterov=nesterov,
                        lars=None if lars is None else dict(eta=lars, clip=lars_clip, eps=lars_eps),
                        **(dict(optimizer=optimizer_name, betas=tuple(betas), adam_eps=adam_eps)
                           if optimizer_name != 'sgd' else {}),
                        **(dict(objective="soft_ce") if mixing_on(mixup, cutmix, mix_prob, mix_switch_prob, label_smoothing)
                           else {}))
    mixer = None
    if optimizer.objective == "soft_ce":
        from x3dhip.mixing import BatchMixer
        mixer = BatchMixer(400, mixup_alpha=mixup, cutmix_alpha=cutmix, prob=1.0 if mix_prob is None else mix_prob,
                           switch_prob=0.5 if mix_switch_prob is None else mix_switch_prob,
                           label_smoothing=label_smoothing, seed=1234 + rank)
        if rank == 0:
            print('mixing: mixup alpha {:g} cutmix alpha {:g} prob {:g} switch prob {:g} label smoothing {:g}'.format(
                mixer.mixup_alpha, mixer.cutmix_alpha, mixer.prob, mixer.switch_prob, mixer.label_smoothing))
    if rank == 0 and hasattr(optimizer, 'hyper'):
        print(hypergroups.describe(optimizer))
    if rank == 0 and lars is not None:
        print(larsmod.describe(optimizer))
    if rank == 0 and optimizer_name != 'sgd':
        print(adammod.describe(optimizer, model))
    mon = getattr(optimizer, 'monitor', None)
    ema = getattr(optimizer, 'ema', None)
    lr_sched = MultiStepLR(optimizer, lr_schedule)
    if ck is not None:
        optimizer.load_state_dict(ck['optimizer_state_dict'])
        lr_sched.load_state_dict(ck['scheduler_state_dict'])
        lr = optimizer.param_groups[0]['lr']
        if ema is not None and 'ema_state_dict' in ck:
            ema.load_state_dict(ck['ema_state_dict'])

    gen = torch.Generator(device=dev)
    gen.manual_seed(1234 + rank)
    pbn_gen = torch.Generator(device=dev)        # the precise-BN batches never touch the training draws
    pbn_gen.manual_seed(987654 + rank)
    pbn_state, pbn_ckpt = {}, {}
    folder_ds = tasks = sampler = None
    if frames_root is not None:
        import random
        import frames as frames_mod
        if isinstance(frames_root, dict):
            kw = dict(frames_root)
            common = dict(sample_duration=frames, gamma_tau=gamma_tau, crop_size=clip_size or crop_size,
                          x3d_version='XL' if x3d_version == 'L' else x3d_version, rng=random.Random(4321 + rank), device=dev)
            resident, pack = kw.pop('resident', 'files'), kw.pop('pack', None)
            if resident == 'files':
                kw.pop('index_bits', None)       # a sync index belongs to a store
                folder_ds = frames_mod.FolderKinetics.from_annotation(
                    kw.pop('root'), kw.pop('anno'), kw.pop('labels'), kw.pop('subset', 'train'), **common, **kw)
            else:
                folder_ds = stored_dataset(frames_mod, resident, pack, kw, 'train', rank, world, common)
        else:
            folder_ds = frames_root
        sampler = random.Random(1234 + rank)
        # the DataLoader task index of each step (the short-cycle counter): the same state machine as `shapes`
        sched, _ = lr_schedule_milestones(int(max_epochs * iterations_per_epoch))
        tasks = cbs.MultigridSchedule(batch_size, sched, steps * num_steps_per_update, LONG_CYCLE).steps()
    val_ds = None
    if val_frames is not None:
        import kinetics
        if isinstance(val_frames, dict):
            kw = dict(val_frames)
            resident, pack = kw.pop('resident', 'files'), kw.pop('pack', None)
            if resident == 'files':
                kw.pop('index_bits', None)       # a sync index belongs to a store
                val_ds = kinetics.Kinetics(kw.pop('root'), kw.pop('anno'), kw.pop('labels'), kw.pop('subset', 'validate'),
                                           sample_duration=frames, gamma_tau=gamma_tau, crops=val_crops,
                                           crop_size=clip_size or crop_size, device=dev, **kw)
            else:
                import frames as frames_mod
                # each rank holds its own shard, the videos rank, rank + world, ... that Kinetics.batches gives it
                val_ds = kinetics.Kinetics.from_dataset(stored_dataset(
                    frames_mod, resident, pack, kw, 'validate', rank, world,
                    dict(sample_duration=frames, gamma_tau=gamma_tau, crop_size=clip_size or crop_size, device=dev)),
                    val_crops, sharded=(rank, world))
        else:
            val_ds = val_frames

    def pbn_batches():
        """precise_bn training batches at the current long cycle's base shape (the short cycle's last task: batch
        multiplier 1, the full crop), drawn with generators of their own."""
        import random
        base_task = 1 if long_ind in (0, 1) else 2
        Tb, Hb = cbs.step_clip_shape(long_ind, base_task, frames, gamma_tau)
        if clip_size is not None:
            Hb = max(8, Hb * clip_size // {'S': 160, 'M': 224, 'XL': 312, 'L': 312}[x3d_version])
        Bb = batch_size * LONG_CYCLE[long_ind] // world
        if 'rng' not in pbn_state:
            pbn_state['rng'], pbn_state['sampler'] = random.Random(8765 + rank), random.Random(5678 + rank)
        for _ in range(precise_bn):
            if folder_ds is None:
                yield device_batch(Bb, Tb, Hb, 400, dev, pbn_gen)[0]
            else:
                picks = [pbn_state['sampler'].randrange(len(folder_ds)) for _ in range(Bb)]
                own, folder_ds.rng = folder_ds.rng, pbn_state['rng']
                try:
                    xb = folder_ds.batch(picks, base_task, long_ind)[0]
                finally:
                    folder_ds.rng = own
                yield xb

    tot_loss = tot_corr = tot_dat = 0.0
    t0 = time.time()
    clips = 0
    done = 0
    bn_splits = model.bn1.num_splits
    long_ind = max(last_long, 0)
    try:
        for n_global, long_ind, (T, H) in shapes:
            # the reference's loop ends with max_epochs (train...:192); the schedule generator itself has no end, and
            # its long-cycle lookup runs off the table one step past schedule[-1]
            if (max_steps_run is not None and done >= max_steps_run) or steps >= total_steps:
                break
            if long_ind != last_long:
                bn_splits = model.update_bn_splits_long_cycle(LONG_CYCLE[long_ind])
                optimizer.invalidate_graphs()   # captured graphs point at the split_bn buffers that were just re-created
                lr_scale_fact = LONG_CYCLE[long_ind] if (last_long == -2 or long_ind == -1) else LONG_CYCLE_LR_SCALE[long_ind]
                last_long = long_ind
                for g in optimizer.param_groups:
                    g['lr'] *= lr_scale_fact
                    lr = g['lr']
                if rank == 0:
                    fr, cr = cbs.long_cycle_shapes(frames, 224)[long_ind]
                    print_stats(long_ind, batch_size, (fr // gamma_tau, cr // 2, int(cr / 2 ** 0.5), cr), gamma_tau,
                                bn_splits, lr)
            if n_global % world != 0:
                raise ValueError("step batch %d is not divisible by the world size %d" % (n_global, world))
            B = n_global // world
            if clip_size is not None:
                H = max(8, H * clip_size // {'S': 160, 'M': 224, 'XL': 312, 'L': 312}[x3d_version])
            if folder_ds is None:
                inputs, labels = device_batch(B, T, H, 400, dev, gen)
            else:
                _, _, task = next(tasks)
                picks = [sampler.randrange(len(folder_ds)) for _ in range(B)]
                inputs, labels, _, _ = folder_ds.batch(picks, task, long_ind)
                T, H = inputs.shape[2], inputs.shape[3]
            step_in, step_lab = inputs, labels
            if mixer is not None:               # labels stays the hard label: the log line's acc is against it
                step_in, step_lab = mixer(inputs, labels,
                                          out=optimizer.static_inputs(inputs.shape) if use_graph else None)
            loss, logits = optimizer.train_step(
                step_in, step_lab, pre_step=lambda: lr_warmup(lr, steps - st_steps, warmup_steps, optimizer))
            clips += n_global
            if not optimizer.stepped:           # a micro-batch of an accumulated step (num_steps_per_update > 1)
                continue
            steps += 1
            done += 1
            lr_sched.step()
            if done % log_every == 0 or done == 1:
                tot_loss = float(loss)
                preds = logits.argmax(1)
                acc = float((preds == labels).float().mean())
                gline = '' if mon is None else ' gnorm {:.4e} clip {:.4f}'.format(float(mon.last_norm()),
                                                                                  float(mon.last_coef()))
                if skip_nonfinite:
                    gline += ' skipped {}'.format(mon.skip_report(max_skip_run))
                if lars is not None:
                    gline += ' ' + larsmod.log_field(optimizer)
                if optimizer_name == 'lamb':
                    gline += ' ' + adammod.log_field(optimizer)
                if rank == 0:
                    dt = time.time() - t0
                    print(' step {} long {} shape ({},{},{}) loss {:.4f} acc {:.3f} lr {:.5f}  {:.1f} clips/s{}'.format(
                        steps, long_ind, B, T, H, tot_loss, acc, optimizer.param_groups[0]['lr'], clips / dt, gline),
                        flush=True)
            if val_every and done % val_every == 0:
                if val_ds is not None:
                    def score():
                        return val_line(validate_topk(model, val_ds.batches(val_batch_size, rank, world), process_group=pg))
                else:
                    Tv, Hv = frames // gamma_tau, crop_size
                    vb = []
                    for _ in range(val_batches):
                        xv, yv = device_batch(val_batch_size * val_crops, Tv, Hv, 400, dev, gen)
                        vb.append((xv.view(val_batch_size, val_crops, 3, Tv, Hv, Hv), yv.view(-1)[:val_batch_size]))

                    def score():
                        return 'Cls Loss: {:.4f} Acc: {:.4f} ({} videos)'.format(*validate(model, vb))

                def report(prefix, line):
                    if prefix:
                        model.aggregate_sub_bn_stats()              # bn.* belong to the live statistics again
                    model.train(True)                               # train...:199-200
                    if rank == 0:
                        print(' {}val after step {}: {}'.format(prefix, steps, line), flush=True)

                def score_pbn(key):
                    # K training batches under the weights as they are now; after the all-gather every rank holds the same
                    # pooled statistics
                    pbn = optimizer.precise_bn.compute(pbn_batches())
                    with pbn.applied():
                        line = score()
                    pbn_ckpt[key] = pbn.state_dict()                # derived data: saved, never loaded
                    return line

                report('', score())
                if precise_bn:
                    report('PBN ', score_pbn('precise_bn_state_dict'))
                if ema is not None:
                    with ema.applied():                             # each rank scores its shard with its own statistics
                        line = score()
                    report('EMA ', line)
                    if precise_bn:
                        with ema.applied():                         # the statistics of the averaged weights
                            line = score_pbn('ema_precise_bn_state_dict')
                        report('EMA PBN ', line)
            if save_every and steps % save_every == 0 and rank == 0:
                _save_ckpt(model, optimizer, lr_sched, long_ind, save_model, steps, pbn_ckpt)
        if save_every and rank == 0 and steps >= total_steps and done > 0 and steps % save_every != 0:
            _save_ckpt(model, optimizer, lr_sched, long_ind, save_model, steps, pbn_ckpt)     # end of the schedule: final checkpoint
    finally:
        # runs on errors too: a rank that raised must not leave the others waiting inside a collective
        torch.cuda.synchronize()
        bad = mon.first_nonfinite() if (mon is not None and rank == 0) else None
        if bad is not None:
            print(' first non-finite gradient: step {} parameter {}'.format(*bad), flush=True)
        if world > 1:
            import torch.distributed as dist
            dist.destroy_process_group()
    return steps, clips / max(time.time() - t0, 1e-9)


if __name__ == '__main__':
    parser = argparse.ArgumentParser()
    parser.add_argument('-gpu', default=None, type=str, help='CUDA_VISIBLE_DEVICES (single-process runs)')
    parser.add_argument('--synthetic', action='store_true', default=True)
    parser.add_argument('--steps', type=int, default=100, help='optimizer steps to run in this invocation')
    parser.add_argument('--start-step', type=int, default=0)
    parser.add_argument('--batch', type=int, default=BS * BS_UPSCALE, help='GLOBAL base batch (reference: 128)')
    parser.add_argument('--max-epochs', type=int, default=120)
    parser.add_argument('--iters-per-epoch', type=int, default=None)
    parser.add_argument('--warmup-steps', type=int, default=8000)
    parser.add_argument('--load', default=None)
    parser.add_argument('--save-every', type=int, default=4000)
    parser.add_argument('--no-graph', action='store_true')
    parser.add_argument('--version', default=X3D_VERSION)
    parser.add_argument('--bf16', action='store_true', help='bf16 storage of the wide bottleneck tensors (fp32 arithmetic)')
    parser.add_argument('--frames-root', default=None, help='root of the folders of frame_%%05d.jpg (with --anno and --labels)')
    parser.add_argument('--anno', default=None, help='Kinetics annotation json of the reference')
    parser.add_argument('--labels', default=None, help='class list, one name per line')
    parser.add_argument('--val-frames-root', default=None, help='frame folders of the validation set (with --val-anno and '
                        '--labels): the validation phase scores them instead of synthetic clips')
    parser.add_argument('--val-anno', default=None, help='annotation json of the validation set')
    parser.add_argument('--val-every', type=int, default=None, help='validate every that many steps')
    parser.add_argument('--val-batch', type=int, default=2, help='videos per validation batch and rank')
    parser.add_argument('--val-crops', type=int, default=3, help='temporal windows per validation video')
    parser.add_argument('--decode-threads', type=int, default=8, help='host threads of the JPEG entropy stage (1..16)')
    parser.add_argument('--resident', choices=('files', 'hbm', 'host'), default='files',
                        help='where the training frames live: files read every step; or a frame store of prepared scans in '
                             'HBM (hbm) or in pinned host memory (host, for a set larger than HBM), decoded by frame id')
    parser.add_argument('--pack', default=None, help='pack file of the training set (tools/pack_frames.py) to load the store '
                                                     'from, each rank its own shard, instead of --frames-root')
    parser.add_argument('--val-resident', choices=('files', 'hbm', 'host'), default='files',
                        help='the same for the validation set')
    parser.add_argument('--val-pack', default=None, help='pack file of the validation set (tools/pack_frames.py '
                                                         '--val-windows) instead of --val-frames-root')
    parser.add_argument('--jpeg-entropy', choices=('host', 'device'), default='host',
                        help='where the JPEG frames are Huffman decoded: host threads, or the GPU (x3djpeg_entropy_decode_batch)')
    parser.add_argument('--index-bits', type=int, nargs='?', const=True, default=None,
                        help='the stores of --resident / --val-resident hbm or host keep a sync index, one entry per that many '
                             'bits of scan, and Huffman decode through it in one pass (x3djpeg_entropy_decode_indexed); no '
                             'value: the library\'s default.  A pack with its index beside it (PACK.idx) is used indexed '
                             'without this')
    parser.add_argument('--clip-grad-norm', type=float, default=None,
                        help='clip the global gradient norm to this value before every update (off by default)')
    parser.add_argument('--monitor', type=int, nargs='?', const=64, default=None, metavar='RING',
                        help='record per-tensor gradient statistics of the last RING updates on the GPU (default 64); the log '
                             'line gains gnorm and clip, and the first non-finite gradient is reported at the end')
    parser.add_argument('--skip-nonfinite', action='store_true',
                        help='drop an update whose gradient has a NaN or an Inf (decided on the GPU; implies --monitor); the '
                             'log line gains skipped')
    parser.add_argument('--max-skip-run', type=int, default=8, metavar='K',
                        help='with --skip-nonfinite: stop when K updates in a row were skipped (default 8)')
    parser.add_argument('--ema-decay', type=float, default=None, metavar='D',
                        help='keep an exponential moving average of the weights and the split-BN statistics with this decay on '
                             'the GPU; every validation is also run with it (lines prefixed EMA) and checkpoints gain '
                             'ema_state_dict (off by default)')
    parser.add_argument('--no-ema-warmup', action='store_true',
                        help='with --ema-decay: use D from the first update on instead of min(D, (1 + k) / (10 + k))')
    parser.add_argument('--precise-bn', type=int, default=None, metavar='K',
                        help='before every validation recompute the BN statistics over K training batches on the GPU and '
                             'validate once more with them (lines prefixed PBN; with --ema-decay also EMA PBN); checkpoints '
                             'gain precise_bn_state_dict (off by default)')
    parser.add_argument('--wd-exempt-1d', action='store_true',
                        help='no weight decay on BatchNorm scale / shift and biases (every parameter with ndim <= 1)')
    parser.add_argument('--head-lr-scale', type=float, default=1.0, metavar='X',
                        help='train the classifier fc2.* at X times the base learning rate (default 1)')
    parser.add_argument('--nesterov', action='store_true', help='Nesterov momentum (off by default)')
    parser.add_argument('--lars', type=float, nargs='?', const=0.001, default=None, metavar='ETA',
                        help='layer-wise adaptive rate scaling on the GPU: every tensor\'s update times eta |w| / (|g| + wd |w| '
                             '+ eps), parameters with ndim <= 1 exempt; bare: eta 0.001 (off by default)')
    parser.add_argument('--lars-clip', action='store_true', help='with --lars: min(ratio / lr, 1) (LARC clipping mode)')
    parser.add_argument('--lars-eps', type=float, default=1e-8, metavar='X', help='with --lars: eps of the ratio (default 1e-8)')
    parser.add_argument('--optimizer', choices=('sgd', 'adamw', 'adam', 'lamb'), default='sgd',
                        help='the update rule on the GPU: SGD with momentum (default), AdamW, Adam with L2, or LAMB')
    parser.add_argument('--betas', type=float, nargs=2, default=(0.9, 0.999), metavar=('B1', 'B2'),
                        help='with an adaptive --optimizer: the decay rates of the two moments (default 0.9 0.999)')
    parser.add_argument('--adam-eps', type=float, default=1e-8, metavar='X',
                        help='with an adaptive --optimizer: eps of the denominator (default 1e-8)')
    parser.add_argument('--mixup', type=float, default=0.0, metavar='A',
                        help='mixup with lam ~ Beta(A, A) on the GPU (0: off); trains against soft targets')
    parser.add_argument('--cutmix', type=float, default=0.0, metavar='A',
                        help='CutMix with lam ~ Beta(A, A), one box over all frames (0: off); trains against soft targets')
    parser.add_argument('--mix-prob', type=float, default=None, metavar='P',
                        help='probability that a batch is mixed at all (default 1)')
    parser.add_argument('--mix-switch-prob', type=float, default=None, metavar='P',
                        help='with --mixup and --cutmix: probability that a batch is CutMix (default 0.5)')
    parser.add_argument('--label-smoothing', type=float, default=0.0, metavar='E',
                        help="label smoothing (timm's rule) in the soft targets (0: off)")
    args = parser.parse_args()
    if (args.pack is not None and args.resident == 'files') or (args.val_pack is not None and args.val_resident == 'files'):
        parser.error('--pack / --val-pack is read into a store: give --resident / --val-resident hbm or host')
    frames_root = None
    if args.pack is not None:
        frames_root = dict(resident=args.resident, pack=args.pack, index_bits=args.index_bits)
    elif args.frames_root is not None:
        if args.anno is None or args.labels is None:
            parser.error('--frames-root needs --anno and --labels')
        frames_root = dict(root=args.frames_root, anno=args.anno, labels=args.labels, threads=args.decode_threads,
                           entropy=args.jpeg_entropy, resident=args.resident, index_bits=args.index_bits)
    val_frames = None
    if args.val_pack is not None:
        val_frames = dict(resident=args.val_resident, pack=args.val_pack, index_bits=args.index_bits)
    elif args.val_frames_root is not None:
        if args.val_anno is None or args.labels is None:
            parser.error('--val-frames-root needs --val-anno and --labels')
        val_frames = dict(root=args.val_frames_root, anno=args.val_anno, labels=args.labels, threads=args.decode_threads,
                          entropy=args.jpeg_entropy, resident=args.val_resident, index_bits=args.index_bits)
    if args.gpu is not None:
        os.environ["CUDA_VISIBLE_DEVICES"] = args.gpu
    run(init_lr=(1.6 / 1024) * args.batch, warmup_steps=args.warmup_steps, max_epochs=args.max_epochs,
        batch_size=args.batch, steps=args.start_step, max_steps_run=args.steps,
        iterations_per_epoch=args.iters_per_epoch, load_ckpt=args.load, save_every=args.save_every,
        use_graph=not args.no_graph, x3d_version=args.version,
        act_dtype=torch.bfloat16 if args.bf16 else torch.float32, frames_root=frames_root, val_every=args.val_every,
        val_batch_size=args.val_batch, val_crops=args.val_crops, val_frames=val_frames,
        clip_grad_norm=args.clip_grad_norm, monitor=args.monitor or False, skip_nonfinite=args.skip_nonfinite,
        max_skip_run=args.max_skip_run, ema_decay=args.ema_decay, ema_warmup=not args.no_ema_warmup,
        precise_bn=args.precise_bn, wd_exempt_1d=args.wd_exempt_1d, head_lr_scale=args.head_lr_scale,
        nesterov=args.nesterov, lars=args.lars, lars_clip=args.lars_clip, lars_eps=args.lars_eps,
        optimizer_name=args.optimizer, betas=tuple(args.betas), adam_eps=args.adam_eps,
        mixup=args.mixup, cutmix=args.cutmix, mix_prob=args.mix_prob, mix_switch_prob=args.mix_switch_prob,
        label_smoothing=args.label_smoothing)
