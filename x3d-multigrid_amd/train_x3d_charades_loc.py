"""Charades localisation fine-tuning for X3D on MI355X -- mirror of the reference's ``train_x3d_charades_loc.py``
(constants :39-51, run :54-221): task 'loc', per-frame logits interpolated to the label length, (cls_loss + loc_loss) / 2,
whole zero-padded videos with masks in validation, per-frame mAP.  The loop itself is charades_train.run, shared with
train_x3d_charades.py.

    python train_x3d_charades_loc.py -gpu 0 --anno data/charades.json --epochs 2 --batch 8 --size 64
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import charades_train  # noqa: E402
import train_x3d_charades as _cls  # noqa: E402

BS = 16
BS_UPSCALE = 2
INIT_LR = 0.02 * BS_UPSCALE

X3D_VERSION = 'M'

CHARADES_ANNO = 'data/charades.json'
CHARADES_DATASET_SIZE = {'train': 7900, 'val': 1850}
CHARADES_MEAN = [0.413, 0.368, 0.338]
CHARADES_STD = [0.131, 0.125, 0.132]  # CALCULATED ON CHARADES TRAINING SET FOR FRAME-WISE MEANS

TASK = 'loc'
SAVE_MODEL = 'models/x3d_charades_loc_rgb_sgd_'


def run(init_lr=INIT_LR, max_epochs=100, anno=CHARADES_ANNO, batch_size=BS * BS_UPSCALE, videos=None,
        x3d_version=X3D_VERSION, load_ckpt=None, resume=None, save_model=SAVE_MODEL, save_every=1000, use_graph=True,
        num_steps_per_update=1, crop_size=None, c_size=224, dropout=0.5, seed=0, device=None, video_hw=(36, 48),
        process_group=None, rank=0, world=1, base_bn_splits=1, clip_grad_norm=None, monitor=False,
        skip_nonfinite=False, max_skip_run=8, ema_decay=None, ema_warmup=True, precise_bn=None, wd_exempt_1d=False,
        head_lr_scale=1.0, nesterov=False, lars=None, lars_clip=False, lars_eps=1e-8, optimizer_name='sgd', betas=(0.9, 0.999),
        adam_eps=1e-8):
    """The reference's run() (train_x3d_charades_loc.py:54-221) over a charades.Charades dataset with task='loc'.
    Arguments as train_x3d_charades.run."""
    if not isinstance(anno, dict):
        with open(anno, 'r') as f:
            anno = json.load(f)
    if videos is None:
        videos = charades_train.synthetic_videos(anno, device or 'cuda:0', video_hw[0], video_hw[1], seed)
    return charades_train.run(TASK, anno, videos, init_lr, max_epochs, batch_size, save_model, x3d_version=x3d_version,
                              load_ckpt=load_ckpt, resume=resume, save_every=save_every, use_graph=use_graph,
                              num_steps_per_update=num_steps_per_update, crop_size=crop_size, c_size=c_size,
                              dropout=dropout, seed=seed, device=device, process_group=process_group, rank=rank,
                              world=world, base_bn_splits=base_bn_splits, clip_grad_norm=clip_grad_norm, monitor=monitor,
                              skip_nonfinite=skip_nonfinite, max_skip_run=max_skip_run, ema_decay=ema_decay,
                              ema_warmup=ema_warmup, precise_bn=precise_bn, wd_exempt_1d=wd_exempt_1d,
                              head_lr_scale=head_lr_scale, nesterov=nesterov, lars=lars, lars_clip=lars_clip,
                              lars_eps=lars_eps, optimizer_name=optimizer_name, betas=betas, adam_eps=adam_eps)


if __name__ == '__main__':
    _cls.main(run, SAVE_MODEL)
