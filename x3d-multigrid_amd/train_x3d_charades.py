"""Charades classification fine-tuning for X3D on MI355X -- mirror of the reference's ``train_x3d_charades.py`` (constants
:37-50, run :53-215): task 'class', multi-label BCE on the clip logits, validation over 10 temporal windows per video
scored by the max over the windows.  The loop itself is charades_train.run, shared with train_x3d_charades_loc.py.

    python train_x3d_charades.py -gpu 0 --anno data/charades.json --epochs 2 --batch 8 --size 64
runs on synthetic videos of the annotation file's lengths; with --frames-root DIR every video of the annotation file that
has a folder DIR/<video id> of JPEG frames is decoded on the GPU into HBM first (frames.charades_videos), and
run(videos=...) takes decoded videos from Python.  --resident compressed keeps the videos in HBM as prepared JPEG scans
instead (x3dhip.jpegstore.FrameStore, about the size of the files: the real dataset fits one GPU that way) and decodes,
per batch, the frames the batch draws.

    python -m torch.distributed.run --nproc-per-node 8 train_x3d_charades.py --anno data/charades.json
fine-tunes on every GPU of the node: one rank per GPU over RCCL, --batch is the global batch, one mAP over all ranks' rows
(charades_train.run, process_group=).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import charades_train  # noqa: E402

BS = 16
BS_UPSCALE = 2
INIT_LR = 0.02 * BS_UPSCALE

X3D_VERSION = 'M'

CHARADES_ANNO = 'data/charades.json'
CHARADES_DATASET_SIZE = {'train': 7900, 'val': 1850}
CHARADES_MEAN = [0.413, 0.368, 0.338]
CHARADES_STD = [0.131, 0.125, 0.132]  # CALCULATED ON CHARADES TRAINING SET FOR FRAME-WISE MEANS

TASK = 'class'
SAVE_MODEL = 'models/x3d_charades_rgb_sgd_'


def run(init_lr=INIT_LR, max_epochs=100, anno=CHARADES_ANNO, batch_size=BS * BS_UPSCALE, videos=None,
        x3d_version=X3D_VERSION, load_ckpt=None, resume=None, save_model=SAVE_MODEL, save_every=1000, use_graph=True,
        num_steps_per_update=1, crop_size=None, c_size=224, dropout=0.5, seed=0, device=None, video_hw=(36, 48),
        process_group=None, rank=0, world=1, base_bn_splits=1, clip_grad_norm=None, monitor=False,
        skip_nonfinite=False, max_skip_run=8, ema_decay=None, ema_warmup=True, precise_bn=None, wd_exempt_1d=False,
        head_lr_scale=1.0, nesterov=False, lars=None, lars_clip=False, lars_eps=1e-8, optimizer_name='sgd', betas=(0.9, 0.999),
        adam_eps=1e-8):
    """The reference's run() (train_x3d_charades.py:53-215) over a charades.Charades dataset.  videos: {id: uint8 CUDA
    tensor [n, H, W, 3] or frames.StoredVideo}; None: synthetic videos of round(24 * duration) frames of video_hw noise for
    every video of the annotation file, on `device` (default cuda:0).  device: where the run takes place; it must be the
    device of the videos given.  process_group / rank / world: data parallel, one rank per GPU (init_distributed).  See
    charades_train.run for the rest."""
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


def init_distributed():
    """(process_group, rank, world, device) of a launch under torch.distributed.run (RANK / WORLD_SIZE / LOCAL_RANK): one
    rank per GPU over RCCL (backend "nccl"), as train_x3d_kinetics_multigrid.run; (None, 0, 1, cuda:0) otherwise.  The
    caller destroys the group.  Test hook: X3D_CHARADES_SINGLE_DEVICE=1 puts every rank on cuda:0 and
    X3D_CHARADES_BACKEND names another backend (gloo), to drive the multi-rank control flow on a one-GPU box."""
    import torch
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = 0 if os.environ.get("X3D_CHARADES_SINGLE_DEVICE") == "1" else int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world == 1:
        return None, 0, 1, dev
    import torch.distributed as dist
    backend = os.environ.get("X3D_CHARADES_BACKEND", "nccl")
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group(backend, rank=rank, world_size=world)
    return dist.group.WORLD, rank, world, dev


def main(run_fn, default_save):
    parser = argparse.ArgumentParser()
    parser.add_argument('-gpu', default=None, type=str, help='CUDA_VISIBLE_DEVICES')
    parser.add_argument('--anno', default=CHARADES_ANNO)
    parser.add_argument('--epochs', type=int, default=100)
    parser.add_argument('--batch', type=int, default=BS * BS_UPSCALE)
    parser.add_argument('--size', type=int, default=None, help='training and testing output size (default: 224 / the version table)')
    parser.add_argument('--load', default=None, help='Kinetics checkpoint to fine-tune from')
    parser.add_argument('--resume', default=None)
    parser.add_argument('--save', default=default_save)
    parser.add_argument('--save-every', type=int, default=1000)
    parser.add_argument('--accumulate', type=int, default=1)
    parser.add_argument('--no-graph', action='store_true')
    parser.add_argument('--version', default=X3D_VERSION)
    parser.add_argument('--frames-root', default=None, help='root of the per-video folders of JPEG frames')
    parser.add_argument('--jpeg-entropy', choices=('host', 'device'), default='host',
                        help='where the JPEG frames are Huffman decoded: host threads, or the GPU (x3djpeg_entropy_decode_batch)')
    parser.add_argument('--resident', choices=('decoded', 'compressed'), default='decoded',
                        help='how the videos of --frames-root stay in HBM: decoded whole, or as prepared JPEG scans in a frame '
                             'store, decoded batch by batch (implies the GPU Huffman decoder)')
    parser.add_argument('--index-bits', type=int, nargs='?', const=True, default=None,
                        help='with --resident compressed: keep a sync index of the stored frames, one entry per that many bits '
                             'of scan, and Huffman decode through it in one pass (x3djpeg_entropy_decode_indexed); no value: '
                             'the library\'s default')
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
                             'the GPU; every validation is also run with it (a line prefixed EMA) and checkpoints gain '
                             'ema_state_dict (off by default)')
    parser.add_argument('--no-ema-warmup', action='store_true',
                        help='with --ema-decay: use D from the first update on instead of min(D, (1 + k) / (10 + k))')
    parser.add_argument('--precise-bn', type=int, default=None, metavar='K',
                        help='before every validation recompute the BN statistics over K training batches on the GPU and '
                             'validate once more with them (a line prefixed PBN; with --ema-decay also EMA PBN); checkpoints '
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
    args = parser.parse_args()
    if args.gpu is not None:
        os.environ["CUDA_VISIBLE_DEVICES"] = args.gpu
    size = {} if args.size is None else dict(crop_size=args.size, c_size=args.size)
    pg, rank, world, dev = init_distributed()
    try:
        if args.frames_root is not None:
            import frames
            with open(args.anno, 'r') as f:
                anno = json.load(f)
            size['videos'] = frames.charades_videos(args.frames_root, anno, str(dev), entropy=args.jpeg_entropy,
                                                       resident=args.resident, index_bits=args.index_bits)
        run_fn(max_epochs=args.epochs, anno=args.anno, batch_size=args.batch, x3d_version=args.version,
               load_ckpt=args.load, resume=args.resume, save_model=args.save, save_every=args.save_every,
               use_graph=not args.no_graph, num_steps_per_update=args.accumulate, device=str(dev), process_group=pg,
               rank=rank, world=world, clip_grad_norm=args.clip_grad_norm, monitor=args.monitor or False,
               skip_nonfinite=args.skip_nonfinite, max_skip_run=args.max_skip_run, ema_decay=args.ema_decay,
               ema_warmup=not args.no_ema_warmup, precise_bn=args.precise_bn, wd_exempt_1d=args.wd_exempt_1d,
               head_lr_scale=args.head_lr_scale, nesterov=args.nesterov, lars=args.lars, lars_clip=args.lars_clip,
               lars_eps=args.lars_eps, optimizer_name=args.optimizer, betas=tuple(args.betas), adam_eps=args.adam_eps,
               **size)
    finally:
        if pg is not None:
            import torch.distributed as dist
            dist.destroy_process_group()


if __name__ == '__main__':
    main(run, SAVE_MODEL)
