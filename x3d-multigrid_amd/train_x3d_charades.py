"""Charades classification fine-tuning for X3D on MI355X -- mirror of the reference's ``train_x3d_charades.py`` (constants
:37-50, run :53-215): task 'class', multi-label BCE on the clip logits, validation over 10 temporal windows per video
scored by the max over the windows.  The loop itself is charades_train.run, shared with train_x3d_charades_loc.py.

    python train_x3d_charades.py -gpu 0 --anno data/charades.json --epochs 2 --batch 8 --size 64
runs on synthetic videos of the annotation file's lengths; with --frames-root DIR every video of the annotation file that
has a folder DIR/<video id> of JPEG frames is decoded on the GPU into HBM first (frames.charades_videos), and
run(videos=...) takes decoded videos from Python.
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
        num_steps_per_update=1, crop_size=None, c_size=224, dropout=0.5, seed=0, device=None, video_hw=(36, 48)):
    """The reference's run() (train_x3d_charades.py:53-215) over a charades.Charades dataset.  videos: {id: uint8 CUDA
    tensor [n, H, W, 3]}; None: synthetic videos of round(24 * duration) frames of video_hw noise for every video of
    the annotation file, on `device` (default cuda:0).  device: where the run takes place; it must be the device of
    the videos given.  See charades_train.run for the rest."""
    if not isinstance(anno, dict):
        with open(anno, 'r') as f:
            anno = json.load(f)
    if videos is None:
        videos = charades_train.synthetic_videos(anno, device or 'cuda:0', video_hw[0], video_hw[1], seed)
    return charades_train.run(TASK, anno, videos, init_lr, max_epochs, batch_size, save_model, x3d_version=x3d_version,
                              load_ckpt=load_ckpt, resume=resume, save_every=save_every, use_graph=use_graph,
                              num_steps_per_update=num_steps_per_update, crop_size=crop_size, c_size=c_size,
                              dropout=dropout, seed=seed, device=device)


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
    args = parser.parse_args()
    if args.gpu is not None:
        os.environ["CUDA_VISIBLE_DEVICES"] = args.gpu
    size = {} if args.size is None else dict(crop_size=args.size, c_size=args.size)
    if args.frames_root is not None:
        import frames
        with open(args.anno, 'r') as f:
            anno = json.load(f)
        size['videos'] = frames.charades_videos(args.frames_root, anno, 'cuda:0', entropy=args.jpeg_entropy)
    run_fn(max_epochs=args.epochs, anno=args.anno, batch_size=args.batch, x3d_version=args.version, load_ckpt=args.load,
           resume=args.resume, save_model=args.save, save_every=args.save_every, use_graph=not args.no_graph,
           num_steps_per_update=args.accumulate, **size)


if __name__ == '__main__':
    main(run, SAVE_MODEL)
