"""test_x3d_kinetics.py with the validation frames in a frame store instead of files: score a checkpoint of
train_x3d_kinetics_multigrid.py on the Kinetics validation set, the frames held as prepared JPEG scans in HBM or in
pinned host memory (x3dhip.jpegstore.FrameStore) and decoded by frame id, so that no file is opened during the pass.

    python score_x3d_kinetics_store.py --load models/x3d_multigrid_kinetics_rgb_sgd_004000.pt --resident hbm --pack val.pack
    python score_x3d_kinetics_store.py --load ... --resident host --frames-root data/kinetics/frames_val \
        --anno data/kinetics/kinetics_val.json --labels data/kinetics/labels.txt

--pack FILE is a pack written by tools/pack_frames.py (--val-windows N with N = --crops holds just the frames needed);
without it the store is filled from the frame folders.  The protocol, the printed validation line and the JSON line are
test_x3d_kinetics.py's (its evaluate()); under torch.distributed.run every rank loads and scores its own shard, the
videos rank, rank + world, ...
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frames  # noqa: E402
import test_x3d_kinetics as files_script  # noqa: E402
import train_x3d_kinetics_multigrid as tk  # noqa: E402
from kinetics import Kinetics  # noqa: E402


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--load', required=True, help='checkpoint of train_x3d_kinetics_multigrid.py')
    parser.add_argument('--resident', choices=('hbm', 'host'), default='hbm',
                        help='where the store keeps the frames: HBM, or pinned host memory')
    parser.add_argument('--pack', default=None, help='pack file of the validation set instead of --frames-root')
    parser.add_argument('--frames-root', default=None, help='root of the folders of frame_%%05d.jpg')
    parser.add_argument('--anno', default=None, help='Kinetics annotation json of the reference')
    parser.add_argument('--labels', default=None, help='class list, one name per line')
    parser.add_argument('--subset', default='validate')
    parser.add_argument('--crops', type=int, default=3, help='temporal windows per video')
    parser.add_argument('--batch', type=int, default=8, help='videos per batch and rank')
    parser.add_argument('--version', default=tk.X3D_VERSION)
    parser.add_argument('--bf16', action='store_true', help='bf16 storage of the wide bottleneck tensors (fp32 arithmetic)')
    parser.add_argument('--decode-threads', type=int, default=8, help='host threads that prepare the frames (1..16)')
    parser.add_argument('--index-bits', type=int, nargs='?', const=True, default=None,
                        help='keep a sync index of the stored frames, one entry per that many bits of scan, and Huffman decode '
                             'through it in one pass; no value: the library\'s default.  A pack with its index beside it '
                             '(PACK.idx) is used indexed without this')
    args = parser.parse_args(argv)
    if args.pack is None and (args.frames_root is None or args.anno is None or args.labels is None):
        parser.error('give --pack, or --frames-root, --anno and --labels')
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    gamma_tau = {'S': 6, 'M': 5, 'XL': 5, 'L': 5}[args.version]
    crop_size = {'S': 160, 'M': 224, 'XL': 312, 'L': 312}[args.version]
    kw = dict(root=args.frames_root, anno=args.anno, labels=args.labels, subset=args.subset, threads=args.decode_threads,
              index_bits=args.index_bits)
    stored = tk.stored_dataset(frames, args.resident, args.pack, kw, args.subset, rank, world,
                               dict(sample_duration=files_script.FRAMES, gamma_tau=gamma_tau, crop_size=crop_size, device=dev))
    dataset = Kinetics.from_dataset(stored, args.crops, sharded=(rank, world))
    return files_script.evaluate(args.load, dataset, batch=args.batch, x3d_version=args.version,
                                 act_dtype=torch.bfloat16 if args.bf16 else torch.float32)


if __name__ == '__main__':
    main()
