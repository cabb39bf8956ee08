"""Score a checkpoint of train_x3d_kinetics_multigrid.py on the Kinetics validation set, the reference's protocol
(train_x3d_kinetics_multigrid.py:239-265, 293-295; kinetics.py:205-239): every video as `--crops` temporal windows, centre
crop scaled, the crop-averaged softmax for the prediction and the cross entropy of the crop-averaged logits.

    python test_x3d_kinetics.py --load models/x3d_multigrid_kinetics_rgb_sgd_004000.pt \
        --frames-root data/kinetics/frames_val --anno data/kinetics/kinetics_val.json --labels data/kinetics/labels.txt
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 test_x3d_kinetics.py --load ... (as above)

Prints the validation line and one JSON line.  Under torch.distributed.run every rank scores the videos rank,
rank + world, ... and the totals are summed over the ranks.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import x3d as resnet_x3d  # noqa: E402
import train_x3d_kinetics_multigrid as tk  # noqa: E402
from kinetics import Kinetics  # noqa: E402

FRAMES = 80


def load_model(ckpt_path, x3d_version, dev, act_dtype=torch.float32):
    """The checkpoint's model as run(load_ckpt=...) loads it: the split-BN buffers are [C * splits], so the splits of the
    checkpoint's long cycle are created before load_state_dict.  The base split count (run() derives it from the batch
    per rank) is read off the checkpoint: splits = base * LONG_CYCLE[long_ind]."""
    ck = torch.load(ckpt_path, map_location='cpu')
    sd = ck['model_state_dict']
    splits = sd['bn1.split_bn.running_mean'].numel() // sd['bn1.bn.running_mean'].numel()
    base_bn_splits = max(1, splits // tk.LONG_CYCLE[ck['long_ind']])
    model = resnet_x3d.generate_model(x3d_version=x3d_version, n_classes=400, n_input_channels=3, dropout=0.5,
                                      base_bn_splits=base_bn_splits, act_dtype=act_dtype)
    model.update_bn_splits_long_cycle(tk.LONG_CYCLE[ck['long_ind']])
    model.load_state_dict(sd)
    return model.to(dev)


def evaluate(load, dataset, batch=8, x3d_version=tk.X3D_VERSION, act_dtype=torch.float32):
    """Scores checkpoint `load` on `dataset` (a kinetics.Kinetics); returns validate_topk's dict.  Rank and world size
    come from the environment, as in run()."""
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
    try:
        model = load_model(load, x3d_version, dev, act_dtype)
        res = tk.validate_topk(model, dataset.batches(batch, rank, world), process_group=pg)
        torch.cuda.synchronize()
    finally:
        if world > 1:
            import torch.distributed as dist
            dist.destroy_process_group()
    if rank == 0:
        print(' ' + tk.val_line(res), flush=True)
        out = {k: v for k, v in res.items() if k != 'class_acc'}
        out['checkpoint'] = load
        print(json.dumps(out, sort_keys=True), flush=True)
    return res


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--load', required=True, help='checkpoint of train_x3d_kinetics_multigrid.py')
    parser.add_argument('--frames-root', default=None, help='root of the folders of frame_%%05d.jpg')
    parser.add_argument('--anno', default=None, help='Kinetics annotation json of the reference')
    parser.add_argument('--labels', default=None, help='class list, one name per line')
    parser.add_argument('--subset', default='validate')
    parser.add_argument('--crops', type=int, default=3, help='temporal windows per video')
    parser.add_argument('--batch', type=int, default=8, help='videos per batch and rank')
    parser.add_argument('--version', default=tk.X3D_VERSION)
    parser.add_argument('--bf16', action='store_true', help='bf16 storage of the wide bottleneck tensors (fp32 arithmetic)')
    parser.add_argument('--decode-threads', type=int, default=8, help='host threads of the JPEG entropy stage (1..16)')
    args = parser.parse_args(argv)
    if args.frames_root is None or args.anno is None or args.labels is None:
        parser.error('--frames-root, --anno and --labels are required')
    local = int(os.environ.get("LOCAL_RANK", "0"))
    gamma_tau = {'S': 6, 'M': 5, 'XL': 5, 'L': 5}[args.version]
    crop_size = {'S': 160, 'M': 224, 'XL': 312, 'L': 312}[args.version]
    dataset = Kinetics(args.frames_root, args.anno, args.labels, args.subset, sample_duration=FRAMES,
                       gamma_tau=gamma_tau, crops=args.crops, crop_size=crop_size,
                       device=torch.device("cuda", local), threads=args.decode_threads)
    return evaluate(args.load, dataset, batch=args.batch, x3d_version=args.version,
                    act_dtype=torch.bfloat16 if args.bf16 else torch.float32)


if __name__ == '__main__':
    main()
