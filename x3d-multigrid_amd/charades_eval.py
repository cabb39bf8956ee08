"""Validation phases of the two Charades scripts, scored by the device-resident APMeter (apmeter.py) without a host
synchronisation per batch: the losses are summed on the device and read once at the end, and the meter's rows never leave
the GPU.  In the style of train_x3d_kinetics_multigrid.validate: eval mode, `aggregate_sub_bn_stats()` first, no
gradients; the model is left in eval mode.

Data parallel: with `process_group=` every rank scores the batches it is given -- rank r of W the global batches
r, r + W, ... -- in a segment-tracking meter; the meters are gathered and merged in global batch order before value()
(apmeter.gather), and the per-batch losses are gathered and summed in global batch order, in fp32, one by one.  Every rank
then returns what one process scoring all the batches in order returns, bit for bit: the same AP, losses and row count.

Training-phase mAP needs nothing here: pass the logits that `Trainer.train_step` returns to the meter on the same stream,
before the next step overwrites them --

    loss, logits = trainer.train_step(x, y)          # objective "bce": logits [B, 157, 1]; "loc": [B, 157, T]
    tr_apm.add_logits(logits, y)                     # "bce"
    tr_apm.add_frames(logits, y, masks)              # "loc"
"""
import torch

import apmeter
from apmeter import APMeter
from x3dhip import ops


def sum_in_global_order(per_rank):
    """per_rank[r]: fp32 CPU tensor [n_r, L], the losses of rank r's batches (global batches r, r + W, ...).  Returns
    (sums fp32 [L], batches): the losses added one by one in global batch order, ((0 + l_0) + l_1) + ... as the
    single-process loop's `sums + loss` does -- fp32 addition is not associative, so the order is part of the result."""
    sums, count = None, 0
    for j in range(max([int(t.shape[0]) for t in per_rank] + [0])):
        for t in per_rank:
            if j < t.shape[0]:
                row = t[j].to(torch.float32)
                sums = row.clone() if sums is None else sums + row
                count += 1
    return sums, count


def _gather_losses(losses, width, dev, process_group):
    """All ranks' per-batch loss vectors (a list of device tensors [width]) -> per_rank for sum_in_global_order."""
    import torch.distributed as dist
    world = dist.get_world_size(process_group)
    cdev = dev if dist.get_backend(process_group) == "nccl" else torch.device("cpu")
    n = torch.tensor([len(losses)], dtype=torch.int64, device=cdev)
    counts = torch.zeros((world, 1), dtype=torch.int64, device=cdev)
    dist.all_gather(list(counts.unbind(0)), n, group=process_group)
    counts = [int(c) for c in counts.cpu().view(-1)]
    mine = torch.zeros((max(counts + [1]), width), dtype=torch.float32, device=cdev)
    if losses:
        mine[:len(losses)].copy_(torch.stack([l.reshape(width) for l in losses]))
    out = torch.zeros((world,) + tuple(mine.shape), dtype=torch.float32, device=cdev)
    dist.all_gather(list(out.unbind(0)), mine, group=process_group)
    out = out.cpu()
    return [out[r, :counts[r]] for r in range(world)]


def _meter(meter, process_group):
    if process_group is None:
        return APMeter() if meter is None else meter
    if meter is None:
        return APMeter(track_segments=True)
    if not meter._track:
        raise ValueError("validation over a process group needs an APMeter(track_segments=True)")
    return meter


def _result(meter, sums, num_iter, names, process_group=None, losses=None, dev=None):
    if process_group is not None:
        meter = apmeter.gather(meter, process_group)
        sums, num_iter = sum_in_global_order(_gather_losses(losses, len(names), dev, process_group))
    ap = meter.value()
    out = {}
    host = sums.cpu() if sums is not None else torch.zeros(len(names))
    for i, name in enumerate(names):
        out[name] = float(host[i]) / max(num_iter, 1)
    if not torch.is_tensor(ap):                     # an empty meter
        ap = torch.zeros(0)
    out["ap"] = ap
    out["map"] = float(ap.mean()) if ap.numel() else 0.0
    out["rows"] = int(meter._bound)                 # exact after value()
    return out


def validate_cls(model, batches, meter=None, process_group=None):
    """Validation phase of train_x3d_charades.py (:135-183, :208-213): every batch is (inputs [b, n, 3, T, H, W],
    labels [b, K] multi-hot); the b*n clips run as one batch, the scores of a video are the max over its n crops of the
    sigmoid, and the loss is BCEWithLogits of the max logits.  Returns {"cls_loss", "loss", "map", "ap", "rows"}
    (losses averaged over batches; "ap" a CPU FloatTensor [K]; "rows" the meter's row count).  process_group: see the
    module docstring (the result is that of all ranks' batches)."""
    meter = _meter(meter, process_group)
    model.train(False)
    model.aggregate_sub_bn_stats()
    sums, num_iter, kept = None, 0, []
    with torch.no_grad():
        for inputs, labels in batches:
            num_iter += 1
            b, n, c, t, h, w = inputs.shape
            logits = model(inputs.reshape(b * n, c, t, h, w))                       # [b*n, K, 1]
            labels = labels.to(logits.device, torch.float32).contiguous()
            maxlogit = meter.add_logits(logits, labels, n_crops=n)                   # [b, K]
            loss, _ = ops.head_bce(maxlogit, labels)
            if process_group is not None:
                kept.append(loss.clone())
            else:
                sums = loss.clone() if sums is None else sums + loss
    res = _result(meter, sums, num_iter, ["cls_loss"], process_group, kept, next(model.parameters()).device)
    res["loss"] = res["cls_loss"]
    return res


def validate_loc(model, batches, meter=None, process_group=None):
    """Validation phase of train_x3d_charades_loc.py (:152-186, :220-225): every batch is (inputs [B, 3, T, H, W],
    labels [B, K, TL], masks [B, TL]); the per-frame logits are interpolated to TL, cls_loss / loc_loss are the script's
    BCEs (ops.loc_losses) and the rows are the masked per-frame sigmoids of the valid frames (APMeter.add_frames).
    Returns {"cls_loss", "loc_loss", "loss", "map", "ap", "rows"}; loss = (cls_loss + loc_loss) / 2 per batch.
    process_group: as validate_cls."""
    meter = _meter(meter, process_group)
    model.train(False)
    model.aggregate_sub_bn_stats()
    sums, num_iter, kept = None, 0, []
    with torch.no_grad():
        for inputs, labels, masks in batches:
            num_iter += 1
            per_frame_logits = model(inputs).contiguous()                            # [B, K, T]
            labels = labels.to(per_frame_logits.device, torch.float32).contiguous()
            masks = masks.to(per_frame_logits.device, torch.float32).contiguous()
            losses, _ = ops.loc_losses(per_frame_logits, labels)                     # (cls_loss, loc_loss)
            meter.add_frames(per_frame_logits, labels, masks)
            if process_group is not None:
                kept.append(losses.clone())
            else:
                sums = losses.clone() if sums is None else sums + losses
    res = _result(meter, sums, num_iter, ["cls_loss", "loc_loss"], process_group, kept, next(model.parameters()).device)
    res["loss"] = (res["cls_loss"] + res["loc_loss"]) / 2
    return res
