"""Validation phases of the two Charades scripts, scored by the device-resident APMeter (apmeter.py) without a host
synchronisation per batch: the losses are summed on the device and read once at the end, and the meter's rows never leave
the GPU.  In the style of train_x3d_kinetics_multigrid.validate: eval mode, `aggregate_sub_bn_stats()` first, no
gradients; the model is left in eval mode.

Each process scores its own batches (under DDP, every rank's meter holds its own shard).

Training-phase mAP needs nothing here: pass the logits that `Trainer.train_step` returns to the meter on the same stream,
before the next step overwrites them --

    loss, logits = trainer.train_step(x, y)          # objective "bce": logits [B, 157, 1]; "loc": [B, 157, T]
    tr_apm.add_logits(logits, y)                     # "bce"
    tr_apm.add_frames(logits, y, masks)              # "loc"
"""
import torch

from apmeter import APMeter
from x3dhip import ops


def _result(meter, sums, num_iter, names):
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


def validate_cls(model, batches, meter=None):
    """Validation phase of train_x3d_charades.py (:135-183, :208-213): every batch is (inputs [b, n, 3, T, H, W],
    labels [b, K] multi-hot); the b*n clips run as one batch, the scores of a video are the max over its n crops of the
    sigmoid, and the loss is BCEWithLogits of the max logits.  Returns {"cls_loss", "loss", "map", "ap", "rows"}
    (losses averaged over batches; "ap" a CPU FloatTensor [K]; "rows" the meter's row count)."""
    meter = APMeter() if meter is None else meter
    model.train(False)
    model.aggregate_sub_bn_stats()
    sums, num_iter = None, 0
    with torch.no_grad():
        for inputs, labels in batches:
            num_iter += 1
            b, n, c, t, h, w = inputs.shape
            logits = model(inputs.reshape(b * n, c, t, h, w))                       # [b*n, K, 1]
            labels = labels.to(logits.device, torch.float32).contiguous()
            maxlogit = meter.add_logits(logits, labels, n_crops=n)                   # [b, K]
            loss, _ = ops.head_bce(maxlogit, labels)
            sums = loss.clone() if sums is None else sums + loss
    res = _result(meter, sums, num_iter, ["cls_loss"])
    res["loss"] = res["cls_loss"]
    return res


def validate_loc(model, batches, meter=None):
    """Validation phase of train_x3d_charades_loc.py (:152-186, :220-225): every batch is (inputs [B, 3, T, H, W],
    labels [B, K, TL], masks [B, TL]); the per-frame logits are interpolated to TL, cls_loss / loc_loss are the script's
    BCEs (ops.loc_losses) and the rows are the masked per-frame sigmoids of the valid frames (APMeter.add_frames).
    Returns {"cls_loss", "loc_loss", "loss", "map", "ap", "rows"}; loss = (cls_loss + loc_loss) / 2 per batch."""
    meter = APMeter() if meter is None else meter
    model.train(False)
    model.aggregate_sub_bn_stats()
    sums, num_iter = None, 0
    with torch.no_grad():
        for inputs, labels, masks in batches:
            num_iter += 1
            per_frame_logits = model(inputs).contiguous()                            # [B, K, T]
            labels = labels.to(per_frame_logits.device, torch.float32).contiguous()
            masks = masks.to(per_frame_logits.device, torch.float32).contiguous()
            losses, _ = ops.loc_losses(per_frame_logits, labels)                     # (cls_loss, loc_loss)
            meter.add_frames(per_frame_logits, labels, masks)
            sums = losses.clone() if sums is None else sums + losses
    res = _result(meter, sums, num_iter, ["cls_loss", "loc_loss"])
    res["loss"] = (res["cls_loss"] + res["loc_loss"]) / 2
    return res
