"""Child processes of tests/test_apmerge_gpu.py and tests/test_charades_ddp_gpu.py (a process group never leaks into the
pytest session).  Modes, argv[1]:
  gather1           one-rank RCCL group: apmeter.gather equals the meter
  validate OUT      under torch.distributed.run, two ranks on cuda:0 over gloo: validate_cls / validate_loc with the group,
                    and the single-process call over all batches; writes OUT.rank<r>.json
  run OUT           under torch.distributed.run: run() of the two scripts on two ranks; writes OUT.rank<r>.json
  single OUT CKPTS  one process: run() with two BN splits (the ranks' normalisation), and the resume of a checkpoint
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "x3d-multigrid_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

NC = 157


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).tolist()


def gather1():
    import torch.distributed as dist
    import apmeter
    from apmeter import APMeter
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        g = torch.Generator().manual_seed(3)
        m = APMeter(track_segments=True)
        for n in (5, 0, 70, 1):
            m.add(torch.rand((n, 4), generator=g).to(dev), (torch.rand((n, 4), generator=g) < 0.3).float().to(dev),
                  torch.rand(n, generator=g).to(dev))
        out = apmeter.gather(m, dist.group.WORLD)
        assert not out._track and out._rows() == 76
        for a, b in ((out.scores, m.scores), (out.weights, m.weights), (out.value(), m.value())):
            assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert torch.equal(out.targets, m.targets)
        empty = apmeter.gather(APMeter(track_segments=True), dist.group.WORLD)
        assert empty.value() == 0
        try:
            apmeter.gather(APMeter(), dist.group.WORLD)
        except ValueError:
            pass
        else:
            raise AssertionError("a meter that does not track segments was gathered")
    finally:
        dist.destroy_process_group()
    print("gather1 ok")


def _model(dev, task, seed):
    import x3d
    from oracle import x3d_oracle as xo
    from x3dhip import synthetic
    net = x3d.generate_model("S", n_classes=NC, dropout=0.0, base_bn_splits=1, task=task)
    net.load_state_dict(synthetic.procedural_state_dict(xo.state_template("S", NC, 1), seed))   # random BN statistics too
    return net.to(dev)


def _pack(res):
    return {"ap": _bits(res["ap"]), "rows": res["rows"], "map": res["map"],
            "losses": {k: res[k] for k in ("cls_loss", "loc_loss", "loss") if k in res}}


def validate(out):
    import charades_eval
    import train_x3d_charades
    import torch.distributed as dist
    from x3dhip import synthetic
    pg, rank, world, dev = train_x3d_charades.init_distributed()
    try:
        T, H, n, TL = 4, 64, 3, 11
        cls_batches, loc_batches = [], []
        for i, b in enumerate((2, 1, 2, 2, 1)):               # five batches: three for rank 0, two for rank 1
            x = synthetic.synthetic_clips(b * n, T, H, H, seed=100 + i).view(b, n, 3, T, H, H).to(dev)
            y = (torch.rand((b, NC), generator=torch.Generator().manual_seed(i)) < 0.1).float().to(dev)
            cls_batches.append((x, y))
            x = synthetic.synthetic_clips(b, T, H, H, seed=200 + i).to(dev)
            y = (torch.rand((b, NC, TL), generator=torch.Generator().manual_seed(10 + i)) < 0.1).float().to(dev)
            masks = torch.ones(b, TL, device=dev)
            masks[b - 1, 4 + i:] = 0
            loc_batches.append((x, y, masks))
        res = {}
        net = _model(dev, "class", 0)
        res["cls"] = _pack(charades_eval.validate_cls(net, cls_batches[rank::world], process_group=pg))
        res["cls_single"] = _pack(charades_eval.validate_cls(net, cls_batches))
        net = _model(dev, "loc", 1)
        res["loc"] = _pack(charades_eval.validate_loc(net, loc_batches[rank::world], process_group=pg))
        res["loc_single"] = _pack(charades_eval.validate_loc(net, loc_batches))
        with open("%s.rank%d.json" % (out, rank), "w") as f:
            json.dump(res, f)
    finally:
        if pg is not None:
            dist.destroy_process_group()


def _fixture(dev):
    """The annotation fixture restricted to 12 training videos (and its testing split), as a dict, with noise videos long
    enough for the dataset's length filter."""
    with open(os.path.join(ROOT, "tests", "golden", "charades_anno.json")) as f:
        full = json.load(f)
    anno, kept = {}, 0
    for vid, rec in full.items():
        if rec["subset"] == "training":
            if kept == 12:
                continue
            kept += 1
        anno[vid] = rec
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    videos = {vid: torch.randint(0, 256, (max(int(round(24 * rec["duration"])), 168), 36, 48, 3), dtype=torch.uint8,
                                 device=dev, generator=g) for vid, rec in anno.items()}
    return anno, videos


def _record(res, dataset_rows):
    import hashlib
    phases = [{k: v for k, v in p.items()} for p in res["phases"]]
    sha = {name: hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]
           for name, t in res["model"].state_dict().items()}
    return {"phases": phases, "steps": res["steps"], "lr": res["lr"], "checkpoints": res["checkpoints"],
            "want_rows": dataset_rows, "model_sha": sha}


def _want_rows(anno, videos, task):
    import charades
    ds = charades.Charades(anno, "testing", videos, task=task, frames=80, gamma_tau=5, crops=10, crop_size=64, c_size=64,
                           scales=[224 / 256., 224 / 256.], mean=charades.CHARADES_MEAN, std=charades.CHARADES_STD)
    return len(ds) if task == "class" else sum(d[2] for d in ds.data)


def _runs(out, pg, rank, world, dev, splits, resume_from=None):
    import train_x3d_charades
    import train_x3d_charades_loc
    anno, videos = _fixture(dev)
    res = {}
    for task, mod in (("class", train_x3d_charades), ("loc", train_x3d_charades_loc)):
        torch.manual_seed(11 + rank)                          # the random 157-way head: rank 0's reaches every rank
        kw = dict(init_lr=0.01, anno=anno, videos=videos, batch_size=4, x3d_version="M", crop_size=64, c_size=64,
                  dropout=0.0, seed=1, device=str(dev), use_graph=(task == "class"))
        r = mod.run(max_epochs=1, save_model="%s_%s_" % (out, task), save_every=3, process_group=pg, rank=rank,
                    world=world, base_bn_splits=splits, **kw)
        res[task] = _record(r, _want_rows(anno, videos, task))
        if resume_from is not None:                           # a checkpoint the two-rank run wrote loads back
            again = mod.run(max_epochs=0, save_model="%s_%s_resumed_" % (out, task), save_every=0,
                            resume=resume_from[task], **kw)
            res[task]["resumed_lr"] = again["lr"]
            res[task]["resumed_momentum"] = bool(again["optimizer"].state_dict())
    with open("%s.rank%d.json" % (out, rank), "w") as f:
        json.dump(res, f)


def run(out):
    import train_x3d_charades
    import torch.distributed as dist
    pg, rank, world, dev = train_x3d_charades.init_distributed()
    try:
        _runs(out, pg, rank, world, dev, splits=1)
    finally:
        if pg is not None:
            dist.destroy_process_group()


def single(out, ckpts):
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    with open(ckpts) as f:
        resume_from = json.load(f)
    _runs(out, None, 0, 1, dev, splits=2, resume_from=resume_from)


if __name__ == "__main__":
    {"gather1": gather1, "validate": validate, "run": run, "single": single}[sys.argv[1]](*sys.argv[2:])
