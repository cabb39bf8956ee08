"""Charades on several ranks: the sharded validation phases and run() of the two scripts on two ranks that share cuda:0
and talk over gloo (test hook X3D_CHARADES_SINGLE_DEVICE / X3D_CHARADES_BACKEND; the production launch is one rank per GPU
over RCCL).  Every child runs under a timeout and every exit status is checked; the children of a test run one launch
after the other, so at most two of them hold the GPU at once."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "charades_ddp_child.py")


def _two_ranks(mode, out, port):
    env = dict(os.environ, X3D_CHARADES_SINGLE_DEVICE="1", X3D_CHARADES_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), CHILD, mode, out]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    ranks = []
    for r in range(2):
        with open("%s.rank%d.json" % (out, r)) as f:
            ranks.append(json.load(f))
    return ranks, res.stdout


def test_sharded_validation_equals_the_single_process_bit_for_bit(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    ranks, _ = _two_ranks("validate", str(tmp_path / "val"), 29642)
    for task in ("cls", "loc"):
        want = ranks[0][task + "_single"]                     # rank 0's own single-process call over all five batches
        assert want["rows"] > 0 and len(want["ap"]) == 157
        for r in range(2):
            got = ranks[r][task]
            assert got["ap"] == want["ap"], (task, r)         # the fp32 bit patterns
            assert got["losses"] == want["losses"], (task, r)
            assert got["rows"] == want["rows"] and got["map"] == want["map"], (task, r)
        assert ranks[1][task + "_single"] == want


def test_run_on_two_ranks(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    out = str(tmp_path / "ddp")
    ranks, printed = _two_ranks("run", out, 29643)
    ckpts = {}
    for task in ("class", "loc"):
        a, b = ranks[0][task], ranks[1][task]
        assert a["phases"] == b["phases"] and a["steps"] == b["steps"] == 6 and a["lr"] == b["lr"]
        # the ranks seeded torch differently: equal models mean that rank 0's parameters (the random head) were broadcast,
        # the averaged gradients kept them equal, and rank 0's buffers were broadcast before the validation
        assert len(a["model_sha"]) > 100
        assert [k for k in a["model_sha"] if a["model_sha"][k] != b["model_sha"][k]] == []
        assert [p["phase"] for p in a["phases"]] == ["train", "train", "val"]
        assert len(a["phases"][0]["losses"]) == 3 and len(a["phases"][0]["maps"]) == 3
        assert a["phases"][2]["rows"] == a["want_rows"] > 0                 # the whole testing split
        # exactly one rank wrote checkpoints
        assert [os.path.basename(p) for p in a["checkpoints"]] == ["ddp_%s_000003.pt" % task, "ddp_%s_000006.pt" % task]
        assert b["checkpoints"] == [] and all(os.path.exists(p) for p in a["checkpoints"])
        ckpts[task] = a["checkpoints"][0]
    assert printed.count("INIT LR") == 2                      # rank 0 alone prints (one line per task)
    with open(out + ".ckpts.json", "w") as f:
        json.dump(ckpts, f)
    # One process with two BatchNorm splits normalises two samples at a time, as the two ranks do.  (Its splits are samples
    # {0, 2} and {1, 3} -- split n % 2 -- where the ranks' chunks are {0, 1} and {2, 3}, so the batch statistics are those
    # of other pairs and the losses differ by more than summation order: measured 2.4e-4 relative at most for 'class',
    # 6.8e-4 for 'loc', against the bound of 1e-3.)
    single_out = str(tmp_path / "single")
    res = subprocess.run([sys.executable, CHILD, "single", single_out, out + ".ckpts.json"], capture_output=True,
                         text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    with open(single_out + ".rank0.json") as f:
        single = json.load(f)
    for task in ("class", "loc"):
        got, want = ranks[0][task]["phases"][0]["losses"][:3], single[task]["phases"][0]["losses"][:3]
        print(task, "two ranks", got, "one process", want)
        for g, w in zip(got, want):
            assert abs(g - w) <= 1e-3 * abs(w), (task, got, want)           # tests/parity.py's plain loss bound
        assert single[task]["phases"][2]["rows"] == ranks[0][task]["phases"][2]["rows"]
        assert single[task]["resumed_lr"] == ranks[0][task]["lr"] and single[task]["resumed_momentum"]
