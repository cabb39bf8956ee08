"""The stand-alone check program of libx3dmix's host code (tests/mix_check.cpp): built and run the way tests/step_program.py
does it for the step library, and the case file it reads."""
import os
import struct
import subprocess

import numpy as np

from tests.step_program import ROOT, compiler

KIND_CLIPS, KIND_TARGETS, KIND_SOFT_CE = 0, 1, 2


def clips_record(x, plan, expected):
    B, P, H, W = x.shape
    return (struct.pack("<8i", KIND_CLIPS, B, P, H, W, 0, 0, 0) + plan.tobytes() + np.ascontiguousarray(x).tobytes()
            + np.ascontiguousarray(expected).tobytes())


def targets_record(labels, plan, C, smoothing, expected):
    B = labels.size
    return (struct.pack("<6if i", KIND_TARGETS, B, 0, 0, 0, C, float(smoothing), 0) + plan.tobytes()
            + np.ascontiguousarray(labels, dtype=np.int64).tobytes() + np.ascontiguousarray(expected).tobytes())


def soft_ce_record(z, t, grad_scale, loss, dlogits):
    R, C = z.shape
    return (struct.pack("<6if i", KIND_SOFT_CE, R, 0, 0, 0, C, float(grad_scale), 0) + np.ascontiguousarray(z).tobytes()
            + np.ascontiguousarray(t).tobytes() + np.asarray(loss, dtype=np.float32).reshape(1).tobytes()
            + np.ascontiguousarray(dlogits).tobytes())


def run(tmp_path, records):
    """tests/mix_check.cpp and csrc_mix/mix_host.cpp compiled with -fsanitize=address,undefined into a program of their own
    and run as a child process on the records; nothing sanitised is loaded into this interpreter.  Gives the words of the
    program's last line and its whole output."""
    cases = str(tmp_path / "mix_cases.bin")
    with open(cases, "wb") as f:
        f.write(struct.pack("<i", len(records)))
        for r in records:
            f.write(r)
    exe = str(tmp_path / "mix_check")
    cmd = [compiler(), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "mix_check.cpp"),
           os.path.join(ROOT, "x3d-multigrid_amd", "csrc_mix", "mix_host.cpp"), "-o", exe]
    # the sanitisers' runtimes linked into the program itself where the compiler ships them so (gcc needs to be told)
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True)
    r = subprocess.run([exe, cases], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout.strip().splitlines()[-1].split(), r.stdout
