"""Identity of the kernel sources a measurement was taken on: sha256 over csrc/*.hip, common.h and include/x3dhip.h (first
16 hex digits) -- computable on the GPU box, where there is no .git -- plus the git commit when available.  The PMC
collections under profiles/ carry it; bench.py drops a collection whose stamp differs from the tree it runs on."""
import glob
import hashlib
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def csrc_sha16():
    h = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(ROOT, "x3d-multigrid_amd", "csrc", "*.hip"))) + \
        [os.path.join(ROOT, "x3d-multigrid_amd", "csrc", "common.h"), os.path.join(ROOT, "include", "x3dhip.h")]
    for f in files:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              stdin=subprocess.DEVNULL, timeout=10).stdout.strip() or None
    except Exception:
        return None


def meta():
    return {"csrc_sha16": csrc_sha16(), "commit": commit()}


def csrc_eval_sha16():
    """The same identity for the evaluation library (libx3deval.so): sha256 over csrc_eval/ (every file, by name) and
    include/x3deval.h, first 16 hex digits.  Kept apart from csrc_sha16, which the gradient-hash record is keyed on."""
    h = hashlib.sha256()
    d = os.path.join(ROOT, "x3d-multigrid_amd", "csrc_eval")
    files = sorted(f for f in glob.glob(os.path.join(d, "*")) if os.path.isfile(f) and not f.endswith(".o")) + \
        [os.path.join(ROOT, "include", "x3deval.h")]
    for f in files:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def csrc_data_sha16():
    """The same identity for the Charades input library (libx3ddata.so): sha256 over csrc_data/ (every file, by name) and
    include/x3ddata.h, first 16 hex digits.  Kept apart from csrc_sha16, which the gradient-hash record is keyed on."""
    h = hashlib.sha256()
    d = os.path.join(ROOT, "x3d-multigrid_amd", "csrc_data")
    files = sorted(f for f in glob.glob(os.path.join(d, "*")) if os.path.isfile(f) and not f.endswith(".o")) + \
        [os.path.join(ROOT, "include", "x3ddata.h")]
    for f in files:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def csrc_jpeg_sha16():
    """The same identity for the JPEG decoder (libx3djpeg.so): sha256 over csrc_jpeg/ (every file, by name) and
    include/x3djpeg.h, first 16 hex digits.  Kept apart from csrc_sha16, which the gradient-hash record is keyed on."""
    h = hashlib.sha256()
    d = os.path.join(ROOT, "x3d-multigrid_amd", "csrc_jpeg")
    files = sorted(f for f in glob.glob(os.path.join(d, "*")) if os.path.isfile(f) and not f.endswith(".o")) + \
        [os.path.join(ROOT, "include", "x3djpeg.h")]
    for f in files:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def csrc_step_sha16():
    """The same identity for the step library (libx3dstep.so): sha256 over csrc_step/ (every file, by name) and
    include/x3dstep.h, first 16 hex digits.  Kept apart from csrc_sha16, which the gradient-hash record is keyed on."""
    h = hashlib.sha256()
    d = os.path.join(ROOT, "x3d-multigrid_amd", "csrc_step")
    files = sorted(f for f in glob.glob(os.path.join(d, "*")) if os.path.isfile(f) and not f.endswith(".o")) + \
        [os.path.join(ROOT, "include", "x3dstep.h")]
    for f in files:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def csrc_mix_sha16():
    """The same identity for the mixing library (libx3dmix.so): sha256 over csrc_mix/ (every file, by name) and
    include/x3dmix.h, first 16 hex digits.  Kept apart from csrc_sha16, which the gradient-hash record is keyed on."""
    h = hashlib.sha256()
    d = os.path.join(ROOT, "x3d-multigrid_amd", "csrc_mix")
    files = sorted(f for f in glob.glob(os.path.join(d, "*")) if os.path.isfile(f) and not f.endswith(".o")) + \
        [os.path.join(ROOT, "include", "x3dmix.h")]
    for f in files:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]
