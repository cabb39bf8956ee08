"""ctypes binding of libx3ddata.so (include/x3ddata.h): the input kernels (clip batches of both datasets, Charades per-frame
labels).

Same discipline as _lib.py: the library is mandatory, torch is imported before it is loaded, the ABI version is checked,
and a failing entry point raises X3DHipError with the library's message.
"""
import ctypes
import os

import numpy as np

from ._lib import X3DHipError

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libx3ddata.so")
ABI_VERSION = 1

_P = ctypes.c_void_p
_I = ctypes.c_int
_Z = ctypes.c_size_t

# name -> (restype, argtypes).  Every symbol include/x3ddata.h declares is listed here; tests/test_charades_data_host.py
# checks the two against each other and against the library's exports.
SIGNATURES = {
    "x3ddata_abi_version": (_I, []),
    "x3ddata_last_error": (ctypes.c_char_p, []),
    "x3ddata_label_job_bytes": (_Z, []),
    "x3ddata_clip_job_bytes": (_Z, []),
    "x3ddata_charades_labels": (_I, [_P, _P, _P, _P, _I, _P, _I, _I, _I, _P, _P, _P, _P]),
    "x3ddata_clip_batch": (_I, [_P, _I, _P, _P, _I, _I, _I, _I, _P, _P, _P]),
}

# X3DDataLabelJob / X3DDataClipJob of include/x3ddata.h
LABEL_JOB_DT = np.dtype([("video", "<i4"), ("start", "<i4"), ("n", "<i4"), ("pad", "<i4")])
CLIP_JOB_DT = np.dtype([("src", "<u8"), ("dst", "<u8"), ("kk", "<u8"), ("bounds", "<u8"),
                        ("dst_cs", "<i8"), ("dst_ts", "<i8"), ("dst_ws", "<i8"), ("tmp_off", "<i8"),
                        ("frames_off", "<i4"), ("Hs", "<i4"), ("Ws", "<i4"), ("x1", "<i4"), ("y1", "<i4"),
                        ("crop", "<i4"), ("out", "<i4"), ("ksize", "<i4"), ("T", "<i4"), ("Tpad", "<i4"), ("flip", "<i4"),
                        ("nwin", "<i4"), ("win_step", "<i4"), ("win_len", "<i4")])

_lib = None


def lib():
    """Load (once) and return the ctypes handle; raises X3DHipError when unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise X3DHipError(
            "libx3ddata.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C x3d-multigrid_amd/csrc_data`). The input path has no fallback." % LIB_PATH)
    import torch  # noqa: F401  (its HIP runtime first: see _lib.lib)
    h = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(h, name)
        except AttributeError as e:
            raise X3DHipError("libx3ddata.so lacks symbol %s (stale build?)" % name) from e
        fn.restype = res
        fn.argtypes = args
    v = h.x3ddata_abi_version()
    if v != ABI_VERSION:
        raise X3DHipError("libx3ddata.so ABI %d != expected %d" % (v, ABI_VERSION))
    if h.x3ddata_label_job_bytes() != LABEL_JOB_DT.itemsize or h.x3ddata_clip_job_bytes() != CLIP_JOB_DT.itemsize:
        raise X3DHipError("libx3ddata.so job structs (%d, %d bytes) differ from the binding's (%d, %d)" % (
            h.x3ddata_label_job_bytes(), h.x3ddata_clip_job_bytes(), LABEL_JOB_DT.itemsize, CLIP_JOB_DT.itemsize))
    _lib = h
    return h


def check(rc):
    if rc != 0:
        raise X3DHipError("libx3ddata: error %d: %s" % (rc, lib().x3ddata_last_error().decode("utf-8", "replace")))
