"""ctypes binding of libx3dmix.so (include/x3dmix.h): mixup / CutMix of a batch of clips, the soft targets and the
soft-target cross entropy.

Same discipline as _lib.py: the library is mandatory, torch is imported before it is loaded, the ABI version is checked,
and a failing entry point raises X3DHipError with the library's message.
"""
import ctypes
import os

import numpy as np

from ._lib import X3DHipError

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libx3dmix.so")
ABI_VERSION = 1

# include/x3dmix.h: X3DMixSample
SAMPLE_DT = np.dtype([("partner", "<i4"), ("lam", "<f4"), ("y0", "<i4"), ("y1", "<i4"), ("x0", "<i4"), ("x1", "<i4"),
                      ("pad", "<i4", (2,))])
SAMPLE_BYTES = 32

_P = ctypes.c_void_p
_I = ctypes.c_int
_Z = ctypes.c_size_t
_F = ctypes.c_float

# name -> (restype, argtypes).  Every symbol include/x3dmix.h declares is listed here; tests/test_mix_host.py checks the two
# against each other and against the library's exports.
SIGNATURES = {
    "x3dmix_abi_version": (_I, []),
    "x3dmix_last_error": (ctypes.c_char_p, []),
    "x3dmix_sample_bytes": (_Z, []),
    "x3dmix_clips": (_I, [_P, _P, _P, _I, _I, _I, _I, _P]),
    "x3dmix_clips_host": (_I, [_P, _P, _P, _I, _I, _I, _I]),
    "x3dmix_targets": (_I, [_P, _P, _I, _I, _F, _P, _P]),
    "x3dmix_targets_host": (_I, [_P, _P, _I, _I, _F, _P]),
    "x3dmix_soft_ce": (_I, [_P, _P, _P, _P, _P, _I, _I, _F, _P, _P]),
    "x3dmix_soft_ce_host": (_I, [_P, _P, _P, _P, _P, _I, _I, _F, _P]),
}

_lib = None


def lib():
    """Load (once) and return the ctypes handle; raises X3DHipError when unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise X3DHipError(
            "libx3dmix.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C x3d-multigrid_amd/csrc_mix`). Batch mixing and the soft-target loss have no fallback." % LIB_PATH)
    import torch  # noqa: F401  (its HIP runtime first: see _lib.lib)
    h = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(h, name)
        except AttributeError as e:
            raise X3DHipError("libx3dmix.so lacks symbol %s (stale build?)" % name) from e
        fn.restype = res
        fn.argtypes = args
    v = h.x3dmix_abi_version()
    if v != ABI_VERSION:
        raise X3DHipError("libx3dmix.so ABI %d != expected %d" % (v, ABI_VERSION))
    if h.x3dmix_sample_bytes() != SAMPLE_BYTES or SAMPLE_DT.itemsize != SAMPLE_BYTES:
        raise X3DHipError("libx3dmix.so: a plan entry of %d bytes, expected %d" % (h.x3dmix_sample_bytes(), SAMPLE_BYTES))
    _lib = h
    return h


def check(rc):
    if rc < 0:
        raise X3DHipError("libx3dmix: error %d: %s" % (rc, lib().x3dmix_last_error().decode("utf-8", "replace")))
    return rc
