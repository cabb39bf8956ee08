"""ctypes binding of libx3deval.so (include/x3deval.h): the evaluation kernels (device-resident AP meter).

Same discipline as _lib.py: the library is mandatory, torch is imported before it is loaded, the ABI version is checked,
and a failing entry point raises X3DHipError with the library's message.
"""
import ctypes
import os

from ._lib import X3DHipError

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libx3deval.so")
ABI_VERSION = 3

# include/x3deval.h state words
S_COUNT, S_CAPACITY, S_OVERFLOW, S_BAD, S_BASE, S_GO, S_BATCHES = 0, 1, 2, 3, 4, 5, 6
STATE_INTS = 8
MAX_CAPACITY = 0x7fffffc0
MAX_FRAMES_B = 1024
CLS_MAX_K = 4096
CLS_MAX_CROPS = 32
MERGE_MAX_SHARDS = 64
MERGE_MAX_MARKS = 1 << 20

_P = ctypes.c_void_p
_I = ctypes.c_int
_Z = ctypes.c_size_t

# name -> (restype, argtypes).  Every symbol include/x3deval.h declares is listed here; tests/test_apmeter_host.py checks
# the two against each other and against the library's exports.
SIGNATURES = {
    "x3deval_abi_version": (_I, []),
    "x3deval_last_error": (ctypes.c_char_p, []),
    "x3deval_ap_reset": (_I, [_P, _I, _P]),
    "x3deval_ap_set_capacity": (_I, [_P, _I, _P]),
    "x3deval_ap_append": (_I, [_P, _P, _P, _P, _I, _P, _P, _P, _I, _P]),
    "x3deval_ap_append_crops": (_I, [_P, _P, _P, _I, _P, _P, _P, _I, _I, _P]),
    "x3deval_ap_append_frames": (_I, [_P, _P, _P, _P, _I, _P, _P, _P, _I, _I, _I, _P]),
    "x3deval_ap_workspace_bytes": (_Z, [_I, _I]),
    "x3deval_ap_value": (_I, [_P, _P, _P, _P, _I, _I, _P, _Z, _P, _P]),
    "x3deval_ap_mark": (_I, [_P, _P, _I, _P]),
    "x3deval_ap_merge_workspace_bytes": (_Z, [_I, _I]),
    "x3deval_ap_merge": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _I, _P, _Z, _P]),
    "x3deval_cls_append_crops": (_I, [_P, _P, _P, _P, _P, _P, _I, _P, _P, _I, _I, _P]),
    "x3deval_cls_value": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P]),
}

_lib = None


def lib():
    """Load (once) and return the ctypes handle; raises X3DHipError when unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise X3DHipError(
            "libx3deval.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C x3d-multigrid_amd/csrc_eval`). The meter has no fallback." % LIB_PATH)
    import torch  # noqa: F401  (its HIP runtime first: see _lib.lib)
    h = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(h, name)
        except AttributeError as e:
            raise X3DHipError("libx3deval.so lacks symbol %s (stale build?)" % name) from e
        fn.restype = res
        fn.argtypes = args
    v = h.x3deval_abi_version()
    if v != ABI_VERSION:
        raise X3DHipError("libx3deval.so ABI %d != expected %d" % (v, ABI_VERSION))
    _lib = h
    return h


def check(rc):
    if rc != 0:
        raise X3DHipError("libx3deval: error %d: %s" % (rc, lib().x3deval_last_error().decode("utf-8", "replace")))
