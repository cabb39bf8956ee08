"""ctypes binding of libx3dstep.so (include/x3dstep.h): the gradient statistics, the step record and clipping by the
global norm.

Same discipline as _lib.py: the library is mandatory, torch is imported before it is loaded, the ABI version is checked,
and a failing entry point raises X3DHipError with the library's message.
"""
import ctypes
import os

import numpy as np

from ._lib import X3DHipError

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libx3dstep.so")
ABI_VERSION = 1

# include/x3dstep.h
ITEM = 2048
ITEMS_PER_GROUP = 4
S_STEP, S_BAD_STEP, S_BAD_SEG, S_NORM, S_COEF = 0, 1, 2, 3, 4
S_SKIP, S_SKIPPED, S_RUN = 5, 6, 7
KEEP_SAVE, KEEP_RESTORE = 0, 1
STATE_WORDS = 8
MAX_SEGMENTS = 1 << 20
MAX_ITEMS = 0x7fffff00
PBN_RUN = 256
PBN_ACC_DOUBLES = 4

ITEM_DT = np.dtype([("start", "<i8"), ("seg", "<i4"), ("len", "<i4")])
KEEP_DT = np.dtype([("addr", "<i8"), ("offset", "<i8"), ("len", "<i4"), ("pad", "<i4")])
PBN_LAYER_DT = np.dtype([("mean_addr", "<i8"), ("var_addr", "<i8"), ("mean_off", "<i8"), ("var_off", "<i8"), ("first", "<i8"),
                         ("C", "<i4"), ("S", "<i4")])
HYPER_DT = np.dtype([("lr_scale", "<f4"), ("wd_scale", "<f4")])
HEADER_DT = np.dtype([("step", "<i8"), ("total", "<f8"), ("norm", "<f8"), ("coef", "<f4"), ("nonfinite", "<i4"),
                      ("first_bad", "<i4"), ("nseg", "<i4")])

_P = ctypes.c_void_p
_I = ctypes.c_int
_L = ctypes.c_int64
_D = ctypes.c_double
_Z = ctypes.c_size_t
_F = ctypes.c_float

# name -> (restype, argtypes).  Every symbol include/x3dstep.h declares is listed here; tests/test_step_host.py checks the
# two against each other and against the library's exports.
SIGNATURES = {
    "x3dstep_abi_version": (_I, []),
    "x3dstep_last_error": (ctypes.c_char_p, []),
    "x3dstep_item_bytes": (_Z, []),
    "x3dstep_header_bytes": (_Z, []),
    "x3dstep_record_bytes": (_Z, [_I]),
    "x3dstep_item_count": (_L, [_P, _I]),
    "x3dstep_build_items": (_L, [_P, _I, _P, _L, _P]),
    "x3dstep_workspace_bytes": (_Z, [_L]),
    "x3dstep_observe": (_I, [_P, _L, _P, _I, _P, _P, _L, _P, _P, _P, _I, _D, _D, _P]),
    "x3dstep_observe_host": (_I, [_P, _L, _P, _I, _P, _P, _L, _P, _P, _P, _I, _D, _D]),
    "x3dstep_keep_bytes": (_Z, []),
    "x3dstep_measure": (_I, [_P, _L, _P, _I, _P, _P, _L, _P, _P, _P, _I, _D, _D, _P]),
    "x3dstep_measure_host": (_I, [_P, _L, _P, _I, _P, _P, _L, _P, _P, _P, _I, _D, _D]),
    "x3dstep_apply": (_I, [_P, _P, _P, _L, _P, _P, _I, _I, _F, _F, _F, _F, _I, _P]),
    "x3dstep_apply_host": (_I, [_P, _P, _P, _L, _P, _P, _I, _I, _F, _F, _F, _F, _I]),
    "x3dstep_hyper_bytes": (_Z, []),
    "x3dstep_apply_groups": (_I, [_P, _P, _P, _L, _P, _L, _P, _I, _P, _P, _I, _F, _F, _F, _F, _I, _I, _P]),
    "x3dstep_apply_groups_host": (_I, [_P, _P, _P, _L, _P, _L, _P, _I, _P, _P, _I, _F, _F, _F, _F, _I, _I]),
    "x3dstep_trust_workspace_bytes": (_Z, [_L]),
    "x3dstep_trust": (_I, [_P, _L, _P, _P, _L, _P, _P, _I, _P, _P, _I, _P, _P, _P, _F, _F, _F, _F, _I, _P]),
    "x3dstep_trust_host": (_I, [_P, _L, _P, _P, _L, _P, _P, _I, _P, _P, _I, _P, _P, _P, _F, _F, _F, _F, _I]),
    "x3dstep_apply_lars": (_I, [_P, _P, _P, _L, _P, _L, _P, _P, _I, _P, _P, _I, _F, _F, _F, _F, _I, _I, _P]),
    "x3dstep_apply_lars_host": (_I, [_P, _P, _P, _L, _P, _L, _P, _P, _I, _P, _P, _I, _F, _F, _F, _F, _I, _I]),
    "x3dstep_lamb_workspace_bytes": (_Z, [_L]),
    "x3dstep_adam": (_I, [_P, _P, _P, _P, _L, _P, _L, _P, _I, _P, _P, _I, _L, _F, _F, _F, _F, _F, _F, _I, _P]),
    "x3dstep_adam_host": (_I, [_P, _P, _P, _P, _L, _P, _L, _P, _I, _P, _P, _I, _L, _F, _F, _F, _F, _F, _F, _I]),
    "x3dstep_lamb_moments": (_I, [_P, _P, _P, _P, _L, _P, _L, _P, _I, _P, _P, _I, _L, _F, _F, _F, _F, _F, _P, _P]),
    "x3dstep_lamb_moments_host": (_I, [_P, _P, _P, _P, _L, _P, _L, _P, _I, _P, _P, _I, _L, _F, _F, _F, _F, _F, _P]),
    "x3dstep_lamb_trust": (_I, [_P, _L, _P, _P, _I, _P, _P, _I, _L, _P, _P, _P, _P, _P]),
    "x3dstep_lamb_trust_host": (_I, [_P, _L, _P, _P, _I, _P, _P, _I, _L, _P, _P, _P, _P]),
    "x3dstep_lamb_apply": (_I, [_P, _P, _P, _L, _P, _L, _P, _P, _I, _P, _P, _I, _L, _F, _F, _F, _F, _F, _P]),
    "x3dstep_lamb_apply_host": (_I, [_P, _P, _P, _L, _P, _L, _P, _P, _I, _P, _P, _I, _L, _F, _F, _F, _F, _F]),
    "x3dstep_keep": (_I, [_P, _I, _P, _L, _P, _L, _P, _I, _P]),
    "x3dstep_keep_host": (_I, [_P, _I, _P, _L, _P, _L, _P, _I]),
    "x3dstep_ema": (_I, [_P, _P, _L, _P, _L, _F, _I, _P]),
    "x3dstep_ema_host": (_I, [_P, _P, _L, _P, _L, _F, _I]),
    "x3dstep_ema_keep": (_I, [_P, _I, _P, _L, _P, _L, _P, _L, _F, _I, _P]),
    "x3dstep_ema_keep_host": (_I, [_P, _I, _P, _L, _P, _L, _P, _L, _F, _I]),
    "x3dstep_swap": (_I, [_P, _P, _L, _P]),
    "x3dstep_swap_host": (_I, [_P, _P, _L]),
    "x3dstep_swap_keep": (_I, [_P, _I, _P, _L, _P, _L, _P]),
    "x3dstep_swap_keep_host": (_I, [_P, _I, _P, _L, _P, _L]),
    "x3dstep_pbn_layer_bytes": (_Z, []),
    "x3dstep_pbn_build_layers": (_L, [_P, _I, _P, _I, _P]),
    "x3dstep_pbn_work_count": (_L, [_P, _I]),
    "x3dstep_pbn_build_work": (_L, [_P, _I, _P, _L]),
    "x3dstep_pbn_accum": (_I, [_P, _I, _P, _L, _P, _P]),
    "x3dstep_pbn_accum_host": (_I, [_P, _I, _P, _L, _P]),
    "x3dstep_pbn_finish": (_I, [_P, _I, _P, _L, _P, _I, _L, _P, _L, _P]),
    "x3dstep_pbn_finish_host": (_I, [_P, _I, _P, _L, _P, _I, _L, _P, _L]),
}

_lib = None


def lib():
    """Load (once) and return the ctypes handle; raises X3DHipError when unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise X3DHipError(
            "libx3dstep.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C x3d-multigrid_amd/csrc_step`). The gradient monitor has no fallback." % LIB_PATH)
    import torch  # noqa: F401  (its HIP runtime first: see _lib.lib)
    h = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(h, name)
        except AttributeError as e:
            raise X3DHipError("libx3dstep.so lacks symbol %s (stale build?)" % name) from e
        fn.restype = res
        fn.argtypes = args
    v = h.x3dstep_abi_version()
    if v != ABI_VERSION:
        raise X3DHipError("libx3dstep.so ABI %d != expected %d" % (v, ABI_VERSION))
    _lib = h
    return h


def check(rc):
    if rc < 0:
        raise X3DHipError("libx3dstep: error %d: %s" % (rc, lib().x3dstep_last_error().decode("utf-8", "replace")))
    return rc
