// Shared helpers of libx3ddata (gfx950 only).  Kept apart from csrc/common.h: the training library's sources are hashed
// by tools/stamp.py and the gradient-hash record, and nothing here may change them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include "../../include/x3ddata.h"

void x3ddata_set_error(const char* fmt, ...);

#define X3DDATA_CHECK_ARG(cond)                                                       \
    do {                                                                              \
        if (!(cond)) {                                                                \
            x3ddata_set_error("%s:%d: argument check failed: %s", __FILE__, __LINE__, #cond); \
            return X3DDATA_EINVAL;                                                    \
        }                                                                             \
    } while (0)

#define X3DDATA_LAUNCH_CHECK()                                                        \
    do {                                                                              \
        hipError_t e_ = hipGetLastError();                                            \
        if (e_ != hipSuccess) {                                                       \
            x3ddata_set_error("%s:%d: launch failed: %s", __FILE__, __LINE__, hipGetErrorString(e_)); \
            return X3DDATA_ELAUNCH;                                                   \
        }                                                                             \
    } while (0)

__host__ __device__ static inline int data_cdiv(int a, int b) { return (a + b - 1) / b; }
