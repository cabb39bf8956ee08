// Shared helpers of libx3djpeg's device stage (gfx950 only).  Kept apart from csrc/common.h: the training library's
// sources are hashed by tools/stamp.py and the gradient-hash record, and nothing here may change them (DESIGN.md
// section 7).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/x3djpeg.h"

void x3djpeg_set_error(const char* fmt, ...);  // host.cpp

#define X3DJPEG_CHECK_ARG(cond)                                                       \
    do {                                                                              \
        if (!(cond)) {                                                                \
            x3djpeg_set_error("%s:%d: argument check failed: %s", __FILE__, __LINE__, #cond); \
            return X3DJPEG_EINVAL;                                                    \
        }                                                                             \
    } while (0)

#define X3DJPEG_LAUNCH_CHECK()                                                        \
    do {                                                                              \
        hipError_t e_ = hipGetLastError();                                            \
        if (e_ != hipSuccess) {                                                       \
            x3djpeg_set_error("%s:%d: launch failed: %s", __FILE__, __LINE__, hipGetErrorString(e_)); \
            return X3DJPEG_ELAUNCH;                                                   \
        }                                                                             \
    } while (0)

__host__ __device__ static inline int jpeg_cdiv(int a, int b) { return (a + b - 1) / b; }
