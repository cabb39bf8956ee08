// Shared helpers of libx3deval (gfx950 only).  Kept apart from csrc/common.h: the training library's sources are hashed
// by tools/stamp.py and the gradient-hash record, and nothing here may change them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include "../../include/x3deval.h"

void x3deval_set_error(const char* fmt, ...);

#define X3DEVAL_CHECK_ARG(cond)                                                       \
    do {                                                                              \
        if (!(cond)) {                                                                \
            x3deval_set_error("%s:%d: argument check failed: %s", __FILE__, __LINE__, #cond); \
            return X3DEVAL_EINVAL;                                                    \
        }                                                                             \
    } while (0)

#define X3DEVAL_LAUNCH_CHECK()                                                        \
    do {                                                                              \
        hipError_t e_ = hipGetLastError();                                            \
        if (e_ != hipSuccess) {                                                       \
            x3deval_set_error("%s:%d: launch failed: %s", __FILE__, __LINE__, hipGetErrorString(e_)); \
            return X3DEVAL_ELAUNCH;                                                   \
        }                                                                             \
    } while (0)

__host__ __device__ static inline int eval_cdiv(int a, int b) { return (a + b - 1) / b; }

// The reservation of an append (one thread): publishes the base row and advances the count, or sets the overflow flag.
__device__ static inline void reserve_rows(int* state, long long n) {
    const long long c = state[X3DEVAL_S_COUNT], cap = state[X3DEVAL_S_CAPACITY];
    if (c + n > cap) {
        state[X3DEVAL_S_OVERFLOW] = 1;
        state[X3DEVAL_S_GO] = 0;
    } else {
        state[X3DEVAL_S_BASE] = (int)c;
        state[X3DEVAL_S_COUNT] = (int)(c + n);
        state[X3DEVAL_S_GO] = 1;
    }
}
