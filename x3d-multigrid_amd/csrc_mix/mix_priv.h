// What mix.hip and mix_host.cpp share beside the arithmetic of mix_core.h: the error text and the argument checks, which
// follow no pointer (the plan, the labels and the clips may be device memory).
#pragma once
#include "mix_core.h"

void x3dmix_set_error(const char* fmt, ...);

int x3dmix_check_clips(const char* who, const float* src, const float* dst, const X3DMixSample* plan, int B, int planes,
                       int H, int W);
int x3dmix_check_targets(const char* who, const int64_t* labels, const X3DMixSample* plan, int B, int C, float smoothing,
                         const float* targets);
int x3dmix_check_soft_ce(const char* who, const float* logits, const float* targets, const float* loss,
                         const float* dlogits, const float* scratch, int R, int C, float grad_scale);
