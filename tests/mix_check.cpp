// Stand-alone check of libx3dmix's host code (csrc_mix/mix_host.cpp), built by tests/mix_program.py with
// -fsanitize=address,undefined.  Reads the records tests/test_mix_host.py wrote -- the clip and target case lists with the
// bytes the numpy restatement expects, and a few cross-entropy cases with the twin's own result -- runs the twins on heap
// buffers of exactly the size each array has, and compares.  Also: the refusals, which must not touch a buffer.
//
// file: int32 count, then per record a header {int32 kind, n0, planes, H, W, C; float f; int32 0} and
//   kind 0 (clips)    n0 = B: plan [B], x [B planes H W] float, expected the same
//   kind 1 (targets)  n0 = B, f = smoothing: plan [B], labels [B] int64, expected [B C] float
//   kind 2 (soft_ce)  n0 = R, f = grad_scale: z [R C], t [R C], loss [1], dlogits [R C]
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "x3dmix.h"

struct Header {
    int32_t kind, n0, planes, H, W, C;
    float f;
    int32_t zero;
};

static FILE* g_in;

template <class T>
static std::unique_ptr<T[]> read_array(size_t n) {
    std::unique_ptr<T[]> p(new T[n]);
    if (fread(p.get(), sizeof(T), n, g_in) != n) {
        printf("short read\n");
        exit(2);
    }
    return p;
}

static int fail(int rec, const char* what) {
    printf("record %d: %s (%s)\n", rec, what, x3dmix_last_error());
    return 1;
}

static int refusals() {
    float a[8] = {0}, b[8] = {0};
    X3DMixSample plan[2];
    memset(plan, 0, sizeof(plan));
    int64_t labels[2] = {0, 1};
    int bad = 0;
    bad += x3dmix_clips_host(a, a, plan, 2, 1, 2, 2) != X3DMIX_EINVAL;          // in place
    bad += x3dmix_clips_host(a, a + 4, plan, 2, 1, 2, 2) != X3DMIX_EINVAL;      // overlapping by half
    bad += x3dmix_clips_host(a + 4, a, plan, 2, 1, 2, 2) != X3DMIX_EINVAL;
    bad += x3dmix_clips_host(a, b, plan, 0, 1, 2, 2) != X3DMIX_EINVAL;
    bad += x3dmix_clips_host(a, b, plan, 2, 1, 0, 2) != X3DMIX_EINVAL;
    bad += x3dmix_clips_host(nullptr, b, plan, 2, 1, 2, 2) != X3DMIX_EINVAL;
    bad += x3dmix_clips_host(a, b, plan, 2, 1 << 20, 1 << 10, 2) != X3DMIX_EINVAL;   // 2^31 elements in a clip
    bad += x3dmix_targets_host(labels, plan, 2, 0, 0.f, a) != X3DMIX_EINVAL;
    bad += x3dmix_targets_host(labels, plan, 2, 4, 1.0f, a) != X3DMIX_EINVAL;
    bad += x3dmix_targets_host(labels, plan, 2, 4, -0.1f, a) != X3DMIX_EINVAL;
    bad += x3dmix_targets_host(labels, nullptr, 2, 4, 0.f, a) != X3DMIX_EINVAL;
    bad += x3dmix_soft_ce_host(a, b, a, b, a, 0, 4, 1.f, nullptr) != X3DMIX_EINVAL;
    bad += x3dmix_soft_ce_host(a, b, a, b, nullptr, 2, 4, 1.f, nullptr) != X3DMIX_EINVAL;
    bad += x3dmix_soft_ce_host(a, b, a, b, a, 2, 4, INFINITY, nullptr) != X3DMIX_EINVAL;
    for (int i = 0; i < 8; ++i) bad += a[i] != 0.f || b[i] != 0.f;
    bad += x3dmix_sample_bytes() != 32 || x3dmix_abi_version() != 1;
    return bad;
}

int main(int argc, char** argv) {
    if (argc != 2 || !(g_in = fopen(argv[1], "rb"))) {
        printf("usage: mix_check CASES\n");
        return 2;
    }
    int32_t count = 0;
    if (fread(&count, 4, 1, g_in) != 1) return 2;
    int done[3] = {0, 0, 0};
    for (int rec = 0; rec < count; ++rec) {
        Header h;
        if (fread(&h, sizeof(h), 1, g_in) != 1) return fail(rec, "no header");
        if (h.kind == 0) {
            const size_t n = (size_t)h.n0 * h.planes * h.H * h.W;
            auto plan = read_array<X3DMixSample>(h.n0);
            auto x = read_array<float>(n);
            auto want = read_array<float>(n);
            std::unique_ptr<float[]> got(new float[n]);
            if (x3dmix_clips_host(x.get(), got.get(), plan.get(), h.n0, h.planes, h.H, h.W)) return fail(rec, "clips refused");
            if (memcmp(got.get(), want.get(), n * 4)) return fail(rec, "clips differ");
        } else if (h.kind == 1) {
            const size_t n = (size_t)h.n0 * h.C;
            auto plan = read_array<X3DMixSample>(h.n0);
            auto labels = read_array<int64_t>(h.n0);
            auto want = read_array<float>(n);
            std::unique_ptr<float[]> got(new float[n]);
            if (x3dmix_targets_host(labels.get(), plan.get(), h.n0, h.C, h.f, got.get())) return fail(rec, "targets refused");
            if (memcmp(got.get(), want.get(), n * 4)) return fail(rec, "targets differ");
        } else if (h.kind == 2) {
            const size_t n = (size_t)h.n0 * h.C;
            auto z = read_array<float>(n);
            auto t = read_array<float>(n);
            auto want_loss = read_array<float>(1);
            auto want = read_array<float>(n);
            std::unique_ptr<float[]> got(new float[n]), sc(new float[h.n0]), loss(new float[1]);
            unsigned long long rng[2] = {7, 41};
            if (x3dmix_soft_ce_host(z.get(), t.get(), loss.get(), got.get(), sc.get(), h.n0, h.C, h.f, rng))
                return fail(rec, "soft_ce refused");
            if (rng[0] != 7 || rng[1] != 42) return fail(rec, "soft_ce: the draw counter");
            // the same code under another compiler and optimisation level: libm's expf / logf are the same, the bits agree
            if (memcmp(loss.get(), want_loss.get(), 4) || memcmp(got.get(), want.get(), n * 4))
                return fail(rec, "soft_ce differs");
        } else {
            return fail(rec, "unknown kind");
        }
        ++done[h.kind];
    }
    if (fgetc(g_in) != EOF) return fail(count, "trailing bytes");
    const int bad = refusals();
    if (bad) {
        printf("%d refusals wrong\n", bad);
        return 1;
    }
    printf("ok %d %d %d\n", done[0], done[1], done[2]);
    return 0;
}
