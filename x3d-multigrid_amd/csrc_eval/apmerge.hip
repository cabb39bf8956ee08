// Segment marks of the AP meter and the merge of several meters' rows into one (include/x3deval.h).
//
// A meter that is to be merged records, after every add, the row count the add left behind (x3deval_ap_mark: one thread,
// on the device, since the host never sees the count).  The merge interleaves the shards' segments -- segment index
// first, shard second -- which is the row order of one process that had seen every add in global order.
//
// Plan (one workgroup): validates the marks, ORs the sticky flags, writes the destination state and the destination offset
// of every segment.  With E_r(j) = the rows of shard r in its segments below j (a mark, clamped at the shard's last one),
//   off(r, j) = sum_r' E_r'(j) + sum_{r' < r} (E_r'(j + 1) - E_r'(j)),
// the exclusive sum of the segment lengths in the interleaved order: one wave takes a segment index j, lane r its shard,
// so round j costs one wave reduction and one wave scan and no round waits for another.
//
// Copy: thread = (source row i, shard r), a tile of classes per workgroup.  One binary search in the shard's marks finds
// the row's segment; the lookup is reused for every class of the tile.  Consecutive lanes read consecutive rows of a class
// and write consecutive rows wherever they share a segment.  Every destination element is stored once, by one thread.
#include "eval_common.h"

namespace {

constexpr int PLAN_NT = 1024;              // threads of the plan workgroup
constexpr int COPY_NT = 256;               // source rows per copy workgroup
constexpr int COPY_KT = 8;                 // classes per copy workgroup
constexpr int WS_HEAD = 16;                // workspace header ints: [0] = 1 when the copy may run

__global__ void ap_mark_kernel(int* state, int* marks, int max_marks) {
    if (threadIdx.x != 0) return;
    const int s = marks[0];
    if (s < 0 || s >= max_marks) {
        state[X3DEVAL_S_OVERFLOW] = 1;
        return;
    }
    marks[1 + s] = state[X3DEVAL_S_COUNT];
    marks[0] = s + 1;
}

// E_r(j): the rows of a shard in its segments below j (mk: the shard's marks, s: its segment count)
__device__ __forceinline__ int rows_below(const int* __restrict__ mk, int s, int j) {
    const int m = j < s ? j : s;
    return m > 0 ? mk[m] : 0;              // mk[1 + (m - 1)]
}

__global__ __launch_bounds__(PLAN_NT) void ap_merge_plan_kernel(const int* __restrict__ states, const int* __restrict__ marks,
                                                                int W, int M, int C, int* __restrict__ dst_state, int Cd,
                                                                int* __restrict__ ws) {
    __shared__ int s_cnt[X3DEVAL_MERGE_MAX_SHARDS];      // the shards' segment counts, clamped to [0, M]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t ms = (size_t)M + 1;
    int sticky_bad = 0, over = 0, inconsistent = 0;
    if (tid < W) {
        const int* st = states + (size_t)tid * X3DEVAL_STATE_INTS;
        const int s = marks[(size_t)tid * ms], n = st[X3DEVAL_S_COUNT];
        over = st[X3DEVAL_S_OVERFLOW] != 0;
        sticky_bad = st[X3DEVAL_S_BAD] != 0;       // travels with the rows (the target was stored as 1): no reason to stop
        inconsistent = s < 0 || s > M || n < 0 || n > C;
        s_cnt[tid] = s < 0 ? 0 : (s > M ? M : s);
    }
    __syncthreads();
    int smax = 0;
    long long total = 0;
    for (int r = 0; r < W; ++r) {
        const int s = s_cnt[r], n = states[(size_t)r * X3DEVAL_STATE_INTS + X3DEVAL_S_COUNT];
        const int* mk = marks + (size_t)r * ms;
        smax = s > smax ? s : smax;
        total += n;
        if (tid == 0) inconsistent |= (s > 0 ? mk[s] : 0) != n;               // the last end is the count
        for (int j = tid; j < s; j += PLAN_NT) inconsistent |= mk[1 + j] < (j > 0 ? mk[j] : 0);
    }
    inconsistent = __syncthreads_or(inconsistent);
    sticky_bad = __syncthreads_or(sticky_bad);
    over = __syncthreads_or(over);
    const int fits = total <= (long long)Cd;
    const int run = !inconsistent && fits;
    if (run) {
        // off(r, j): wave = segment index, lane = shard (W <= 64)
        const int s = lane < W ? s_cnt[lane] : 0;
        const int* mk = marks + (size_t)(lane < W ? lane : 0) * ms;
        for (int j = wave; j < smax; j += PLAN_NT / 64) {
            const int e0 = lane < W ? rows_below(mk, s, j) : 0;
            const int len = lane < W ? rows_below(mk, s, j + 1) - e0 : 0;
            int base = e0, inc = len;
            for (int o = 32; o > 0; o >>= 1) base += __shfl_xor(base, o);
            for (int o = 1; o < 64; o <<= 1) {
                const int u = __shfl_up(inc, o);
                if (lane >= o) inc += u;
            }
            if (lane < W && j < s) ws[WS_HEAD + (size_t)lane * M + j] = base + inc - len;
        }
    }
    if (tid == 0) {
        for (int i = 0; i < X3DEVAL_STATE_INTS; ++i) dst_state[i] = 0;
        dst_state[X3DEVAL_S_COUNT] = run ? (int)total : 0;
        dst_state[X3DEVAL_S_CAPACITY] = Cd;
        dst_state[X3DEVAL_S_OVERFLOW] = over || !fits;
        dst_state[X3DEVAL_S_BAD] = sticky_bad || inconsistent;
        ws[0] = run;
    }
}

__global__ __launch_bounds__(COPY_NT) void ap_merge_copy_kernel(const int* __restrict__ states, const int* __restrict__ marks,
                                                                const float* __restrict__ scores,
                                                                const uint8_t* __restrict__ targets,
                                                                const float* __restrict__ weights, int M, int K, int C,
                                                                float* __restrict__ dst_scores, uint8_t* __restrict__ dst_targets,
                                                                float* __restrict__ dst_weights, int Cd,
                                                                const int* __restrict__ ws) {
    if (ws[0] == 0) return;
    const int r = blockIdx.y;
    const int i = blockIdx.x * COPY_NT + threadIdx.x;
    if (i >= states[(size_t)r * X3DEVAL_STATE_INTS + X3DEVAL_S_COUNT]) return;
    const int* mk = marks + (size_t)r * ((size_t)M + 1);
    // the first segment whose end is past row i (segments of length 0 are stepped over); the plan has checked that the
    // ends are non-decreasing and that the last one is the count, so the search ends inside [0, s)
    int lo = 0, hi = mk[0] - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (mk[1 + mid] > i) hi = mid;
        else lo = mid + 1;
    }
    const size_t d = (size_t)ws[WS_HEAD + (size_t)r * M + lo] + (size_t)(i - (lo > 0 ? mk[lo] : 0));
    const int k0 = blockIdx.z * COPY_KT;
    const size_t src = ((size_t)r * K + k0) * (size_t)C + i;
    float sv[COPY_KT];
    uint8_t tv[COPY_KT];
#pragma unroll
    for (int k = 0; k < COPY_KT; ++k) {
        if (k0 + k < K) {
            sv[k] = scores[src + (size_t)k * C];
            tv[k] = targets[src + (size_t)k * C];
        }
    }
#pragma unroll
    for (int k = 0; k < COPY_KT; ++k) {
        if (k0 + k < K) {
            dst_scores[(size_t)(k0 + k) * Cd + d] = sv[k];
            dst_targets[(size_t)(k0 + k) * Cd + d] = tv[k];
        }
    }
    if (weights && blockIdx.z == 0) dst_weights[d] = weights[(size_t)r * C + i];
}

}  // namespace

extern "C" int x3deval_ap_mark(int* state, int* marks, int max_marks, void* stream) {
    X3DEVAL_CHECK_ARG(state && marks && max_marks >= 0 && max_marks <= X3DEVAL_MERGE_MAX_MARKS);
    hipLaunchKernelGGL(ap_mark_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, marks, max_marks);
    X3DEVAL_LAUNCH_CHECK();
    return X3DEVAL_OK;
}

extern "C" size_t x3deval_ap_merge_workspace_bytes(int nshards, int max_marks) {
    if (nshards <= 0 || nshards > X3DEVAL_MERGE_MAX_SHARDS || max_marks < 0 || max_marks > X3DEVAL_MERGE_MAX_MARKS) return 0;
    return sizeof(int) * ((size_t)WS_HEAD + (size_t)nshards * (size_t)max_marks);
}

extern "C" int x3deval_ap_merge(const int* states, const int* marks, const float* scores, const uint8_t* targets,
                                const float* weights, int nshards, int max_marks, int K, int capacity, int* dst_state,
                                float* dst_scores, uint8_t* dst_targets, float* dst_weights, int dst_capacity,
                                void* workspace, size_t workspace_bytes, void* stream) {
    X3DEVAL_CHECK_ARG(states && marks && scores && targets && dst_state && dst_scores && dst_targets && workspace);
    X3DEVAL_CHECK_ARG((weights == nullptr) == (dst_weights == nullptr));
    X3DEVAL_CHECK_ARG(nshards >= 1 && nshards <= X3DEVAL_MERGE_MAX_SHARDS);
    X3DEVAL_CHECK_ARG(max_marks >= 0 && max_marks <= X3DEVAL_MERGE_MAX_MARKS);
    X3DEVAL_CHECK_ARG(K > 0 && capacity > 0 && capacity <= X3DEVAL_MAX_CAPACITY);
    X3DEVAL_CHECK_ARG(dst_capacity > 0 && dst_capacity <= X3DEVAL_MAX_CAPACITY);
    X3DEVAL_CHECK_ARG(workspace_bytes >= x3deval_ap_merge_workspace_bytes(nshards, max_marks));
    const int gz = eval_cdiv(K, COPY_KT);
    X3DEVAL_CHECK_ARG(gz <= 65535);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ap_merge_plan_kernel, dim3(1), dim3(PLAN_NT), 0, s, states, marks, nshards, max_marks, capacity,
                       dst_state, dst_capacity, (int*)workspace);
    hipLaunchKernelGGL(ap_merge_copy_kernel, dim3(eval_cdiv(capacity, COPY_NT), nshards, gz), dim3(COPY_NT), 0, s, states,
                       marks, scores, targets, weights, max_marks, K, capacity, dst_scores, dst_targets, dst_weights,
                       dst_capacity, (const int*)workspace);
    X3DEVAL_LAUNCH_CHECK();
    return X3DEVAL_OK;
}
