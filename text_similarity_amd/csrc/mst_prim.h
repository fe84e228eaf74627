// Minimum spanning tree of the mutual-reachability graph by Prim's algorithm (included by search.hip, after the helpers it
// uses): the O(N^2 d) stage of HDBSCAN.  Everything is a SQUARED distance.  d2(a, b) is the float32 value the Euclidean search
// returns for the pair, bit for bit: exact_load_query and wave_scores unchanged, the rows read through l2_f32 (-dist^2 inside,
// the sign flipped here).  w(a, b) = max(d2(a, b), core2[a], core2[b]); without core2 it is d2 alone.
//
// The tree starts as {row 0}; best[j] = +inf, from[j] = -1.  Step t = 0 .. N-2 is two launches:
//   mst_step_kernel  every row j outside the tree is scored against row cur, 64 rows per wave per round, 256 per workgroup;
//                    w(cur, j) < best[j] (strict: the earlier endpoint keeps a tie, a NaN never updates) sets best[j] and
//                    from[j]; the workgroup writes the smallest (best[j], j) of its free rows — the lower row on a tie —
//                    to its slot.  A 64-row group with no free row is not loaded (wave-uniform).
//   mst_pick_kernel  one workgroup reduces the slots to `next`, writes edge t = (from[next], next, best[next]), marks next as
//                    in the tree and stores it in the device word cur.
// cur, best, from and the slots are read only in a LATER launch than the one that wrote them, so the launch boundary orders
// every hand-off; no workgroup waits for another and the host reads nothing back between steps.  The grid is one workgroup
// per 256 rows, never capped: there is one path for every N.  If every best is +inf the lowest free row wins with from = -1.
// A one-launch form (the workgroups' minima through a 64-bit atomic minimum, the last arrival at an agent-scope ticket picks)
// gave the same trees and was measured against this one: 4 % and 10 % faster per step at N = 5 000 and 20 000, 16 % slower at
// 100 000, where the time is (profiles/hdbscan_ab.txt).  This form was kept.
#pragma once

namespace tsim {
constexpr int MST_IN_TREE = -2;            // from[j] of a row in the tree (a free row holds -1 or its best endpoint)
constexpr int MST_NO_ROW = 0x7fffffff;     // the row of a slot without a free row: after every real row

__device__ __forceinline__ bool mst_key_before(float w1, int j1, float w2, int j2) { return w1 < w2 || (w1 == w2 && j1 < j2); }

__global__ __launch_bounds__(256) void mst_init_kernel(int64_t N, float *__restrict__ best, int32_t *__restrict__ from,
                                                       int32_t *__restrict__ cur) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < N) {
        best[j] = INFINITY;
        from[j] = j == 0 ? MST_IN_TREE : -1;
    }
    if (j == 0) *cur = 0;
}

__global__ __launch_bounds__(256) void mst_step_kernel(int64_t N, const l2_f32 *__restrict__ xr, int64_t ldr, int d,
                                                       const float *__restrict__ core2, const int32_t *__restrict__ cur_p,
                                                       float *__restrict__ best, int32_t *__restrict__ from,
                                                       float *__restrict__ slot_w, int32_t *__restrict__ slot_j) {
    __shared__ float red_w[4];
    __shared__ int red_j[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t g0 = (int64_t)blockIdx.x * 256 + wave * 64;   // the wave's 64-row group
    float my_w = INFINITY;
    int my_j = MST_NO_ROW;
    if (g0 < N) {   // wave-uniform
        const int nvalid = (int)(N - g0 < 64 ? N - g0 : 64);
        const bool valid = lane < nvalid;
        const int row = (int)(g0 + (valid ? lane : 0));   // in [0, N)
        const bool is_free = valid && from[row] != MST_IN_TREE;
        if (__any(is_free)) {   // wave-uniform: a group inside the tree costs no row loads
            const int cur = *cur_p;
            ExactQuery<l2_f32> eqr;
            exact_load_query<l2_f32, NORM_NONE>(eqr, xr + (int64_t)cur * ldr, d, lane);
            float w = -wave_scores<l2_f32, false>(eqr, xr, ldr, row, nvalid, d, lane);
            if (core2) {
                const float ca = core2[cur], cb = core2[row];
                w = ca > w ? ca : w;
                w = cb > w ? cb : w;
            }
            if (is_free) {
                float b = best[row];
                if (w < b) {
                    b = w;
                    best[row] = w;
                    from[row] = cur;
                }
                my_w = b;
                my_j = row;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ow = __shfl_xor(my_w, o, 64);
        const int oj = __shfl_xor(my_j, o, 64);
        if (mst_key_before(ow, oj, my_w, my_j)) {
            my_w = ow;
            my_j = oj;
        }
    }
    if (lane == 0) {
        red_w[wave] = my_w;
        red_j[wave] = my_j;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int v = 1; v < 4; ++v)
            if (mst_key_before(red_w[v], red_j[v], my_w, my_j)) {
                my_w = red_w[v];
                my_j = red_j[v];
            }
        slot_w[blockIdx.x] = my_w;
        slot_j[blockIdx.x] = my_j;
    }
}

__global__ __launch_bounds__(256) void mst_pick_kernel(int64_t nslots, const float *__restrict__ slot_w,
                                                       const int32_t *__restrict__ slot_j, const float *__restrict__ best,
                                                       int32_t *__restrict__ from, int32_t *__restrict__ cur_p,
                                                       int32_t *__restrict__ out_from, int32_t *__restrict__ out_to,
                                                       float *__restrict__ out_w2) {
    __shared__ float red_w[4];
    __shared__ int red_j[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float my_w = INFINITY;
    int my_j = MST_NO_ROW;
    for (int64_t s = threadIdx.x; s < nslots; s += 256) {
        const float ow = slot_w[s];
        const int oj = slot_j[s];
        if (mst_key_before(ow, oj, my_w, my_j)) {
            my_w = ow;
            my_j = oj;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ow = __shfl_xor(my_w, o, 64);
        const int oj = __shfl_xor(my_j, o, 64);
        if (mst_key_before(ow, oj, my_w, my_j)) {
            my_w = ow;
            my_j = oj;
        }
    }
    if (lane == 0) {
        red_w[wave] = my_w;
        red_j[wave] = my_j;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int v = 1; v < 4; ++v)
            if (mst_key_before(red_w[v], red_j[v], my_w, my_j)) {
                my_w = red_w[v];
                my_j = red_j[v];
            }
        if (my_j != MST_NO_ROW) {   // (a step always finds a free row: N - 1 steps over N - 1 free rows)
            *out_from = from[my_j];
            *out_to = my_j;
            *out_w2 = best[my_j];
            from[my_j] = MST_IN_TREE;
            *cur_p = my_j;
        }
    }
}

struct MstWs {
    size_t cur, best, from, slot_w, slot_j, total;
    int64_t nslots;
};
static void plan_workspace_mst(int64_t N, MstWs *w) {
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += align256(bytes); return at; };
    w->nslots = (N + 255) / 256;
    w->cur = take(4);
    w->best = take((size_t)N * 4);
    w->from = take((size_t)N * 4);
    w->slot_w = take((size_t)w->nslots * 4);
    w->slot_j = take((size_t)w->nslots * 4);
    w->total = o;
}
}  // namespace tsim

extern "C" size_t tsim_mst_prim_workspace_bytes(int64_t N) {
    if (N <= 0 || N >= (1ll << 31) - 64) return 0;
    tsim::MstWs w;
    tsim::plan_workspace_mst(N, &w);
    return w.total;
}

extern "C" int tsim_mst_prim(const float *rows_f32, int64_t ld_rows, int64_t N, int d, const float *core2, int32_t *out_from,
                             int32_t *out_to, float *out_w2, void *workspace, size_t workspace_bytes, void *stream) {
    using namespace tsim;
    const char *what = "mst_prim";
    TSIM_REQUIRE(N > 0 && N < (1ll << 31) - 64, "%s: N=%lld outside 1..2^31-65", what, (long long)N);
    TSIM_REQUIRE(d >= 1 && d < 64 * XS_MAXI, "%s: d=%d outside 1..%d", what, d, 64 * XS_MAXI - 1);
    TSIM_REQUIRE(ld_rows >= d, "%s: float32 row stride %lld < d=%d", what, (long long)ld_rows, d);
    TSIM_REQUIRE(rows_f32 && (N == 1 || (out_from && out_to && out_w2)), "%s: null pointer", what);
    if (N == 1) return TSIM_OK;   // no edge, no launch
    MstWs w;
    plan_workspace_mst(N, &w);
    if (!workspace || workspace_bytes < w.total) return fail(TSIM_ENOMEM, "%s: workspace %zu B < %zu B", what, workspace_bytes, w.total);
    hipStream_t st = as_stream(stream);
    char *ws = reinterpret_cast<char *>(workspace);
    int32_t *cur = reinterpret_cast<int32_t *>(ws + w.cur);
    float *best = reinterpret_cast<float *>(ws + w.best);
    int32_t *from = reinterpret_cast<int32_t *>(ws + w.from);
    float *slot_w = reinterpret_cast<float *>(ws + w.slot_w);
    int32_t *slot_j = reinterpret_cast<int32_t *>(ws + w.slot_j);
    const dim3 grid((unsigned)w.nslots);
    hipLaunchKernelGGL(mst_init_kernel, grid, dim3(256), 0, st, N, best, from, cur);
    TSIM_HIP_CHECK(hipGetLastError());
    const l2_f32 *xr = reinterpret_cast<const l2_f32 *>(rows_f32);
    for (int64_t t = 0; t < N - 1; ++t) {
        hipLaunchKernelGGL(mst_step_kernel, grid, dim3(256), 0, st, N, xr, ld_rows, d, core2, cur, best, from, slot_w, slot_j);
        hipLaunchKernelGGL(mst_pick_kernel, dim3(1), dim3(256), 0, st, w.nslots, slot_w, slot_j, best, from, cur, out_from + t,
                           out_to + t, out_w2 + t);
        if ((t & 1023) == 1023 || t == N - 2) TSIM_HIP_CHECK(hipGetLastError());
    }
    return TSIM_OK;
}
