// Graph index, insertion (included by search.hip behind graph_search.h): the two kernels that link a batch of new rows into a
// built graph — include/tsim_graph_insert.h states both rules in full, tests/graph_insert_cases.py restates them in numpy.
//
// graph_insert_prune_kernel: graph_prune_kernel's detour count with the neighbour lists that exist at insertion time.  One
// workgroup per new row i: the lists N(cand[i][a]) — a graph row for an old candidate, the first R candidates of a batch row —
// are gathered into LDS (K0 R words), D[j] counts the lists of better-ranked candidates that hold cand[i][j] (LDS atomics), and
// the R candidates of smallest (D, j) are the forward row.  Integers only.
//
// graph_link_reverse_kernel: one workgroup per target t.  Its graph row is read once into LDS; the front half of its valid
// entries stays; the rest and the incoming rows form the pool, deduplicated IN ORDER, 256 source entries a step (an entry is
// fresh when it is in neither the kept half, nor the pool so far, nor earlier in its own step), at most 256 entries; row t is
// resident in ExactQuery and the pool is dealt to the four waves in batches of eight (exact_score_batch, as the beam search
// deals a step's rows); one SlList flush orders it; the row is written in place.  A workgroup touches no graph row but its own.
// House rule for ids, as everywhere: negative is padding, an id beyond the rows is never dereferenced and raises a status bit.
#pragma once

#include "../../include/tsim_graph_insert.h"

namespace tsim {
constexpr int GRAPH_LINK_POOL = TSIM_GRAPH_LINK_POOL;
static_assert(GRAPH_LINK_POOL == 256 && GRAPH_LINK_POOL <= SL_NB, "one thread per pool entry of a step, one block of the list");
static_assert(GRAPH_MAX_R <= 64, "a graph row is compacted by one wave");

__global__ __launch_bounds__(256) void graph_insert_prune_kernel(int64_t B, const int32_t *__restrict__ cand, int K0,
                                                                 const int32_t *__restrict__ graph, int64_t n, int R,
                                                                 int32_t *__restrict__ out_f, int32_t *__restrict__ out_d,
                                                                 int32_t *__restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) int insert_smem[];
    int *nb = insert_smem, *g = nb + K0 * R, *D = g + K0;
    __shared__ int st_s;
    const int tid = threadIdx.x;
    const int64_t end = n + B;   // ids below it are usable
    for (int64_t i = blockIdx.x; i < B; i += gridDim.x) {
        for (int t = tid; t < K0; t += 256) {
            g[t] = cand[i * K0 + t];
            D[t] = 0;
        }
        if (tid == 0) st_s = 0;
        __syncthreads();
        for (int p = tid; p < K0 * R; p += 256) {
            const int a = p / R, c = p - a * R;
            const int ga = g[a];
            const bool ok = ga >= 0 && ga < end;
            const int64_t at = ok ? ga : 0;   // clamped: loaded, dropped
            const int v = at < n ? graph[at * R + c] : cand[(at - n) * K0 + c];
            nb[p] = ok ? v : -1;
        }
        __syncthreads();
        for (int p = tid; p < K0 * K0; p += 256) {
            const int a = p / K0, j = p - a * K0;
            const int tg = g[j];
            if (a < j && tg >= 0 && tg < end) {
                bool found = false;
                for (int c = 0; c < R; ++c) found |= nb[a * R + c] == tg;
                if (found) atomicAdd(D + j, 1);
            }
        }
        __syncthreads();
        for (int j = tid; j < K0; j += 256) {
            if (!(g[j] >= 0 && g[j] < end)) D[j] = K0;
            if (g[j] >= end) atomicOr(&st_s, TSIM_GRAPH_INSERT_ST_ROW);
        }
        __syncthreads();
        for (int j = tid; j < K0; j += 256) {
            const int dj = D[j];
            int r = 0;
            for (int c = 0; c < K0; ++c) r += D[c] < dj || (D[c] == dj && c < j);
            if (r < R) out_f[i * R + r] = dj < K0 ? g[j] : -1;
            if (out_d) out_d[i * K0 + j] = dj;
        }
        if (status && tid == 0) status[i] = st_s;
        __syncthreads();
    }
}

template <typename T, bool COS>
__global__ __launch_bounds__(256) void graph_link_reverse_kernel(int64_t N, const T *__restrict__ xr, int64_t ldr, int d,
                                                                 int32_t *graph, int R, const int32_t *__restrict__ targets,
                                                                 int64_t Tn, const int64_t *__restrict__ in_lims,
                                                                 const int32_t *__restrict__ in_ids, int kp,
                                                                 int32_t *__restrict__ status) {
    SlList<int, false> top = sl_shared_list<int, false>();
    __shared__ int valid_s[GRAPH_MAX_R], pool_s[GRAPH_LINK_POOL], step_s[256], cnt_s[4], nvalid_s, st_s;
    const int tid = threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = R / 2, k = R - h;   // (kp: sl_list_len(k))
    const int64_t total = in_lims[Tn] > 0 ? in_lims[Tn] : 0;
    for (int64_t j = blockIdx.x; j < Tn; j += gridDim.x) {   // workgroup-uniform
        const int64_t t = targets[j];
        if (t < 0 || t >= N) {
            if (status && tid == 0) status[j] = TSIM_GRAPH_LINK_ST_ROW;
            continue;
        }
        if (wave == 0) {   // the row's non-negative entries, in order
            const int v = lane < R ? graph[t * R + lane] : -1;
            const unsigned long long m = __ballot(v >= 0);
            if (v >= 0) valid_s[__popcll(m & ((1ull << lane) - 1))] = v;
            if (lane == 0) {
                nvalid_s = __popcll(m);
                st_s = 0;
            }
        }
        ExactQuery<T> eqr;
        exact_load_query<T, COS>(eqr, xr + t * ldr, d, lane);
        top.reset(kp);   // (a barrier)
        const int nvalid = nvalid_s, nk = nvalid < h ? nvalid : h, nrest = nvalid - nk;
        int64_t lo = in_lims[j], hi = in_lims[j + 1];
        int bits = 0;
        {
            const int64_t lo_c = lo < 0 ? 0 : lo > total ? total : lo;
            const int64_t hi_c = hi < lo_c ? lo_c : hi > total ? total : hi;
            if (lo_c != lo || hi_c != hi) bits |= TSIM_GRAPH_LINK_ST_LIMS;
            lo = lo_c;
            hi = hi_c;
        }
        // the pool: valid[nk ..) then the incoming rows, fresh entries in order, a step of 256 source entries at a time
        const int64_t L = nrest + (hi - lo);
        int npool = 0;
        for (int64_t p0 = 0; p0 < L && npool <= GRAPH_LINK_POOL; p0 += 256) {   // workgroup-uniform
            const int64_t p = p0 + tid;
            const int id = p >= L ? -1 : p < nrest ? valid_s[nk + p] : in_ids[lo + p - nrest];
            step_s[tid] = id;
            __syncthreads();
            bool fresh = id >= 0;
            if (fresh) {
                const int held = npool < GRAPH_LINK_POOL ? npool : GRAPH_LINK_POOL;
                for (int c = 0; c < nk; ++c) fresh &= valid_s[c] != id;
                for (int c = 0; c < held; ++c) fresh &= pool_s[c] != id;
                for (int c = 0; c < tid; ++c) fresh &= step_s[c] != id;
            }
            const unsigned long long m = __ballot(fresh);
            if (lane == 0) cnt_s[wave] = __popcll(m);
            __syncthreads();
            int at = npool + __popcll(m & ((1ull << lane) - 1)), all = 0;
#pragma unroll
            for (int wv = 0; wv < 4; ++wv) {
                at += wv < wave ? cnt_s[wv] : 0;
                all += cnt_s[wv];
            }
            if (fresh && at < GRAPH_LINK_POOL) pool_s[at] = id;
            npool += all;
            __syncthreads();
        }
        if (npool > GRAPH_LINK_POOL) {
            bits |= TSIM_GRAPH_LINK_ST_CUT;
            npool = GRAPH_LINK_POOL;
        }
        const SlBound<int> w = top.bound(k);
        for (int b = wave * 8; b < npool; b += 32) {   // wave-uniform: batches of eight rows, dealt round the four waves
            const int nv = npool - b < 8 ? npool - b : 8;
            const int id = pool_s[b + (lane < nv ? lane : 0)];
            const bool usable = id < N;
            const int row = usable ? id : 0;   // clamped: the row is loaded and scored, the score dropped
            const float s = exact_score_batch<T, COS, 8>(eqr, xr, ldr, row, 0, nv, d, lane);
            if (lane < nv) {
                if (usable) top.offer(s, row, w);
                else bits |= TSIM_GRAPH_LINK_ST_ROW;
            }
        }
        if (bits) atomicOr(&st_s, bits);
        top.flush(kp);   // (its first barrier: the status bits are in)
        if (tid < R) {
            const int c = tid - nk;
            const int best = c >= 0 && c < k ? top.top_i[c] : sl_pad<int>();
            graph[t * R + tid] = tid < nk ? valid_s[tid] : best != sl_pad<int>() ? best : -1;
        }
        if (status && tid == 0) status[j] = st_s;
        __syncthreads();
    }
}
}  // namespace tsim

extern "C" int tsim_graph_insert_prune(const int32_t *cand, int64_t B, int K0, const int32_t *graph, int64_t n, int R,
                                       int32_t *out_forward, int32_t *out_detours, int32_t *out_status, void *stream) {
    using namespace tsim;
    const char *what = "graph_insert_prune";
    TSIM_REQUIRE(cand && graph && out_forward, "%s: null pointer", what);
    TSIM_REQUIRE(B > 0 && n > 0 && n + B < (1ll << 31) - 64 && B < (1ll << 31) && n < (1ll << 31),
                 "%s: B=%lld new rows on n=%lld, outside 1 <= B, 1 <= n, n + B < 2^31-64", what, (long long)B, (long long)n);
    TSIM_REQUIRE(K0 >= 1 && K0 <= GRAPH_PRUNE_MAX_K0, "%s: K0=%d outside 1..%d", what, K0, GRAPH_PRUNE_MAX_K0);
    TSIM_REQUIRE(R >= 1 && R <= K0 && R <= GRAPH_MAX_R, "%s: R=%d outside 1..min(K0=%d, %d)", what, R, K0, GRAPH_MAX_R);
    const size_t lds = (size_t)(K0 * R + 2 * K0) * 4;   // at most 33 KiB
    const unsigned grid = (unsigned)(B < 16384 ? B : 16384);
    hipLaunchKernelGGL(graph_insert_prune_kernel, dim3(grid), dim3(256), lds, as_stream(stream), B, cand, K0, graph, n, R, out_forward,
                       out_detours, out_status);
    TSIM_HIP_CHECK(hipGetLastError());
    return TSIM_OK;
}

extern "C" int tsim_graph_link_reverse(int space, const float *rows_f32, int64_t ld_rows, int64_t N, int d, int32_t *graph, int R,
                                       const int32_t *targets, int64_t T, const int64_t *in_lims, const int32_t *in_ids,
                                       int32_t *out_status, void *stream) {
    using namespace tsim;
    const char *what = "graph_link_reverse";
    TSIM_REQUIRE(rows_f32 && graph && targets && in_lims && in_ids, "%s: null pointer", what);
    TSIM_REQUIRE(space == TSIM_SPACE_COSINE || space == TSIM_SPACE_DOT || space == TSIM_SPACE_L2, "%s: unknown space %d", what, space);
    TSIM_REQUIRE(N > 0 && N < (1ll << 31) - 64, "%s: N=%lld outside 1..2^31-65", what, (long long)N);
    TSIM_REQUIRE(T > 0 && T <= N, "%s: T=%lld targets, outside 1..N=%lld (targets are distinct rows)", what, (long long)T, (long long)N);
    TSIM_REQUIRE(R >= 1 && R <= GRAPH_MAX_R, "%s: degree R=%d outside 1..%d", what, R, GRAPH_MAX_R);
    TSIM_REQUIRE(d >= 1 && d <= 64 * XS_MAXI, "%s: d=%d outside 1..%d", what, d, 64 * XS_MAXI);
    TSIM_REQUIRE(space != TSIM_SPACE_L2 || d < 64 * XS_MAXI, "%s: d=%d (the Euclidean space takes d <= %d)", what, d, 64 * XS_MAXI - 1);
    TSIM_REQUIRE(ld_rows >= d, "%s: float32 row stride %lld < d=%d", what, (long long)ld_rows, d);
    hipStream_t st = as_stream(stream);
    const unsigned grid = (unsigned)(T < 65536 ? T : 65536);
    const int kp = sl_list_len(R - R / 2);
    if (space == TSIM_SPACE_COSINE)
        hipLaunchKernelGGL((graph_link_reverse_kernel<float, true>), dim3(grid), dim3(256), 0, st, N, rows_f32, ld_rows, d, graph, R, targets,
                           T, in_lims, in_ids, kp, out_status);
    else if (space == TSIM_SPACE_DOT)
        hipLaunchKernelGGL((graph_link_reverse_kernel<float, false>), dim3(grid), dim3(256), 0, st, N, rows_f32, ld_rows, d, graph, R, targets,
                           T, in_lims, in_ids, kp, out_status);
    else   // (float32 rows read through l2_f32: with_score_mode says why)
        hipLaunchKernelGGL((graph_link_reverse_kernel<l2_f32, false>), dim3(grid), dim3(256), 0, st, N,
                           reinterpret_cast<const l2_f32 *>(rows_f32), ld_rows, d, graph, R, targets, T, in_lims, in_ids, kp, out_status);
    TSIM_HIP_CHECK(hipGetLastError());
    return TSIM_OK;
}
