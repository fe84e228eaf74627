// Exact range search (tsim_cosine_range_scan / tsim_dot_range_scan / tsim_l2_range_scan / tsim_range_fill and their _tau forms): every corpus row
// whose exact score is >= tau (Euclidean: whose squared distance is <= the radius, which travels in tau / tau_q), tau one float per call or one per query (tau_q[q]); tsim_range_merge joins per-shard results.  Included by search.hip behind the exact-score helpers, the guard helpers and plan_collect, which it uses as they are.
//
// Pipeline of one scan:   range_setup  ->  K1 in COLLECT mode (k1_launch_collect, unchanged)  ->  range_finalize  ->  range_bf<count>
//          of one fill:   range_fill (status 1)  ->  range_bf<fill>  ->  range_bf_sort (status 2)
// The guard is simpler than top-k's: there is no k-th competitor, only the fixed tau.  A row with exact score s >= tau has an MFMA
// score m >= s - eps_q >= tau - eps_q (guard_eps bounds |m - s|), so collecting every row with m strictly above a threshold placed
// below tau - eps_q misses no hit; the exact re-score then drops the few rows of the band [tau - eps_q, tau) that came with them.
// SM_L2: the operands are the augmented rows of the Euclidean top-k (l2_rows / l2_query_rows, ld = pad_dim(d + 1)), the exact
// scores are -dist^2 (rows of l2_f32) in every list until range_fill_negate flips the sign of the output, and the threshold is
// guard_tau_l2(r, eps_q, nqs, |q|^2): every row whose float32 distance could be <= r has an MFMA score above it.  A hit is
// es >= -r, which on es = -dist^2 is exactly dist^2 <= r (false for NaN, true for r = 0 against -0).
#pragma once

namespace tsim {

constexpr int RS_CAP = TSIM_RANGE_SLOT_CAP;   // entries of one query's collect buffer (and of range_finalize's LDS sort)
static_assert(RS_CAP >= 1024 && (RS_CAP & (RS_CAP - 1)) == 0, "TSIM_RANGE_SLOT_CAP: a power of two >= 1024");
enum { RCTL_QCOUNT = 0, RCTL_NUNRES = 1, RCTL_WORDS = 4 };
enum { RST_COLLECTED = 1, RST_EXACT = 2 };   // out_status values (include/tsim.h)

struct RangeArgs {
    float tau;                // the threshold of every query when tau_q is null (SM_L2: the squared radius)
    const float *tau_q;       // device [Q], or null: the threshold of query q (the _tau entries)
    int ld;
    const float *rho_c_max;   // device, or null (cosine: the a-priori bound)
    float rho_c_default;
    const float *c_maxnorm;   // SM_DOT: the corpus rows' max-norm word; SM_L2: the same word (A = dot_scale of it)
    int *ctl;                 // RCTL_* words
    int *gthr;                // [Q] collect threshold of slot q as an ordered int (k1_topk.h float_to_ordered)
    int *qmap;                // [Q] identity: slot q = query q
    int *cnt;                 // [Q] entries the collect pass appended (may exceed RS_CAP)
    float *eps;               // [Q] the query's bound on |MFMA score - exact score| (DOT: in the MFMA domain)
    int *status;              // [Q] RST_*
    int *nhit;                // [Q] status 1: sorted hits held in buf
    int *unres_q;             // [Q] status-2 queries, compact (ctl[RCTL_NUNRES] of them)
    unsigned long long *cursor;   // [Q] fill: entries of a status-2 query written so far
    unsigned long long *buf;      // [Q][RS_CAP] score bits | (uint64)(shard row) << 32
};

// The threshold of query q.  Every kernel compares against this one value, so a query of a _tau call is answered exactly as by
// the scalar call with tau = tau_q[q]; a NaN there fails every comparison below (no finite collect threshold: status 2, no hit).
__device__ __forceinline__ float rs_tau(const RangeArgs &a, int64_t q) { return a.tau_q ? a.tau_q[q] : a.tau; }
// the value exact scores are compared with (>=): tau; rows of l2_f32 score -dist^2, so the radius changes sign (exactly)
template <bool L2>
__device__ __forceinline__ float rs_cut(const RangeArgs &a, int64_t q) { return L2 ? -rs_tau(a, q) : rs_tau(a, q); }

// entry order (score desc, row asc); RS_PAD = (-inf, row 2^32 - 1) ranks behind every real entry (rows are < 2^31)
constexpr unsigned long long RS_PAD = 0xffffffffff800000ull;
__device__ __forceinline__ bool rs_before(unsigned long long a, unsigned long long b) {
    const float sa = __uint_as_float((uint32_t)a), sb = __uint_as_float((uint32_t)b);
    return sa > sb || (sa == sb && (uint32_t)(a >> 32) < (uint32_t)(b >> 32));
}

// sort e[0..n) by rs_before; n a power of two; a 256-thread workgroup (sl_sort on packed entries); barrier on return
__device__ __forceinline__ void rs_sort(unsigned long long *e, int n) {
    for (int size = 2; size <= n; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < n / 2; t += 256) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const unsigned long long ei = e[i], ej = e[j];
                if ((i & size) == 0 ? rs_before(ej, ei) : rs_before(ei, ej)) {
                    e[i] = ej;
                    e[j] = ei;
                }
            }
            __syncthreads();
        }
}

// =====================================================================================================
// range_setup: one wave per query.  rho_q from the query's two rows, eps_q = guard_eps, then the collect threshold in the MFMA
// domain: cosine guard_tau(tau, eps_q) (a float strictly below tau - eps_q), dot guard_tau_dot(tau, eps_q, nq S) (below
// tau / (nq S) - eps_q with the conversion slack on the safe side).  Both return "collect everything" (-FLT_MAX) when no finite
// threshold is safe: tau = -inf, a non-finite S, eps_q = inf, a zero query with tau <= 0 whose quotient leaves the float range.
// Such a query would overflow any buffer: it is handed to the exact pass at once (status 2) and its slot collects nothing.
// SM_L2: rho_q over the d + 1 elements of the augmented row, the threshold guard_tau_l2 of the radius (no finite one for
// r = +inf, NaN, a non-finite |q|^2 or nqs).
// Writes everything k1_launch_collect reads: gthr, the identity qmap, qcount = Q, zeroed counters.
// =====================================================================================================
template <int SM>
__global__ __launch_bounds__(256) void range_setup_kernel(int64_t Q, const float *__restrict__ xq, int64_t ldq,
                                                          const unit_t *__restrict__ uq, int d, RangeArgs a) {
    constexpr bool DOT = SM == SM_DOT, L2 = SM == SM_L2;
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.ctl[RCTL_QCOUNT] = (int)Q;
        a.ctl[RCTL_NUNRES] = 0;
    }
    if (q >= Q) return;
    float eps, thr;
    if constexpr (L2) {
        ExactQuery<l2_f32> eqr;
        exact_load_query<l2_f32, NORM_SQ>(eqr, reinterpret_cast<const l2_f32 *>(xq) + q * ldq, d, lane);   // norm = |q|^2
        const double A = dot_scale(*a.c_maxnorm);
        const double nq = sqrt(eqr.norm + A * A);   // nq' of l2_query_rows_kernel, the same bits
        eps = guard_eps(query_rho_l2(eqr, uq + q * a.ld, d, A, nq, lane), *a.rho_c_max, a.ld);
        thr = guard_tau_l2(rs_tau(a, q), eps, l2_nqs(eqr.norm, A), eqr.norm);   // (the radius)
    } else {
        ExactQuery<float> eqr;
        exact_load_query<float, true>(eqr, xq + q * ldq, d, lane);   // norm = max(|q|, 1e-8): the scale the unit row was made with
        const float rho_c = a.rho_c_max ? *a.rho_c_max : a.rho_c_default;
        eps = guard_eps(query_rho<DOT>(eqr, uq + q * a.ld, d, lane), rho_c, a.ld);
        const float tau = rs_tau(a, q);
        if constexpr (DOT) thr = guard_tau_dot(tau, eps, eqr.norm * dot_scale(*a.c_maxnorm));
        else thr = guard_tau(tau, eps);
    }
    const bool everything = !(thr > -3.4e38f);
    if (lane != 0) return;
    a.gthr[q] = float_to_ordered(everything ? INFINITY : thr);
    a.qmap[q] = (int)q;
    a.cnt[q] = 0;
    a.eps[q] = eps;
    a.status[q] = everything ? RST_EXACT : RST_COLLECTED;
    a.nhit[q] = 0;
}

// =====================================================================================================
// range_finalize: one workgroup per query.  Every collected row is re-scored exactly (exact_score_batch: the bits the top-k
// entries return), the bound |m - s| <= eps_q is checked on each, rows below tau are dropped, the survivors are sorted in LDS by
// (score desc, row asc) and written back over the query's collect buffer for the fill.  An overflowed buffer, or a row on which
// the bound fails (operands that are not images of the float32 rows), sends the query to the exact pass.
// =====================================================================================================
template <int SM>
__global__ __launch_bounds__(256) void range_finalize_kernel(int64_t Q, const float *__restrict__ xq, int64_t ldq,
                                                             const float *__restrict__ xc, int64_t ldc, int d,
                                                             int64_t *__restrict__ out_counts, int32_t *__restrict__ out_status,
                                                             RangeArgs a) {
    constexpr bool COS = SM == SM_COS, DOT = SM == SM_DOT, L2 = SM == SM_L2;
    using T = std::conditional_t<L2, l2_f32, float>;   // (l2_f32: a struct of one float, the layout of the float32 rows)
    const T *tq = reinterpret_cast<const T *>(xq), *tc = reinterpret_cast<const T *>(xc);
    __shared__ unsigned long long ent[RS_CAP];
    __shared__ int s_keep, s_bad;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t q = blockIdx.x; q < Q; q += gridDim.x) {
        const int n = a.cnt[q];
        bool exact = a.status[q] == RST_EXACT || n > RS_CAP;   // workgroup-uniform
        int keep = 0;
        if (!exact) {
            if (threadIdx.x == 0) {
                s_keep = 0;
                s_bad = 0;
            }
            __syncthreads();
            int np = 64;
            while (np < n) np <<= 1;   // <= RS_CAP
            ExactQuery<T> eqr;
            exact_load_query<T, L2 ? NORM_SQ : NORM_COS>(eqr, tq + q * ldq, d, lane);
            double nqs = 1.0;
            if constexpr (DOT) nqs = eqr.norm * dot_scale(*a.c_maxnorm);
            if constexpr (L2) nqs = l2_nqs(eqr.norm, dot_scale(*a.c_maxnorm));
            const float eps = a.eps[q], tau = rs_cut<L2>(a, q);
            unsigned long long *slot = a.buf + q * RS_CAP;
            bool bad = false;
            int mine = 0;
            for (int g0 = wave * 64; g0 < np; g0 += 256) {   // wave-uniform
                const int e = g0 + lane;
                unsigned long long v = RS_PAD;
                if (g0 < n) {
                    const unsigned long long in = slot[e < n ? e : g0];
                    const int row = (int)(in >> 32);
                    const int nvalid = n - g0 < 64 ? n - g0 : 64;
                    const float es = wave_scores<T, COS>(eqr, tc, ldc, row, nvalid, d, lane);
                    if (e < n) {
                        const float ms = __uint_as_float((uint32_t)in);
                        float err;
                        if constexpr (DOT) err = (float)fabs((double)ms - (double)es / nqs);
                        else if constexpr (L2) err = l2_err(ms, es, nqs, eqr.norm);
                        else err = fabsf(ms - es);
                        if (!(err <= eps)) bad = true;
                        if (es >= tau) {
                            v = (unsigned long long)__float_as_uint(es) | ((unsigned long long)(uint32_t)row << 32);
                            ++mine;
                        }
                    }
                }
                ent[e] = v;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
            if (lane == 0 && mine) atomicAdd(&s_keep, mine);
            if (__any(bad) && lane == 0) s_bad = 1;
            __syncthreads();
            rs_sort(ent, np);
            exact = s_bad != 0;
            keep = s_keep;
            if (!exact)
                for (int t = threadIdx.x; t < keep; t += 256) slot[t] = ent[t];
        }
        if (threadIdx.x == 0) {
            a.status[q] = exact ? RST_EXACT : RST_COLLECTED;
            a.nhit[q] = exact ? 0 : keep;
            out_counts[q] = exact ? 0 : keep;   // (exact: range_bf_count adds the hits up)
            if (out_status) out_status[q] = exact ? RST_EXACT : RST_COLLECTED;
            if (exact) a.unres_q[atomicAdd(a.ctl + RCTL_NUNRES, 1)] = (int)q;
        }
        __syncthreads();
    }
}

// =====================================================================================================
// Exact pass for status-2 queries: every row of the shard scored with the arithmetic of bf_partial_kernel (exact_score's bits).
//   (T = l2_f32: the rows scored as -dist^2 against -radius; COS is false then)
//   range_bf_kernel<COS, FILL = false>: workgroup (chunk c, slot u) counts the chunk's hits of query unres_q[u] into out_counts;
//   range_bf_kernel<COS, FILL = true>:  the same pass writes each hit straight into the query's segment [lims[q], lims[q+1]) of
//                                       the output (no per-query scratch: a query may hit the whole shard), in arrival order;
//   range_bf_sort_kernel:               one workgroup per query sorts its segment in place by (score desc, index asc).
// =====================================================================================================
constexpr int RS_BF_MAXCH = 256;

template <bool COS, bool FILL, typename T = float>
__global__ __launch_bounds__(256) void range_bf_kernel(int64_t Q, int64_t N, int rows_per_chunk, const float *__restrict__ xq,
                                                       int64_t ldq, const float *__restrict__ xc, int64_t ldc, int d,
                                                       int64_t *__restrict__ out_counts, const int64_t *__restrict__ lims,
                                                       float *__restrict__ out_s, int64_t *__restrict__ out_i, int64_t idx_offset,
                                                       RangeArgs a) {
    static_assert(!(COS && is_l2_rows<T>), "rows of l2_f32 have no cosine");
    const T *tq = reinterpret_cast<const T *>(xq), *tc = reinterpret_cast<const T *>(xc);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int nu = a.ctl[RCTL_NUNRES];
    nu = nu < Q ? nu : (int)Q;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_chunk;
    const int64_t r1 = r0 + rows_per_chunk < N ? r0 + rows_per_chunk : N;
    for (int u = blockIdx.y; u < nu; u += gridDim.y) {
        const int q = a.unres_q[u];
        const float tau = rs_cut<is_l2_rows<T>>(a, q);
        ExactQuery<T> eqr;
        exact_load_query<T, COS>(eqr, tq + (int64_t)q * ldq, d, lane);
        int64_t seg0 = 0, seglen = 0;
        if constexpr (FILL) {
            seg0 = lims[q];
            seglen = lims[q + 1] - seg0;
        }
        int count = 0;
        for (int64_t g0 = r0 + wave * 64; g0 < r1; g0 += 256) {   // wave-uniform
            const int nvalid = r1 - g0 < 64 ? (int)(r1 - g0) : 64;
            const int row = (int)(g0 + (lane < nvalid ? lane : 0));
            const float s = wave_scores<T, COS>(eqr, tc, ldc, row, nvalid, d, lane);
            const bool hit = lane < nvalid && s >= tau;
            const unsigned long long hits = __ballot(hit);
            if (hits == 0) continue;
            if constexpr (FILL) {
                unsigned long long pos = 0;
                if (lane == 0) pos = atomicAdd(a.cursor + q, (unsigned long long)__popcll(hits));
                pos = __shfl(pos, 0, 64) + __popcll(hits & ((1ull << lane) - 1ull));
                if (hit && (int64_t)pos < seglen) {   // (a segment shorter than the count the scan reported is never overrun)
                    out_s[seg0 + pos] = s;
                    out_i[seg0 + pos] = (int64_t)row + idx_offset;
                }
            } else {
                count += __popcll(hits);
            }
        }
        if constexpr (!FILL)
            if (lane == 0 && count) atomicAdd(reinterpret_cast<unsigned long long *>(out_counts + q), (unsigned long long)count);
    }
}

// In-place sort of one segment by (score desc, index asc): the bitonic network in its all-ascending form (the first step of
// every merge pairs i with i ^ (size - 1), the others i with i + stride), which sorts ANY length: positions >= n stand for
// entries that rank last, no exchange ever moves one, so pairs that reach past n are skipped.  Blocks of RS_SORT_B entries are
// sorted, and later finished after each merge's long strides, in LDS; only strides >= RS_SORT_B touch global memory (a barrier
// orders a workgroup's own global accesses).  1 024 threads.
constexpr int RS_SORT_B = 4096;
constexpr int RS_SORT_T = 1024;

__device__ __forceinline__ void rs_cmpx(float *s, int64_t *ix, int64_t i, int64_t j) {
    const float si = s[i], sj = s[j];
    const int64_t ii = ix[i], ij = ix[j];
    if (key_before(sj, ij, si, ii)) {
        s[i] = sj;
        s[j] = si;
        ix[i] = ij;
        ix[j] = ii;
    }
}

__device__ __forceinline__ void rs_pair(bool flip, int64_t t, int64_t stride, int64_t size, int64_t &i, int64_t &j) {
    if (flip) {
        i = (t / stride) * size + (t % stride);
        j = (t / stride) * size + size - 1 - (t % stride);
    } else {
        i = 2 * t - (t & (stride - 1));
        j = i + stride;
    }
}

// every block of RS_SORT_B entries through LDS.  WHOLE: the merges of size 2 .. RS_SORT_B (sorts the block); else the strides
// RS_SORT_B/2 .. 1 of a larger merge whose long strides have run in global memory.
template <bool WHOLE>
__device__ __forceinline__ void rs_sort_blocks(float *s, int64_t *ix, int64_t n, float *ls, int64_t *li) {
    for (int64_t b0 = 0; b0 < n; b0 += RS_SORT_B) {
        const int nl = n - b0 < RS_SORT_B ? (int)(n - b0) : RS_SORT_B;
        for (int t = threadIdx.x; t < nl; t += RS_SORT_T) {
            ls[t] = s[b0 + t];
            li[t] = ix[b0 + t];
        }
        __syncthreads();
        // (WHOLE: a merge whose upper half lies past the block's end has nothing to do)
        for (int size = WHOLE ? 2 : RS_SORT_B; size <= RS_SORT_B && (!WHOLE || (size >> 1) < nl); size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int t = threadIdx.x; t < RS_SORT_B / 2; t += RS_SORT_T) {
                    int64_t i, j;
                    rs_pair(WHOLE && stride == size >> 1, t, stride, size, i, j);
                    if (j < nl) rs_cmpx(ls, li, i, j);
                }
                __syncthreads();
            }
        for (int t = threadIdx.x; t < nl; t += RS_SORT_T) {
            s[b0 + t] = ls[t];
            ix[b0 + t] = li[t];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(RS_SORT_T) void range_bf_sort_kernel(int64_t Q, const int64_t *__restrict__ lims, float *out_s,
                                                                   int64_t *out_i, RangeArgs a) {
    __shared__ float ls[RS_SORT_B];
    __shared__ int64_t li[RS_SORT_B];
    int nu = a.ctl[RCTL_NUNRES];
    nu = nu < Q ? nu : (int)Q;
    for (int u = blockIdx.x; u < nu; u += gridDim.x) {
        const int q = a.unres_q[u];
        float *s = out_s + lims[q];
        int64_t *ix = out_i + lims[q];
        const int64_t n = lims[q + 1] - lims[q];
        if (n < 2) continue;   // workgroup-uniform
        rs_sort_blocks<true>(s, ix, n, ls, li);
        int64_t npow = RS_SORT_B;
        while (npow < n) npow <<= 1;
        for (int64_t size = 2 * RS_SORT_B; size <= npow; size <<= 1) {
            for (int64_t stride = size >> 1; stride >= RS_SORT_B; stride >>= 1) {
                for (int64_t t = threadIdx.x; t < npow / 2; t += RS_SORT_T) {
                    int64_t i, j;
                    rs_pair(stride == size >> 1, t, stride, size, i, j);
                    if (j < n) rs_cmpx(s, ix, i, j);
                }
                __syncthreads();
            }
            rs_sort_blocks<false>(s, ix, n, ls, li);
        }
    }
}

// status-1 queries: the sorted hits range_finalize left in the collect buffer go to [lims[q], lims[q+1]).  One wave per query.
__global__ __launch_bounds__(256) void range_fill_kernel(int64_t Q, const int64_t *__restrict__ lims, float *__restrict__ out_s,
                                                         int64_t *__restrict__ out_i, int64_t idx_offset, RangeArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= Q || a.status[q] != RST_COLLECTED) return;
    const int64_t seg0 = lims[q], seglen = lims[q + 1] - seg0;
    const int n = a.nhit[q] < seglen ? a.nhit[q] : (int)seglen;
    for (int t = lane; t < n; t += 64) {
        const unsigned long long e = a.buf[q * RS_CAP + t];
        out_s[seg0 + t] = __uint_as_float((uint32_t)e);
        out_i[seg0 + t] = (int64_t)(uint32_t)(e >> 32) + idx_offset;
    }
}

// SM_L2, the last kernel of a fill: the segments hold -dist^2 in (score desc, index asc) order; the sign flip (exact) leaves
// squared distances in (distance asc, index asc) order.  The host does not know T = lims[Q]: the kernel reads it.
__global__ __launch_bounds__(256) void range_fill_negate_kernel(float *__restrict__ out_s, const int64_t *__restrict__ total) {
    const int64_t n = *total;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out_s[i] = -out_s[i];
}

// Workspace layout of one range scan + fill (byte offsets)
struct RangeWs {
    size_t ctl, gthr, qmap, cnt, eps, status, nhit, unres_q, cursor, buf, total;
};

static void plan_workspace_range(int64_t Q, RangeWs *w) {
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += align256(bytes); return at; };
    w->ctl = take(RCTL_WORDS * 4);
    w->gthr = take((size_t)Q * 4);
    w->qmap = take((size_t)Q * 4);
    w->cnt = take((size_t)Q * 4);
    w->eps = take((size_t)Q * 4);
    w->status = take((size_t)Q * 4);
    w->nhit = take((size_t)Q * 4);
    w->unres_q = take((size_t)Q * 4);
    w->cursor = take((size_t)Q * 8);
    w->buf = take((size_t)Q * RS_CAP * 8);
    w->total = o;
}

static RangeArgs make_range_args(const RangeWs &w, char *ws, float tau, const float *tau_q, int ld, const float *ec_rho_max, const float *ec_maxnorm) {
    RangeArgs a;
    a.tau = tau;
    a.tau_q = tau_q;
    a.ld = ld;
    a.rho_c_max = ec_rho_max;
    a.rho_c_default = rho_apriori(ld);
    a.c_maxnorm = ec_maxnorm;
    a.ctl = reinterpret_cast<int *>(ws + w.ctl);
    a.gthr = reinterpret_cast<int *>(ws + w.gthr);
    a.qmap = reinterpret_cast<int *>(ws + w.qmap);
    a.cnt = reinterpret_cast<int *>(ws + w.cnt);
    a.eps = reinterpret_cast<float *>(ws + w.eps);
    a.status = reinterpret_cast<int *>(ws + w.status);
    a.nhit = reinterpret_cast<int *>(ws + w.nhit);
    a.unres_q = reinterpret_cast<int *>(ws + w.unres_q);
    a.cursor = reinterpret_cast<unsigned long long *>(ws + w.cursor);
    a.buf = reinterpret_cast<unsigned long long *>(ws + w.buf);
    return a;
}

// chunks of the exact pass: at least 256 rows each, at most RS_BF_MAXCH (a single status-2 query still spreads over the chip)
static void plan_range_bf(int64_t N, int *nch, int *rows) {
    int64_t c = (N + 255) / 256;
    c = c < 1 ? 1 : c > RS_BF_MAXCH ? RS_BF_MAXCH : c;
    *rows = (int)((N + c - 1) / c);
    *nch = (int)((N + *rows - 1) / *rows);
}

static int range_check_shapes(const char *what, const float *eq_f32, int64_t ldq_f32, int64_t Q, const float *ec_f32, int64_t ldc_f32,
                              int64_t N, int d, float tau, const float *tau_q, const void *workspace, size_t workspace_bytes,
                              RangeWs *w) {
    TSIM_REQUIRE(tau_q || tau == tau, "%s: the threshold is NaN", what);   // (a NaN in tau_q[q]: query q has no hit, status 2)
    TSIM_REQUIRE(eq_f32 && ec_f32, "%s: the float32 matrices are required (there is no unit-rows-only range search)", what);
    TSIM_REQUIRE(Q > 0 && N > 0, "%s: empty input Q=%lld N=%lld", what, (long long)Q, (long long)N);
    TSIM_REQUIRE(N < (1ll << 31) - 64 && Q < (1ll << 31) - 512, "%s: shard too large for 32-bit row ids", what);
    TSIM_REQUIRE(d > 0 && d <= 64 * XS_MAXI && ldq_f32 >= d && ldc_f32 >= d, "%s: float32 row strides %lld/%lld < d=%d", what,
                 (long long)ldq_f32, (long long)ldc_f32, d);
    plan_workspace_range(Q, w);
    if (!workspace || workspace_bytes < w->total)
        return fail(TSIM_ENOMEM, "%s: workspace %zu B < %zu B", what, workspace_bytes, w->total);
    return TSIM_OK;
}

static int range_scan(int sm, const char *what, const void *eq, const float *eq_f32, int64_t ldq_f32, int64_t Q, const void *ec,
                      const float *ec_f32, int64_t ldc_f32, const float *ec_maxnorm, const float *ec_rho_max, int64_t N, int d, int ld,
                      float tau, const float *tau_q, int64_t *out_counts, int32_t *out_status, void *workspace, size_t workspace_bytes,
                      void *stream) {
    RangeWs w;
    int rc = range_check_shapes(what, eq_f32, ldq_f32, Q, ec_f32, ldc_f32, N, d, tau, tau_q, workspace, workspace_bytes, &w);
    if (rc) return rc;
    TSIM_REQUIRE(eq && ec && out_counts, "%s: null pointer", what);
    const int dw = d + (sm == SM_L2);   // width of the half operands (L2: one element longer than the rows)
    TSIM_REQUIRE(ld == tsim_pad_dim(dw) && ld > 0, "%s: rows must be padded to tsim_pad_dim(%d)=%d (got ld=%d)", what, dw, tsim_pad_dim(dw), ld);
    TSIM_REQUIRE((((uintptr_t)eq | (uintptr_t)ec) & 15) == 0, "%s: embedding matrices must be 16-byte aligned", what);
    hipStream_t st = as_stream(stream);
    const unit_t *uq = (const unit_t *)eq, *uc = (const unit_t *)ec;
    const RangeArgs a = make_range_args(w, reinterpret_cast<char *>(workspace), tau, tau_q, ld, ec_rho_max, ec_maxnorm);
    const dim3 qgrid((unsigned)((Q + 3) / 4));
    if (sm == SM_DOT) hipLaunchKernelGGL(range_setup_kernel<SM_DOT>, qgrid, dim3(256), 0, st, Q, eq_f32, ldq_f32, uq, d, a);
    else if (sm == SM_L2) hipLaunchKernelGGL(range_setup_kernel<SM_L2>, qgrid, dim3(256), 0, st, Q, eq_f32, ldq_f32, uq, d, a);
    else hipLaunchKernelGGL(range_setup_kernel<SM_COS>, qgrid, dim3(256), 0, st, Q, eq_f32, ldq_f32, uq, d, a);
    TSIM_HIP_CHECK(hipGetLastError());
    TopkPlan cp;
    plan_collect(Q, N, ld, &cp);
    K1Collect coll{};
    coll.qcount = a.ctl + RCTL_QCOUNT;
    coll.qmap = a.qmap;
    coll.buf = a.buf;
    coll.cnt = a.cnt;
    coll.cap = RS_CAP;
    rc = k1_launch_collect(cp, ld, uq, Q, uc, N, a.gthr, coll, st);
    if (rc) return rc;
    const dim3 fgrid((unsigned)(Q < 4096 ? Q : 4096));
    if (sm == SM_DOT)
        hipLaunchKernelGGL(range_finalize_kernel<SM_DOT>, fgrid, dim3(256), 0, st, Q, eq_f32, ldq_f32, ec_f32, ldc_f32, d, out_counts,
                           out_status, a);
    else if (sm == SM_L2)
        hipLaunchKernelGGL(range_finalize_kernel<SM_L2>, fgrid, dim3(256), 0, st, Q, eq_f32, ldq_f32, ec_f32, ldc_f32, d, out_counts,
                           out_status, a);
    else
        hipLaunchKernelGGL(range_finalize_kernel<SM_COS>, fgrid, dim3(256), 0, st, Q, eq_f32, ldq_f32, ec_f32, ldc_f32, d, out_counts,
                           out_status, a);
    TSIM_HIP_CHECK(hipGetLastError());
    int nch, rows;
    plan_range_bf(N, &nch, &rows);
    const dim3 bgrid((unsigned)nch, (unsigned)(Q < 64 ? Q : 64));   // (workgroups leave at once when no query took status 2)
    if (sm == SM_DOT)
        hipLaunchKernelGGL((range_bf_kernel<false, false>), bgrid, dim3(256), 0, st, Q, N, rows, eq_f32, ldq_f32, ec_f32, ldc_f32, d,
                           out_counts, (const int64_t *)nullptr, (float *)nullptr, (int64_t *)nullptr, (int64_t)0, a);
    else if (sm == SM_L2)
        hipLaunchKernelGGL((range_bf_kernel<false, false, l2_f32>), bgrid, dim3(256), 0, st, Q, N, rows, eq_f32, ldq_f32, ec_f32, ldc_f32,
                           d, out_counts, (const int64_t *)nullptr, (float *)nullptr, (int64_t *)nullptr, (int64_t)0, a);
    else
        hipLaunchKernelGGL((range_bf_kernel<true, false>), bgrid, dim3(256), 0, st, Q, N, rows, eq_f32, ldq_f32, ec_f32, ldc_f32, d,
                           out_counts, (const int64_t *)nullptr, (float *)nullptr, (int64_t *)nullptr, (int64_t)0, a);
    TSIM_HIP_CHECK(hipGetLastError());
    return TSIM_OK;
}

// =====================================================================================================
// tsim_range_merge: R CSR results of the same Q queries over disjoint row sets (global indices; every segment sorted by
// (score desc, index asc)) -> one CSR result in the same order.  Merge by rank: an entry's place in its query's output segment
// is its offset within its own segment plus, for every other list, the number of that list's entries of the query that rank
// ahead of it, found by binary search (entries equal in score AND index rank by list number, so the result is a permutation of
// the input whatever the data).  No scratch, no LDS, no dependence on a segment's length; every output slot is written exactly
// once, by the thread of the entry that belongs there, so the result is deterministic.
// Work is cut by ENTRY, not by query: thread t of the launch takes entry p of the query-major enumeration of all input entries
// (query q holds the positions [lims_out[q], lims_out[q+1]), its lists one after the other), so one query that returns whole
// shards spreads over the chip like 4 096 queries of a hundred hits.  Finding (q, list) costs log2 Q + R cached reads, small
// against the R binary searches.  Whatever the data, a write lands inside the entry's own output segment: the place is < the sum
// of the R segment lengths, and it is checked against the segment lims_out gives.
// ASC (tsim_range_merge_asc): the segments are sorted by (score asc, index asc) — squared distances — and so is the output.
// =====================================================================================================
constexpr int RM_PER = 4;   // entries per thread

template <bool ASC>
__global__ __launch_bounds__(256) void range_merge_kernel(int R, int64_t Q, const int64_t *__restrict__ lims_in,
                                                          const float *__restrict__ s_in, const int64_t *__restrict__ i_in,
                                                          const int64_t *__restrict__ lims_out, float *__restrict__ out_s,
                                                          int64_t *__restrict__ out_i, int64_t total) {
    for (int k = 0; k < RM_PER; ++k) {
        const int64_t p = ((int64_t)blockIdx.x * RM_PER + k) * 256 + threadIdx.x;
        if (p >= total) return;
        int64_t lo = 0, hi = Q;   // the query whose output segment holds position p: the first q with lims_out[q + 1] > p
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (lims_out[mid + 1] > p) hi = mid;
            else lo = mid + 1;
        }
        if (lo >= Q) return;      // (total beyond lims_out[Q])
        const int64_t q = lo, seg0 = lims_out[q], seglen = lims_out[q + 1] - seg0;
        int64_t o = p - seg0;     // position among the query's input entries, list after list
        if (o < 0) continue;
        int r = 0;
        int64_t b0 = 0;
        for (; r < R; ++r) {
            b0 = lims_in[r * (Q + 1) + q];
            const int64_t len = lims_in[r * (Q + 1) + q + 1] - b0;
            if (o < len) break;
            if (len > 0) o -= len;
        }
        if (r == R) continue;     // (lims_out counts more entries than the lists hold)
        const float s = s_in[b0 + o];
        const int64_t i = i_in[b0 + o];
        int64_t pos = o;
        for (int r2 = 0; r2 < R; ++r2) {
            if (r2 == r) continue;
            const int64_t b = lims_in[r2 * (Q + 1) + q];
            int64_t l = 0, h = lims_in[r2 * (Q + 1) + q + 1] - b;
            while (l < h) {       // entries of list r2 ahead of (s, i): strictly ahead, and the equal one too when r2 < r
                const int64_t mid = (l + h) >> 1;
                const float ms = s_in[b + mid];
                bool ahead = ASC ? ms < s : ms > s;
                if (ms == s) {    // (the index is read on a tie of the score only)
                    const int64_t mi = i_in[b + mid];
                    ahead = mi < i || (mi == i && r2 < r);
                }
                if (ahead) l = mid + 1;
                else h = mid;
            }
            pos += l;
        }
        if (pos < seglen) {
            out_s[seg0 + pos] = s;
            out_i[seg0 + pos] = i;
        }
    }
}
}  // namespace tsim

extern "C" size_t tsim_range_workspace_bytes(int64_t Q, int64_t N) {
    if (Q <= 0 || N <= 0) return 0;
    tsim::RangeWs w;
    tsim::plan_workspace_range(Q, &w);
    return w.total;
}

extern "C" int tsim_cosine_range_scan_tau(const void *eq, const float *eq_f32, int64_t ldq_f32, int64_t Q, const void *ec,
                                          const float *ec_f32, int64_t ldc_f32, const float *ec_rho_max, int64_t N, int d, int ld,
                                          const float *tau_q, int64_t *out_counts, int32_t *out_status, void *workspace,
                                          size_t workspace_bytes, void *stream) {
    TSIM_REQUIRE(tau_q, "cosine_range_scan_tau: null threshold array");
    return tsim::range_scan(tsim::SM_COS, "cosine_range_scan_tau", eq, eq_f32, ldq_f32, Q, ec, ec_f32, ldc_f32, nullptr, ec_rho_max, N,
                            d, ld, 0.f, tau_q, out_counts, out_status, workspace, workspace_bytes, stream);
}

extern "C" int tsim_cosine_range_scan(const void *eq, const float *eq_f32, int64_t ldq_f32, int64_t Q, const void *ec,
                                      const float *ec_f32, int64_t ldc_f32, const float *ec_rho_max, int64_t N, int d, int ld,
                                      float tau, int64_t *out_counts, int32_t *out_status, void *workspace, size_t workspace_bytes,
                                      void *stream) {
    return tsim::range_scan(tsim::SM_COS, "cosine_range_scan", eq, eq_f32, ldq_f32, Q, ec, ec_f32, ldc_f32, nullptr, ec_rho_max, N, d,
                            ld, tau, nullptr, out_counts, out_status, workspace, workspace_bytes, stream);
}

static int dot_range_scan(const char *what, const void *eq, const float *eq_f32, int64_t ldq_f32, int64_t Q, const void *ec,
                          const float *ec_f32, int64_t ldc_f32, const float *ec_maxnorm, const float *ec_rho_max, int64_t N, int d, int ld,
                          float tau, const float *tau_q, int64_t *out_counts, int32_t *out_status, void *workspace,
                          size_t workspace_bytes, void *stream) {
    using namespace tsim;
    TSIM_REQUIRE(tau_q || tau == tau, "%s: the threshold is NaN", what);
    TSIM_REQUIRE(eq_f32 && ec_f32, "%s: the float32 matrices are required", what);
    TSIM_REQUIRE(ec_maxnorm && ec_rho_max, "%s: the corpus rows' max-norm word and measured rho_max are required", what);
    return range_scan(SM_DOT, what, eq, eq_f32, ldq_f32, Q, ec, ec_f32, ldc_f32, ec_maxnorm, ec_rho_max, N, d, ld, tau, tau_q,
                      out_counts, out_status, workspace, workspace_bytes, stream);
}

extern "C" int tsim_dot_range_scan(const void *eq, const float *eq_f32, int64_t ldq_f32, int64_t Q, const void *ec,
                                   const float *ec_f32, int64_t ldc_f32, const float *ec_maxnorm, const float *ec_rho_max, int64_t N,
                                   int d, int ld, float tau, int64_t *out_counts, int32_t *out_status, void *workspace,
                                   size_t workspace_bytes, void *stream) {
    return dot_range_scan("dot_range_scan", eq, eq_f32, ldq_f32, Q, ec, ec_f32, ldc_f32, ec_maxnorm, ec_rho_max, N, d, ld, tau, nullptr,
                          out_counts, out_status, workspace, workspace_bytes, stream);
}

extern "C" int tsim_dot_range_scan_tau(const void *eq, const float *eq_f32, int64_t ldq_f32, int64_t Q, const void *ec,
                                       const float *ec_f32, int64_t ldc_f32, const float *ec_maxnorm, const float *ec_rho_max,
                                       int64_t N, int d, int ld, const float *tau_q, int64_t *out_counts, int32_t *out_status,
                                       void *workspace, size_t workspace_bytes, void *stream) {
    TSIM_REQUIRE(tau_q, "dot_range_scan_tau: null threshold array");
    return dot_range_scan("dot_range_scan_tau", eq, eq_f32, ldq_f32, Q, ec, ec_f32, ldc_f32, ec_maxnorm, ec_rho_max, N, d, ld, 0.f,
                          tau_q, out_counts, out_status, workspace, workspace_bytes, stream);
}

static int l2_range_scan(const char *what, const void *eq, const float *eq_f32, int64_t ldq_f32, int64_t Q, const void *ec,
                         const float *ec_f32, int64_t ldc_f32, const float *ec_maxnorm, const float *ec_rho_max, int64_t N, int d, int ld,
                         float radius, const float *radius_q, int64_t *out_counts, int32_t *out_status, void *workspace,
                         size_t workspace_bytes, void *stream) {
    using namespace tsim;
    TSIM_REQUIRE(radius_q || radius == radius, "%s: the radius is NaN", what);
    TSIM_REQUIRE(eq_f32 && ec_f32, "%s: the float32 matrices are required", what);
    TSIM_REQUIRE(ec_maxnorm && ec_rho_max, "%s: the corpus rows' max-norm word and measured rho_max are required", what);
    TSIM_REQUIRE(d > 0 && d < 64 * XS_MAXI, "%s: d=%d (1 .. %d: the half rows are d + 1 wide)", what, d, 64 * XS_MAXI - 1);
    return range_scan(SM_L2, what, eq, eq_f32, ldq_f32, Q, ec, ec_f32, ldc_f32, ec_maxnorm, ec_rho_max, N, d, ld, radius, radius_q,
                      out_counts, out_status, workspace, workspace_bytes, stream);
}

extern "C" int tsim_l2_range_scan(const void *eq_aug, const float *eq_f32, int64_t ldq_f32, int64_t Q, const void *ec_aug,
                                  const float *ec_f32, int64_t ldc_f32, const float *ec_maxnorm, const float *ec_rho_max, int64_t N,
                                  int d, int ld, float radius, int64_t *out_counts, int32_t *out_status, void *workspace,
                                  size_t workspace_bytes, void *stream) {
    return l2_range_scan("l2_range_scan", eq_aug, eq_f32, ldq_f32, Q, ec_aug, ec_f32, ldc_f32, ec_maxnorm, ec_rho_max, N, d, ld, radius,
                         nullptr, out_counts, out_status, workspace, workspace_bytes, stream);
}

extern "C" int tsim_l2_range_scan_tau(const void *eq_aug, const float *eq_f32, int64_t ldq_f32, int64_t Q, const void *ec_aug,
                                      const float *ec_f32, int64_t ldc_f32, const float *ec_maxnorm, const float *ec_rho_max,
                                      int64_t N, int d, int ld, const float *radius_q, int64_t *out_counts, int32_t *out_status,
                                      void *workspace, size_t workspace_bytes, void *stream) {
    TSIM_REQUIRE(radius_q, "l2_range_scan_tau: null radius array");
    return l2_range_scan("l2_range_scan_tau", eq_aug, eq_f32, ldq_f32, Q, ec_aug, ec_f32, ldc_f32, ec_maxnorm, ec_rho_max, N, d, ld, 0.f,
                         radius_q, out_counts, out_status, workspace, workspace_bytes, stream);
}

static int range_fill(const char *what, int space, const float *eq_f32, int64_t ldq_f32, int64_t Q, const float *ec_f32,
                      int64_t ldc_f32, int64_t N, int d, float tau, const float *tau_q, const int64_t *lims, float *out_scores,
                      int64_t *out_idx, int64_t idx_offset, void *workspace, size_t workspace_bytes, void *stream) {
    using namespace tsim;
    TSIM_REQUIRE(space == TSIM_SPACE_COSINE || space == TSIM_SPACE_DOT || space == TSIM_SPACE_L2, "%s: unknown space %d", what, space);
    TSIM_REQUIRE(space != TSIM_SPACE_L2 || d < 64 * XS_MAXI, "%s: d=%d (the Euclidean space takes d <= %d)", what, d, 64 * XS_MAXI - 1);
    RangeWs w;
    int rc = range_check_shapes(what, eq_f32, ldq_f32, Q, ec_f32, ldc_f32, N, d, tau, tau_q, workspace, workspace_bytes, &w);
    if (rc) return rc;
    // out_scores / out_idx may be null when the scan reported no hit at all (lims[Q] == 0): nothing is written then
    TSIM_REQUIRE(lims, "%s: null pointer", what);
    hipStream_t st = as_stream(stream);
    const RangeArgs a = make_range_args(w, reinterpret_cast<char *>(workspace), tau, tau_q, 0, nullptr, nullptr);
    TSIM_HIP_CHECK(hipMemsetAsync(a.cursor, 0, (size_t)Q * 8, st));
    hipLaunchKernelGGL(range_fill_kernel, dim3((unsigned)((Q + 3) / 4)), dim3(256), 0, st, Q, lims, out_scores, out_idx, idx_offset, a);
    TSIM_HIP_CHECK(hipGetLastError());
    int nch, rows;
    plan_range_bf(N, &nch, &rows);
    const dim3 bgrid((unsigned)nch, (unsigned)(Q < 64 ? Q : 64));
    if (space == TSIM_SPACE_DOT)
        hipLaunchKernelGGL((range_bf_kernel<false, true>), bgrid, dim3(256), 0, st, Q, N, rows, eq_f32, ldq_f32, ec_f32, ldc_f32, d,
                           (int64_t *)nullptr, lims, out_scores, out_idx, idx_offset, a);
    else if (space == TSIM_SPACE_L2)
        hipLaunchKernelGGL((range_bf_kernel<false, true, l2_f32>), bgrid, dim3(256), 0, st, Q, N, rows, eq_f32, ldq_f32, ec_f32, ldc_f32, d,
                           (int64_t *)nullptr, lims, out_scores, out_idx, idx_offset, a);
    else
        hipLaunchKernelGGL((range_bf_kernel<true, true>), bgrid, dim3(256), 0, st, Q, N, rows, eq_f32, ldq_f32, ec_f32, ldc_f32, d,
                           (int64_t *)nullptr, lims, out_scores, out_idx, idx_offset, a);
    TSIM_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(range_bf_sort_kernel, dim3((unsigned)(Q < 256 ? Q : 256)), dim3(RS_SORT_T), 0, st, Q, lims, out_scores, out_idx, a);
    TSIM_HIP_CHECK(hipGetLastError());
    if (space == TSIM_SPACE_L2) {   // every kernel above wrote -dist^2
        hipLaunchKernelGGL(range_fill_negate_kernel, dim3(1024), dim3(256), 0, st, out_scores, lims + Q);
        TSIM_HIP_CHECK(hipGetLastError());
    }
    return TSIM_OK;
}

extern "C" int tsim_range_fill(int space, const float *eq_f32, int64_t ldq_f32, int64_t Q, const float *ec_f32, int64_t ldc_f32,
                               int64_t N, int d, float tau, const int64_t *lims, float *out_scores, int64_t *out_idx,
                               int64_t idx_offset, void *workspace, size_t workspace_bytes, void *stream) {
    return range_fill("range_fill", space, eq_f32, ldq_f32, Q, ec_f32, ldc_f32, N, d, tau, nullptr, lims, out_scores, out_idx,
                      idx_offset, workspace, workspace_bytes, stream);
}

extern "C" int tsim_range_fill_tau(int space, const float *eq_f32, int64_t ldq_f32, int64_t Q, const float *ec_f32, int64_t ldc_f32,
                                   int64_t N, int d, const float *tau_q, const int64_t *lims, float *out_scores, int64_t *out_idx,
                                   int64_t idx_offset, void *workspace, size_t workspace_bytes, void *stream) {
    TSIM_REQUIRE(tau_q, "range_fill_tau: null threshold array");
    return range_fill("range_fill_tau", space, eq_f32, ldq_f32, Q, ec_f32, ldc_f32, N, d, 0.f, tau_q, lims, out_scores, out_idx,
                      idx_offset, workspace, workspace_bytes, stream);
}

template <bool ASC>
static int range_merge(const char *what, const int64_t *lims_in, const float *scores_in, const int64_t *idx_in, int nlists, int64_t Q,
                       const int64_t *lims_out, int64_t total, float *out_scores, int64_t *out_idx, void *stream) {
    using namespace tsim;
    TSIM_REQUIRE(nlists >= 1 && nlists <= TSIM_RANGE_MERGE_MAX_LISTS, "%s: %d lists (1 .. %d)", what, nlists,
                 TSIM_RANGE_MERGE_MAX_LISTS);
    TSIM_REQUIRE(Q >= 0 && total >= 0, "%s: bad shape Q=%lld total=%lld", what, (long long)Q, (long long)total);
    TSIM_REQUIRE(Q < (1ll << 31) - 512 && total < (1ll << 33), "%s: Q=%lld total=%lld too large for one launch", what, (long long)Q,
                 (long long)total);
    if (Q == 0 || total == 0) return TSIM_OK;
    TSIM_REQUIRE(lims_in && scores_in && idx_in && lims_out && out_scores && out_idx, "%s: null pointer", what);
    const int64_t per = 256 * (int64_t)RM_PER;
    hipLaunchKernelGGL(range_merge_kernel<ASC>, dim3((unsigned)((total + per - 1) / per)), dim3(256), 0, as_stream(stream), nlists, Q,
                       lims_in, scores_in, idx_in, lims_out, out_scores, out_idx, total);
    TSIM_HIP_CHECK(hipGetLastError());
    return TSIM_OK;
}

extern "C" int tsim_range_merge(const int64_t *lims_in, const float *scores_in, const int64_t *idx_in, int nlists, int64_t Q,
                                const int64_t *lims_out, int64_t total, float *out_scores, int64_t *out_idx, void *stream) {
    return range_merge<false>("range_merge", lims_in, scores_in, idx_in, nlists, Q, lims_out, total, out_scores, out_idx, stream);
}

extern "C" int tsim_range_merge_asc(const int64_t *lims_in, const float *scores_in, const int64_t *idx_in, int nlists, int64_t Q,
                                    const int64_t *lims_out, int64_t total, float *out_scores, int64_t *out_idx, void *stream) {
    return range_merge<true>("range_merge_asc", lims_in, scores_in, idx_in, nlists, Q, lims_out, total, out_scores, out_idx, stream);
}
