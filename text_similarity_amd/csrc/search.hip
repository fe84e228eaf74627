// Similarity-search kernels for gfx950 (MI355X): row L2-normalise, fused MFMA cosine + per-query top-k,
// candidate finalisation (fixed-order re-scoring), list merge, dense cos_sim, masked mean-pool.
//
// Reference call sites replaced (see include/tsim.h for the per-function citations):
//   /root/reference/src/pipeline/search_pipeline.py:73-78   expand_as + F.cosine_similarity + torch.topk
//   /root/reference/src/utils/metrics.py:81-101             cos_sim
//   /root/reference/src/modules/modules.py:158-171          AvgPoolingStrategy.forward
//   /root/reference/src/modules/modules.py:174-181          CLSPoolingStrategy.forward (and max / mean-sqrt-len pooling)
#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "common.h"
#include "k1_topk.h"

namespace tsim {

// =====================================================================================================
// l2norm_rows: one wave per row, canonical float64 scale (common.h).  HBM-bound: reads rows*d*(4|2) B, writes
// rows*ld_out*2 B.
// =====================================================================================================
template <typename T>
__device__ __forceinline__ float load_as_f32(const T *p);
template <>
__device__ __forceinline__ float load_as_f32<float>(const float *p) { return *p; }
template <>
__device__ __forceinline__ float load_as_f32<bf16_t>(const bf16_t *p) { return bf16_to_f32(*p); }
template <>
__device__ __forceinline__ float load_as_f32<unit_t>(const unit_t *p) { return (float)*p; }
// A float32 element of rows that are compared by Euclidean distance (tsim_l2_topk_ex): the exact-score routines below take
// squared differences of such rows where they take products of plain float rows.  The row type carries the metric, so the
// kernels of the other spaces keep their template arguments — and their code objects — as they were.
struct l2_f32 { float x; };
template <>
__device__ __forceinline__ float load_as_f32<l2_f32>(const l2_f32 *p) { return p->x; }
template <typename T>
constexpr bool is_l2_rows = std::is_same_v<T, l2_f32>;

// rho_max (optional): the largest rounding residual rho_r = || half(u_r) - u_r ||_2 of the rows written, u_r = the exact unit
// row x_r / max(|x_r|, eps) — the quantity the search's exactness guard is built on (guard_eps below).  Accumulated with an
// atomic max on the float's bit pattern (non-negative floats order like ints), so one word can span many calls (an index
// that grows): the caller zeroes it once.
template <typename T>
__global__ __launch_bounds__(256) void l2norm_rows_kernel(const T *__restrict__ x, int64_t rows, int d,
                                                          int64_t ld_in, unit_t *__restrict__ out, int ld_out,
                                                          float eps, float *__restrict__ rho_max) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const T *xr = x + row * ld_in;
    double ss = 0.0;
    for (int j = lane; j < d; j += 64) {
        const double v = (double)load_as_f32<T>(xr + j);
        ss = fma(v, v, ss);
    }
    const double inv = canonical_inv_norm(ss, eps);
    unit_t *o = out + row * (int64_t)ld_out;
    double r2 = 0.0;
    for (int j = lane; j < ld_out; j += 64) {
        unit_t hv = (unit_t)0;
        if (j < d) {
            const double u = (double)load_as_f32<T>(xr + j) * inv;
            hv = f64_to_f16(u);
            const double e = (double)(float)hv - u;
            r2 = fma(e, e, r2);
        }
        o[j] = hv;
    }
    if (rho_max) {
        const float rho = rho_round_up(sqrt(wave_sum_f64(r2)));
        if (lane == 0) rho_publish(rho_max, rho);
    }
}

// =====================================================================================================
// Operands of the inner-product search (tsim_dot_topk_ex), one wave per row like l2norm_rows.
//   max_norm_rows:   raises *maxnorm to an upper bound of the rows' L2 norms (common.h dot_scale); +inf for a row with a
//                    non-finite element.  Read-then-atomic like rho_publish.
//   dot_scaled_rows: out[r] = half(x[r] / S), S = dot_scale(*maxnorm), zero-padded to ld_out; rho_max raised to the row's
//                    residual || out[r] - x[r] / S ||_2 with every subnormal element counted as kept AND as flushed
//                    (flush_safe_err).  A non-finite word gives S = inf, zero rows (NaN where x is not finite) and rho = 2.
// =====================================================================================================
template <typename T>
__global__ __launch_bounds__(256) void max_norm_rows_kernel(const T *__restrict__ x, int64_t rows, int d, int64_t ld_in,
                                                            float *__restrict__ maxnorm) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const T *xr = x + row * ld_in;
    double ss = 0.0;
    for (int j = lane; j < d; j += 64) {
        const double v = (double)load_as_f32<T>(xr + j);
        ss = fma(v, v, ss);
    }
    const double n = sqrt(wave_sum_f64(ss));
    // (1 + 1e-12) covers the float64 rounding of the sum and the root; beyond the float range (or NaN) -> inf
    const float word = n < 3.0e38 ? f32_round_up(n * (1.0 + 1e-12)) : INFINITY;
    if (lane == 0) rho_publish(maxnorm, word);
}

template <typename T>
__global__ __launch_bounds__(256) void dot_scaled_rows_kernel(const T *__restrict__ x, int64_t rows, int d, int64_t ld_in,
                                                              const float *__restrict__ maxnorm, unit_t *__restrict__ out,
                                                              int ld_out, float *__restrict__ rho_max) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const double S = dot_scale(*maxnorm);
    const double inv = 1.0 / S;   // a power of two: x * inv is exact (0 when S = inf)
    const T *xr = x + row * ld_in;
    unit_t *o = out + row * (int64_t)ld_out;
    double r2 = 0.0;
    for (int j = lane; j < ld_out; j += 64) {
        unit_t hv = (unit_t)0;
        if (j < d) {
            const double v = (double)load_as_f32<T>(xr + j) * inv;
            hv = f64_to_f16(v);
            const double e = flush_safe_err((double)(float)hv, v);
            r2 = fma(e, e, r2);
        }
        o[j] = hv;
    }
    if (rho_max) {
        const float rho = S < INFINITY ? rho_round_up(sqrt(wave_sum_f64(r2))) : 2.f;
        if (lane == 0) rho_publish(rho_max, rho);
    }
}

// =====================================================================================================
// Operands of the Euclidean search (tsim_l2_topk_ex): rows one element longer, so that the MFMA's inner product ranks by
// distance (include/tsim.h).  A = dot_scale(*maxnorm), S = 2 A.  One wave per row like the kernels above.
//   l2_rows:       corpus row (c, -|c|^2 / (2A)) / S: |.| <= sqrt(1.25) / 2 < 1.  |c|^2 is the canonical float64 sum of
//                  l2norm_rows; 1 / S and 1 / (4 A^2) are powers of two, so every element is rounded once, to half.  rho_max as
//                  in dot_scaled_rows (flush-safe, over the d + 1 elements); a non-finite word gives zero rows and rho = 2.
//   l2_query_rows: query row (q, A) / nq', nq' = sqrt(|q|^2 + A^2) in float64, each element rounded once to half; a non-finite
//                  nq' gives a zero row (the search then answers the query by brute force).
// =====================================================================================================
template <typename T>
__global__ __launch_bounds__(256) void l2_rows_kernel(const T *__restrict__ x, int64_t rows, int d, int64_t ld_in,
                                                      const float *__restrict__ maxnorm, unit_t *__restrict__ out, int ld_out,
                                                      float *__restrict__ rho_max) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const double A = dot_scale(*maxnorm);
    const bool finite = A < INFINITY;
    const double inv = finite ? 0.5 / A : 0.0;   // 1 / S
    const T *xr = x + row * ld_in;
    double ss = 0.0;
    for (int j = lane; j < d; j += 64) {
        const double v = (double)load_as_f32<T>(xr + j);
        ss = fma(v, v, ss);
    }
    const double extra = finite ? -(wave_sum_f64(ss) * (inv * inv)) : 0.0;   // -|c|^2 / (2 A S)
    unit_t *o = out + row * (int64_t)ld_out;
    double r2 = 0.0;
    for (int j = lane; j < ld_out; j += 64) {
        unit_t hv = (unit_t)0;
        if (j <= d && finite) {
            const double v = j < d ? (double)load_as_f32<T>(xr + j) * inv : extra;
            hv = f64_to_f16(v);
            const double e = flush_safe_err((double)(float)hv, v);
            r2 = fma(e, e, r2);
        }
        o[j] = hv;
    }
    if (rho_max) {
        const float rho = finite ? rho_round_up(sqrt(wave_sum_f64(r2))) : 2.f;
        if (lane == 0) rho_publish(rho_max, rho);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void l2_query_rows_kernel(const T *__restrict__ x, int64_t rows, int d, int64_t ld_in,
                                                            const float *__restrict__ maxnorm, unit_t *__restrict__ out,
                                                            int ld_out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const double A = dot_scale(*maxnorm);
    const T *xr = x + row * ld_in;
    double ss = 0.0;
    for (int j = lane; j < d; j += 64) {
        const double v = (double)load_as_f32<T>(xr + j);
        ss = fma(v, v, ss);
    }
    const double nq = sqrt(wave_sum_f64(ss) + A * A);   // >= A > 0
    const bool finite = nq < INFINITY;
    const double inv = finite ? 1.0 / nq : 0.0;
    unit_t *o = out + row * (int64_t)ld_out;
    for (int j = lane; j < ld_out; j += 64) {
        unit_t hv = (unit_t)0;
        if (j <= d && finite) hv = f64_to_f16((j < d ? (double)load_as_f32<T>(xr + j) : A) * inv);
        o[j] = hv;
    }
}

// out_scores of an L2 call hold -dist^2 until the last kernel of the call: negation is exact, so the lists, merges and the
// (score desc, index asc) order of every kernel in between serve distances unchanged.  -(-inf) = +inf is the padding.
__global__ __launch_bounds__(256) void l2_negate_scores_kernel(float *__restrict__ s, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) s[i] = -s[i];
}

// =====================================================================================================
// Exact scores.  Two definitions, both evaluated in float64 in ONE canonical order and rounded once to float32, so that
// GPU and oracle agree bit for bit (oracle/search_ref._lane_sum): lane l accumulates the products of elements j = l,
// l + 64, ... in that order (fma of an exact product == multiply + add), then an xor butterfly 32, 16, .., 1.
//   COS = true  (float32 rows): the reference's score, F.cosine_similarity of the float32 embeddings
//                /root/reference/src/pipeline/search_pipeline.py:76-77: x.y / (max(|x|, eps) * max(|y|, eps))
//                (oracle/search_ref.exact_cosine);
//   COS = false (unit rows as stored): the inner product of the stored unit rows (oracle/search_ref.canonical_scores).
// MFMA scores only SELECT candidates; every score that is returned or compared for the final order is one of these.
// A third, for rows of l2_f32 (tsim_l2_topk_ex): -(squared Euclidean distance).  Lane l adds (q_j - c_j)^2 for j = l, l + 64, ...
// with the difference, the square and the sum each rounded to float64 on its own (the square of a float64 difference is not
// exact, so a fused multiply-add would not be restatable in numpy), the same butterfly, one rounding to float32, then the sign.
// =====================================================================================================
constexpr int XS_MAXI = 12;   // 64 * 12 = 768 elements per row at most
constexpr double XS_EPS = (double)1e-8f;
// what exact_load_query leaves in ExactQuery::norm (`false` / `true` of the cosine and inner-product callers: NONE / COS)
enum { NORM_NONE = 0, NORM_COS = 1, NORM_SQ = 2 };

template <typename T>
struct ExactQuery {
    double v[XS_MAXI];   // this lane's elements j = lane + 64 i of the query row (0 beyond d)
    double norm;         // NORM_COS: max(|q|, eps);  NORM_SQ (L2): |q|^2
};

// This lane's elements j = lane + 64 i, i < NI, of a row as float64 (0 beyond d).  BRANCH-FREE: the address of an element past
// the end is clamped to the row's last one and the value replaced after the load.  (`j < d ? load : 0` compiles to a branch
// around every load with s_waitcnt vmcnt(0) behind it: the six loads of a 384-wide row became six dependent round trips, the
// 16 candidates of a query 96 — 45 of the finalize kernel's 88 us at Q = 256.)  1 <= d <= 64 NI.
template <typename T, int NI>
__device__ __forceinline__ void row_elems_f64(double (&c)[NI], const T *row, int d, int lane) {
    float x[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int j = lane + 64 * i;
        x[i] = load_as_f32<T>(row + (j < d ? j : d - 1));
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) c[i] = lane + 64 * i < d ? (double)x[i] : 0.0;
}

template <typename T, int NORM, int NI>
__device__ __forceinline__ void exact_load_query_ni(ExactQuery<T> &q, const T *row, int d, int lane) {
    double c[NI];
    row_elems_f64<T, NI>(c, row, d, lane);
    double ss = 0.0;
#pragma unroll
    for (int i = 0; i < XS_MAXI; ++i) {
        q.v[i] = i < NI ? c[i < NI ? i : 0] : 0.0;
        ss = fma(q.v[i], q.v[i], ss);   // (+0 beyond d: the sum is that of the elements below d, in their order)
    }
    q.norm = 1.0;
    if constexpr (NORM == NORM_COS) q.norm = fmax(sqrt(wave_sum_f64(ss)), XS_EPS);
    if constexpr (NORM == NORM_SQ) q.norm = wave_sum_f64(ss);
}
template <typename T, int NORM>
__device__ __forceinline__ void exact_load_query(ExactQuery<T> &q, const T *row, int d, int lane) {
    if (d <= 64 * (XS_MAXI / 2)) exact_load_query_ni<T, NORM, XS_MAXI / 2>(q, row, d, lane);   // wave-uniform
    else exact_load_query_ni<T, NORM, XS_MAXI>(q, row, d, lane);
}
// the norm exact_load_query<T, NORM_COS> sets, from the elements already held (the same fma chain: the +0 terms change nothing)
template <typename T>
__device__ __forceinline__ double exact_query_norm(const ExactQuery<T> &q) {
    double ss = 0.0;
#pragma unroll
    for (int i = 0; i < XS_MAXI; ++i) ss = fma(q.v[i], q.v[i], ss);
    return fmax(sqrt(wave_sum_f64(ss)), XS_EPS);
}
// |q|^2 as exact_load_query<T, NORM_SQ> sets it, from the elements already held
template <typename T>
__device__ __forceinline__ double exact_query_sumsq(const ExactQuery<T> &q) {
    double ss = 0.0;
#pragma unroll
    for (int i = 0; i < XS_MAXI; ++i) ss = fma(q.v[i], q.v[i], ss);
    return wave_sum_f64(ss);
}

// acc + diff * diff with the product and the sum each rounded to float64 on its own.  Contraction is switched off for this
// block: under hipcc's default (fp-contract=fast) a product and a sum fuse into v_fma / v_fmac_f64, and the __dmul_rn /
// __dadd_rn of this ROCm's headers are a plain `*` and `+` that fuse just the same.
__device__ __forceinline__ double add_square_unfused(double acc, double diff) {
#pragma clang fp contract(off)
    const double sq = diff * diff;
    return acc + sq;
}

// per-lane partial sums of the query against one row: dot (and |row|^2 for COS); L2: the squared differences in `dot`.
// C is the element type of the corpus row.  It only says how an element is loaded (float32 rows: T itself; rows of IEEE half:
// unit_t, widened exactly by load_as_f32); the metric stays with T, the query's type, which ExactQuery carries.
template <typename T, bool COS, int NI, typename C = T>
__device__ __forceinline__ void exact_partials(const ExactQuery<T> &q, const C *row, int d, int lane, double &dot, double &cc) {
    double c[NI];
    row_elems_f64<C, NI>(c, row, d, lane);
    dot = 0.0;
    cc = 0.0;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        if constexpr (is_l2_rows<T>) {
            const double diff = q.v[i] - c[i];   // (0 - 0 beyond d: the sum is that of the elements below d)
            dot = add_square_unfused(dot, diff);
        } else {
            dot = fma(q.v[i], c[i], dot);
        }
        if constexpr (COS) cc = fma(c[i], c[i], cc);
    }
}

// exact score of the query against one row (all 64 lanes take part and get the same value)
template <typename T, bool COS>
__device__ __forceinline__ float exact_score(const ExactQuery<T> &q, const T *row, int d, int lane) {
    double dot, cc;
    if (d <= 64 * (XS_MAXI / 2)) exact_partials<T, COS, XS_MAXI / 2>(q, row, d, lane, dot, cc);   // wave-uniform
    else exact_partials<T, COS, XS_MAXI>(q, row, d, lane, dot, cc);
    dot = wave_sum_f64(dot);
    if constexpr (COS) {
        const double nc = fmax(sqrt(wave_sum_f64(cc)), XS_EPS);
        return (float)(dot / (q.norm * nc));
    }
    if constexpr (is_l2_rows<T>) return -(float)dot;
    return (float)dot;
}

// NB rows against the query at once: lane t0 + u (u < NB) returns the exact score of the row held (as my_i) by lane
// t0 + u < nvalid; other lanes return garbage.  Same bits as exact_score: per lane the same fma chains, and the wave sums are
// the SAME xor-butterfly trees (32, 16, .., 1) — evaluated as a reduce-scatter: with NV values to sum, a lane sends the half of
// them its partner keeps and adds what it receives to the half it keeps itself (own + partner commutes, so both lanes of a
// pair would have computed the same bits), NV/2 + NV/4 + .. exchanges instead of 6 NV.  All NB rows' loads are in flight
// together: one memory round trip per batch — at small Q this kernel is a chain of round trips and butterflies and nothing else
// (one wave per query, 64 workgroups at Q = 256: 45 of its 88 us were four dependent gathers of four rows each).
template <int N, int O, int NV>   // N values still held per lane, next exchange with lane ^ O (compile-time indices throughout)
__device__ __forceinline__ void butterfly_reduce_scatter(double (&acc)[NV], int lane) {
    if constexpr (O > 0) {
        if constexpr (N > 1) {
            const bool up = (lane & O) != 0;   // this lane keeps the upper half
#pragma unroll
            for (int v = 0; v < N / 2; ++v) {
                const double send = up ? acc[v] : acc[v + N / 2];
                const double keep = up ? acc[v + N / 2] : acc[v];
                acc[v] = keep + __shfl_xor(send, O, 64);
            }
            butterfly_reduce_scatter<N / 2, O / 2>(acc, lane);
        } else {
            acc[0] += __shfl_xor(acc[0], O, 64);
            butterfly_reduce_scatter<1, O / 2>(acc, lane);
        }
    }
}

template <typename T, bool COS, int NB, typename C = T>
__device__ __forceinline__ float exact_score_batch(const ExactQuery<T> &q, const C *xc, int64_t ldc, int my_i, int t0, int nvalid,
                                                   int d, int lane) {
    constexpr int NV = (COS ? 2 : 1) * NB;
    static_assert(NV >= 2 && NV <= 32 && (NV & (NV - 1)) == 0, "batch size");
    constexpr int LOG = NV == 32 ? 5 : NV == 16 ? 4 : NV == 8 ? 3 : NV == 4 ? 2 : 1;
    double acc[NV];
    const C *rows[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        const int t = t0 + u < nvalid ? t0 + u : t0;   // past the end: repeat a valid one, result unused
        rows[u] = xc + (int64_t)__shfl(my_i, t, 64) * ldc;
    }
    if (d <= 64 * (XS_MAXI / 2)) {   // wave-uniform
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            double dot, cc;
            exact_partials<T, COS, XS_MAXI / 2, C>(q, rows[u], d, lane, dot, cc);
            if constexpr (COS) { acc[2 * u] = dot; acc[2 * u + 1] = cc; }
            else acc[u] = dot;
        }
    } else {
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            double dot, cc;
            exact_partials<T, COS, XS_MAXI, C>(q, rows[u], d, lane, dot, cc);
            if constexpr (COS) { acc[2 * u] = dot; acc[2 * u + 1] = cc; }
            else acc[u] = dot;
        }
    }
    butterfly_reduce_scatter<NV, 32>(acc, lane);
    // value v ended up in the lanes with (lane >> (6 - LOG)) == v
    constexpr int SH = 6 - LOG;
    float score;
    if constexpr (COS) {
        const double other = __shfl_xor(acc[0], 1 << SH, 64);          // even v (dot) lanes receive cc
        const double nc = fmax(sqrt(other), XS_EPS);
        score = (float)(acc[0] / (q.norm * nc));
    } else if constexpr (is_l2_rows<T>) {
        score = -(float)acc[0];
    } else {
        score = (float)acc[0];
    }
    const int u = lane - t0;
    const int src = ((COS ? 2 * u : u) << SH) & 63;
    return __shfl(score, src, 64);
}

template <typename I>   // int row ids within a shard, int64_t ids across shards
__device__ __forceinline__ bool key_before(float s1, I i1, float s2, I i2) {
    // true if (s1,i1) ranks strictly ahead of (s2,i2)
    return s1 > s2 || (s1 == s2 && i1 < i2);
}
__device__ __forceinline__ float float_below(float f) {   // the next float towards -inf (finite f)
    if (f == 0.f) return -1.17549435e-38f;
    const int b = __float_as_int(f);
    return __int_as_float(f > 0.f ? b - 1 : b + 1);
}

// control words of one search call (zeroed on the stream before the first kernel)
enum { CTL_NFLAG = 0, CTL_NUNRES = 1, CTL_WORDS = 4 };
// per-query status written to out_status (all results are exact; the status says which pass produced them)
enum { ST_PASS1 = 0, ST_WIDENED = 1, ST_BRUTE = 2 };
// score modes of the kernels that see exact scores:
//   SM_UNIT: inner product of the unit rows as stored;  SM_COS: cosine of the float32 rows (tsim_cosine_topk_ex);
//   SM_DOT:  inner product of the float32 rows (tsim_dot_topk_ex).  The corpus operand is half(c / S) (dot_scaled_rows), the
//            query operand the unit row of q, so the MFMA score approximates q.c / (nq S), nq = max(|q|, 1e-8) (the scale
//            the unit row was made with): monotone in q.c for a fixed query, and bounded by guard_eps exactly as for COS.
//            Exact scores live in the other domain; dot_bound_up / guard_tau_dot convert with nqs = nq S.
//   SM_L2:   squared Euclidean distance of the float32 rows (tsim_l2_topk_ex).  Operands: l2_rows / l2_query_rows, one element
//            longer than the rows, so the MFMA score approximates (|q|^2 - dist^2) / (2 nqs), nqs = nq' S: falling in dist^2 for
//            a fixed query and bounded by guard_eps like the others (|q' / nq'| = 1, |c' / S| <= 1).  Exact scores are -dist^2;
//            l2_bound_low / guard_tau_l2 convert.
enum { SM_UNIT = 0, SM_COS = 1, SM_DOT = 2, SM_L2 = 3 };

struct GuardArgs {
    // COS (float32 rows given): eps = guard_eps(rho_q, rho_c, ld) — a BOUND on |MFMA score - exact score| for the query against
    // every row of the shard (common.h).  rho_q is computed from the query's two rows in the kernel; rho_c = *rho_c_max when
    // the caller has the measured residual maximum of the shard's unit rows (tsim_l2norm_rows), else the a-priori bound.
    // Unit rows only: the scores differ by float32 accumulation alone: eps = max(c1 * largest difference seen, floor),
    // floor = ld * 2^-23 (rigorous for unit rows; c1 covers callers whose rows are not quite unit).
    float c1;
    float floor;
    const float *rho_c_max;   // device, or null
    float rho_c_default;      // rho_apriori(ld)
    int ld;
    int *ctl;          // CTL_* words
    int *flag_q;       // [Q] flagged queries, compact
    int *flag_thr;     // [Q] per slot: collection threshold as an ordered int (k1_topk.h float_to_ordered)
    float *flag_eps;   // [Q] per slot: the query's eps (COS)
    int *unres_q;      // [Q] queries left to the brute-force pass, compact
    int *status;       // [Q] or null
    const float *c_maxnorm;   // SM_DOT: the corpus rows' max-norm word (device), S = dot_scale(*c_maxnorm); SM_L2: A = that, S = 2 A
};

// rho of a query row: || stored half row - exact unit row ||_2 from the float32 row already held in `q` (all 64 lanes take part).
// FLUSH (SM_DOT): subnormal elements count with the larger of their kept and flushed errors (flush_safe_err).
template <bool FLUSH = false>
__device__ __forceinline__ float query_rho(const ExactQuery<float> &q, const unit_t *urow, int d, int lane) {
    double r2 = 0.0;
    const double inv = 1.0 / q.norm;
    auto body = [&](auto nic) __attribute__((always_inline)) {
        constexpr int NI = decltype(nic)::value;
        double u[NI];
        row_elems_f64<unit_t, NI>(u, urow, d, lane);
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            double e = u[i] - q.v[i] * inv;   // (0 - 0 beyond d)
            if constexpr (FLUSH) e = flush_safe_err(u[i], q.v[i] * inv);
            r2 = fma(e, e, r2);
        }
    };
    if (d <= 64 * (XS_MAXI / 2)) body(std::integral_constant<int, XS_MAXI / 2>{});   // wave-uniform
    else body(std::integral_constant<int, XS_MAXI>{});
    return rho_round_up(sqrt(wave_sum_f64(r2)));
}
// SM_L2: rho of an augmented query row (q, A) / nq against its stored half row, over the d + 1 elements, flush-safe.
template <typename T>
__device__ __forceinline__ float query_rho_l2(const ExactQuery<T> &q, const unit_t *urow, int d, double A, double nq, int lane) {
    double r2 = 0.0;
    const double inv = 1.0 / nq;
    auto body = [&](auto nic) __attribute__((always_inline)) {
        constexpr int NI = decltype(nic)::value;
        double u[NI];
        row_elems_f64<unit_t, NI>(u, urow, d + 1, lane);
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const double e = flush_safe_err(u[i], (lane + 64 * i == d ? A : q.v[i]) * inv);   // (0 against 0 beyond d)
            r2 = fma(e, e, r2);
        }
    };
    if (d + 1 <= 64 * (XS_MAXI / 2)) body(std::integral_constant<int, XS_MAXI / 2>{});   // wave-uniform
    else body(std::integral_constant<int, XS_MAXI>{});
    return rho_round_up(sqrt(wave_sum_f64(r2)));
}
__device__ __forceinline__ float guard_rho_c(const GuardArgs &g) { return g.rho_c_max ? *g.rho_c_max : g.rho_c_default; }
// collection threshold for "every row whose exact score could reach `target`": MFMA score >= target - eps.  Returned one float
// below (target - eps) so that the float rounding of the subtraction is on the safe side; eps = inf -> collect everything.
__device__ __forceinline__ float guard_tau(float target, float eps) {
    if (!(eps < 3.0e38f) || !(target > -3.0e38f)) return -3.4028234e38f;
    float tau = float_below((float)((double)target - (double)eps));
    if ((double)tau + (double)eps >= (double)target) tau = float_below(tau);
    return tau;
}
// SM_DOT conversions between the MFMA domain (q.c / (nq S)) and the exact one (q.c), nqs = nq S (float64, > 0).  The float64
// operations round to within 2^-52 of the true value each; the 1e-15 slack puts every result on the safe side.
//   dot_bound_up:  an upper bound of the exact score of any row whose MFMA score is <= m, given |MFMA - exact / nqs| <= eps;
//   guard_tau_dot: a collection threshold for rows whose exact score could reach sk: every such row has an MFMA score > tau.
__device__ __forceinline__ double dot_bound_up(float m, float eps, double nqs) {
    const double b = ((double)m + (double)eps) * nqs;
    return b + fabs(b) * 1e-15;
}
__device__ __forceinline__ float guard_tau_dot(float sk, float eps, double nqs) {
    if (!(eps < 3.0e38f) || !(sk > -3.0e38f) || !(nqs > 0.0 && nqs < INFINITY)) return -3.4028234e38f;
    const double t = (double)sk / nqs;
    const double lo = t - (double)eps - (fabs(t) + (double)eps) * 1e-15;
    if (!(lo > -3.0e38)) return -3.4028234e38f;
    return float_below((float)lo);   // (float)lo is within one float of lo: one step down is below it
}

// SM_L2 conversions (proof: include/tsim.h tsim_l2_topk_ex).  qq = |q|^2 and nqs = nq' S in float64; dk = a float32 squared
// distance (the k-th of a list).  The MFMA score m of a row obeys |m - (|q|^2 - dist^2) / (2 nqs)| <= eps; 1e-13 in MFMA units and
// 1e-14 relative cover every float64 rounding on the way (qq, nq', the stored operands' definitions, the canonical dist^2).
//   l2_dist_up:   above every float64 distance that can round to a float32 <= dk: dk plus one float32 ulp of it (the 2^-22 of
//                 guard_eps is in MFMA units and does not cover that rounding when |q| >> A);
//   l2_bound_low: a lower bound of dist^2 of any row whose MFMA score is <= m;
//   guard_tau_l2: every row whose float32 distance could be <= dk has an MFMA score > tau.
// (host and device: tsim_l2_guard_host evaluates the same three functions for the CPU replay of the guard)
__host__ __device__ inline double l2_dist_up(float dk) { return (double)dk * (1.0 + 1.1921e-7) + 1e-44; }
__host__ __device__ inline double l2_bound_low(float m, float eps, double nqs, double qq) {
    const double b = ((double)m + (double)eps + 1e-13) * 2.0 * nqs;
    return qq - b - (qq + fabs(b)) * 1e-14;
}
// the real number guard_tau_l2 steps below; -inf when no finite threshold is safe
__host__ __device__ inline double l2_tau_lo(float dk, float eps, double nqs, double qq) {
    if (!(eps < 3.0e38f) || !(dk < 3.0e38f) || !(nqs > 0.0 && nqs < INFINITY) || !(qq < INFINITY)) return -INFINITY;
    const double up = l2_dist_up(dk);
    const double t = (qq - up - (qq + up) * 1e-14) / (2.0 * nqs);
    const double lo = t - (double)eps - 1e-13 - (fabs(t) + (double)eps) * 1e-15;
    return lo > -3.0e38 ? lo : -INFINITY;
}
__device__ __forceinline__ float guard_tau_l2(float dk, float eps, double nqs, double qq) {
    const double lo = l2_tau_lo(dk, eps, nqs, qq);
    if (!(lo > -3.0e38)) return -3.4028234e38f;
    return float_below((float)lo);   // (float)lo is within one float of lo: one step down is below it
}
__device__ __forceinline__ double l2_nqs(double qq, double A) { return sqrt(qq + A * A) * 2.0 * A; }   // nq' S
// |MFMA score - its exact counterpart| net of the float32 rounding of the distance (es = -dist^2 as stored): what the
// consistency checks compare with eps
__device__ __forceinline__ float l2_err(float ms, float es, double nqs, double qq) {
    const double inv = 0.5 / nqs;
    return (float)(fabs((double)ms - (qq + (double)es) * inv) + (double)es * 6.0e-8 * inv);
}

// The KL best entries of a query's partial lists by (MFMA score desc, index asc): lane t < KL returns the t-th
// (my_i = -1 when there are fewer).  ps / pi: the query's lists, nlists of KL entries each, sorted, padded with (-inf, -1).
// M = entries a LANE keeps (KL: all it could ever contribute).  The insertion network is the cost of this routine — the branch
// around it is taken whenever ANY lane has an entry to insert, i.e. nearly always: 8 VALU per position and entry, ~4 000 per
// query at KL = 16, and at Q = 4 096 the finalize kernel is VALU-throughput-bound on exactly that (45 us).  The KL winners are
// spread over 64 lanes, so a lane almost never contributes more than a few: with M = 4 the network is a quarter.  EXACTNESS is
// kept by a check, not by the odds: a lane's discarded entries all rank behind its M-th kept one, so they can only matter if the
// lane had all M of its kept entries popped by the merge; in that case (returned as false) the caller repeats with M = KL.
// (thr_update needs only a valid lower bound and never repeats.)
template <int KL, int LB = 4, int M = KL>
__device__ __forceinline__ bool select_kl_best(const float *__restrict__ ps, const int *__restrict__ pi, int P2, int lane,
                                               float &my_s_out, int &my_i_out) {
    // 1a. one pass: every lane keeps the M best of its E/64 entries in a sorted register list
    float ls[M];
    int li[M];
#pragma unroll
    for (int j = 0; j < M; ++j) {
        ls[j] = -INFINITY;
        li[j] = 0x7fffffff;
    }
    bool dropped = false;   // this lane let go of an entry (or of the rest of a list) that it might have contributed
    auto consider = [&](float s, int i) {
        if (i >= 0) {
            if (key_before(s, i, ls[M - 1], li[M - 1])) {
#pragma unroll
                for (int j = 0; j < M; ++j) {
                    const bool ahead = key_before(s, i, ls[j], li[j]);
                    const float ns = ahead ? ls[j] : s;
                    const int ni = ahead ? li[j] : i;
                    ls[j] = ahead ? s : ls[j];
                    li[j] = ahead ? i : li[j];
                    s = ns;
                    i = ni;
                }
                if (M < KL && i != 0x7fffffff) dropped = true;   // a kept entry fell off the end
            } else if (M < KL) {
                dropped = true;
            }
        }
    };
    // Lists are sorted and padded with (-inf, -1): a lane walks whole lists (list = lane, lane+64, ...).  With pre-pass
    // thresholds most lists hold 0-3 entries, so the first four entries (16 + 16 B) of FOUR lists are requested together —
    // one memory round trip per 256 lists instead of two per list (the walk was a chain of dependent loads: 16 round trips
    // at Q = 256, where P2 = 512) — and only a list that is full that far is walked on.  (Eight lists at a time cost 32 more
    // registers: 160 instead of <= 128, one wave per SIMD less, and the kernel — pure latency — ran 152 us instead of 80 at
    // Q = 4096; LB = 8 is the small-batch form, where occupancy is idle anyway.)
    for (int l0 = lane; l0 < P2; l0 += 64 * LB) {
        int4 iv[LB];
        float4 sv[LB];
#pragma unroll
        for (int u = 0; u < LB; ++u) {
            const int l = l0 + 64 * u;
            iv[u] = make_int4(-1, -1, -1, -1);
            sv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (l < P2) {
                iv[u] = *reinterpret_cast<const int4 *>(pi + (int64_t)l * KL);
                sv[u] = *reinterpret_cast<const float4 *>(ps + (int64_t)l * KL);
            }
        }
#pragma unroll
        for (int u = 0; u < LB; ++u) {
            if (iv[u].x < 0) continue;
            consider(sv[u].x, iv[u].x);
            consider(sv[u].y, iv[u].y);
            consider(sv[u].z, iv[u].z);
            consider(sv[u].w, iv[u].w);
            if (iv[u].w < 0) continue;
            // the list is sorted: once an entry does not beat this lane's last kept one, nothing behind it does — and every step
            // of the walk is a dependent memory round trip (full lists, as after phase A: 3 per list, 8 lists per lane in a row)
            if (!key_before(sv[u].w, iv[u].w, ls[M - 1], li[M - 1])) {
                if (M < KL) dropped = true;   // (the list may go on)
                continue;
            }
            const float *lsrc = ps + (int64_t)(l0 + 64 * u) * KL;
            const int *isrc = pi + (int64_t)(l0 + 64 * u) * KL;
#pragma unroll 1
            for (int j = 4; j < KL; j += 4) {
                const int4 jv = *reinterpret_cast<const int4 *>(isrc + j);
                if (jv.x < 0) break;
                const float4 tv = *reinterpret_cast<const float4 *>(lsrc + j);
                consider(tv.x, jv.x);
                consider(tv.y, jv.y);
                consider(tv.z, jv.z);
                consider(tv.w, jv.w);
                if (jv.w < 0) break;
                if (!key_before(tv.w, jv.w, ls[M - 1], li[M - 1])) {
                    if (M < KL) dropped = true;
                    break;
                }
            }
        }
    }

    // 1b. KL rounds of a 64-way merge of the list heads; the winning lane pops its head
    float my_s = -INFINITY;
    int my_i = -1;
    int npop = 0;
    for (int t = 0; t < KL; ++t) {
        float bs = ls[0];
        int bi = li[0];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float os = __shfl_xor(bs, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (key_before(os, oi, bs, bi)) {
                bs = os;
                bi = oi;
            }
        }
        if (bi == 0x7fffffff) break;  // fewer than KL valid entries (uniform)
        if (lane == t) {
            my_s = bs;
            my_i = bi;
        }
        if (li[0] == bi) {  // row ids are unique across partitions: exactly one lane owns the winner
#pragma unroll
            for (int j = 0; j + 1 < M; ++j) {
                ls[j] = ls[j + 1];
                li[j] = li[j + 1];
            }
            ls[M - 1] = -INFINITY;
            li[M - 1] = 0x7fffffff;
            ++npop;
        }
    }
    my_s_out = my_s;
    my_i_out = my_i;
    if constexpr (M < KL) return !__any(dropped && npop == M);
    return true;
}

// Two-phase main pass: after the list kernel has scored the first rows of the shard (phase A: lists p2_first .. +p2_count of
// every query), the KL-th best MFMA score found so far replaces the pre-pass bound in the query's shared threshold word.
// Phase B then streams the rest of the shard against a bound taken from 4x more rows than the pre-pass sample: its
// candidate events (the expensive, branchy side of the selection filter) fall accordingly.
template <int KL>
__global__ __launch_bounds__(256) void thr_update_kernel(const float *__restrict__ part_s, const int *__restrict__ part_i,
                                                         int P2_total, int p2_first, int p2_count, int64_t Q,
                                                         int *__restrict__ gthr) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= Q) return;
    float my_s;
    int my_i;
    // (lanes keep four entries: should one lane hold more than four of the KL best, the KL-th of what was kept is still the score
    // of a real row with KL - 1 others at or above it: a valid, slightly weaker bound)
    (void)select_kl_best<KL, 4, 4>(part_s + (q * P2_total + p2_first) * KL, part_i + (q * P2_total + p2_first) * KL, p2_count, lane, my_s,
                                   my_i);
    const float kth = __shfl(my_s, KL - 1, 64);
    const int kth_i = __shfl(my_i, KL - 1, 64);
    if (lane == 0 && kth_i >= 0) atomicMax(gthr + q, float_to_ordered(kth));   // KL rows score at least kth
}

// =====================================================================================================
// K2: cos_topk_finalize — one wave per query.
//   1. select the KL best of the P2*KL partial entries by (MFMA score desc, index asc);
//   2. re-score them exactly (above);
//   3. order by (exact score desc, index asc) and emit the first k;
//   4. GUARD: every row outside the KL candidates has an MFMA score <= cut = the KL-th selected one, hence an exact
//      score <= cut + eps when eps bounds |MFMA - exact| for the query.  eps is estimated from the candidates themselves
//      (c1 x the largest difference observed, never below `floor`).  If cut + eps < the k-th exact score nothing outside
//      can reach the list and the result stands; otherwise the query is FLAGGED: the widening pass (K1 in COLLECT mode)
//      gathers every row whose MFMA score exceeds (k-th exact score - eps) and widen_finalize re-scores all of them.
// =====================================================================================================
// NB: rows per exact re-score batch, LB: lists per walk round trip.  <4, 4>: 120 registers, four waves per SIMD (large Q: the
// kernel is latency-bound and lives on occupancy); <16 or 8, 8>: everything in flight at once for Q <= 1024, where at most one
// workgroup per CU exists anyway.
template <int KL, typename T, int SM, int NB, int LB>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NB > 4 ? 1 : KL == 16 ? 4 : 2))) void cos_topk_finalize_kernel(const float *__restrict__ part_s,
                                                                const int *__restrict__ part_i, int P2,
                                                                int64_t Q, int64_t N, const T *__restrict__ xq, int64_t ldq,
                                                                const T *__restrict__ xc, int64_t ldc, int d, int k,
                                                                const unit_t *__restrict__ uq, const int *__restrict__ gthr,
                                                                float *__restrict__ out_s,
                                                                int64_t *__restrict__ out_i,
                                                                int64_t idx_offset, GuardArgs g) {
    constexpr bool COS = SM == SM_COS, DOT = SM == SM_DOT, L2 = SM == SM_L2;
    static_assert(L2 == is_l2_rows<T>, "SM_L2 scores rows of l2_f32");
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= Q) return;
    const int64_t E = (int64_t)P2 * KL;
    const float *ps = part_s + q * E;
    const int *pi = part_i + q * E;

    float my_s;  // lane t < KL ends up holding the t-th selected candidate
    int my_i;
#if defined(TSIM_FIN_DIAG) && (TSIM_FIN_DIAG & 1)   // TIMING-ONLY (wrong results): no selection, the first list's entries
    my_s = lane < KL ? ps[lane] : -INFINITY;
    my_i = lane < KL ? pi[lane] : -1;
    if (my_i < 0 && lane < KL) { my_i = (int)((q * 977 + lane * 131) % N); my_s = 0.f; }
#else
    // (lanes keeping four entries + a repeat with all KL when the exactness check fails measured SLOWER here, 56-58 us against
    // 44-49: after the main pass the lists are short and the second instantiation costs more than the smaller network saves;
    // thr_update, whose lists are full, gains: 27 -> 16 us)
    (void)select_kl_best<KL, LB, KL>(ps, pi, P2, lane, my_s, my_i);
#endif
    const int nvalid = __popcll(__ballot(my_i >= 0));   // candidates sit in lanes 0 .. nvalid-1

    // 2. exact re-score: the wave works on one candidate at a time (coalesced row reads)
    ExactQuery<T> eqr;
    exact_load_query<T, COS>(eqr, xq + q * ldq, d, lane);   // (DOT, L2: the norm is taken in the guard, not held across the loop)
    float cs = -INFINITY;
#pragma unroll 1
    for (int t0 = 0; t0 < nvalid; t0 += NB) {   // NB candidates per step: their row reads overlap, their wave sums share shuffles
#if defined(TSIM_FIN_DIAG) && (TSIM_FIN_DIAG & 2)   // TIMING-ONLY (wrong results): no exact re-score
        const float sc = my_s;
#else
        const float sc = exact_score_batch<T, COS, NB>(eqr, xc, ldc, my_i, t0, nvalid, d, lane);
#endif
        if (lane >= t0 && lane < t0 + NB && lane < nvalid) cs = sc;
    }
    // 3. final order among the candidates: rank by counting
    int rank = 0;
    for (int t = 0; t < KL; ++t) {
        const float os = __shfl(cs, t, 64);
        const int oi = __shfl(my_i, t, 64);
        if (oi >= 0 && key_before(os, oi, cs, my_i)) rank++;
    }
    if (lane < KL && my_i >= 0 && rank < k) {
        out_s[q * k + rank] = cs;
        out_i[q * k + rank] = (int64_t)my_i + idx_offset;
    }
    if (lane >= nvalid && lane < k) {   // fewer valid candidates than k: pad
        out_s[q * k + lane] = -INFINITY;
        out_i[q * k + lane] = -1;
    }
    // 4. guard.  Rows that are not among the candidates: either they lost against the KL-th list entry (MFMA score <= it), or
    // the list kernel dropped them against the query's shared bound, whose final (largest) value is gthr[q] — also when the
    // bound came from a kernel that accumulates in another order (pre-pass in the 16x16x32 form, lists of 32 in the 32x32x16
    // form): cut = max of the two bounds whatever their origin.  Fewer than KL entries mean "every row was a candidate" only
    // if nothing was ever filtered (the bound word still holds its initial value).
    const int bkey = gthr ? gthr[q] : K1_GTHR_INIT;
    const bool filtered = bkey > K1_GTHR_INIT;
    bool safe = N <= KL || (nvalid < KL && !filtered);
    float tau = 0.f, eps = 0.f;
    double nqs = 1.0;
    (void)nqs;
    if (!safe) {
        const float err = wave_max(lane < nvalid ? fabsf(my_s - cs) : 0.f);
        if constexpr (COS) {
            eps = guard_eps(query_rho(eqr, uq + q * g.ld, d, lane), guard_rho_c(g), g.ld);
            // the bound must hold on the candidates too; if it does not, the unit rows are not the canonical images of the
            // float32 rows (or rho_c_max is stale): trust nothing, score the whole shard exactly
            if (!(err <= eps)) eps = INFINITY;
        } else if constexpr (DOT) {
            eqr.norm = exact_query_norm(eqr);   // nq = max(|q|, 1e-8): converts between the score domains
            eps = guard_eps(query_rho<true>(eqr, uq + q * g.ld, d, lane), *g.rho_c_max, g.ld);
            nqs = eqr.norm * dot_scale(*g.c_maxnorm);
            const double inv_nqs = 1.0 / nqs;   // (a consistency check, not the proof: one reciprocal, no per-lane division)
            const float derr = wave_max(lane < nvalid ? (float)fabs((double)my_s - (double)cs * inv_nqs) : 0.f);
            if (!(derr <= eps)) eps = INFINITY;   // (as for COS: the rows are not the images of the float32 rows)
        } else if constexpr (L2) {
            const double A = dot_scale(*g.c_maxnorm);
            eqr.norm = exact_query_sumsq(eqr);   // |q|^2
            const double nq = sqrt(eqr.norm + A * A);   // nq' of l2_query_rows_kernel, the same bits
            nqs = l2_nqs(eqr.norm, A);
            eps = guard_eps(query_rho_l2(eqr, uq + q * g.ld, d, A, nq, lane), *g.rho_c_max, g.ld);
            const float derr = wave_max(lane < nvalid ? l2_err(my_s, cs, nqs, eqr.norm) : 0.f);
            if (!(derr <= eps) || !(nqs < INFINITY) || !(eqr.norm < INFINITY)) eps = INFINITY;   // (non-finite: brute force)
        } else {
            eps = fmaxf(g.c1 * err, g.floor);
        }
        float cut = nvalid >= KL ? __shfl(my_s, KL - 1, 64) : -INFINITY;
        if (filtered) cut = fmaxf(cut, ordered_to_float(bkey));
        const unsigned long long kth = __ballot(lane < nvalid && rank == k - 1);   // at most one lane
        const float sk = kth ? __shfl(cs, __ffsll((long long)kth) - 1, 64) : -INFINITY;   // fewer than k candidates: no k-th score
        if constexpr (DOT) {
            safe = kth != 0 && dot_bound_up(cut, eps, nqs) < (double)sk;
            tau = guard_tau_dot(sk, eps, nqs);
        } else if constexpr (L2) {   // (sk = -(k-th distance); no k-th entry: +inf, everything is collected)
            safe = kth != 0 && l2_bound_low(cut, eps, nqs, eqr.norm) > l2_dist_up(-sk);
            tau = guard_tau_l2(-sk, eps, nqs, eqr.norm);
        } else {
            safe = kth != 0 && (double)cut + (double)eps < (double)sk;
            tau = guard_tau(sk, eps);   // rows at or below tau cannot reach sk
        }
    }
    if (lane == 0) {
        if (!safe) {
            const int slot = atomicAdd(g.ctl + CTL_NFLAG, 1);
            g.flag_q[slot] = (int)q;
            g.flag_thr[slot] = float_to_ordered(tau);
            g.flag_eps[slot] = eps;
        }
        if (g.status) g.status[q] = safe ? ST_PASS1 : ST_WIDENED;
    }
}

// k > 28: every query goes to the widening pass (or straight to the brute-force pass: all_brute).  gthr[q] = B, the k-th
// largest block maximum = a lower bound of the k-th best MFMA score: k rows score >= B on the MFMA, hence >= B - eps exactly,
// so the k-th best EXACT score is >= B - eps and every row of the exact top-k has an MFMA score >= B - 2 eps: that is the
// collection threshold.  One wave per query (COS, DOT: the query's rho comes from its two rows).  DOT: the argument holds with
// the exact scores taken in the MFMA domain (q.c / (nq S), a monotone map), so the threshold needs no conversion here.
// L2: the same in the domain (|q|^2 - dist^2) / (2 nqs), except that distances are ranked after their rounding to float32: a row
// of the top-k may lie one float32 ulp of a distance behind the k rows above B - eps, in MFMA units at most dist^2 2^-23 /
// (2 nqs) <= (nq' / A) 2^-24 (dist^2 <= 2 nq'^2): `margin` widens the band by that.  The threshold is a choice, not the proof:
// widen_finalize's guard decides with the threshold that was used.
template <int SM>
__global__ __launch_bounds__(256) void flag_all_kernel(int64_t Q, const int *__restrict__ gthr, bool all_brute,
                                                       const float *__restrict__ xq, int64_t ldq, const unit_t *__restrict__ uq,
                                                       int d, GuardArgs g) {
    constexpr bool COS = SM == SM_COS, DOT = SM == SM_DOT, L2 = SM == SM_L2;
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q == 0 && lane == 0) g.ctl[all_brute ? CTL_NUNRES : CTL_NFLAG] = (int)Q;
    if (q >= Q) return;
    float eps = g.floor;
    float margin = 0.f;
    (void)margin;
    if constexpr (L2) {
        if (!all_brute) {
            ExactQuery<float> eqr;
            exact_load_query<float, NORM_SQ>(eqr, xq + q * ldq, d, lane);
            const double A = dot_scale(*g.c_maxnorm), nq = sqrt(eqr.norm + A * A);
            eps = guard_eps(query_rho_l2(eqr, uq + q * g.ld, d, A, nq, lane), *g.rho_c_max, g.ld);
            margin = (float)(nq / A * 6.0e-8);
        }
    }
    if constexpr (COS || DOT) {
        if (!all_brute) {
            ExactQuery<float> eqr;
            exact_load_query<float, true>(eqr, xq + q * ldq, d, lane);
            eps = guard_eps(query_rho<DOT>(eqr, uq + q * g.ld, d, lane), guard_rho_c(g), g.ld);
        }
    }
    if (lane != 0) return;
    if (all_brute) {
        g.unres_q[q] = (int)q;
    } else {
        g.flag_q[q] = (int)q;
        const int key = gthr[q];
        if constexpr (L2) g.flag_thr[q] = key <= K1_GTHR_INIT ? key : float_to_ordered(guard_tau(ordered_to_float(key), 2.f * eps * 1.000001f + margin));
        else g.flag_thr[q] = key <= K1_GTHR_INIT ? key : float_to_ordered(guard_tau(ordered_to_float(key), 2.f * eps * 1.000001f));
        g.flag_eps[q] = eps;
    }
    if (g.status) g.status[q] = all_brute ? ST_BRUTE : ST_WIDENED;
}

// =====================================================================================================
// thr_select: gthr[q] = ordered-int form of the KL-th largest of the query's P2 block maxima (pre-pass output,
// [Q][P2] floats).  One wave per query; KL rounds of (lane-local max, wave max, owner removes one instance).
// =====================================================================================================
// VPL = values per lane >= P2 / 64.  (With the one 32-value form every round cost ~140 VALU instructions whatever P2 was — 20 us at
// any Q, and four waves per SIMD share the pipe; typical P2 is 512.)
// zero_base / zero_words: the call's control words and per-slot counters, cleared here instead of by a memset of their own when
// this kernel is the one in front of the main pass (one launch and its gap less per search).
template <int VPL>
__global__ __launch_bounds__(256) void thr_select_kernel(const float *__restrict__ bmax, int P2, int64_t Q, int KL,
                                                         int *__restrict__ gthr, int *__restrict__ zero_base, int zero_words) {
    for (int w = blockIdx.x * 256 + threadIdx.x; w < zero_words; w += gridDim.x * 256) zero_base[w] = 0;
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= Q) return;
    float v[VPL];
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int e = lane + 64 * i;
        v[i] = e < P2 ? bmax[q * P2 + e] : -INFINITY;
    }
    float best = -INFINITY;
    for (int t = 0; t < KL; ++t) {
        float lm = v[0];
#pragma unroll
        for (int i = 1; i < VPL; ++i) lm = fmaxf(lm, v[i]);
        best = wave_max(lm);
        const unsigned long long owners = __ballot(lm == best);
        if (lane == __ffsll((long long)owners) - 1) {   // one owner removes one instance
            bool done = false;
#pragma unroll
            for (int i = 0; i < VPL; ++i) {
                const bool hit = !done && v[i] == best;
                v[i] = hit ? -INFINITY : v[i];
                done = done || hit;
            }
        }
    }
    if (lane == 0) gthr[q] = best > -INFINITY ? float_to_ordered(best) : K1_GTHR_INIT;
}

static void launch_thr_select(const float *bmax, int P2, int64_t Q, int KL, int *gthr, hipStream_t st, int *zero_base = nullptr,
                              int zero_words = 0) {
    const dim3 grid((unsigned)((Q + 3) / 4));
    static_assert(K1_PREPASS_MAX_P2 == 2048, "dispatch below covers P2 <= 2048");
    if (P2 <= 512) hipLaunchKernelGGL(thr_select_kernel<8>, grid, dim3(256), 0, st, bmax, P2, Q, KL, gthr, zero_base, zero_words);
    else if (P2 <= 1024) hipLaunchKernelGGL(thr_select_kernel<16>, grid, dim3(256), 0, st, bmax, P2, Q, KL, gthr, zero_base, zero_words);
    else hipLaunchKernelGGL(thr_select_kernel<32>, grid, dim3(256), 0, st, bmax, P2, Q, KL, gthr, zero_base, zero_words);
}

// =====================================================================================================
// merge of sorted per-shard / per-chunk lists: [nlists, Q, k_in] -> [Q, k_out]; one wave per query.
// =====================================================================================================
__global__ __launch_bounds__(256) void topk_merge_kernel(const float *__restrict__ scores,
                                                         const int64_t *__restrict__ idx, int nlists,
                                                         int64_t Q, int k_in, int k_out,
                                                         int64_t lstride_s, int64_t lstride_i,
                                                         float *__restrict__ out_s,
                                                         int64_t *__restrict__ out_i) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= Q) return;
    const int E = nlists * k_in;
    float last_s = INFINITY;
    int64_t last_i = -1;
    for (int t = 0; t < k_out; ++t) {
        float bs = -INFINITY;
        int64_t bi = INT64_MAX;
        for (int e = lane; e < E; e += 64) {
            const int l = e / k_in, j = e % k_in;
            const int64_t off = q * k_in + j;
            const float s = scores[(int64_t)l * lstride_s + off];
            const int64_t i = idx[(int64_t)l * lstride_i + off];
            if (i >= 0 && key_before(last_s, last_i, s, i) && key_before(s, i, bs, bi)) {
                bs = s;
                bi = i;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float os = __shfl_xor(bs, o, 64);
            const int64_t oi = __shfl_xor(bi, o, 64);
            if (key_before(os, oi, bs, bi)) {
                bs = os;
                bi = oi;
            }
        }
        const bool none = bi == INT64_MAX;
        if (lane == 0) {
            out_s[q * k_out + t] = none ? -INFINITY : bs;
            out_i[q * k_out + t] = none ? -1 : bi;
        }
        if (!none) {
            last_s = bs;
            last_i = bi;
        } else {
            last_s = -INFINITY;
            last_i = INT64_MAX;  // nothing ranks after this: remaining slots pad
        }
    }
}

// =====================================================================================================
// Sorted lists in LDS (sl_*): what the widening pass and the brute-force pass (every k, 1 .. 1 024) and tsim_topk_merge_strided
// with k_out > 64 keep their entries in.  Lists are sorted by (score desc, index asc), new entries are sorted with a bitonic
// network and merged in by rank (each entry's place in the other list by binary search), never selected one round at a time.
// Padding is (-inf, PAD): it ranks behind every real entry, a real entry with score -inf included; NaN scores become padding
// (the list kernels never select them either).
//
// The running list (SlList, one per workgroup of 256 threads) holds the best kp >= k entries seen so far, kp a power of two
// (sl_list_len).  Its protocol, per query: reset; then for every block of at most SL_NB candidate entries: every thread reads
// bound(k), the list's k-th entry, BEFORE anyone offers (the list does not change until flush); offer() appends the entries
// that rank before the bound to the block through an LDS counter; flush() reads the count BEHIND a barrier (so n > 0 is
// workgroup-uniform), sorts the block and merges it in, and resets the counter BEHIND the absorb, then a barrier.  After the
// last flush the first k entries are the exact top-k; store_raw / sl_store_result write them, and the kernel puts a barrier
// before the next query's reset.
// =====================================================================================================
constexpr int SL_MAX_K = 1024;   // TSIM_TOPK_MAX_K
constexpr int SL_NB = 1024;      // entries of one block merged into a running list

// length of the running list for k entries: the smallest power of two >= max(k, 64)
static inline int sl_list_len(int k) {
    int kp = 64;
    while (kp < k) kp <<= 1;
    return kp;
}

template <typename I>
__device__ __forceinline__ I sl_pad();
template <>
__device__ __forceinline__ int sl_pad<int>() { return 0x7fffffff; }
template <>
__device__ __forceinline__ int64_t sl_pad<int64_t>() { return INT64_MAX; }

// sort s/ix[0..n) by (score desc, index asc); n a power of two; a 256-thread workgroup; entries written before the call
// must be behind a barrier, and the sorted list is behind one on return
template <typename I>
__device__ __forceinline__ void sl_sort(float *s, I *ix, int n) {
    for (int size = 2; size <= n; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < n / 2; t += 256) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const float si = s[i], sj = s[j];
                const I ii = ix[i], ij = ix[j];
                if ((i & size) == 0 ? key_before(sj, ij, si, ii) : key_before(si, ii, sj, ij)) {
                    s[i] = sj;
                    s[j] = si;
                    ix[i] = ij;
                    ix[j] = ii;
                }
            }
            __syncthreads();
        }
}

// number of entries of the sorted list a[0..n) that rank before (s, i) (LE: before it or equal to it)
template <typename I, bool LE>
__device__ __forceinline__ int sl_count(const float *as, const I *ai, int n, float s, I i) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const bool p = LE ? !key_before(s, i, as[mid], ai[mid]) : key_before(as[mid], ai[mid], s, i);
        lo = p ? mid + 1 : lo;
        hi = p ? hi : mid;
    }
    return lo;
}

// Merge the sorted block b[0..nb) into the sorted list t[0..kp): afterwards t holds the first kp of both.  kp + nb <= 2048.
// Ranks: t's entry i lands at i + (block entries before it), the block's entry j at j + (list entries before or equal to
// it) — a permutation of 0 .. kp+nb-1 even where entries are equal.
// DEDUP (tsim_topk_merge): an entry equal in (score, index) to the one before it in the merged order is dropped, and the
// list is refilled with padding behind the survivors.  m_s / m_i: kp + nb entries of scratch; wsum: 4 ints.
template <typename I, bool DEDUP>
__device__ __forceinline__ void sl_merge(float *ts, I *ti, int kp, const float *bs, const I *bi, int nb, float *m_s, I *m_i,
                                         int *wsum) {
    constexpr int R = 2048 / 256;
    float vs[R] = {};
    I vi[R] = {};
    int rk[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int t = threadIdx.x + 256 * r;
        rk[r] = 0x7fffffff;
        if (t < kp) {
            vs[r] = ts[t];
            vi[r] = ti[t];
            rk[r] = t + sl_count<I, false>(bs, bi, nb, vs[r], vi[r]);
        } else if (t < kp + nb) {
            vs[r] = bs[t - kp];
            vi[r] = bi[t - kp];
            if (vi[r] != sl_pad<I>()) rk[r] = t - kp + sl_count<I, true>(ts, ti, kp, vs[r], vi[r]);   // (padding: rank >= kp)
        }
    }
    __syncthreads();
    if constexpr (!DEDUP) {
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (rk[r] < kp) {
                ts[rk[r]] = vs[r];
                ti[rk[r]] = vi[r];
            }
        __syncthreads();
    } else {
        const int n = kp + nb;
        for (int t = threadIdx.x; t < n; t += 256) {   // block padding never got a rank: it is all alike
            m_s[t] = -INFINITY;
            m_i[t] = sl_pad<I>();
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (rk[r] < n) {
                m_s[rk[r]] = vs[r];
                m_i[rk[r]] = vi[r];
            }
        __syncthreads();
        // survivors: real entries not equal to their predecessor; thread t owns positions 8t .. 8t+7
        constexpr int PER = 2048 / 256;
        int keep = 0;
#pragma unroll
        for (int e = 0; e < PER; ++e) {
            const int p = threadIdx.x * PER + e;
            keep |= (p < n && m_i[p] != sl_pad<I>() && !(p > 0 && m_s[p] == m_s[p - 1] && m_i[p] == m_i[p - 1])) << e;
        }
        const int mine = __popc(keep);
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        int x = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(x, o, 64);
            if (lane >= o) x += y;
        }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        int base = x - mine, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            base += w < wave ? wsum[w] : 0;
            total += wsum[w];
        }
#pragma unroll
        for (int e = 0; e < PER; ++e) {
            if ((keep >> e) & 1) {
                const int p = threadIdx.x * PER + e;
                if (base < kp) {
                    ts[base] = m_s[p];
                    ti[base] = m_i[p];
                }
                ++base;
            }
        }
        for (int t = total + threadIdx.x; t < kp; t += 256) {
            ts[t] = -INFINITY;
            ti[t] = sl_pad<I>();
        }
        __syncthreads();
    }
}

// The first k entries of a sorted list as the caller sees them: padding becomes (-inf, -1), a row gets idx_offset; NEG (the
// Euclidean space, whose lists hold -dist^2) negates the scores, padding +inf.
template <bool NEG, typename I>
__device__ __forceinline__ void sl_store_result(const float *s, const I *ix, int k, float *out_s, int64_t *out_i, int64_t at,
                                                int64_t idx_offset) {
    for (int t = threadIdx.x; t < k; t += 256) {
        const I row = ix[t];
        const bool pad = row == sl_pad<I>();
        out_s[at + t] = pad ? (NEG ? INFINITY : -INFINITY) : NEG ? -s[t] : s[t];
        out_i[at + t] = pad ? -1 : (int64_t)row + idx_offset;
    }
}

template <typename I>
struct SlBound {   // the list's k-th entry
    float s;
    I i;
};
// The running list (protocol: the block comment above): a handle on the LDS arrays that sl_shared_list declares.  The arrays
// are separate __shared__ variables: as members of one __shared__ struct the same code measured up to 1.9 % slower (DESIGN.md,
// "One running-list type").
template <typename I, bool DEDUP>
struct SlList {
    float *top_s, *blk_s, *m_s;   // m_s, m_i, wsum: sl_merge's scratch, null unless DEDUP
    I *top_i, *blk_i, *m_i;
    int *nb, *wsum;               // nb: entries offered to the block since the last flush

    __device__ __forceinline__ void reset(int kp) {
        for (int t = threadIdx.x; t < kp; t += 256) {
            top_s[t] = -INFINITY;
            top_i[t] = sl_pad<I>();
        }
        if (threadIdx.x == 0) *nb = 0;
        __syncthreads();
    }
    __device__ __forceinline__ SlBound<I> bound(int k) const { return {top_s[k - 1], top_i[k - 1]}; }
    // append (s, i) to the block when it ranks before the bound; NaN is dropped
    __device__ __forceinline__ void offer(float s, I i, SlBound<I> w) {
        if (s == s && key_before(s, i, w.s, w.i)) {
            const int p = atomicAdd(nb, 1);
            blk_s[p] = s;
            blk_i[p] = i;
        }
    }
    // sort the block (padded to a power of two) and merge it into the list
    __device__ __forceinline__ void flush(int kp) {
        __syncthreads();
        const int n = *nb;
        if (n > 0) {   // workgroup-uniform
            int np = 1;
            while (np < n) np <<= 1;
            for (int t = n + threadIdx.x; t < np; t += 256) {
                blk_s[t] = -INFINITY;
                blk_i[t] = sl_pad<I>();
            }
            __syncthreads();
            sl_sort(blk_s, blk_i, np);
            sl_merge<I, DEDUP>(top_s, top_i, kp, blk_s, blk_i, np, m_s, m_i, wsum);
        }
        if (threadIdx.x == 0) *nb = 0;
        __syncthreads();
    }
    // the first k entries as they are, padding included (a chunk list)
    __device__ __forceinline__ void store_raw(float *dst_s, I *dst_i, int64_t at, int k) const {
        for (int t = threadIdx.x; t < k; t += 256) {
            dst_s[at + t] = top_s[t];
            dst_i[at + t] = top_i[t];
        }
    }
    template <bool NEG>
    __device__ __forceinline__ void store_result(float *out_s, int64_t *out_i, int64_t at, int k, int64_t idx_offset) const {
        sl_store_result<NEG>(top_s, top_i, k, out_s, out_i, at, idx_offset);
    }
};
// The workgroup's list: one set of arrays per (I, DEDUP), 16 388 B, with the scratch of DEDUP 49 172 B.
template <typename I, bool DEDUP>
__device__ __forceinline__ SlList<I, DEDUP> sl_shared_list() {
    __shared__ float top_s[SL_MAX_K], blk_s[SL_NB];
    __shared__ I top_i[SL_MAX_K], blk_i[SL_NB];
    __shared__ int nb;
    if constexpr (DEDUP) {
        __shared__ float m_s[SL_MAX_K + SL_NB];
        __shared__ I m_i[SL_MAX_K + SL_NB];
        __shared__ int wsum[4];
        return {top_s, blk_s, m_s, top_i, blk_i, m_i, &nb, wsum};
    }
    return {top_s, blk_s, nullptr, top_i, blk_i, nullptr, &nb, nullptr};
}

// Exact scores of the rows held by lanes 0 .. nvalid-1 (my_i), eight at a time (exact_score_batch: the bits of exact_score).
template <typename T, bool COS, typename C = T>
__device__ __forceinline__ float wave_scores(const ExactQuery<T> &q, const C *xc, int64_t ldc, int my_i, int nvalid, int d,
                                             int lane) {
    constexpr int NB = 8;
    float mine = 0.f;
    for (int t0 = 0; t0 < nvalid; t0 += NB) {
        const float s = exact_score_batch<T, COS, NB, C>(q, xc, ldc, my_i, t0, nvalid, d, lane);
        if (lane >= t0 && lane < t0 + NB) mine = s;
    }
    return mine;
}

// =====================================================================================================
// widen_finalize: one workgroup per FLAGGED query (slot).  Re-scores every entry the widening pass collected for it (every
// row whose MFMA score exceeded the slot's threshold; at most cap, a power of two >= 4k), sorts the entries in LDS, writes the
// first k and repeats the guard with the threshold that was actually used and the errors seen on this larger sample.  An
// overflowed buffer or a failed guard hands the query to the brute-force pass.  Dynamic LDS: cap floats + cap ints.
// =====================================================================================================
template <typename T, int SM>
__global__ __launch_bounds__(256) void widen_finalize_kernel(const unsigned long long *__restrict__ coll_buf,
                                                             const int *__restrict__ coll_cnt, int cap, int64_t Q,
                                                             const T *__restrict__ xq, int64_t ldq,
                                                             const T *__restrict__ xc, int64_t ldc, int d, int k,
                                                             float *__restrict__ out_s, int64_t *__restrict__ out_i,
                                                             int64_t idx_offset, GuardArgs g) {
    constexpr bool COS = SM == SM_COS, DOT = SM == SM_DOT, L2 = SM == SM_L2;
    static_assert(L2 == is_l2_rows<T>, "SM_L2 scores rows of l2_f32");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *sc = reinterpret_cast<float *>(smem);
    int *ix = reinterpret_cast<int *>(sc + cap);
    __shared__ float s_err[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int nflag = g.ctl[CTL_NFLAG];
    nflag = nflag < Q ? nflag : (int)Q;
    for (int slot = blockIdx.x; slot < nflag; slot += gridDim.x) {
        const int q = g.flag_q[slot];
        const int n = coll_cnt[slot];
        bool resolved = n <= cap;
        if (resolved) {   // workgroup-uniform
            int np = 64;
            while (np < n || np < k) np <<= 1;   // <= cap (a power of two >= 4k)
            ExactQuery<T> eqr;
            exact_load_query<T, L2 ? NORM_SQ : COS || DOT>(eqr, xq + (int64_t)q * ldq, d, lane);
            double nqs = 1.0;
            if constexpr (DOT) nqs = eqr.norm * dot_scale(*g.c_maxnorm);
            if constexpr (L2) nqs = l2_nqs(eqr.norm, dot_scale(*g.c_maxnorm));
            float err = 0.f;
            for (int g0 = wave * 64; g0 < np; g0 += 256) {   // wave-uniform
                const int e = g0 + lane;
                float s = -INFINITY;
                int row = sl_pad<int>();
                if (g0 < n) {
                    const unsigned long long ent = coll_buf[(int64_t)slot * cap + (e < n ? e : g0)];
                    const int my_row = (int)(ent >> 32);
                    const int nvalid = n - g0 < 64 ? n - g0 : 64;
                    const float es = wave_scores<T, COS>(eqr, xc, ldc, my_row, nvalid, d, lane);
                    if (e < n) {
                        const float ms = __uint_as_float((uint32_t)ent);
                        if constexpr (DOT) err = fmaxf(err, (float)fabs((double)ms - (double)es / nqs));
                        else if constexpr (L2) err = fmaxf(err, l2_err(ms, es, nqs, eqr.norm));
                        else err = fmaxf(err, fabsf(ms - es));
                        if (es == es) {
                            s = es;
                            row = my_row;
                        }
                    }
                }
                sc[e] = s;
                ix[e] = row;
            }
            err = wave_max(err);
            if (lane == 0) s_err[wave] = err;
            __syncthreads();
            sl_sort(sc, ix, np);
            sl_store_result<false>(sc, ix, k, out_s, out_i, (int64_t)q * k, idx_offset);
            // guard again with the threshold the collection used: every row that was NOT collected has an MFMA score below
            // it, hence an exact score below thr + eps.  COS: eps is the query's bound from the first pass (and it must hold on
            // everything that was re-scored here, else the inputs are inconsistent -> brute force); unit rows only: the largest
            // difference seen on this larger sample with half the safety factor of the first pass (not below 1).
            const float errmax = fmaxf(fmaxf(s_err[0], s_err[1]), fmaxf(s_err[2], s_err[3]));
            float eps;
            if constexpr (COS || DOT || L2) {
                eps = g.flag_eps[slot];
                if (!(errmax <= eps)) eps = INFINITY;
            } else {
                eps = fmaxf(fmaxf(0.5f * g.c1, 1.f) * errmax, g.floor);
            }
            const float thr = ordered_to_float(g.flag_thr[slot]);
            const float sk = ix[k - 1] == sl_pad<int>() ? -INFINITY : sc[k - 1];
            if constexpr (DOT) resolved = n >= k && dot_bound_up(thr, eps, nqs) < (double)sk;
            else if constexpr (L2) resolved = n >= k && l2_bound_low(thr, eps, nqs, eqr.norm) > l2_dist_up(-sk);
            else resolved = n >= k && (double)thr + (double)eps < (double)sk;
        }
        if (threadIdx.x == 0) {
            if (!resolved) g.unres_q[atomicAdd(g.ctl + CTL_NUNRES, 1)] = q;
            if (g.status) g.status[q] = resolved ? ST_WIDENED : ST_BRUTE;
        }
        __syncthreads();
    }
}

// =====================================================================================================
// Brute-force exact pass for the queries nothing else resolved: every row of the shard is scored exactly.
//   bf_partial: workgroup (chunk c, slot u) passes the chunk's rows in blocks of SL_NB through a running list and writes its
//               first k entries, padding included.
//   bf_merge:   one workgroup per slot passes the chunk lists through a running list, one per block, and writes the result.
// HBM-bound (N*d*4 bytes per query); last resort for every k, and the serving path for k > 28 on small shards.
// =====================================================================================================
template <typename T, bool COS>
__global__ __launch_bounds__(256) void bf_partial_kernel(int64_t Q, int64_t N, int rows_per_chunk,
                                                         const T *__restrict__ xq, int64_t ldq,
                                                         const T *__restrict__ xc, int64_t ldc, int d, int k, int kp,
                                                         float *__restrict__ bf_s, int *__restrict__ bf_i, GuardArgs g) {
    SlList<int, false> top = sl_shared_list<int, false>();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nch = gridDim.x, chunk = blockIdx.x;
    int nu = g.ctl[CTL_NUNRES];
    nu = nu < Q ? nu : (int)Q;
    const int64_t r0 = (int64_t)chunk * rows_per_chunk;
    const int64_t r1 = r0 + rows_per_chunk < N ? r0 + rows_per_chunk : N;
    for (int u = blockIdx.y; u < nu; u += gridDim.y) {
        const int q = g.unres_q[u];
        ExactQuery<T> eqr;
        exact_load_query<T, COS>(eqr, xq + (int64_t)q * ldq, d, lane);
        top.reset(kp);
        for (int64_t b = r0; b < r1; b += SL_NB) {
            const int nb = (int)(r1 - b < SL_NB ? r1 - b : SL_NB);
            const SlBound<int> w = top.bound(k);
            for (int g0 = wave * 64; g0 < nb; g0 += 256) {   // wave-uniform
                const int e = g0 + lane;
                const int nvalid = nb - g0 < 64 ? nb - g0 : 64;
                const int row = (int)(b + (e < nb ? e : g0));
                const float s = wave_scores<T, COS>(eqr, xc, ldc, row, nvalid, d, lane);
                if (e < nb) top.offer(s, row, w);
            }
            top.flush(kp);
        }
        top.store_raw(bf_s, bf_i, ((int64_t)u * nch + chunk) * k, k);
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void bf_merge_kernel(int64_t Q, int nch, int k, int kp, const float *__restrict__ bf_s,
                                                       const int *__restrict__ bf_i, float *__restrict__ out_s,
                                                       int64_t *__restrict__ out_i, int64_t idx_offset, GuardArgs g) {
    SlList<int, false> top = sl_shared_list<int, false>();
    int nu = g.ctl[CTL_NUNRES];
    nu = nu < Q ? nu : (int)Q;
    for (int u = blockIdx.x; u < nu; u += gridDim.x) {
        const int q = g.unres_q[u];
        top.reset(kp);
        for (int c = 0; c < nch; ++c) {
            const SlBound<int> w = top.bound(k);
            for (int t = threadIdx.x; t < k; t += 256) {
                const int64_t at = ((int64_t)u * nch + c) * k + t;
                top.offer(bf_s[at], bf_i[at], w);
            }
            top.flush(kp);
        }
        top.store_result<false>(out_s, out_i, (int64_t)q * k, k, idx_offset);
        if (threadIdx.x == 0 && g.status) g.status[q] = ST_BRUTE;
        __syncthreads();
    }
}

// topk_merge for 64 < k_out <= 1024: one workgroup per query; the nlists * k_in entries pass in blocks of SL_NB through a
// running list that drops duplicates of (score, index).  Same output as topk_merge_kernel.
__global__ __launch_bounds__(256) void topk_merge_large_kernel(const float *__restrict__ scores, const int64_t *__restrict__ idx,
                                                               int nlists, int64_t Q, int k_in, int k_out, int kp,
                                                               int64_t lstride_s, int64_t lstride_i, float *__restrict__ out_s,
                                                               int64_t *__restrict__ out_i) {
    SlList<int64_t, true> top = sl_shared_list<int64_t, true>();
    const int64_t E = (int64_t)nlists * k_in;
    for (int64_t q = blockIdx.x; q < Q; q += gridDim.x) {
        top.reset(kp);
        for (int64_t e0 = 0; e0 < E; e0 += SL_NB) {
            const SlBound<int64_t> w = top.bound(k_out);
            for (int64_t e = e0 + threadIdx.x; e < E && e < e0 + SL_NB; e += 256) {
                const int l = (int)(e / k_in), j = (int)(e % k_in);
                const int64_t off = q * k_in + j;
                const int64_t i = idx[(int64_t)l * lstride_i + off];
                if (i >= 0) top.offer(scores[(int64_t)l * lstride_s + off], i, w);
            }
            top.flush(kp);
        }
        top.store_result<false>(out_s, out_i, q * k_out, k_out, 0);
        __syncthreads();
    }
}

// =====================================================================================================
// dense cos_sim (A8): float32, rows normalised by division exactly like the reference, 64x64 tiles.
// Evaluation-sized inputs only; not on the search path.
// =====================================================================================================
__global__ __launch_bounds__(256) void cos_sim_kernel(const float *__restrict__ a, int64_t na,
                                                      const float *__restrict__ b, int64_t nb, int d,
                                                      float *__restrict__ out) {
    __shared__ float sa[16][65], sb[16][65];
    __shared__ float norm_a[64], norm_b[64];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int64_t i0 = (int64_t)blockIdx.y * 64, j0 = (int64_t)blockIdx.x * 64;
    // row norms of this tile's 64 + 64 rows: 4 threads per row
    {
        const int rr = threadIdx.x >> 2, part = threadIdx.x & 3;
        float s1 = 0.f, s2 = 0.f;
        if (i0 + rr < na)
            for (int kk = part; kk < d; kk += 4) { float v = a[(i0 + rr) * d + kk]; s1 = fmaf(v, v, s1); }
        if (j0 + rr < nb)
            for (int kk = part; kk < d; kk += 4) { float v = b[(j0 + rr) * d + kk]; s2 = fmaf(v, v, s2); }
        s1 += __shfl_xor(s1, 1, 64); s1 += __shfl_xor(s1, 2, 64);
        s2 += __shfl_xor(s2, 1, 64); s2 += __shfl_xor(s2, 2, 64);
        if (part == 0) { norm_a[rr] = sqrtf(s1); norm_b[rr] = sqrtf(s2); }
    }
    __syncthreads();
    float acc[4][4] = {};
    for (int k0 = 0; k0 < d; k0 += 16) {
        for (int e = threadIdx.x; e < 64 * 16; e += 256) {
            const int rr = e >> 4, kk = e & 15;
            float va = 0.f, vb = 0.f;
            if (k0 + kk < d) {
                if (i0 + rr < na) va = a[(i0 + rr) * d + k0 + kk] / norm_a[rr];
                if (j0 + rr < nb) vb = b[(j0 + rr) * d + k0 + kk] / norm_b[rr];
            }
            sa[kk][rr] = va;
            sb[kk][rr] = vb;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            float av[4], bv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { av[u] = sa[kk][ty * 4 + u]; bv[u] = sb[kk][tx * 4 + u]; }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[u][v] = fmaf(av[u], bv[v], acc[u][v]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int64_t i = i0 + ty * 4 + u, j = j0 + tx * 4 + v;
            if (i < na && j < nb) out[i * nb + j] = acc[u][v];
        }
}

// =====================================================================================================
// masked mean-pool on a padded [B,S,H] tensor (A4).  One thread per (b, h); HBM-bound.
// MODE (TSIM_POOL_*, tsim_pool): MEAN is the A4 kernel unchanged; MEAN_SQRT_LEN divides the same sum by sqrt(max(sum of the
// mask, 1e-9)); CLS takes the first token whose mask entry is non-zero (the packed layout's first token), MAX the elementwise
// max over those tokens.  No token: a zero row, as the packed forward gives.
// =====================================================================================================
template <typename T, int MODE = TSIM_POOL_MEAN>
__global__ __launch_bounds__(256) void mean_pool_kernel(const T *__restrict__ hidden,
                                                        const int32_t *__restrict__ mask, int S, int H,
                                                        float *__restrict__ out) {
    const int64_t bidx = blockIdx.y;
    const int hh = blockIdx.x * 256 + threadIdx.x;
    if (hh >= H) return;
    const T *hp = hidden + bidx * S * (int64_t)H + hh;
    const int32_t *mp = mask + bidx * S;
    if constexpr (MODE == TSIM_POOL_CLS || MODE == TSIM_POOL_MAX) {
        float v = MODE == TSIM_POOL_MAX ? -INFINITY : 0.f;
        bool any = false;
        for (int s = 0; s < S; ++s) {
            if (mp[s] == 0) continue;
            const float x = load_as_f32<T>(hp + (int64_t)s * H);
            if (MODE == TSIM_POOL_CLS) {
                v = x;
                any = true;
                break;
            }
            v = fmaxf(v, x);
            any = true;
        }
        out[bidx * H + hh] = any ? v : 0.f;
        return;
    }
    float sum = 0.f, msum = 0.f;
    for (int s = 0; s < S; ++s) {
        const float m = (float)mp[s];
        sum = fmaf(load_as_f32<T>(hp + (int64_t)s * H), m, sum);
        msum += m;
    }
    out[bidx * H + hh] = sum / (MODE == TSIM_POOL_MEAN_SQRT_LEN ? sqrtf(fmaxf(msum, 1e-9f)) : fmaxf(msum, 1e-9f));
}

// =====================================================================================================
// host side
// =====================================================================================================
static inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

}  // namespace tsim

using namespace tsim;

extern "C" int tsim_pad_dim(int d) {
    const int sizes[] = {128, 256, 384, 512, 768};
    for (int s : sizes)
        if (d <= s) return s;
    return 0;
}

extern "C" int tsim_l2norm_rows(const void *x, int x_dtype, int64_t rows, int d, int64_t ld_in, void *out_f16,
                                int ld_out, float eps, float *rho_max, void *stream) {
    TSIM_REQUIRE(x && out_f16, "l2norm_rows: null pointer");
    TSIM_REQUIRE(rows >= 0 && d > 0 && ld_in >= d && ld_out >= d, "l2norm_rows: bad shape rows=%lld d=%d ld_in=%lld ld_out=%d",
                 (long long)rows, d, (long long)ld_in, ld_out);
    if (rows == 0) return TSIM_OK;
    const unsigned grid = (unsigned)((rows + 3) / 4);
    if (x_dtype == TSIM_F32)
        hipLaunchKernelGGL(l2norm_rows_kernel<float>, dim3(grid), dim3(256), 0, as_stream(stream),
                           (const float *)x, rows, d, ld_in, (unit_t *)out_f16, ld_out, eps, rho_max);
    else if (x_dtype == TSIM_BF16)
        hipLaunchKernelGGL(l2norm_rows_kernel<bf16_t>, dim3(grid), dim3(256), 0, as_stream(stream),
                           (const bf16_t *)x, rows, d, ld_in, (unit_t *)out_f16, ld_out, eps, rho_max);
    else
        return fail(TSIM_EINVAL, "l2norm_rows: unknown dtype %d", x_dtype);
    TSIM_HIP_CHECK(hipGetLastError());
    return TSIM_OK;
}

template <typename F>
static int dot_prep_launch(const char *what, const void *x, int x_dtype, int64_t rows, int d, int64_t ld_in, F launch) {
    TSIM_REQUIRE(rows >= 0 && d > 0 && ld_in >= d, "%s: bad shape rows=%lld d=%d ld_in=%lld", what, (long long)rows, d,
                 (long long)ld_in);
    if (rows == 0) return TSIM_OK;
    const dim3 grid((unsigned)((rows + 3) / 4));
    if (x_dtype == TSIM_F32) launch(grid, (const float *)x);
    else if (x_dtype == TSIM_BF16) launch(grid, (const bf16_t *)x);
    else return fail(TSIM_EINVAL, "%s: unknown dtype %d", what, x_dtype);
    TSIM_HIP_CHECK(hipGetLastError());
    return TSIM_OK;
}

extern "C" int tsim_max_norm_rows(const void *x, int x_dtype, int64_t rows, int d, int64_t ld_in, float *maxnorm, void *stream) {
    TSIM_REQUIRE(x && maxnorm, "max_norm_rows: null pointer");
    return dot_prep_launch("max_norm_rows", x, x_dtype, rows, d, ld_in, [&](dim3 grid, auto xt) {
        using T = std::remove_const_t<std::remove_pointer_t<decltype(xt)>>;
        hipLaunchKernelGGL(max_norm_rows_kernel<T>, grid, dim3(256), 0, as_stream(stream), xt, rows, d, ld_in, maxnorm);
    });
}

extern "C" int tsim_dot_scaled_rows(const void *x, int x_dtype, int64_t rows, int d, int64_t ld_in, const float *maxnorm,
                                    void *out_f16, int ld_out, float *rho_max, void *stream) {
    TSIM_REQUIRE(x && maxnorm && out_f16, "dot_scaled_rows: null pointer");
    TSIM_REQUIRE(ld_out >= d, "dot_scaled_rows: ld_out=%d < d=%d", ld_out, d);
    return dot_prep_launch("dot_scaled_rows", x, x_dtype, rows, d, ld_in, [&](dim3 grid, auto xt) {
        using T = std::remove_const_t<std::remove_pointer_t<decltype(xt)>>;
        hipLaunchKernelGGL(dot_scaled_rows_kernel<T>, grid, dim3(256), 0, as_stream(stream), xt, rows, d, ld_in, maxnorm,
                           (unit_t *)out_f16, ld_out, rho_max);
    });
}

extern "C" double tsim_dot_scale(float maxnorm) { return dot_scale(maxnorm); }

extern "C" int tsim_l2_rows(const void *x, int x_dtype, int64_t rows, int d, int64_t ld_in, const float *maxnorm, void *out_f16,
                            int ld_out, float *rho_max, void *stream) {
    TSIM_REQUIRE(x && maxnorm && out_f16, "l2_rows: null pointer");
    TSIM_REQUIRE(ld_out >= d + 1, "l2_rows: ld_out=%d < d+1=%d", ld_out, d + 1);
    return dot_prep_launch("l2_rows", x, x_dtype, rows, d, ld_in, [&](dim3 grid, auto xt) {
        using T = std::remove_const_t<std::remove_pointer_t<decltype(xt)>>;
        hipLaunchKernelGGL(l2_rows_kernel<T>, grid, dim3(256), 0, as_stream(stream), xt, rows, d, ld_in, maxnorm,
                           (unit_t *)out_f16, ld_out, rho_max);
    });
}

extern "C" int tsim_l2_query_rows(const void *x, int x_dtype, int64_t rows, int d, int64_t ld_in, const float *maxnorm,
                                  void *out_f16, int ld_out, void *stream) {
    TSIM_REQUIRE(x && maxnorm && out_f16, "l2_query_rows: null pointer");
    TSIM_REQUIRE(ld_out >= d + 1, "l2_query_rows: ld_out=%d < d+1=%d", ld_out, d + 1);
    return dot_prep_launch("l2_query_rows", x, x_dtype, rows, d, ld_in, [&](dim3 grid, auto xt) {
        using T = std::remove_const_t<std::remove_pointer_t<decltype(xt)>>;
        hipLaunchKernelGGL(l2_query_rows_kernel<T>, grid, dim3(256), 0, as_stream(stream), xt, rows, d, ld_in, maxnorm,
                           (unit_t *)out_f16, ld_out);
    });
}

static thread_local hipEvent_t g_ev_start = nullptr, g_ev_stop = nullptr;

extern "C" void tsim_time_next_topk(void *start_event, void *stop_event) {
    g_ev_start = reinterpret_cast<hipEvent_t>(start_event);
    g_ev_stop = reinterpret_cast<hipEvent_t>(stop_event);
}

namespace tsim {
constexpr int TOPK_MAX_LISTS = 28;   // largest k the list kernels (KL = 32) serve
constexpr int TOPK_MAX_K = 64;       // largest k of tsim_cosine_topk_ex / tsim_dot_topk_ex / tsim_cosine_topk_workspace_bytes
constexpr int TOPK_LARGE_MAX_K = TSIM_TOPK_MAX_K;   // largest k of the _large entries
static_assert(TOPK_LARGE_MAX_K == SL_MAX_K, "LDS lists of the brute-force kernels");

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Workspace of one search call: byte offsets, and the sizes the widening and brute-force passes run with.
//   part_s / part_i: partial lists of the list kernels; empty for k > 28.
//   cap: collect-buffer entries per slot, the smallest power of two >= 4k and >= 1 024 (the bound of flag_all_kernel sits near
//        rank 1.4 k on Gaussian rows, the 2 eps band adds a few hundred).  kp: LDS list length of the brute-force pass.
//   bf_nch chunks of bf_rows rows in the brute-force pass: at most 64, of at least 256 rows; for k > 64 of at least SL_NB rows
//        and no more than keep the chunk lists (Q x chunks x k entries of 8 B) within BF_BUDGET.
constexpr size_t BF_BUDGET = (size_t)256 << 20;
struct SearchWs {
    size_t part_s, part_i, gthr, bmax, ctl, flag_q, flag_thr, flag_eps, unres_q, coll_cnt, coll_buf, bf_s, bf_i, total;
    int cap, kp, bf_nch, bf_rows;
};

static void plan_workspace(int64_t Q, int64_t N, int k, SearchWs *w) {
    size_t part = 0;
    if (k <= TOPK_MAX_LISTS) {   // the plan depends on the padded width only through the wave count: take the larger layout
        for (int D : {384, 768}) {
            TopkPlan a, pa, pb;
            plan_topk(Q, N, D, k, &a);
            size_t e = a.part_elems;
            if (N >= 4 * 131072) {   // two-phase main pass: the lists of both launches side by side
                plan_topk(Q, 131072, D, k, &pa);
                plan_topk(Q, N - 131072, D, k, &pb);
                if (pa.part_elems + pb.part_elems > e) e = pa.part_elems + pb.part_elems;
            }
            if (e > part) part = e;
        }
    }
    w->cap = 1024;
    while (w->cap < 4 * k) w->cap <<= 1;
    w->kp = sl_list_len(k);
    const bool large = k > TOPK_MAX_K;
    const int64_t min_rows = large ? SL_NB : 256, within_budget = large ? (int64_t)(BF_BUDGET / ((size_t)Q * k * 8)) : 64;
    const int64_t nch = std::max<int64_t>(1, std::min<int64_t>({64, (N + min_rows - 1) / min_rows, within_budget}));
    w->bf_nch = (int)nch;
    w->bf_rows = (int)((N + nch - 1) / nch);
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += align256(bytes); return at; };
    w->part_s = take(part * 4);
    w->part_i = take(part * 4);
    w->gthr = take((size_t)Q * 4);
    w->bmax = take((size_t)Q * K1_PREPASS_MAX_P2 * 4);
    w->ctl = take(CTL_WORDS * 4);   // ctl .. coll_cnt contiguous: cleared together, coll_buf - ctl bytes
    w->flag_q = take((size_t)Q * 4);
    w->flag_thr = take((size_t)Q * 4);
    w->flag_eps = take((size_t)Q * 4);
    w->unres_q = take((size_t)Q * 4);
    w->coll_cnt = take((size_t)Q * 4);
    w->coll_buf = take((size_t)Q * w->cap * 8);
    w->bf_s = take((size_t)Q * w->bf_nch * k * 4);
    w->bf_i = take((size_t)Q * w->bf_nch * k * 4);
    w->total = o;
}

// plan of the widening pass: enough chunks that ONE flagged query block still spreads over the chip
static void plan_collect(int64_t Q, int64_t N, int D, TopkPlan *p) {
    plan_topk(Q, N, D, 1, p);
    int64_t nch = 256, max_ch = (N + 255) / 256;
    if (nch > max_ch) nch = max_ch;
    if (nch < 8) {   // the kernel's block map wants 1, 2, 4 or >= 8 chunks
        int p2 = 1;
        while (p2 * 2 <= nch) p2 *= 2;
        nch = p2;
    }
    int64_t rpc = (N + nch - 1) / nch;
    rpc = (rpc + K1_TILE_ROWS - 1) / K1_TILE_ROWS * K1_TILE_ROWS;
    p->rows_per_chunk = (int)rpc;
    p->nchunks = (int)((N + rpc - 1) / rpc);
    if (p->nchunks < 8 && (p->nchunks & (p->nchunks - 1))) {   // rounding produced 3, 5, 6 or 7 chunks: use fewer, longer ones
        int p2 = 1;
        while (p2 * 2 <= p->nchunks) p2 *= 2;
        rpc = (N + p2 - 1) / p2;
        rpc = (rpc + K1_TILE_ROWS - 1) / K1_TILE_ROWS * K1_TILE_ROWS;
        p->rows_per_chunk = (int)rpc;
        p->nchunks = (int)((N + rpc - 1) / rpc);
    }
    p->P2 = p->nchunks * 2;
}

// block maxima over the WHOLE shard in >= 2*kneed partitions (k > 28: the kneed-th largest block maximum is a lower bound
// of the kneed-th best MFMA score); false when the shard is too small for that many partitions
static bool plan_fullmax(int64_t Q, int64_t N, int D, int kneed, TopkPlan *p) {
    plan_topk(Q, N, D, 1, p);
    int64_t nch = 512 / p->nqb;
    if (nch < kneed) nch = kneed;            // P2 = 2 nch >= 2 kneed
    if (nch > K1_PREPASS_MAX_P2 / 2) nch = K1_PREPASS_MAX_P2 / 2;
    int64_t rpc = (N + nch - 1) / nch;
    rpc = (rpc + K1_TILE_ROWS - 1) / K1_TILE_ROWS * K1_TILE_ROWS;
    p->rows_per_chunk = (int)rpc;
    p->nchunks = (int)((N + rpc - 1) / rpc);
    p->P2 = p->nchunks * 2;
    p->part_elems = (size_t)Q * p->P2;
    // every partition (a lane half of a chunk: rows 4h..4h+3 of each group of 8) must hold at least one row
    return p->nchunks >= 8 && p->P2 >= kneed && p->P2 <= K1_PREPASS_MAX_P2 && N - (int64_t)(p->nchunks - 1) * rpc >= 8;
}

// Two-phase main pass (large shards): phase A = the first K1_PHASE_A_ROWS rows, phase B = the rest.
constexpr int64_t K1_PHASE_A_ROWS = 131072;
static bool plan_two_phase(int64_t Q, int64_t N, int D, int k, TopkPlan *pa, TopkPlan *pb) {
    // one or two query blocks: the chip is filled by corpus chunks alone and two extra launches cost more than the tighter
    // bound saves (Q = 256: 0.37 -> 0.44 ms); from four query blocks on the second phase wins (Q = 4096: -3 %)
    if (N < 4 * K1_PHASE_A_ROWS || Q <= 768) return false;
    plan_topk(Q, K1_PHASE_A_ROWS, D, k, pa);
    plan_topk(Q, N - K1_PHASE_A_ROWS, D, k, pb);
    return true;
}

// The operands of one search call, and the rows its exact scores are taken from: the float32 rows (SM_COS, SM_DOT) or the unit
// rows themselves (SM_UNIT, d = ld).
struct SearchOperands {
    const unit_t *uq, *uc;
    const float *q_f32, *c_f32;
    int64_t ldq_f32, ldc_f32;
    int d, ld;
};
template <typename T>
struct ExactRows {
    using row_t = T;
    const T *xq;
    int64_t ldq;
    const T *xc;
    int64_t ldc;
    int d;
};

// The one place the runtime score mode becomes a compile-time one: f(ExactRows<T>, std::integral_constant<int, SM>).
template <typename F>
static void with_score_mode(int sm, const SearchOperands &o, F f) {
    const ExactRows<float> rf{o.q_f32, o.ldq_f32, o.c_f32, o.ldc_f32, o.d};   // (null rows in SM_UNIT, where it is not used)
    if (sm == SM_COS) f(rf, std::integral_constant<int, SM_COS>{});
    else if (sm == SM_DOT) f(rf, std::integral_constant<int, SM_DOT>{});
    else if (sm == SM_L2)   // (the float32 rows read through l2_f32, a struct of one float: the same layout, and the kernels only
                            // ever load from them; the type is what keeps the other spaces' instantiations as they were)
        f(ExactRows<l2_f32>{reinterpret_cast<const l2_f32 *>(o.q_f32), o.ldq_f32, reinterpret_cast<const l2_f32 *>(o.c_f32), o.ldc_f32,
                            o.d},
          std::integral_constant<int, SM_L2>{});
    else f(ExactRows<unit_t>{o.uq, o.ld, o.uc, o.ld, o.ld}, std::integral_constant<int, SM_UNIT>{});
}

// Widening pass + its finalisation, then the brute-force pass for whatever is still unresolved (all launches leave at once
// when there is nothing to do)
static int search_tail(int sm, const SearchWs &w, char *ws, int64_t Q, int64_t N, const SearchOperands &o, int k, float *out_s,
                       int64_t *out_i, int64_t idx_offset, const GuardArgs &g, bool run_collect, hipStream_t st) {
    if (run_collect) {
        TopkPlan cp;
        plan_collect(Q, N, o.ld, &cp);
        K1Collect coll{};
        coll.qcount = g.ctl + CTL_NFLAG;
        coll.qmap = g.flag_q;
        coll.buf = reinterpret_cast<unsigned long long *>(ws + w.coll_buf);
        coll.cnt = reinterpret_cast<int *>(ws + w.coll_cnt);
        coll.cap = w.cap;
        int rc = k1_launch_collect(cp, o.ld, o.uq, Q, o.uc, N, g.flag_thr, coll, st);
        if (rc) return rc;
        const unsigned wg = (unsigned)(Q < 2048 ? Q : 2048);
        with_score_mode(sm, o, [&](auto x, auto smc) {
            using T = typename decltype(x)::row_t;
            constexpr int SM = decltype(smc)::value;
            hipLaunchKernelGGL((widen_finalize_kernel<T, SM>), dim3(wg), dim3(256), (size_t)w.cap * 8, st, coll.buf, coll.cnt, w.cap, Q,
                               x.xq, x.ldq, x.xc, x.ldc, x.d, k, out_s, out_i, idx_offset, g);
        });
        TSIM_HIP_CHECK(hipGetLastError());
    }
    float *bf_s = reinterpret_cast<float *>(ws + w.bf_s);
    int *bf_i = reinterpret_cast<int *>(ws + w.bf_i);
    const unsigned us = (unsigned)(Q < 64 ? Q : 64);
    // (brute force has no guard: DOT scores exactly like UNIT, on the float32 rows; L2 by its row type)
    with_score_mode(sm, o, [&](auto x, auto smc) {
        using T = typename decltype(x)::row_t;
        constexpr bool COS = decltype(smc)::value == SM_COS;
        hipLaunchKernelGGL((bf_partial_kernel<T, COS>), dim3(w.bf_nch, us), dim3(256), 0, st, Q, N, w.bf_rows, x.xq, x.ldq, x.xc,
                           x.ldc, x.d, k, w.kp, bf_s, bf_i, g);
    });
    TSIM_HIP_CHECK(hipGetLastError());
    const unsigned mg = (unsigned)(Q < 1024 ? Q : 1024);
    hipLaunchKernelGGL(bf_merge_kernel, dim3(mg), dim3(256), 0, st, Q, w.bf_nch, k, w.kp, bf_s, bf_i, out_s, out_i, idx_offset, g);
    TSIM_HIP_CHECK(hipGetLastError());
    if (sm == SM_L2) {   // every kernel above wrote -dist^2 (and -inf padding)
        const int64_t n = Q * k;
        hipLaunchKernelGGL(l2_negate_scores_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, out_s, n);
        TSIM_HIP_CHECK(hipGetLastError());
    }
    return TSIM_OK;
}

// GuardArgs of one call over its workspace words
static GuardArgs make_guard(char *ws, const SearchWs &w, int ld, const float *ec_rho_max, const float *ec_maxnorm,
                            int32_t *out_status) {
    GuardArgs g;
    g.c1 = 4.0f;
    // unit rows only: float32 accumulation of ld exact products of unit rows, any order, rounding or truncation per step
    // (ld * 2^-23 |a||b|, |a|,|b| <= 1 + 2^-10) + the final rounding of the exact score
    g.floor = (float)ld * 1.1920929e-7f * 1.003f + 2.4e-7f;
    g.rho_c_max = ec_rho_max;
    g.rho_c_default = rho_apriori(ld);
    g.ld = ld;
    g.flag_eps = reinterpret_cast<float *>(ws + w.flag_eps);
    g.ctl = reinterpret_cast<int *>(ws + w.ctl);
    g.flag_q = reinterpret_cast<int *>(ws + w.flag_q);
    g.flag_thr = reinterpret_cast<int *>(ws + w.flag_thr);
    g.unres_q = reinterpret_cast<int *>(ws + w.unres_q);
    g.status = out_status;
    g.c_maxnorm = ec_maxnorm;
    return g;
}

// k > 28: no list kernel.  Block maxima over the whole shard give a lower bound of the k-th best MFMA score; flag_all_kernel
// turns it into every query's collection threshold (or hands every query to brute force: *ok = false, shard too small).
// The control words must be cleared on the stream before.
static int threshold_all(int sm, int64_t Q, int64_t N, const SearchOperands &o, int k, float *bmax, int *gthr, const GuardArgs &g,
                         bool *ok, hipStream_t st) {
    TopkPlan fp;
    *ok = plan_fullmax(Q, N, o.ld, k, &fp);
    if (*ok) {
        int rc0 = k1_launch_blockmax(fp, o.ld, o.uq, Q, o.uc, N, bmax, st);
        if (rc0) return rc0;
        launch_thr_select(bmax, fp.P2, Q, k, gthr, st);
        TSIM_HIP_CHECK(hipGetLastError());
    }
    with_score_mode(sm, o, [&](auto, auto smc) {   // (SM_UNIT: the float32 query rows are null and not read)
        hipLaunchKernelGGL(flag_all_kernel<decltype(smc)::value>, dim3((unsigned)((Q + 3) / 4)), dim3(256), 0, st, Q, gthr, !*ok,
                           o.q_f32, o.ldq_f32, o.uq, o.d, g);
    });
    TSIM_HIP_CHECK(hipGetLastError());
    return TSIM_OK;
}

// finalize of the list kernels' partial lists (p.KL = 16 or 32)
static void launch_finalize(int sm, const TopkPlan &p, const float *part_s, const int *part_i, int64_t Q, int64_t N,
                            const SearchOperands &o, int k, const int *gthr, float *out_s, int64_t *out_i, int64_t idx_offset,
                            const GuardArgs &g, hipStream_t st) {
    const dim3 grid((unsigned)((Q + 3) / 4));
    auto launch = [&](auto x, auto smc, auto klc) {
        using T = typename decltype(x)::row_t;
        constexpr int SM = decltype(smc)::value, KL = decltype(klc)::value;
        constexpr int LBW = KL == 16 ? 8 : 4;   // (eight lists of 32 at a time spill)
        if (Q <= 1024 && x.d <= 384)
            hipLaunchKernelGGL((cos_topk_finalize_kernel<KL, T, SM, 16, LBW>), grid, dim3(256), 0, st, part_s, part_i, p.P2, Q, N, x.xq,
                               x.ldq, x.xc, x.ldc, x.d, k, o.uq, gthr, out_s, out_i, idx_offset, g);
        else if (Q <= 1024)
            hipLaunchKernelGGL((cos_topk_finalize_kernel<KL, T, SM, 8, LBW>), grid, dim3(256), 0, st, part_s, part_i, p.P2, Q, N, x.xq,
                               x.ldq, x.xc, x.ldc, x.d, k, o.uq, gthr, out_s, out_i, idx_offset, g);
        else
            hipLaunchKernelGGL((cos_topk_finalize_kernel<KL, T, SM, 4, 4>), grid, dim3(256), 0, st, part_s, part_i, p.P2, Q, N, x.xq,
                               x.ldq, x.xc, x.ldc, x.d, k, o.uq, gthr, out_s, out_i, idx_offset, g);
    };
    with_score_mode(sm, o, [&](auto x, auto smc) {
        if (p.KL == 16) launch(x, smc, std::integral_constant<int, 16>{});
        else launch(x, smc, std::integral_constant<int, 32>{});
    });
}
}  // namespace tsim

#include "range_search.h"   // exact range search: kernels and entry points, on the helpers above
#include "list_search.h"    // exact top-k within candidate lists: the indirect form of the brute-force pass
#include "code_search.h"    // what the two code searches below share: list carve, flush policy, merge, re-score, host drivers
#include "hamming_search.h" // binary embeddings: sign-bit codes, exact Hamming top-k, re-score against the +-1 expansion
#include "int8_search.h"    // int8 embeddings: calibrated quantiser, exact inner-product top-k on the int8 MFMA, re-score
#include "ivf_search.h"     // inverted lists: exact scan of the contiguous lists each query probes
#include "pq_search.h"      // product quantisation: the PQ encoder, integer lookup tables, exact ADC top-k in the code-search frame
#include "ivfpq_search.h"   // IVF-PQ: residual tables and the exact ADC scan of the PQ-coded lists each query probes
#include "graph_search.h"   // graph index: beam search over a proximity graph with the exact scores, and the kNN-graph pruning
#include "graph_insert.h"   // graph index, insertion: forward edges by detour count, reverse edges by the exact score, in place
#include "community_select.h"   // community detection: the de-overlap of candidate communities, in rounds or in one workgroup
#include "mst_prim.h"       // HDBSCAN: Prim's minimum spanning tree of the mutual-reachability graph, on the exact squared distances

extern "C" int tsim_cosine_topk_plan(int64_t Q, int64_t N, int ld, int k, int32_t plan[4]) {
    if (Q <= 0 || N <= 0 || k <= 0 || k > TOPK_MAX_K || !plan || tsim_pad_dim(ld) != ld)
        return fail(TSIM_EINVAL, "tsim_cosine_topk_plan: bad arguments (Q=%lld N=%lld ld=%d k=%d)", (long long)Q, (long long)N, ld, k);
    TopkPlan p;
    plan_topk(Q, N, ld, k <= TOPK_MAX_LISTS ? k : 10, &p);
    plan[0] = p.nqb;
    plan[1] = p.nchunks;
    plan[2] = p.rows_per_chunk;
    // block mapping of cos_topk_partial_kernel: >= 8 chunks: XCD x owns chunks x, x+8, ... with all their query blocks;
    // fewer: 8 / nchunks XCDs share a chunk and split its query blocks
    plan[3] = p.nchunks >= 8 ? ((p.nchunks + 7) / 8) * p.nqb : (p.nqb + (8 / p.nchunks) - 1) / (8 / p.nchunks);
    return TSIM_OK;
}

extern "C" size_t tsim_cosine_topk_workspace_bytes(int64_t Q, int64_t N, int k) {
    return k <= TOPK_MAX_K ? tsim_topk_large_workspace_bytes(Q, N, k) : 0;
}

extern "C" size_t tsim_topk_large_workspace_bytes(int64_t Q, int64_t N, int k) {
    if (Q <= 0 || N <= 0 || k <= 0 || k > TOPK_LARGE_MAX_K) return 0;
    SearchWs w;
    plan_workspace(Q, N, k, &w);
    return w.total;
}

// One search call: validate, plan, [k <= 28: pre-pass, main pass, finalize | else: threshold_all], tail.  sm: SM_UNIT (no
// float32 matrices), SM_COS, SM_DOT or SM_L2 (float32 matrices given).  `what` names the entry point in error messages, kmax is its
// largest k.
static int topk_search(int sm, const char *what, int kmax, const void *eq, const float *eq_f32, int64_t ldq_f32, int64_t Q,
                       const void *ec, const float *ec_f32, int64_t ldc_f32, const float *ec_maxnorm, const float *ec_rho_max,
                       int64_t N, int d, int ld, int k, float *out_scores, int64_t *out_idx, int32_t *out_status,
                       int64_t idx_offset, void *workspace, size_t workspace_bytes, void *stream) {
    const int dw = d + (sm == SM_L2);   // width of the half operands (L2: one element longer than the rows)
    if (sm == SM_DOT || sm == SM_L2) {
        TSIM_REQUIRE(eq_f32 && ec_f32, "%s: the float32 matrices are required", what);
        TSIM_REQUIRE(ec_maxnorm && ec_rho_max, "%s: the corpus rows' max-norm word and measured rho_max are required", what);
    }
    TSIM_REQUIRE(eq && ec && out_scores && out_idx, "%s: null pointer", what);
    TSIM_REQUIRE(Q > 0 && N > 0, "%s: empty input Q=%lld N=%lld", what, (long long)Q, (long long)N);
    TSIM_REQUIRE(k >= 1 && k <= kmax, "%s: k=%d outside 1..%d", what, k, kmax);
    TSIM_REQUIRE(N < (1ll << 31) - 64 && Q < (1ll << 31) - 512, "%s: shard too large for 32-bit row ids", what);
    TSIM_REQUIRE((sm != SM_L2 || d > 0) && ld == tsim_pad_dim(dw) && ld > 0, "%s: rows must be padded to tsim_pad_dim(%d)=%d (got ld=%d)",
                 what, dw, tsim_pad_dim(dw), ld);
    TSIM_REQUIRE((((uintptr_t)eq | (uintptr_t)ec) & 15) == 0, "%s: embedding matrices must be 16-byte aligned", what);
    TSIM_REQUIRE((eq_f32 == nullptr) == (ec_f32 == nullptr), "%s: pass both float32 matrices or neither", what);
    if (eq_f32) TSIM_REQUIRE(ldq_f32 >= d && ldc_f32 >= d, "%s: float32 row strides %lld/%lld < d=%d", what, (long long)ldq_f32,
                             (long long)ldc_f32, d);
    hipStream_t st = as_stream(stream);
    const unit_t *uq = (const unit_t *)eq, *uc = (const unit_t *)ec;
    const SearchOperands o{uq, uc, eq_f32, ec_f32, ldq_f32, ldc_f32, d, ld};
    SearchWs w;
    plan_workspace(Q, N, k, &w);
    if (!workspace || workspace_bytes < w.total)
        return fail(TSIM_ENOMEM, "%s: workspace %zu B < %zu B", what, workspace_bytes, w.total);
    char *ws = reinterpret_cast<char *>(workspace);
    float *part_s = reinterpret_cast<float *>(ws + w.part_s);
    int *part_i = reinterpret_cast<int *>(ws + w.part_i);
    int *gthr = reinterpret_cast<int *>(ws + w.gthr);   // per-query shared threshold words, re-initialised every call
    float *bmax = reinterpret_cast<float *>(ws + w.bmax);
    const GuardArgs g = make_guard(ws, w, ld, ec_rho_max, ec_maxnorm, out_status);
    // ctl .. coll_cnt are contiguous: one memset clears the control words and the per-slot counters — or the threshold kernel of
    // the pre-pass does (nothing in front of it touches them)
    const size_t ctl_bytes = w.coll_buf - w.ctl;

    bool run_collect = true;
    if (k <= TOPK_MAX_LISTS) {
        TopkPlan p, pp;
        plan_topk(Q, N, ld, k, &p);
        if (plan_prepass(Q, N, p, &pp)) {
            // threshold pre-pass: block maxima over the first rows, KL-th largest per query -> initial shared bounds
            const int64_t S = (int64_t)pp.nchunks * pp.rows_per_chunk;
            int rc0 = k1_launch_blockmax(pp, ld, uq, Q, uc, S, bmax, st);
            if (rc0) return rc0;
            launch_thr_select(bmax, pp.P2, Q, p.KL, gthr, st, reinterpret_cast<int *>(ws + w.ctl), (int)(ctl_bytes / 4));
            TSIM_HIP_CHECK(hipGetLastError());
        } else {
            TSIM_HIP_CHECK(hipMemsetAsync(gthr, 0x80, (size_t)Q * 4, st));
            TSIM_HIP_CHECK(hipMemsetAsync(ws + w.ctl, 0, ctl_bytes, st));
        }
        hipEvent_t ev0 = g_ev_start, ev1 = g_ev_stop;
        g_ev_start = g_ev_stop = nullptr;
        if (ev0) TSIM_HIP_CHECK(hipEventRecord(ev0, st));
        TopkPlan pa, pb;
        if (plan_two_phase(Q, N, ld, k, &pa, &pb)) {
            // main pass in two launches: rows [0, NA) with the pre-pass bounds, then the rest with the KL-th best score of
            // phase A as the bound (thr_update_kernel).  Lists of both phases sit side by side: P2 = pa.P2 + pb.P2.
            const int64_t NA = K1_PHASE_A_ROWS;
            p.P2 = pa.P2 + pb.P2;
            K1Collect ra{}, rb{};
            ra.p2_base = 0; ra.p2_total = p.P2; ra.row_base = 0;
            rb.p2_base = pa.P2; rb.p2_total = p.P2; rb.row_base = (int)NA;
            int rc = p.KL == 16 ? k1_launch_kl16(pa, ld, uq, Q, uc, NA, part_s, part_i, gthr, st, ra)
                                : k1_launch_kl32(pa, ld, uq, Q, uc, NA, part_s, part_i, gthr, st, ra);
            if (rc) return rc;
            const unsigned ug = (unsigned)((Q + 3) / 4);
            if (p.KL == 16) hipLaunchKernelGGL(thr_update_kernel<16>, dim3(ug), dim3(256), 0, st, part_s, part_i, p.P2, 0, pa.P2, Q, gthr);
            else hipLaunchKernelGGL(thr_update_kernel<32>, dim3(ug), dim3(256), 0, st, part_s, part_i, p.P2, 0, pa.P2, Q, gthr);
            TSIM_HIP_CHECK(hipGetLastError());
            rc = p.KL == 16 ? k1_launch_kl16(pb, ld, uq, Q, uc + NA * ld, N - NA, part_s, part_i, gthr, st, rb)
                            : k1_launch_kl32(pb, ld, uq, Q, uc + NA * ld, N - NA, part_s, part_i, gthr, st, rb);
            if (rc) return rc;
        } else {
            int rc = p.KL == 16 ? k1_launch_kl16(p, ld, uq, Q, uc, N, part_s, part_i, gthr, st)
                                : k1_launch_kl32(p, ld, uq, Q, uc, N, part_s, part_i, gthr, st);
            if (rc) return rc;
        }
        if (ev1) TSIM_HIP_CHECK(hipEventRecord(ev1, st));
        launch_finalize(sm, p, part_s, part_i, Q, N, o, k, gthr, out_scores, out_idx, idx_offset, g, st);
        TSIM_HIP_CHECK(hipGetLastError());
    } else {
        // k > 28: no list kernel.  Every row above (bound - margin) is collected and re-scored; widen_finalize's guard decides
        // whether that was enough.
        TSIM_HIP_CHECK(hipMemsetAsync(ws + w.ctl, 0, ctl_bytes, st));
        int rc = threshold_all(sm, Q, N, o, k, bmax, gthr, g, &run_collect, st);
        if (rc) return rc;
    }
    return search_tail(sm, w, ws, Q, N, o, k, out_scores, out_idx, idx_offset, g, run_collect, st);
}

extern "C" int tsim_cosine_topk_ex(const void *eq, const float *eq_f32, int64_t ldq_f32, int64_t Q, const void *ec,
                                   const float *ec_f32, int64_t ldc_f32, const float *ec_rho_max, int64_t N, int d, int ld, int k,
                                   float *out_scores, int64_t *out_idx, int32_t *out_status, int64_t idx_offset,
                                   void *workspace, size_t workspace_bytes, void *stream) {
    return topk_search(eq_f32 ? SM_COS : SM_UNIT, "cosine_topk", TOPK_MAX_K, eq, eq_f32, ldq_f32, Q, ec, ec_f32, ldc_f32, nullptr,
                       ec_rho_max, N, d, ld, k, out_scores, out_idx, out_status, idx_offset, workspace, workspace_bytes, stream);
}

extern "C" int tsim_dot_topk_ex(const void *eq, const float *eq_f32, int64_t ldq_f32, int64_t Q, const void *ec,
                                const float *ec_f32, int64_t ldc_f32, const float *ec_maxnorm, const float *ec_rho_max, int64_t N,
                                int d, int ld, int k, float *out_scores, int64_t *out_idx, int32_t *out_status, int64_t idx_offset,
                                void *workspace, size_t workspace_bytes, void *stream) {
    return topk_search(SM_DOT, "dot_topk", TOPK_MAX_K, eq, eq_f32, ldq_f32, Q, ec, ec_f32, ldc_f32, ec_maxnorm, ec_rho_max, N, d, ld,
                       k, out_scores, out_idx, out_status, idx_offset, workspace, workspace_bytes, stream);
}

extern "C" int tsim_cosine_topk_large(const void *eq, const float *eq_f32, int64_t ldq_f32, int64_t Q, const void *ec,
                                      const float *ec_f32, int64_t ldc_f32, const float *ec_rho_max, int64_t N, int d, int ld,
                                      int k, float *out_scores, int64_t *out_idx, int32_t *out_status, int64_t idx_offset,
                                      void *workspace, size_t workspace_bytes, void *stream) {
    return topk_search(eq_f32 ? SM_COS : SM_UNIT, "cosine_topk", TOPK_LARGE_MAX_K, eq, eq_f32, ldq_f32, Q, ec, ec_f32, ldc_f32,
                       nullptr, ec_rho_max, N, d, ld, k, out_scores, out_idx, out_status, idx_offset, workspace, workspace_bytes,
                       stream);
}

extern "C" int tsim_dot_topk_large(const void *eq, const float *eq_f32, int64_t ldq_f32, int64_t Q, const void *ec,
                                   const float *ec_f32, int64_t ldc_f32, const float *ec_maxnorm, const float *ec_rho_max,
                                   int64_t N, int d, int ld, int k, float *out_scores, int64_t *out_idx, int32_t *out_status,
                                   int64_t idx_offset, void *workspace, size_t workspace_bytes, void *stream) {
    return topk_search(SM_DOT, "dot_topk", TOPK_LARGE_MAX_K, eq, eq_f32, ldq_f32, Q, ec, ec_f32, ldc_f32, ec_maxnorm, ec_rho_max, N,
                       d, ld, k, out_scores, out_idx, out_status, idx_offset, workspace, workspace_bytes, stream);
}

extern "C" int tsim_l2_guard_host(float m, float eps, double nqs, double qq, float dk, double out[3]) {
    TSIM_REQUIRE(out, "l2_guard_host: null pointer");
    out[0] = l2_dist_up(dk);
    out[1] = l2_bound_low(m, eps, nqs, qq);
    out[2] = l2_tau_lo(dk, eps, nqs, qq);
    return TSIM_OK;
}

extern "C" int tsim_l2_topk_ex(const void *eq_aug, const float *eq_f32, int64_t ldq_f32, int64_t Q, const void *ec_aug,
                               const float *ec_f32, int64_t ldc_f32, const float *ec_maxnorm, const float *ec_rho_max, int64_t N,
                               int d, int ld, int k, float *out_scores, int64_t *out_idx, int32_t *out_status, int64_t idx_offset,
                               void *workspace, size_t workspace_bytes, void *stream) {
    return topk_search(SM_L2, "l2_topk", TOPK_MAX_K, eq_aug, eq_f32, ldq_f32, Q, ec_aug, ec_f32, ldc_f32, ec_maxnorm, ec_rho_max,
                       N, d, ld, k, out_scores, out_idx, out_status, idx_offset, workspace, workspace_bytes, stream);
}

extern "C" int tsim_l2_topk_large(const void *eq_aug, const float *eq_f32, int64_t ldq_f32, int64_t Q, const void *ec_aug,
                                  const float *ec_f32, int64_t ldc_f32, const float *ec_maxnorm, const float *ec_rho_max,
                                  int64_t N, int d, int ld, int k, float *out_scores, int64_t *out_idx, int32_t *out_status,
                                  int64_t idx_offset, void *workspace, size_t workspace_bytes, void *stream) {
    return topk_search(SM_L2, "l2_topk", TOPK_LARGE_MAX_K, eq_aug, eq_f32, ldq_f32, Q, ec_aug, ec_f32, ldc_f32, ec_maxnorm,
                       ec_rho_max, N, d, ld, k, out_scores, out_idx, out_status, idx_offset, workspace, workspace_bytes, stream);
}

extern "C" int tsim_cosine_topk(const void *eq, int64_t Q, const void *ec, int64_t N, int d, int ld, int k,
                                float *out_scores, int64_t *out_idx, int64_t idx_offset, void *workspace,
                                size_t workspace_bytes, void *stream) {
    return tsim_cosine_topk_ex(eq, nullptr, 0, Q, ec, nullptr, 0, nullptr, N, d, ld, k, out_scores, out_idx, nullptr, idx_offset,
                               workspace, workspace_bytes, stream);
}

extern "C" int tsim_topk_merge_strided(const float *scores, const int64_t *idx, int nlists, int64_t Q, int k_in, int k_out,
                                       int64_t list_stride_scores, int64_t list_stride_idx, float *out_scores,
                                       int64_t *out_idx, void *stream) {
    TSIM_REQUIRE(scores && idx && out_scores && out_idx, "topk_merge: null pointer");
    TSIM_REQUIRE(nlists >= 1 && Q >= 0 && k_in >= 1 && k_out >= 1, "topk_merge: bad shape");
    TSIM_REQUIRE(nlists == 1 || (list_stride_scores >= Q * k_in && list_stride_idx >= Q * k_in),
                 "topk_merge: list strides %lld / %lld < Q * k_in = %lld", (long long)list_stride_scores,
                 (long long)list_stride_idx, (long long)(Q * k_in));
    if (Q == 0) return TSIM_OK;
    if (k_out > TOPK_MAX_K && k_out <= TOPK_LARGE_MAX_K) {   // sort-and-merge in LDS instead of k_out rounds of a wave max
        hipLaunchKernelGGL(topk_merge_large_kernel, dim3((unsigned)(Q < 4096 ? Q : 4096)), dim3(256), 0, as_stream(stream), scores,
                           idx, nlists, Q, k_in, k_out, sl_list_len(k_out), list_stride_scores, list_stride_idx, out_scores, out_idx);
        TSIM_HIP_CHECK(hipGetLastError());
        return TSIM_OK;
    }
    hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)((Q + 3) / 4)), dim3(256), 0, as_stream(stream), scores,
                       idx, nlists, Q, k_in, k_out, list_stride_scores, list_stride_idx, out_scores, out_idx);
    TSIM_HIP_CHECK(hipGetLastError());
    return TSIM_OK;
}

extern "C" int tsim_topk_merge(const float *scores, const int64_t *idx, int nlists, int64_t Q, int k_in, int k_out,
                               float *out_scores, int64_t *out_idx, void *stream) {
    return tsim_topk_merge_strided(scores, idx, nlists, Q, k_in, k_out, Q * k_in, Q * k_in, out_scores, out_idx, stream);
}

extern "C" int tsim_cos_sim(const float *a, int64_t na, const float *b, int64_t nb, int d, float *out, void *stream) {
    TSIM_REQUIRE(a && b && out, "cos_sim: null pointer");
    TSIM_REQUIRE(na >= 0 && nb >= 0 && d > 0, "cos_sim: bad shape");
    if (na == 0 || nb == 0) return TSIM_OK;
    dim3 grid((unsigned)((nb + 63) / 64), (unsigned)((na + 63) / 64));
    hipLaunchKernelGGL(cos_sim_kernel, grid, dim3(256), 0, as_stream(stream), a, na, b, nb, d, out);
    TSIM_HIP_CHECK(hipGetLastError());
    return TSIM_OK;
}

extern "C" int tsim_mean_pool(const void *hidden, int hidden_dtype, const int32_t *mask, int64_t B, int S, int H,
                              float *out, void *stream) {
    TSIM_REQUIRE(hidden && mask && out, "mean_pool: null pointer");
    TSIM_REQUIRE(B >= 0 && S > 0 && H > 0 && B < 65536, "mean_pool: bad shape B=%lld S=%d H=%d", (long long)B, S, H);
    if (B == 0) return TSIM_OK;
    dim3 grid((unsigned)((H + 255) / 256), (unsigned)B);
    if (hidden_dtype == TSIM_F32)
        hipLaunchKernelGGL(mean_pool_kernel<float>, grid, dim3(256), 0, as_stream(stream), (const float *)hidden,
                           mask, S, H, out);
    else if (hidden_dtype == TSIM_BF16)
        hipLaunchKernelGGL(mean_pool_kernel<bf16_t>, grid, dim3(256), 0, as_stream(stream), (const bf16_t *)hidden,
                           mask, S, H, out);
    else
        return fail(TSIM_EINVAL, "mean_pool: unknown dtype %d", hidden_dtype);
    TSIM_HIP_CHECK(hipGetLastError());
    return TSIM_OK;
}

// CLSPoolingStrategy / max / mean-sqrt-len pooling on the padded layout (/root/reference/src/modules/modules.py:154-181)
extern "C" int tsim_pool(const void *hidden, int hidden_dtype, const int32_t *mask, int64_t B, int S, int H, int mode, float *out,
                         void *stream) {
    TSIM_REQUIRE(hidden && mask && out, "pool: null pointer");
    TSIM_REQUIRE(B >= 0 && S > 0 && H > 0 && B < 65536, "pool: bad shape B=%lld S=%d H=%d", (long long)B, S, H);
    TSIM_REQUIRE(mode >= TSIM_POOL_MEAN && mode <= TSIM_POOL_MEAN_SQRT_LEN, "pool: unknown mode %d", mode);
    TSIM_REQUIRE(hidden_dtype == TSIM_F32 || hidden_dtype == TSIM_BF16, "pool: unknown dtype %d", hidden_dtype);
    if (mode == TSIM_POOL_MEAN) return tsim_mean_pool(hidden, hidden_dtype, mask, B, S, H, out, stream);
    if (B == 0) return TSIM_OK;
    dim3 grid((unsigned)((H + 255) / 256), (unsigned)B);
    hipStream_t st = as_stream(stream);
#define PL(T, M) hipLaunchKernelGGL((mean_pool_kernel<T, M>), grid, dim3(256), 0, st, (const T *)hidden, mask, S, H, out)
#define PL_T(T) do { if (mode == TSIM_POOL_CLS) PL(T, TSIM_POOL_CLS); else if (mode == TSIM_POOL_MAX) PL(T, TSIM_POOL_MAX); \
                     else PL(T, TSIM_POOL_MEAN_SQRT_LEN); } while (0)
    if (hidden_dtype == TSIM_F32) PL_T(float); else PL_T(bf16_t);
#undef PL_T
#undef PL
    TSIM_HIP_CHECK(hipGetLastError());
    return TSIM_OK;
}
