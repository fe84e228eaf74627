// Internal helpers shared by the HIP translation units of libtsim.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string>

#include "../../include/tsim.h"

namespace tsim {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef uint16_t bf16_t;  // storage type of a bfloat16 element
// Unit rows for the search are IEEE half: 11 significand bits against bf16's 8 make the MFMA selection scores 8x closer
// to the exact cosine (the elements of a unit row are <= 1 in magnitude, so the narrower exponent costs nothing; the f16
// MFMA runs at the bf16 rate), which is what keeps the exactness guard of the search (search.hip) quiet.
typedef _Float16 unit_t;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;

constexpr int WAVE = 64;

void set_error(const std::string &msg);
int fail(int code, const char *fmt, ...);

#define TSIM_HIP_CHECK(expr)                                                                      \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess)                                                                     \
            return ::tsim::fail(TSIM_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                                __FILE__, __LINE__);                                              \
    } while (0)

#define TSIM_REQUIRE(cond, ...)                                   \
    do {                                                          \
        if (!(cond)) return ::tsim::fail(TSIM_EINVAL, __VA_ARGS__); \
    } while (0)

// ---------------------------------------------------------------- device helpers
__device__ __forceinline__ float bf16_to_f32(bf16_t v) { return __uint_as_float(((uint32_t)v) << 16); }

// round-to-nearest-even float -> bf16 bits; the plain cast lowers to v_cvt_pk_bf16_f32 on gfx950 and
// keeps NaN a NaN (MI355X_MICROARCH.md "Correctness boundaries").
__device__ __forceinline__ bf16_t f32_to_bf16(float f) {
    __bf16 b = (__bf16)f;
    return __builtin_bit_cast(bf16_t, b);
}

__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
    return (uint32_t)f32_to_bf16(lo) | ((uint32_t)f32_to_bf16(hi) << 16);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// Canonical row scale for unit rows, reproducible bit for bit on the host (oracle/search_ref.l2_normalize):
// sum of squares in float64 (each lane's partial in element order j = lane, lane+64, ..., then an xor butterfly
// 32,16,..,1 — every lane ends with the same bits), inv = 1 / max(sqrt(ss), eps) in float64; an element is then
// double(x) * inv rounded ONCE to bf16 (f64_to_bf16).
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double canonical_inv_norm(double lane_partial_ss, float eps) {
    const double ss = wave_sum_f64(lane_partial_ss);
    return 1.0 / fmax(sqrt(ss), (double)eps);
}
// float64 -> bf16 with ONE correct rounding (nearest, ties to even).  Going through float32 would round twice: a
// value within half a float ulp of a bf16 midpoint lands ON the midpoint and the tie rule then decides.  The
// midpoint case is detected on the float bits and undone by stepping one float ulp back towards the true value.
__device__ __forceinline__ bf16_t f64_to_bf16(double v) {
    const float f = (float)v;
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (bf16_t)0x7fc0;  // NaN
    if ((u & 0xffffu) == 0x8000u) {
        const double fd = fabs((double)f), av = fabs(v);
        if (av < fd) u -= 1u;
        else if (av > fd) u += 1u;
    }
    u += 0x7fffu + ((u >> 16) & 1u);
    return (bf16_t)(u >> 16);
}
// float64 -> IEEE half with ONE correct rounding: float32 by round-to-odd (truncate towards zero, set the last bit when
// anything was lost), then the hardware's nearest-even float32 -> half conversion; with 13+ spare bits the sticky last bit
// makes the second rounding see exactly which side of every half-precision midpoint the true value lies on (also in the
// subnormal half range).  numpy's float64 -> float16 cast (oracle/search_ref.unit_rows) rounds once as well.
__device__ __forceinline__ unit_t f64_to_f16(double v) {
    float f = (float)v;
    if ((double)f != v && f == f) {   // inexact (and not NaN)
        uint32_t u = __float_as_uint(f);
        if (fabs((double)f) > fabs(v)) u -= 1u;   // back to the truncation towards zero (magnitude bits only change)
        u |= 1u;
        f = __uint_as_float(u);
    }
    return (unit_t)f;
}
__device__ __forceinline__ unit_t canonical_unit_elem(float x, double inv) { return f64_to_f16((double)x * inv); }
// the same scale rounded once to float32: sentence-transformers' Normalize (F.normalize, eps 1e-12) on a float32 row
__device__ __forceinline__ float canonical_scale_f32(float x, double inv) { return (float)((double)x * inv); }

// ---- the search's exactness guard (search.hip; restated in oracle/search_ref.guard_eps) ------------------------------------
// A stored half row is u^ = u + delta, u = x / max(|x|, eps) the exact unit row, rho = |delta|_2 its rounding residual.
// For two rows, by Cauchy-Schwarz (|u| <= 1):   | u^q . u^c  -  u_q . u_c |  <=  rho_q + rho_c + rho_q rho_c,
// and u_q . u_c IS the reference's F.cosine_similarity of the float32 rows.  The MFMA score differs from u^q . u^c by the
// float32 accumulation of ld products that are exact in float32 (11 x 11 significand bits): at most
// ld * 2^-23 * |u^q| |u^c| for ANY summation order with rounding or truncation to float32 at every step.  One more 2^-22
// covers the final rounding of the exact score to float32 and a tie on it.  Every constant is rounded UP.
// ASSUMPTION, pinned: rho is the selection error of a row only if the f16 MFMA KEEPS subnormal half operands (|h| < 2^-14); one
// that flushed them would err by |u| on such an element.  Measured on MI355X (gfx950): it keeps them, for A and for B.
// tests/test_search_subnormal_gpu.py holds rows with 767 subnormal halves at d = 768 whose selection score a flush would lower by
// 2.5 eps — out of the first pass and below the widening threshold (tests/test_guard_cpu.py replays that: a wrong list, status
// 1) — and demands the oracle's lists; DESIGN.md section 7 has the numbers.  The inner-product path does not rest on this
// (flush_safe_err below); should a part flush, l2norm_rows_kernel, query_rho<false> and rho_apriori take the same treatment.
//   rho_round_up: float upper bound of a float64 residual norm; NaN / oversized values (rows with NaN or inf elements) are
//                 clamped to 2, which sends every query that meets them to the brute-force pass.
__device__ __forceinline__ float rho_round_up(double r) {
    const float f = (float)(r * (1.0 + 1e-6));
    return f < 2.f ? f : 2.f;
}
// raise *word to rho (non-negative floats order like their bit patterns).  The word is read first: once it holds a value near
// the maximum almost no row beats it, so a million rows cost a handful of atomics instead of a million serialised ones
// (measured: 11 ms -> sub-ms for 1 M rows).
__device__ __forceinline__ void rho_publish(float *word, float rho) {
    const int bits = __float_as_int(rho);
    if (bits > __hip_atomic_load(reinterpret_cast<int *>(word), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMax(reinterpret_cast<int *>(word), bits);
}
// a-priori residual bound of a canonical unit row (every element rounded to nearest half): relative 2^-11 per normal element,
// absolute 2^-25 per subnormal one  ->  rho <= 2^-11 |u| + sqrt(ld) 2^-25.  Used when the caller has no measured rho_max.
__host__ __device__ __forceinline__ float rho_apriori(int ld) {
    return 4.8828125e-4f * 1.000001f + sqrtf((float)ld) * 2.98023224e-8f * 1.000001f;
}
__device__ __forceinline__ float guard_eps(float rho_q, float rho_c, int ld) {
    const double acc = (double)ld * 1.1920928955078125e-7 * (1.0 + rho_q) * (1.0 + rho_c);
    const double e = (double)rho_q + (double)rho_c + (double)rho_q * (double)rho_c + acc + 2.384185791015625e-7;
    return (float)(e * (1.0 + 1e-6));
}

// ---- inner-product search (tsim_dot_topk_ex): corpus rows scaled by one power of two ------------------------------------------
// The max-norm word of a set of rows is a float >= max_r |c_r| (float64 norm in the canonical order, rounded up); a row with a
// non-finite element, or a norm beyond the float range, makes it +inf.  S = dot_scale(word) is the smallest power of two not
// below it (1 for an all-zero set, +inf for a non-finite word); the stored rows are half(c_r / S), |c_r / S| <= 1.  Every
// kernel that needs S derives it from the word with this one function, so rows and search always agree on it.
__host__ __device__ inline double dot_scale(float maxnorm) {
    if (!(maxnorm <= 3.4028234663852886e38f)) return INFINITY;   // inf or NaN
    if (maxnorm <= 0.f) return 1.0;
    int e = 0;
    const double fr = frexp((double)maxnorm, &e);   // maxnorm = fr 2^e, fr in [0.5, 1)
    return ldexp(1.0, fr == 0.5 ? e - 1 : e);
}
// the smallest float >= v (v >= 0 finite)
__device__ __forceinline__ float f32_round_up(double v) {
    float f = (float)v;
    if ((double)f < v) f = __uint_as_float(__float_as_uint(f) + 1u);
    return f;
}
// Residual of one scaled element v -> half h: |h - v| when the f16 MFMA keeps subnormal inputs, |v| when it flushes them to
// zero; for a subnormal (or zero) h the larger of the two, so the bound holds either way.
__device__ __forceinline__ double flush_safe_err(double h, double v) {
    const double e = h - v;
    return fabs(h) < 6.103515625e-05 ? fmax(fabs(e), fabs(v)) : e;   // 2^-14: smallest normal half
}

// GELU of two values without transcendentals, in packed fp32 (v_pk_fma_f32 / v_pk_mul_f32: two values per issue slot).
//   gelu(x) = x * Phi(x),  Phi(x) ~ 1/2 + xc * S(xc^2),  xc = clamp(x, -4, 4),  S = degree-8 Chebyshev fit of
//   (Phi(sqrt u) - 1/2) / sqrt u on u in [0, 16]  (fp32 Horner: relative error <= 2.5e-5 for x > 0, absolute error
//   <= 4e-5 on [-4, 0] — two orders below the bf16 resolution of the stored result; beyond |x| = 4 Phi is frozen at
//   Phi(+-4) = 1 - 3.2e-5 / 3.2e-5).  26 issue cycles per value against 64 for the Abramowitz-Stegun erf form it replaced
//   (rcp + exp + 12 VALU): the FFN1 epilogue is VALU-bound.
typedef __attribute__((ext_vector_type(2))) float f32x2;
__device__ __forceinline__ void gelu2(float &a, float &b) {
    const f32x2 x = {a, b};
    const f32x2 xc = {__builtin_amdgcn_fmed3f(a, -4.0f, 4.0f), __builtin_amdgcn_fmed3f(b, -4.0f, 4.0f)};
    const f32x2 u = xc * xc;
    f32x2 p = {9.56756410e-11f, 9.56756410e-11f};
    p = __builtin_elementwise_fma(p, u, (f32x2){-8.02642397e-09f, -8.02642397e-09f});
    p = __builtin_elementwise_fma(p, u, (f32x2){3.00262883e-07f, 3.00262883e-07f});
    p = __builtin_elementwise_fma(p, u, (f32x2){-6.72069427e-06f, -6.72069427e-06f});
    p = __builtin_elementwise_fma(p, u, (f32x2){1.02510894e-04f, 1.02510894e-04f});
    p = __builtin_elementwise_fma(p, u, (f32x2){-1.15122017e-03f, -1.15122017e-03f});
    p = __builtin_elementwise_fma(p, u, (f32x2){9.92152281e-03f, 9.92152281e-03f});
    p = __builtin_elementwise_fma(p, u, (f32x2){-6.64609522e-02f, -6.64609522e-02f});
    p = __builtin_elementwise_fma(p, u, (f32x2){3.98939520e-01f, 3.98939520e-01f});
    const f32x2 phi = __builtin_elementwise_fma(xc, p, (f32x2){0.5f, 0.5f});
    const f32x2 y = x * phi;
    a = y[0];
    b = y[1];
}

// async global -> LDS copy of 16 bytes per lane; LDS destination = wave-uniform base + lane*16.
__device__ __forceinline__ void glds16(const void *gsrc, void *lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)gsrc,
                                     (__attribute__((address_space(3))) void *)lds_wave_base, 16, 0, 0);
}

// ds_read_b128 at addr + immediate offset, and a COUNTED wait that names the register it releases (so that no use of it is
// scheduled above the wait): the building blocks of hand-rolled LDS prefetch pipelines (hipcc's own schedule tends to wait
// lgkmcnt(0) right behind the read it has just issued)
typedef __attribute__((ext_vector_type(4))) uint32_t lds_u32x4;
template <int OFF>
__device__ __forceinline__ void lds_read_b128_imm(lds_u32x4 &dst, uint32_t addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF) : "memory");
}
template <int N>
__device__ __forceinline__ void lgkm_wait_counted(lds_u32x4 &released) {   // all but the N youngest LDS operations are done
    asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(released) : "n"(N) : "memory");
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ void wait_lgkmcnt0() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// Opt a kernel in to more than 64 KiB of dynamic LDS.  The attribute is per DEVICE (a process may drive several GPUs), so each
// call site keeps one flag per device: `static DevOnce once; TSIM_MAX_LDS(once, kern, bytes);`
struct DevOnce { bool done[64] = {}; };
#define TSIM_MAX_LDS(once, kern, bytes)                                                                              \
    do {                                                                                                             \
        int dev_ = 0;                                                                                                \
        TSIM_HIP_CHECK(hipGetDevice(&dev_));                                                                         \
        if (dev_ < 0 || dev_ >= 64 || !(once).done[dev_]) {                                                          \
            TSIM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern),                                 \
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (bytes)));                \
            if (dev_ >= 0 && dev_ < 64) (once).done[dev_] = true;                                                    \
        }                                                                                                            \
    } while (0)

}  // namespace tsim
