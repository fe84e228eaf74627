/*
 * tsim.h — C ABI of libtsim.so, the MI355X (gfx950) embed-and-search engine.
 *
 * The reference (cr1m5onk1ng/text_similarity) has no FFI of its own: its boundary for this path is a
 * Python API whose arithmetic lives in torch / transformers.  Each entry point below replaces one of
 * those call sites; the Python classes in text_similarity_amd/ keep the reference's names and
 * signatures and reach these functions through ctypes (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in _host; the caller owns all buffers;
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream); calls only enqueue
 *     work on it, they never synchronise and never allocate device memory (except tsim_encoder_create);
 *   - EVERY launch, memset and async copy of a call goes to `stream`, nothing to any other stream; only tsim_encoder_create and
 *     tsim_encoder_error_flags synchronise.  Calls on different streams may overlap when they are given different workspaces (and,
 *     for the encoder, different handles);
 *   - `workspace` (where an entry takes one) is scratch of at least the entry's *_workspace_bytes: its contents on entry are
 *     UNSPECIFIED AND IGNORED — a call initialises what it reads, whatever an earlier call of any entry left there — and
 *     meaningless afterwards.  The two two-call protocols are the exception stated at their entries: tsim_*_range_scan* ->
 *     tsim_range_fill*, and tsim_community_select_rounds (first_round == 0 initialises) -> further rounds / _finish, keep their
 *     state in the workspace, which must be untouched between the calls (tests/test_workspace_poison_gpu.py,
 *     tests/test_side_stream_gpu.py; DESIGN.md section 3 lists every region with its first writer and first reader);
 *   - return value 0 = ok, otherwise a TSIM_E* code; tsim_last_error() gives the message for the calling
 *     thread;
 *   - "unit rows" are row-major IEEE half (float16) L2-normalised rows with a row stride of `ld` elements, ld a multiple
 *     of 8 and every row 16-byte aligned; tsim_pad_dim(d) is the stride the engine itself produces.  Half, not bf16:
 *     the elements of a unit row are <= 1, the f16 MFMA runs at the bf16 rate, and 11 significand bits keep the MFMA
 *     selection scores within ~1e-4 of the exact cosine (bf16: ~1e-3), which keeps the exactness guard quiet.
 */
#ifndef TSIM_H
#define TSIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSIM_OK 0
#define TSIM_EINVAL 1      /* bad argument (shape, alignment, unsupported size) */
#define TSIM_EHIP 2        /* a HIP runtime call failed */
#define TSIM_ENOMEM 3      /* workspace too small / allocation failed */
#define TSIM_EUNSUPPORTED 4

#define TSIM_F32 0
#define TSIM_BF16 1

#define TSIM_ARCH_BERT 0
#define TSIM_ARCH_MPNET 1
/* the BERT graph with MPNet's position rule: rows pad_id+1 .. pad_id+len, one token-type row added to every token
 * (HF RobertaModel, XLMRobertaModel, CamembertModel).  DistilBERT is TSIM_ARCH_BERT with type_emb == NULL. */
#define TSIM_ARCH_ROBERTA 2

int tsim_version(void);
const char *tsim_last_error(void);

/* Row stride (elements) of the engine's internal unit-row matrices for an embedding width d:
 * the smallest supported kernel width >= d (128, 256, 384, 512 or 768); 0 if d > 768. */
int tsim_pad_dim(int d);

/* ---------------------------------------------------------------------------------------------
 * A7  F.cosine_similarity operand preparation   /root/reference/src/pipeline/search_pipeline.py:77
 * out[r, :d] = half( x[r, :] / max(||x[r, :]||_2, eps) ), out[r, d:ld_out] = 0, evaluated canonically: float64 sum of
 * squares in a fixed order, float64 reciprocal, one rounding float64 -> half (oracle/search_ref.unit_rows is bit-identical).
 * torch divides each operand by max(norm, eps) with eps = 1e-8; a zero row stays zero, so its score
 * against anything is 0.  x_dtype is TSIM_F32 or TSIM_BF16, ld_in its row stride in elements.
 * rho_max (device float, may be NULL): atomically raised to the largest rounding residual of the rows written,
 * rho_r = || out[r] - x[r] / max(||x[r]||, eps) ||_2 (rounded up).  The caller zeroes the word once and may let several calls
 * accumulate into it (a corpus that grows); tsim_cosine_topk_ex turns it into a PROVEN bound on |MFMA score - exact score|. */
int tsim_l2norm_rows(const void *x, int x_dtype, int64_t rows, int d, int64_t ld_in,
                     void *out_f16, int ld_out, float eps, float *rho_max, void *stream);

/* ---------------------------------------------------------------------------------------------
 * A6/A7/A9  the per-query loop `expand_as -> F.cosine_similarity -> torch.topk`
 *           /root/reference/src/pipeline/search_pipeline.py:73-78, fused.
 * eq_unit [Q, ld] and ec_unit [N, ld] are L2-normalised half rows (tsim_l2norm_rows).  MFMA inner products of those rows
 * (scores live in registers, survivors go through per-lane queues in LDS; the N x Q matrix is never written) SELECT
 * candidates; every score that is returned, and the final order, comes from an exact re-score:
 *   - eq_f32 / ec_f32 given (float32 embeddings, row strides ldq_f32 / ldc_f32 elements): the reference's value
 *     x.y / (max(|x|, 1e-8) * max(|y|, 1e-8)) of the float32 rows, evaluated in float64 in a fixed order and rounded once
 *     to float32 (oracle/search_ref.exact_cosine) — torch's own float32 evaluation differs from it by rounding only;
 *   - eq_f32 == ec_f32 == NULL: the inner product of the unit rows as stored (oracle/search_ref.canonical_scores).
 * Results are ordered by (score descending, index ascending) — the tie rule torch.topk leaves undefined.
 * Exactness guard (a proof, not an estimate).  A stored half row is u^ = u + delta with u the exact unit row and
 * rho = |delta|_2; for any two rows |u^q.u^c - u_q.u_c| <= rho_q + rho_c + rho_q rho_c (Cauchy-Schwarz), u_q.u_c is the
 * reference's cosine, and the MFMA's float32 accumulation adds at most ld 2^-23 (1+rho_q)(1+rho_c).  eps_q = that bound with
 * rho_q measured from the query's own two rows and rho_c = *ec_rho_max, the largest residual of the shard's unit rows as
 * reported by tsim_l2norm_rows / tsim_encoder_forward (NULL: the a-priori bound 2^-11 + sqrt(ld) 2^-25 of a correctly rounded
 * unit row, about twice as loose).  Every row that was NOT re-scored has an MFMA score <= cut, hence an exact score
 * <= cut + eps_q: if that is below the k-th exact score the list stands (status 0).  Otherwise EVERY row whose MFMA score
 * exceeds (k-th exact score - eps_q) is collected and re-scored (status 1); if more than 1 024 rows qualify, or the bound is
 * seen to fail on a re-scored row (unit rows that are not the images of the float32 rows), the whole shard is scored exactly
 * for that query (status 2).  With unit rows only (no float32 matrices) the two scores differ by float32 accumulation alone
 * and eps = max(4 x the largest difference seen, ld 2^-23).  out_status [Q] int32 (may be NULL) reports the pass per query.
 * out_scores [Q, k] float32, out_idx [Q, k] int64 = shard row index + idx_offset (-1 / -inf when the shard has fewer
 * than k rows).  1 <= k <= 64 (k > 28 skips the list kernel: block maxima -> collect -> re-score).
 * workspace: tsim_cosine_topk_workspace_bytes(Q, N, k).
 * tsim_cosine_topk(...) == tsim_cosine_topk_ex with NULL float32 matrices and NULL status. */
size_t tsim_cosine_topk_workspace_bytes(int64_t Q, int64_t N, int k);
/* Introspection (host only, no launch): how the main pass of a search of Q queries against N rows of padded width ld is cut.
 * plan[0] = query blocks, plan[1] = corpus chunks, plan[2] = rows per chunk, plan[3] = the largest number of workgroups any one
 * XCD receives (workgroup b runs on XCD b % 8; a round is 32 of them).  Returns TSIM_OK or TSIM_EINVAL. */
int tsim_cosine_topk_plan(int64_t Q, int64_t N, int ld, int k, int32_t plan[4]);
int tsim_cosine_topk_ex(const void *eq_unit, const float *eq_f32, int64_t ldq_f32, int64_t Q,
                        const void *ec_unit, const float *ec_f32, int64_t ldc_f32, const float *ec_rho_max, int64_t N,
                        int d, int ld, int k, float *out_scores, int64_t *out_idx, int32_t *out_status,
                        int64_t idx_offset, void *workspace, size_t workspace_bytes, void *stream);
int tsim_cosine_topk(const void *eq_unit, int64_t Q, const void *ec_unit, int64_t N, int d, int ld,
                     int k, float *out_scores, int64_t *out_idx, int64_t idx_offset,
                     void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Exact inner-product search (sentence-transformers models scored by dot product; hnswlib's space='ip').
 *
 * Operands.  The corpus rows c_r (float32 or bf16, x_dtype) are scaled by ONE power of two per corpus, S = the smallest 2^e
 * >= max_r |c_r|, and stored as half(c_r / S) (each element rounded once; scaling by 2^e is exact), so every element and every
 * MFMA score lies in [-1, 1].  S comes from a device "max-norm word" (float, caller-owned, zeroed once): tsim_max_norm_rows
 * raises it to an upper bound of the rows' L2 norms (float64 in the canonical order of tsim_l2norm_rows, rounded up); a row
 * with a non-finite element, or a norm beyond the float range, makes it +inf — never a fault — and the caller can read it.
 * tsim_dot_scale(word) is the host form of the one rule every kernel uses: 1 for an all-zero corpus (word 0), +inf for a
 * non-finite word, else the smallest power of two >= word.  Several tsim_max_norm_rows calls may accumulate into one word;
 * rows made before the word grew must be made again (their S changed).
 * tsim_dot_scaled_rows writes out[r, :d] = half(x[r, :] / S), out[r, d:ld_out] = 0, and raises rho_max (may be NULL) to the
 * largest residual || out[r] - x[r] / S ||_2, rounded up, where a subnormal half element counts with the larger of its
 * rounding error and its own magnitude: the bound holds whether or not the f16 MFMA flushes subnormal inputs.  A non-finite
 * word gives zero rows (NaN where x is not finite) and rho 2. */
int tsim_max_norm_rows(const void *x, int x_dtype, int64_t rows, int d, int64_t ld_in, float *maxnorm, void *stream);
int tsim_dot_scaled_rows(const void *x, int x_dtype, int64_t rows, int d, int64_t ld_in, const float *maxnorm,
                         void *out_f16, int ld_out, float *rho_max, void *stream);
double tsim_dot_scale(float maxnorm_host);
/* Top-k by inner product: out_scores[q, j] = float32(q . c) of the float32 rows, summed in float64 in the canonical lane order
 * of the exact re-score (oracle/search_ref._lane_sum) and rounded once; order (score desc, index asc).  eq_unit: the queries'
 * unit rows (tsim_l2norm_rows, eps 1e-8); ec_scaled: tsim_dot_scaled_rows of the float32 corpus ec_f32 under ec_maxnorm, with
 * ec_rho_max its measured residual maximum.  eq_f32, ec_f32, ec_maxnorm and ec_rho_max are REQUIRED (NULL: TSIM_EINVAL; the
 * a-priori residual bound does not cover flushed subnormals).  The rest as tsim_cosine_topk_ex: same workspace
 * (tsim_cosine_topk_workspace_bytes), out_status, idx_offset, 1 <= k <= 64, -1 / -inf padding, stream.
 * Guard.  The MFMA score m approximates q.c / (nq S), nq = max(|q|, 1e-8) — monotone in q.c for a fixed query, so the main
 * pass selects by the right quantity — and |m - q.c / (nq S)| <= eps_q = guard_eps(rho_q, rho_c, ld) by the same
 * Cauchy-Schwarz argument as for cosine (|c / S| <= 1), rho_q measured flush-safe from the query's two rows, rho_c =
 * *ec_rho_max.  The guard converts between the domains with the query's float64 nq and S, slack on the safe side: the first
 * pass stands when (cut + eps_q) nq S < the k-th exact score; otherwise every row with m > k-th exact / (nq S) - eps_q is
 * collected (status 1), and brute force (status 2) takes over as for cosine.  A zero query scores 0 against every row: its
 * result is the first k rows by index. */
int tsim_dot_topk_ex(const void *eq_unit, const float *eq_f32, int64_t ldq_f32, int64_t Q, const void *ec_scaled,
                     const float *ec_f32, int64_t ldc_f32, const float *ec_maxnorm, const float *ec_rho_max, int64_t N,
                     int d, int ld, int k, float *out_scores, int64_t *out_idx, int32_t *out_status, int64_t idx_offset,
                     void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Exact Euclidean search: top-k by squared L2 distance of the float32 rows (the default space of hnswlib and faiss).
 *
 * The idea.  argmin_c |q - c|^2 = argmax_c (q.c - |c|^2 / 2): an inner product of vectors one element longer, so the MFMA
 * selection pass of the other spaces runs unchanged.  A = tsim_dot_scale(word), word the corpus' max-norm word
 * (tsim_max_norm_rows), S = 2 A.
 *   corpus row   c' = (c, -|c|^2 / (2A)):  |c'| <= A sqrt(1.25) < S, stored as half(c' / S) — no second max pass;
 *   query row    q' = (q, A):  stored as the unit row half(q' / nq'), nq' = sqrt(|q|^2 + A^2) >= A > 0;
 *   MFMA score   m ~ q'.c' / (nq' S) = (q.c - |c|^2 / 2) / nqs = (|q|^2 - dist^2) / (2 nqs),  nqs = nq' S, dist^2 = |q - c|^2:
 *                for a fixed query it falls as dist^2 grows.  A (not 1) in the extra column balances the two parts: the
 *                guard's window in dist^2 is about 1e-3 |q| |c| whatever the overall scale of the embeddings.
 * The half operands are ld = tsim_pad_dim(d + 1) wide, so d <= 767 (d = 384 runs the 512-wide kernel).
 * tsim_l2_rows writes out[r, :d] = half(x[r] / S), out[r, d] = half(-|x_r|^2 / (2 A S)) with |x_r|^2 the float64 sum in the
 * canonical order of tsim_l2norm_rows, zeros up to ld_out (>= d + 1, else TSIM_EINVAL), and raises rho_max (may be NULL) to the
 * flush-safe residual of the d + 1 elements as tsim_dot_scaled_rows does.  A non-finite word gives zero rows and rho 2.
 * tsim_l2_query_rows writes the augmented unit rows: float64 throughout, one rounding to half per element; a non-finite nq'
 * gives a zero row.  Both words must be the ones the search is given: rows made before the word grew must be made again. */
int tsim_l2_rows(const void *x, int x_dtype, int64_t rows, int d, int64_t ld_in, const float *maxnorm, void *out_f16,
                 int ld_out, float *rho_max, void *stream);
int tsim_l2_query_rows(const void *x, int x_dtype, int64_t rows, int d, int64_t ld_in, const float *maxnorm, void *out_f16,
                       int ld_out, void *stream);
/* Top-k by distance: out_scores[q, j] = float32(sum_j (q_j - c_j)^2) of the float32 rows, ASCENDING, ties to the lower index;
 * padding +inf / -1.  Canonical evaluation (restated in numpy by tests/test_l2_search_*.py): diff = (double)q_j - (double)c_j;
 * lane l adds diff * diff for j = l, l + 64, ... with the multiply and the add rounded separately (no fused multiply-add: diff^2
 * is not exact in float64); the xor butterfly 32 .. 1; one rounding to float32.  eq_aug / ec_aug: tsim_l2_query_rows /
 * tsim_l2_rows of eq_f32 / ec_f32 under ec_maxnorm, ec_rho_max the residual word of tsim_l2_rows; all four are REQUIRED, and
 * ld == tsim_pad_dim(d + 1) (else TSIM_EINVAL).  tsim_l2_topk_ex: 1 <= k <= 64; tsim_l2_topk_large: 1 <= k <= TSIM_TOPK_MAX_K
 * (below).  Workspace functions, out_status, idx_offset and stream as for the dot entries.
 * Guard (a proof, as for dot).  |q' / nq'| = 1 and |c' / S| <= 1, so the Cauchy-Schwarz argument of tsim_cosine_topk_ex gives
 * |m - (|q|^2 - dist^2) / (2 nqs)| <= eps_q = guard_eps(rho_q, rho_c, ld), rho_q measured flush-safe over the d + 1 elements of the
 * query's two rows, rho_c = *ec_rho_max.  The guard works with the query's float64 |q|^2 and nqs; 1e-13 in MFMA units and 1e-14
 * relative cover every float64 rounding (of |q|^2, nq', the definitions of the stored elements, the canonical dist^2) on the
 * safe side.
 *   Lower bound.  A row with m <= cut has (|q|^2 - dist^2) / (2 nqs) <= cut + eps_q, i.e. dist^2 >= |q|^2 - 2 nqs (cut + eps_q).
 *   The ulp.  Distances are compared after rounding to float32.  The 2^-22 term of guard_eps is in MFMA units: it does NOT cover
 *   that rounding when |q| >> A (a float32 ulp of dist^2 ~ |q|^2 is (|q| / A) 2^-24 in MFMA units).  So the k-th distance dk
 *   carries one float32 ulp: up(dk) = dk (1 + 2^-23) + 2^-149 (rounded up) lies above every real number that rounds to a float32
 *   <= dk.  The first pass stands (status 0) when the lower bound of every row outside the candidates exceeds up(dk): such a row
 *   rounds to a distance > dk and cannot enter the list, not even through a tie.
 *   Collection.  A row whose float32 distance is <= dk has dist^2 <= up(dk), hence m >= (|q|^2 - up(dk)) / (2 nqs) - eps_q > tau,
 *   tau one float below that value: every such row is collected (status 1), and the guard is repeated with the threshold that
 *   was used.  For k > 28 the block-maxima threshold B - 2 eps_q is widened by the same ulp, (nq' / A) 2^-24 in MFMA units.
 *   Brute force (status 2) takes over as for cosine, and whenever nqs or |q|^2 is not finite.
 * Known, not fixed: a corpus clustered far from the origin (radius << 0.05 |c|) puts every row inside the window, and every
 * query lands in brute force — exact but slow; centring the corpus is the remedy and is left to the caller.
 * Internally the lists hold -dist^2 (negation is exact), so sorting, merging and the tie rule are those of the other spaces;
 * the last kernel of the call flips the sign. */
/* Introspection (host only, no launch): the guard's three conversions as the kernels evaluate them, for a CPU replay of the
 * proof.  m: an MFMA score (a cut or a threshold), eps: eps_q, nqs = nq' S, qq = |q|^2, dk: a float32 k-th squared distance.
 * out[0] = up(dk); out[1] = the lower bound of dist^2 of any row with MFMA score <= m; out[2] = the real number the collection
 * threshold tau is taken one float below (-inf: no finite threshold is safe, everything is collected). */
int tsim_l2_guard_host(float m, float eps, double nqs, double qq, float dk, double out[3]);
int tsim_l2_topk_ex(const void *eq_aug, const float *eq_f32, int64_t ldq_f32, int64_t Q, const void *ec_aug,
                    const float *ec_f32, int64_t ldc_f32, const float *ec_maxnorm, const float *ec_rho_max, int64_t N,
                    int d, int ld, int k, float *out_scores, int64_t *out_idx, int32_t *out_status, int64_t idx_offset,
                    void *workspace, size_t workspace_bytes, void *stream);
int tsim_l2_topk_large(const void *eq_aug, const float *eq_f32, int64_t ldq_f32, int64_t Q, const void *ec_aug,
                       const float *ec_f32, int64_t ldc_f32, const float *ec_maxnorm, const float *ec_rho_max, int64_t N,
                       int d, int ld, int k, float *out_scores, int64_t *out_idx, int32_t *out_status, int64_t idx_offset,
                       void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Top-k for k up to TSIM_TOPK_MAX_K: the per-query `torch.topk` of /root/reference/src/pipeline/search_pipeline.py:78 and
 * hnswlib's `knn_query` (search_pipeline.py:138) take any k; retrieve-then-rerank and
 * recall@100 / recall@1000 evaluations ask for 100 to 1 000 candidates per query.
 * tsim_cosine_topk_large / tsim_dot_topk_large take the argument lists of tsim_cosine_topk_ex / tsim_dot_topk_ex and return
 * the same results (scores, order, padding, out_status, idx_offset) for 1 <= k <= TSIM_TOPK_MAX_K; else TSIM_EINVAL.
 * For k <= 64 they ARE those entries: the same kernels, the same workspace, the same bits.  For k > 64: the k-th largest of
 * >= 2k block maxima of the MFMA scores over the whole shard is a proven lower bound of the k-th best (the k > 28 argument of
 * tsim_cosine_topk_ex, which does not depend on k); every row whose MFMA score exceeds bound - 2 eps_q is collected (at most
 * the smallest power of two >= max(4k, 1 024) rows per query), re-scored exactly, sorted, and the guard of the widening pass
 * decides (status 1).  An overflowing collection, a failed guard, or a shard too small for 2k partitions goes to an exact
 * brute-force pass (status 2) that keeps its lists sorted in LDS.
 * workspace: tsim_topk_large_workspace_bytes(Q, N, k), the exact byte count the call uses (0 outside 1..TSIM_TOPK_MAX_K;
 * equal to tsim_cosine_topk_workspace_bytes for k <= 64).  It grows with Q x k; callers slice large query sets. */
#define TSIM_TOPK_MAX_K 1024
size_t tsim_topk_large_workspace_bytes(int64_t Q, int64_t N, int k);
int tsim_cosine_topk_large(const void *eq_unit, const float *eq_f32, int64_t ldq_f32, int64_t Q,
                           const void *ec_unit, const float *ec_f32, int64_t ldc_f32, const float *ec_rho_max, int64_t N,
                           int d, int ld, int k, float *out_scores, int64_t *out_idx, int32_t *out_status,
                           int64_t idx_offset, void *workspace, size_t workspace_bytes, void *stream);
int tsim_dot_topk_large(const void *eq_unit, const float *eq_f32, int64_t ldq_f32, int64_t Q, const void *ec_scaled,
                        const float *ec_f32, int64_t ldc_f32, const float *ec_maxnorm, const float *ec_rho_max, int64_t N,
                        int d, int ld, int k, float *out_scores, int64_t *out_idx, int32_t *out_status, int64_t idx_offset,
                        void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Exact range search: every corpus row whose score reaches a threshold (faiss `range_search`; what sentence-transformers'
 * paraphrase_mining / community_detection and near-duplicate removal are built on).  Operands as for tsim_cosine_topk_ex /
 * tsim_dot_topk_ex: unit (cosine) or scaled (inner product) half rows select, the float32 rows decide.  The float32 matrices
 * are REQUIRED (NULL: TSIM_EINVAL; there is no unit-rows-only mode), for dot also ec_maxnorm and ec_rho_max.
 * Definition.  Row r is a hit of query q iff s(q, r) >= tau compared in float32, s being exactly the float32 score the top-k
 * entry of the same space returns for the pair (cosine: oracle/search_ref.exact_cosine; dot: float32 of the float64 lane-ordered
 * sum).  tau is one float per call — NaN is TSIM_EINVAL, -inf returns every row (of non-NaN score), a tau above every score
 * returns nothing — or, in the _tau entries below, one float per query.  The hits of a query are ordered by (score desc, index asc).  Nothing is ever truncated: the result is the
 * complete set for any tau and any data.
 * The result size depends on the data, so the call is split where the host has to allocate:
 *   1. tsim_cosine_range_scan / tsim_dot_range_scan: threshold set-up -> ONE collect pass of the MFMA kernel over the corpus ->
 *      exact re-score, filter and sort per query -> exact counting for the queries that need it.  Writes out_counts [Q] int64
 *      (hits per query) and out_status [Q] int32 (may be NULL); its state stays in the workspace.
 *   2. the caller makes lims [Q+1] int64, the exclusive prefix sum of out_counts (lims[0] = 0, lims[Q] = T), and allocates
 *      out_scores [T] float32 and out_idx [T] int64;
 *   3. tsim_range_fill with the SAME workspace (untouched in between), float32 matrices, Q, N, d and tau writes the hits of
 *      query q to [lims[q], lims[q+1]) — the CSR layout of faiss — with out_idx = shard row + idx_offset.  A segment shorter
 *      than the scan's count is never overrun.  It may be repeated (e.g. with another idx_offset).
 * tsim_range_workspace_bytes(Q, N): the exact byte count (0 for Q <= 0 or N <= 0); it grows with Q * TSIM_RANGE_SLOT_CAP * 8 and
 * not with N; callers slice large query sets.
 * Guard (a proof, not an estimate).  eps_q = guard_eps(rho_q, rho_c, ld) bounds |m - s| for the query against EVERY row of the
 * shard, m the MFMA score (the Cauchy-Schwarz + accumulation argument of tsim_cosine_topk_ex; rho_q measured from the query's
 * two rows, rho_c = *ec_rho_max, cosine with NULL: the a-priori bound).  Cosine: a hit has s >= tau, hence m >= s - eps_q >=
 * tau - eps_q > thr_q, where thr_q is a float STRICTLY below the real number tau - eps_q (the subtraction in float64, rounded
 * to float32, stepped down until thr_q + eps_q < tau holds in float64); the collect pass appends every row with m > thr_q, so
 * no hit is left uncollected.  Dot: m approximates q.c / (nq S) with |m - s / (nq S)| <= eps_q (nq = max(|q|, 1e-8), S the
 * corpus scale); a hit has s >= tau, hence m >= tau / (nq S) - eps_q > thr_q, the float below that quotient minus eps_q minus
 * 1e-15 of its magnitude (which covers the float64 roundings of the division and the subtraction).  When no finite thr_q is
 * safe (tau = -inf, non-finite S, rows with NaN / inf that make rho 2, a zero query whose quotient leaves the float range) the
 * query is not collected at all and goes to the exact pass.  The exact re-score then removes the rows of the band
 * [tau - eps_q, tau) that were collected with the hits.
 * Status per query: 1 = answered from the collected rows; 2 = more than TSIM_RANGE_SLOT_CAP rows were collected (or no finite
 * threshold existed), or a re-scored row showed |m - s| > eps_q (operands that are not the images of the float32 rows), and
 * the query was answered by an exact pass over the float32 rows of the whole shard with the arithmetic of the top-k
 * brute-force pass: counted in the scan, written straight into the caller's segment and sorted there in the fill, so that a
 * query that hits the whole shard needs no scratch of its own.  Status 0 is not used.
 * Per-query thresholds.  tsim_cosine_range_scan_tau / tsim_dot_range_scan_tau / tsim_range_fill_tau are the three entries above
 * with `float tau` replaced by `const float *tau_q`, a device pointer to float32 [Q] (NULL: TSIM_EINVAL): query q is answered
 * exactly as by the scalar call with tau = tau_q[q] — same hits, scores, order and status rule, the same kernels reading
 * tau_q[q] where they read tau.  -inf returns every row (of non-NaN score) through the exact pass, +inf or a value above every
 * score nothing.  A NaN cannot be refused without reading the array; it is defined instead: that query has no hit and status 2
 * (no finite collect threshold exists for it, and no score compares >= NaN).  The scan and the fill of one call must be given
 * the SAME array, unchanged in between, as the scalar entries must be given the same tau.  The guard above is stated per query
 * (eps_q, thr_q) and holds with tau_q[q] in the place of tau: no step of it relates one query's threshold to another's.
 * Merging.  tsim_range_merge joins `nlists` (1 .. TSIM_RANGE_MERGE_MAX_LISTS) results of the same Q queries over DISJOINT row
 * sets, already carrying global indices (idx_offset), into one: lims_in int64 [nlists, Q+1] holds ABSOLUTE offsets into
 * scores_in / idx_in — segment q of list r is [lims_in[r][q], lims_in[r][q+1]), sorted by (score desc, index asc) as the fill
 * leaves it; the lists may lie anywhere in the two buffers (e.g. padded to a common length by an all-gather).  The caller makes
 * lims_out [Q+1], the exclusive prefix sum of the per-query totals over the lists, passes total = lims_out[Q] from the host (it
 * sized out_scores / out_idx [total] with it) and gets segment q of the output = the union of the nlists segments ordered by
 * (score desc, index asc).  Entries equal in score AND index (which disjoint shards do not produce) are ordered by list
 * number: the output is always a permutation of the input.  Segments may have any length, also 0; a whole list may be empty;
 * nlists = 1 is a copy; Q = 0 or total = 0 returns without a launch.  No workspace.  An output segment shorter than the lists'
 * total for the query is never overrun.
 * Euclidean space.  tsim_l2_range_scan / tsim_l2_range_scan_tau: every row within a SQUARED radius (faiss' L2 convention for
 * range_search).  Row r is a hit of query q iff float32(dist^2(q, r)) <= radius, dist^2 being exactly the float32 value
 * tsim_l2_topk_ex returns for the pair.  The comparison is <=, the counterpart of >= in the other spaces; faiss compares with <,
 * so a row AT the radius is a hit here and not there (pass the float32 below the radius for faiss' set).  Operands and limits
 * are those of tsim_l2_topk_ex: eq_aug / ec_aug from tsim_l2_query_rows / tsim_l2_rows, ld == tsim_pad_dim(d + 1), d <= 767,
 * ec_maxnorm and ec_rho_max REQUIRED; the argument order is that of the dot entries, the radius (one float, NaN: TSIM_EINVAL, or
 * radius_q, device float32 [Q]) in the threshold's place.  The fill is tsim_range_fill / tsim_range_fill_tau with space =
 * TSIM_SPACE_L2 and the same radius; it writes squared distances, each segment ordered by (distance asc, index asc).
 * radius < 0: no hit; 0: exactly the rows equal to the query; +inf: every row (of non-NaN distance) through the exact pass,
 * status 2; NaN in radius_q: no hit, status 2.  Status as above.
 * Guard.  A hit has float32 dist^2 <= r, so its float64 dist^2 < up(r) = l2_dist_up(r) (tsim_l2_topk_ex, "The ulp").  By
 * |m - (|q|^2 - dist^2) / (2 nqs)| <= eps_q its MFMA score is m > (|q|^2 - up(r)) / (2 nqs) - eps_q > thr_q = guard_tau_l2(r,
 * eps_q, nqs, |q|^2), the threshold the widening pass of the top-k uses with r in the place of the k-th distance: the row is
 * collected.  The re-score drops the rows of the band that came with the hits.  Internally every list holds -dist^2 (a hit is
 * -dist^2 >= -r, the same comparison); the last kernel of the fill flips the sign.
 * Known, not fixed: a corpus whose norms spread over decades, or one clustered far from the origin, puts every row inside the
 * window; such queries overflow the slot and end in status 2 — exact but slow.
 * tsim_range_merge_asc: tsim_range_merge for segments sorted by (score asc, index asc) — the squared distances of the
 * Euclidean entries; same arguments, limits and tie rule. */
#define TSIM_RANGE_SLOT_CAP 2048
#define TSIM_RANGE_MERGE_MAX_LISTS 64
#define TSIM_SPACE_COSINE 0
#define TSIM_SPACE_DOT 1
#define TSIM_SPACE_L2 2
size_t tsim_range_workspace_bytes(int64_t Q, int64_t N);
int tsim_cosine_range_scan(const void *eq_unit, const float *eq_f32, int64_t ldq_f32, int64_t Q, const void *ec_unit,
                           const float *ec_f32, int64_t ldc_f32, const float *ec_rho_max, int64_t N, int d, int ld, float tau,
                           int64_t *out_counts, int32_t *out_status, void *workspace, size_t workspace_bytes, void *stream);
int tsim_dot_range_scan(const void *eq_unit, const float *eq_f32, int64_t ldq_f32, int64_t Q, const void *ec_scaled,
                        const float *ec_f32, int64_t ldc_f32, const float *ec_maxnorm, const float *ec_rho_max, int64_t N,
                        int d, int ld, float tau, int64_t *out_counts, int32_t *out_status, void *workspace,
                        size_t workspace_bytes, void *stream);
int tsim_range_fill(int space, const float *eq_f32, int64_t ldq_f32, int64_t Q, const float *ec_f32, int64_t ldc_f32, int64_t N,
                    int d, float tau, const int64_t *lims, float *out_scores, int64_t *out_idx, int64_t idx_offset,
                    void *workspace, size_t workspace_bytes, void *stream);
int tsim_cosine_range_scan_tau(const void *eq_unit, const float *eq_f32, int64_t ldq_f32, int64_t Q, const void *ec_unit,
                               const float *ec_f32, int64_t ldc_f32, const float *ec_rho_max, int64_t N, int d, int ld,
                               const float *tau_q, int64_t *out_counts, int32_t *out_status, void *workspace,
                               size_t workspace_bytes, void *stream);
int tsim_dot_range_scan_tau(const void *eq_unit, const float *eq_f32, int64_t ldq_f32, int64_t Q, const void *ec_scaled,
                            const float *ec_f32, int64_t ldc_f32, const float *ec_maxnorm, const float *ec_rho_max, int64_t N,
                            int d, int ld, const float *tau_q, int64_t *out_counts, int32_t *out_status, void *workspace,
                            size_t workspace_bytes, void *stream);
int tsim_range_fill_tau(int space, const float *eq_f32, int64_t ldq_f32, int64_t Q, const float *ec_f32, int64_t ldc_f32,
                        int64_t N, int d, const float *tau_q, const int64_t *lims, float *out_scores, int64_t *out_idx,
                        int64_t idx_offset, void *workspace, size_t workspace_bytes, void *stream);
int tsim_range_merge(const int64_t *lims_in, const float *scores_in, const int64_t *idx_in, int nlists, int64_t Q,
                     const int64_t *lims_out, int64_t total, float *out_scores, int64_t *out_idx, void *stream);
int tsim_l2_range_scan(const void *eq_aug, const float *eq_f32, int64_t ldq_f32, int64_t Q, const void *ec_aug,
                       const float *ec_f32, int64_t ldc_f32, const float *ec_maxnorm, const float *ec_rho_max, int64_t N,
                       int d, int ld, float radius, int64_t *out_counts, int32_t *out_status, void *workspace,
                       size_t workspace_bytes, void *stream);
int tsim_l2_range_scan_tau(const void *eq_aug, const float *eq_f32, int64_t ldq_f32, int64_t Q, const void *ec_aug,
                           const float *ec_f32, int64_t ldc_f32, const float *ec_maxnorm, const float *ec_rho_max, int64_t N,
                           int d, int ld, const float *radius_q, int64_t *out_counts, int32_t *out_status, void *workspace,
                           size_t workspace_bytes, void *stream);
int tsim_range_merge_asc(const int64_t *lims_in, const float *scores_in, const int64_t *idx_in, int nlists, int64_t Q,
                         const int64_t *lims_out, int64_t total, float *out_scores, int64_t *out_idx, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Exact filtered search: the best k of each query among the rows of a LIST (hnswlib's `knn_query(filter=...)`, faiss'
 * `SearchParameters(sel=IDSelectorBatch(ids))`, and the re-scoring of someone else's candidates: a lexical first stage, the
 * senses of a lemma, the [Q, m] index output of an earlier search).  Float32 rows only: eq_f32 [Q, d], ec_f32 [N, d], row strides
 * ldq_f32 / ldc_f32 >= d elements.  No half rows, no rho, no max-norm word: nothing is selected by MFMA, every listed row is
 * scored exactly.
 * Scores are those of the top-k entries of the same space, bit for bit: tsim_cosine_list_topk the reference's cosine of the
 * float32 rows (tsim_cosine_topk_ex with float32 matrices), tsim_dot_list_topk float32(q . c) (tsim_dot_topk_ex),
 * tsim_l2_list_topk the squared distance (tsim_l2_topk_ex; -dist^2 inside, the sign flipped by the last kernel).  A list that holds
 * every row once returns what those entries return.
 * Lists.  cand [T]: row numbers, cand_dtype TSIM_I32 or TSIM_I64.  Either lims != NULL and shared == 0: int64 [Q+1], query q owns
 * cand[lims[q] .. lims[q+1]) (CSR, as tsim_range_fill writes it); or lims == NULL and shared == 1: every query owns cand[0 .. T),
 * no CSR replicated.  Both or neither: TSIM_EINVAL.  T == 0 is legal (cand may be NULL then).
 *   - a negative entry is padding and is skipped: the -1 padded [Q, m] out_idx of an earlier search can be passed as it is
 *     (lims[q] = q m);
 *   - an entry >= N is never dereferenced; it is skipped and sets TSIM_LIST_ST_ROW in out_status[q];
 *   - lims are expected non-decreasing within [0, T].  They are replaced by their running maximum clamped to [0, T] before
 *     anything reads them: a decreasing pair gives an EMPTY list, a pair pointing outside [0, T] an in-range one, and every
 *     query one of whose two words was changed gets TSIM_LIST_ST_LIMS;
 *   - lists are expected to hold distinct rows.  A row listed twice is scored twice and returned twice, in adjacent
 *     positions (equal score, equal index); callers that cannot promise distinct rows remove duplicates first (ops does).
 * Output.  out_scores [Q, k] float32, out_idx [Q, k] int64 = row + idx_offset, ordered by (score desc, row asc), Euclidean by
 * (dist^2 asc, row asc); 1 <= k <= TSIM_TOPK_MAX_K; a list with fewer than k usable entries (a row of NaN score is not usable)
 * is padded with -inf / -1 (Euclidean +inf / -1).  out_status [Q] int32 (may be NULL): 0 or the TSIM_LIST_ST_* bits.
 * Limits: 1 <= d <= 768 (Euclidean <= 767, as tsim_l2_topk_ex), N < 2^31 - 64.
 * Work.  cand is cut into slices of TSIM_LIST_SLICE entries; one workgroup scores the part of one query's list inside one slice
 * (shared lists: inside a chunk of slices) and keeps the running sorted list of the brute-force pass; one workgroup per query
 * merges.  The host never learns the list lengths: the grid and tsim_list_topk_workspace_bytes(Q, T, k) — pure host, 0 for Q <= 0,
 * T < 0 or k outside 1..TSIM_TOPK_MAX_K, non-decreasing in each argument, the same for both forms — depend on (Q, T, k) alone, and
 * no call reads device memory back.  CSR needs (Q + ceil(T / TSIM_LIST_SLICE)) k 8 B, whatever the lengths; callers slice large
 * query sets. */
#define TSIM_I32 2 /* int32 row numbers */
#define TSIM_I64 3 /* int64 row numbers */
#define TSIM_LIST_SLICE 1024
#define TSIM_LIST_ST_ROW 1  /* the list held an entry >= N */
#define TSIM_LIST_ST_LIMS 2 /* the query's lims pair was decreasing or outside [0, T] */
size_t tsim_list_topk_workspace_bytes(int64_t Q, int64_t T, int k);
int tsim_cosine_list_topk(const float *eq_f32, int64_t ldq_f32, int64_t Q, const float *ec_f32, int64_t ldc_f32, int64_t N, int d,
                          const void *cand, int cand_dtype, int64_t T, const int64_t *lims, int shared, int k, float *out_scores,
                          int64_t *out_idx, int64_t idx_offset, int32_t *out_status, void *workspace, size_t workspace_bytes,
                          void *stream);
int tsim_dot_list_topk(const float *eq_f32, int64_t ldq_f32, int64_t Q, const float *ec_f32, int64_t ldc_f32, int64_t N, int d,
                       const void *cand, int cand_dtype, int64_t T, const int64_t *lims, int shared, int k, float *out_scores,
                       int64_t *out_idx, int64_t idx_offset, int32_t *out_status, void *workspace, size_t workspace_bytes,
                       void *stream);
int tsim_l2_list_topk(const float *eq_f32, int64_t ldq_f32, int64_t Q, const float *ec_f32, int64_t ldc_f32, int64_t N, int d,
                      const void *cand, int cand_dtype, int64_t T, const int64_t *lims, int shared, int k, float *out_scores,
                      int64_t *out_idx, int64_t idx_offset, int32_t *out_status, void *workspace, size_t workspace_bytes,
                      void *stream);
/* The same search over a corpus of IEEE HALF rows: the second stage of a refine search (faiss IndexRefine(SQfp16)), whose row
 * store keeps half the bytes of the float32 rows.  space: TSIM_SPACE_COSINE / _DOT / _L2 (anything else: TSIM_EINVAL).  eq_f32
 * [Q, d] float32 as above; ec_f16 [N, d] IEEE half, row stride ldc_f16 >= d counted in ELEMENTS — any stride, odd ones included,
 * so a row need only be 2-byte aligned.  The score is the score of the float32 entry of the same space for the same query
 * against the rows widened to float32, bit for bit (the widening is exact; subnormal halves are kept, not flushed).  Lists,
 * padding, status bits, order, limits on k and d, workspace and argument errors: those of the three entries above. */
int tsim_list_topk_f16(int space, const float *eq_f32, int64_t ldq_f32, int64_t Q, const void *ec_f16, int64_t ldc_f16, int64_t N,
                       int d, const void *cand, int cand_dtype, int64_t T, const int64_t *lims, int shared, int k, float *out_scores,
                       int64_t *out_idx, int64_t idx_offset, int32_t *out_status, void *workspace, size_t workspace_bytes,
                       void *stream);

/* ---------------------------------------------------------------------------------------------
 * Community detection, the de-overlap step (sentence-transformers' `util.community_detection`, "fast clustering": every group
 * of at least min_size rows within a threshold of a centre row, largest first, no row in two groups; no cluster count is
 * needed).  The candidate communities are the segments of an exact range search of the rows against themselves (above); what
 * is left is sequential by definition and runs here on the device.
 * Input: a CSR in PRIORITY order.  lims int64 [C+1], members int32 [T]: community c lists members[lims[c] .. lims[c+1]), in the
 * order its members are to be kept.  N: the number of rows; min_size >= 1.
 * Definition.  taken = {}; for c = 0 .. C-1: free = the entries of c whose row is not in taken; if len(free) >= min_size, c is
 * accepted and its free rows join taken.  A row listed twice in one community is tested twice and counts twice.
 * Output: accept int32 [C] (1 = accepted) and keep uint8 [T] (1 iff the entry is a free entry of an ACCEPTED community, else
 * 0): the caller compacts.  status: ONE int32 word, 0 or the TSIM_COMMUNITY_ST_* bits.
 *   - a negative member is padding and is skipped;
 *   - a member >= N is never dereferenced; it is dropped (keep 0, not counted) and sets TSIM_COMMUNITY_ST_ROW;
 *   - lims are replaced by their running maximum clamped to [0, T] before anything reads them, as the list search does: a
 *     decreasing pair gives an EMPTY community (never accepted: min_size >= 1), and a changed word sets
 *     TSIM_COMMUNITY_ST_LIMS.
 * Two forms with the same results (csrc/community_select.h has the argument):
 *   tsim_community_select_rounds runs rounds first_round .. first_round + max_rounds - 1 of the parallel form: per round one
 *     claim launch (every undecided community counts its free members — fewer than min_size rejects it for good — and offers
 *     its rank to each of them with an atomic minimum) and one decide launch (a community accepts iff it won every member it
 *     claimed).  The highest-priority undecided community is decided in every round, so C rounds always suffice; a chain of L
 *     communities each sharing a row with the next needs L.  undecided int32 [max_rounds]: word r receives the number of
 *     communities still undecided after round first_round + r — the host reads it and stops at the first 0 (further rounds are
 *     harmless).  first_round == 0 initialises first: status, accept, keep and the workspace; max_rounds == 0 then only
 *     initialises.  The rounds of one de-overlap are numbered consecutively over however many calls, with the SAME arguments and
 *     workspace, untouched in between.  first_round + max_rounds <= 2^30.
 *   tsim_community_select_finish decides every community still undecided in ONE workgroup, in order, and leaves *undecided
 *     (one word) 0.  After an initialising call without rounds it is the whole de-overlap.
 * tsim_community_select_workspace_bytes(C, N): pure host, 0 for C < 0, N <= 0 or sizes beyond the limits, non-decreasing in each
 * argument: (C + 1) 8 + C 4 + N 12 bytes and alignment.  Limits: C < 2^31 - 1, N < 2^31 - 64, T < 2^40.  C == 0 and T == 0 are
 * legal (members and keep may be NULL when T == 0).  No call reads device memory back. */
#define TSIM_COMMUNITY_ST_ROW 1  /* a community listed a member >= N */
#define TSIM_COMMUNITY_ST_LIMS 2 /* a lims word was decreasing or outside [0, T] */
size_t tsim_community_select_workspace_bytes(int64_t C, int64_t N);
int tsim_community_select_rounds(const int64_t *lims, const int32_t *members, int64_t C, int64_t T, int64_t N, int min_size,
                                 int64_t first_round, int max_rounds, int32_t *accept, uint8_t *keep, int32_t *status,
                                 int32_t *undecided, void *workspace, size_t workspace_bytes, void *stream);
int tsim_community_select_finish(const int64_t *lims, const int32_t *members, int64_t C, int64_t T, int64_t N, int min_size,
                                 int32_t *accept, uint8_t *keep, int32_t *status, int32_t *undecided, void *workspace,
                                 size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * HDBSCAN (`hdbscan.HDBSCAN` / `sklearn.cluster.HDBSCAN` with metric="euclidean", cluster_selection_method="eom"): density
 * clustering without a cluster count or a threshold.  Two stages: the minimum spanning tree of the mutual-reachability graph
 * over all row pairs (O(N^2 d), on the device) and the tree stage (O(N log N), on the host).
 *
 * tsim_mst_prim: Prim's algorithm from row 0, everything in SQUARED distances.  rows_f32 [N, d] float32 on the device, rows
 * ld_rows elements apart.  d2(a, b) is the float32 value tsim_l2_topk_ex and the list entries return for the pair, bit for bit.
 * w(a, b) = max(d2(a, b), core2[a], core2[b]) with core2 float32 [N] on the device (the squared core distances: the last
 * column of the rows' exact Euclidean top-min_samples against themselves); core2 == NULL: w = d2, the plain Euclidean tree.
 *   best[j] = +inf, from[j] = -1, cur = 0, the tree = {0}.  Step t = 0 .. N-2, for every row j outside the tree: if
 *   w(cur, j) < best[j] (STRICT: the earlier endpoint keeps a tie, a NaN never updates) then best[j] = w(cur, j), from[j] = cur;
 *   next = the row outside the tree with the smallest (best[j], j) — the lower row wins a tie;
 *   out_from[t] = from[next], out_to[t] = next, out_w2[t] = best[next]; next joins the tree and becomes cur.
 * out_from, out_to int32 [N-1] and out_w2 float32 [N-1] on the device.  N == 1 writes nothing and launches nothing.  Rows are
 * expected finite; on any input the call makes exactly N - 1 steps and reads nothing outside rows_f32[0 .. N) and core2[0 .. N)
 * (if every best is +inf the lowest free row is taken with from = -1).  Two launches per step, enqueued by the host without a
 * read in between: one scores the free rows against row cur (a 64-row group inside the tree is not loaded), one reduces the
 * workgroups' minima and moves cur, a device word.  Limits: 1 <= d <= 767, ld_rows >= d, 1 <= N < 2^31 - 64, else TSIM_EINVAL
 * before any launch; a workspace below tsim_mst_prim_workspace_bytes(N) (pure host; 0 beyond the limits; 8 N bytes, 8 per 256
 * rows and alignment) is TSIM_ENOMEM.
 *
 * tsim_hdbscan_tree_labels: the tree stage with cluster_selection_method="eom", allow_single_cluster=False,
 * cluster_selection_epsilon=0, on HOST pointers (host-only code, no GPU).  from, to int32 [N-1], w2 float32 [N-1]: the edges
 * above, squared; N >= 1; min_cluster_size >= 2.  out_labels int32 [N]: the cluster of every row, -1 for noise;
 * *out_n_clusters: the cluster count.
 *   1. The edges are ordered by (w2 asc, step asc) and merged by union-find: merge k makes node N + k with the component of
 *      `from` as its left child, the component of `to` as its right child, distance sqrt((double)w2).
 *   2. Condensing, breadth-first from the root, left child before right: lambda = 1 / distance (+inf at distance 0); a child of
 *      fewer than min_cluster_size rows sheds its rows at that lambda; when both children are large enough two new clusters
 *      are numbered, left first; otherwise the larger child continues its parent's cluster.
 *   3. stability(c) = sum over the condensed rows of c, in their order, of (lambda - birth(c)) size, in float64.
 *   4. By descending cluster number, the root never selected: a cluster whose children's summed stability is strictly greater
 *      takes that sum and is unselected, otherwise its descendants are unselected.
 *   5. A row's label is the rank (ascending cluster number) of the selected cluster it fell out of or of its nearest selected
 *      ancestor; -1 without one.
 * Edges that are no spanning tree of 0 .. N-1 (an endpoint out of range, a cycle) are TSIM_EINVAL; nothing is read or written
 * out of bounds.  tests/hdbscan_cases.py restates both stages in numpy; tests/golden/hdbscan.npz pins the labels against
 * scikit-learn on separated clusters. */
size_t tsim_mst_prim_workspace_bytes(int64_t N);
int tsim_mst_prim(const float *rows_f32, int64_t ld_rows, int64_t N, int d, const float *core2, int32_t *out_from, int32_t *out_to,
                  float *out_w2, void *workspace, size_t workspace_bytes, void *stream);
int tsim_hdbscan_tree_labels(const int32_t *from, const int32_t *to, const float *w2, int64_t N, int min_cluster_size,
                             int32_t *out_labels, int32_t *out_n_clusters);

/* ---------------------------------------------------------------------------------------------
 * Binary embeddings: sign-bit codes, exact Hamming top-k and the re-score of its candidates (sentence-transformers'
 * `quantize_embeddings(precision="ubinary")` with `semantic_search_faiss(..., rescore=True)`; faiss' `IndexBinaryFlat`).
 * Codes.  A code row is the `np.packbits(x > 0, axis=1)` bytes of the float row: element 8j is bit 7 of byte j, the last byte
 * is zero-filled.  1 <= d <= 1024.  Rows lie tsim_code_bytes(d) bytes apart — ceil(d / 8) rounded up to a multiple of 16 (0 for a
 * d outside 1..1024), so every row is read with 16-byte loads — or further: ldq, ldc and ld_code are in BYTES, multiples of 16
 * and >= tsim_code_bytes(d), and the rows start on a 16-byte boundary (else TSIM_EINVAL).  The bytes from ceil(d / 8) to
 * tsim_code_bytes(d) are zero in everything the library writes; what it READS may hold anything at bit positions >= d: they
 * never count.
 * tsim_pack_sign_rows: x [rows, d] float32 (TSIM_F32) or bf16 (TSIM_BF16), row stride ld_in >= d elements -> codes, the first
 * tsim_code_bytes(d) bytes of each row.  The bit is x > 0: 0.0, -0.0, NaN, -inf and negative subnormals give 0, positive
 * subnormals and +inf 1.  HBM-bound on x.
 * tsim_hamming_topk: the k rows of c_codes [N] nearest to each row of q_codes [Q] by Hamming distance over the first d bits.
 * Exact: the true top-k, ordered by (distance asc, row asc).  out_dist [Q, k] int32, out_idx [Q, k] int64 = row + idx_offset;
 * N < k is padded with (INT32_MAX, -1) as faiss pads, N == 0 is legal (c_codes may be NULL then).  1 <= k <= TSIM_TOPK_MAX_K,
 * N < 2^31 - 64, Q <= 8 x 65535 per call.  One pass over the codes per group of min(8, ceil(Q / 4)) queries (each lane loads its
 * row once and compares it with the group's query codes, held in scalar registers), a running sorted list per (chunk of rows,
 * query), one merge workgroup per query.  workspace: tsim_hamming_topk_workspace_bytes(Q, N, k) — pure host, 0 for Q <= 0, N < 0 or k outside
 * 1..TSIM_TOPK_MAX_K, non-decreasing in each argument, never above 64 MiB + what one list per query takes.  The call reads
 * nothing back from the device.
 * tsim_sign_rescore_topk: the second stage.  Each query's candidates cand [Q, m] int64 (row numbers) are scored with the
 * float32 query eq_f32 [Q, d] (row stride ldq_f32 >= d elements) against the +-1 expansion of their codes, s_j = bit_j ? +1 : -1:
 * score = float32(sum_j q_j s_j), the sum in float64 in the canonical lane order of the exact scores above (lane l adds elements
 * l, l + 64, .., then the xor butterfly 32 .. 1; restated in oracle/search_ref._lane_sum) and rounded once — for d <= 768 the
 * bits tsim_dot_list_topk gives on the unpacked +-1 float32 matrix.  out_scores [Q, k] float32, out_idx [Q, k] int64 =
 * row + idx_offset, ordered by (score desc, row asc), short lists padded with (-inf, -1).  A negative entry of cand is padding and
 * is skipped (the out_idx of tsim_hamming_topk can be passed as it stands, idx_offset 0); an entry >= N is never dereferenced and
 * sets TSIM_LIST_ST_ROW in out_status[q] (int32 [Q], may be NULL; written, not accumulated); a row listed twice is returned
 * twice.  m >= 0, 1 <= k <= TSIM_TOPK_MAX_K.  No workspace. */
int tsim_code_bytes(int d);
int tsim_pack_sign_rows(const void *x, int x_dtype, int64_t rows, int d, int64_t ld_in, uint8_t *codes, int64_t ld_code,
                        void *stream);
size_t tsim_hamming_topk_workspace_bytes(int64_t Q, int64_t N, int k);
int tsim_hamming_topk(const uint8_t *q_codes, int64_t ldq, int64_t Q, const uint8_t *c_codes, int64_t ldc, int64_t N, int d, int k,
                      int32_t *out_dist, int64_t *out_idx, int64_t idx_offset, void *workspace, size_t workspace_bytes,
                      void *stream);
int tsim_sign_rescore_topk(const float *eq_f32, int64_t ldq_f32, int64_t Q, const uint8_t *c_codes, int64_t ldc, int64_t N, int d,
                           const int64_t *cand, int64_t m, int k, float *out_scores, int64_t *out_idx, int64_t idx_offset,
                           int32_t *out_status, void *stream);

/* ---------------------------------------------------------------------------------------------
 * int8 embeddings: calibrated scalar quantisation, exact inner-product top-k on the codes and the re-score of its candidates
 * (sentence-transformers' `quantize_embeddings(precision="int8", ranges=...)` with `semantic_search_faiss` /
 * `semantic_search_usearch(..., rescore=True)`; usearch's `Index(dtype="i8", metric="ip")`).
 * Codes.  A code row is d int8 values, 1 <= d <= 1024.  Rows lie tsim_int8_bytes(d) bytes apart — d rounded up to a multiple of 16
 * (0 for a d outside 1..1024) — or further: ldq, ldc and ld_code are in BYTES, multiples of 16 and >= tsim_int8_bytes(d), and the
 * rows start on a 16-byte boundary (else TSIM_EINVAL).  The bytes from d to tsim_int8_bytes(d) are zero in everything the library
 * writes; what it READS may hold anything there: bytes at positions >= d never count.
 * tsim_quantize_int8_rows (replaces `quantize_embeddings(x, "int8", ranges=ranges)`): x [rows, d] float32, row stride
 * ld_in >= d elements; ranges [2, d] float32 contiguous on the device, row 0 the per-column start (minimum), row 1 the maximum.
 * In float32: step = (ranges[1] - ranges[0]) / 255, t = (x - ranges[0]) / step - 128, code = trunc(t) towards zero — numpy's
 * `astype(np.int8)` wherever that is defined.  Where it is not: t saturates to [-128, 127], +-inf included, and NaN (a NaN input,
 * or 0 / 0 in a constant column) gives 0.  HBM-bound on x.
 * tsim_int8_ip_topk (replaces usearch's i8 inner-product search / faiss' IndexFlatIP over int8 rows): the k rows of c_codes [N]
 * with the largest score = sum_{j < d} q_j c_j for each row of q_codes [Q], the sum an exact int32 (|score| <= 2^24).  Exact: the
 * true top-k, ordered by (score desc, row asc).  out_score [Q, k] int32, out_idx [Q, k] int64 = row + idx_offset; N < k is padded
 * with (INT32_MIN, -1), N == 0 is legal (c_codes may be NULL then).  1 <= k <= TSIM_TOPK_MAX_K, N < 2^31 - 64, at most 65535
 * query groups per call (a group is at most 16 queries while k <= 64, else 8; fewer for a small Q).  One pass over the codes per group on
 * v_mfma_i32_16x16x64_i8 (the group's queries stay in registers as the B operand, 16 code rows at a time are loaded straight
 * into the A operand), a running sorted list per (chunk of rows, query), one merge workgroup per query.  workspace:
 * tsim_int8_ip_topk_workspace_bytes(Q, N, k) — pure host, 0 for Q <= 0, N < 0 or k outside 1..TSIM_TOPK_MAX_K, non-decreasing in
 * each argument, never above 64 MiB + what one list per query takes.  The call reads nothing back from the device.
 * tsim_int8_rescore_topk (replaces the `rescore=True` stage: float query x int8 document): the contract of
 * tsim_sign_rescore_topk with the code value in place of +-1: score = float32(sum_j q_j c_j), the sum in float64 in the canonical
 * lane order (oracle/search_ref._lane_sum) and rounded once — for d <= 768 the bits tsim_dot_list_topk gives on the codes as a
 * float32 matrix.  Ordered by (score desc, row asc), padded with (-inf, -1); negative entries of cand are skipped, an entry >= N
 * is never dereferenced and sets TSIM_LIST_ST_ROW in out_status[q] (may be NULL), a row listed twice is returned twice.
 * No workspace. */
int tsim_int8_bytes(int d);
int tsim_quantize_int8_rows(const float *x, int64_t rows, int d, int64_t ld_in, const float *ranges, int8_t *codes, int64_t ld_code,
                            void *stream);
size_t tsim_int8_ip_topk_workspace_bytes(int64_t Q, int64_t N, int k);
int tsim_int8_ip_topk(const int8_t *q_codes, int64_t ldq, int64_t Q, const int8_t *c_codes, int64_t ldc, int64_t N, int d, int k,
                      int32_t *out_score, int64_t *out_idx, int64_t idx_offset, void *workspace, size_t workspace_bytes,
                      void *stream);
int tsim_int8_rescore_topk(const float *eq_f32, int64_t ldq_f32, int64_t Q, const int8_t *c_codes, int64_t ldc, int64_t N, int d,
                           const int64_t *cand, int64_t m, int k, float *out_scores, int64_t *out_idx, int64_t idx_offset,
                           int32_t *out_status, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Product quantisation (PQ): a learned 8-bit code per sub-vector, scored against the FLOAT query by table lookups (asymmetric
 * distance computation, ADC; faiss' `IndexPQ` with nbits = 8).  The float query is never quantised.
 * Codebooks.  codebooks [M, 256, dsub] float32 contiguous on the device, dsub = d / M, finite (not checked here): 1 <= d <= 1024,
 * 1 <= M <= 64, d % M == 0 and dsub <= 64 (else TSIM_EINVAL).
 * Codes.  A code row is M bytes, byte m the centroid number of sub-vector m.  Rows lie tsim_pq_code_bytes(M) bytes apart — M rounded
 * up to a multiple of 16 (0 for an M outside 1..64) — or further: ldc and ld_code are in BYTES, multiples of 16 and
 * >= tsim_pq_code_bytes(M), and the rows start on a 16-byte boundary (else TSIM_EINVAL).  The bytes from M to tsim_pq_code_bytes(M)
 * are zero in everything the library writes; what it READS may hold anything there: they are never used as sub-quantisers.
 * tsim_pq_encode_rows: x [rows, d] float32 (TSIM_F32) or bf16 (TSIM_BF16), row stride ld_in >= d elements -> codes, the first
 * tsim_pq_code_bytes(M) bytes of each row.  Per sub-vector, dist_j in float64: dist = 0, then for i = 0 .. dsub - 1 in that order
 * t = (double)x_i - (double)c_ji, p = t t, dist = dist + p — each one rounded IEEE operation, no FMA.  The code is the first j with
 * dist_j < best, best = +inf at the start: ties go to the lower j; a sub-vector holding a NaN or an infinity gets code 0.
 * tsim_pq_tables: per query of eq_f32 [Q, d] (row stride ldq_f32 >= d) the INTEGER lookup table.  L[m][j] in float64 by the same
 * ordered, uncontracted operations: space TSIM_SPACE_DOT sum_i q_i c_ji, TSIM_SPACE_L2 -dist as above (other spaces: TSIM_EINVAL).
 * A = max |L| over the query's table; A zero, NaN or infinite: the table is all zero and e = 0.  Otherwise with A < 2^x
 * (x = ilogb(A) + 1): e = 23 - ceil(log2 M) - x and T[m][j] = (int32) rint(L[m][j] 2^e), half to even.  tables [Q, M, 256] int32
 * (16-byte aligned), exps [Q] int32 = e.  Then sum_m max_j |T[m][j]| <= 2^23 + M / 2 < 2^24.  Q == 0 is legal.
 * tsim_pq_adc_topk: score(q, r) = sum_m tables[q][m][code_r[m]], an int32 independent of the order of the additions (tables whose
 * sum_m max_j |T| exceeds 2^24 are outside the contract: the running lists carry scores as float32).  TSIM_SPACE_DOT: the top k by
 * (score desc, row asc), out_val [Q, k] int32 = score, N < k padded with (INT32_MIN, -1).  TSIM_SPACE_L2 (scores <= 0): ordered by
 * (-score asc, row asc), out_val = -score, padded with (INT32_MAX, -1).  out_idx [Q, k] int64 = row + idx_offset; N == 0 is legal
 * (c_codes may be NULL then).  The value v of query q stands for the float v 2^-exps[q].  1 <= k <= TSIM_TOPK_MAX_K, N < 2^31 - 64,
 * Q <= 65535 per call.  A workgroup serves one query and one chunk of rows: it copies the query's table into LDS (M KiB), every
 * lane loads a code row once with 16-byte loads and sums M LDS lookups; a running sorted list per (chunk of rows, query), one
 * merge workgroup per query.  workspace: tsim_pq_adc_topk_workspace_bytes(Q, N, M, k) — pure host, 0 for Q <= 0, N < 0, M outside 1..64
 * or k outside 1..TSIM_TOPK_MAX_K, non-decreasing in Q, N and k, never above 64 MiB + what one list per query takes; it does not
 * hold the tables, which are the caller's (Q M KiB: callers slice large query sets).  The call reads nothing back from the device. */
int tsim_pq_code_bytes(int M);
int tsim_pq_encode_rows(const void *x, int x_dtype, int64_t rows, int d, int64_t ld_in, const float *codebooks, int M, uint8_t *codes,
                        int64_t ld_code, void *stream);
int tsim_pq_tables(int space, const float *eq_f32, int64_t ldq_f32, int64_t Q, const float *codebooks, int d, int M, int32_t *tables,
                   int32_t *exps, void *stream);
size_t tsim_pq_adc_topk_workspace_bytes(int64_t Q, int64_t N, int M, int k);
int tsim_pq_adc_topk(int space, const int32_t *tables, int64_t Q, const uint8_t *c_codes, int64_t ldc, int64_t N, int M, int k,
                     int32_t *out_val, int64_t *out_idx, int64_t idx_offset, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Inverted-file (IVF) scan: the best k of each query among the rows of the LISTS it probes (faiss' `IndexIVFFlat` after its coarse
 * quantiser; what makes one query cheaper than a pass over the corpus).  rows_f32 [N, d] float32, row stride ld_rows >= d, holds
 * the rows in LIST order: list l is rows [list_off[l], list_off[l+1]), list_off int64 [nlist+1].  row_ids int32 [N] gives, for each
 * POSITION, the id that is reported and ranked by.  probes int64 [Q, nprobe] contiguous: the list numbers of each query, e.g. the
 * out_idx of a top-k call of the queries against the nlist centroids, as it stands.  eq_f32 [Q, d], row stride ldq_f32 >= d.
 * Scores are those of the list entries above, bit for bit (space: TSIM_SPACE_COSINE / _DOT / _L2, the last through -dist^2 inside, the
 * sign flipped by the last kernel).  out_scores [Q, k] float32, out_idx [Q, k] int64 = id + idx_offset, ordered by (score desc, ID
 * asc), Euclidean by (dist^2 asc, id asc) — equal rows in different lists rank as in a search of all rows; fewer than k usable rows
 * pad with -inf / -1 (Euclidean +inf / -1).  1 <= k <= TSIM_TOPK_MAX_K, 1 <= d <= 768 (Euclidean <= 767), N < 2^31 - 64,
 * Q nprobe < 2^31 - 1, nprobe >= 1.
 *   - a negative probes entry is padding and is skipped;
 *   - a probes entry >= nlist is never dereferenced; it is skipped and sets TSIM_IVF_ST_LIST in out_status[q];
 *   - a list probed twice by one query is scanned twice and its rows are returned twice, in adjacent positions, as a row listed
 *     twice is in the list entries;
 *   - a negative row_ids entry is a tombstone: the row is loaded and scored and the score dropped;
 *   - an empty list is legal;
 *   - list_off is expected non-decreasing within [0, N].  Otherwise every word counts as the running maximum of the words up to it,
 *     clamped to [0, N] (the rule of the list entries' lims): a decreasing pair gives an EMPTY list, and every query that probed a
 *     list one of whose two words was changed gets TSIM_IVF_ST_OFF.  Nothing outside rows_f32[0 .. N) and row_ids[0 .. N) is read;
 *   - out_status [Q] int32 (may be NULL): 0 or the TSIM_IVF_ST_* bits; written, not accumulated.
 * Work.  A list is cut into segments of TSIM_IVF_SEG rows; the workgroups of a (query, probe) pair take its segments in turn, each
 * keeping the running sorted list of the brute-force pass; one workgroup per query merges.  max_list_len is a SIZING HINT only (the
 * length of the longest list, which the caller knows on the host): it sets the grid and the slots per pair — enough for a single
 * query with a few tens of probes to reach every CU — and a longer list is still scanned completely; the result never depends on
 * it.  workspace: tsim_ivf_scan_workspace_bytes(Q, nprobe, max_list_len, k) — pure host, 0 for Q <= 0, nprobe <= 0, max_list_len < 0 or
 * k outside 1..TSIM_TOPK_MAX_K, non-decreasing in each argument, never above 64 MiB + what one list per (query, probe) takes; callers
 * slice large query sets.  The call reads nothing back from the device. */
#define TSIM_IVF_SEG 512
#define TSIM_IVF_ST_LIST 1 /* probes held an entry >= nlist */
#define TSIM_IVF_ST_OFF 2  /* a probed list's list_off pair was decreasing or outside [0, N] */
size_t tsim_ivf_scan_workspace_bytes(int64_t Q, int nprobe, int64_t max_list_len, int k);
int tsim_ivf_scan_topk(int space, const float *eq_f32, int64_t ldq_f32, int64_t Q, const float *rows_f32, int64_t ld_rows, int64_t N,
                       int d, const int64_t *list_off, int64_t nlist, const int32_t *row_ids, const int64_t *probes, int nprobe,
                       int64_t max_list_len, int k, float *out_scores, int64_t *out_idx, int64_t idx_offset, int32_t *out_status,
                       void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * IVF-PQ: PQ codes in inverted lists, by default of each row's RESIDUAL to its list centroid (faiss' `IndexIVFPQ` with 8-bit
 * codes).  (d, M) and codebooks as for tsim_pq_*; centroids [nlist, d] float32, row stride ld_cent >= d, finite (not checked);
 * list_off, row_ids and probes as for tsim_ivf_scan_topk, the code rows in list order, ldc >= tsim_pq_code_bytes(M) bytes apart.
 * A probes entry < 0 or >= nlist is padding: its table is not written and never read.
 * Encoding.  A row x of list l has the code tsim_pq_encode_rows gives r, r_i = float32(x_i - c_l,i) (one rounded subtraction),
 * or x itself when the index does not code residuals; then tsim_pq_tables (one table a query, no bias) serves the scan.
 * tsim_ivfpq_tables, the tables of residual codes:
 *   TSIM_SPACE_DOT: tables [Q, M, 256] with L as tsim_pq_tables, and bias [Q, nprobe]: B[j] = sum_{i < d} (double)q_i
 *     (double)c_{l_j},i in that order, no FMA.  A = max(max |L|, max over valid probes |B|), x = ilogb(A) + 1,
 *     e = 23 - ceil(log2(M + 1)) - x, T = rint(L 2^e), bias = rint(B 2^e), half to even; the bias of a padding probe is 0.
 *   TSIM_SPACE_L2: tables [Q nprobe, M, 256], one per (query, probe) pair: L_p[m][j] = -dist(rq_m, c_mj) with
 *     rq_i = float32(q_i - c_l,i); A = max |L_p| over all valid pairs of the QUERY (one exponent a query),
 *     e = 23 - ceil(log2 M) - x.  bias may be NULL; when given it is zeroed.
 *   A query with a NaN or an infinity among these entries, or with A == 0, gets zero tables, zero biases and e = 0.  exps [Q].
 *   workspace: tsim_ivfpq_tables_workspace_bytes(Q, nprobe) (0 for Q <= 0, nprobe < 1 or Q nprobe >= 2^31 - 1; needed by
 *   TSIM_SPACE_L2 only).  Q == 0 is legal.
 * tsim_ivfpq_scan_topk: score(q, r in probe j) = bias[q nprobe + j] (0 when bias is NULL) + sum_m T[m][code_r[m]], T the table of
 *   pair q nprobe + j (tables_per_pair != 0) or of query q.  |bias| + sum_m max_j |T| must stay below 2^24.  The exact top k over
 *   the rows of the probed lists: TSIM_SPACE_DOT by (score desc, id asc), out_val = score, padded (INT32_MIN, -1); TSIM_SPACE_L2 by
 *   (-score asc, id asc), out_val = -score, padded (INT32_MAX, -1); out_idx = row_ids value + idx_offset.  A negative row_ids entry
 *   is a tombstone (loaded, scored, dropped); list_off and out_status (TSIM_IVF_ST_*) behave as in tsim_ivf_scan_topk, and so does
 *   the hint max_list_len, with segments of TSIM_IVFPQ_SEG rows.  workspace: tsim_ivfpq_scan_workspace_bytes(Q, nprobe,
 *   max_list_len, k), 0 for bad arguments, non-decreasing in each.  The calls read nothing back from the device. */
#ifndef TSIM_IVFPQ_SEG /* (a variant build may set another multiple of 256 to measure it: tools/bench_ivfpq.py --scan-only) */
#define TSIM_IVFPQ_SEG 4096
#endif
size_t tsim_ivfpq_tables_workspace_bytes(int64_t Q, int nprobe);
int tsim_ivfpq_tables(int space, const float *eq_f32, int64_t ldq_f32, int64_t Q, const float *centroids, int64_t ld_cent,
                      int64_t nlist, const int64_t *probes, int nprobe, const float *codebooks, int d, int M, int32_t *tables,
                      int32_t *bias, int32_t *exps, void *workspace, size_t workspace_bytes, void *stream);
size_t tsim_ivfpq_scan_workspace_bytes(int64_t Q, int nprobe, int64_t max_list_len, int k);
int tsim_ivfpq_scan_topk(int space, const int32_t *tables, int tables_per_pair, const int32_t *bias, int64_t Q,
                         const uint8_t *c_codes, int64_t ldc, int64_t N, int M, const int64_t *list_off, int64_t nlist,
                         const int32_t *row_ids, const int64_t *probes, int nprobe, int64_t max_list_len, int k, int32_t *out_val,
                         int64_t *out_idx, int64_t idx_offset, int32_t *out_status, void *workspace, size_t workspace_bytes,
                         void *stream);

/* ---------------------------------------------------------------------------------------------
 * Graph index: beam search over a fixed-degree proximity graph (the family of hnswlib's base layer and of CAGRA), and the
 * rank-based pruning that makes such a graph out of an exact kNN graph.
 * tsim_graph_search.  rows_f32 [N, d] float32 (row stride ld_rows >= d), eq_f32 [Q, d] (ldq_f32 >= d), space and scores as for the
 * list entries above, bit for bit.  graph int32 [N, R] contiguous, 1 <= R <= TSIM_GRAPH_MAX_DEGREE: row r's neighbours.  entries int32
 * [n_entries], 1 <= n_entries <= TSIM_GRAPH_MAX_ENTRIES: the rows every query starts from.  In both, a negative id is padding and an
 * id >= N is never dereferenced and sets TSIM_GRAPH_ST_ROW in out_status[q].  row_ids int32 [N] (may be NULL): a negative entry marks
 * the row a tombstone.  k <= ef <= TSIM_GRAPH_MAX_EF, 1 <= width <= TSIM_GRAPH_MAX_WIDTH, max_iters >= 1, 1 <= d <= 768 (Euclidean
 * <= 767), N < 2^31 - 64.  Per query:
 *   1. visited = {}; the beam is empty, holds at most ef (score, row) entries and is ordered by (score desc, row asc), Euclidean by
 *      (dist^2 asc, row asc);
 *   2. every distinct usable entry point joins visited, is scored and offered to the beam;
 *   3. at most max_iters times: the parents are the best `width` beam entries not yet expanded, chosen at the start of the iteration
 *      (none: stop); they are marked expanded; every neighbour graph[parent][0 .. R) of every parent that is usable and not in
 *      visited joins visited and is scored — a NaN score is dropped, the row stays visited; the beam becomes the best ef of (beam +
 *      the rows just scored); a row pushed out of the beam stays visited;
 *   4. if the cap ended the loop while an unexpanded entry was left, TSIM_GRAPH_ST_ITERS is set;
 *   5. the first k beam entries that are no tombstones are the result (tombstones are traversed and route the search; they are never
 *      returned): out_scores [Q, k], out_idx [Q, k] = row_ids[row] when row_ids is given, else row + idx_offset; fewer than k pad
 *      with -inf / -1 (Euclidean +inf / -1).
 * The beam's rows are distinct and its order total, so the result is a function of the arguments alone.  visited is exact: an
 * open-addressing table in LDS of the smallest power of two >= 2 (n_entries + max_iters width R) slots, the most rows a query can
 * visit, and at least 64.  The table may take TSIM_GRAPH_MAX_TABLE_BYTES (16 384 visits); a call that needs more is TSIM_EINVAL
 * with a message.  It is sized per call: a small max_iters leaves LDS for several workgroups a CU.
 * tsim_graph_search_lds_bytes: the LDS of one workgroup of such a call (TSIM_GRAPH_STATIC_LDS_BYTES for the beam and the staging + the
 * table), pure host, 0 for arguments outside the ranges above, non-decreasing in each argument; the call is accepted iff it is
 * <= TSIM_GRAPH_STATIC_LDS_BYTES + TSIM_GRAPH_MAX_TABLE_BYTES.  out_status [Q] int32 (may be NULL): written, not accumulated.
 * One workgroup per query; no workspace; the call reads nothing back from the device.
 * tsim_graph_search_seeded.  The same search with entry points per QUERY, given in two levels: step 2 takes, for query q, the rows
 * seeds[probes[q][p]][s] for all p < n_probe, s < n_seeds — 1 <= n_probe n_seeds <= TSIM_GRAPH_MAX_ENTRIES of them (n_entries of
 * the table sizing above) — and every other step is tsim_graph_search's.  seeds int32 [n_lists, n_seeds] contiguous (may be NULL):
 * row l holds the rows a search entering through list l starts from.  seeds == NULL: n_lists and n_seeds are ignored, n_seeds = 1,
 * n_lists = N and a probe IS a row — the plain entries [Q, E] form.  probes int32 [Q, n_probe] (row stride ld_probes >= n_probe; may be
 * NULL): the lists of each query.  The id rule holds at both levels: a negative probe or seed is padding, a probe >= n_lists or a
 * seed >= N is never dereferenced and sets TSIM_GRAPH_ST_ROW; repeats are harmless (visited dedupes them).  Exactly one of probes
 * and centroids is given.  probes == NULL: centroids float32 [n_lists, d] (row stride ld_centroids >= d), 1 <= n_lists <=
 * TSIM_GRAPH_MAX_COARSE_LISTS, and the kernel finds the probes first: the n_probe centroids of best score to the query in the
 * index's space — the scores of the list entries above, bit for bit — ordered by (score desc, list asc), a NaN score dropped, -1
 * where fewer are usable.  out_probes int32 [Q, n_probe] contiguous (may be NULL): the probes the query used, given or found.
 * tsim_graph_prune.  knn int32 [N, K0] contiguous, 1 <= K0 <= TSIM_GRAPH_PRUNE_MAX_K0: each row's nearest other rows, best first
 * (entries < 0 or >= N are unusable).  D[i][b] = #{a < b : knn[i][a] usable and knn[i][b] among knn[knn[i][a]][0 .. b)} — the number
 * of two-hop detours through a better-ranked neighbour — and D[i][b] = K0 for an unusable knn[i][b].  out_forward int32 [N, R],
 * 1 <= R <= min(K0, TSIM_GRAPH_MAX_DEGREE): the R entries of knn[i] of smallest (D, b), in that order, unusable ones as -1.
 * out_detours int32 [N, K0] (may be NULL): D. */
#define TSIM_GRAPH_MAX_DEGREE 64
#define TSIM_GRAPH_MAX_ENTRIES 256
#define TSIM_GRAPH_MAX_WIDTH 4
#define TSIM_GRAPH_MAX_EF 1024
#define TSIM_GRAPH_MAX_TABLE_BYTES 131072
#define TSIM_GRAPH_STATIC_LDS_BYTES 18432
#define TSIM_GRAPH_PRUNE_MAX_K0 128
#define TSIM_GRAPH_MAX_COARSE_LISTS 4096 /* centroids the seeded search's own coarse phase takes */
#define TSIM_GRAPH_ST_ROW 1   /* the graph, the entry points or the seeds held an id >= N, or the probes one >= n_lists, that the query met */
#define TSIM_GRAPH_ST_ITERS 2 /* max_iters ended the search with an unexpanded beam entry left */
size_t tsim_graph_search_lds_bytes(int n_entries, int R, int width, int max_iters);
int tsim_graph_search(int space, const float *eq_f32, int64_t ldq_f32, int64_t Q, const float *rows_f32, int64_t ld_rows, int64_t N,
                      int d, const int32_t *graph, int R, const int32_t *entries, int n_entries, const int32_t *row_ids, int ef,
                      int width, int max_iters, int k, float *out_scores, int64_t *out_idx, int64_t idx_offset, int32_t *out_status,
                      void *stream);
int tsim_graph_search_seeded(int space, const float *eq_f32, int64_t ldq_f32, int64_t Q, const float *rows_f32, int64_t ld_rows,
                             int64_t N, int d, const int32_t *graph, int R, const int32_t *seeds, int64_t n_lists, int n_seeds,
                             const int32_t *probes, int64_t ld_probes, int n_probe, const float *centroids, int64_t ld_centroids,
                             const int32_t *row_ids, int ef, int width, int max_iters, int k, float *out_scores, int64_t *out_idx,
                             int64_t idx_offset, int32_t *out_status, int32_t *out_probes, void *stream);
int tsim_graph_prune(const int32_t *knn, int64_t N, int K0, int R, int32_t *out_forward, int32_t *out_detours, void *stream);

/* Measurement hook (bench.py): the NEXT tsim_cosine_topk call of the calling thread records `start` right before
 * and `stop` right after the launch of its dominant kernel (cos_topk_partial) on the call's stream.  Both are
 * hipEvent_t handles passed as void*; the hook is cleared by that call.  Pass NULLs to cancel. */
void tsim_time_next_topk(void *start_event, void *stop_event);

/* Merge `nlists` sorted candidate lists per query (the per-shard results of tsim_cosine_topk on the
 * shards of a partitioned corpus, or the per-chunk results of search_pipeline.py:60 `corpus_chunk_size`
 * chunking): scores/idx are [nlists, Q, k_in]; output [Q, k_out] by (score desc, index asc);
 * entries with idx < 0 are ignored, an entry equal in (score, index) to the one before it is emitted once, unused slots are
 * (-inf, -1).  64 < k_out <= TSIM_TOPK_MAX_K runs a sort-and-merge kernel with the same output. */
int tsim_topk_merge(const float *scores, const int64_t *idx, int nlists, int64_t Q, int k_in,
                    int k_out, float *out_scores, int64_t *out_idx, void *stream);
/* The same with the lists `list_stride_scores` / `list_stride_idx` ELEMENTS apart (>= Q * k_in): merges the per-rank
 * [scores | indices] buffers of an all-gather in place, without re-stacking them (distributed/sharded_search.py). */
int tsim_topk_merge_strided(const float *scores, const int64_t *idx, int nlists, int64_t Q, int k_in, int k_out,
                            int64_t list_stride_scores, int64_t list_stride_idx, float *out_scores,
                            int64_t *out_idx, void *stream);

/* ---------------------------------------------------------------------------------------------
 * A8  cos_sim(a, b)   /root/reference/src/utils/metrics.py:81-101
 * out[i, j] = <a_i/||a_i||, b_j/||b_j||> in float32, dense [Na, Nb]; no eps (a zero row gives NaN,
 * as in the reference).  For evaluation-sized inputs; the search path never materialises this. */
int tsim_cos_sim(const float *a, int64_t na, const float *b, int64_t nb, int d, float *out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * A4  AvgPoolingStrategy.forward   /root/reference/src/modules/modules.py:158-171
 *     (== OnnxSentenceTransformerWrapper.forward, src/models/sentence_encoder.py:35-38)
 * out[b, :] = sum_s hidden[b, s, :] * mask[b, s] / max(sum_s mask[b, s], 1e-9); hidden is float32 or bf16
 * [B, S, H] contiguous, mask int32 [B, S]; out float32 [B, H]. */
int tsim_mean_pool(const void *hidden, int hidden_dtype, const int32_t *mask, int64_t B, int S, int H,
                   float *out, void *stream);

/* The pooling strategies of /root/reference/src/modules/modules.py:154-195 on the padded layout (mode: TSIM_POOL_*, see
 * tsim_encoder_forward_head).  Mask entries weight the sums (MEAN, MEAN_SQRT_LEN); for CLS and MAX a token is in when its
 * mask entry is non-zero, and CLS takes the first such token.  mode MEAN == tsim_mean_pool bit for bit. */
int tsim_pool(const void *hidden, int hidden_dtype, const int32_t *mask, int64_t B, int S, int H, int mode,
              float *out, void *stream);
/* Dense + Normalize of sentence-transformers on float32 rows x [B, d_in]: out [B, d_out] = act(w x + b), then
 * x / max(|x|, 1e-12) when normalize (tsim_encoder_forward_head gives the arithmetic).  w == NULL: no projection
 * (d_out == d_in; act and Normalize only).  b may be NULL.  x, w and out 16-byte aligned. */
int tsim_dense_rows(const float *x, int64_t B, int d_in, const float *w, const float *b, int d_out, int act,
                    int normalize, float *out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * A3  context_embedder(**features)[0]  — the HF AutoModel forward the reference calls at
 *     /root/reference/src/models/sentence_encoder.py:33,107-108,118 (layer arithmetic:
 *     src/models/bert_of_theseus.py:185-211, 244-336, 346-350, 411-414, 424-428), followed by A4.
 */
typedef struct tsim_encoder tsim_encoder;

/* Projection operand formats.  TSIM_W_MXFP8: weights AND the activations entering each projection are OCP MXFP8
 * (e4m3 elements, one E8M0 power-of-two scale per 32 consecutive elements of the contraction axis), multiplied by
 * v_mfma_scale_f32_32x32x64_f8f6f4 (twice the bf16 MFMA rate); needs hidden % 256 == 0 and ffn % 256 == 0.
 * The reference has no fp8 path (HF fp32 forward, src/models/sentence_encoder.py:33): this is north_star's config 5. */
#define TSIM_W_BF16 0
#define TSIM_W_MXFP8 1

/* bf16 [rows, K] (device) -> MXFP8: q_out uint8 [rows, K] e4m3 bytes, scale_out uint8 [rows, K/32] E8M0 bytes.
 * K % 32 == 0.  Bit-exact restatement: oracle/fp8_ref.mx_quantize. */
int tsim_quantize_mxfp8(const void *x_bf16, int64_t rows, int K, void *q_out, void *scale_out, void *stream);

/* out_f32 [M, N] = dequant(xq, xs) [M, K] @ dequant(wq, ws) [N, K]^T + bias  on the block-scaled fp8 MFMA (the projection
 * kernel of the MXFP8 encoder, exposed for parity tests).  N % 256 == 0, K % 128 == 0, K >= 256; xq, xs and out_f32 must be
 * allocated for M rounded up to a multiple of 256 rows (the kernel works on whole 256-row tiles). */
int tsim_gemm_mxfp8(const void *xq, const void *xs, const void *wq, const void *ws, const float *bias, float *out_f32,
                    int M, int N, int K, void *stream);

typedef struct tsim_encoder_config {
    int32_t arch;          /* TSIM_ARCH_BERT | TSIM_ARCH_MPNET | TSIM_ARCH_ROBERTA */
    int32_t num_layers, hidden, heads, ffn, vocab, max_pos;
    int32_t pad_id;        /* MPNet, RoBERTa: position ids skip tokens equal to pad_id */
    int32_t rel_buckets;   /* MPNet relative-position buckets (32) */
    float ln_eps;
    int32_t max_tokens;    /* capacity of the activation workspace, in packed tokens per call */
    int32_t max_seqs;      /* capacity in sequences per call */
    int32_t weight_dtype;  /* TSIM_W_BF16 | TSIM_W_MXFP8 (projection operands; BASELINE.json configs[4]) */
} tsim_encoder_config;

/* Per-layer weights, all HOST pointers to float32 in torch nn.Linear layout [out, in]; the engine
 * converts to bf16 and uploads.  rel_bias_host is [rel_buckets, heads] or NULL for BERT. */
typedef struct tsim_layer_weights_host {
    const float *wq, *bq, *wk, *bk, *wv, *bv, *wo, *bo, *ln1_g, *ln1_b;
    const float *w1, *b1, *w2, *b2, *ln2_g, *ln2_b;
} tsim_layer_weights_host;

typedef struct tsim_encoder_weights_host {
    const float *word_emb, *pos_emb, *type_emb /* row 0 (tsim_encoder_set_token_types: all rows); NULL for MPNet and DistilBERT */,
        *emb_ln_g, *emb_ln_b;
    const float *rel_bias;
    const tsim_layer_weights_host *layers;
} tsim_encoder_weights_host;

/* Accepted shapes (anything else: TSIM_EUNSUPPORTED / TSIM_EINVAL with a message that names the accepted values, before any
 * launch): hidden 64, 384, 768 or 1024; heads with hidden / heads = 16, 32 or 64 (any count, a multiple of 4 or not);
 * ffn a multiple of 64, and at least 128 unless hidden is 64; TSIM_W_MXFP8 with hidden and ffn multiples of 256.  DESIGN.md
 * "Encoder routes by configuration" names the kernel and the test of every class of these; tsim_encoder_route_host (below)
 * answers the same question without a GPU. */
int tsim_encoder_create(const tsim_encoder_config *cfg, const tsim_encoder_weights_host *w,
                        tsim_encoder **out);
void tsim_encoder_destroy(tsim_encoder *enc);

/* Forward on PACKED tokens (no padding work): token t of sequence b lives at cu_seqlens[b] <= t <
 * cu_seqlens[b+1]; tok_ids/tok_pos int32 [T] (tok_pos = position-embedding row, tok_col = column of the
 * token in the padded batch, used for MPNet's relative bias; pass tok_col = NULL to use tok_pos).
 * max_len = the longest sequence of the batch (sizes the attention grid); max_len (+ pad_id + 1 for MPNet and RoBERTa, whose
 * position rows start there) must not exceed max_pos, else TSIM_EINVAL.
 * Outputs (either may be NULL): pooled_f32 [B, hidden] = masked mean-pool (A4), un-normalised like the
 * reference's encode_text; unit_f16 [B, ld_unit] = L2-normalised half rows ready for tsim_cosine_topk, with
 * unit_rho_max (device float, may be NULL) raised to their largest rounding residual exactly as tsim_l2norm_rows does;
 * last_hidden_bf16 [T, hidden] = the final hidden states of the packed tokens (token embeddings; tests read them too). */
int tsim_encoder_forward(tsim_encoder *enc, const int32_t *tok_ids, const int32_t *tok_pos,
                         const int32_t *tok_col, const int32_t *cu_seqlens, int32_t T, int32_t B,
                         int32_t max_len, float *pooled_f32, void *unit_f16, int ld_unit, float *unit_rho_max,
                         void *last_hidden_bf16, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Cross-encoder re-ranking: `cross_encoder.predict([[query, text], ...])`   /root/reference/src/pipeline/ranking_pipeline.py:27-33
 * (the reference takes a sentence_transformers CrossEncoder, i.e. HF BertForSequenceClassification on
 * `[CLS] a [SEP] b [SEP]` with token types 0 / 1).  BERT only.
 *
 * BERT only (TSIM_EINVAL for MPNet): upload all n_types rows of the token-type table [n_types, hidden] (HF
 * embeddings.token_type_embeddings).  Untyped forwards keep adding row 0 of it. */
int tsim_encoder_set_token_types(tsim_encoder *enc, const float *type_emb_host, int32_t n_types);
/* Sequence-classification head, float32 host arrays in nn.Linear layout: pool_w [H,H], pool_b [H] (HF bert.pooler.dense),
 * cls_w [num_labels,H], cls_b [num_labels] (HF classifier); 1 <= num_labels <= 32.  BERT only (TSIM_EINVAL for MPNet).
 * logits[b] = cls_w . tanh(pool_w . h[CLS of b] + pool_b) + cls_b, with h the final bf16 hidden state read in place; every sum
 * in float32 in an order fixed by H alone (rows are batch-composition invariant bit for bit).  A zero-length sequence
 * reads a zero CLS row. */
int tsim_encoder_set_cls_head(tsim_encoder *enc, const float *pool_w_host, const float *pool_b_host,
                              const float *cls_w_host, const float *cls_b_host, int32_t num_labels);
/* The same head with the activation between its two layers chosen: act = TSIM_ACT_TANH (tsim_encoder_set_cls_head; also HF
 * RobertaClassificationHead: classifier.dense, tanh, classifier.out_proj) or TSIM_ACT_RELU (HF
 * DistilBertForSequenceClassification: pre_classifier, ReLU, classifier).  hidden <= 1024. */
int tsim_encoder_set_cls_head_act(tsim_encoder *enc, const float *pool_w_host, const float *pool_b_host,
                                  const float *cls_w_host, const float *cls_b_host, int32_t num_labels, int32_t act);
/* tsim_encoder_forward plus tok_type int32 [T] (token-type row of each token; NULL = all 0, bit-identical to
 * tsim_encoder_forward) and logits_f32 [B, num_labels] (NULL = no head).  logits_f32 without a head, or tok_type without a
 * type table: TSIM_EINVAL.  A type id outside [0, n_types) is clamped and raises TSIM_ENC_ERR_TOKEN_TYPE. */
int tsim_encoder_forward_ex(tsim_encoder *enc, const int32_t *tok_ids, const int32_t *tok_type, const int32_t *tok_pos,
                            const int32_t *tok_col, const int32_t *cu_seqlens, int32_t T, int32_t B, int32_t max_len,
                            float *pooled_f32, void *unit_f16, int ld_unit, float *unit_rho_max,
                            void *last_hidden_bf16, float *logits_f32, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Sentence-embedding heads: the pooling strategies of /root/reference/src/modules/modules.py:154-195
 * (AvgPoolingStrategy, CLSPoolingStrategy, BertPoolingStrategy = tanh(Linear(CLS row))) and the sentence-transformers
 * module chain a checkpoint directory declares in modules.json (Pooling -> optional Dense -> optional Normalize), which the
 * reference reaches through its --pooling switch (src/training/train_sts.py:41-44) and HF checkpoints.
 * Pooling modes (rows of one sequence, float32 sums over the tokens in ascending order):
 *   MEAN           sum / max(len, 1e-9)            (A4; the default forward)
 *   CLS            the first token's row            (the reference's `embeddings[:0:]` is an empty slice; its evident
 *                                                    meaning, `embeddings[:, 0]`, is what runs)
 *   MAX            elementwise max over the tokens
 *   MEAN_SQRT_LEN  sum / sqrt(max(len, 1e-9))
 * A zero-length sequence pools to a zero row in every mode (sentence-transformers' max would give -1e9 there; tokenised
 * text always carries special tokens, so the case does not come from text).
 * Dense:     out[b] = act(W x[b] + bias), W [d_out, d_in] in nn.Linear layout, float32; every output element is one fmaf
 *            chain over the d_in products in an order fixed by d_in alone, so rows are batch-composition invariant bit
 *            for bit.  8 <= d_in, d_out <= 1024, both multiples of 8.
 * Normalize: sentence-transformers' F.normalize(x, dim=1) = x / max(|x|_2, 1e-12), evaluated as tsim_l2norm_rows does
 *            (float64 sum of squares in its canonical order, float64 scale) and rounded once to float32. */
#define TSIM_POOL_MEAN 0
#define TSIM_POOL_CLS 1
#define TSIM_POOL_MAX 2
#define TSIM_POOL_MEAN_SQRT_LEN 3
#define TSIM_ACT_IDENTITY 0
#define TSIM_ACT_TANH 1
#define TSIM_ACT_RELU 2 /* classification heads only (tsim_encoder_set_cls_head_act); a Dense refuses it */
typedef struct tsim_sentence_head {
    int32_t pool_mode;               /* TSIM_POOL_* */
    int32_t d_out;                   /* 0 = no Dense */
    const float *dense_w, *dense_b;  /* DEVICE, caller-owned: [d_out, hidden], [d_out] or NULL (no bias) */
    int32_t dense_act;               /* TSIM_ACT_* */
    int32_t normalize;               /* 0 / 1 */
} tsim_sentence_head;

/* tsim_encoder_forward_ex without logits, plus a head.  emb_f32 [B, d_out ? d_out : hidden] = the final rows (may be NULL);
 * unit_f16 [B, ld_unit] = exactly tsim_l2norm_rows(final rows, eps 1e-8) with unit_rho_max raised as it does (final width
 * <= 768).  The head is fused into the kernel that writes the final rows: the pooling kernel without a Dense, the Dense
 * kernel otherwise; the pre-Dense rows live in encoder scratch (no allocation).  head == NULL: bit-identical to
 * tsim_encoder_forward_ex with emb_f32 as pooled_f32.  Bad head: TSIM_EINVAL. */
int tsim_encoder_forward_head(tsim_encoder *enc, const int32_t *tok_ids, const int32_t *tok_type, const int32_t *tok_pos,
                              const int32_t *tok_col, const int32_t *cu_seqlens, int32_t T, int32_t B, int32_t max_len,
                              const tsim_sentence_head *head, float *emb_f32, void *unit_f16, int ld_unit,
                              float *unit_rho_max, void *last_hidden_bf16, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Word-in-context embeddings: WordEncoderModel.encode  /root/reference/src/models/word_encoder.py:46-50 with
 * WordPoolingStrategy.forward  /root/reference/src/modules/modules.py:68-74, and GWSCModel's
 * `torch.mean(embedded_1[i][w1_c1], dim=0)`  word_encoder.py:85-92 — the mean of the final hidden states over the token
 * positions of a target word — on the device, behind the unchanged packed forward.
 * Arguments: those of tsim_encoder_forward_ex (same meaning, same optional outputs: one call can return sentence and word
 * embeddings), then the span table in CSR form and the span outputs:
 *   span_seq [S] int32       the sequence (0 .. B-1) span s belongs to;
 *   span_cu  [S+1] int32     span s lists span_tok[span_cu[s] .. span_cu[s+1]);
 *   span_tok [n_span_tok] int32   token positions inside the sequence, 0-based, the first token ([CLS]) is 0.  A LIST, not a
 *                            range: any order, gaps and repeats are legal, a repeated position counts as often as it is
 *                            listed (as `embedded[i][positions]` does), a list may be longer than the sequence;
 *   n_span_tok               the length of span_tok (= span_cu[S] of a well-formed table; what the kernel clamps offsets to);
 *   span_out_f32 [S, hidden] (may be NULL) the means.  Fixed arithmetic, restated bit for bit on the host by
 *                            tests/test_span_pool_gpu.py: each bf16 element widened to float32, float32 adds in list order
 *                            starting from 0, ONE float32 division by the list length.  An EMPTY list gives a zero row
 *                            (torch.mean of an empty selection is NaN);
 *   span_unit_f16 [S, ld_span_unit] (may be NULL; hidden <= 768) exactly tsim_l2norm_rows(span rows, eps 1e-8), with
 *                            span_rho_max (may be NULL) raised as it raises rho_max — the call runs that routine on the
 *                            means.  Without span_out_f32 the means live in encoder scratch (S <= 1.5 x max_tokens then).
 * Nothing faults on a bad table: a position outside [0, len(sequence)), a span_seq outside [0, B) and list offsets outside
 * [0, n_span_tok] or out of order are clamped into range and computed anyway (a position listed for an EMPTY sequence adds
 * zeros), and raise TSIM_ENC_ERR_SPAN in the flag word of tsim_encoder_error_flags.
 * S == 0: tsim_encoder_forward_ex, bit for bit (the span arguments are not read).  S > 0 needs B > 0 and at least one span
 * output, else TSIM_EINVAL. */
int tsim_encoder_forward_spans(tsim_encoder *enc, const int32_t *tok_ids, const int32_t *tok_type, const int32_t *tok_pos,
                               const int32_t *tok_col, const int32_t *cu_seqlens, int32_t T, int32_t B, int32_t max_len,
                               float *pooled_f32, void *unit_f16, int ld_unit, float *unit_rho_max,
                               void *last_hidden_bf16, float *logits_f32, const int32_t *span_seq, const int32_t *span_cu,
                               const int32_t *span_tok, int32_t S, int32_t n_span_tok, float *span_out_f32,
                               void *span_unit_f16, int ld_span_unit, float *span_rho_max, void *stream);

/* Kernels cannot raise HF's IndexError: a token id outside [0, vocab), a token type outside [0, n_types), a position row outside [0, max_pos), a span-table entry out of range or a token whose
 * column is >= the max_len passed to tsim_encoder_forward is clamped / computed anyway and leaves a bit in a per-encoder
 * flag word.  This call copies the word to *flags_host, clears it and SYNCHRONISES `stream` (the only entry point that
 * does): 0 = every forward since the last call was clean.  The Python wrappers call it at the end of encode_text. */
#define TSIM_ENC_ERR_TOKEN_ID 1
#define TSIM_ENC_ERR_POSITION 2
#define TSIM_ENC_ERR_MAX_LEN 4
#define TSIM_ENC_ERR_TOKEN_TYPE 8
#define TSIM_ENC_ERR_SPAN 16   /* tsim_encoder_forward_spans: a position, sequence index or list offset of the span table */
int tsim_encoder_error_flags(tsim_encoder *enc, int32_t *flags_host, void *stream);

/* Introspection (host only, no launch): the work items of workgroup b of G in a chained LayerNorm-GEMM + projection launch of the
 * hidden-384 layer, as the kernel computes them.  The launch has one workgroup per whole 256-token block (blocks == G, anything
 * else is refused): workgroup b owns block b, all ntiles = N / 96 items of it; the rem_blocks * ntiles items of the blocks behind them are cut into G contiguous shares.  An item
 * is block * ntiles + feature tile.  Returns the number of items of workgroup b (negative: bad arguments) and writes the first
 * min(count, cap) of them. */
int tsim_chain_items_host(int blocks, int rem_blocks, int ntiles, int G, int b, int32_t *items, int cap);

/* Introspection (host only, no launch): the kernels an encoder of configuration cfg runs in layer `layer` of a forward of T
 * tokens, as tsim_encoder_create plans them and the forward executes them (DESIGN.md "Encoder routes by configuration").
 * A configuration that tsim_encoder_create refuses is refused here with the same code and text. */
#define TSIM_FAMILY_H64 0             /* hidden 64: gemm_bf16 tiles */
#define TSIM_FAMILY_H384_PACKED 1     /* hidden 384, BERT family: qkv, h1 and the residual stream block-packed */
#define TSIM_FAMILY_H384_ROWMAJOR 2   /* hidden 384, MPNet or an ffn gemm_xres2 does not take */
#define TSIM_FAMILY_PP 3              /* hidden 768 / 1024, bf16: gemm_pp + res_ln_rows */
#define TSIM_FAMILY_PP_MX 4           /* hidden 768 / 1024, MXFP8 operands: gemm_pp_mx + res_ln_rows<QUANT> */
/* form[]: the projections of a layer ... */
#define TSIM_ROUTE_QKV 0
#define TSIM_ROUTE_O 1       /* O-projection + residual + LayerNorm */
#define TSIM_ROUTE_FFN1 2    /* + GELU */
#define TSIM_ROUTE_FFN2 3    /* + residual + LayerNorm */
/* ... and their kernel forms */
#define TSIM_FORM_BF16_128x64 1          /* gemm_bf16 128 x 64 tile */
#define TSIM_FORM_BF16_128x128 2         /* gemm_bf16 128 x 128 tile */
#define TSIM_FORM_XRES2 3                /* gemm_xres2, row-major output */
#define TSIM_FORM_XRES2_PACKED 4         /* gemm_xres2<PK>, or chained behind the previous LayerNorm GEMM (chain_blocks) */
#define TSIM_FORM_PP_256_PACKED_W 5      /* gemm_pp, 256-wide feature tile, tile-major copy of W */
#define TSIM_FORM_PP_256 6               /* gemm_pp, 256-wide feature tile, row-major W */
#define TSIM_FORM_PP_128 7               /* gemm_pp, 128-wide feature tile, row-major W */
#define TSIM_FORM_PP_MX 8                /* gemm_pp_mx (QKV behind quant_mx in layer 0; FFN1 with the GELU_MX epilogue) */
#define TSIM_FORM_BF16_RES_LN 9          /* gemm_bf16 128 x 64 tile with the residual + LayerNorm epilogue */
#define TSIM_FORM_LN384 10               /* hidden-384 LayerNorm GEMM: row segments by T (seg[]) */
#define TSIM_FORM_PP_RES_LN_PACKED_W 11  /* gemm_pp F32 on the tile-major copy of W + res_ln_rows */
#define TSIM_FORM_PP_RES_LN 12           /* gemm_pp F32 on row-major W + res_ln_rows */
#define TSIM_FORM_PP_MX_RES_LN 13        /* (quant_mx +) gemm_pp_mx F32 + res_ln_rows<QUANT> */
/* row segments of a TSIM_FORM_LN384 projection */
#define TSIM_SEG_LN_ROWS 1          /* ln_rows_gemm: whole 256-token blocks */
#define TSIM_SEG_LN_ROWS_CHAINED 2  /* ln_rows_xres2: the same blocks, their workgroups run the next projection too */
#define TSIM_SEG_LN_TAIL 3          /* ln_tail_gemm */
#define TSIM_SEG_LN_SPLIT2 4        /* ln_split, 2 feature slices per row block, + ln_split_finish */
#define TSIM_SEG_LN_SPLIT4 5        /* ln_split, 4 feature slices */
#define TSIM_SEG_BF16_128x384 6     /* gemm_bf16 128 x 384 tile, RES_LN epilogue */
#define TSIM_SEG_BF16_64x384 7      /* gemm_bf16 64 x 384 tile, RES_LN epilogue */
/* weight images beside the row-major bf16 matrices, and scratch buffers beside x0, x1, qkv, ctx, h1 */
#define TSIM_IMG_PP_QKV_O 1   /* tile-major copies of the QKV and O matrices (gemm_pp) */
#define TSIM_IMG_LN_KTILE 2   /* O and FFN2 matrices as k-tile LDS images (gemm_bf16 x 384 tiles) */
#define TSIM_IMG_LN_FRAG 4    /* O and FFN2 matrices as MFMA fragment images (ln_rows, ln_tail, ln_split) */
#define TSIM_IMG_MXFP8 8      /* e4m3 bytes (tile-major) and E8M0 scales of all four matrices */
#define TSIM_BUF_YBUF 1       /* fp32 pre-LayerNorm sums */
#define TSIM_BUF_LNIMG 2      /* ln_split's accumulator images */
#define TSIM_BUF_MX_ACT 4     /* MXFP8 images of the projections' inputs */
#define TSIM_ROUTE_MAX_SEGS 4

typedef struct tsim_route_segment {
    int32_t form, row0, rows;   /* TSIM_SEG_*; rows [row0, row0 + rows) */
} tsim_route_segment;

typedef struct tsim_encoder_route {
    int32_t family;         /* TSIM_FAMILY_* */
    int32_t form[4];        /* TSIM_FORM_* by TSIM_ROUTE_* */
    int32_t images;         /* TSIM_IMG_* bits */
    int32_t buffers;        /* TSIM_BUF_* bits */
    int32_t chain_blocks;   /* 256-token blocks whose LayerNorm workgroups run the next projection too (FFN1 behind O, the
                             * next layer's QKV behind FFN2); 0: none at this configuration or T */
    int32_t qkv_chained;    /* 1: the previous layer's FFN2 launch has run this layer's QKV */
    int32_t n_seg[2];       /* segments of O ([0]) and FFN2 ([1]); 0 unless their form is TSIM_FORM_LN384 */
    tsim_route_segment seg[2][TSIM_ROUTE_MAX_SEGS];   /* in row order; they partition [0, T) */
} tsim_encoder_route;

int tsim_encoder_route_host(const tsim_encoder_config *cfg, int32_t T, int32_t layer, tsim_encoder_route *out);

/* ---- tokenizer (host code, no GPU): BERT WordPiece for pure-ASCII sentences -------------------------------------------------
 * Replaces, for the sentences it handles, the host tokenizer call of the reference's encode_text
 * (/root/reference/src/models/sentence_encoder.py:144-153: tokenizer(text=batch, padding=True, truncation=True,
 * max_length=...)) with the same ids: BertNormalizer (clean_text, lowercase) -> BertPreTokenizer -> WordPiece -> prefix /
 * suffix special ids -> truncation on the right to max_len, as the `tokenizers` library the reference depends on does it.
 * The vocabulary is one blob of UTF-8 keys + vocab_size + 1 byte offsets; the id of a key is its position.  `added_*`: the
 * contents of the library's added / special tokens, as written and, for the tokens the library matches on the normalised
 * text (normalized=True, the default of add_tokens), also as its normaliser rewrites them.  A sentence that holds one of
 * them in its raw bytes or in its normalised text (control characters dropped, white space mapped to ' ', lower-cased when
 * `lowercase`), or any non-ASCII byte, is NOT handled.  The contents are fixed at creation: after the tokenizer gains a
 * token, create a new handle.  Thread-safe after creation. */
int tsim_wordpiece_create(const char *vocab_text, const int64_t *vocab_offsets, int32_t vocab_size,
                          const char *continuing_prefix, int32_t unk_id, const int32_t *prefix_ids, int32_t n_prefix,
                          const int32_t *suffix_ids, int32_t n_suffix, int32_t lowercase, int32_t max_input_chars_per_word,
                          const char *added_text, const int64_t *added_offsets, int32_t n_added, void **handle);
void tsim_wordpiece_destroy(void *handle);
/* n sentences (one blob + n + 1 byte offsets) on n_threads host threads (<= 0: all cores).  out_ids receives the ids of the
 * handled sentences back to back (sentence order); out_capacity (in ids) must be at least sum_i min(max_len, bytes_i +
 * specials), e.g. total bytes + n * specials, else TSIM_ENOMEM.  out_lens[i] = ids of sentence i (0 when not handled),
 * handled[i] = 1 / 0: the caller tokenises the others with the library itself. */
int tsim_wordpiece_encode(void *handle, const char *text, const int64_t *text_offsets, int64_t n, int32_t max_len,
                          int32_t n_threads, int32_t *out_ids, int64_t out_capacity, int32_t *out_lens, uint8_t *handled);

#ifdef __cplusplus
}
#endif
#endif /* TSIM_H */
