/*
 * tsim_graph_insert.h — the two entries that insert rows into a built proximity graph (tsim.h, "Graph index") instead of
 * rebuilding it.  They are exported by the same libtsim.so and obey every Convention of tsim.h: device pointers, all work on
 * `stream`, nothing read back, nothing allocated, TSIM_EINVAL (with tsim_last_error) before any launch.  Neither takes a
 * workspace.  They live in a header of their own until the next change that may touch the entry registry of tsim.h
 * (DESIGN.md section 3); the semantics below are final.
 *
 * One insertion step links B new rows n .. n + B - 1 into a graph over the rows 0 .. n - 1 (text_similarity_amd/ops.py
 * graph_insert; tests/graph_insert_cases.py restates it in numpy):
 *   1. candidates: C[x] int32 [K0] per new row x, best first, -1 padded — the beam search of x over the graph as it stands merged
 *      with the exact search of x among the B new rows (the caller's work: tsim_graph_search*, tsim_*_list_topk, a merge);
 *   2. forward edges, tsim_graph_insert_prune: the build's detour rule with the neighbour lists that exist at insertion time;
 *   3. reverse edges, tsim_graph_link_reverse: every row some new row chose takes its choosers into the back half of its own row,
 *      by the exact score against itself.
 *
 * tsim_graph_insert_prune.  cand int32 [B, K0] contiguous, 1 <= K0 <= TSIM_GRAPH_PRUNE_MAX_K0; graph int32 [n, R] contiguous,
 * n >= 1, 1 <= R <= min(K0, TSIM_GRAPH_MAX_DEGREE); B >= 1 and n + B < 2^31 - 64.  Row i of cand belongs to the new row n + i.
 * An id c is USABLE when 0 <= c < n + B; a negative id is padding; an id >= n + B is never dereferenced, is never chosen and sets
 * TSIM_GRAPH_INSERT_ST_ROW in out_status[i].  The neighbour list of a usable c is
 *      N(c) = graph[c][0 .. R)            when c < n,
 *      N(c) = cand[c - n][0 .. R)         when c is a row of the batch (the row itself included).
 * D[i][j] = #{a < j : cand[i][a] usable and cand[i][j] in N(cand[i][a])} for a usable cand[i][j] — the two-hop detours through
 * a better-ranked candidate — and D[i][j] = K0 for an unusable one.  out_forward int32 [B, R]: the R entries of cand[i] of
 * smallest (D, j), in that order, unusable ones as -1.  out_detours int32 [B, K0] (may be NULL): D.  out_status int32 [B] (may
 * be NULL): written, not accumulated.  Integers only.  One workgroup per new row: the K0 neighbour lists in LDS (K0 R words, at
 * most 32 KiB), counted with LDS atomics.
 *
 * tsim_graph_link_reverse.  rows_f32 [N, d] float32 (row stride ld_rows >= d), 1 <= d <= 768 (Euclidean <= 767), 1 <= N <
 * 2^31 - 64; space TSIM_SPACE_COSINE / _DOT / _L2 and scores as for the list entries of tsim.h, bit for bit.  graph int32 [N, R]
 * contiguous, 1 <= R <= TSIM_GRAPH_MAX_DEGREE, UPDATED IN PLACE.  targets int32 [T], 1 <= T <= N: DISTINCT rows (a target < 0 or
 * >= N is skipped and sets TSIM_GRAPH_LINK_ST_ROW).  in_ids int32 with in_lims int64 [T + 1] (CSR; in_lims[T] is the length of
 * in_ids): target j's incoming rows are in_ids[in_lims[j] .. in_lims[j + 1]), in the caller's order; bounds that decrease or
 * leave [0, in_lims[T]] are clamped and set TSIM_GRAPH_LINK_ST_LIMS.  For target t = targets[j], with h = R / 2:
 *   valid  = the non-negative entries of graph[t], in order;  kept = valid[0 .. h): they stay, at the front of the row;
 *   pool   = valid[h ..) followed by the incoming rows; negative ids, ids in kept and later repeats of an id are dropped, and the
 *            pool is cut to its first TSIM_GRAPH_LINK_POOL entries (a cut sets TSIM_GRAPH_LINK_ST_CUT);
 *   chosen = the R - h pool entries of best exact score AGAINST ROW t, ordered by (score desc, id asc), Euclidean (dist^2 asc, id
 *            asc) — the ids of tsim_*_list_topk of rows_f32[t] against the pool, k = R - h.  A NaN score is dropped; a pool id
 *            >= N is never dereferenced, is dropped and sets TSIM_GRAPH_LINK_ST_ROW;
 *   graph[t] = kept ++ chosen, -1 padded.
 * out_status int32 [T] (may be NULL): written, not accumulated.  One workgroup per target; it reads and writes its own graph row
 * only and the float rows are read-only, so no order between workgroups matters and nothing needs a second buffer.
 */
#ifndef TSIM_GRAPH_INSERT_H
#define TSIM_GRAPH_INSERT_H

#include "tsim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TSIM_GRAPH_INSERT_ST_ROW 1 /* a candidate id >= n + B */
#define TSIM_GRAPH_LINK_POOL 256   /* pool entries a target scores */
#define TSIM_GRAPH_LINK_ST_CUT 1   /* the pool held more than TSIM_GRAPH_LINK_POOL entries */
#define TSIM_GRAPH_LINK_ST_ROW 2   /* the target or a pool id was >= N (or the target negative) */
#define TSIM_GRAPH_LINK_ST_LIMS 4  /* the target's bounds in in_lims were clamped */

int tsim_graph_insert_prune(const int32_t *cand, int64_t B, int K0, const int32_t *graph, int64_t n, int R, int32_t *out_forward,
                            int32_t *out_detours, int32_t *out_status, void *stream);
int tsim_graph_link_reverse(int space, const float *rows_f32, int64_t ld_rows, int64_t N, int d, int32_t *graph, int R,
                            const int32_t *targets, int64_t T, const int64_t *in_lims, const int32_t *in_ids, int32_t *out_status,
                            void *stream);

#ifdef __cplusplus
}
#endif
#endif
