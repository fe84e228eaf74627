// Graph index (included by search.hip, after the helpers it uses): a beam search over a fixed-degree proximity graph, and the
// detour count that prunes an exact kNN graph into one (CAGRA's rank-based optimisation).  Scores are those of the list
// search, bit for bit: exact_load_query and exact_score_batch unchanged, the Euclidean rows read through l2_f32 (-dist^2
// inside, the sign flipped on output).  So a result is a subset of the flat search's, with identical scores.
//
// The search, per query (include/tsim.h states it in full; tests/graph_cases.py restates it in numpy):
//   visited = {}, beam = {} (capacity ef, ordered (score desc, row asc));
//   every distinct usable entry point joins visited, is scored and offered to the beam;
//   at most max_iters times: the parents are the best `width` beam entries not yet expanded (none: stop); they are marked
//   expanded; every neighbour of every parent that is usable and not in visited joins visited and is scored (NaN: dropped, the
//   row stays visited); the beam becomes the best ef of (beam + the new rows).
// The rows of the beam are distinct and the order is total, so the result does not depend on which lane, wave or parent
// delivers a row first — the only freedom the kernel takes.
//
// Work.  One 256-thread workgroup per query, grid-strided.  In LDS:
//   - the beam: the running list (SlList, kp = sl_list_len(ef) entries, offers bounded by the ef-th entry: its first ef entries
//     are the best ef of everything scored so far, which is what "best ef of (beam + new)" is by induction);
//   - visited: an open-addressing table of row numbers in DYNAMIC LDS, linear probing, insertion by compare-and-swap — of
//     several lanes offering one id exactly one sees the empty slot and scores the row.  The host sizes it to a power of two
//     >= 2 (E + max_iters width R), the most rows a query can visit, so it is never more than half full and a probe always
//     ends at the id or at an empty slot; nothing resets it.  The EXPANDED mark rides in the table: an expanded row r is
//     stored as ~r (negative), so SlList stays as it is;
//   - stage: the rows that won their insertion in this iteration (at most width R <= 256, or E <= 256), compacted through an
//     LDS counter and dealt to the four waves in batches of eight (exact_score_batch: the eight row loads of a batch are in
//     flight together, and the four waves' batches overlap).
// An iteration is two dependent memory round trips — the parents' graph rows (one lane per neighbour), then the neighbours'
// rows — plus the scoring and one merge of at most 256 entries into the beam.
// Entry points come shared (tsim_graph_search: entries [E], the same for every query) or per query (tsim_graph_search_seeded:
// GraphSeeds below) — one kernel, instantiated for either; they differ before and in the entry step (it == -1) only.
// House rule for ids: a negative id is padding, an id >= N is never dereferenced and raises TSIM_GRAPH_ST_ROW; a tombstone
// (row_ids[row] < 0) is traversed like any row and dropped only from the OUTPUT.
#pragma once

namespace tsim {
constexpr int GRAPH_MAX_R = TSIM_GRAPH_MAX_DEGREE;
constexpr int GRAPH_MAX_E = TSIM_GRAPH_MAX_ENTRIES;
constexpr int GRAPH_MAX_WIDTH = TSIM_GRAPH_MAX_WIDTH;
constexpr int GRAPH_STAGE = 256;                                  // ids of one step: E, or width R
constexpr int64_t GRAPH_MAX_SLOTS = TSIM_GRAPH_MAX_TABLE_BYTES / 4;   // 128 KiB of table: 16 384 visits
constexpr int GRAPH_MIN_SLOTS = 64;
constexpr int GRAPH_EMPTY = 0x7fffffff;                           // (rows are < 2^31 - 64; ~row is negative)
constexpr int GRAPH_PRUNE_MAX_K0 = TSIM_GRAPH_PRUNE_MAX_K0;
static_assert(GRAPH_MAX_WIDTH * GRAPH_MAX_R <= GRAPH_STAGE && GRAPH_MAX_E <= GRAPH_STAGE, "one lane per id of a step");
static_assert(SL_MAX_K >= TSIM_GRAPH_MAX_EF && SL_NB >= GRAPH_STAGE, "the beam is a running list, a step one block of it");

// slots of the visited table: the smallest power of two >= 2 (E + max_iters width R), at least GRAPH_MIN_SLOTS; saturates
// above the cap so that the caller's comparison fails
static inline int64_t graph_table_slots(int E, int R, int width, int64_t max_iters) {
    const int64_t visits = (int64_t)E + std::min<int64_t>(max_iters, (int64_t)1 << 32) * width * R;
    int64_t s = GRAPH_MIN_SLOTS;
    while (s < 2 * visits && s <= GRAPH_MAX_SLOTS) s <<= 1;
    return s;
}

__device__ __forceinline__ unsigned graph_hash(int id, int shift) { return ((unsigned)id * 2654435761u) >> shift; }

// true when THIS call put id into the table (it was absent and no other lane got there first)
__device__ __forceinline__ bool graph_visit(int *tab, unsigned mask, int shift, int id) {
    unsigned h = graph_hash(id, shift);
    for (;;) {   // ends: the table is never more than half full
        const int old = atomicCAS(tab + h, GRAPH_EMPTY, id);
        if (old == GRAPH_EMPTY) return true;
        if (old == id || old == ~id) return false;
        h = (h + 1) & mask;
    }
}
// the slot that holds id (as id or as ~id), -1 when it is absent
__device__ __forceinline__ int graph_slot(const int *tab, unsigned mask, int shift, int id) {
    unsigned h = graph_hash(id, shift);
    for (;;) {
        const int v = tab[h];
        if (v == id || v == ~id) return (int)h;
        if (v == GRAPH_EMPTY) return -1;
        h = (h + 1) & mask;
    }
}

// Per-query entry points (tsim_graph_search_seeded), in two levels: query q enters through the lists probes[q][0 .. P) and a
// list l through the rows seeds[l][0 .. S) (seeds null: S = 1 and a probe is a row), E = P S ids.  probes null: the kernel finds
// them first, the P of the T centroids of best score to the query, through the beam's own running list.
struct GraphSeeds {
    const int32_t *seeds, *probes;
    const void *centroids;   // T rows of the stored rows' type
    int64_t T, ld_probes, ld_centroids;
    int S, P, pp;   // pp: sl_list_len(P)
    int32_t *out_probes;
};

using GraphShared = const int32_t *__restrict__;   // the entry points every query starts from

// EN = GraphShared: tsim_graph_search (the code it had before the seeded form existed: profiles/graph_entries_ab.txt compares
// the code objects); EN = GraphSeeds: tsim_graph_search_seeded, which differs before and in the entry step only.
template <typename T, bool COS, typename EN>
__global__ __launch_bounds__(256) void graph_search_kernel(int64_t Q, int64_t N, const T *__restrict__ xq, int64_t ldq,
                                                           const T *__restrict__ xr, int64_t ldr, int d,
                                                           const int32_t *__restrict__ graph, int R, EN entries, int E,
                                                           const int32_t *__restrict__ row_ids, int ef, int width, int max_iters,
                                                           int slots, int shift, int k, int kp, float *__restrict__ out_s,
                                                           int64_t *__restrict__ out_i, int64_t idx_offset,
                                                           int32_t *__restrict__ status) {
    constexpr bool SEEDED = std::is_same<EN, GraphSeeds>::value;
    [[maybe_unused]] const EN &sd = entries;
    extern __shared__ __attribute__((aligned(16))) int graph_tab[];
    SlList<int, false> top = sl_shared_list<int, false>();
    __shared__ unsigned long long open_s[TSIM_GRAPH_MAX_EF / 64];   // beam entries not yet expanded, one bit each
    __shared__ int stage[GRAPH_STAGE], par_s[GRAPH_MAX_WIDTH], cnt_s[4], nnew_s, st_s;
    constexpr bool NEG = is_l2_rows<T>;
    const int tid = threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned mask = (unsigned)slots - 1;
    const int nw = (ef + 63) >> 6;
    for (int64_t q = blockIdx.x; q < Q; q += gridDim.x) {   // workgroup-uniform
        ExactQuery<T> eqr;
        exact_load_query<T, COS>(eqr, xq + q * ldq, d, lane);
        for (int t = tid; t < slots; t += 256) graph_tab[t] = GRAPH_EMPTY;
        if (tid == 0) {
            nnew_s = 0;
            st_s = 0;
        }
        if constexpr (SEEDED) {   // the query's P probes into stage, which nothing uses before the entry step
            if (sd.probes) {
                if (tid < sd.P) stage[tid] = sd.probes[q * sd.ld_probes + tid];
            } else {
                // the P best centroids: the running list, blocks of 256 centroids, eight to a wave's batch as below
                const T *xc = static_cast<const T *>(sd.centroids);
                const int pp = sd.pp, nc = (int)sd.T;
                top.reset(pp);
                for (int c0 = 0; c0 < nc; c0 += GRAPH_STAGE) {   // workgroup-uniform
                    const int n = nc - c0 < GRAPH_STAGE ? nc - c0 : GRAPH_STAGE;
                    const SlBound<int> w = top.bound(sd.P);
                    for (int b = wave * 8; b < n; b += 32) {   // wave-uniform
                        const int nvalid = n - b < 8 ? n - b : 8;
                        const int row = c0 + b + (lane < nvalid ? lane : 0);
                        const float s = exact_score_batch<T, COS, 8>(eqr, xc, sd.ld_centroids, row, 0, nvalid, d, lane);
                        if (lane < nvalid) top.offer(s, row, w);
                    }
                    top.flush(pp);
                }
                if (tid < sd.P) stage[tid] = top.top_i[tid] == sl_pad<int>() ? -1 : top.top_i[tid];
                __syncthreads();   // (the list is read: the reset below may overwrite it)
            }
        }
        top.reset(kp);   // (a barrier)
        if constexpr (SEEDED)
            if (sd.out_probes && tid < sd.P) sd.out_probes[q * sd.P + tid] = stage[tid];
        int bits = 0;
        for (int it = -1;; ++it) {   // it == -1: the entry points
            int cnt = E;
            if (it >= 0) {
                for (int t0 = wave * 64; t0 < nw * 64; t0 += 256) {   // wave-uniform
                    const int t = t0 + lane;
                    const int r = t < ef ? top.top_i[t] : sl_pad<int>();
                    bool open = false;
                    if (r != sl_pad<int>()) {
                        const int s = graph_slot(graph_tab, mask, shift, r);
                        open = s >= 0 && graph_tab[s] == r;
                    }
                    const unsigned long long m = __ballot(open);
                    if (lane == 0) open_s[t0 >> 6] = m;
                }
                __syncthreads();
                // thread j < width looks for the j-th open entry; every thread counts them
                int seen = 0, mine = -1;
                for (int wd = 0; wd < nw; ++wd) {
                    unsigned long long m = open_s[wd];
                    const int c = __popcll(m);
                    if (mine < 0 && tid < width && seen + c > tid) {
                        for (int j = seen; j < tid; ++j) m &= m - 1;
                        mine = wd * 64 + __ffsll(m) - 1;
                    }
                    seen += c;
                }
                const int np = seen < width ? seen : width;
                if (np == 0) break;
                if (it >= max_iters) {
                    bits |= TSIM_GRAPH_ST_ITERS;
                    break;
                }
                if (tid < np) {
                    const int r = top.top_i[mine];
                    const int s = graph_slot(graph_tab, mask, shift, r);
                    if (s >= 0) graph_tab[s] = ~r;   // (a beam row is always in the table)
                    par_s[tid] = r;
                }
                __syncthreads();
                cnt = np * R;
            }
            const int t = tid < cnt ? tid : 0;
            int id;
            if constexpr (SEEDED) {
                if (it < 0) {   // workgroup-uniform
                    const int l = stage[t / sd.S];
                    const bool ok = l >= 0 && l < sd.T;
                    if (tid < cnt && l >= sd.T) bits |= TSIM_GRAPH_ST_ROW;
                    id = !ok ? -1 : sd.seeds ? sd.seeds[(int64_t)l * sd.S + t % sd.S] : l;
                    __syncthreads();   // everyone has read its probe: stage takes the rows of the step
                } else {
                    id = graph[(int64_t)par_s[t / R] * R + t % R];
                }
            } else {
                id = it < 0 ? entries[t] : graph[(int64_t)par_s[t / R] * R + t % R];
            }
            if (tid < cnt && id >= N) bits |= TSIM_GRAPH_ST_ROW;
            if (tid < cnt && id >= 0 && id < N && graph_visit(graph_tab, mask, shift, id)) stage[atomicAdd(&nnew_s, 1)] = id;
            __syncthreads();
            const int n = nnew_s;
            const SlBound<int> w = top.bound(ef);
            for (int b = wave * 8; b < n; b += 32) {   // wave-uniform: batches of eight rows, dealt round the four waves
                const int nvalid = n - b < 8 ? n - b : 8;
                const int row = stage[b + (lane < nvalid ? lane : 0)];
                const float s = exact_score_batch<T, COS, 8>(eqr, xr, ldr, row, 0, nvalid, d, lane);
                if (lane < nvalid) top.offer(s, row, w);
            }
            top.flush(kp);   // (its first barrier: everyone has read nnew_s and stage)
            if (tid == 0) nnew_s = 0;
        }
        if (bits) atomicOr(&st_s, bits);
        // the first k beam entries that are no tombstones, in order
        int done = 0;
        for (int t0 = 0; t0 < nw * 64 && done < k; t0 += 256) {   // workgroup-uniform
            const int t = t0 + tid;
            const int r = t < ef ? top.top_i[t] : sl_pad<int>();
            const bool real = r != sl_pad<int>();
            const int id = row_ids ? row_ids[real ? r : 0] : 0;
            const bool keep = real && id >= 0;
            const unsigned long long m = __ballot(keep);
            if (lane == 0) cnt_s[wave] = __popcll(m);
            __syncthreads();
            int at = done + __popcll(m & ((1ull << lane) - 1)), all = 0;
#pragma unroll
            for (int wv = 0; wv < 4; ++wv) {
                at += wv < wave ? cnt_s[wv] : 0;
                all += cnt_s[wv];
            }
            if (keep && at < k) {
                const float s = top.top_s[t];
                out_s[q * k + at] = NEG ? -s : s;
                out_i[q * k + at] = row_ids ? (int64_t)id : (int64_t)r + idx_offset;
            }
            done += all;
            __syncthreads();
        }
        for (int t = done + tid; t < k; t += 256) {
            out_s[q * k + t] = NEG ? INFINITY : -INFINITY;
            out_i[q * k + t] = -1;
        }
        if (status && tid == 0) status[q] = st_s;   // (behind the barriers of the loop above, or of the last flush when k == 0)
        __syncthreads();
    }
}

// Detour counts of an exact kNN graph g0 [N, K0] (rank order) and the forward list they select.  One workgroup per node i:
// the K0 rows of g0 its neighbours own are gathered into LDS, D[b] = #{a < b : g0[i][b] in g0[g0[i][a]][0..b)} (an unusable
// g0[i][a] owns no row; an unusable g0[i][b] gets D = K0, behind every count), and F[i] = the R entries of smallest (D, b).
__global__ __launch_bounds__(256) void graph_prune_kernel(int64_t N, const int32_t *__restrict__ g0, int K0, int R,
                                                          int32_t *__restrict__ out_f, int32_t *__restrict__ out_d) {
    extern __shared__ __attribute__((aligned(16))) int prune_smem[];
    int *nb = prune_smem, *g = nb + K0 * K0, *D = g + K0;
    const int tid = threadIdx.x;
    for (int64_t i = blockIdx.x; i < N; i += gridDim.x) {
        for (int t = tid; t < K0; t += 256) {
            g[t] = g0[i * K0 + t];
            D[t] = 0;
        }
        __syncthreads();
        for (int p = tid; p < K0 * K0; p += 256) {
            const int a = p / K0, c = p - a * K0;
            const int ga = g[a];
            const bool ok = ga >= 0 && ga < N;
            const int v = g0[(int64_t)(ok ? ga : 0) * K0 + c];   // clamped: loaded, dropped
            nb[p] = ok ? v : -1;
        }
        __syncthreads();
        for (int p = tid; p < K0 * K0; p += 256) {
            const int a = p / K0, b = p - a * K0;
            const int tg = g[b];
            if (a < b && tg >= 0 && tg < N) {
                bool found = false;
                for (int c = 0; c < b; ++c) found |= nb[a * K0 + c] == tg;
                if (found) atomicAdd(D + b, 1);
            }
        }
        __syncthreads();
        for (int b = tid; b < K0; b += 256)
            if (!(g[b] >= 0 && g[b] < N)) D[b] = K0;
        __syncthreads();
        for (int b = tid; b < K0; b += 256) {
            const int db = D[b];
            int r = 0;
            for (int c = 0; c < K0; ++c) r += D[c] < db || (D[c] == db && c < b);
            if (r < R) out_f[i * R + r] = db < K0 ? g[b] : -1;
            if (out_d) out_d[i * K0 + b] = db;
        }
        __syncthreads();
    }
}
}  // namespace tsim

extern "C" size_t tsim_graph_search_lds_bytes(int n_entries, int R, int width, int max_iters) {
    using namespace tsim;
    if (n_entries < 1 || n_entries > GRAPH_MAX_E || R < 1 || R > GRAPH_MAX_R || width < 1 || width > GRAPH_MAX_WIDTH || max_iters < 1)
        return 0;
    return (size_t)TSIM_GRAPH_STATIC_LDS_BYTES + (size_t)graph_table_slots(n_entries, R, width, max_iters) * 4;
}

extern "C" int tsim_graph_search(int space, const float *eq_f32, int64_t ldq_f32, int64_t Q, const float *rows_f32, int64_t ld_rows,
                                 int64_t N, int d, const int32_t *graph, int R, const int32_t *entries, int n_entries,
                                 const int32_t *row_ids, int ef, int width, int max_iters, int k, float *out_scores, int64_t *out_idx,
                                 int64_t idx_offset, int32_t *out_status, void *stream) {
    using namespace tsim;
    const char *what = "graph_search";
    TSIM_REQUIRE(eq_f32 && rows_f32 && graph && entries && out_scores && out_idx, "%s: null pointer", what);
    TSIM_REQUIRE(space == TSIM_SPACE_COSINE || space == TSIM_SPACE_DOT || space == TSIM_SPACE_L2, "%s: unknown space %d", what, space);
    TSIM_REQUIRE(Q > 0 && N > 0, "%s: bad shape Q=%lld N=%lld", what, (long long)Q, (long long)N);
    TSIM_REQUIRE(R >= 1 && R <= GRAPH_MAX_R, "%s: degree R=%d outside 1..%d", what, R, GRAPH_MAX_R);
    TSIM_REQUIRE(n_entries >= 1 && n_entries <= GRAPH_MAX_E, "%s: %d entry points, outside 1..%d", what, n_entries, GRAPH_MAX_E);
    TSIM_REQUIRE(width >= 1 && width <= GRAPH_MAX_WIDTH, "%s: width=%d outside 1..%d", what, width, GRAPH_MAX_WIDTH);
    TSIM_REQUIRE(k >= 1 && k <= TOPK_LARGE_MAX_K, "%s: k=%d outside 1..%d", what, k, TOPK_LARGE_MAX_K);
    TSIM_REQUIRE(ef >= k && ef <= TSIM_GRAPH_MAX_EF, "%s: ef=%d outside k=%d..%d", what, ef, k, TSIM_GRAPH_MAX_EF);
    TSIM_REQUIRE(max_iters >= 1, "%s: max_iters=%d < 1", what, max_iters);
    TSIM_REQUIRE(d >= 1 && d <= 64 * XS_MAXI, "%s: d=%d outside 1..%d", what, d, 64 * XS_MAXI);
    TSIM_REQUIRE(space != TSIM_SPACE_L2 || d < 64 * XS_MAXI, "%s: d=%d (the Euclidean space takes d <= %d)", what, d, 64 * XS_MAXI - 1);
    TSIM_REQUIRE(ldq_f32 >= d && ld_rows >= d, "%s: float32 row strides %lld/%lld < d=%d", what, (long long)ldq_f32, (long long)ld_rows,
                 d);
    TSIM_REQUIRE(N < (1ll << 31) - 64 && Q < (1ll << 31), "%s: too large for 32-bit row ids (N=%lld, Q=%lld)", what, (long long)N,
                 (long long)Q);
    const int64_t slots = graph_table_slots(n_entries, R, width, max_iters);
    TSIM_REQUIRE(slots <= GRAPH_MAX_SLOTS,
                 "%s: a query may visit %d + %d * %d * %d rows; the visited table holds at most %lld (%d B of LDS): lower max_iters", what,
                 n_entries, max_iters, width, R, (long long)(GRAPH_MAX_SLOTS / 2), TSIM_GRAPH_MAX_TABLE_BYTES);
    int shift = 32;
    while ((1ll << (32 - shift)) < slots) --shift;
    hipStream_t st = as_stream(stream);
    const int kp = sl_list_len(ef);
    const unsigned grid = (unsigned)(Q < 65536 ? Q : 65536);
    const size_t lds = (size_t)slots * 4;
    static DevOnce once_cos, once_dot, once_l2;
    if (space == TSIM_SPACE_COSINE) {
        TSIM_MAX_LDS(once_cos, (graph_search_kernel<float, true, GraphShared>), TSIM_GRAPH_MAX_TABLE_BYTES);
        hipLaunchKernelGGL((graph_search_kernel<float, true, GraphShared>), dim3(grid), dim3(256), lds, st, Q, N, eq_f32, ldq_f32, rows_f32,
                           ld_rows, d, graph, R, entries, n_entries, row_ids, ef, width, max_iters, (int)slots, shift, k, kp, out_scores, out_idx,
                           idx_offset, out_status);
    } else if (space == TSIM_SPACE_DOT) {
        TSIM_MAX_LDS(once_dot, (graph_search_kernel<float, false, GraphShared>), TSIM_GRAPH_MAX_TABLE_BYTES);
        hipLaunchKernelGGL((graph_search_kernel<float, false, GraphShared>), dim3(grid), dim3(256), lds, st, Q, N, eq_f32, ldq_f32, rows_f32,
                           ld_rows, d, graph, R, entries, n_entries, row_ids, ef, width, max_iters, (int)slots, shift, k, kp, out_scores, out_idx,
                           idx_offset, out_status);
    } else {   // (float32 rows read through l2_f32: with_score_mode says why)
        TSIM_MAX_LDS(once_l2, (graph_search_kernel<l2_f32, false, GraphShared>), TSIM_GRAPH_MAX_TABLE_BYTES);
        hipLaunchKernelGGL((graph_search_kernel<l2_f32, false, GraphShared>), dim3(grid), dim3(256), lds, st, Q, N,
                           reinterpret_cast<const l2_f32 *>(eq_f32), ldq_f32, reinterpret_cast<const l2_f32 *>(rows_f32), ld_rows, d, graph,
                           R, entries, n_entries, row_ids, ef, width, max_iters, (int)slots, shift, k, kp, out_scores, out_idx, idx_offset,
                           out_status);
    }
    TSIM_HIP_CHECK(hipGetLastError());
    return TSIM_OK;
}

extern "C" int tsim_graph_search_seeded(int space, const float *eq_f32, int64_t ldq_f32, int64_t Q, const float *rows_f32,
                                        int64_t ld_rows, int64_t N, int d, const int32_t *graph, int R, const int32_t *seeds,
                                        int64_t n_lists, int n_seeds, const int32_t *probes, int64_t ld_probes, int n_probe,
                                        const float *centroids, int64_t ld_centroids, const int32_t *row_ids, int ef, int width,
                                        int max_iters, int k, float *out_scores, int64_t *out_idx, int64_t idx_offset,
                                        int32_t *out_status, int32_t *out_probes, void *stream) {
    using namespace tsim;
    const char *what = "graph_search_seeded";
    TSIM_REQUIRE(eq_f32 && rows_f32 && graph && out_scores && out_idx, "%s: null pointer", what);
    TSIM_REQUIRE((probes != nullptr) != (centroids != nullptr), "%s: exactly one of probes and centroids must be given", what);
    TSIM_REQUIRE(space == TSIM_SPACE_COSINE || space == TSIM_SPACE_DOT || space == TSIM_SPACE_L2, "%s: unknown space %d", what, space);
    TSIM_REQUIRE(Q > 0 && N > 0, "%s: bad shape Q=%lld N=%lld", what, (long long)Q, (long long)N);
    TSIM_REQUIRE(R >= 1 && R <= GRAPH_MAX_R, "%s: degree R=%d outside 1..%d", what, R, GRAPH_MAX_R);
    const int S = seeds ? n_seeds : 1;          // without a seed table a probe is a row
    const int64_t T = seeds ? n_lists : N;
    TSIM_REQUIRE(S >= 1 && n_probe >= 1 && (int64_t)S * n_probe <= GRAPH_MAX_E,
                 "%s: %d probes of %d seeds: the entry points must number 1..%d", what, n_probe, S, GRAPH_MAX_E);
    TSIM_REQUIRE(T >= 1 && T < (1ll << 31) - 64, "%s: %lld lists, outside 1..2^31-65", what, (long long)T);
    TSIM_REQUIRE(!centroids || T <= TSIM_GRAPH_MAX_COARSE_LISTS, "%s: the kernel's coarse phase takes at most %d centroids, not %lld",
                 what, TSIM_GRAPH_MAX_COARSE_LISTS, (long long)T);
    TSIM_REQUIRE(!probes || ld_probes >= n_probe, "%s: probes row stride %lld < n_probe=%d", what, (long long)ld_probes, n_probe);
    TSIM_REQUIRE(width >= 1 && width <= GRAPH_MAX_WIDTH, "%s: width=%d outside 1..%d", what, width, GRAPH_MAX_WIDTH);
    TSIM_REQUIRE(k >= 1 && k <= TOPK_LARGE_MAX_K, "%s: k=%d outside 1..%d", what, k, TOPK_LARGE_MAX_K);
    TSIM_REQUIRE(ef >= k && ef <= TSIM_GRAPH_MAX_EF, "%s: ef=%d outside k=%d..%d", what, ef, k, TSIM_GRAPH_MAX_EF);
    TSIM_REQUIRE(max_iters >= 1, "%s: max_iters=%d < 1", what, max_iters);
    TSIM_REQUIRE(d >= 1 && d <= 64 * XS_MAXI, "%s: d=%d outside 1..%d", what, d, 64 * XS_MAXI);
    TSIM_REQUIRE(space != TSIM_SPACE_L2 || d < 64 * XS_MAXI, "%s: d=%d (the Euclidean space takes d <= %d)", what, d, 64 * XS_MAXI - 1);
    TSIM_REQUIRE(ldq_f32 >= d && ld_rows >= d && (!centroids || ld_centroids >= d), "%s: float32 row strides %lld/%lld/%lld < d=%d", what,
                 (long long)ldq_f32, (long long)ld_rows, (long long)ld_centroids, d);
    TSIM_REQUIRE(N < (1ll << 31) - 64 && Q < (1ll << 31), "%s: too large for 32-bit row ids (N=%lld, Q=%lld)", what, (long long)N,
                 (long long)Q);
    const int E = S * n_probe;
    const int64_t slots = graph_table_slots(E, R, width, max_iters);
    TSIM_REQUIRE(slots <= GRAPH_MAX_SLOTS,
                 "%s: a query may visit %d + %d * %d * %d rows; the visited table holds at most %lld (%d B of LDS): lower max_iters", what,
                 E, max_iters, width, R, (long long)(GRAPH_MAX_SLOTS / 2), TSIM_GRAPH_MAX_TABLE_BYTES);
    int shift = 32;
    while ((1ll << (32 - shift)) < slots) --shift;
    hipStream_t st = as_stream(stream);
    const int kp = sl_list_len(ef);
    const unsigned grid = (unsigned)(Q < 65536 ? Q : 65536);
    const size_t lds = (size_t)slots * 4;
    const GraphSeeds sd{seeds, probes, centroids, T, ld_probes, ld_centroids, S, n_probe, sl_list_len(n_probe), out_probes};
    static DevOnce once_cos, once_dot, once_l2;
    if (space == TSIM_SPACE_COSINE) {
        TSIM_MAX_LDS(once_cos, (graph_search_kernel<float, true, GraphSeeds>), TSIM_GRAPH_MAX_TABLE_BYTES);
        hipLaunchKernelGGL((graph_search_kernel<float, true, GraphSeeds>), dim3(grid), dim3(256), lds, st, Q, N, eq_f32, ldq_f32, rows_f32,
                           ld_rows, d, graph, R, sd, E, row_ids, ef, width, max_iters, (int)slots, shift, k, kp, out_scores, out_idx,
                           idx_offset, out_status);
    } else if (space == TSIM_SPACE_DOT) {
        TSIM_MAX_LDS(once_dot, (graph_search_kernel<float, false, GraphSeeds>), TSIM_GRAPH_MAX_TABLE_BYTES);
        hipLaunchKernelGGL((graph_search_kernel<float, false, GraphSeeds>), dim3(grid), dim3(256), lds, st, Q, N, eq_f32, ldq_f32, rows_f32,
                           ld_rows, d, graph, R, sd, E, row_ids, ef, width, max_iters, (int)slots, shift, k, kp, out_scores, out_idx,
                           idx_offset, out_status);
    } else {   // (float32 rows, and centroids, read through l2_f32)
        TSIM_MAX_LDS(once_l2, (graph_search_kernel<l2_f32, false, GraphSeeds>), TSIM_GRAPH_MAX_TABLE_BYTES);
        hipLaunchKernelGGL((graph_search_kernel<l2_f32, false, GraphSeeds>), dim3(grid), dim3(256), lds, st, Q, N,
                           reinterpret_cast<const l2_f32 *>(eq_f32), ldq_f32, reinterpret_cast<const l2_f32 *>(rows_f32), ld_rows, d, graph,
                           R, sd, E, row_ids, ef, width, max_iters, (int)slots, shift, k, kp, out_scores, out_idx, idx_offset, out_status);
    }
    TSIM_HIP_CHECK(hipGetLastError());
    return TSIM_OK;
}

extern "C" int tsim_graph_prune(const int32_t *knn, int64_t N, int K0, int R, int32_t *out_forward, int32_t *out_detours,
                                void *stream) {
    using namespace tsim;
    const char *what = "graph_prune";
    TSIM_REQUIRE(knn && out_forward, "%s: null pointer", what);
    TSIM_REQUIRE(N > 0 && N < (1ll << 31) - 64, "%s: N=%lld outside 1..2^31-65", what, (long long)N);
    TSIM_REQUIRE(K0 >= 1 && K0 <= GRAPH_PRUNE_MAX_K0, "%s: K0=%d outside 1..%d", what, K0, GRAPH_PRUNE_MAX_K0);
    TSIM_REQUIRE(R >= 1 && R <= K0 && R <= GRAPH_MAX_R, "%s: R=%d outside 1..min(K0=%d, %d)", what, R, K0, GRAPH_MAX_R);
    const size_t lds = (size_t)(K0 * K0 + 2 * K0) * 4;
    static DevOnce once;
    TSIM_MAX_LDS(once, graph_prune_kernel, (GRAPH_PRUNE_MAX_K0 * GRAPH_PRUNE_MAX_K0 + 2 * GRAPH_PRUNE_MAX_K0) * 4);
    const unsigned grid = (unsigned)(N < 16384 ? N : 16384);
    hipLaunchKernelGGL(graph_prune_kernel, dim3(grid), dim3(256), lds, as_stream(stream), N, knn, K0, R, out_forward, out_detours);
    TSIM_HIP_CHECK(hipGetLastError());
    return TSIM_OK;
}
