// De-overlap of candidate communities (included by search.hip, after list_search.h whose list_prep_kernel it uses): the one
// sequential step of community detection ("fast clustering": every group of at least min_size rows within a threshold of a
// centre row, largest first, no row in two groups).  The candidates come as a CSR in PRIORITY order — community c owns
// members[lims[c] .. lims[c+1]) — and the definition is the loop
//     taken = {}; for c in 0 .. C-1: free = [j in members(c), j not in taken]; if len(free) >= min_size: accept c, taken |= free
// (a member listed twice is tested twice and counts twice).  Outputs: accept[c] (0 / 1) and keep[t] (1 iff entry t of members
// is in the free list of an ACCEPTED community); the caller compacts.  Ids follow the house rule: a negative member is padding,
// a member >= N is never dereferenced, is dropped and sets TSIM_COMMUNITY_ST_ROW; lims go through list_prep_kernel (running
// maximum clamped to [0, T]: a decreasing pair is an empty community) and a changed word sets TSIM_COMMUNITY_ST_LIMS.
//
// Two forms, same results.
//
// Rounds (parallel).  state[c] is undecided, accepted or rejected; owner[j] is the accepted community that took row j, or none.
// A round is two launches, one wave per undecided community:
//   claim:  count the members whose owner is none ("free").  count < min_size: rejected for good.  Else offer the key
//           (round key, c) to claim[j] of every free member with atomicMin.  The round key falls as the round number grows, so
//           an offer of this round always beats what earlier rounds left in claim[j]: the array is never cleared.
//   decide: a member was free in the claim launch iff claim[j] carries this round's key (a free row was offered at least its own
//           community's key; a taken row was offered nothing).  c accepts iff every such member carries c's own key; it then
//           sets keep for them and owner[j] = c.  The decide launch never READS owner: owner words written by a community that
//           accepts in the same launch must not make a lower-priority community see a shared row as taken and accept on a
//           stale count.
// Why this is the sequential loop.  Invariant: every decided community has the decision, and every accepted one the free list,
// that the loop gives it; a row owned while an undecided community c lists it is owned by a community of higher priority.
//   (a) The highest-priority undecided community is decided in every round: it is rejected, or its key is the smallest offered
//       anywhere, so it wins every free member.  The rounds end after at most C of them.
//   (b) No community takes a row that a higher-priority undecided one still holds free: the higher one offered a smaller key.
//       So two communities accepting in one launch share no free row, and when c accepts, the undecided communities above it
//       have free lists — which only shrink — disjoint from c's: whatever the loop lets them take later, it is not c's.  The
//       decided ones above it are final by the invariant.  Hence c's free list now is the loop's.
//   (c) Rejection uses an upper bound: owned rows are a subset of what the loop has taken when it reaches c (invariant, and
//       (b) for the rows of lower-priority communities), so count >= the loop's count, and count < min_size rejects there too.
// Every decide launch writes ONE device word: the number of communities still undecided.  The host loops over rounds and reads
// that word; there is no grid-wide barrier, no cooperative launch, no waiting between workgroups, only vector atomics.
//
// Serial finish.  One workgroup walks the undecided communities in order: ballot / LDS count of the free members, then keep,
// a barrier, then owner (the barrier keeps a member listed twice free for both of its entries).  It is what remains when the
// caller's round budget is used up — a chain c0 ~ c1 ~ c2 ... in which each shares a row with the next needs one round per link
// — and with no rounds before it, it is the whole de-overlap.
#pragma once

namespace tsim {
constexpr int CM_UNDECIDED = 0, CM_ACCEPTED = 1, CM_REJECTED = 2;
constexpr int32_t CM_NONE = -1;
constexpr uint32_t CM_KEY0 = 0x7fffffffu;      // the key of round 0; round r has CM_KEY0 - r, the cleared word has 0xffffffff
constexpr int64_t CM_MAX_ROUND = 1ll << 30;
constexpr int CM_FIN_T = 1024;
constexpr unsigned CM_MAX_GRID = 2048;

__global__ __launch_bounds__(256) void community_init_kernel(int64_t C, int64_t N, const int64_t *__restrict__ lims,
                                                             const int64_t *__restrict__ clean, int32_t *__restrict__ state,
                                                             int32_t *__restrict__ owner, unsigned long long *__restrict__ claim,
                                                             int32_t *__restrict__ accept, int32_t *__restrict__ status) {
    const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
    bool changed = false;
    for (int64_t c = i0; c < C; c += step) {
        state[c] = CM_UNDECIDED;
        accept[c] = 0;
        changed |= clean[c] != lims[c] || clean[c + 1] != lims[c + 1];
    }
    for (int64_t j = i0; j < N; j += step) {
        owner[j] = CM_NONE;
        claim[j] = ~0ull;
    }
    if (__any(changed) && (threadIdx.x & 63) == 0) atomicOr(status, TSIM_COMMUNITY_ST_LIMS);   // (the word was cleared before the launch)
}

__device__ __forceinline__ int cm_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void community_claim_kernel(int64_t C, int64_t N, const int64_t *__restrict__ L,
                                                              const int32_t *__restrict__ members, int min_size, uint32_t rkey,
                                                              int32_t *__restrict__ state, const int32_t *__restrict__ owner,
                                                              unsigned long long *__restrict__ claim, int32_t *__restrict__ status,
                                                              int32_t *__restrict__ undecided) {
    const int lane = threadIdx.x & 63;
    if (blockIdx.x == 0 && threadIdx.x == 0) *undecided = 0;   // the decide launch of this round counts into it
    bool big = false;
    for (int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); c < C; c += (int64_t)gridDim.x * 4) {   // wave-uniform
        if (state[c] != CM_UNDECIDED) continue;
        const int64_t lo = L[c], hi = L[c + 1];
        int count = 0;
        for (int64_t t = lo + lane; t < hi; t += 64) {
            const int32_t j = members[t];
            big |= j >= N;
            count += j >= 0 && j < N && owner[j] == CM_NONE;
        }
        count = cm_wave_sum(count);
        if (count < min_size) {   // free members only ever shrink
            if (lane == 0) state[c] = CM_REJECTED;
            continue;
        }
        const unsigned long long key = ((unsigned long long)rkey << 32) | (uint32_t)c;
        for (int64_t t = lo + lane; t < hi; t += 64) {
            const int32_t j = members[t];
            // (claim[j] only ever falls, so a plain load is an upper bound of it: at or below the key, the atomic would change
            // nothing — most offers to a contested row end here)
            if (j >= 0 && j < N && owner[j] == CM_NONE && claim[j] > key) atomicMin(claim + j, key);
        }
    }
    if (__any(big) && lane == 0) atomicOr(status, TSIM_COMMUNITY_ST_ROW);
}

// (owner is written and never read here: "free" is what the claim launch left in claim[])
__global__ __launch_bounds__(256) void community_decide_kernel(int64_t C, int64_t N, const int64_t *__restrict__ L,
                                                               const int32_t *__restrict__ members, uint32_t rkey,
                                                               int32_t *__restrict__ state, int32_t *__restrict__ owner,
                                                               const unsigned long long *__restrict__ claim,
                                                               int32_t *__restrict__ accept, uint8_t *__restrict__ keep,
                                                               int32_t *__restrict__ undecided) {
    const int lane = threadIdx.x & 63;
    int left = 0;
    for (int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); c < C; c += (int64_t)gridDim.x * 4) {   // wave-uniform
        if (state[c] != CM_UNDECIDED) continue;
        const int64_t lo = L[c], hi = L[c + 1];
        bool lost = false;
        for (int64_t t = lo + lane; t < hi; t += 64) {
            const int32_t j = members[t];
            if (j < 0 || j >= N) continue;
            const unsigned long long k = claim[j];
            lost |= (uint32_t)(k >> 32) == rkey && (uint32_t)k != (uint32_t)c;
        }
        if (__any(lost)) {
            ++left;
            continue;
        }
        for (int64_t t = lo + lane; t < hi; t += 64) {
            const int32_t j = members[t];
            if (j < 0 || j >= N) continue;
            if ((uint32_t)(claim[j] >> 32) == rkey) {   // free in the claim launch, and won
                keep[t] = 1;
                owner[j] = (int32_t)c;
            }
        }
        if (lane == 0) {
            state[c] = CM_ACCEPTED;
            accept[c] = 1;
        }
    }
    if (left && lane == 0) atomicAdd(undecided, left);
}

__global__ __launch_bounds__(CM_FIN_T) void community_finish_kernel(int64_t C, int64_t N, const int64_t *__restrict__ L,
                                                                    const int32_t *__restrict__ members, int min_size,
                                                                    int32_t *__restrict__ state, int32_t *owner,
                                                                    int32_t *__restrict__ accept, uint8_t *__restrict__ keep,
                                                                    int32_t *__restrict__ status, int32_t *__restrict__ undecided) {
    __shared__ unsigned long long todo[CM_FIN_T / 64];
    __shared__ int wsum[CM_FIN_T / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool big = false;
    for (int64_t c0 = 0; c0 < C; c0 += CM_FIN_T) {
        const int64_t mine = c0 + threadIdx.x;
        const unsigned long long m = __ballot(mine < C && state[mine] == CM_UNDECIDED);
        if (lane == 0) todo[wave] = m;
        __syncthreads();
        for (int w = 0; w < CM_FIN_T / 64; ++w) {
            unsigned long long bits = todo[w];   // workgroup-uniform, as the whole walk
            while (bits) {
                const int b = __ffsll((long long)bits) - 1;
                bits &= bits - 1;
                const int64_t c = c0 + w * 64 + b;
                const int64_t lo = L[c], hi = L[c + 1];
                int count = 0;
                for (int64_t t = lo + threadIdx.x; t < hi; t += CM_FIN_T) {
                    const int32_t j = members[t];
                    big |= j >= N;
                    count += j >= 0 && j < N && owner[j] == CM_NONE;
                }
                count = cm_wave_sum(count);
                if (lane == 0) wsum[wave] = count;
                __syncthreads();
                int total = 0;
                for (int v = 0; v < CM_FIN_T / 64; ++v) total += wsum[v];
                if (total >= min_size) {
                    for (int64_t t = lo + threadIdx.x; t < hi; t += CM_FIN_T) {
                        const int32_t j = members[t];
                        if (j >= 0 && j < N && owner[j] == CM_NONE) keep[t] = 1;
                    }
                    __syncthreads();   // every entry was tested against the owners as they stood: a row listed twice is kept twice
                    for (int64_t t = lo + threadIdx.x; t < hi; t += CM_FIN_T)
                        if (keep[t]) owner[members[t]] = (int32_t)c;
                }
                if (threadIdx.x == 0) {
                    state[c] = total >= min_size ? CM_ACCEPTED : CM_REJECTED;
                    accept[c] = total >= min_size;
                }
                __syncthreads();   // owner before the next community's count; wsum is free again
            }
        }
        __syncthreads();   // (todo is free again)
    }
    if (__any(big) && lane == 0) atomicOr(status, TSIM_COMMUNITY_ST_ROW);
    if (threadIdx.x == 0) *undecided = 0;
}

struct CommunityWs {
    size_t clean, state, owner, claim, total;
};
static void plan_workspace_community(int64_t C, int64_t N, CommunityWs *w) {
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += align256(bytes); return at; };
    w->clean = take((size_t)(C + 1) * 8);
    w->state = take((size_t)C * 4);
    w->owner = take((size_t)N * 4);
    w->claim = take((size_t)N * 8);
    w->total = o;
}

static int community_check(const char *what, const int64_t *lims, const int32_t *members, int64_t C, int64_t T, int64_t N, int min_size,
                           const int32_t *accept, const uint8_t *keep, const int32_t *status, const int32_t *undecided,
                           void *workspace, size_t workspace_bytes, CommunityWs *w) {
    TSIM_REQUIRE(lims && accept && status && undecided && (members || T == 0) && (keep || T == 0), "%s: null pointer", what);
    TSIM_REQUIRE(C >= 0 && T >= 0 && N > 0, "%s: bad shape C=%lld T=%lld N=%lld", what, (long long)C, (long long)T, (long long)N);
    TSIM_REQUIRE(min_size >= 1, "%s: min_size=%d < 1", what, min_size);
    TSIM_REQUIRE(C < (1ll << 31) - 1 && N < (1ll << 31) - 64 && T < (1ll << 40), "%s: too large for one launch (C=%lld N=%lld T=%lld)",
                 what, (long long)C, (long long)N, (long long)T);
    plan_workspace_community(C, N, w);
    if (!workspace || workspace_bytes < w->total) return fail(TSIM_ENOMEM, "%s: workspace %zu B < %zu B", what, workspace_bytes, w->total);
    return TSIM_OK;
}
}  // namespace tsim

extern "C" size_t tsim_community_select_workspace_bytes(int64_t C, int64_t N) {
    if (C < 0 || N <= 0 || C >= (1ll << 31) - 1 || N >= (1ll << 31) - 64) return 0;
    tsim::CommunityWs w;
    tsim::plan_workspace_community(C, N, &w);
    return w.total;
}

extern "C" int tsim_community_select_rounds(const int64_t *lims, const int32_t *members, int64_t C, int64_t T, int64_t N, int min_size,
                                            int64_t first_round, int max_rounds, int32_t *accept, uint8_t *keep, int32_t *status,
                                            int32_t *undecided, void *workspace, size_t workspace_bytes, void *stream) {
    using namespace tsim;
    const char *what = "community_select_rounds";
    CommunityWs w;
    const int rc = community_check(what, lims, members, C, T, N, min_size, accept, keep, status, undecided, workspace, workspace_bytes, &w);
    if (rc) return rc;
    TSIM_REQUIRE(max_rounds >= 0 && first_round >= 0 && first_round + max_rounds <= CM_MAX_ROUND, "%s: rounds %lld + %d outside 0..%lld",
                 what, (long long)first_round, max_rounds, (long long)CM_MAX_ROUND);
    hipStream_t st = as_stream(stream);
    char *ws = reinterpret_cast<char *>(workspace);
    int64_t *clean = reinterpret_cast<int64_t *>(ws + w.clean);
    int32_t *state = reinterpret_cast<int32_t *>(ws + w.state);
    int32_t *owner = reinterpret_cast<int32_t *>(ws + w.owner);
    unsigned long long *claim = reinterpret_cast<unsigned long long *>(ws + w.claim);
    if (first_round == 0) {
        TSIM_HIP_CHECK(hipMemsetAsync(status, 0, 4, st));
        if (T > 0) TSIM_HIP_CHECK(hipMemsetAsync(keep, 0, (size_t)T, st));
        hipLaunchKernelGGL(list_prep_kernel, dim3(1), dim3(LIST_PREP_T), 0, st, C, T, lims, clean, (int32_t *)nullptr);
        TSIM_HIP_CHECK(hipGetLastError());
        const int64_t most = C > N ? C : N;
        hipLaunchKernelGGL(community_init_kernel, dim3((unsigned)std::min<int64_t>((most + 255) / 256, CM_MAX_GRID)), dim3(256), 0, st, C,
                           N, lims, clean, state, owner, claim, accept, status);
        TSIM_HIP_CHECK(hipGetLastError());
    }
    if (C == 0) {
        if (max_rounds > 0) TSIM_HIP_CHECK(hipMemsetAsync(undecided, 0, (size_t)max_rounds * 4, st));
        return TSIM_OK;
    }
    const dim3 grid((unsigned)std::min<int64_t>((C + 3) / 4, CM_MAX_GRID));
    for (int r = 0; r < max_rounds; ++r) {
        const uint32_t rkey = CM_KEY0 - (uint32_t)(first_round + r);
        hipLaunchKernelGGL(community_claim_kernel, grid, dim3(256), 0, st, C, N, clean, members, min_size, rkey, state, owner, claim, status,
                           undecided + r);
        hipLaunchKernelGGL(community_decide_kernel, grid, dim3(256), 0, st, C, N, clean, members, rkey, state, owner, claim, accept, keep,
                           undecided + r);
        TSIM_HIP_CHECK(hipGetLastError());
    }
    return TSIM_OK;
}

extern "C" int tsim_community_select_finish(const int64_t *lims, const int32_t *members, int64_t C, int64_t T, int64_t N, int min_size,
                                            int32_t *accept, uint8_t *keep, int32_t *status, int32_t *undecided, void *workspace,
                                            size_t workspace_bytes, void *stream) {
    using namespace tsim;
    const char *what = "community_select_finish";
    CommunityWs w;
    const int rc = community_check(what, lims, members, C, T, N, min_size, accept, keep, status, undecided, workspace, workspace_bytes, &w);
    if (rc) return rc;
    char *ws = reinterpret_cast<char *>(workspace);
    hipLaunchKernelGGL(community_finish_kernel, dim3(1), dim3(CM_FIN_T), 0, as_stream(stream), C, N,
                       reinterpret_cast<const int64_t *>(ws + w.clean), members, min_size, reinterpret_cast<int32_t *>(ws + w.state),
                       reinterpret_cast<int32_t *>(ws + w.owner), accept, keep, status, undecided);
    TSIM_HIP_CHECK(hipGetLastError());
    return TSIM_OK;
}
