"""Community detection restated in numpy / plain Python, and the case makers of its tests.

``select_ref`` is the literal de-overlap loop of include/tsim.h (the definition), with the house id rules spelled out;
``rounds_model`` is the parallel form of csrc/community_select.h (claim with a minimum, decide from the claims alone) written
round by round; ``detect_ref`` is the whole pipeline — steps 1 to 4 of ops.community_detection — fed a range result."""
import numpy as np

ST_ROW, ST_LIMS = 1, 2


def clean_lims(lims, T):
    """list_prep_kernel: the running maximum clamped to [0, T]."""
    lims = np.asarray(lims, dtype=np.int64)
    return np.clip(np.maximum.accumulate(np.maximum(lims, 0)), 0, T)


def select_ref(lims, members, N, min_size):
    """(accept int32 [C], keep uint8 [T], status): the sequential loop."""
    members = np.asarray(members)
    T, C = len(members), len(lims) - 1
    L = clean_lims(lims, T)
    status = ST_LIMS if (L != np.asarray(lims)).any() else 0
    if (members >= N).any():
        status |= ST_ROW
    accept, keep = np.zeros(C, np.int32), np.zeros(T, np.uint8)
    taken = set()
    for c in range(C):
        free = [t for t in range(L[c], L[c + 1]) if 0 <= members[t] < N and int(members[t]) not in taken]
        if len(free) >= min_size:       # a member listed twice was tested twice and counts twice
            accept[c] = 1
            keep[free] = 1
            taken.update(int(members[t]) for t in free)
    return accept, keep, status


def rounds_model(lims, members, N, min_size, max_rounds=None):
    """(accept, keep, rounds): the parallel form.  Every round: each undecided community counts its members without an owner
    (count < min_size: rejected), offers its rank to claim[j] of each by minimum; then, from the claims alone, a community
    accepts iff every member it claimed carries its own rank.  Stops when nothing is undecided (or after max_rounds, returning
    what is decided so far and the undecided set)."""
    members = np.asarray(members)
    T, C = len(members), len(lims) - 1
    L = clean_lims(lims, T)
    UND, ACC, REJ = 0, 1, 2
    state = np.zeros(C, np.int8)
    owner = np.full(N, -1, np.int64)
    accept, keep = np.zeros(C, np.int32), np.zeros(T, np.uint8)
    rounds = 0
    while (state == UND).any() and (max_rounds is None or rounds < max_rounds):
        rounds += 1
        claim = np.full(N, C, np.int64)
        free_of = {}
        for c in np.nonzero(state == UND)[0]:                      # claim launch: reads owner, writes claim and rejections
            free = [t for t in range(L[c], L[c + 1]) if 0 <= members[t] < N and owner[members[t]] < 0]
            if len(free) < min_size:
                state[c] = REJ
                continue
            free_of[c] = free
            for t in free:
                claim[members[t]] = min(claim[members[t]], c)
        new_owner = owner.copy()
        for c in np.nonzero(state == UND)[0]:                      # decide launch: reads claim only, writes owner
            mine = [t for t in range(L[c], L[c + 1]) if 0 <= members[t] < N and claim[members[t]] < C]
            assert mine == free_of[c]                              # "free" is recoverable from the claims
            if all(claim[members[t]] == c for t in mine):
                state[c] = ACC
                accept[c] = 1
                keep[mine] = 1
                new_owner[members[mine]] = c
        owner = new_owner
    return accept, keep, rounds, np.nonzero(state == UND)[0]


def csr(lists):
    lims = np.zeros(len(lists) + 1, np.int64)
    lims[1:] = np.cumsum([len(x) for x in lists])
    mem = np.concatenate([np.asarray(x, np.int32) for x in lists]) if lists else np.zeros(0, np.int32)
    return lims, mem.astype(np.int32)


def chain_case(n=40, size=12):
    """n communities, each sharing exactly its LAST row with the FIRST row of the next: community i can only be decided after
    community i - 1 (it loses the shared row to it), so the parallel form needs n rounds.  Every one is accepted for
    min_size <= size - 1."""
    lists, base = [], 0
    for _ in range(n):
        lists.append(list(range(base, base + size)))
        base += size - 1
    return lists, base + 1


def random_case(rng, C, N, max_len, dup=False):
    lists = []
    for _ in range(C):
        n = int(rng.integers(0, max_len + 1))
        if rng.random() < 0.5:      # a window of neighbouring rows: communities overlap heavily, as range hits do
            start = int(rng.integers(0, N))
            x = (start + rng.permutation(min(2 * n + 1, N))[:n]) % N
        else:
            x = rng.integers(0, N, size=n) if dup else rng.permutation(N)[:n]
        lists.append(x.astype(np.int32))
    return lists


def detect_ref(lims, scores, idx, N, min_size):
    """Steps 1-4 from a range result of the rows against themselves (``lims, scores, idx`` as ops.cosine_range returns them, on
    the host): (lims [K+1], members [M], centres [K], labels [N], scores [M])."""
    lims, idx, scores = np.asarray(lims), np.asarray(idx), np.asarray(scores)
    cand = [(i, idx[lims[i]:lims[i + 1]], scores[lims[i]:lims[i + 1]]) for i in range(N) if lims[i + 1] - lims[i] >= min_size]
    cand.sort(key=lambda c: (-len(c[1]), c[0]))
    taken, out = set(), []
    for pos, (i, mem, sc) in enumerate(cand):
        free = [t for t in range(len(mem)) if int(mem[t]) not in taken]
        if len(free) >= min_size:
            out.append((pos, i, mem[free], sc[free]))
            taken.update(int(j) for j in mem[free])
    out.sort(key=lambda o: (-len(o[2]), o[0]))
    K = len(out)
    olims = np.zeros(K + 1, np.int64)
    olims[1:] = np.cumsum([len(o[2]) for o in out])
    members = np.concatenate([o[2] for o in out]).astype(np.int64) if K else np.zeros(0, np.int64)
    msc = np.concatenate([o[3] for o in out]).astype(np.float32) if K else np.zeros(0, np.float32)
    centres = np.array([o[1] for o in out], np.int64)
    labels = np.full(N, -1, np.int64)
    for k, o in enumerate(out):
        labels[o[2]] = k
    return olims, members, centres, labels, msc


def planted_rows(d, seed=5, sizes=(20, 35, 50, 70, 95, 120), noise_rows=200, sigma=0.05):
    """Six planted clusters (a centre of unit variance per element + sigma noise per element, as the mixture of
    tools/bench_graph.py, then normalised: members of one cluster score about 1 / (1 + sigma^2) against each other, whatever d) and
    isotropic unit rows (pairs score about N(0, 1/d): 0.75 is more than four deviations out at d = 32), shuffled; returns
    (rows float32 [N, d], planted int64 [N]: the cluster number or -1)."""
    rng = np.random.default_rng(seed)
    parts, lab = [], []
    for k, n in enumerate(sizes):
        c = rng.standard_normal(d)
        parts.append(c[None, :] + sigma * rng.standard_normal((n, d)))
        lab += [k] * n
    parts.append(rng.standard_normal((noise_rows, d)))
    lab += [-1] * noise_rows
    x = np.concatenate(parts)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    p = rng.permutation(len(x))
    return np.ascontiguousarray(x[p].astype(np.float32)), np.asarray(lab, np.int64)[p]
