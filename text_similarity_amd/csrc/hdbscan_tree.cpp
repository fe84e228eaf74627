// Host-side tree stage of HDBSCAN (C ABI: include/tsim.h "HDBSCAN"): from the N - 1 edges of the mutual-reachability minimum
// spanning tree (tsim_mst_prim, squared weights) to one label per row.  It restates the tree stage of scikit-learn's
// sklearn.cluster.HDBSCAN / the hdbscan package (third-party dependencies of the reference's topic pipeline,
// /root/reference/src/pipeline/topic_modeling.py, not vendored in it; the published algorithm: Campello, Moulavi, Sander 2013)
// for cluster_selection_method="eom", allow_single_cluster=False, cluster_selection_epsilon=0:
//   single linkage   edges by (w2 asc, step asc), union-find; merge k is node N + k = (component of from, component of to);
//   condensed tree   breadth-first from the root, left before right; lambda = 1 / distance; children below min_cluster_size
//                    shed their rows; two large children become two new clusters, left first;
//   stability        sum of (lambda - birth) size over a cluster's condensed rows, float64, in row order;
//   selection        descending cluster number, the root excluded: children's summed stability strictly greater -> take the sum
//                    and unselect, else unselect the descendants;
//   labels           the rank of the nearest selected ancestor-or-self of the cluster a row fell out of, or -1.
// O(N log N) for the sort, O(N) for the rest.  tests/hdbscan_cases.tree_labels_ref is the numpy restatement this file is
// tested against; tests/hdbscan_tree_driver.cpp runs it under the sanitizers.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <vector>

#include "tsim.h"

namespace {

// float32 -> a key whose unsigned order is the numeric order; -0 as +0; every NaN last (numpy's stable argsort)
uint32_t order_key(float v) {
    if (v != v) return 0xffffffffu;
    if (v == 0.f) v = 0.f;
    uint32_t u;
    memcpy(&u, &v, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

struct CondensedRow {
    int64_t parent, child;   // parent: a cluster number (>= N); child: a row (< N) or a cluster number
    double lambda;
    int64_t size;
};

}  // namespace

extern "C" int tsim_hdbscan_tree_labels(const int32_t *from, const int32_t *to, const float *w2, int64_t N, int min_cluster_size,
                                        int32_t *out_labels, int32_t *out_n_clusters) {
    if (N < 1 || N >= (1ll << 31) - 64 || min_cluster_size < 2 || !out_labels || !out_n_clusters) return TSIM_EINVAL;
    if (N > 1 && (!from || !to || !w2)) return TSIM_EINVAL;
    const int64_t E = N - 1;
    // 1. single linkage
    std::vector<int64_t> order((size_t)E);
    for (int64_t e = 0; e < E; ++e) order[(size_t)e] = e;
    std::stable_sort(order.begin(), order.end(),
                     [&](int64_t a, int64_t b) { return order_key(w2[a]) < order_key(w2[b]); });
    std::vector<int64_t> uf((size_t)N), node_of((size_t)N), left((size_t)E), right((size_t)E), size((size_t)E);
    std::vector<double> dist((size_t)E);
    for (int64_t i = 0; i < N; ++i) uf[(size_t)i] = node_of[(size_t)i] = i;
    auto find = [&](int64_t x) {
        int64_t r = x;
        while (uf[(size_t)r] != r) r = uf[(size_t)r];
        while (uf[(size_t)x] != r) {
            const int64_t nx = uf[(size_t)x];
            uf[(size_t)x] = r;
            x = nx;
        }
        return r;
    };
    auto count = [&](int64_t node) { return node < N ? (int64_t)1 : size[(size_t)(node - N)]; };
    for (int64_t k = 0; k < E; ++k) {
        const int64_t e = order[(size_t)k];
        const int64_t a = from[e], b = to[e];
        if (a < 0 || a >= N || b < 0 || b >= N) return TSIM_EINVAL;
        const int64_t ra = find(a), rb = find(b);
        if (ra == rb) return TSIM_EINVAL;   // a cycle: N - 1 merges of distinct components are a spanning tree
        const int64_t na = node_of[(size_t)ra], nb = node_of[(size_t)rb];
        left[(size_t)k] = na;
        right[(size_t)k] = nb;
        dist[(size_t)k] = sqrt((double)w2[e]);
        size[(size_t)k] = count(na) + count(nb);
        uf[(size_t)rb] = ra;
        node_of[(size_t)ra] = N + k;
    }
    for (int64_t i = 0; i < N; ++i) out_labels[i] = -1;
    *out_n_clusters = 0;
    if (N == 1) return TSIM_OK;

    // 2. condensed tree
    const int64_t root = 2 * N - 2;
    const double INF = std::numeric_limits<double>::infinity();
    std::vector<int64_t> relabel((size_t)(root + 1), -1);
    std::vector<uint8_t> ignore((size_t)(root + 1), 0);
    std::vector<CondensedRow> rows;
    rows.reserve((size_t)N + 64);
    std::vector<int64_t> queue, sub;
    queue.reserve((size_t)(root + 1));
    queue.push_back(root);
    for (size_t h = 0; h < queue.size(); ++h) {   // breadth-first, left before right
        const int64_t node = queue[h];
        if (node >= N) {
            queue.push_back(left[(size_t)(node - N)]);
            queue.push_back(right[(size_t)(node - N)]);
        }
    }
    int64_t next_label = N + 1;
    relabel[(size_t)root] = N;
    auto shed = [&](int64_t top, int64_t cluster, double lambda) {   // every row below `top` leaves `cluster` at lambda
        sub.clear();
        sub.push_back(top);
        for (size_t h = 0; h < sub.size(); ++h) {
            const int64_t s = sub[h];
            if (s >= N) {
                sub.push_back(left[(size_t)(s - N)]);
                sub.push_back(right[(size_t)(s - N)]);
            } else {
                rows.push_back({cluster, s, lambda, 1});
            }
            ignore[(size_t)s] = 1;
        }
    };
    for (const int64_t node : queue) {
        if (node < N || ignore[(size_t)node]) continue;
        const int64_t l = left[(size_t)(node - N)], r = right[(size_t)(node - N)];
        const double d = dist[(size_t)(node - N)];
        const double lambda = d > 0.0 ? 1.0 / d : INF;
        const int64_t lc = count(l), rc = count(r), me = relabel[(size_t)node];
        if (lc >= min_cluster_size && rc >= min_cluster_size) {
            relabel[(size_t)l] = next_label++;
            rows.push_back({me, relabel[(size_t)l], lambda, lc});
            relabel[(size_t)r] = next_label++;
            rows.push_back({me, relabel[(size_t)r], lambda, rc});
        } else if (lc < min_cluster_size && rc < min_cluster_size) {
            shed(l, me, lambda);
            shed(r, me, lambda);
        } else if (lc < min_cluster_size) {
            relabel[(size_t)r] = me;
            shed(l, me, lambda);
        } else {
            relabel[(size_t)l] = me;
            shed(r, me, lambda);
        }
    }

    // 3. stability
    const int64_t C = next_label - N;   // clusters N .. N + C - 1, the root first
    std::vector<double> birth((size_t)C, 0.0), stab((size_t)C, 0.0);
    std::vector<int64_t> cparent((size_t)C, -1), kid0((size_t)C, -1), kid1((size_t)C, -1);
    for (const CondensedRow &row : rows)
        if (row.child >= N) {
            const int64_t c = row.child - N, p = row.parent - N;
            birth[(size_t)c] = row.lambda;
            cparent[(size_t)c] = p;
            (kid0[(size_t)p] < 0 ? kid0 : kid1)[(size_t)p] = c;   // (row order: left, then right)
        }
    birth[0] = 0.0;
    for (const CondensedRow &row : rows) {
        const size_t p = (size_t)(row.parent - N);
        stab[p] += (row.lambda - birth[p]) * (double)row.size;
    }

    // 4. selection
    std::vector<uint8_t> selected((size_t)C, 1);
    selected[0] = 0;
    for (int64_t c = C - 1; c >= 1; --c) {
        double subtree = 0.0;
        if (kid0[(size_t)c] >= 0) subtree = stab[(size_t)kid0[(size_t)c]] + stab[(size_t)kid1[(size_t)c]];
        if (subtree > stab[(size_t)c]) {
            selected[(size_t)c] = 0;
            stab[(size_t)c] = subtree;
        } else {
            sub.clear();
            if (kid0[(size_t)c] >= 0) {
                sub.push_back(kid0[(size_t)c]);
                sub.push_back(kid1[(size_t)c]);
            }
            for (size_t h = 0; h < sub.size(); ++h) {
                const int64_t s = sub[h];
                selected[(size_t)s] = 0;
                if (kid0[(size_t)s] >= 0) {
                    sub.push_back(kid0[(size_t)s]);
                    sub.push_back(kid1[(size_t)s]);
                }
            }
        }
    }

    // 5. labels: the nearest selected ancestor-or-self, resolved top-down (a parent's number is below its children's)
    std::vector<int32_t> label_of((size_t)C, -1);
    int32_t n_sel = 0;
    for (int64_t c = 1; c < C; ++c) {
        if (selected[(size_t)c]) label_of[(size_t)c] = n_sel++;
        else label_of[(size_t)c] = label_of[(size_t)cparent[(size_t)c]];
    }
    for (const CondensedRow &row : rows)
        if (row.child < N) out_labels[row.child] = label_of[(size_t)(row.parent - N)];
    *out_n_clusters = n_sel;
    return TSIM_OK;
}
