"""Writes tests/golden/hdbscan.npz: the rows, the parameters and scikit-learn's labels of the HDBSCAN parity cases.

    python tools/make_hdbscan_golden.py

Needs scikit-learn (the fixture was written with 1.7.2).  Every case is Gaussian blobs with separated centres and a tenth of
uniform noise (tests/hdbscan_cases.blobs); the labels are ``sklearn.cluster.HDBSCAN(min_cluster_size, min_samples,
algorithm="brute").fit(rows as float64).labels_``.  The restatement (tests/hdbscan_cases.hdbscan_ref: float32 squared distances,
ties by step) must give the SAME labels, numbering included, for a case to be written — the assertion below is exact; a case
that fails it gets another seed in hdbscan_cases.GOLDEN_CASES, never a looser comparison.  On overlapping blobs a few labels
may differ from scikit-learn (float32 against float64 distances, the order among tied merges): parity is pinned here, on
separated clusters, and the restatement is the definition elsewhere (HDBSCAN)."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import hdbscan_cases as hc    # noqa: E402


def main():
    import sklearn
    from sklearn.cluster import HDBSCAN
    out = {"sklearn_version": np.array(sklearn.__version__), "n_cases": np.array(len(hc.GOLDEN_CASES), dtype=np.int64)}
    for i in range(len(hc.GOLDEN_CASES)):
        rows, mcs, ms = hc.golden_case(i)
        sk = HDBSCAN(min_cluster_size=mcs, min_samples=ms, algorithm="brute").fit(rows.astype(np.float64)).labels_
        labels, n_clusters, _, _ = hc.hdbscan_ref(rows, mcs, ms)
        assert np.array_equal(labels, sk), (i, int((labels != sk).sum()))
        assert n_clusters == int(sk.max()) + 1 >= 2 and (sk == -1).any()
        out[f"rows_{i}"] = np.array(rows)
        out[f"params_{i}"] = np.array([mcs, ms], dtype=np.int64)
        out[f"labels_{i}"] = sk.astype(np.int32)
        print(f"case {i}: {rows.shape[0]} x {rows.shape[1]}, min_cluster_size {mcs}, min_samples {ms}: {n_clusters} clusters, "
              f"{int((sk == -1).sum())} noise rows")
    np.savez_compressed(hc.GOLDEN, **out)
    print(hc.GOLDEN, os.path.getsize(hc.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
