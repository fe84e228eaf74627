"""CPU checks of bench.py --dump-outputs: what is written, in which dtypes, and the seeded row sample beyond the size cap."""
import os

import numpy as np
import torch

import bench


def _outputs(q, k=10, d=384, n=1_000_000):
    g = torch.Generator().manual_seed(0)
    return (torch.randn((q, k), generator=g), torch.randint(0, n, (q, k), generator=g),
            torch.randn((q, d), generator=g))


def test_dump_writes_every_output_exactly(tmp_path):
    s, i, e = _outputs(64)
    info = bench.dump_outputs(str(tmp_path), s, i, e)
    assert info["arrays"] == {"scores": [64, 10], "indices": [64, 10], "embeddings": [64, 384]}
    got = {n: np.load(tmp_path / f"{n}.npy") for n in info["arrays"]}
    assert got["scores"].dtype == np.float32 and np.array_equal(got["scores"], s.numpy())
    assert got["indices"].dtype == np.float64 and np.array_equal(got["indices"], i.numpy())
    assert got["embeddings"].dtype == np.float32 and np.array_equal(got["embeddings"], e.numpy())


def test_dump_samples_the_same_rows_under_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 256 << 10)
    s, i, e = _outputs(1000)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), s, i, e)
        assert sum(os.path.getsize(tmp_path / run / f) for f in os.listdir(tmp_path / run)) <= 256 << 10
    rows = np.load(tmp_path / "a" / "query_rows.npy")
    assert 0 < len(rows) < 1000 and np.array_equal(rows, np.load(tmp_path / "b" / "query_rows.npy"))
    r = rows.astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "a" / "embeddings.npy"), e.numpy()[r])
    assert np.array_equal(np.load(tmp_path / "a" / "indices.npy"), i.numpy()[r])
    assert np.array_equal(np.load(tmp_path / "a" / "scores.npy"), s.numpy()[r])
