"""Two ranks, the real HIP kernels: ShardedCorpusSearch.range_search over torch.distributed must return, on every rank, exactly
the one-GPU ops.cosine_range over the concatenated corpus — lims, scores and indices bit for bit — for one selective threshold
and for a per-query threshold array.  As in tests/test_sharded_gpu.py both ranks share cuda:0, the collectives run on gloo
(device tensors staged through host memory) and the ranks come from multiprocessing's fork server, which conftest.py starts
before anything touches the GPU.  n_total = 30 001 (shards of 15 001 / 15 000), Q = 65 (33 / 32: padded for the exchange, the
padding dropped), d = 384.  Two children open the GPU, the parent only after both have left."""
import multiprocessing as mp
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N_TOTAL, Q_TOTAL, D = 30001, 65, 384
TAU = 0.17          # cosines of Gaussian rows at d = 384 are ~ N(0, 1/384): 3.3 sigma, about 15 of 30 001 rows per query
CHILD_TIME_LIMIT = 240


def _data():
    rng = np.random.default_rng(2025)
    corpus = (rng.standard_normal((N_TOTAL, D)) * np.exp(rng.uniform(-1, 1, (N_TOTAL, 1)))).astype(np.float32)
    queries = rng.standard_normal((Q_TOTAL, D)).astype(np.float32)
    corpus[N_TOTAL - 1] = corpus[3] * 2.0        # same direction on the LAST shard: equal cosine, ordered by index across ranks
    queries[0] = corpus[3]
    tau = np.full(Q_TOTAL, TAU, np.float32)
    tau[1::7] = 0.14
    tau[2::7] = 0.2
    tau[3] = -np.inf                             # every row of both shards
    tau[4] = np.inf
    tau[40] = np.nan
    tau[64] = 0.05                               # the last query (alone in no slice): thousands of hits, the exact pass
    return corpus, queries, tau


def _rank_main(rank, world, port, out_dir):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from text_similarity_amd import ops
        from text_similarity_amd.distributed.sharded_search import ShardedCorpusSearch, shard_bounds
        dev = torch.device("cuda:0")
        torch.cuda.set_device(dev)
        corpus, queries, tau = _data()
        lo, hi = shard_bounds(N_TOTAL, world, rank)
        cf = torch.from_numpy(corpus[lo:hi]).to(dev)
        cu, rho = ops.l2norm_rows(cf, return_rho=True)
        eng = ShardedCorpusSearch(cu, D, lo, corpus_f32_local=cf, corpus_rho=rho)
        qlo, qhi = shard_bounds(Q_TOTAL, world, rank)
        counts = [shard_bounds(Q_TOTAL, world, r)[1] - shard_bounds(Q_TOTAL, world, r)[0] for r in range(world)]
        q_local = torch.from_numpy(queries[qlo:qhi]).to(dev)
        out = {}
        for name, thr in (("scalar", TAU), ("array", torch.from_numpy(tau[qlo:qhi].copy()).to(dev))):
            lims, s, i = eng.range_search(q_local, thr, counts=counts)
            torch.cuda.synchronize()
            out.update({f"{name}_lims": lims.cpu().numpy(), f"{name}_s": s.cpu().numpy(), f"{name}_i": i.cpu().numpy()})
        np.savez(os.path.join(out_dir, f"r{rank}.npz"), **out)
    finally:
        dist.destroy_process_group()


def test_two_ranks_range_search_equals_one_gpu(tmp_path):
    world = 2
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("forkserver")
    procs = [ctx.Process(target=_rank_main, args=(r, world, port, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    codes = []
    for p in procs:
        p.join(CHILD_TIME_LIMIT)
        codes.append(p.exitcode)
    for p in procs:                              # a rank past its time limit is ended; nothing is started after a failure
        if p.exitcode is None:
            p.kill()
            p.join()
    assert codes == [0] * world, f"rank exit codes {codes} (None: time limit of {CHILD_TIME_LIMIT} s)"
    import torch
    from text_similarity_amd import ops
    corpus, queries, tau = _data()
    cf, qf = torch.from_numpy(corpus).to("cuda:0"), torch.from_numpy(queries).to("cuda:0")
    qn, cn = ops.l2norm_rows(qf), ops.l2norm_rows(cf)
    for name, thr in (("scalar", TAU), ("array", torch.from_numpy(tau).to("cuda:0"))):
        ref_lims, ref_s, ref_i = (t.cpu().numpy() for t in ops.cosine_range(qn, cn, D, thr, eq_f32=qf, ec_f32=cf))
        assert ref_i[0] == 3 and ref_i[1] == N_TOTAL - 1 and ref_s[0].view(np.uint32) == ref_s[1].view(np.uint32)
        sizes = np.diff(ref_lims)
        assert ref_lims.shape == (Q_TOTAL + 1,) and 5 * Q_TOTAL < ref_lims[-1]
        if name == "array":
            assert sizes[3] == N_TOTAL and sizes[4] == 0 and sizes[40] == 0 and sizes[64] > 2048
        for r in range(world):
            got = np.load(tmp_path / f"r{r}.npz")
            np.testing.assert_array_equal(got[f"{name}_lims"], ref_lims)
            np.testing.assert_array_equal(got[f"{name}_i"], ref_i)
            np.testing.assert_array_equal(got[f"{name}_s"].view(np.uint32), ref_s.view(np.uint32))
