"""Two ranks at k = 100 (k > 64: tsim_cosine_topk_large per shard, then the sort-and-merge form of tsim_topk_merge_strided on the
all-gathered candidates): ShardedCorpusSearch must return, on every rank, exactly the single-GPU result over the concatenated
corpus.  The harness of tests/test_sharded_gpu.py: both ranks share cuda:0, gloo collectives, ranks started from the fork server
conftest.py launches before anything touches the GPU."""
import multiprocessing as mp
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _data(n_total, q_total, d):
    rng = np.random.default_rng(2025)
    corpus = (rng.standard_normal((n_total, d)) * np.exp(rng.uniform(-1, 1, (n_total, 1)))).astype(np.float32)
    queries = rng.standard_normal((q_total, d)).astype(np.float32)
    corpus[n_total - 1] = corpus[3] * 2.0        # same direction on the LAST shard: equal cosine, tie -> row 3 first
    queries[0] = corpus[3]
    return corpus, queries


def _rank_main(rank, world, port, n_total, q_total, d, k, out_dir):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from text_similarity_amd import ops
        from text_similarity_amd.distributed.sharded_search import ShardedCorpusSearch, shard_bounds
        dev = torch.device("cuda:0")
        torch.cuda.set_device(dev)
        corpus, queries = _data(n_total, q_total, d)
        lo, hi = shard_bounds(n_total, world, rank)
        cf = torch.from_numpy(corpus[lo:hi]).to(dev)
        cu, rho = ops.l2norm_rows(cf, return_rho=True)
        eng = ShardedCorpusSearch(cu, d, lo, corpus_f32_local=cf, corpus_rho=rho)
        ql = q_total // world
        s, i = eng.search(torch.from_numpy(queries[rank * ql:(rank + 1) * ql]).to(dev), k)
        torch.cuda.synchronize()
        np.savez(os.path.join(out_dir, f"r{rank}.npz"), s=s.cpu().numpy(), i=i.cpu().numpy())
    finally:
        dist.destroy_process_group()


def test_two_ranks_k100_equal_one_gpu(tmp_path):
    import torch
    from oracle.search_ref import cosine_topk_f32
    from text_similarity_amd import ops
    world, n_total, q_total, d, k = 2, 30001, 64, 384, 100
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("forkserver")
    procs = [ctx.Process(target=_rank_main, args=(r, world, port, n_total, q_total, d, k, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
        assert p.exitcode == 0, f"rank exited with {p.exitcode}"
    corpus, queries = _data(n_total, q_total, d)
    cf, qf = torch.from_numpy(corpus).to("cuda:0"), torch.from_numpy(queries).to("cuda:0")
    ref_s, ref_i = ops.cosine_topk(ops.l2norm_rows(qf), ops.l2norm_rows(cf), d, k, eq_f32=qf, ec_f32=cf)
    ref_s, ref_i = ref_s.cpu().numpy(), ref_i.cpu().numpy()
    assert ref_i[0, 0] == 3 and ref_i[0, 1] == n_total - 1
    os_, oi = cosine_topk_f32(queries[:2], corpus, k)                 # and the one-GPU result is the oracle's
    np.testing.assert_array_equal(ref_i[:2], oi)
    np.testing.assert_array_equal(ref_s[:2], os_)
    for r in range(world):
        got = np.load(tmp_path / f"r{r}.npz")
        np.testing.assert_array_equal(got["i"], ref_i)
        np.testing.assert_array_equal(got["s"], ref_s)
