"""One rank of the sharded search (shard.ShardedIVF, pqh_shard_search_merge through
shard.search_merge), run by tests/test_gpu_zz_shard_search.py under torch.distributed.run with
the gloo backend and every rank on cuda:0 (a fresh process per rank).  Every rank builds the
index of its row block of the same 3001 rows and searches; rank 0 writes every rank's merged
result to --out (.npz) for the test to compare with the numpy references.

  --case plain|residual|wide|masked|removed|fail
wide: k = 100 on a context raised to 256; masked: keep= leaves rank 1 nothing, so its record is
all padding; removed: remove() of global ids in both blocks, then live_count(); fail: rank 1
passes a non-zero status -- both ranks must return from the collective with padding, and
search_status must report the failure on rank 0."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

N, D, NLIST, NPROBE, NQ = 3001, 32, 16, 4, 5


def world_of(case):
    import merge_ref as mref
    res = case == "residual"
    return mref.search_world(N, D, NLIST, NQ, 8 if res else 4, residual=res, spread=True)


def masks(starts):
    """(keep over the global ids that leaves the second block nothing, removed global ids of
    both blocks)"""
    rng = np.random.default_rng(21)
    keep = rng.random(N) < 0.5
    keep[starts[1]:starts[2]] = False
    return keep, rng.choice(N, 400, replace=False).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="plain")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch
    import torch.distributed as dist
    from pq_huffman_amd import codec, shard
    from pq_huffman_amd.capi import PqhError

    dist.init_process_group("gloo")
    world, rank = dist.get_world_size(), dist.get_rank()
    torch.cuda.set_device(0)
    w = world_of(a.case)
    ctx = codec.Context(0)
    k = 10
    if a.case == "wide":
        ctx.set_search_max_k(256)
        k = 100
    b, e = shard.row_range(N, world, rank)
    starts = [shard.row_range(N, world, r)[0] for r in range(world)] + [N]
    pq, coarse = codec.PQ(ctx, w["cent"]), codec.Coarse(ctx, w["cc"])
    comm = shard.TorchComm(world, rank)
    xd = torch.from_numpy(np.ascontiguousarray(w["x"][b:e])).cuda()
    qd = torch.from_numpy(w["q"]).cuda()
    ivf = shard.ShardedIVF.build(ctx, comm, pq, coarse, xd, chunk_vectors=8,
                                 residual=a.case == "residual")
    assert (ivf.id_base, ivf.n_total, ivf.local.n_ids) == (b, N, e - b)
    extra = {}
    if a.case == "fail":
        d, i = ivf.local.search(qd, NPROBE, k)
        md, mi, state = shard.search_merge(ctx, comm, d, i, ivf.id_base, status=-3 if rank == 1 else 0)
        try:
            shard.search_status(ctx, state)
            raise AssertionError(f"rank {rank} did not see the failure")
        except PqhError as err:
            assert err.status == -9 and "another rank" in str(err), str(err)
        extra["failed"] = np.int64(1)
    else:
        kw = {}
        keep, gone = masks(starts)
        if a.case == "masked":
            kw["keep"] = torch.from_numpy(keep).cuda()
        if a.case == "removed":
            ivf.remove(torch.from_numpy(gone).cuda())
            extra["live"] = np.int64(ivf.live_count())
        md, mi = ivf.search(qd, NPROBE, k, **kw)
        if a.case == "masked" and rank == 1:       # this rank's own record was all padding
            assert (ivf.local.search(qd, NPROBE, k, keep=kw["keep"][b:e])[1] == -1).all()
    torch.cuda.synchronize()
    codec.decode_status(ctx)
    codec.ivf_status(ctx)
    every = [None] * world
    dist.all_gather_object(every, (md.cpu().numpy(), mi.cpu().numpy()))
    if rank == 0:
        np.savez(a.out, dist=np.stack([r[0] for r in every]), ids=np.stack([r[1] for r in every]),
                 **extra)
    dist.barrier()
    ctx.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
