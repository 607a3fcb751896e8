"""The top-k merge alone and the price of the sharded search's collective on one rank
(diagnostic): per-call HIP-event times over back-to-back calls after a
warm-up, every time [the smallest, the largest] of --rounds timings.

  merge    codec.merge_topk (pqh_topk_merge) at 512 queries x {2, 8} parts x {64, 256} entries a
           part, top_k = the entries of a part, beside the torch formulation of the same result
           in the same process: add the bases, concatenate, sort by (dist, id), slice.  Equality
           of the two is checked first.
  shard    IVF.search of --rows x 128 rows in 1,024 lists (512 queries x 16 probes, k = 64) beside
           the same search followed by shard.search_merge on a one-rank communicator: the
           difference is the pack, the gather (a copy on one rank) and the merge

    python tools/bench_merge.py [--rows 1000000] [--chunk 4] [--reps 50] [--rounds 5]
                                [--out FILE.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from pq_huffman_amd import codec, shard  # noqa: E402


def timed(fn, reps, budget_ms=400.0):
    """ms per call over back-to-back calls; slow calls get fewer than `reps` of them"""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    reps = max(1, min(reps, int(budget_ms / max(e0.elapsed_time(e1), 1e-3))))
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def spread(fn, reps, rounds, scale=1.0):
    """[smallest, largest] of `rounds` timings of fn, each `timed`"""
    t = [scale * timed(fn, reps) for _ in range(rounds)]
    return [min(t), max(t)]


def torch_merge(dist, ids, bases, k):
    """the torch formulation: bases added, parts concatenated, a stable sort by id and then by
    dist (so ties come in id order), the first k; padding is (+inf, -1)"""
    parts, nq, k_in = dist.shape
    moved = torch.where(ids >= 0, ids + bases[:, None, None], ids)
    d = torch.where(ids >= 0, dist, torch.full_like(dist, float("inf")))
    d = d.permute(1, 0, 2).reshape(nq, parts * k_in)
    i = moved.permute(1, 0, 2).reshape(nq, parts * k_in)
    key = torch.where(i >= 0, i, torch.full_like(i, torch.iinfo(torch.int64).max))
    order = key.argsort(dim=1, stable=True)
    d, i = d.gather(1, order), i.gather(1, order)
    order = d.argsort(dim=1, stable=True)[:, :k]
    return d.gather(1, order), i.gather(1, order)


def merge_inputs(parts, nq, k_in, dev, seed=1):
    """every part a sorted top-k_in of its own rows, distances with ties, a tenth padding"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    dist = (torch.randint(0, 4096, (parts, nq, k_in), generator=g).float() / 16.0).sort(dim=2).values
    ids = torch.stack([torch.stack([torch.randperm(100_000, generator=g)[:k_in] for _ in range(nq)])
                       for _ in range(parts)])
    pad = torch.arange(k_in)[None, None, :] >= (k_in - torch.randint(0, k_in // 5 + 1, (parts, nq, 1),
                                                                       generator=g))
    dist[pad], ids[pad] = float("inf"), -1
    bases = torch.arange(parts, dtype=torch.int64) * 100_000
    return dist.to(dev), ids.to(dev), bases.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = codec.Context(0).set_search_max_k(256)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "rounds": a.rounds, "merge": {}}
    nq = 512
    for parts in (2, 8):
        for k_in in (64, 256):
            dist, ids, bases = merge_inputs(parts, nq, k_in, dev)
            out = (torch.empty((nq, k_in), dtype=torch.float32, device=dev),
                   torch.empty((nq, k_in), dtype=torch.int64, device=dev))
            got = codec.merge_topk(ctx, dist, ids, k_in, bases, out=out)
            want = torch_merge(dist, ids, bases, k_in)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (parts, k_in)
            r = res["merge"][f"{parts}x{k_in}"] = {
                "pqh_topk_merge_us": spread(
                    lambda: codec.merge_topk(ctx, dist, ids, k_in, bases, out=out), a.reps,
                    a.rounds, 1e3),
                "torch_us": spread(lambda: torch_merge(dist, ids, bases, k_in), a.reps, a.rounds,
                                   1e3)}
            print(f"merge 512 queries x {parts} parts x {k_in}: pqh_topk_merge "
                  f"{r['pqh_topk_merge_us']} us, torch {r['torch_us']} us", flush=True)

    d, m, n, nlist, nprobe, k = 128, 8, a.rows, 1024, 16, 64
    x = bench.make_data(torch, n, d, 0x5EED, 0, dev)
    q = bench.make_data(torch, nq, d, 0x5EED, 1, dev)
    init = x[torch.arange(nlist, device=dev) * (n // nlist) + 3].contiguous()
    cq = codec.Coarse(ctx, codec.kmeans_train(ctx, x, init.cpu().numpy()[None], 2))
    sample = torch.arange(min(n, 200_000), device=dev) * (n // min(n, 200_000))
    pq = codec.PQ(ctx, bench.train_centroids(torch, x[sample], m, 256))
    sh = shard.ShardedIVF.build(ctx, None, pq, cq, x, chunk_vectors=a.chunk)
    codec.ivf_status(ctx)
    ivf = sh.local

    def sharded():
        dd, ii = ivf.search(q, nprobe, k)
        return shard.search_merge(ctx, sh.comm, dd, ii, sh.id_base)

    md, mi, state = sharded()
    shard.search_status(ctx, state)
    want = torch_merge(*[t[None] for t in ivf.search(q, nprobe, k)],
                       torch.zeros(1, dtype=torch.int64, device=dev), k)
    assert torch.equal(md, want[0]) and torch.equal(mi, want[1])
    res["shard"] = {"rows": n, "nlist": nlist, "nq": nq, "nprobe": nprobe, "top_k": k,
                    "chunk": a.chunk,
                    "ivf_search_ms": spread(lambda: ivf.search(q, nprobe, k), a.reps, a.rounds),
                    "ivf_search_and_search_merge_ms": spread(sharded, a.reps, a.rounds)}
    codec.decode_status(ctx)
    print(f"one rank, {n} rows: IVF.search {res['shard']['ivf_search_ms']} ms, with search_merge "
          f"{res['shard']['ivf_search_and_search_merge_ms']} ms", flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
