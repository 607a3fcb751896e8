"""The exact re-rank (diagnostic): codec.rerank on ready candidates
beside what a caller without it writes in torch -- gather the candidates' rows, decode SQ8 codes,
(row - q)^2 summed, then a sort by (dist, id) -- at nq in {1, 512, 4,096} x c in {64, 256} x
stores f32, bf16 and sq8 of `--rows` x 128 bench rows in 1,024 lists, k = 10, L2.  Beside them
IVF.search(rerank=c) and IVF.search(k=c) (their difference is what the re-rank adds) and
IVF.search(refine=c) on the same index with a 16 x 256 second code.  The methods alternate
`--rounds` times after a warm-up, each timing HIP events over back-to-back calls, the best of
the rounds reported, every round kept.  At every point the kernel's output for eight of the
queries is checked against tests/rerank_ref.py, ids and bits.  Then recall@10 against Flat (512
queries, nprobe 16) without a second stage, with refine= and with rerank= over the three stores.

    python tools/bench_rerank.py [--rows 1000000] [--reps 20] [--rounds 3] [--out FILE.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import rerank_ref  # noqa: E402
from bench_flat import timed  # noqa: E402
from bench_flat_lists import recall  # noqa: E402
from pq_huffman_amd import codec  # noqa: E402


def torch_rerank(store, q, cand, k):
    """the caller's code: the same result in another arithmetic and in several launches"""
    at = cand.clamp(min=0)
    rows = store[at].float() if not isinstance(store, tuple) else \
        store[0].vmin + store[1][at][:, :, :store[0].d].float() * store[0].step
    dist = ((rows - q[:, None]) ** 2).sum(-1)
    dist[cand < 0] = float("inf")
    o = cand.argsort(dim=1, stable=True)
    dist, ids = dist.gather(1, o), cand.gather(1, o)
    o = dist.argsort(dim=1, stable=True)
    return dist.gather(1, o)[:, :k], ids.gather(1, o)[:, :k]


def checked(ctx, store, host, q, cand, k):
    """eight queries of the point against the reference, ids and bits; host: the store's numpy
    twin (rows as float32, or (codes, (vmin, step)))"""
    pick = torch.linspace(0, q.shape[0] - 1, min(8, q.shape[0])).long().to(q.device)
    got = codec.rerank(ctx, store, q[pick].contiguous(), cand[pick].contiguous(), k)
    x, sq = host if isinstance(host, tuple) else (host, None)
    want = rerank_ref.rerank(q[pick].cpu().numpy(), x, cand[pick].cpu().numpy(), k, "l2", sq)
    return bool(np.array_equal(got[1].cpu().numpy(), want[1]) and
                np.array_equal(got[0].cpu().numpy().view(np.uint32), want[0].view(np.uint32)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = codec.Context(0).set_search_max_k(256)
    n, d, k, nlist, nprobe = a.rows, 128, 10, 1024, 16
    x = bench.make_data(torch, n, d, 0x5EED, 0, dev)
    q_all = bench.make_data(torch, 4096, d, 0x5EED, 1, dev)
    sample = x[torch.arange(min(n, 200_000), device=dev) * (n // min(n, 200_000))]
    pq = codec.PQ(ctx, bench.train_centroids(torch, sample, 8, 256))
    pq2 = codec.PQ(ctx, bench.train_centroids(torch, codec.pq_residuals(ctx, pq, sample), 16, 256))
    init = x[torch.arange(nlist, device=dev) * (n // nlist) + 3].contiguous()
    cq = codec.Coarse(ctx, codec.kmeans_train(ctx, x, init.cpu().numpy()[None], 2))
    ivf = codec.IVF.build(ctx, pq, cq, x, chunk_vectors=4, context=True, refine_pq=pq2)
    sq = codec.SQ.train(ctx, x)
    stores = {"f32": x, "bf16": x.to(torch.bfloat16), "sq8": (sq, sq.encode(x))}
    hosts = {"f32": x.cpu().numpy(), "bf16": stores["bf16"].float().cpu().numpy(),
             "sq8": (stores["sq8"][1].cpu().numpy()[:, :d], (sq.vmin.cpu().numpy(), sq.step.cpu().numpy()))}
    bytes_row = {"f32": 4 * d, "bf16": 2 * d, "sq8": d}
    codec.ivf_status(ctx)
    res = {"device": torch.cuda.get_device_name(0), "rows": n, "reps": a.reps, "rounds": a.rounds,
           "points": {}}
    for nq in (1, 512, 4096):
        q = q_all[:nq].contiguous()
        for c in (64, 256):
            cand = ivf.search(q, nprobe, c)[1].contiguous()
            for name, store in stores.items():
                ivf.set_rows(store)
                methods = {"kernel_ms": lambda: codec.rerank(ctx, store, q, cand, k),
                           "torch_ms": lambda: torch_rerank(store, q, cand, k),
                           "search_rerank_ms": lambda: ivf.search(q, nprobe, k, rerank=c),
                           "search_k_c_ms": lambda: ivf.search(q, nprobe, c),
                           "search_refine_ms": lambda: ivf.search(q, nprobe, k, refine=c)}
                for fn in methods.values():   # the warm-up
                    fn()
                torch.cuda.synchronize()
                times = {m: [] for m in methods}
                for _ in range(a.rounds):
                    for m, fn in methods.items():
                        times[m].append(timed(fn, a.reps))
                p = {"nq": nq, "c": c, "store": name, "equals_reference": checked(ctx, store, hosts[name], q, cand, k)}
                for m, t in times.items():
                    p[m], p[m + "_all"] = min(t), t
                p["rerank_adds_ms"] = p["search_rerank_ms"] - p["search_k_c_ms"]
                p["torch_over_kernel"] = p["torch_ms"] / p["kernel_ms"]
                valid = int((cand >= 0).sum().item())
                p["gathered_gb_per_s"] = valid * bytes_row[name] / (p["kernel_ms"] * 1e6)
                res["points"][f"nq{nq}_c{c}_{name}"] = p
                print(json.dumps(p), flush=True)
    flat = codec.Flat(ctx, x)
    q = q_all[:512].contiguous()
    exact = flat.search(q, 10)[1]
    rec = {"none": recall(ivf.search(q, nprobe, 10)[1], exact)}
    for c in (64, 256):
        rec[f"refine{c}"] = recall(ivf.search(q, nprobe, 10, refine=c)[1], exact)
        for name, store in stores.items():
            ivf.set_rows(store)
            rec[f"rerank{c}_{name}"] = recall(ivf.search(q, nprobe, 10, rerank=c)[1], exact)
    flat.close()
    codec.ivf_status(ctx)
    res["recall_at_10"] = rec
    print(json.dumps({"recall_at_10": rec}), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write("\n")


if __name__ == "__main__":
    main()
