"""IVF-Flat beside the routes a caller had (diagnostic):
codec.IVFFlat.search over the probed lists of `--rows` bench rows, codec.Flat.search over all the
rows (the only exact answer before it: the gate) and codec.IVF.search(schedule="auto") over the
same lists (the compressed alternative).  The methods alternate `--rounds` times after a warm-up,
each timing HIP events over back-to-back calls, the best of the rounds reported.  Beside the times:
the scan kernel alone (flat_search_lists on ready probes) and its pair-steps per second, and
recall@10 of IVFFlat and IVF against Flat at nprobe 1, 4, 16, 64.

  points   1,024 lists: (512 queries, 16 probes), (1, 16), (4,096, 64); 4,096 lists: (512, 16)

    python tools/bench_flat_lists.py [--rows 1000000] [--reps 20] [--rounds 3] [--out FILE.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from bench_flat import timed  # noqa: E402
from pq_huffman_amd import codec  # noqa: E402


def recall(ids, exact):
    hit = (ids[:, :, None] == exact[:, None, :]).any(dim=2).float().sum(dim=1)
    return float((hit / exact.shape[1]).mean().item())


def point(ctx, flat, index, ivf, q, nprobe, k, reps, rounds):
    """one point: the methods alternating, the best of `rounds`"""
    d = index.x_sorted.shape[1]
    probes = index.coarse.probe(q, nprobe, index.offsets)[2]
    methods = {"ivfflat_ms": lambda: index.search(q, nprobe, k),
               "flat_ms": lambda: flat.search(q, k),
               "ivf_adc_ms": lambda: ivf.search(q, nprobe, k, schedule="auto"),
               "scan_ms": lambda: codec.flat_search_lists(ctx, index.x_sorted, index.offsets, probes, q, k)}
    for fn in methods.values():   # the warm-up
        fn()
    torch.cuda.synchronize()
    res = {"n": index.n, "d": d, "nlist": index.coarse.nlist, "nq": q.shape[0], "nprobe": nprobe, "k": k}
    times = {name: [] for name in methods}
    for _ in range(rounds):
        for name, fn in methods.items():
            times[name].append(timed(fn, reps))
    for name, t in times.items():
        res[name] = min(t)
        res[name + "_all"] = t
    sizes = index.offsets[1:] - index.offsets[:-1]
    res["pair_rows"] = int(sizes[probes.clamp(min=0)].sum().item())   # (query, row) pairs scored
    res["pair_steps_per_s"] = res["pair_rows"] * d / (res["scan_ms"] * 1e-3)
    res["speedup_over_flat"] = res["flat_ms"] / res["ivfflat_ms"]
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = codec.Context(0)
    n, d, k = a.rows, 128, 64
    x = bench.make_data(torch, n, d, 0x5EED, 0, dev)
    q = bench.make_data(torch, 4096, d, 0x5EED, 1, dev)
    flat = codec.Flat(ctx, x)
    sample = torch.arange(min(n, 200_000), device=dev) * (n // min(n, 200_000))
    pq = codec.PQ(ctx, bench.train_centroids(torch, x[sample], 8, 256))
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "rounds": a.rounds,
           "points": {}, "recall_at_10": {}}
    for nlist, shapes in ((1024, ((512, 16), (1, 16), (4096, 64))), (4096, ((512, 16),))):
        init = x[torch.arange(nlist, device=dev) * (n // nlist) + 3].contiguous()
        cq = codec.Coarse(ctx, codec.kmeans_train(ctx, x, init.cpu().numpy()[None], 2))
        index = codec.IVFFlat.build(ctx, cq, x)
        ivf = codec.IVF.build(ctx, pq, cq, x, chunk_vectors=4, context=True)
        codec.ivf_status(ctx)
        for nq, nprobe in shapes:
            res["points"][f"nlist{nlist}_nq{nq}_nprobe{nprobe}"] = point(
                ctx, flat, index, ivf, q[:nq], nprobe, k, a.reps, a.rounds)
        if nlist == 1024:   # what the coarse quantizer loses, and what the PQ loses below it
            exact = flat.search(q[:512], 10)[1]
            for nprobe in (1, 4, 16, 64):
                res["recall_at_10"][f"nprobe{nprobe}"] = {
                    "ivfflat": recall(index.search(q[:512], nprobe, 10)[1], exact),
                    "ivf_adc": recall(ivf.search(q[:512], nprobe, 10)[1], exact)}
            print(json.dumps(res["recall_at_10"]), flush=True)
        codec.ivf_status(ctx)
        del index, ivf
        cq.close()
    flat.close()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write("\n")


if __name__ == "__main__":
    main()
