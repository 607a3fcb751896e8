"""IVF-SQ8 beside IVF-Flat (diagnostic): codec.IVFSQ.search and
codec.IVFFlat.search over the same quantizer, lists and queries of `--rows` bench rows.  The
methods alternate `--rounds` times after a warm-up, each timing HIP events over back-to-back
calls, the best of the rounds reported; beside them the two scan kernels alone on ready probes.
Then recall@10 of both against Flat at nprobe 1, 4, 16, 64, the bytes a row of IVFSQ, IVFFlat and
IVF, and the times of SQ.train and sq.encode over all the rows.  `--scan-only` stops after the
1,024-list points (for comparing builds of the scan, e.g. -DPQH_SQ_JC=128 through PQH_LIB).

  points   1,024 lists: (512 queries, 16 probes), (1, 16), (4,096, 64); 4,096 lists: (512, 16)

    python tools/bench_sq.py [--rows 1000000] [--reps 20] [--rounds 3] [--scan-only] [--out FILE.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from bench_flat import timed  # noqa: E402
from bench_flat_lists import recall  # noqa: E402
from pq_huffman_amd import codec  # noqa: E402


def point(ctx, sq_index, flat_index, q, nprobe, k, reps, rounds):
    """one point: the methods alternating, the best of `rounds`"""
    probes = flat_index.coarse.probe(q, nprobe, flat_index.offsets)[2]
    methods = {"ivfsq_ms": lambda: sq_index.search(q, nprobe, k),
               "ivfflat_ms": lambda: flat_index.search(q, nprobe, k),
               "sq_scan_ms": lambda: codec.sq_search_lists(ctx, sq_index.sq, sq_index.codes,
                                                           sq_index.offsets, probes, q, k),
               "flat_scan_ms": lambda: codec.flat_search_lists(ctx, flat_index.x_sorted,
                                                               flat_index.offsets, probes, q, k)}
    for fn in methods.values():   # the warm-up
        fn()
    torch.cuda.synchronize()
    res = {"n": sq_index.n, "d": sq_index.sq.d, "nlist": sq_index.coarse.nlist, "nq": q.shape[0],
           "nprobe": nprobe, "k": k}
    times = {name: [] for name in methods}
    for _ in range(rounds):
        for name, fn in methods.items():
            times[name].append(timed(fn, reps))
    for name, t in times.items():
        res[name] = min(t)
        res[name + "_all"] = t
    res["ivfsq_over_ivfflat"] = res["ivfsq_ms"] / res["ivfflat_ms"]
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--scan-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = codec.Context(0)
    n, d, k = a.rows, 128, 64
    x = bench.make_data(torch, n, d, 0x5EED, 0, dev)
    q = bench.make_data(torch, 4096, d, 0x5EED, 1, dev)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "rounds": a.rounds, "points": {}}
    sq = codec.SQ.train(ctx, x)
    if not a.scan_only:
        res["train_ms"] = min(timed(lambda: codec.SQ.train(ctx, x), a.reps) for _ in range(a.rounds))
        res["encode_ms"] = min(timed(lambda: sq.encode(x), a.reps) for _ in range(a.rounds))
    plans = ((1024, ((512, 16), (1, 16), (4096, 64))), (4096, ((512, 16),)))
    for nlist, shapes in plans[:1] if a.scan_only else plans:
        init = x[torch.arange(nlist, device=dev) * (n // nlist) + 3].contiguous()
        cq = codec.Coarse(ctx, codec.kmeans_train(ctx, x, init.cpu().numpy()[None], 2))
        flat_index = codec.IVFFlat.build(ctx, cq, x)
        sq_index = codec.IVFSQ.build(ctx, cq, x, sq=sq)
        codec.ivf_status(ctx)
        for nq, nprobe in shapes:
            res["points"][f"nlist{nlist}_nq{nq}_nprobe{nprobe}"] = point(
                ctx, sq_index, flat_index, q[:nq], nprobe, k, a.reps, a.rounds)
        if nlist == 1024 and not a.scan_only:
            flat = codec.Flat(ctx, x)
            exact = flat.search(q[:512], 10)[1]
            res["recall_at_10"] = {
                f"nprobe{nprobe}": {"ivfsq": recall(sq_index.search(q[:512], nprobe, 10)[1], exact),
                                    "ivfflat": recall(flat_index.search(q[:512], nprobe, 10)[1], exact)}
                for nprobe in (1, 4, 16, 64)}
            flat.close()
            sample = torch.arange(min(n, 200_000), device=dev) * (n // min(n, 200_000))
            pq = codec.PQ(ctx, bench.train_centroids(torch, x[sample], 8, 256))
            ivf = codec.IVF.build(ctx, pq, cq, x, chunk_vectors=4, context=True)
            # the rows alone; every index holds its ids beside them (8 bytes a row as perm)
            res["bytes_per_row"] = {"ivfsq": sq_index.codes.numel() / n,
                                    "ivfflat": flat_index.x_sorted.numel() * 4 / n,
                                    "ivf": ivf.enc.nbytes / n}
            print(json.dumps({k_: res[k_] for k_ in ("recall_at_10", "bytes_per_row")}), flush=True)
            del ivf
        codec.ivf_status(ctx)
        del flat_index, sq_index
        cq.close()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write("\n")


if __name__ == "__main__":
    main()
