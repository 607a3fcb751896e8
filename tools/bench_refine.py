"""The fused re-rank beside the route it replaces (diagnostic): per-call HIP-event times on one
index with a refinement stream -- --rows SIFT-shaped rows, --nlist lists, --nprobe probes,
M = 8, K = 256, a 16 x 256 refinement codebook trained on pq_residuals, context mode -- in
chunks of 4 and of 64 rows, for nq in {8, 64, 512} queries, refine = 64 candidates, k = 10.
Per point:
    stage_one   IVF.search(k = 64), the scan that yields the candidates
    fused       codec.refine on those candidates (pqh_refine_stream, one launch)
    codes       the same over plain codes (pqh_refine_codes): what the two row walks cost
    replaced    the same result from the calls the library had before: codec.fetch at both
                levels, then torch for the sum, the distance and the sort
    search      IVF.search(k = 10, refine = 64) end to end
`fused` and `replaced` are timed alternately in the same process, --repeats times each after a
warm-up (min / median / max are kept).  The fused result is checked bit for bit against the
call over plain codes; against the torch route only the agreement of the ids is recorded (torch
sums the squares in another order).

    python tools/bench_refine.py [--rows 1000000] [--nlist 1024] [--nprobe 16] [--reps 20]
                                 [--repeats 5] [--out profiles/refine_bench.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from bench_search_filter import same, timed  # noqa: E402
from pq_huffman_amd import codec  # noqa: E402


# the compiler's metadata of the two instantiations (hipcc -Rpass-analysis=kernel-resource-usage,
# gfx950), kept beside the times they belong to; copied by hand when pqh_refine.hip changes
KERNEL_RESOURCES = {
    "refine_rows<stream>": {"vgprs": 33, "agprs": 0, "sgprs": 85, "lds_static_bytes": 2688,
                            "lds_dynamic_bytes": "4 * d", "vgpr_spills": 0, "sgpr_spills": 0,
                            "scratch_bytes_per_lane": 0, "occupancy_waves_per_simd": 8},
    "refine_rows<codes>": {"vgprs": 33, "agprs": 0, "sgprs": 46, "lds_static_bytes": 2688,
                           "lds_dynamic_bytes": "4 * d", "vgpr_spills": 0, "sgpr_spills": 0,
                           "scratch_bytes_per_lane": 0, "occupancy_waves_per_simd": 8},
}


def stats(t):
    t = sorted(t)
    return {"min": t[0], "median": t[len(t) // 2], "max": t[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    d, n, k, cand = 128, a.rows, 10, 64
    x = bench.make_data(torch, n, d, 0x5EED, 0, dev)
    sample = x[:200_000]
    ctx = codec.Context(0)
    pq = codec.PQ(ctx, bench.train_centroids(torch, sample, 8, 256))
    pq2 = codec.PQ(ctx, bench.train_centroids(torch, codec.pq_residuals(ctx, pq, sample), 16, 256))
    coarse = codec.Coarse(ctx, bench.train_centroids(torch, sample, 1, a.nlist))
    queries = x[torch.arange(512, device=dev) * 997 % n].contiguous()
    res = {"rows": n, "nlist": a.nlist, "nprobe": a.nprobe, "m": 8, "k": 256, "refine_m": 16,
           "refine": cand, "top_k": k, "context": 1, "reps": a.reps, "repeats": a.repeats,
           "kernel_resources": KERNEL_RESOURCES, "points": []}
    for chunk in (4, 64):
        ivf = codec.IVF.build(ctx, pq, coarse, x, chunk_vectors=chunk, refine_pq=pq2)
        codec.ivf_status(ctx)
        l1 = (ivf.tables, ivf.pq, ivf.enc)
        l2 = (ivf.refine_tables, ivf.refine_pq, ivf.refine_enc)
        plain = ((pq, codec.decode(ctx, *l1[::2])), (pq2, codec.decode(ctx, *l2[::2])))
        codec.decode_status(ctx)
        bits = (ivf.enc.bits / n, ivf.refine_enc.bits / n)
        for nq in (8, 64, 512):
            q = queries[:nq]
            rows = ivf.search(q, a.nprobe, cand)[1]
            rows = torch.where(rows >= 0, ivf.inv[rows.clamp(min=0)], rows).contiguous()   # stream rows

            def replaced():
                flat = rows.clamp(min=0).reshape(-1)
                y = codec.fetch(ctx, *l1, flat).add_(codec.fetch(ctx, *l2, flat))
                dist = (q[:, None, :] - y.view(nq, cand, d)).square_().sum(dim=2)
                dist[rows < 0] = float("inf")
                top, at = torch.topk(dist, k, dim=1, largest=False)
                return top, torch.gather(rows, 1, at)

            calls = {"stage_one": lambda: ivf.search(q, a.nprobe, cand),
                     "fused": lambda: codec.refine(ctx, l1, l2, q, rows, k),
                     "codes": lambda: codec.refine(ctx, *plain, q, rows, k),
                     "replaced": replaced,
                     "search": lambda: ivf.search(q, a.nprobe, k, refine=cand)}
            got = calls["fused"]()
            assert same(got, calls["codes"]()), (chunk, nq)
            old = replaced()
            agree = float(sum(len(set(g.tolist()) & set(o.tolist()))
                              for g, o in zip(got[1].cpu(), old[1].cpu()))) / (nq * k)
            times = {w: [] for w in calls}
            for fn in calls.values():
                fn()
            for _ in range(a.repeats):                    # (alternately, the same process)
                for w, fn in calls.items():
                    times[w].append(timed(fn, a.reps))
            codec.decode_status(ctx)
            point = {"chunk": chunk, "nq": nq, "bits_per_row": bits, "ids_shared_with_torch": agree}
            point.update({w + "_ms": stats(t) for w, t in times.items()})
            res["points"].append(point)
            print(f"chunk={chunk} nq={nq} shared={agree:.4f}: " +
                  "  ".join(f"{w} {point[w + '_ms']['median']:.4f} ms "
                            f"[{point[w + '_ms']['min']:.4f}, {point[w + '_ms']['max']:.4f}]"
                            for w in calls), flush=True)
        del ivf, plain
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
