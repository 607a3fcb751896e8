"""What the wide list costs and what it buys (diagnostic): per-call HIP-event times on the index
of tools/bench_refine.py -- --rows SIFT-shaped rows, --nlist lists, --nprobe probes, M = 8,
K = 256, a 16 x 256 refinement codebook trained on pq_residuals, context mode -- in chunks of 4
and of 64 rows, for nq in {8, 64, 512} queries, on a context with set_search_max_k(256).
Per point and per candidate count c in {64, 128, 256}:
    stage_one   IVF.search(k = c), the scan that yields the candidates
    fused       codec.refine on those candidates to k = 10 (pqh_refine_stream, one launch)
    codes       the same over plain codes (pqh_refine_codes)
    search      IVF.search(k = 10, refine = c) end to end
    recall      recall@10 of `search` against the exact neighbours, brute force in torch on the
                same GPU (fp32 distances over the vectors themselves), and the share of the
                exact top 10 among the c candidates
The calls of a point are timed alternately in one process, --repeats times each after a warm-up;
min / median / max are kept, and for c > 64 the ratio to c = 64 of the same repeat.
Then the route a caller of 256 neighbours had before, at one whole-stream shape (--rows rows,
64 queries): codec.decode of the stream, a torch gather-and-sum over the tables and
torch.topk(256), alternated with codec.search(k = 256); the agreement of the ids is recorded, not
asserted (torch sums in another order).

    python tools/bench_search_wide.py [--rows 1000000] [--nlist 1024] [--nprobe 16] [--reps 20]
                                      [--repeats 5] [--out profiles/search_wide_bench.json]
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

CANDS = (64, 128, 256)

# the compiler's metadata of the wide kernels (hipcc -Rpass-analysis=kernel-resource-usage,
# gfx950; the whole listing is profiles/search_wide_resources.txt), copied by hand
KERNEL_RESOURCES = {
    "adc_scan<..., KR = 4> (72 instantiations)": {
        "vgprs": "98-176", "agprs": 0, "sgprs": 106, "vgpr_spills": 0,
        "sgpr_spills_to_vgpr_lanes": "75-214", "scratch_bytes_per_lane": 0,
        "occupancy_waves_per_simd": "2-4", "launch_bound_threads": 512,
        "lds_dynamic_bytes": "max(tables + stages, waves * QB * 256 * 12) <= 98304 for the exchange"},
    "adc_merge_wide": {"vgprs": 98, "agprs": 0, "sgprs": 106, "vgpr_spills": 0, "sgpr_spills_to_vgpr_lanes": 18,
                       "scratch_bytes_per_lane": 0, "occupancy_waves_per_simd": 4,
                       "lds_static_bytes": 46080},
    "refine_rows_wide<stream>": {"vgprs": 40, "agprs": 0, "sgprs": 92, "vgpr_spills": 0,
                                 "sgpr_spills": 0, "scratch_bytes_per_lane": 0,
                                 "occupancy_waves_per_simd": 8, "lds_static_bytes": 13824,
                                 "lds_dynamic_bytes": "4 * d"},
    "refine_rows_wide<codes>": {"vgprs": 40, "agprs": 0, "sgprs": 92, "vgpr_spills": 0,
                                "sgpr_spills": 0, "scratch_bytes_per_lane": 0,
                                "occupancy_waves_per_simd": 8, "lds_static_bytes": 13824,
                                "lds_dynamic_bytes": "4 * d"},
}


def stats(t):
    t = sorted(t)
    return {"min": t[0], "median": t[len(t) // 2], "max": t[-1]}


def exact_top10(x, q, block=32):
    """int64 (nq, 10): the nearest rows of x by fp32 squared distance, brute force"""
    out = []
    xx = (x * x).sum(dim=1)
    for s in range(0, q.shape[0], block):
        qq = q[s:s + block]
        dist = xx[None, :] - 2.0 * (qq @ x.t())
        out.append(torch.topk(dist, 10, dim=1, largest=False).indices)
    return torch.cat(out)


def shared(ids, exact):
    """the mean share of exact[i] found in ids[i]"""
    hit = (ids[:, :, None] == exact[:, None, :]).any(dim=1)
    return float(hit.float().mean().item())


def whole_stream(ctx, pq, tabs, enc, queries, reps, repeats):
    """codec.search(k = 256) over the whole stream beside decode + gather + topk in torch"""
    n, m = enc.n, pq.m
    lut = codec.adc_tables(ctx, pq, queries)
    lut_t = lut.permute(1, 2, 0).contiguous()
    full = torch.empty((n, m), dtype=torch.uint8, device=queries.device)

    def torch_route():
        codec.decode(ctx, tabs, enc, out=full)
        dist = lut_t[0].index_select(0, full[:, 0].to(torch.int32))
        for i in range(1, m):
            dist = dist + lut_t[i].index_select(0, full[:, i].to(torch.int32))
        return torch.topk(dist, 256, dim=0, largest=False, sorted=True)

    calls = {"search_256": lambda: codec.search(ctx, tabs, enc, lut, 256),
             "search_64": lambda: codec.search(ctx, tabs, enc, lut, 64),
             "torch_decode_gather_topk_256": torch_route}
    got, old = calls["search_256"](), torch_route()
    agree = float(sum(len(set(g.tolist()) & set(o.tolist()))
                      for g, o in zip(got[1].cpu(), old.indices.t().cpu()))) / (got[1].numel())
    times = {w: [] for w in calls}
    for _ in range(repeats):
        for w, fn in calls.items():
            times[w].append(timed(fn, reps))
    codec.decode_status(ctx)
    res = {"rows": n, "nq": queries.shape[0], "chunk": enc.chunk_vectors, "ids_shared_with_torch": agree}
    res.update({w + "_ms": stats(t) for w, t in times.items()})
    print(f"whole stream rows={n} nq={queries.shape[0]} shared={agree:.4f}: " +
          "  ".join(f"{w} {res[w + '_ms']['median']:.4f} ms" for w in calls), flush=True)
    return res


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
    d, n, k = 128, a.rows, 10
    x = bench.make_data(torch, n, d, 0x5EED, 0, dev)
    sample = x[:200_000]
    ctx = codec.Context(0).set_search_max_k(max(CANDS))
    pq = codec.PQ(ctx, bench.train_centroids(torch, sample, 8, 256))
    pq2 = codec.PQ(ctx, bench.train_centroids(torch, codec.pq_residuals(ctx, pq, sample), 16, 256))
    coarse = codec.Coarse(ctx, bench.train_centroids(torch, sample, 1, a.nlist))
    # (held-out rows of the same mixture, not rows of x: a row is its own nearest neighbour)
    queries = bench.make_data(torch, 512, d, 0x5EED, 1, dev)
    exact = exact_top10(x, queries)
    res = {"rows": n, "nlist": a.nlist, "nprobe": a.nprobe, "m": 8, "k": 256, "refine_m": 16,
           "candidates": list(CANDS), "top_k": k, "context": 1, "reps": a.reps, "repeats": a.repeats,
           "kernel_resources": KERNEL_RESOURCES, "points": []}
    for chunk in (4, 64):
        ivf = codec.IVF.build(ctx, pq, coarse, x, chunk_vectors=chunk, refine_pq=pq2)
        codec.ivf_status(ctx)
        l1 = (ivf.tables, ivf.pq, ivf.enc)
        l2 = (ivf.refine_tables, ivf.refine_pq, ivf.refine_enc)
        plain = ((pq, codec.decode(ctx, *l1[::2])), (pq2, codec.decode(ctx, *l2[::2])))
        codec.decode_status(ctx)
        for nq in (8, 64, 512):
            q = queries[:nq]
            calls, point = {}, {"chunk": chunk, "nq": nq}
            for c in CANDS:
                ids = ivf.search(q, a.nprobe, c)[1]
                rows = torch.where(ids >= 0, ivf.inv[ids.clamp(min=0)], ids).contiguous()   # stream rows
                calls[f"stage_one_{c}"] = lambda c=c: ivf.search(q, a.nprobe, c)
                calls[f"fused_{c}"] = lambda c=c, rows=rows: codec.refine(ctx, l1, l2, q, rows, k)
                calls[f"codes_{c}"] = lambda c=c, rows=rows: codec.refine(ctx, *plain, q, rows, k)
                calls[f"search_{c}"] = lambda c=c: ivf.search(q, a.nprobe, k, refine=c)
                assert same(calls[f"fused_{c}"](), calls[f"codes_{c}"]()), (chunk, nq, c)
                point[f"candidates_share_{c}"] = shared(ids, exact[:nq])
                point[f"recall_at_10_{c}"] = shared(calls[f"search_{c}"]()[1], exact[:nq])
            point["recall_at_10_unrefined"] = shared(ivf.search(q, a.nprobe, k)[1], exact[:nq])
            times = {w: [] for w in calls}
            for fn in calls.values():
                fn()
            for _ in range(a.repeats):                    # (alternately, the same process)
                for w, fn in calls.items():
                    times[w].append(timed(fn, a.reps))
            codec.decode_status(ctx)
            point.update({w + "_ms": stats(t) for w, t in times.items()})
            for what in ("stage_one", "fused", "codes", "search"):
                for c in CANDS[1:]:
                    point[f"{what}_{c}_over_64"] = stats(
                        [t / t64 for t, t64 in zip(times[f"{what}_{c}"], times[f"{what}_64"])])
            res["points"].append(point)
            print(f"chunk={chunk} nq={nq}: " + "  ".join(
                f"{w} {point[w + '_ms']['median']:.4f}" for w in calls) + " ms;  recall@10 " +
                "  ".join(f"{c}: {point[f'recall_at_10_{c}']:.4f} (share {point[f'candidates_share_{c}']:.4f})"
                          for c in CANDS), flush=True)
        if chunk == 4:
            res["whole_stream"] = whole_stream(ctx, pq, ivf.tables, ivf.enc, queries[:64], a.reps,
                                               a.repeats)
        del ivf, plain
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
