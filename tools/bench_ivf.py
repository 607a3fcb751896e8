"""The inverted-file front end on the bench's own data (diagnostic): per-call HIP-event times
of Coarse.assign, Coarse.layout, Coarse.probe and IVF.search over back-to-back calls after a
warm-up, and beside each point, in the same process, the route a caller had before: a torch
coarse search (||x||^2 - 2 x C^T + ||c||^2 by matmul, then argmin / topk) feeding
codec.ivf_layout and codec.probe_ranges.  That route is context, not a gate: it does not
produce the same bits.

  assign   --rows x 128 at nlist in {1024, 4096}: ms, and the ratio of the 3 * n * nlist * d
           lane-operations of the direct form to the time (lane-operations per second, and as
           a share of 256 CUs x 128 lanes at --ghz; the clock the run held is NOT measured)
  layout   --rows and --layout-rows list ids at nlist 1024
  probe    nq in {1, 8, 64, 512}, nprobe 16, nlist 1024, and its share of the search_ranges
           call it feeds on the --rows stream (context mode, M = 8, K = 256, --chunk rows per
           chunk: the stream of tools/bench_search_ranges.py, stored list by list)
  search   IVF.search at the same points beside the sum of its three parts

    python tools/bench_ivf.py [--rows 1000000] [--layout-rows 125000000] [--chunk 4]
                              [--reps 20] [--ghz 2.4] [--out FILE.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from pq_huffman_amd import codec  # noqa: E402


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


def torch_dists(x, c, c2):
    return (x * x).sum(dim=1, keepdim=True) - 2.0 * (x @ c.t()) + c2


def torch_assign(x, c, step=262_144):
    """the matmul route, in slabs of rows so that the distance matrix stays a few GB"""
    c2 = (c * c).sum(dim=1)[None]
    return torch.cat([torch_dists(x[i:i + step], c, c2).argmin(dim=1)
                      for i in range(0, x.shape[0], step)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--layout-rows", type=int, default=125_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--chunk", type=int, default=4)
    ap.add_argument("--ghz", type=float, default=2.4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    d, m, n = 128, 8, a.rows
    x = bench.make_data(torch, n, d, 0x5EED, 0, dev)
    cent = bench.train_centroids(torch, bench.make_data(torch, 200_000, d, 0x5EED, 0, dev), m, 256)
    ctx = codec.Context(0)
    pq = codec.PQ(ctx, cent)
    res = {"rows": n, "d": d, "reps": a.reps, "nominal_ghz": a.ghz, "clock_measured": False}
    lanes_per_s = 256 * 128 * a.ghz * 1e9

    # ---- assign
    res["assign"] = []
    coarse = {}
    for nlist in (1024, 4096):
        # (rows of the data as centroids: the time does not depend on how good they are)
        c = x[torch.arange(nlist, device=dev) * (n // nlist) + 3].contiguous()
        coarse[nlist] = cq = codec.Coarse(ctx, c.cpu().numpy())
        out = torch.empty(n, dtype=torch.int32, device=dev)
        t = timed(lambda: cq.assign(x, out=out), a.reps)
        t_torch = timed(lambda: torch_assign(x, c), a.reps)
        agree = float((out.long() == torch_assign(x, c)).float().mean().item())
        ops = 3.0 * n * nlist * d
        res["assign"].append({"nlist": nlist, "ms": t, "lane_ops": ops,
                              "lane_ops_per_s": ops / (t * 1e-3),
                              "share_of_vector_rate_at_nominal_clock": ops / (t * 1e-3) / lanes_per_s,
                              "torch_matmul_argmin_ms": t_torch, "rows_agreeing_with_torch": agree})
        print(f"assign n={n} nlist={nlist}: {t:.3f} ms = {ops / (t * 1e-3) / 1e12:.2f} T lane-ops/s "
              f"({100 * ops / (t * 1e-3) / lanes_per_s:.1f} % of 256 x 128 lanes at {a.ghz} GHz, "
              f"clock not measured)  torch matmul + argmin {t_torch:.3f} ms  "
              f"(same list for {100 * agree:.2f} % of the rows)", flush=True)

    # ---- layout
    res["layout"] = []
    cq = coarse[1024]
    for rows in sorted({n, a.layout_rows}):
        ids = torch.randint(0, 1024, (rows,), dtype=torch.int32, device=dev,
                            generator=torch.Generator(device=dev).manual_seed(7))
        t = timed(lambda: cq.layout(ids), a.reps)
        codec.ivf_status(ctx)
        ids64 = ids.long()
        t_torch = timed(lambda: codec.ivf_layout(ids64, 1024), a.reps)
        perm, offsets = cq.layout(ids)
        tp, to = codec.ivf_layout(ids64, 1024)
        assert torch.equal(perm, tp) and torch.equal(offsets, to)
        res["layout"].append({"rows": rows, "nlist": 1024, "ms": t, "ns_per_row": t * 1e6 / rows,
                              "torch_sort_searchsorted_ms": t_torch})
        print(f"layout rows={rows} nlist=1024: {t:.3f} ms ({t * 1e6 / rows:.3f} ns per row)  "
              f"torch sort + searchsorted {t_torch:.3f} ms", flush=True)
        del ids, ids64, perm, offsets, tp, to
        ctx.release_scratch()
        torch.cuda.empty_cache()

    # ---- probe and the whole search, on the index of the same rows
    ivf = codec.IVF.build(ctx, pq, cq, x, chunk_vectors=a.chunk, context=True)
    codec.ivf_status(ctx)
    c = x[torch.arange(1024, device=dev) * (n // 1024) + 3].contiguous()
    c2 = (c * c).sum(dim=1)[None]
    queries_all = x[torch.arange(512, device=dev) * 997 + 5].contiguous()
    res["index"] = {"rows": n, "nlist": 1024, "chunk": a.chunk, "bits_per_row": ivf.enc.bits / n,
                    "largest_list": int((ivf.offsets[1:] - ivf.offsets[:-1]).max().item())}
    res["probe"] = []
    nprobe, k = 16, 10
    for nq in (1, 8, 64, 512):
        q = queries_all[:nq].contiguous()
        t_lut = timed(lambda: codec.adc_tables(ctx, pq, q), a.reps)
        t_probe = timed(lambda: cq.probe(q, nprobe, ivf.offsets, lists=False), a.reps)
        lut = codec.adc_tables(ctx, pq, q)
        ptr, ranges, probes, _ = cq.probe(q, nprobe, ivf.offsets)
        probed = int(ranges[:, 1].sum().item())
        t_scan = timed(lambda: codec.search_ranges(ctx, ivf.tables, ivf.enc, lut, ptr, ranges, k),
                       a.reps)
        t_all = timed(lambda: ivf.search(q, nprobe, k), a.reps)
        codec.decode_status(ctx)
        codec.ivf_status(ctx)

        def torch_probe():
            lists = torch_dists(q, c, c2).topk(nprobe, dim=1, largest=False).indices
            return codec.probe_ranges(ivf.offsets, lists)
        t_torch = timed(torch_probe, a.reps)
        res["probe"].append({"nq": nq, "nprobe": nprobe, "nlist": 1024, "k": k,
                             "probed_rows": probed, "adc_tables_ms": t_lut, "probe_ms": t_probe,
                             "search_ranges_ms": t_scan,
                             "probe_share_of_search_ranges": t_probe / t_scan,
                             "ivf_search_ms": t_all,
                             "sum_of_parts_ms": t_lut + t_probe + t_scan,
                             "torch_matmul_topk_probe_ranges_ms": t_torch})
        print(f"probe nq={nq} nprobe={nprobe}: {t_probe:.4f} ms = {100 * t_probe / t_scan:.1f} % of "
              f"search_ranges {t_scan:.4f} ms ({probed} probed rows)  adc_tables {t_lut:.4f} ms  "
              f"IVF.search {t_all:.4f} ms vs parts {t_lut + t_probe + t_scan:.4f} ms  "
              f"torch matmul + topk + probe_ranges {t_torch:.4f} ms", flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
