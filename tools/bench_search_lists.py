"""The list-major probe search beside the query-major one (diagnostic): per-call HIP-event
times of codec.search_lists and of codec.search_ranges / codec.search_range_tables on the same
stream and the same probes, in one process, for nq in {1, 8, 64, 512} queries probing nprobe in
{1, 16, 64} of --nlist equal contiguous lists (the points of tools/bench_search_ranges.py), with
one table per query and with one per (query, list) pair, and the work units of every call.
Context mode, SIFT shape (M = 8, K = 256), --chunk rows per chunk, the 1M-row batch repeated to
fill --rows.  Both forms give the same bits, which is checked at every point.

    python tools/bench_search_lists.py [--rows 1000000] [--chunk 4] [--nlist 1024] [--k 10]
                                       [--reps 20] [--out FILE.json]

With --out the result (one JSON object per --rows value) is merged into that file
(profiles/search_lists_bench.json holds the runs DESIGN.md section 4.5.6 quotes).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from pq_huffman_amd import codec  # noqa: E402

QB = 8   # the pairs of a unit at M = 8


def timed(fn, reps, budget_ms=300.0):
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


def same(a, b):
    return torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--chunk", type=int, default=4)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    d, m, k = 128, 8, a.k
    base = 1_000_000
    x = bench.make_data(torch, base, d, 0x5EED, 0, dev)
    cent = bench.train_centroids(torch, bench.make_data(torch, 200_000, d, 0x5EED, 0, dev), m, 256)
    ctx = codec.Context(0)
    pq = codec.PQ(ctx, cent)
    rows1 = pq.assign(x)
    nq_max = 512
    queries = x[torch.arange(nq_max, device=dev) * 997 + 5].contiguous()   # of the data's rows
    del x
    rows = rows1.repeat((a.rows + base - 1) // base, 1)[:a.rows].contiguous()
    n, C, nlist = rows.shape[0], a.chunk, a.nlist
    tabs = codec.Tables(ctx, m, 256, True).build(codec.histogram(ctx, rows, 256, True))
    enc = codec.encode(ctx, tabs, rows, chunk_vectors=C)
    del rows
    torch.cuda.empty_cache()
    lut_all = codec.adc_tables(ctx, pq, queries)
    # equal contiguous lists; every query probes its own nprobe of them (fixed seed)
    offsets = torch.arange(nlist + 1, dtype=torch.int64, device=dev) * n // nlist
    gen = torch.Generator().manual_seed(0x5EED)
    order = torch.rand((nq_max, nlist), generator=gen).argsort(dim=1)
    res = {"rows": n, "chunk": C, "m": m, "k": 256, "top_k": k, "context": 1, "nlist": nlist,
           "bits_per_row": enc.bits / n, "reps": a.reps, "points": []}
    for nq in (1, 8, 64, 512):
        lut = lut_all[:nq].contiguous()
        for nprobe in (1, 16, 64):
            probes = order[:nq, :nprobe].contiguous().to(dev)
            ptr, ranges = codec.probe_ranges(offsets, probes)
            per_list = torch.bincount(probes.reshape(-1), minlength=nlist)
            units = int(((per_list + QB - 1) // QB).sum().item())
            # (a table per pair: the query's own, so that both table forms give the same bits)
            lut_pair = lut.repeat_interleave(nprobe, dim=0).contiguous()
            outs = [(torch.empty((nq, k), dtype=torch.float32, device=dev),
                     torch.empty((nq, k), dtype=torch.int64, device=dev)) for _ in range(4)]
            t_rq = timed(lambda: codec.search_ranges(ctx, tabs, enc, lut, ptr, ranges, k,
                                                     out=outs[0]), a.reps)
            t_lq = timed(lambda: codec.search_lists(ctx, tabs, enc, lut, offsets, probes, k,
                                                    out=outs[1]), a.reps)
            t_rp = timed(lambda: codec.search_range_tables(ctx, tabs, enc, lut_pair, ptr, ranges,
                                                           k, out=outs[2]), a.reps)
            t_lp = timed(lambda: codec.search_lists(ctx, tabs, enc, lut_pair, offsets, probes, k,
                                                    out=outs[3]), a.reps)
            codec.decode_status(ctx)
            assert all(same(outs[0], o) for o in outs[1:])
            res["points"].append({
                "nq": nq, "nprobe": nprobe, "pairs_per_list": nq * nprobe / nlist, "units": units,
                "lists_probed": int((per_list > 0).sum().item()),
                "search_ranges_ms": t_rq, "search_lists_ms": t_lq,
                "search_range_tables_ms": t_rp, "search_lists_pair_tables_ms": t_lp,
                "speedup_shared_tables": t_rq / t_lq, "speedup_pair_tables": t_rp / t_lp})
            print(f"rows={n} nq={nq} nprobe={nprobe} units={units}: table per query: ranges "
                  f"{t_rq:.4f} ms lists {t_lq:.4f} ms ({t_rq / t_lq:.2f}x)  table per pair: "
                  f"ranges {t_rp:.4f} ms lists {t_lp:.4f} ms ({t_rp / t_lp:.2f}x)", flush=True)
            del lut_pair
    if a.out:
        runs = {}
        if os.path.exists(a.out):
            with open(a.out) as fh:
                runs = json.load(fh)
        runs[str(n)] = res
        with open(a.out, "w") as fh:
            json.dump(runs, fh, indent=1, sort_keys=True)
            fh.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
