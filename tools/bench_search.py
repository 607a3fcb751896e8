"""ADC search of one compressed stream on the bench's own data (diagnostic): per-call
HIP-event times of codec.search (decode and scan fused, the codes never written) for
nq in {1, 8, 64} queries and k in {10, 64}, beside the two routes a caller had before it, timed
in the same process: pqh_decode of everything followed by codec.search_codes, and the outside
yardstick written in torch -- pqh_decode of everything, a gather of the table entries part by
part, their sum and torch.topk.  Context mode, SIFT shape (M = 8, K = 256), --chunk rows per
chunk (the bench's 4), the 1M-row batch repeated to fill --rows.

    python tools/bench_search.py [--rows 1000000] [--chunk 4] [--reps 20] [--out FILE.json]

With --out the result (one JSON object per --rows value) is merged into that file.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from pq_huffman_amd import codec  # noqa: E402


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--chunk", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    d, m = 128, 8
    base = 1_000_000
    x = bench.make_data(torch, base, d, 0x5EED, 0, dev)
    cent = bench.train_centroids(torch, bench.make_data(torch, 200_000, d, 0x5EED, 0, dev), m, 256)
    ctx = codec.Context(0)
    pq = codec.PQ(ctx, cent)
    rows1 = pq.assign(x)
    queries = x[torch.arange(64, device=dev) * 997 + 5].contiguous()   # 64 of the data's rows
    del x
    rows = rows1.repeat((a.rows + base - 1) // base, 1)[:a.rows].contiguous()
    n, C = rows.shape[0], a.chunk
    counts = codec.histogram(ctx, rows, 256, True)
    tabs = codec.Tables(ctx, m, 256, True).build(counts)
    enc = codec.encode(ctx, tabs, rows, chunk_vectors=C)
    full = torch.empty_like(rows)
    t_full = timed(lambda: codec.decode(ctx, tabs, enc, out=full), a.reps)
    codec.decode_status(ctx)
    assert torch.equal(full, rows)
    del rows
    lut_all = codec.adc_tables(ctx, pq, queries)
    t_lut = timed(lambda: codec.adc_tables(ctx, pq, queries, out=lut_all), a.reps)
    res = {"rows": n, "chunk": C, "m": m, "k": 256, "context": 1, "bits_per_row": enc.bits / n,
           "reps": a.reps, "decode_all_ms": t_full, "adc_tables_64_ms": t_lut,
           "lds_b128_reads_per_row_design": {"query_batch": 8, "reads": m * 8 // 4},
           "search": []}
    slow_reps = max(2, min(a.reps, 200_000_000 // max(n, 1)))
    for nq in (1, 8, 64):
        lut = lut_all[:nq].contiguous()
        lut_t = lut.permute(1, 2, 0).contiguous()   # [m][K][nq]: a row's entries for every query
        for k in (10, 64):
            out = (torch.empty((nq, k), dtype=torch.float32, device=dev),
                   torch.empty((nq, k), dtype=torch.int64, device=dev))
            out2 = (torch.empty_like(out[0]), torch.empty_like(out[1]))
            t_s = timed(lambda: codec.search(ctx, tabs, enc, lut, k, out=out), a.reps)
            codec.decode_status(ctx)

            def decode_then_scan():
                codec.decode(ctx, tabs, enc, out=full)
                codec.search_codes(ctx, full, lut, k, out=out2)
            t_c = timed(decode_then_scan, a.reps)
            t_c_only = timed(lambda: codec.search_codes(ctx, full, lut, k, out=out2), a.reps)
            assert torch.equal(out[1], out2[1]) and torch.equal(out[0], out2[0])

            def torch_route():
                codec.decode(ctx, tabs, enc, out=full)
                dist = lut_t[0].index_select(0, full[:, 0].to(torch.int32))
                for i in range(1, m):
                    dist = dist + lut_t[i].index_select(0, full[:, i].to(torch.int32))
                return torch.topk(dist, min(k, n), dim=0, largest=False, sorted=True)
            try:
                t_t = timed(torch_route, slow_reps)
                top = torch_route()
                # (torch.topk breaks ties its own way: the distances must agree, the ids need not)
                assert torch.equal(top.values.t().contiguous(), out[0][:, :min(k, n)])
                del top
            except torch.OutOfMemoryError:
                t_t = None
            torch.cuda.empty_cache()
            res["search"].append({
                "nq": nq, "k": k, "search_ms": t_s, "decode_all_search_codes_ms": t_c,
                "search_codes_ms": t_c_only, "torch_decode_gather_topk_ms": t_t,
                "search_rows_queries_per_s": n * nq / (t_s * 1e-3),
                "search_codes_rows_queries_per_s": n * nq / (t_c_only * 1e-3),
                "speedup_over_torch": (t_t / t_s) if t_t else None})
            print(f"rows={n} nq={nq} k={k}: search {t_s:.4f} ms  decode all + search_codes "
                  f"{t_c:.4f} ms (scan alone {t_c_only:.4f})  torch decode + gather + topk "
                  f"{t_t if t_t is None else round(t_t, 4)} ms", flush=True)
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
