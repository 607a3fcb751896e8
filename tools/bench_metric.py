"""The inner-product metric beside its L2 twins on the bench's own data (diagnostic): per-call
HIP-event times over back-to-back calls after a warm-up, --rows x 128 rows (the bench's
mixture, centred, so that inner products have both signs) in 1,024 lists, M = 8, K = 256,
context mode, --chunk rows per chunk, 512 queries x 16 probes, k = 64.

Every time is [the smallest, the largest] of --rounds timings.

  assign   Coarse.assign of all rows, metric l2 and ip
  probe    Coarse.probe of the queries, l2 and ip
  tables   adc_tables (nq tables) and adc_tables_residual (nq * nprobe tables), l2 and ip
  scan     search_ranges on the plain L2 index's stream and ranges, fed L2 tables and ip tables:
           the scan itself does not know the metric
  search   IVF.search of four indexes on the same coarse quantizer -- plain and residual, each
           built with metric l2 and ip -- beside the rows its probes reach (the lists of an ip index are the less even ones, so
           the same probes reach more rows) and recall@10 of the exact answer of its own metric

    python tools/bench_metric.py [--rows 1000000] [--chunk 4] [--reps 20] [--rounds 5]
                                 [--out FILE.json]
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


def spread(fn, reps, rounds, scale=1.0):
    """[smallest, largest] of `rounds` timings of fn, each `timed`"""
    t = [scale * timed(fn, reps) for _ in range(rounds)]
    return [min(t), max(t)]


def exact_top(x, q, k, metric, step=131_072):
    """ids (nq, k) of the exact answer: the smallest squared L2 or the largest inner product"""
    best_d = torch.full((q.shape[0], k), float("inf"), device=x.device)
    best_i = torch.full((q.shape[0], k), -1, dtype=torch.int64, device=x.device)
    for i in range(0, x.shape[0], step):
        xs = x[i:i + step]
        d = -(q @ xs.t())
        if metric == "l2":
            d = 2.0 * d + (xs * xs).sum(dim=1)[None]
        dd, ii = d.topk(min(k, xs.shape[0]), dim=1, largest=False)
        dd, sel = torch.cat([best_d, dd], dim=1).topk(k, dim=1, largest=False)
        best_i = torch.cat([best_i, ii + i], dim=1).gather(1, sel)
        best_d = dd
    return best_i


def recall(ids, exact):
    hit = (ids[:, :, None] == exact[:, None, :]).any(dim=2).float().sum(dim=1)
    return float((hit / exact.shape[1]).mean().item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    d, m, n, nlist, nprobe, k, nq = 128, 8, a.rows, 1024, 16, 64, 512
    x = bench.make_data(torch, n, d, 0x5EED, 0, dev)
    mean = x.mean(dim=0)
    x -= mean
    q = bench.make_data(torch, nq, d, 0x5EED, 1, dev) - mean        # other rows of the mixture
    ctx = codec.Context(0)
    init = x[torch.arange(nlist, device=dev) * (n // nlist) + 3].contiguous()
    cq = codec.Coarse(ctx, codec.kmeans_train(ctx, x, init.cpu().numpy()[None], 2))
    res = {"device": torch.cuda.get_device_name(0), "rows": n, "d": d, "nlist": nlist, "m": m,
           "k_pq": 256, "chunk": a.chunk, "nq": nq, "nprobe": nprobe, "top_k": k, "reps": a.reps,
           "rounds": a.rounds}
    sample = torch.arange(200_000, device=dev) * (n // 200_000)

    lists_buf = torch.empty(n, dtype=torch.int32, device=dev)
    for metric in ("l2", "ip"):
        r = res[metric] = {}
        r["coarse_assign_ms"] = spread(lambda: cq.assign(x, out=lists_buf, metric=metric), a.reps,
                                       a.rounds)
        lists = cq.assign(x, metric=metric)
        perm, offsets = cq.layout(lists)
        codec.ivf_status(ctx)
        sizes = offsets[1:] - offsets[:-1]
        r["largest_list"], r["empty_lists"] = int(sizes.max().item()), int((sizes == 0).sum().item())
        r["coarse_probe_us"] = spread(lambda: cq.probe(q, nprobe, offsets, metric=metric), a.reps,
                                      a.rounds, 1e3)
        ptr, ranges, probes, _ = cq.probe(q, nprobe, offsets, metric=metric)
        r["probed_rows"] = int(ranges[:, 1].sum().item())
        cent_p = bench.train_centroids(torch, x[sample], m, 256)
        cent_r = bench.train_centroids(torch, cq.residuals(x, lists, perm)[sample], m, 256)
        pq_p, pq_r = codec.PQ(ctx, cent_p), codec.PQ(ctx, cent_r)
        lut = torch.empty((nq, m, 256), dtype=torch.float32, device=dev)
        lut_r = torch.empty((nq * nprobe, m, 256), dtype=torch.float32, device=dev)
        r["adc_tables_us"] = spread(
            lambda: codec.adc_tables(ctx, pq_p, q, out=lut, metric=metric), a.reps, a.rounds, 1e3)
        r["adc_tables_residual_us"] = spread(
            lambda: codec.adc_tables_residual(ctx, pq_r, cq, q, probes, out=lut_r, metric=metric),
            a.reps, a.rounds, 1e3)
        del lut, lut_r
        exact = exact_top(x, q, 10, metric)
        for kind, pq in (("plain", pq_p), ("residual", pq_r)):
            ivf = codec.IVF.build(ctx, pq, cq, x, chunk_vectors=a.chunk, context=True,
                                  residual=kind == "residual", metric=metric)
            codec.ivf_status(ctx)
            r[f"ivf_search_{kind}_ms"] = spread(lambda: ivf.search(q, nprobe, k), a.reps, a.rounds)
            codec.decode_status(ctx)
            r[f"recall_at_10_{kind}"] = recall(ivf.search(q, nprobe, k)[1][:, :10], exact)
            r[f"bits_per_row_{kind}"] = ivf.enc.bits / n
            if metric == "l2" and kind == "plain":
                # the scan alone, on this index's stream and ranges, fed either kind of table
                out = (torch.empty((nq, k), dtype=torch.float32, device=dev),
                       torch.empty((nq, k), dtype=torch.int64, device=dev))
                for name in ("l2", "ip"):
                    t = codec.adc_tables(ctx, pq, q, metric=name)
                    res[f"scan_same_ranges_{name}_tables_ms"] = spread(
                        lambda: codec.search_ranges(ctx, ivf.tables, ivf.enc, t, ptr, ranges, k,
                                                    out=out), a.reps, a.rounds)
                codec.decode_status(ctx)
            del ivf
            torch.cuda.empty_cache()
        print(f"{metric} [smallest, largest of {a.rounds}]: assign {r['coarse_assign_ms']} ms  probe "
              f"{r['coarse_probe_us']} us  adc_tables {r['adc_tables_us']} us  adc_tables_residual "
              f"{r['adc_tables_residual_us']} us  IVF.search plain {r['ivf_search_plain_ms']} ms "
              f"residual {r['ivf_search_residual_ms']} ms on {r['probed_rows']} probed rows "
              f"(largest list {r['largest_list']}, {r['empty_lists']} empty)  recall@10 plain "
              f"{r['recall_at_10_plain']:.3f} residual {r['recall_at_10_residual']:.3f}", flush=True)
        pq_p.close()
        pq_r.close()
    print(f"scan on the same ranges: {res['scan_same_ranges_l2_tables_ms']} ms with L2 tables, "
          f"{res['scan_same_ranges_ip_tables_ms']} ms with ip tables", flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
