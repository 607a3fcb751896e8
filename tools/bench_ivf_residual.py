"""The residual inverted file on the bench's own data (diagnostic): per-call HIP-event times
over back-to-back calls after a warm-up, one index of --rows x 128 rows in 1,024 lists built
twice on the same coarse quantizer -- plain (the PQ trained on x) and residual (the PQ trained
on x - c[list]) -- M = 8, K = 256, context mode, --chunk rows per chunk.

  residuals  Coarse.residuals(x, lists, perm) beside the torch gather x[perm] it replaces in
             IVF.build, timed in the same process: ms per 1M rows and GB/s of the 8 * d bytes
             a row moves (the centroids come from L2)
  tables     adc_tables_residual (nq * nprobe tables) beside adc_tables (nq tables)
  scan       search_range_tables beside search_ranges on the SAME stream and ranges: the
             difference is the price of one table per range; and the table bytes a probed row
             costs at the least (one load of m * K * 4 bytes per range that has rows)
  search     IVF.search residual and plain, and recall@10 of both against the exact
             neighbours (torch, fp32) of queries drawn from the data's own mixture, beside the
             share of those neighbours that lie in a probed list at all
  long       --long-rows > 0: the residual index's codes repeated to that many rows as 1,024
             equal contiguous lists (the stream of tools/bench_search_ranges.py): the scan
             pair again where a list is thousands of steps

    python tools/bench_ivf_residual.py [--rows 1000000] [--long-rows 125000000] [--chunk 4]
                                       [--reps 20] [--out FILE.json]
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


def exact_neighbours(x, q, k, step=131_072):
    """ids (nq, k) of the k nearest rows of x by squared L2, slab by slab"""
    q2 = (q * q).sum(dim=1, keepdim=True)
    best_d = torch.full((q.shape[0], k), float("inf"), device=x.device)
    best_i = torch.full((q.shape[0], k), -1, dtype=torch.int64, device=x.device)
    for i in range(0, x.shape[0], step):
        xs = x[i:i + step]
        d = q2 - 2.0 * (q @ xs.t()) + (xs * xs).sum(dim=1)[None]
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
    ap.add_argument("--long-rows", type=int, default=125_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--chunk", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    d, m, n, nlist, nprobe, k = 128, 8, a.rows, 1024, 16, 10
    x = bench.make_data(torch, n, d, 0x5EED, 0, dev)
    queries_all = bench.make_data(torch, 512, d, 0x5EED, 1, dev)    # other rows of the mixture
    ctx = codec.Context(0)
    init = x[torch.arange(nlist, device=dev) * (n // nlist) + 3].contiguous()
    cq = codec.Coarse(ctx, codec.kmeans_train(ctx, x, init.cpu().numpy()[None], 2))
    lists = cq.assign(x)
    perm, offsets = cq.layout(lists)
    codec.ivf_status(ctx)
    res = {"device": torch.cuda.get_device_name(0), "rows": n, "d": d, "nlist": nlist, "m": m,
           "k_pq": 256, "chunk": a.chunk, "nprobe": nprobe, "top_k": k, "reps": a.reps}

    # ---- residuals beside the gather
    buf = torch.empty((n, d), dtype=torch.float32, device=dev)
    t_res = timed(lambda: cq.residuals(x, lists, perm, out=buf), a.reps)
    t_id = timed(lambda: cq.residuals(x, lists, None, out=buf), a.reps)
    t_gather = timed(lambda: torch.index_select(x, 0, perm, out=buf), a.reps)
    codec.ivf_status(ctx)
    moved = 8.0 * d * n
    res["residuals"] = {"ms": t_res, "ms_per_1m_rows": t_res * 1e6 / n,
                        "gb_per_s": moved / (t_res * 1e-3) / 1e9,
                        "identity_perm_ms": t_id, "identity_perm_gb_per_s": moved / (t_id * 1e-3) / 1e9,
                        "torch_gather_ms": t_gather,
                        "torch_gather_gb_per_s": moved / (t_gather * 1e-3) / 1e9}
    print(f"residuals n={n}: {t_res:.4f} ms ({moved / (t_res * 1e-3) / 1e9:.0f} GB/s of 8 d bytes a "
          f"row; identity perm {t_id:.4f} ms)  torch x[perm] {t_gather:.4f} ms "
          f"({moved / (t_gather * 1e-3) / 1e9:.0f} GB/s)", flush=True)

    # ---- the two indexes
    sample = torch.arange(200_000, device=dev) * (n // 200_000)
    cent_plain = bench.train_centroids(torch, x[sample], m, 256)
    cent_res = bench.train_centroids(torch, cq.residuals(x, lists, perm)[sample], m, 256)
    del buf
    pq_p, pq_r = codec.PQ(ctx, cent_plain), codec.PQ(ctx, cent_res)
    ivf_p = codec.IVF.build(ctx, pq_p, cq, x, chunk_vectors=a.chunk, context=True)
    ivf_r = codec.IVF.build(ctx, pq_r, cq, x, chunk_vectors=a.chunk, context=True, residual=True)
    codec.ivf_status(ctx)
    err_p = pq_p.error(x, pq_p.assign(x))
    rr = cq.residuals(x, lists)
    err_r = pq_r.error(rr, pq_r.assign(rr))
    del rr
    sizes = ivf_r.offsets[1:] - ivf_r.offsets[:-1]
    res["index"] = {"bits_per_row_plain": ivf_p.enc.bits / n, "bits_per_row_residual": ivf_r.enc.bits / n,
                    "pq_error_plain": err_p, "pq_error_residual": err_r,
                    "largest_list": int(sizes.max().item()), "mean_list": n / nlist}
    print(f"index: {ivf_p.enc.bits / n:.2f} bits per row plain, {ivf_r.enc.bits / n:.2f} residual; "
          f"PQ error {err_p:.1f} plain, {err_r:.1f} residual; largest list "
          f"{int(sizes.max().item())} rows", flush=True)

    exact = exact_neighbours(x, queries_all, k)
    table_bytes = m * 256 * 4
    res["points"] = []
    for nq in (1, 8, 64, 512):
        q = queries_all[:nq].contiguous()
        ptr, ranges, probes, _ = cq.probe(q, nprobe, ivf_r.offsets)
        probed = int(ranges[:, 1].sum().item())
        with_rows = int((ranges[:, 1] > 0).sum().item())
        lut_r = torch.empty((nq * nprobe, m, 256), dtype=torch.float32, device=dev)
        t_tab_r = timed(lambda: codec.adc_tables_residual(ctx, pq_r, cq, q, probes, out=lut_r), a.reps)
        t_tab = timed(lambda: codec.adc_tables(ctx, pq_r, q), a.reps)
        lut_q = codec.adc_tables(ctx, pq_r, q)
        out = (torch.empty((nq, k), dtype=torch.float32, device=dev),
               torch.empty((nq, k), dtype=torch.int64, device=dev))
        t_rt = timed(lambda: codec.search_range_tables(ctx, ivf_r.tables, ivf_r.enc, lut_r, ptr,
                                                       ranges, k, out=out), a.reps)
        t_rg = timed(lambda: codec.search_ranges(ctx, ivf_r.tables, ivf_r.enc, lut_q, ptr, ranges,
                                                 k, out=out), a.reps)
        t_sr = timed(lambda: ivf_r.search(q, nprobe, k), a.reps)
        t_sp = timed(lambda: ivf_p.search(q, nprobe, k), a.reps)
        codec.decode_status(ctx)
        codec.ivf_status(ctx)
        rec_r = recall(ivf_r.search(q, nprobe, k)[1], exact[:nq])
        rec_p = recall(ivf_p.search(q, nprobe, k)[1], exact[:nq])
        # what no PQ can exceed: the exact neighbours that lie in a probed list at all
        reach = float((lists[exact[:nq]].long()[:, :, None] == probes[:, None, :]).any(dim=2)
                      .float().mean().item())
        res["points"].append({
            "exact_neighbours_in_probed_lists": reach,
            "nq": nq, "probed_rows": probed, "ranges_with_rows": with_rows,
            "adc_tables_residual_us": t_tab_r * 1e3, "adc_tables_us": t_tab * 1e3,
            "search_range_tables_ms": t_rt, "search_ranges_ms": t_rg,
            "per_range_tables_cost": t_rt / t_rg,
            "table_bytes_per_probed_row_at_least": with_rows * table_bytes / max(probed, 1),
            "ivf_search_residual_ms": t_sr, "ivf_search_plain_ms": t_sp,
            "recall_at_10_residual": rec_r, "recall_at_10_plain": rec_p})
        print(f"nq={nq}: adc_tables_residual {t_tab_r * 1e3:.1f} us (adc_tables {t_tab * 1e3:.1f} us)  "
              f"search_range_tables {t_rt:.4f} ms vs search_ranges {t_rg:.4f} ms on {probed} probed "
              f"rows ({with_rows * table_bytes / max(probed, 1):.1f} table bytes a row at least)  "
              f"IVF.search residual {t_sr:.4f} ms plain {t_sp:.4f} ms  recall@10 residual "
              f"{rec_r:.3f} plain {rec_p:.3f} ({reach:.3f} of the exact neighbours lie in the probed "
              f"lists)", flush=True)

    # ---- long lists: the same codes repeated, 1,024 equal contiguous lists
    if a.long_rows > 0:
        rows1 = codec.decode(ctx, ivf_r.tables, ivf_r.enc)
        codec.decode_status(ctx)
        del x, ivf_p, ivf_r, exact
        torch.cuda.empty_cache()
        rows = rows1.repeat((a.long_rows + n - 1) // n, 1)[:a.long_rows].contiguous()
        nl = rows.shape[0]
        tabs = codec.Tables(ctx, m, 256, True).build(codec.histogram(ctx, rows, 256, True))
        enc = codec.encode(ctx, tabs, rows, chunk_vectors=a.chunk)
        del rows, rows1
        torch.cuda.empty_cache()
        off = torch.arange(nlist + 1, dtype=torch.int64, device=dev) * nl // nlist
        order = torch.rand((512, nlist), generator=torch.Generator().manual_seed(0x5EED)).argsort(dim=1)
        res["long"] = {"rows": nl, "list_rows": nl // nlist, "points": []}
        for nq in (1, 8, 64):
            q = queries_all[:nq].contiguous()
            probes = order[:nq, :nprobe].contiguous().to(dev)
            ptr, ranges = codec.probe_ranges(off, probes)
            probed = int(ranges[:, 1].sum().item())
            lut_r = codec.adc_tables_residual(ctx, pq_r, cq, q, probes)
            lut_q = codec.adc_tables(ctx, pq_r, q)
            out = (torch.empty((nq, k), dtype=torch.float32, device=dev),
                   torch.empty((nq, k), dtype=torch.int64, device=dev))
            t_rt = timed(lambda: codec.search_range_tables(ctx, tabs, enc, lut_r, ptr, ranges, k,
                                                           out=out), a.reps)
            t_rg = timed(lambda: codec.search_ranges(ctx, tabs, enc, lut_q, ptr, ranges, k, out=out),
                         a.reps)
            codec.decode_status(ctx)
            res["long"]["points"].append({
                "nq": nq, "probed_rows": probed, "search_range_tables_ms": t_rt,
                "search_ranges_ms": t_rg, "per_range_tables_cost": t_rt / t_rg,
                "table_bytes_per_probed_row_at_least": nq * nprobe * table_bytes / probed})
            print(f"long rows={nl} nq={nq}: search_range_tables {t_rt:.4f} ms vs search_ranges "
                  f"{t_rg:.4f} ms on {probed} probed rows", flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
