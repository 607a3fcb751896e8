"""The probe search on the bench's own data (diagnostic): per-call HIP-event times of
codec.search_ranges for nq in {1, 8, 64, 512} queries probing nprobe in {1, 16, 64} of
--nlist equal contiguous lists, k in {10, 64}, beside two yardsticks timed in the same
process: codec.search of the whole stream for the same nq, and the route a caller had before
-- codec.decode_range of each probed list into one buffer, then codec.search_codes on it,
query by query.  One further point is the price of the plan and of one query per workgroup:
one query with a single whole-stream range beside codec.search at nq = 1.  Context mode, SIFT
shape (M = 8, K = 256), --chunk rows per chunk, the 1M-row batch repeated to fill --rows (the
stream of tools/bench_search.py).

    python tools/bench_search_ranges.py [--rows 1000000] [--chunk 4] [--nlist 1024]
                                        [--reps 20] [--out FILE.json]

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--chunk", type=int, default=4)
    ap.add_argument("--nlist", type=int, default=1024)
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
    nq_max = 512
    queries = x[torch.arange(nq_max, device=dev) * 997 + 5].contiguous()   # of the data's rows
    del x
    rows = rows1.repeat((a.rows + base - 1) // base, 1)[:a.rows].contiguous()
    n, C, nlist = rows.shape[0], a.chunk, a.nlist
    tabs = codec.Tables(ctx, m, 256, True).build(codec.histogram(ctx, rows, 256, True))
    enc = codec.encode(ctx, tabs, rows, chunk_vectors=C)
    full = torch.empty_like(rows)
    t_full = timed(lambda: codec.decode(ctx, tabs, enc, out=full), a.reps)
    codec.decode_status(ctx)
    assert torch.equal(full, rows)
    del rows, full
    torch.cuda.empty_cache()
    lut_all = codec.adc_tables(ctx, pq, queries)
    # equal contiguous lists; every query probes its own nprobe of them (fixed seed)
    offsets = torch.arange(nlist + 1, dtype=torch.int64, device=dev) * n // nlist
    offsets_h = offsets.cpu().tolist()
    gen = torch.Generator().manual_seed(0x5EED)
    order = torch.rand((nq_max, nlist), generator=gen).argsort(dim=1)
    res = {"rows": n, "chunk": C, "m": m, "k": 256, "context": 1, "nlist": nlist,
           "bits_per_row": enc.bits / n, "reps": a.reps, "decode_all_ms": t_full,
           "decode_ns_per_row": t_full * 1e6 / n, "points": []}

    for k in (10, 64):   # one query, one range: the whole stream
        out = (torch.empty((1, k), dtype=torch.float32, device=dev),
               torch.empty((1, k), dtype=torch.int64, device=dev))
        out2 = (torch.empty_like(out[0]), torch.empty_like(out[1]))
        ptr = torch.tensor([0, 1], dtype=torch.int64, device=dev)
        whole = torch.tensor([[0, n]], dtype=torch.int64, device=dev)
        lut = lut_all[:1].contiguous()
        t_r = timed(lambda: codec.search_ranges(ctx, tabs, enc, lut, ptr, whole, k, out=out), a.reps)
        t_s = timed(lambda: codec.search(ctx, tabs, enc, lut, k, out=out2), a.reps)
        codec.decode_status(ctx)
        assert torch.equal(out[1], out2[1]) and torch.equal(out[0], out2[0])
        res.setdefault("whole_stream_one_query", []).append(
            {"k": k, "search_ranges_ms": t_r, "search_ms": t_s})
        print(f"rows={n} one whole-stream range, nq=1 k={k}: search_ranges {t_r:.4f} ms  "
              f"search {t_s:.4f} ms", flush=True)

    for nq in (1, 8, 64, 512):
        lut = lut_all[:nq].contiguous()
        for k in (10, 64):
            out = (torch.empty((nq, k), dtype=torch.float32, device=dev),
                   torch.empty((nq, k), dtype=torch.int64, device=dev))
            out_s = (torch.empty_like(out[0]), torch.empty_like(out[1]))
            out_1 = (torch.empty((1, k), dtype=torch.float32, device=dev),
                     torch.empty((1, k), dtype=torch.int64, device=dev))
            t_s = timed(lambda: codec.search(ctx, tabs, enc, lut, k, out=out_s), a.reps)
            for nprobe in (1, 16, 64):
                probes = order[:nq, :nprobe].contiguous()
                ptr, ranges = codec.probe_ranges(offsets, probes.to(dev))
                probed = int(ranges[:, 1].sum().item())
                t_r = timed(lambda: codec.search_ranges(ctx, tabs, enc, lut, ptr, ranges, k,
                                                        out=out), a.reps)
                codec.decode_status(ctx)
                probes_h = probes.tolist()
                longest = max(sum(offsets_h[l + 1] - offsets_h[l] for l in p) for p in probes_h)
                buf = torch.empty((longest, m), dtype=torch.uint8, device=dev)

                def decode_lists_then_scan():
                    for q in range(nq):
                        at = 0
                        for l in probes_h[q]:
                            cnt = offsets_h[l + 1] - offsets_h[l]
                            codec.decode_range(ctx, tabs, enc, offsets_h[l], cnt, out=buf[at:at + cnt])
                            at += cnt
                        codec.search_codes(ctx, buf[:at], lut[q:q + 1], k, out=out_1)
                t_d = timed(decode_lists_then_scan, a.reps)
                codec.decode_status(ctx)
                # (the buffer's rows have their own numbering: the distances must agree)
                assert torch.equal(out_1[0][0], out[0][nq - 1])
                del buf
                res["points"].append({
                    "nq": nq, "nprobe": nprobe, "k": k, "probed_rows": probed,
                    "search_ranges_ms": t_r, "search_whole_stream_ms": t_s,
                    "decode_range_search_codes_ms": t_d,
                    "ns_per_probed_row": t_r * 1e6 / max(probed, 1),
                    "speedup_over_whole_stream": t_s / t_r,
                    "speedup_over_decode_range_route": t_d / t_r})
                print(f"rows={n} nq={nq} nprobe={nprobe} k={k}: search_ranges {t_r:.4f} ms "
                      f"({t_r * 1e6 / max(probed, 1):.4f} ns per probed row)  search of the whole "
                      f"stream {t_s:.4f} ms  decode_range + search_codes {t_d:.4f} ms", flush=True)
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
