"""Random access into one compressed stream on the bench's own data (diagnostic): per-launch
HIP-event times of codec.decode_rows / codec.fetch for 2^10 ... 2^20 uniformly random ids and
of codec.decode_range for the whole stream and a 1 % slice, each beside the route that was
there before them, timed in the same process: pqh_decode of everything, then index_select
(and pq.reconstruct for fetch) or a copy of the slice.  Context mode, SIFT shape (M = 8,
K = 256), --chunk rows per chunk (the bench's 4), the 1M-row batch repeated to fill --rows.

    python tools/bench_select.py [--rows 1000000] [--chunk 4] [--reps 20] [--out FILE.json]

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
    for _ in range(3):
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
    res = {"rows": n, "chunk": C, "m": m, "k": 256, "context": 1, "bits_per_row": enc.bits / n,
           "reps": a.reps, "decode_all_ms": t_full, "select": []}
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    crossover = None
    for lg in range(10, 21):
        cnt = 1 << lg
        ids = torch.randint(0, n, (cnt,), generator=gen, device=dev, dtype=torch.int64)
        out_c = torch.empty((cnt, m), dtype=torch.uint8, device=dev)
        out_f = torch.empty((cnt, d), dtype=torch.float32, device=dev)
        t_sel = timed(lambda: codec.decode_rows(ctx, tabs, enc, ids, out=out_c), a.reps)
        t_fet = timed(lambda: codec.fetch(ctx, tabs, pq, enc, ids, out=out_f), a.reps)
        codec.decode_status(ctx)
        assert torch.equal(out_c, rows.index_select(0, ids))
        assert torch.equal(out_f, pq.reconstruct(out_c))

        def old_codes():
            codec.decode(ctx, tabs, enc, out=full)
            return full.index_select(0, ids)

        def old_fetch():
            return pq.reconstruct(old_codes())
        t_old = timed(old_codes, a.reps)
        t_oldf = timed(old_fetch, a.reps)
        res["select"].append({"ids": cnt, "decode_rows_ms": t_sel, "decode_all_gather_ms": t_old,
                              "fetch_ms": t_fet, "decode_all_gather_reconstruct_ms": t_oldf})
        if t_sel < t_old:
            crossover = cnt
        print(f"rows={n} ids=2^{lg}: decode_rows {t_sel:.4f} ms  (decode all + gather {t_old:.4f})"
              f"  fetch {t_fet:.4f} ms  (decode all + gather + reconstruct {t_oldf:.4f})", flush=True)
    res["decode_rows_wins_up_to_ids"] = crossover
    # ranges: the whole stream, and a 1 % slice that starts and ends inside a chunk
    t_rall = timed(lambda: codec.decode_range(ctx, tabs, enc, 0, n, out=full), a.reps)
    assert torch.equal(full, rows)
    first, cnt = n // 2 + 1, n // 100
    out_s = torch.empty((cnt, m), dtype=torch.uint8, device=dev)
    t_rs = timed(lambda: codec.decode_range(ctx, tabs, enc, first, cnt, out=out_s), a.reps)
    codec.decode_status(ctx)
    assert torch.equal(out_s, rows[first:first + cnt])

    def old_slice():
        codec.decode(ctx, tabs, enc, out=full)
        out_s.copy_(full[first:first + cnt])
    t_olds = timed(old_slice, a.reps)
    res.update({"range_all_ms": t_rall, "range_all_over_decode_all": t_rall / t_full,
                "range_slice_rows": cnt, "range_slice_ms": t_rs, "decode_all_copy_slice_ms": t_olds})
    print(f"rows={n}: decode all {t_full:.4f} ms  decode_range(all) {t_rall:.4f} ms "
          f"(x{t_rall / t_full:.3f})  decode_range(1 %) {t_rs:.4f} ms  (decode all + copy "
          f"{t_olds:.4f})  decode_rows wins up to {crossover} ids", flush=True)
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
