"""The regroup pass of IVF.add / IVF.compact beside the calls it replaces (diagnostic): HIP-event
times on one --nlist-list index of --rows SIFT-shaped rows, M = 8, K = 256, context mode, in
chunks of 4 and of 64 rows.  Per chunk size and row map:
    decode     (a) pqh_decode of the whole stream
    composed   (b) the route the library had: decode, then out[dest] = codes in torch (the rows
               with a destination and their destinations gathered outside the timed region)
    scatter    (c) pqh_decode_scatter through the map
    plan       pqh_ivf_regroup for that map
The maps: the identity, the regroup map for --add new rows (gaps left in every list), and
compaction maps with 10 % and 90 % of the rows dropped at random.  The three are timed
alternately in one process, --repeats times each after a warm-up (min / median / max), and (c) is
checked against (b) byte for byte.  Then, once per chunk size, wall-clock with a device
synchronisation around it:
    add        (d) a whole IVF.add of --add rows
    compact        a whole IVF.compact after remove() of 10 % of the ids

    python tools/bench_ivf_regroup.py [--rows 10000000] [--add 1000000] [--nlist 1024]
                                      [--reps 10] [--repeats 5] [--out profiles/ivf_regroup_bench.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from bench_search_filter import timed  # noqa: E402
from pq_huffman_amd import codec  # noqa: E402

# the compiler's metadata (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), kept beside the
# times they belong to; copied by hand when pqh_regroup.hip changes.  scat_rows<code type, u64
# words of a row (0: part by part), context>
KERNEL_RESOURCES = {
    "keep_popc": {"vgprs": 4, "sgprs": 12, "lds_bytes": 0, "spills": 0, "scratch": 0},
    "regroup_plan": {"vgprs": 14, "sgprs": 34, "lds_bytes": 0, "spills": 0, "scratch": 0},
    "scat_rows<u8,1,ctx>": {"vgprs": 31, "sgprs": 91, "lds_static_bytes": 256, "spills": 0, "scratch": 0},
    "scat_rows<u8,2,ctx>": {"vgprs": 34, "sgprs": 94, "lds_static_bytes": 256, "spills": 0, "scratch": 0},
    "scat_rows<u8,0,ctx>": {"vgprs": 31, "sgprs": 105, "lds_static_bytes": 256, "spills": 0, "scratch": 0},
    "scat_rows<u8,1>": {"vgprs": 26, "sgprs": 88, "lds_static_bytes": 256, "spills": 0, "scratch": 0},
    "scat_rows<u8,2>": {"vgprs": 27, "sgprs": 92, "lds_static_bytes": 256, "spills": 0, "scratch": 0},
    "scat_rows<u8,0>": {"vgprs": 27, "sgprs": 104, "lds_static_bytes": 256, "spills": 0, "scratch": 0},
    "scat_rows<u16,2>": {"vgprs": 27, "sgprs": 92, "lds_static_bytes": 256, "spills": 0, "scratch": 0},
    "scat_rows<u16,0>": {"vgprs": 27, "sgprs": 106, "lds_static_bytes": 256, "spills": 0, "scratch": 0},
}


def stats(t):
    t = sorted(t)
    return {"min": t[0], "median": t[len(t) // 2], "max": t[-1]}


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--add", type=int, default=1_000_000)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    d, n, m = 128, a.rows, 8
    x = bench.make_data(torch, n, d, 0x5EED, 0, dev)
    extra = bench.make_data(torch, a.add, d, 0xADD, 0, dev)
    sample = x[:200_000]
    ctx = codec.Context(0)
    pq = codec.PQ(ctx, bench.train_centroids(torch, sample, m, 256))
    coarse = codec.Coarse(ctx, bench.train_centroids(torch, sample, 1, a.nlist))
    gen = torch.Generator(device=dev).manual_seed(5)
    res = {"rows": n, "add": a.add, "nlist": a.nlist, "m": m, "k": 256, "context": 1,
           "reps": a.reps, "repeats": a.repeats, "kernel_resources": KERNEL_RESOURCES, "points": []}
    for chunk in (4, 64):
        ivf = codec.IVF.build(ctx, pq, coarse, x, chunk_vectors=chunk)
        codec.ivf_status(ctx)
        tables, enc = ivf.tables, ivf.enc
        _, add_offsets = coarse.layout(coarse.assign(extra))
        plans = {"identity": (None, None), "add": (None, add_offsets)}
        for drop in (10, 90):
            keep = torch.rand(n, device=dev, generator=gen) >= drop / 100.0
            plans[f"drop{drop}"] = (codec.pack_mask(ctx, keep), None)
        tmp = torch.empty((n, m), dtype=torch.uint8, device=dev)
        for name, (words, add) in plans.items():
            def plan():
                return codec.ivf_regroup(ctx, ivf.offsets, words, add, n=n)
            new_offsets, dest, _ = plan()
            n_out = int(new_offsets[-1].item())
            rows = torch.nonzero(dest >= 0).reshape(-1)
            to = dest[rows]
            whole = rows.numel() == n
            out_b = torch.zeros((n_out, m), dtype=torch.uint8, device=dev)
            out_c = torch.zeros((n_out, m), dtype=torch.uint8, device=dev)

            def composed():
                codec.decode(ctx, tables, enc, out=tmp)
                out_b[to] = tmp if whole else tmp[rows]

            calls = {"decode": lambda: codec.decode(ctx, tables, enc, out=tmp),
                     "composed": composed,
                     "scatter": lambda: codec.decode_scatter(ctx, tables, enc, dest, out_c),
                     "plan": plan}
            times = {w: [] for w in calls}
            for fn in calls.values():
                fn()
            assert torch.equal(out_b, out_c), (chunk, name)
            for _ in range(a.repeats):                    # (alternately, the same process)
                for w, fn in calls.items():
                    times[w].append(timed(fn, a.reps))
            codec.decode_status(ctx)
            codec.ivf_status(ctx)
            point = {"chunk": chunk, "map": name, "rows_out": n_out, "rows_kept": rows.numel(),
                     "bits_per_row": enc.bits / n}
            point.update({w + "_ms": stats(t) for w, t in times.items()})
            res["points"].append(point)
            print(json.dumps(point), flush=True)
            del out_b, out_c, rows, to, dest
        del tmp
        add_ms, first = wall_ms(lambda: ivf.add(extra))
        assert first == n and ivf.enc.n == n + a.add
        gone = torch.randperm(n + a.add, device=dev, generator=gen)[:(n + a.add) // 10]
        ivf.remove(gone)
        compact_ms, dropped = wall_ms(ivf.compact)
        assert dropped == gone.numel()
        point = {"chunk": chunk, "add_ms": add_ms, "compact_ms": compact_ms,
                 "compact_dropped": dropped, "rows_after": ivf.enc.n}
        res["points"].append(point)
        print(json.dumps(point), flush=True)
        del ivf, tables, enc
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
