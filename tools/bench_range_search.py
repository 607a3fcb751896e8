"""The range search beside the top-k search (diagnostic): per-call HIP-event times on one
index of --rows rows, SIFT shape (M = 8, K = 256, context mode), --chunk rows per chunk, for nq
in {8, 64, 512} queries.

  count     pqh_range_count_stream alone beside codec.search(k = 64) on the same stream and
            tables, the two interleaved repeat by repeat (the count pass does less per row: a
            compare and a popcount where the top-k scan offers to its lists).
  fill      count, fill and both at radii that give about 1e-5, 1e-3 and 0.1 of the rows per
            query (each query's own quantile of its distances).  The library built with
            -DPQH_RADIUS_NO_SKIP (PQH_LIB=... --tag noskip) has the fill pass decode every
            share whatever it counted: the two runs' fill times are what the skip rule removes.
  ivf       IVF.range_search beside IVF.search(k = 64) at 512 queries x --nprobe probes, plain
            and residual, every query's radius the distance of its 64th neighbour.

Every result is checked against the scan over the decoded codes (range_search_codes), bit for
bit.  Every point is timed --repeats times (min / median / max are kept).

    python tools/bench_range_search.py [--rows 1000000] [--chunk 4] [--nlist 1024] [--nprobe 16]
                                       [--reps 20] [--repeats 5] [--tag NAME] [--out FILE.json]
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from pq_huffman_amd import capi, codec  # noqa: E402


def timed(fn, reps, budget_ms=50.0):
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


def stats(t):
    t = sorted(t)
    return {"min": t[0], "median": t[len(t) // 2], "max": t[-1]}


def interleaved(fns, reps, repeats):
    """name -> spread, the calls timed in turn within every repeat"""
    t = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            t[name].append(timed(fn, reps))
    return {name: stats(v) for name, v in t.items()}


def fmt(s):
    return f"{s['median']:.4f} ms [{s['min']:.4f}, {s['max']:.4f}]"


def passes(ctx, tabs, enc, lut, radius, capacity):
    """(count, fill, lims, dist, ids): the two C calls over one plan and one set of buffers"""
    lib = capi.lib()
    nq = lut.shape[0]
    nbytes = ctypes.c_ulonglong(0)
    capi.check(lib.pqh_range_plan_bytes(ctx.ptr, enc.n, tabs.m, tabs.k, enc.chunk_vectors, nq, -1,
                                        0, ctypes.byref(nbytes)), "pqh_range_plan_bytes")
    plan = torch.empty((nbytes.value + 7) // 8, dtype=torch.int64, device=lut.device)
    lims = torch.empty(nq + 1, dtype=torch.int64, device=lut.device)
    dist = torch.empty(capacity, dtype=torch.float32, device=lut.device)
    ids = torch.empty(capacity, dtype=torch.int64, device=lut.device)
    args = (ctx.ptr, tabs.ptr, *codec._index_args(enc), lut.data_ptr(), nq, None, None, -1, 0,
            radius.data_ptr(), None, plan.data_ptr(), plan.numel() * 8, lims.data_ptr())

    def count():
        capi.check(lib.pqh_range_count_stream(*args), "pqh_range_count_stream")

    def fill():
        capi.check(lib.pqh_range_fill_stream(*args, capacity, 0, dist.data_ptr(), ids.data_ptr()),
                   "pqh_range_fill_stream")
    return count, fill, lims, dist, ids, nbytes.value


def quantile_radii(lut, codes, fractions):
    """fraction -> float32 (nq,): per query the distance below which that share of the rows lies"""
    n = codes.shape[0]
    idx = codes.long()
    out = {f: torch.empty(lut.shape[0], dtype=torch.float32, device=lut.device) for f in fractions}
    for q in range(lut.shape[0]):
        d = lut[q, 0][idx[:, 0]]
        for i in range(1, codes.shape[1]):
            d = d + lut[q, i][idx[:, i]]
        for f in fractions:
            out[f][q] = torch.kthvalue(d, max(1, int(f * n)) + 1).values
    return out


def same(a, b):
    return (torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and
            torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=4)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, default=16)
    ap.add_argument("--no-ivf", action="store_true")
    ap.add_argument("--tag", default="range")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    d, m, n = 128, 8, a.rows
    fractions = (1e-5, 1e-3, 0.1)
    x = bench.make_data(torch, n, d, 0x5EED, 0, dev)
    sample = x[:200_000]
    ctx = codec.Context(0)
    pq = codec.PQ(ctx, bench.train_centroids(torch, sample, m, 256))
    coarse = codec.Coarse(ctx, bench.train_centroids(torch, sample, 1, a.nlist))
    ivf = codec.IVF.build(ctx, pq, coarse, x, chunk_vectors=a.chunk)
    codec.ivf_status(ctx)
    queries = x[torch.arange(512, device=dev) * 997 % n].contiguous()
    codes = codec.decode(ctx, ivf.tables, ivf.enc)
    codec.decode_status(ctx)
    lut_all = codec.adc_tables(ctx, pq, queries)
    radii = quantile_radii(lut_all, codes, fractions)
    res = {"rows": n, "chunk": a.chunk, "m": m, "k": 256, "context": 1, "nlist": a.nlist,
           "nprobe": a.nprobe, "bits_per_row": ivf.enc.bits / n, "reps": a.reps,
           "repeats": a.repeats, "lib": os.path.basename(capi.LIB_PATH), "count": [], "fill": [],
           "ivf": []}

    for nq in (8, 64, 512):
        lut = lut_all[:nq].contiguous()
        # ---- the count pass beside the top-k scan (radius: the 1e-3 quantile)
        count, _, _, _, _, plan_bytes = passes(ctx, ivf.tables, ivf.enc, lut,
                                               radii[1e-3][:nq].contiguous(), 0)
        t = interleaved({"search_k64": lambda: codec.search(ctx, ivf.tables, ivf.enc, lut, 64),
                         "count": count}, a.reps, a.repeats)
        res["count"].append({"nq": nq, "plan_bytes": plan_bytes, **t})
        print(f"chunk={a.chunk} nq={nq}: search(k=64) {fmt(t['search_k64'])}  count pass "
              f"{fmt(t['count'])}  plan {plan_bytes} B", flush=True)
        # ---- count and fill at three selectivities
        for f in fractions:
            rad = radii[f][:nq].contiguous()
            want = codec.range_search_codes(ctx, codes, lut, rad)
            total = int(want[0][-1].item())
            count, fill, lims, dist, ids, _ = passes(ctx, ivf.tables, ivf.enc, lut, rad, total)
            count()
            fill()
            assert same((lims, dist, ids), want), (nq, f)

            def both():
                count()
                fill()
            t = interleaved({"count": count, "fill": fill, "both": both}, a.reps, a.repeats)
            res["fill"].append({"nq": nq, "fraction": f, "hits": total, **t})
            print(f"chunk={a.chunk} nq={nq} fraction={f:g} hits={total}: count {fmt(t['count'])}  "
                  f"fill {fmt(t['fill'])}  both {fmt(t['both'])}", flush=True)
        codec.decode_status(ctx)

    if not a.no_ivf:
        q = queries
        lists = coarse.assign(x)
        perm, _ = coarse.layout(lists)
        cent_res = bench.train_centroids(torch, coarse.residuals(x, lists, perm)[:200_000], m, 256)
        ivf_r = codec.IVF.build(ctx, codec.PQ(ctx, cent_res), coarse, x, chunk_vectors=a.chunk,
                                residual=True)
        codec.ivf_status(ctx)
        for kind, index in (("plain", ivf), ("residual", ivf_r)):
            top = index.search(q, a.nprobe, 64)
            rad = top[0][:, -1].contiguous()
            got = index.range_search(q, a.nprobe, rad)
            hits = int(got[0][-1].item())
            t = interleaved({"search_k64": lambda: index.search(q, a.nprobe, 64),
                             "range_search": lambda: index.range_search(q, a.nprobe, rad)},
                            a.reps, a.repeats)
            res["ivf"].append({"kind": kind, "nq": 512, "hits": hits, **t})
            print(f"ivf {kind} nq=512 nprobe={a.nprobe} hits={hits}: IVF.search(k=64) "
                  f"{fmt(t['search_k64'])}  IVF.range_search {fmt(t['range_search'])}", flush=True)
        codec.decode_status(ctx)

    if a.out:
        runs = {}
        if os.path.exists(a.out):
            with open(a.out) as fh:
                runs = json.load(fh)
        runs[f"{a.tag}_chunk{a.chunk}"] = res
        with open(a.out, "w") as fh:
            json.dump(runs, fh, indent=1, sort_keys=True)
            fh.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
