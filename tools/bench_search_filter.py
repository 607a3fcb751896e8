"""The filtered search beside the unfiltered one (diagnostic): per-call HIP-event times of
codec.search and of IVF.search (--nlist lists, --nprobe probes, schedule "query" and "list") on
one index, for nq in {8, 64, 512} queries, with keep=None, with an all-ones mask, with random
masks that keep 50 %, 10 % and 1 % of the rows, and with clustered masks of the same fractions
that keep or drop whole lists (deletions by partition: the case where whole steps are passed
over).  The plain search runs on the index's own stream, so a clustered mask is contiguous runs
of its rows.  Context mode, SIFT shape (M = 8, K = 256), --chunk rows per chunk, --rows rows.
Every point is timed --repeats times (min / median / max are kept) and checked bit for bit
against an unfiltered search over plain codes of the kept rows alone (search_codes,
search_codes_ranges on the compacted rows, the ids mapped back).

    python tools/bench_search_filter.py [--rows 1000000] [--chunk 4] [--nlist 1024] [--nprobe 16]
                                        [--k 10] [--reps 20] [--repeats 5] [--unfiltered]
                                        [--tag NAME] [--out FILE.json]

--unfiltered times the keep=None points alone and passes no keep= anywhere, so the same file
runs against a build from before the filter, for the comparison of the unfiltered paths.
With --out the result is merged into that file under "<tag>_chunk<C>"
(profiles/search_filter_bench.json holds the runs DESIGN.md section 4.5.7 quotes).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from pq_huffman_amd import codec  # noqa: E402


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


def spread(fn, reps, repeats):
    t = sorted(timed(fn, reps) for _ in range(repeats))
    return {"min": t[0], "median": t[len(t) // 2], "max": t[-1]}


def same(a, b):
    return torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))


def compacted(codes, kept):
    """(codes of the kept stream rows, those rows, first[r] = the kept rows before row r)"""
    if kept is None:
        return codes, None, None
    rows = torch.nonzero(kept).reshape(-1)
    first = torch.zeros(kept.numel() + 1, dtype=torch.int64, device=kept.device)
    first[1:] = torch.cumsum(kept.to(torch.int64), 0)
    return codes[rows].contiguous(), rows, first


def back(res, rows):
    """the ids of a search over compacted rows as stream rows"""
    if rows is None or rows.numel() == 0:
        return res
    return res[0], torch.where(res[1] >= 0, rows[res[1].clamp(min=0)], res[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=4)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, default=16)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--unfiltered", action="store_true")
    ap.add_argument("--tag", default="filter")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    d, m, k, n = 128, 8, a.k, a.rows
    x = bench.make_data(torch, n, d, 0x5EED, 0, dev)
    sample = x[:200_000]
    ctx = codec.Context(0)
    pq = codec.PQ(ctx, bench.train_centroids(torch, sample, m, 256))
    coarse = codec.Coarse(ctx, bench.train_centroids(torch, sample, 1, a.nlist))
    ivf = codec.IVF.build(ctx, pq, coarse, x, chunk_vectors=a.chunk)
    codec.ivf_status(ctx)
    queries = x[torch.arange(512, device=dev) * 997 % n].contiguous()
    lists = coarse.assign(x).to(torch.int64)              # by caller row
    del x, sample
    codes = codec.decode(ctx, ivf.tables, ivf.enc)
    codec.decode_status(ctx)
    lut_all = codec.adc_tables(ctx, pq, queries)

    gen = torch.Generator().manual_seed(0x5EED)
    masks = {"none": None}
    if not a.unfiltered:
        masks["ones"] = torch.ones(n, dtype=torch.bool, device=dev)
        for pct in (50, 10, 1):
            masks[f"random{pct}"] = (torch.rand(n, generator=gen) < pct / 100).to(dev)
        for pct in (50, 10, 1):
            of_list = (torch.rand(a.nlist, generator=gen) < pct / 100).to(dev)
            masks[f"clustered{pct}"] = of_list[lists]
    res = {"rows": n, "chunk": a.chunk, "m": m, "k": 256, "top_k": k, "context": 1,
           "nlist": a.nlist, "nprobe": a.nprobe, "bits_per_row": ivf.enc.bits / n, "reps": a.reps,
           "repeats": a.repeats, "points": []}
    for name, keep in masks.items():
        kw = {} if keep is None else {"keep": keep}
        kept = None if keep is None else keep[ivf.perm]       # by stream row
        words = None if keep is None else codec.pack_mask(ctx, keep, ivf.perm)
        kww = {} if keep is None else {"keep": words}
        ref_codes, ref_rows, first = compacted(codes, kept)
        ref_offsets = ivf.offsets if first is None else first[ivf.offsets]
        for nq in (8, 64, 512):
            q, lut = queries[:nq], lut_all[:nq].contiguous()
            # the references: unfiltered calls over the kept rows alone
            want_plain = back(codec.search_codes(ctx, ref_codes, lut, k), ref_rows)
            _, _, probes, _ = coarse.probe(q, a.nprobe, ivf.offsets)
            ptr, ranges = codec.probe_ranges(ref_offsets, probes)
            want_ivf = back(codec.search_codes_ranges(ctx, ref_codes, lut, ptr, ranges, k), ref_rows)
            want_ivf = (want_ivf[0], torch.where(want_ivf[1] >= 0,
                                                 ivf.perm[want_ivf[1].clamp(min=0)], want_ivf[1]))
            calls = {
                "plain": lambda: codec.search(ctx, ivf.tables, ivf.enc, lut, k, **kww),
                "ivf_query": lambda: ivf.search(q, a.nprobe, k, schedule="query", **kw),
                "ivf_list": lambda: ivf.search(q, a.nprobe, k, schedule="list", **kw),
            }
            point = {"mask": name, "kept": 1.0 if keep is None else float(keep.float().mean()), "nq": nq}
            for what, fn in calls.items():
                assert same(fn(), want_plain if what == "plain" else want_ivf), (name, nq, what)
                point[what + "_ms"] = spread(fn, a.reps, a.repeats)
            codec.decode_status(ctx)
            res["points"].append(point)
            print(f"chunk={a.chunk} mask={name} kept={point['kept']:.3f} nq={nq}: " +
                  "  ".join(f"{w} {point[w + '_ms']['median']:.4f} ms "
                            f"[{point[w + '_ms']['min']:.4f}, {point[w + '_ms']['max']:.4f}]"
                            for w in calls), flush=True)
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
