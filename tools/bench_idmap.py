"""The Elias-Fano id map beside the int64 perm / inv it replaces (diagnostic): HIP-event times of
back-to-back calls, median [min, max] of --repeats repeats, the two sides of every row timed
alternately, repeat by repeat, in one process.  The baseline is always the int64 path.
    ids        perm[rows.clamp(min=0)] + where            | idmap.ids(rows)
               512 x 64 and 512 x 256 rows (1/64 of them -1) of a --rows map
    pack       pack_mask(keep, perm)                      | idmap.pack_mask(keep), --rows and --big
    build      IdMap(perm, offsets) alone, --rows and --big rows, with the bytes per id
    search     IVF.search on the plain twin               | the same on the compressed twin
               512 queries x 16 probes, k = 64, with and without keep=
    add        IVF.add of --add rows, wall clock with a device synchronisation around it

    python tools/bench_idmap.py [--rows 1000000] [--big 10000000] [--add 100000] [--nlist 1024]
                                [--reps 20] [--repeats 5] [--out profiles/idmap_bench.json]
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


def stats(t):
    t = sorted(t)
    return {"min": t[0], "median": t[len(t) // 2], "max": t[-1]}


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def pair(res, name, base, new, a, **extra):
    """both sides alternately; one point"""
    times = {"base": [], "new": []}
    for _ in range(a.repeats):
        times["base"].append(timed(base, a.reps))
        times["new"].append(timed(new, a.reps))
    point = dict(what=name, base_ms=stats(times["base"]), new_ms=stats(times["new"]), **extra)
    point["ratio_of_medians"] = point["new_ms"]["median"] / point["base_ms"]["median"]
    res["points"].append(point)
    print(json.dumps(point), flush=True)


def layout_of(n, nlist, n_ids, dev, gen):
    """a perm and offsets as an index of n rows of n_ids ids has them: random lists, the ids
    ascending inside each"""
    lists = torch.randint(0, nlist, (n,), device=dev, generator=gen, dtype=torch.int32)
    perm, offsets = codec.ivf_layout(lists.long(), nlist)
    if n_ids > n:   # a compacted index: n of the n_ids ids, in the same order
        ids = torch.sort(torch.randperm(n_ids, device=dev, generator=gen)[:n]).values
        perm = ids[perm]
    return perm.contiguous(), offsets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--big", type=int, default=10_000_000)
    ap.add_argument("--add", type=int, default=100_000)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = codec.Context(0)
    gen = torch.Generator(device=dev).manual_seed(7)
    res = {"rows": a.rows, "big": a.big, "add": a.add, "nlist": a.nlist, "reps": a.reps,
           "repeats": a.repeats, "points": []}

    # ---- the map alone ----
    for n, n_ids, nlist in ((a.rows, a.rows, a.nlist), (a.big, a.big + a.big // 10, 4 * a.nlist)):
        perm, offsets = layout_of(n, nlist, n_ids, dev, gen)
        build = [timed(lambda: codec.IdMap(ctx, perm, offsets, n_ids), a.reps) for _ in range(a.repeats)]
        m = codec.IdMap(ctx, perm, offsets, n_ids)
        codec.ivf_status(ctx)
        assert torch.equal(m.decode(), perm)
        point = {"what": "build", "rows": n, "n_ids": n_ids, "nlist": nlist, "ms": stats(build),
                 "bytes": m.nbytes, "bytes_per_id": m.nbytes / n_ids,
                 "bytes_per_row_without_reverse": codec.idmap_bytes(n, n_ids, nlist, False) / n,
                 "int64_bytes_per_id": (8 * n + 8 * n_ids) / n_ids}
        res["points"].append(point)
        print(json.dumps(point), flush=True)
        decode = [timed(lambda: m.decode(), a.reps) for _ in range(a.repeats)]
        res["points"].append({"what": "decode", "rows": n, "ms": stats(decode)})
        print(json.dumps(res["points"][-1]), flush=True)
        if n == a.rows:
            for k in (64, 256):
                rows = torch.randint(0, n, (512, k), device=dev, generator=gen)
                rows[torch.rand((512, k), device=dev, generator=gen) < 1 / 64] = -1
                want = torch.where(rows >= 0, perm[rows.clamp(min=0)], rows)
                assert torch.equal(m.ids(rows), want)
                pair(res, f"ids 512x{k}", lambda: torch.where(rows >= 0, perm[rows.clamp(min=0)], rows),
                     lambda: m.ids(rows), a, rows=n)
        if n_ids == n:
            keep = torch.rand(n_ids, device=dev, generator=gen) < 0.5
            assert torch.equal(m.pack_mask(keep), codec.pack_mask(ctx, keep, perm))
            pair(res, "pack_mask", lambda: codec.pack_mask(ctx, keep, perm), lambda: m.pack_mask(keep),
                 a, rows=n)
        else:
            keep = torch.rand(n_ids, device=dev, generator=gen) < 0.5
            assert torch.equal(m.pack_mask(keep), codec.pack_mask(ctx, keep[perm]))
            pair(res, "pack_mask (compacted: keep[perm] first)",
                 lambda: codec.pack_mask(ctx, keep[perm]), lambda: m.pack_mask(keep), a, rows=n)
        codec.ivf_status(ctx)
        del perm, offsets, m, keep

    # ---- the index ----
    d, m_parts, n = 128, 8, a.rows
    x = bench.make_data(torch, n, d, 0x5EED, 0, dev)
    extra = bench.make_data(torch, a.add, d, 0xADD, 0, dev)
    sample = x[:200_000]
    pq = codec.PQ(ctx, bench.train_centroids(torch, sample, m_parts, 256))
    coarse = codec.Coarse(ctx, bench.train_centroids(torch, sample, 1, a.nlist))
    plain = codec.IVF.build(ctx, pq, coarse, x)
    packed = codec.IVF.build(ctx, pq, coarse, x, compress_ids=True)
    q = x[torch.randperm(n, device=dev, generator=gen)[:512]] + 1.0
    keep = torch.rand(n, device=dev, generator=gen) < 0.5
    for kp, name in ((None, "search"), (keep, "search keep=")):
        for schedule in ("query", "list"):
            want, got = plain.search(q, 16, 64, schedule, keep=kp), packed.search(q, 16, 64, schedule, keep=kp)
            assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])
            pair(res, f"{name} {schedule}", lambda: plain.search(q, 16, 64, schedule, keep=kp),
                 lambda: packed.search(q, 16, 64, schedule, keep=kp), a, rows=n, id_bytes_base=plain.id_bytes(),
                 id_bytes_new=packed.id_bytes())
    base_ms, _ = wall_ms(lambda: plain.add(extra))
    new_ms, _ = wall_ms(lambda: packed.add(extra))
    assert torch.equal(packed.idmap.decode(), plain.perm)
    res["points"].append({"what": "add", "rows": n, "add": a.add, "base_ms": base_ms, "new_ms": new_ms,
                          "id_bytes_base": plain.id_bytes(), "id_bytes_new": packed.id_bytes()})
    print(json.dumps(res["points"][-1]), flush=True)
    codec.ivf_status(ctx)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
