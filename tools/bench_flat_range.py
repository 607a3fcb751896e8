"""The flat range search beside the flat top-k of the same build (diagnostic; DESIGN.md section
4.5.22): codec.Flat over `--rows` of bench's SIFT-like 128-d rows, L2 and IP, nq = 1, 512 and
4,096, every query's radius its 64th neighbour's distance as Flat.search returns it.  Timed: the
count pass (pqh_flat_range_count), the fill pass (pqh_flat_range_fill) over the plan the count
left, the whole Python call (both, the read of lims[-1] between them and the allocations), and
Flat.search(k = 64) on the same inputs.  The methods alternate `--rounds` times after a warm-up,
each timing HIP events over back-to-back calls, the best of the rounds reported, with the chains
run (count and fill) and the fallback beside them; every point checks the hit counts against the
top-k's distances below the radius.

    python tools/bench_flat_range.py [--rows 1000000] [--reps 20] [--rounds 3] [--out FILE.json]
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from bench_flat import timed  # noqa: E402
from pq_huffman_amd import codec  # noqa: E402


def point(ctx, x, q, metric, reps, rounds):
    """one point: the methods alternating, the best of `rounds`"""
    n, nq = x.shape[0], q.shape[0]
    lib, sfx = codec.lib(), "_ip" if metric == "ip" else ""
    flat = codec.Flat(ctx, x)
    dist, _ = flat.search(q, 64, metric=metric)
    radius = dist[:, 63].contiguous()
    nbytes = ctypes.c_ulonglong(0)
    codec.check(lib.pqh_flat_range_plan_bytes(ctx.ptr, flat.ptr, nq, ctypes.byref(nbytes)))
    plan = torch.empty(nbytes.value // 8, dtype=torch.int64, device=x.device)
    lims = torch.empty(nq + 1, dtype=torch.int64, device=x.device)
    args = (ctx.ptr, flat.ptr, codec._ptr(q), nq, q.stride(0), codec._ptr(radius), None,
            codec._ptr(plan), nbytes.value, codec._ptr(lims))

    def count():
        codec.check(getattr(lib, "pqh_flat_range_count" + sfx)(*args))

    count()
    res = {"n": n, "d": x.shape[1], "nq": nq, "metric": metric, "hits": int(lims[-1].item())}
    res["count_chains"], res["fallback"] = flat.counts()
    # the rows strictly below the 64th neighbour's distance are among the top 64
    assert torch.equal(lims[1:] - lims[:-1], (dist < radius[:, None]).sum(dim=1)), res
    out = (torch.empty(res["hits"], dtype=torch.float32, device=x.device),
           torch.empty(res["hits"], dtype=torch.int64, device=x.device))

    def fill():
        codec.check(getattr(lib, "pqh_flat_range_fill" + sfx)(*args, res["hits"], 0,
                                                              codec._ptr(out[0]), codec._ptr(out[1])))

    fill()
    res["fill_chains"] = flat.counts()[0]
    res["count_chain_share"] = res["count_chains"] / (n * nq)
    methods = {"count_ms": count, "fill_ms": fill,
               "range_ms": lambda: flat.range_search(q, radius, metric=metric),
               "topk_ms": lambda: flat.search(q, 64, metric=metric)}
    for fn in methods.values():   # the warm-up
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in methods}
    for _ in range(rounds):
        for name, fn in methods.items():
            times[name].append(timed(fn, reps))
    for name, t in times.items():
        res[name] = min(t)
        res[name + "_all"] = t
    flat.close()
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = codec.Context(0)
    x = bench.make_data(torch, a.rows, 128, 0x5EED, 0, dev)
    q = bench.make_data(torch, 4096, 128, 0x5EED, 1, dev)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "rounds": a.rounds, "points": {}}
    for metric in ("l2", "ip"):
        for nq in (1, 512, 4096):
            res["points"][f"{metric}_nq{nq}"] = point(ctx, x, q[:nq], metric, a.reps, a.rounds)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write("\n")


if __name__ == "__main__":
    main()
