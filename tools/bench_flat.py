"""The flat (exact) search beside the routes a caller had (diagnostic):
codec.Flat.search over `--rows` raw fp32 rows, Coarse(ctx, x).probe over the same rows (the only
in-library top-k over raw rows before it; k <= 64), and torch's matmul plus topk (another
arithmetic: context, not a gate).  The methods alternate `--rounds` times after a warm-up, each
timing HIP events over back-to-back calls, the best of the rounds reported; Flat and the probe
are compared on every query of every point, and the chains / fallback counts stand beside the
times.

  gate     bench's SIFT-like rows and Gaussian rows, 128-d, 512 queries, k = 64, both metrics
  beside   on the SIFT-like rows, L2: k = 10 and 256, nq = 1 and 4,096, and d = 768

    python tools/bench_flat.py [--rows 1000000] [--reps 20] [--rounds 3] [--out FILE.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from pq_huffman_amd import codec  # noqa: E402


def timed(fn, reps, budget_ms=600.0):
    """ms per call over back-to-back calls; slow calls get fewer than `reps` of them"""
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


def torch_topk(x, q, k, metric):
    s = q @ x.T
    if metric == "l2":
        s = (x * x).sum(1)[None, :] - 2.0 * s
        return (s.topk(k, largest=False)[0] + (q * q).sum(1)[:, None],)
    return (-s.topk(k, largest=True)[0],)


def point(ctx, x, q, k, metric, reps, rounds, coarse):
    """one point: the methods alternating, the best of `rounds`; Flat against the probe"""
    n = x.shape[0]
    flat = codec.Flat(ctx, x)
    methods = {"flat_ms": lambda: flat.search(q, k, metric=metric),
               "torch_ms": lambda: torch_topk(x, q, k, metric)}
    if coarse is not None and k <= 64:
        offsets = torch.arange(n + 1, device=x.device)
        methods["probe_ms"] = lambda: coarse.probe(q, k, offsets, metric=metric)[2:]
    for fn in methods.values():   # the warm-up
        fn()
    torch.cuda.synchronize()
    res = {"n": n, "d": x.shape[1], "nq": q.shape[0], "k": k, "metric": metric}
    dist, ids = flat.search(q, k, metric=metric)
    res["chains"], res["fallback"] = flat.counts()
    res["chain_share"] = res["chains"] / (n * q.shape[0])
    if "probe_ms" in methods:
        probes, pdist = methods["probe_ms"]()
        res["equal_to_probe"] = bool(torch.equal(ids, probes) and
                                     torch.equal(dist.view(torch.int32), pdist.view(torch.int32)))
        assert res["equal_to_probe"], res
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
    ctx = codec.Context(0).set_search_max_k(256)
    n = a.rows
    g = torch.Generator(device=dev).manual_seed(0x5EED)
    data = {"sift_like": (bench.make_data(torch, n, 128, 0x5EED, 0, dev),
                          bench.make_data(torch, 4096, 128, 0x5EED, 1, dev)),
            "gaussian": (torch.randn((n, 128), generator=g, device=dev),
                         torch.randn((4096, 128), generator=g, device=dev))}
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "rounds": a.rounds,
           "gate": {}, "beside": {}}
    for name, (x, q) in data.items():
        coarse = codec.Coarse(ctx, x.cpu().numpy())
        for metric in ("l2", "ip"):
            res["gate"][f"{name}_{metric}"] = point(ctx, x, q[:512], 64, metric, a.reps, a.rounds,
                                                    coarse)
        if name == "sift_like":
            for k, nq in ((10, 512), (256, 512), (64, 1), (64, 4096)):
                res["beside"][f"k{k}_nq{nq}"] = point(ctx, x, q[:nq], k, "l2", a.reps, a.rounds,
                                                      coarse)
        coarse.close()
    del data
    x = bench.make_data(torch, n, 768, 0x5EED, 0, dev)
    q = bench.make_data(torch, 512, 768, 0x5EED, 1, dev)
    res["beside"]["d768"] = point(ctx, x, q, 64, "l2", a.reps, a.rounds, None)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write("\n")


if __name__ == "__main__":
    main()
