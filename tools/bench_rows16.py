"""Half-precision rows beside fp32 rows (diagnostic): codec.IVFFlat with
fp32, fp16 and bf16 storage of the same rows (bench rows rounded to bf16 first, so that all three
hold the same values) over one quantizer, lists and queries, and codec.Flat over the same three.
The forms alternate `--rounds` times after a warm-up, each timing HIP events over back-to-back
calls, the best of the rounds reported; beside the IVFFlat searches the scan kernels alone on
ready probes.  `--scan-only` stops after the 1,024-list points (for comparing builds of the scan,
e.g. -DPQH_ROWS16_JC=64 through PQH_LIB).

  points   1,024 lists: (512 queries, 16 probes), (1, 16), (4,096, 64); 4,096 lists: (512, 16)
           Flat: 512 queries, k = 64, d = 128 and d = 768

    python tools/bench_rows16.py [--rows 1000000] [--reps 20] [--rounds 3] [--scan-only] [--out FILE.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from bench_flat import timed  # noqa: E402
from pq_huffman_amd import codec  # noqa: E402

STORES = ("f32", "f16", "bf16")


def best(methods, reps, rounds):
    """the methods alternating after a warm-up: name -> (best ms, every round's ms)"""
    for fn in methods.values():
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in methods}
    for _ in range(rounds):
        for name, fn in methods.items():
            times[name].append(timed(fn, reps))
    res = {}
    for name, t in times.items():
        res[name + "_ms"] = min(t)
        res[name + "_ms_all"] = t
    return res


def ratios(res, stem):
    for s in STORES[1:]:
        res[f"{stem}_{s}_over_f32"] = res[f"{stem}_{s}_ms"] / res[f"{stem}_f32_ms"]
    return res


def point(ctx, index, q, nprobe, k, reps, rounds):
    probes = index["f32"].coarse.probe(q, nprobe, index["f32"].offsets)[2]
    methods = {}
    for s in STORES:
        methods[f"ivfflat_{s}"] = lambda s=s: index[s].search(q, nprobe, k)
    for s in STORES:
        methods[f"scan_{s}"] = lambda s=s: codec.flat_search_lists(ctx, index[s].x_sorted,
                                                                    index[s].offsets, probes, q, k)
    res = {"n": index["f32"].n, "nlist": index["f32"].coarse.nlist, "nq": q.shape[0],
           "nprobe": nprobe, "k": k, **best(methods, reps, rounds)}
    print(json.dumps(ratios(ratios(res, "ivfflat"), "scan")), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--scan-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = codec.Context(0)
    n, d, k = a.rows, 128, 64
    # rounded to bf16 (8 significant bits, a value of all three types): the same rows in every form
    x = bench.make_data(torch, n, d, 0x5EED, 0, dev).bfloat16().float()
    q = bench.make_data(torch, 4096, d, 0x5EED, 1, dev)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "rounds": a.rounds, "points": {},
           "flat": {}}
    plans = ((1024, ((512, 16), (1, 16), (4096, 64))), (4096, ((512, 16),)))
    for nlist, shapes in plans[:1] if a.scan_only else plans:
        init = x[torch.arange(nlist, device=dev) * (n // nlist) + 3].contiguous()
        cq = codec.Coarse(ctx, codec.kmeans_train(ctx, x, init.cpu().numpy()[None], 2))
        index = {s: codec.IVFFlat.build(ctx, cq, x, store=s) for s in STORES}
        codec.ivf_status(ctx)
        for nq, nprobe in shapes:
            res["points"][f"nlist{nlist}_nq{nq}_nprobe{nprobe}"] = point(
                ctx, index, q[:nq], nprobe, k, a.reps, a.rounds)
        codec.ivf_status(ctx)
        del index
        cq.close()
    for dd in () if a.scan_only else (128, 768):
        xs = x if dd == d else bench.make_data(torch, n * d // dd, dd, 0x5EED, 2, dev).bfloat16().float()
        qs = q[:512] if dd == d else bench.make_data(torch, 512, dd, 0x5EED, 3, dev)
        rows = {"f32": xs, "f16": xs.half(), "bf16": xs.bfloat16()}
        flats = {s: codec.Flat(ctx, rows[s]) for s in STORES}
        r = {"n": xs.shape[0], "d": dd, "nq": 512, "k": k,
             **best({f"flat_{s}": lambda s=s: flats[s].search(qs, k) for s in STORES}, a.reps, a.rounds)}
        for s in STORES:
            flats[s].search(qs, k)
            r[f"chains_{s}"], r[f"fallback_{s}"] = flats[s].counts()
            flats[s].close()
        res["flat"][f"d{dd}"] = ratios(r, "flat")
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write("\n")


if __name__ == "__main__":
    main()
