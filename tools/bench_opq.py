"""The rotated index on the bench's own data (diagnostic): per-call HIP-event times over
back-to-back calls after a warm-up.

  rotate   pqh_rotate of --rows x 128 and --rows x 96 (a dense random R): ms, the ratio of the
           2 * n * d^2 lane-operations of the chain to the time (and as a share of 256 CUs x 128
           lanes at --ghz; the clock the run held is NOT measured), and beside it torch.matmul
           of the same operands -- context only: another arithmetic, not the same bits
  moments  cross_moments of --moment-rows x 128 against itself (wall clock: the call waits)
  train    one opq_train at m = 8, K = 256 on --train-rows rows, outer = 8, inner = 2, from the
           identity: wall clock, and the error of every round
  search   IVF.search with and without rotation= at 1 and 512 queries on the 1,024-list index of
           tools/bench_ivf.py (nprobe 16, k 10); the same R-less index is what a build from
           before the rotation gives, so its column is the comparison
  bytes    the stream's bits per row with and without the rotation, both codebooks of as many
           Lloyd iterations, and the quantization error of both: a rotation that balances the
           subspaces flattens the symbol histograms, so some of what it gains in error it pays
           for in Huffman gain

    python tools/bench_opq.py [--rows 1000000] [--moment-rows 262144] [--train-rows 262144]
                              [--chunk 4] [--reps 20] [--ghz 2.4] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--moment-rows", type=int, default=262_144)
    ap.add_argument("--train-rows", type=int, default=262_144)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--chunk", type=int, default=4)
    ap.add_argument("--ghz", type=float, default=2.4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    d, m, k, n = 128, 8, 256, a.rows
    ctx = codec.Context(0)
    x = bench.make_data(torch, n, d, 0x5EED, 0, dev)
    res = {"rows": n, "reps": a.reps, "nominal_ghz": a.ghz, "clock_measured": False}
    lanes_per_s = 256 * 128 * a.ghz * 1e9

    # ---- rotate
    res["rotate"] = []
    for dd in (128, 96):
        xs = x[:, :dd].contiguous()
        R = np.random.default_rng(dd).normal(size=(dd, dd)).astype(np.float32)
        rot = codec.Rotation(ctx, R)
        Rd = torch.from_numpy(R).to(dev)
        out = torch.empty((n, dd), dtype=torch.float32, device=dev)
        t = timed(lambda: rot.apply(xs, out=out), a.reps)
        t_t = timed(lambda: rot.apply(xs, out=out, transpose=True), a.reps)
        t_torch = timed(lambda: torch.matmul(xs, Rd, out=out), a.reps)
        ops = 2.0 * n * dd * dd
        res["rotate"].append({"d": dd, "ms": t, "transpose_ms": t_t, "lane_ops": ops,
                              "share_of_vector_rate_at_nominal_clock": ops / (t * 1e-3) / lanes_per_s,
                              "gb_per_s": 2.0 * n * dd * 4 / (t * 1e-3) / 1e9,
                              "torch_matmul_ms": t_torch})
        print(f"rotate n={n} d={dd}: {t:.3f} ms (transpose {t_t:.3f} ms) = "
              f"{100 * ops / (t * 1e-3) / lanes_per_s:.1f} % of 256 x 128 lanes at {a.ghz} GHz "
              f"(clock not measured), {2.0 * n * dd * 4 / (t * 1e-3) / 1e9:.0f} GB/s of rows;  "
              f"torch.matmul {t_torch:.3f} ms (another arithmetic)", flush=True)
        rot.close()
        del xs, out, Rd

    # ---- moments
    xm = x[:a.moment_rows]
    codec.cross_moments(ctx, xm, xm)
    walls = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        codec.cross_moments(ctx, xm, xm)
        walls.append((time.perf_counter() - t0) * 1e3)
    res["moments"] = {"rows": a.moment_rows, "d": d, "wall_ms_min": min(walls),
                      "wall_ms_median": sorted(walls)[2], "products": float(a.moment_rows) * d * d}
    print(f"cross_moments {a.moment_rows} x {d} x {d}: {min(walls):.3f} ms min, "
          f"{sorted(walls)[2]:.3f} ms median of 5 (wall clock, the call waits)", flush=True)

    # ---- train
    xt = x[:a.train_rows]
    g = torch.Generator(device=dev).manual_seed(7)
    rows = torch.randperm(a.train_rows, generator=g, device=dev)[:k]
    init = np.ascontiguousarray(xt[rows].cpu().numpy().reshape(k, m, d // m).transpose(1, 0, 2))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    R, cent, errors = codec.opq_train(ctx, xt, m, k, init, outer=8, inner=2)
    t_train = time.perf_counter() - t0
    t0 = time.perf_counter()
    plain_cent = codec.kmeans_train(ctx, xt, init, 18)
    t_plain = time.perf_counter() - t0
    pq_plain = codec.PQ(ctx, plain_cent)
    plain_err = pq_plain.error(xt, pq_plain.assign(xt))
    res["train"] = {"rows": a.train_rows, "m": m, "k": k, "outer": 8, "inner": 2,
                    "wall_s": t_train, "plain_18_iterations_wall_s": t_plain, "errors": errors,
                    "plain_error": plain_err, "ratio": errors[-1] / plain_err}
    print(f"opq_train {a.train_rows} x {d}, m={m} K={k}, 8 x 2: {t_train:.2f} s "
          f"(18 plain Lloyd iterations {t_plain:.2f} s)  error {errors[0]:.1f} -> {errors[-1]:.1f}, "
          f"plain PQ {plain_err:.1f} (ratio {errors[-1] / plain_err:.3f})", flush=True)

    # ---- search and bytes: twin indexes on the 1,024 lists of tools/bench_ivf.py
    rot = codec.Rotation(ctx, R)
    c = x[torch.arange(1024, device=dev) * (n // 1024) + 3].contiguous()
    cq = codec.Coarse(ctx, c.cpu().numpy())
    cq_r = codec.Coarse(ctx, rot.apply(c).cpu().numpy())
    pq_r = codec.PQ(ctx, cent)
    plain = codec.IVF.build(ctx, pq_plain, cq, x, chunk_vectors=a.chunk, context=True)
    turned = codec.IVF.build(ctx, pq_r, cq_r, x, chunk_vectors=a.chunk, context=True, rotation=rot)
    codec.ivf_status(ctx)
    xr = rot.apply(x)
    res["bytes"] = {"plain_bits_per_row": plain.enc.bits / n, "rotated_bits_per_row": turned.enc.bits / n,
                    "plain_error": pq_plain.error(x, pq_plain.assign(x)),
                    "rotated_error": pq_r.error(xr, pq_r.assign(xr))}
    del xr
    print(f"stream: {plain.enc.bits / n:.2f} bits per row plain, {turned.enc.bits / n:.2f} rotated "
          f"(of {8 * m} raw); error {res['bytes']['plain_error']:.1f} plain, "
          f"{res['bytes']['rotated_error']:.1f} rotated", flush=True)
    queries_all = x[torch.arange(512, device=dev) * 997 + 5].contiguous()
    res["search"] = []
    for nq in (1, 512):
        q = queries_all[:nq].contiguous()
        pair = []
        for _ in range(3):   # the two sides alternately
            pair.append((timed(lambda: plain.search(q, 16, 10), a.reps),
                         timed(lambda: turned.search(q, 16, 10), a.reps)))
        t_rot = timed(lambda: rot.apply(q), a.reps)
        tp, tr = min(p[0] for p in pair), min(p[1] for p in pair)
        res["search"].append({"nq": nq, "nprobe": 16, "k": 10, "plain_ms": tp, "rotated_ms": tr,
                              "rotate_queries_ms": t_rot, "pairs_ms": pair})
        print(f"IVF.search nq={nq}: {tp:.4f} ms plain, {tr:.4f} ms rotated (min of 3 each, "
              f"alternated); rotating the queries alone {t_rot:.4f} ms", flush=True)
    codec.decode_status(ctx)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
