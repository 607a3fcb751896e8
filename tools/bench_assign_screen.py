"""PQ assignment mode 2 (the LDS-resident screen) beside mode 1 (the exact kernel) at shapes no
MFMA kernel served before (diagnostic): HIP-event times over back-to-back calls
after a warm-up that also builds the prepared image, the two modes alternating three times, the
best of the three, and the codes compared at every point.  Standard-normal rows and codes.

  768-d, m = 16, K = 256 (dsub 48) | 128-d, m = 16, K = 16 | 128-d, m = 8, K = 1024, --rows rows
  262,144 x 128, m = 1, K = 1024: the assignment of a coarse Lloyd iteration, and the same through
  kmeans_train (one iteration, host clock: the call is synchronous), modes 0 and 2

    python tools/bench_assign_screen.py [--rows 1000000] [--reps 10] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pq_huffman_amd import codec  # noqa: E402


def timed(fn, reps, budget_ms=1500.0):
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


def assign_point(ctx, n, d, m, k, reps, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((n, d), device="cuda", generator=g)
    cent = torch.randn((m, k, d // m), device="cuda", generator=g).cpu().numpy()
    pq = codec.PQ(ctx, cent)
    out = {mode: pq.assign_parts(x, mode=mode) for mode in (1, 2)}   # (warm-up; builds the image)
    reranked, fallback = pq.screen_counts()
    equal = bool(torch.equal(out[1], out[2]))
    ms = {1: [], 2: []}
    for _ in range(3):
        for mode in (1, 2):
            ms[mode].append(timed(lambda: pq.assign_parts(x, parts=out[mode], mode=mode), reps))
    pq.close()
    return dict(n=n, d=d, m=m, k=k, dsub=d // m, mode1_ms=min(ms[1]), mode2_ms=min(ms[2]),
                mode1_all=ms[1], mode2_all=ms[2], ratio=min(ms[1]) / min(ms[2]),
                reranked=reranked, fallback=fallback, pairs=n * m, codes_equal=equal)


def kmeans_point(ctx, n, d, k, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((n, d), device="cuda", generator=g)
    init = x[:k].cpu().numpy().reshape(1, k, d)
    ms, got = {0: [], 2: []}, {}
    for it in range(4):   # (the first round is the warm-up)
        for mode in (0, 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got[mode] = codec.kmeans_train(ctx, x, init, 1, mode=mode)
            if it:
                ms[mode].append((time.perf_counter() - t0) * 1e3)
    return dict(n=n, d=d, m=1, k=k, dsub=d, iters=1, mode0_ms=min(ms[0]), mode2_ms=min(ms[2]),
                mode0_all=ms[0], mode2_all=ms[2], ratio=min(ms[0]) / min(ms[2]),
                centroids_equal=got[0].tobytes() == got[2].tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    ctx = codec.Context(0)
    res = dict(device=torch.cuda.get_device_name(0), points=[
        assign_point(ctx, a.rows, 768, 16, 256, a.reps, 1),
        assign_point(ctx, a.rows, 128, 16, 16, a.reps, 2),
        assign_point(ctx, a.rows, 128, 8, 1024, a.reps, 3),
        assign_point(ctx, 262_144, 128, 1, 1024, a.reps, 4)],
        kmeans=kmeans_point(ctx, 262_144, 128, 1024, 4))
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
