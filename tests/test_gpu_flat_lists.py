"""codec.flat_search_lists and codec.IVFFlat on the GPU: ids and the raw bits of dist equal those
of the definition (tests/flat_lists_ref.py).  No tolerance anywhere: every distance is the chain."""
import numpy as np
import pytest

import flat_lists_ref
import ivf_ref

pytestmark = pytest.mark.gpu


def _normal(n, d, nq, rng):
    return (rng.standard_normal((n, d)).astype(np.float32),
            rng.standard_normal((nq, d)).astype(np.float32))


def _near_ties(n, d, nq, rng):
    """every row of the first half twice, some a third time one ulp off in one coordinate, and
    queries that are copies of rows (the world of test_gpu_flat.py)"""
    x, q = _normal(n, d, nq, rng)
    half = n // 2
    x[half:2 * half] = x[:half]
    for v in range(0, half // 2, 3):
        x[v + 1] = x[v]
        x[v + 1, v % d] = np.nextafter(x[v, v % d], np.float32(np.inf))
    q[::4] = x[rng.integers(0, n, size=len(q[::4]))]
    return x, q


WORLDS = {"normal": _normal, "near_ties": _near_ties,
          "grid": lambda n, d, nq, rng: ivf_ref.integer_grid(n, d, nq, int(rng.integers(1 << 30)))}

# name: (list lengths, d, ld_x, nq, nprobe, k, options).  A tile is 256 rows, a unit holds 16
# pairs (4 when k > 64), a unit of a list is cut into groups from a mean list of 2,048 rows on
# or when the units are fewer than the compute units -- every case here -- and groups= sets them.
# ld_x == d with d % 4 == 0 takes the float4 loads, everything else the scalar ones.
EDGE = [0, 1, 63, 64, 65, 257, 2300]
CASES = {
    "edges": (EDGE, 32, 35, 6, 3, 64, {}),
    "edges_one_group": (EDGE, 32, 32, 6, 3, 64, {"groups": 1}),
    "edges_three_groups": (EDGE, 32, 32, 6, 3, 64, {"groups": 3, "minus": True}),
    "pairs_17": ([300, 40], 3, 5, 17, 2, 1, {}),
    "pairs_5_wide": ([700, 65, 0], 33, 40, 5, 3, 200, {}),
    "wide_edges": (EDGE, 8, 8, 9, 4, 200, {"id_base": 7}),
    "d1": ([257, 64], 1, 2, 3, 2, 64, {}),
    "d130": ([65, 300, 1], 130, 133, 4, 2, 10, {"id_base": 2 ** 40 - 5}),
    "padding": ([5, 3, 0, 1000], 16, 16, 3, 2, 64, {"probes": [[0, 1], [2, -1], [1, 2]]}),
    "nprobe_above_nlist": ([70, 0, 130], 5, 8, 4, 5, 64, {"minus": True}),
    "tile_masked": ([1200, 300], 32, 32, 7, 2, 64, {"keep": "tile"}),
    "none_kept": ([300, 300], 4, 4, 3, 2, 5, {"keep": "none"}),
    "near_ties": ([500, 700, 65], 8, 8, 20, 2, 10, {"world": "near_ties"}),
    "grid": ([500, 700, 65], 8, 12, 20, 2, 64, {"world": "grid", "keep": "half"}),
}
KEEPS = {"tile": lambda n, rng: (rng.random(n) < 0.5) & (np.arange(n) // 256 != 2),
         "half": lambda n, rng: rng.random(n) < 0.5, "none": lambda n, rng: np.zeros(n, bool)}


@pytest.fixture(scope="module")
def gpu():
    import torch
    from pq_huffman_amd import codec
    assert torch.cuda.is_available()
    return torch, codec, codec.Context(0), codec.Context(0).set_search_max_k(256)


def _equal(got, want):
    got = [t.cpu().numpy() for t in got]
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_cases(gpu, metric, case):
    torch, codec, ctx, wide = gpu
    lengths, d, ld_x, nq, nprobe, k, opt = CASES[case]
    rng = np.random.default_rng(len(case) + d)
    offsets = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    n, nlist = int(offsets[-1]), len(lengths)
    x, q = WORLDS[opt.get("world", "normal")](n, d, nq, rng)
    if "probes" in opt:
        probes = np.array(opt["probes"], np.int64)
    else:   # every query on the longest list, then distinct others, -1 behind them
        probes = np.full((nq, nprobe), -1, np.int64)
        longest = int(np.argmax(lengths))
        others = [l for l in range(nlist) if l != longest]
        for i in range(nq):
            row = [longest] + list(rng.permutation(others))
            probes[i, :min(nprobe, nlist)] = row[:nprobe]
        if opt.get("minus"):
            probes[::2, -1] = -1
    keep = KEEPS[opt["keep"]](n, rng) if "keep" in opt else None
    base = opt.get("id_base", 0)
    buf = torch.full((n, ld_x), float("nan"), device="cuda")   # NaN between the rows
    buf[:, :d] = torch.from_numpy(x)
    c = wide if k > 64 else ctx
    c.set_tuning(search_groups=opt.get("groups", 0))
    try:
        got = codec.flat_search_lists(c, buf, torch.from_numpy(offsets).cuda(),
                                      torch.from_numpy(probes).cuda(), torch.from_numpy(q).cuda(), k,
                                      metric=metric, id_base=base, d=d,
                                      keep=None if keep is None else torch.from_numpy(keep).cuda())
        codec.ivf_status(c)
    finally:
        c.set_tuning(search_groups=0)
    _equal(got, flat_lists_ref.search(q, x, offsets, probes, k, metric, keep, base))


def test_bad_probes_and_offsets_are_reported_and_skipped(gpu):
    torch, codec, ctx, _ = gpu
    x, q = _normal(300, 8, 3, np.random.default_rng(2))
    offsets = np.array([0, 100, 90, 250, 400], np.int64)   # list 1 reversed, list 3 past n
    probes = np.array([[0, 1], [7, 2], [3, -5]], np.int64)
    got = codec.flat_search_lists(ctx, torch.from_numpy(x).cuda(), torch.from_numpy(offsets).cuda(),
                                  torch.from_numpy(probes).cuda(), torch.from_numpy(q).cuda(), 10)
    with pytest.raises(codec.PqhError):
        codec.ivf_status(ctx)
    _equal(got, flat_lists_ref.search(q, x, offsets, probes, 10))


def test_no_rows_and_no_queries(gpu):
    torch, codec, ctx, _ = gpu
    zero = torch.zeros(3, dtype=torch.int64, device="cuda")
    probes = torch.zeros((2, 1), dtype=torch.int64, device="cuda")
    q = torch.ones((2, 8), device="cuda")
    dist, rows = codec.flat_search_lists(ctx, torch.zeros((0, 8), device="cuda"), zero, probes, q, 4)
    assert torch.isinf(dist).all() and (rows == -1).all()
    assert codec.flat_search_lists(ctx, q, zero, probes[:0], q[:0], 4)[0].shape == (0, 4)


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_ivfflat_probing_every_list_is_flat(gpu, metric):
    torch, codec, ctx, _ = gpu
    n, d, nlist, nq, k = 3000, 16, 8, 12, 10
    x, q = _normal(n, d, nq, np.random.default_rng(9))
    xd, qd = torch.from_numpy(x).cuda(), torch.from_numpy(q).cuda()
    coarse = codec.Coarse(ctx, x[:nlist])
    index = codec.IVFFlat.build(ctx, coarse, xd, metric=metric, assign="screen")
    flat = codec.Flat(ctx, xd)
    dist, ids = index.search(qd, nlist, k)
    want = flat.search(qd, k, metric=metric)
    assert torch.equal(ids, want[1]) and torch.equal(dist.view(torch.int32), want[0].view(torch.int32))
    gone = ids[:, 0].unique()
    index.remove(ids[:, 0])
    assert index.live_count() == n - gone.numel()
    keep = torch.ones(n, dtype=torch.bool, device="cuda")
    keep[gone] = False
    for got in (index.search(qd, nlist, k), index.search(qd, nlist, k, keep=keep)):
        assert not torch.isin(got[1], gone).any()
        want = flat.search(qd, k, metric=metric, keep=keep)
        assert torch.equal(got[1], want[1]) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
    flat.close()
    coarse.close()
