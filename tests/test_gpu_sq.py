"""codec.SQ, codec.sq_search_lists and codec.IVFSQ on the GPU against the definition
(tests/sq_ref.py): parameters, codes, decoded rows, ids and the raw bits of dist.  No tolerance
anywhere."""
import numpy as np
import pytest

import sq_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    from pq_huffman_amd import codec
    assert torch.cuda.is_available()
    return torch, codec, codec.Context(0), codec.Context(0).set_search_max_k(256)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _equal(got, want):
    got = [t.cpu().numpy() for t in got]
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(_bits(got[0]), _bits(want[0]))


def _normal(n, d, nq, rng):
    return (rng.standard_normal((n, d)).astype(np.float32),
            rng.standard_normal((nq, d)).astype(np.float32))


def _near_ties(n, d, nq, rng):
    """every row of the first half twice, some a third time one ulp off in one coordinate, and
    queries that are copies of rows"""
    x, q = _normal(n, d, nq, rng)
    half = n // 2
    x[half:2 * half] = x[:half]
    for v in range(0, half // 2, 3):
        x[v + 1] = x[v]
        x[v + 1, v % d] = np.nextafter(x[v, v % d], np.float32(np.inf))
    q[::4] = x[rng.integers(0, n, size=len(q[::4]))]
    return x, q


@pytest.mark.parametrize("perm", [False, True])
@pytest.mark.parametrize("n,d,ld_x", [(1, 1, 1), (257, 3, 5), (1000, 64, 64), (300, 130, 133)])
def test_train_encode_decode(gpu, n, d, ld_x, perm):
    torch, codec, ctx, _ = gpu
    rng = np.random.default_rng(n + d)
    x = (3 * rng.standard_normal((n, d)) + 1).astype(np.float32)
    if d > 1:   # a constant column, and one with a NaN and an inf among its values
        x[:, 0] = 2.5
        x[0, d - 1], x[1, d - 1] = np.nan, -np.inf
    buf = torch.full((n, ld_x), float("nan"), device="cuda")   # NaN between the rows
    buf[:, :d] = torch.from_numpy(x)
    xd = buf[:, :d]
    sq = codec.SQ.train(ctx, xd)
    vmin, step = sq_ref.train(x)
    assert np.array_equal(_bits(sq.vmin.cpu().numpy()), _bits(vmin))
    assert np.array_equal(_bits(sq.step.cpu().numpy()), _bits(step))
    p = rng.permutation(n) if perm else np.arange(n)
    want = sq_ref.encode(x[p], vmin, step)
    dec = sq_ref.decode(want, vmin, step)
    rows = np.array([-1, n - 1, 0, -1], np.int64)
    for ld in ((d + 3) // 4 * 4, d + 1 if (d + 1) % 4 else d + 2):   # dword stores, byte stores
        codes = sq.encode(xd, torch.from_numpy(p).cuda() if perm else None, ld=ld)
        assert codes.shape == (n, ld) and not codes[:, d:].any()
        assert np.array_equal(codes[:, :d].cpu().numpy(), want)
        assert np.array_equal(_bits(sq.decode(codes).cpu().numpy()), _bits(dec))
        got = sq.decode(codes, torch.from_numpy(rows).cuda()).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(np.where(rows[:, None] < 0, np.float32(0), dec[rows])))
    codec.ivf_status(ctx)


# name: (list lengths, d, ld_c, nq, nprobe, k, options).  A tile is 256 rows, a chunk 64
# dimensions, a unit holds 16 pairs (4 when k > 64); groups= sets the groups of a unit.  ld_c % 4
# == 0 takes the dword loads, everything else the byte loads.
EDGE = [0, 1, 63, 64, 65, 257, 2300]
CASES = {
    "edges": (EDGE, 32, 32, 6, 3, 64, {}),
    "edges_bytes": (EDGE, 32, 35, 6, 3, 64, {"groups": 1}),
    "three_groups": (EDGE, 64, 64, 6, 3, 64, {"groups": 3, "minus": True}),
    "pairs_17": ([300, 40], 3, 3, 17, 2, 1, {}),
    "d1": ([257, 64], 1, 4, 3, 2, 64, {}),
    **{f"chunk_d{d}": ([65, 300, 1], d, (d + 3) // 4 * 4, 4, 2, 10, {"id_base": 2 ** 40 - 5})
       for d in (63, 65, 128, 130)},
    "wide": ([700, 65, 0], 33, 36, 5, 3, 200, {}),
    "wide_edges": (EDGE, 8, 8, 9, 4, 200, {}),
    "tile_masked": ([1200, 300], 32, 32, 7, 2, 64, {"keep": "tile"}),
    "none_kept": ([300, 300], 4, 4, 3, 2, 5, {"keep": "none"}),
    "ties": ([500, 700, 65], 8, 8, 20, 2, 10, {"ties": True}),
}
KEEPS = {"tile": lambda n, rng: (rng.random(n) < 0.5) & (np.arange(n) // 256 != 2),
         "none": lambda n, rng: np.zeros(n, bool)}


def _device_codes(torch, codes, ld_c):
    buf = torch.full((len(codes), ld_c), 255, dtype=torch.uint8, device="cuda")   # 255 between the rows
    buf[:, :codes.shape[1]] = torch.from_numpy(codes)
    return buf


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_search_lists(gpu, metric, case):
    torch, codec, ctx, wide = gpu
    lengths, d, ld_c, nq, nprobe, k, opt = CASES[case]
    rng = np.random.default_rng(len(case) + d)
    offsets = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    n, nlist = int(offsets[-1]), len(lengths)
    x, q = (_near_ties if opt.get("ties") else _normal)(n, d, nq, rng)
    # (ties: trained on a tenth of the rows, so that the codes 0 and 255 clamp the others)
    vmin, step = sq_ref.train(x[::10] if opt.get("ties") else x)
    codes = sq_ref.encode(x, vmin, step)
    # every query on the longest list, then distinct others, -1 behind them
    probes = np.full((nq, nprobe), -1, np.int64)
    longest = int(np.argmax(lengths))
    others = [l for l in range(nlist) if l != longest]
    for i in range(nq):
        probes[i, :min(nprobe, nlist)] = ([longest] + list(rng.permutation(others)))[:nprobe]
    if opt.get("minus"):
        probes[::2, -1] = -1
    keep = KEEPS[opt["keep"]](n, rng) if "keep" in opt else None
    base = opt.get("id_base", 0)
    c = wide if k > 64 else ctx
    sq = codec.SQ(c, torch.from_numpy(vmin).cuda(), torch.from_numpy(step).cuda())
    c.set_tuning(search_groups=opt.get("groups", 0))
    try:
        got = codec.sq_search_lists(c, sq, _device_codes(torch, codes, ld_c), torch.from_numpy(offsets).cuda(),
                                    torch.from_numpy(probes).cuda(), torch.from_numpy(q).cuda(), k,
                                    metric=metric, id_base=base,
                                    keep=None if keep is None else torch.from_numpy(keep).cuda())
        codec.ivf_status(c)
    finally:
        c.set_tuning(search_groups=0)
    _equal(got, sq_ref.search(q, codes, vmin, step, offsets, probes, k, metric, keep, base))


def test_bad_probes_and_offsets_are_reported_and_skipped(gpu):
    torch, codec, ctx, _ = gpu
    x, q = _normal(300, 8, 3, np.random.default_rng(2))
    vmin, step = sq_ref.train(x)
    codes = sq_ref.encode(x, vmin, step)
    offsets = np.array([0, 100, 90, 250, 400], np.int64)   # list 1 reversed, list 3 past n
    probes = np.array([[0, 1], [7, 2], [3, -5]], np.int64)
    sq = codec.SQ(ctx, torch.from_numpy(vmin).cuda(), torch.from_numpy(step).cuda())
    got = codec.sq_search_lists(ctx, sq, _device_codes(torch, codes, 8), torch.from_numpy(offsets).cuda(),
                                torch.from_numpy(probes).cuda(), torch.from_numpy(q).cuda(), 10)
    with pytest.raises(codec.PqhError):
        codec.ivf_status(ctx)
    _equal(got, sq_ref.search(q, codes, vmin, step, offsets, probes, 10))


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_ivfsq_probing_every_list_is_flat_over_the_decoded_rows(gpu, metric):
    torch, codec, ctx, _ = gpu
    n, d, nlist, nq, k = 3000, 16, 8, 12, 10
    x, q = _normal(n, d, nq, np.random.default_rng(9))
    xd, qd = torch.from_numpy(x).cuda(), torch.from_numpy(q).cuda()
    coarse = codec.Coarse(ctx, x[:nlist])
    index = codec.IVFSQ.build(ctx, coarse, xd, metric=metric)
    vmin, step = sq_ref.train(x)
    dec = sq_ref.decode(sq_ref.encode(x, vmin, step), vmin, step)
    ids = torch.tensor([5, -1, n - 1, 0, -1], device="cuda")
    want = np.where(ids.cpu().numpy()[:, None] < 0, np.float32(0), dec[ids.cpu().numpy()])
    assert np.array_equal(_bits(index.fetch(ids).cpu().numpy()), _bits(want))
    rows = index.fetch(torch.arange(n, device="cuda"))
    assert np.array_equal(_bits(rows.cpu().numpy()), _bits(dec))
    assert index.nbytes() == n * d + 8 * n + 8 * (nlist + 1) + 8 * d
    flat = codec.Flat(ctx, rows)
    dist, ids = index.search(qd, nlist, k)
    want = flat.search(qd, k, metric=metric)
    assert torch.equal(ids, want[1]) and torch.equal(dist.view(torch.int32), want[0].view(torch.int32))
    gone = ids[:, 0].unique()
    index.remove(ids[:, 0])
    assert index.live_count() == n - gone.numel()
    keep = torch.ones(n, dtype=torch.bool, device="cuda")
    keep[gone] = False
    for got in (index.search(qd, nlist, k), index.search(qd, nlist, k, keep=keep)):
        want = flat.search(qd, k, metric=metric, keep=keep)
        assert torch.equal(got[1], want[1]) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
    codec.ivf_status(ctx)
    flat.close()
    coarse.close()
