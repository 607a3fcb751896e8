"""Flat, flat_search_lists and IVFFlat over float16 and bfloat16 rows on the GPU.  Every 16-bit
value is an fp32 value, so the expectation is the fp32 definition (tests/flat_ref.py,
tests/flat_lists_ref.py) over the converted rows: ids equal, dist equal bit for bit."""
import numpy as np
import pytest

import flat_lists_ref
import flat_ref

pytestmark = pytest.mark.gpu
DTYPES = ["float16", "bfloat16"]


def _exact(x, dtype):
    """x rounded so that every value is one of dtype (then torch's .to(dtype) is exact)"""
    if dtype == "float16":
        return x.astype(np.float16).astype(np.float32)
    return (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def _normal(n, d, nq, rng, dtype):
    return (_exact(rng.standard_normal((n, d)).astype(np.float32), dtype),
            rng.standard_normal((nq, d)).astype(np.float32))


def _near_ties(n, d, nq, rng, dtype):
    """duplicated rows, and queries that are copies of rows"""
    x, q = _normal(n, d, nq, rng, dtype)
    x[n // 2:2 * (n // 2)] = x[:n // 2]
    q[::4] = x[rng.integers(0, n, size=len(q[::4]))]
    return x, q


def _extremes(n, d, nq, rng, dtype):
    """the ends of fp16 scattered in: +-65504, the smallest subnormal, -0.0"""
    x, q = _normal(n, d, nq, rng, dtype)
    for i, v in enumerate((65504.0, -65504.0, 2.0 ** -24, -2.0 ** -24, -0.0)):
        x[rng.integers(0, n, 40), rng.integers(0, d, 40)] = v
    return _exact(x, dtype), q


WORLDS = {"normal": _normal, "near_ties": _near_ties, "extremes": _extremes}
# name: (list lengths, d, ld_x, nq, nprobe, k, options): the geometry of test_gpu_flat_lists.py
# (a tile is 256 rows, a unit 16 pairs, 4 when k > 64).  An even ld_x on a base of 4 bytes takes
# the 16-byte loads, anything else the element loads.
EDGE = [0, 1, 63, 64, 65, 257, 2300]
CASES = {
    "edges_odd_stride": (EDGE, 32, 35, 6, 3, 64, {}),
    "edges_one_group": (EDGE, 32, 32, 6, 3, 64, {"groups": 1}),
    "edges_three_groups": (EDGE, 32, 32, 6, 3, 64, {"groups": 3, "minus": True}),
    "pairs_17": ([300, 40], 3, 5, 17, 2, 1, {}),
    "wide_odd_d": ([700, 65, 0], 33, 40, 5, 3, 200, {}),
    "d1": ([257, 64], 1, 2, 3, 2, 64, {}),
    "d130": ([65, 300, 1], 130, 132, 4, 2, 10, {"id_base": 2 ** 40 - 5}),
    "tile_masked": ([1200, 300], 32, 32, 7, 2, 64, {"keep": "tile"}),
    "none_kept": ([1200, 300], 32, 32, 7, 2, 64, {"keep": "none"}),
    "base_off_4_bytes": ([300, 40], 32, 32, 5, 2, 64, {"shift": 1}),
    "near_ties": ([500, 700, 65], 8, 8, 20, 2, 10, {"world": "near_ties"}),
    "extremes": ([300, 40], 32, 32, 5, 2, 64, {"world": "extremes"}),
}
KEEPS = {"tile": lambda n, rng: (rng.random(n) < 0.5) & (np.arange(n) // 256 != 2),
         "none": lambda n, rng: np.zeros(n, bool)}


@pytest.fixture(scope="module")
def gpu():
    import torch
    from pq_huffman_amd import codec
    assert torch.cuda.is_available()
    return torch, codec, codec.Context(0), codec.Context(0).set_search_max_k(256)


def _rows(torch, x, ld_x, dtype, shift=0):
    """x as a device tensor of dtype, rows ld_x elements apart from element `shift` of its
    buffer on, NaN everywhere else"""
    n, d = x.shape
    flat = torch.full((n * ld_x + shift,), float("nan"), dtype=getattr(torch, dtype), device="cuda")
    buf = flat[shift:].view(n, ld_x)
    buf[:, :d] = torch.from_numpy(x).to(buf.dtype)
    assert np.array_equal(buf[:, :d].float().cpu().numpy().view(np.uint32), x.view(np.uint32))
    return buf


def _equal(got, want):
    got = [t.cpu().numpy() if hasattr(t, "cpu") else t for t in got[:2]]
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_list_scan(gpu, dtype, metric, case):
    torch, codec, ctx, wide = gpu
    lengths, d, ld_x, nq, nprobe, k, opt = CASES[case]
    rng = np.random.default_rng(len(case) + d)
    offsets = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    n, nlist = int(offsets[-1]), len(lengths)
    x, q = WORLDS[opt.get("world", "normal")](n, d, nq, rng, dtype)
    probes = np.full((nq, nprobe), -1, np.int64)   # the longest list, then distinct others
    longest = int(np.argmax(lengths))
    for i in range(nq):
        row = [longest] + list(rng.permutation([l for l in range(nlist) if l != longest]))
        probes[i, :min(nprobe, nlist)] = row[:nprobe]
    if opt.get("minus"):
        probes[::2, -1] = -1
    keep = KEEPS[opt["keep"]](n, rng) if "keep" in opt else None
    base = opt.get("id_base", 0)
    c = wide if k > 64 else ctx
    c.set_tuning(search_groups=opt.get("groups", 0))
    try:
        got = codec.flat_search_lists(c, _rows(torch, x, ld_x, dtype, opt.get("shift", 0)),
                                      torch.from_numpy(offsets).cuda(), torch.from_numpy(probes).cuda(),
                                      torch.from_numpy(q).cuda(), k, metric=metric, id_base=base, d=d,
                                      keep=None if keep is None else torch.from_numpy(keep).cuda())
        codec.ivf_status(c)
    finally:
        c.set_tuning(search_groups=0)
    _equal(got, flat_lists_ref.search(q, x, offsets, probes, k, metric, keep, base))


def _flat(gpu, x, q, k, metric, dtype, ld_x=None, **kw):
    torch, codec, ctx, wide = gpu
    flat = codec.Flat(wide if k > 64 else ctx, _rows(torch, x, ld_x or x.shape[1], dtype), d=x.shape[1])
    dist, ids = flat.search(torch.from_numpy(q).cuda(), k, metric=metric, **kw)
    counts = flat.counts()
    flat.close()
    return dist.cpu().numpy(), ids.cpu().numpy(), counts


# (n, d, nq, k, ld_x): a partial tile, d off 16 with more than four waves of queries, aligned
# drains over three slabs, the wide list, panels with a short last one, and d > 1,024 (no screen)
SHAPES = [(1, 1, 1, 1, 1), (33, 16, 1, 7, 16), (300, 17, 129, 10, 20), (2500, 128, 70, 64, 128),
          (5000, 32, 40, 200, 32), (700, 136, 33, 10, 136), (40, 1032, 3, 5, 1032)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_flat_shapes(gpu, dtype, metric, shape):
    n, d, nq, k, ld_x = shape
    x, q = _normal(n, d, nq, np.random.default_rng(1000 * n + d), dtype)
    got = _flat(gpu, x, q, k, metric, dtype, ld_x)
    _equal(got, flat_ref.search(q, x, k, metric))
    assert got[2][1] == (nq if d > 1024 else 0)   # only d > 1,024 is not screened


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_flat_mask_and_a_non_finite_row(gpu, dtype, metric):
    torch = gpu[0]
    n, d, nq, k = 2500, 48, 70, 10
    rng = np.random.default_rng(3)
    x, q = _normal(n, d, nq, rng, dtype)
    keep = (rng.random(n) < 0.5) & ((np.arange(n) // 32) != 33)   # an empty tile of 32
    base = 2 ** 40 - 5
    got = _flat(gpu, x, q, k, metric, dtype, keep=torch.from_numpy(keep).cuda(), id_base=base)
    _equal(got, flat_ref.search(q, x, k, metric, keep=keep, id_base=base))
    x[40, 1] = np.inf   # through Cmax to the all-rows path: still the definition
    got = _flat(gpu, x, q, k, metric, dtype, id_base=5)
    _equal(got, flat_ref.search(q, x, k, metric, id_base=5))
    assert got[2][1] > 0 and ((got[1] >= -1) & (got[1] < 5 + n)).all()


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_screen_still_separates(gpu, dtype, metric):
    n, d, nq, k = 16384, 64, 64, 10   # test_gpu_flat.py's shape and cap
    x, q = _normal(n, d, nq, np.random.default_rng(5), dtype)
    got = _flat(gpu, x, q, k, metric, dtype)
    _equal(got, flat_ref.search(q, x, k, metric))
    chains, fallback = got[2]
    print(dtype, metric, "chains", chains, "share", chains / (nq * n), "fallback", fallback)
    assert fallback == 0 and chains < 0.25 * nq * n, got[2]


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_ivfflat_stores_16_bit_rows(gpu, dtype, metric):
    torch, codec, ctx, _ = gpu
    n, d, nlist, nq, k = 3000, 16, 8, 12, 10
    rng = np.random.default_rng(9)
    x, q = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((nq, d)).astype(np.float32)
    xd, qd, t = torch.from_numpy(x).cuda(), torch.from_numpy(q).cuda(), getattr(torch, dtype)
    coarse = codec.Coarse(ctx, x[:nlist])
    index = codec.IVFFlat.build(ctx, coarse, xd, metric=metric, store={"float16": "f16", "bfloat16": "bf16"}[dtype])
    assert index.x_sorted.dtype == t and index.nbytes() == n * (2 * d + 8)
    flat = codec.Flat(ctx, xd.to(t))
    want = flat.search(qd, k, metric=metric)
    _equal(index.search(qd, nlist, k), [w.cpu().numpy() for w in want])
    # a 16-bit x gives the same index when it has the same lists: rows that round to themselves
    same = codec.IVFFlat.build(ctx, coarse, xd.to(t), metric=metric)
    again = codec.IVFFlat.build(ctx, coarse, xd.to(t).float(), metric=metric, store=None)
    assert same.x_sorted.dtype == t and torch.equal(same.perm, again.perm)
    assert torch.equal(same.x_sorted.float(), again.x_sorted)
    _equal(same.search(qd, nlist, k), [w.cpu().numpy() for w in want])
    gone = want[1][:, 0].unique()
    index.remove(want[1][:, 0])
    assert index.live_count() == n - gone.numel()
    keep = torch.ones(n, dtype=torch.bool, device="cuda")
    keep[gone] = False
    want = [w.cpu().numpy() for w in flat.search(qd, k, metric=metric, keep=keep)]
    for got in (index.search(qd, nlist, k), index.search(qd, nlist, k, keep=keep)):
        _equal(got, want)
    flat.close()
    coarse.close()
