"""codec.Flat on the GPU: ids and the raw bits of dist equal those of the definition
(tests/flat_ref.py), whatever the screen separates.  No tolerance anywhere: the screen only
chooses which (query, row) pairs the definition's chain is run for."""
import numpy as np
import pytest

import flat_ref
import ivf_ref

pytestmark = pytest.mark.gpu

# (n, d, nq, k, ld_x).  The launch plan cuts the rows into slabs of 1,024 at these sizes (one
# query group: a slab per compute unit, never below 1,024 rows), so (2500, ...) has three slabs
# and (5000, ...) five, and their top-k cross the slab boundaries; every other shape is one slab.
# d = 130 and 520 take the panel form of the screen (two and five panels, the last one short),
# d = 1030 the chain for every pair.
SHAPES = [(1, 1, 1, 1, 1), (31, 5, 33, 64, 7), (33, 16, 1, 7, 16), (300, 17, 129, 10, 20),
          (2500, 128, 70, 64, 128), (5000, 32, 40, 200, 32), (700, 130, 33, 10, 133),
          (260, 520, 5, 10, 520), (40, 1030, 3, 5, 1030)]
MID = (2500, 48, 70, 10)   # three slabs, three waves of queries, d not a multiple of 16


def _normal(n, d, nq, rng, scale=1.0):
    return ((rng.standard_normal((n, d)) * scale).astype(np.float32),
            (rng.standard_normal((nq, d)) * scale).astype(np.float32))


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


def _mixed_exact(n, d, nq, rng):
    """two rows and two queries of three bf16-exact, inside every tile of 32"""
    x, q = _normal(n, d, nq, rng)
    x.view(np.uint32)[np.arange(n) % 3 != 0] &= np.uint32(0xFFFF0000)
    q.view(np.uint32)[np.arange(nq) % 3 != 0] &= np.uint32(0xFFFF0000)
    return x, q


WORLDS = {
    "normal": _normal,
    "grid": lambda n, d, nq, rng: ivf_ref.integer_grid(n, d, nq, int(rng.integers(1 << 30))),
    "near_ties": _near_ties,
    "offset": lambda n, d, nq, rng: tuple(a + np.float32(1000) for a in _normal(n, d, nq, rng)),
    "up": lambda n, d, nq, rng: _normal(n, d, nq, rng, 2.0 ** 40),
    "down": lambda n, d, nq, rng: _normal(n, d, nq, rng, 2.0 ** -40),
    "mixed_exact": _mixed_exact,
}


@pytest.fixture(scope="module")
def gpu():
    import torch
    from pq_huffman_amd import codec
    assert torch.cuda.is_available()
    return torch, codec, codec.Context(0), codec.Context(0).set_search_max_k(256)


def _search(gpu, x, q, k, metric, ld_x=None, **kw):
    """Flat.search of rows ld_x floats apart, NaN between them -> numpy (dist, ids), counts"""
    torch, codec, ctx, wide = gpu
    n, d = x.shape
    buf = torch.full((n, ld_x or d), float("nan"), device="cuda")
    buf[:, :d] = torch.from_numpy(x)
    flat = codec.Flat(wide if k > 64 else ctx, buf, d=d)
    dist, ids = flat.search(torch.from_numpy(q).cuda(), k, metric=metric, **kw)
    counts = flat.counts()
    flat.close()
    return dist.cpu().numpy(), ids.cpu().numpy(), counts


def _equal(got, want):
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_shapes(gpu, metric, shape):
    n, d, nq, k, ld_x = shape
    x, q = _normal(n, d, nq, np.random.default_rng(1000 * n + d))
    got = _search(gpu, x, q, k, metric, ld_x)
    _equal(got, flat_ref.search(q, x, k, metric))
    assert got[2][1] == (nq if d > 1024 else 0)   # only d > 1,024 is not screened


@pytest.mark.parametrize("world", sorted(WORLDS))
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_worlds(gpu, metric, world):
    n, d, nq, k = MID
    x, q = WORLDS[world](n, d, nq, np.random.default_rng(len(world)))
    _equal(_search(gpu, x, q, k, metric), flat_ref.search(q, x, k, metric))


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_non_finite(gpu, metric):
    n, d, nq, k = MID
    x, q = _normal(n, d, nq, np.random.default_rng(7))
    bad = q.copy()
    for i, v in enumerate((np.nan, np.inf, -np.inf)):
        bad[(7 * i + 3) % nq, i % d] = v
    finite = np.isfinite(bad).all(axis=1)
    got = _search(gpu, x, bad, k, metric, id_base=5)
    want = flat_ref.search(q, x, k, metric, id_base=5)
    assert got[2][1] == 3   # the three queries took the all-rows path
    _equal((got[0][finite], got[1][finite]), (want[0][finite], want[1][finite]))
    for i, v in enumerate((np.nan, np.inf, -np.inf)):
        x[(11 * i + 40) % n, i % d] = v
    for ids in (got[1], _search(gpu, x, bad, k, metric, id_base=5)[1]):
        assert ((ids >= -1) & (ids < 5 + n)).all()


KEEPS = {"tenth": lambda n, rng: rng.random(n) < 0.1,
         "empty_tile": lambda n, rng: (rng.random(n) < 0.5) & ((np.arange(n) // 32) != 33),
         "none": lambda n, rng: np.zeros(n, bool)}


@pytest.mark.parametrize("mask", sorted(KEEPS))
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_keep_and_id_base(gpu, metric, mask):
    torch = gpu[0]
    n, d, nq, k = MID
    rng = np.random.default_rng(3)
    x, q = _normal(n, d, nq, rng)
    keep = KEEPS[mask](n, rng)
    base = 2 ** 40 - 5
    got = _search(gpu, x, q, 64, metric, keep=torch.from_numpy(keep).cuda(), id_base=base)
    _equal(got, flat_ref.search(q, x, 64, metric, keep=keep, id_base=base))


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_equals_the_probe(gpu, metric):
    torch, codec, ctx, _ = gpu
    x, q = _near_ties(1500, 24, 40, np.random.default_rng(11))
    coarse = codec.Coarse(ctx, x)
    _, _, probes, pdist = coarse.probe(torch.from_numpy(q).cuda(), 64,
                                       torch.arange(1501, device="cuda"), metric=metric)
    _equal(_search(gpu, x, q, 64, metric), (pdist.cpu().numpy(), probes.cpu().numpy()))
    coarse.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_the_screen_separates(gpu, metric):
    n, d, nq, k = 16384, 64, 64, 10
    x, q = _normal(n, d, nq, np.random.default_rng(5))
    got = _search(gpu, x, q, k, metric)
    _equal(got, flat_ref.search(q, x, k, metric))
    chains, fallback = got[2]
    assert fallback == 0 and chains < 0.25 * nq * n, got[2]


def test_no_rows_and_no_queries(gpu):
    empty = np.zeros((0, 8), np.float32)
    dist, ids, _ = _search(gpu, empty, np.ones((3, 8), np.float32), 4, "l2")
    assert np.isinf(dist).all() and (ids == -1).all()
    assert _search(gpu, np.ones((5, 8), np.float32), empty, 4, "ip")[0].shape == (0, 4)
