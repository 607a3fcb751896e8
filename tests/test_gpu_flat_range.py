"""codec.Flat.range_search on the GPU: lims, ids and the raw bits of dist equal those of the
definition (ivf_ref.dists / metric_ref.nip, the fp32 chains, compared with the radius by a strict
<), whatever the screen separates.  No tolerance anywhere.

The plan cuts the rows into slabs of 1,024 at these sizes (one or two query groups on 256 compute
units, never below 1,024 rows): (2500, ...) has three slabs with hits across the cuts, every other
shape of SHAPES one.  d = 130 and 520 take the panel form (two and five panels, the last one
short), d = 1030 the chain for every pair.  EPOCHS runs with search_groups = 1: one slab of 5,024
rows, 157 tiles, two epochs of 64 tiles and one of 29."""
import ctypes

import numpy as np
import pytest

import ivf_ref
import metric_ref
from test_gpu_flat import WORLDS, _normal

pytestmark = pytest.mark.gpu

# (n, d, nq, ld_x)
SHAPES = [(1, 1, 1, 1), (31, 5, 33, 7), (33, 16, 1, 16), (300, 17, 129, 20), (2500, 128, 70, 128),
          (700, 130, 33, 133), (260, 520, 5, 520), (40, 1030, 3, 1030)]
MID = (2500, 48, 70)   # three slabs, three waves of queries, d not a multiple of 16
EPOCHS = (5000, 8, 40)
SPECIAL = [0.0, -1.0, np.inf, np.nan, 2.0 ** 60]


@pytest.fixture(scope="module")
def gpu():
    import torch
    from pq_huffman_amd import codec
    assert torch.cuda.is_available()
    return torch, codec, codec.Context(0)


def _dists(q, x, metric):
    with np.errstate(over="ignore", invalid="ignore"):
        return metric_ref.nip(q, x) if metric == "ip" else ivf_ref.dists(q, x)


def _kth(dist, ks):
    """query i's ks[i % len(ks)]-th smallest distance: the strict < sits on a value that occurs"""
    n = dist.shape[1]
    srt = np.sort(dist, axis=1)
    return np.array([srt[i, min(max(ks[i % len(ks)], 1), n) - 1] for i in range(len(dist))],
                    np.float32)


def _radii(dist):
    """the k-th distances, k cycling through {1, 2, 33, n // 2, n}, and from query 5 on every
    second run of five the special radii"""
    n = dist.shape[1]
    r = _kth(dist, [1, 2, 33, n // 2, n])
    for i in range(5, len(r)):
        if i % 10 >= 5:
            r[i] = SPECIAL[i % 5]
    return r


def _want(dist, radius, keep=None, id_base=0):
    with np.errstate(invalid="ignore"):
        hit = dist < radius[:, None]
    if keep is not None:
        hit &= keep[None, :]
    qs, rows = np.nonzero(hit)   # (ascending query, then ascending row)
    lims = np.concatenate([[0], np.cumsum(hit.sum(axis=1))]).astype(np.int64)
    return lims, dist[qs, rows], rows.astype(np.int64) + id_base


def _search(gpu, x, q, radius, metric, ld_x=None, ctx=None, **kw):
    """Flat.range_search of rows ld_x apart, NaN between them -> numpy (lims, dist, ids), counts"""
    torch, codec, ctx0 = gpu
    x = x if torch.is_tensor(x) else torch.from_numpy(x)
    n, d = x.shape
    buf = torch.full((n, ld_x or d), float("nan"), device="cuda", dtype=x.dtype)
    buf[:, :d] = x
    flat = codec.Flat(ctx or ctx0, buf, d=d)
    radius = torch.from_numpy(radius).cuda() if isinstance(radius, np.ndarray) else radius
    got = flat.range_search(torch.from_numpy(q).cuda(), radius, metric=metric, **kw)
    counts = flat.counts()
    flat.close()
    return tuple(t.cpu().numpy() for t in got), counts


def _equal(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[2], want[2])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_shapes(gpu, metric, shape):
    n, d, nq, ld_x = shape
    x, q = _normal(n, d, nq, np.random.default_rng(1000 * n + d))
    dist = _dists(q, x, metric)
    radius = _radii(dist)
    got, counts = _search(gpu, x, q, radius, metric, ld_x)
    _equal(got, _want(dist, radius))
    assert counts[1] == (nq if d > 1024 else 0)   # only d > 1,024 is not screened


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_epochs(gpu, metric):
    n, d, nq = EPOCHS
    x, q = _normal(n, d, nq, np.random.default_rng(17))
    dist = _dists(q, x, metric)
    radius = _kth(dist, [n // 2, n // 7, 3])
    radius[0] = np.inf   # every row
    want = _want(dist, radius)
    for row in (2047, 2048, 4095, 4096):   # both sides of both epoch boundaries
        assert (want[2] == row).sum() > 1
    ctx = gpu[1].Context(0).set_tuning(search_groups=1)
    _equal(_search(gpu, x, q, radius, metric, ctx=ctx)[0], want)


@pytest.mark.parametrize("world", ["near_ties", "up", "down", "mixed_exact"])
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_worlds(gpu, metric, world):
    n, d, nq = MID
    x, q = WORLDS[world](n, d, nq, np.random.default_rng(len(world)))
    dist = _dists(q, x, metric)
    radius = _kth(dist, [33])
    if world == "near_ties":   # rows 3i and 3i + n / 2 share the value, row 3i + 1 is an ulp off
        radius = dist[np.arange(nq), 3 * np.arange(nq)].copy()
    _equal(_search(gpu, x, q, radius, metric)[0], _want(dist, radius))


@pytest.mark.parametrize("shape", [(300, 17, 40), (1100, 32, 40)], ids=["odd", "vec"])
@pytest.mark.parametrize("rows", ["float16", "bfloat16"])
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_row_types(gpu, metric, rows, shape):
    torch = gpu[0]
    x, q = _normal(*shape, np.random.default_rng(23))
    x16 = torch.from_numpy(x).to(getattr(torch, rows))
    dist = _dists(q, x16.float().numpy(), metric)
    radius = _kth(dist, [1, 33, shape[0] // 2])
    got = _search(gpu, x16, q, radius, metric)[0]
    _equal(got, _search(gpu, x16.float(), q, radius, metric)[0])
    _equal(got, _want(dist, radius))


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_keep_and_id_base(gpu, metric):
    torch = gpu[0]
    n, d, nq = MID
    rng = np.random.default_rng(3)
    x, q = _normal(n, d, nq, rng)
    keep = rng.random(n) < 0.5
    keep[32 * 5:32 * 9] = False    # whole tiles empty
    keep[1000:1015] = False        # and one that cuts a tile
    dist = _dists(q, x, metric)
    radius = _kth(dist, [33, n // 2, n])
    got = _search(gpu, x, q, radius, metric, keep=torch.from_numpy(keep).cuda(), id_base=2 ** 40)[0]
    assert keep[got[2] - 2 ** 40].all()
    _equal(got, _want(dist, radius, keep, 2 ** 40))


def test_capacity(gpu):
    torch, codec, _ = gpu
    n, d, nq = MID
    x, q = _normal(n, d, nq, np.random.default_rng(29))
    dist = _dists(q, x, "l2")
    radius = _kth(dist, [33, 2])
    want = _want(dist, radius)
    total, cut = int(want[0][-1]), int(want[0][-1]) // 2
    # the Python call: the first `cut` entries, lims full
    got = _search(gpu, x, q, radius, "l2", capacity=cut)[0]
    _equal(got, (want[0], want[1][:cut], want[2][:cut]))
    got = _search(gpu, x, q, radius, "l2", capacity=total + 3)[0]
    assert np.isinf(got[1][total:]).all() and (got[2][total:] == -1).all()
    # the two calls themselves, over a buffer longer than the capacity
    ctx = codec.Context(0)
    xd, qd, rd = (torch.from_numpy(a).cuda() for a in (x, q, radius))
    flat = codec.Flat(ctx, xd)
    nbytes = ctypes.c_ulonglong(0)
    codec.check(codec.lib().pqh_flat_range_plan_bytes(ctx.ptr, flat.ptr, nq, ctypes.byref(nbytes)))
    plan = torch.zeros(nbytes.value // 8, dtype=torch.int64, device="cuda")
    lims = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
    args = (ctx.ptr, flat.ptr, codec._ptr(qd), nq, d, codec._ptr(rd), None, codec._ptr(plan),
            nbytes.value, codec._ptr(lims))
    codec.check(codec.lib().pqh_flat_range_count(*args))

    def fill():
        out = (torch.full((total,), -7.0, device="cuda"),
               torch.full((total,), -7, dtype=torch.int64, device="cuda"))
        codec.check(codec.lib().pqh_flat_range_fill(*args, cut, 0, codec._ptr(out[0]), codec._ptr(out[1])))
        return lims.cpu().numpy(), out[0].cpu().numpy(), out[1].cpu().numpy()

    first, again = fill(), fill()
    _equal(first, again)
    _equal((first[0], first[1][:cut], first[2][:cut]), (want[0], want[1][:cut], want[2][:cut]))
    assert (first[1][cut:] == -7.0).all() and (first[2][cut:] == -7).all()
    # another geometry (one slab in the place of three): nothing is written, and it is reported
    ctx.set_tuning(search_groups=1)
    other = fill()
    assert (other[1] == -7.0).all() and (other[2] == -7).all()
    with pytest.raises(codec.PqhError):
        codec.decode_status(ctx)
    flat.close()


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_non_finite(gpu, metric):
    n, d, nq = MID
    x, q = _normal(n, d, nq, np.random.default_rng(7))
    radius = _kth(_dists(q, x, metric), [33])
    bad = q.copy()
    for i, v in enumerate((np.nan, np.inf, -np.inf)):
        bad[(7 * i + 3) % nq, i % d] = v
    finite = np.flatnonzero(np.isfinite(bad).all(axis=1))
    got, counts = _search(gpu, x, bad, radius, metric)
    assert counts[1] == 3   # the three queries took the all-rows path
    want = _want(_dists(bad, x, metric), radius)
    assert got[0][4] == got[0][3]   # the NaN query: every distance is NaN, no hit
    for i in finite:
        a, b = (slice(t[0][i], t[0][i + 1]) for t in (got, want))
        _equal((a.stop - a.start, got[1][a], got[2][a]), (b.stop - b.start, want[1][b], want[2][b]))
    x[1234, 5] = np.nan   # a NaN row: every query by the chain, that row no hit
    got, counts = _search(gpu, x, q, radius, metric)
    assert counts[1] == nq
    _equal(got, _want(_dists(q, x, metric), radius))


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_the_screen_separates(gpu, metric):
    n, d, nq = 16384, 64, 64
    x, q = _normal(n, d, nq, np.random.default_rng(5))
    dist = _dists(q, x, metric)
    radius = _kth(dist, [10])
    # the candidate rule of DESIGN.md 4.5.22 in numpy: S <= T with exact scores
    x64, q64 = x.astype(np.float64), q.astype(np.float64)
    X = (q * q).sum(axis=1, dtype=np.float32)
    cmax = np.float32((x64 * x64).sum(axis=1).max())
    tau = np.float32((115.0 + 14.6 * d) * 2.0 ** -22 * (1 + 2.0 ** -9)) * (X + cmax)
    if metric == "ip":
        S, T = -(q64 @ x64.T), radius + tau
    else:
        S, T = (x64 * x64).sum(axis=1)[None, :] - 2.0 * (q64 @ x64.T), (radius - X) + tau
    share = (S <= T[:, None]).mean()
    got, (chains, fallback) = _search(gpu, x, q, radius, metric)
    _equal(got, _want(dist, radius))
    print(f"simulated share {share:.6f}, chains {chains} of {nq * n}")
    assert fallback == 0 and chains < 2 * share * nq * n


def test_no_rows_and_no_queries(gpu):
    empty = np.zeros((0, 8), np.float32)
    (lims, dist, ids), _ = _search(gpu, empty, np.ones((3, 8), np.float32), 1.0, "l2")
    assert (lims == 0).all() and lims.shape == (4,) and dist.shape == ids.shape == (0,)
    (lims, dist, ids), _ = _search(gpu, np.ones((5, 8), np.float32), empty, 1.0, "ip")
    assert lims.tolist() == [0] and dist.shape == ids.shape == (0,)
