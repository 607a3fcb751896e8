"""Coarse.assign(method="screen") on the GPU: list ids and the raw bits of dist equal those of the
definition (tests/ivf_ref.py, tests/metric_ref.py), whatever the screen separates.  No tolerance
anywhere: the screen only chooses which lists the definition's chain is run for."""
import numpy as np
import pytest

import ivf_ref
import metric_ref

pytestmark = pytest.mark.gpu

# (n, d, nlist, ld_x): every edge of the tiling; d = 130 and 520 take the LDS-resident forms (two
# waves, one wave), d = 1030 is handed to the direct kernel
SHAPES = [(1, 1, 1, 1), (33, 5, 2, 7), (129, 16, 31, 16), (300, 17, 33, 20),
          (257, 128, 257, 128), (130, 130, 1030, 133), (200, 520, 3, 520), (5, 1030, 3, 1030)]
SCREEN_MAX_D = 1024


def _normal(n, d, nlist, rng, scale=1.0):
    return ((rng.standard_normal((n, d)) * scale).astype(np.float32),
            (rng.standard_normal((nlist, d)) * scale).astype(np.float32))


def _near_ties(n, d, nlist, rng):
    """every centroid twice (l and l + nlist / 2), a third copy of some one ulp off in one
    coordinate, and rows that are copies of centroids"""
    x, c = _normal(n, d, nlist, rng)
    half = nlist // 2
    c[half:2 * half] = c[:half]
    for l in range(0, half // 2, 3):
        c[l + 1] = c[l]
        c[l + 1, l % d] = np.nextafter(c[l, l % d], np.float32(np.inf))
    x[::4] = c[rng.integers(0, nlist, size=len(x[::4]))]
    return x, c


def _mixed_exact(n, d, nlist, rng):
    """two rows of three bf16-exact, inside every block of 32"""
    x, c = _normal(n, d, nlist, rng)
    bits = x.view(np.uint32)
    bits[np.arange(n) % 3 != 0] &= np.uint32(0xFFFF0000)
    return x, c


def _non_finite(n, d, nlist, rng):
    x, c = _normal(n, d, nlist, rng)
    for i, v in enumerate((np.nan, np.inf, -np.inf)):
        x[(7 * i + 3) % n, i % d] = v
    return x, c


WORLDS = {
    "normal": _normal,
    "grid": lambda n, d, nlist, rng: ivf_ref.integer_grid(n, d, nlist, int(rng.integers(1 << 30))),
    "near_ties": _near_ties,
    "offset": lambda n, d, nlist, rng: tuple(a + np.float32(1000) for a in _normal(n, d, nlist, rng)),
    "up": lambda n, d, nlist, rng: _normal(n, d, nlist, rng, 2.0 ** 40),
    "down": lambda n, d, nlist, rng: _normal(n, d, nlist, rng, 2.0 ** -40),
    "mixed_exact": _mixed_exact,
    "non_finite": _non_finite,
}


@pytest.fixture(scope="module")
def gpu():
    import torch
    from pq_huffman_amd import codec
    assert torch.cuda.is_available()
    return torch, codec, codec.Context(0)


def _check(gpu, metric, world, x, c, ld_x):
    """both outputs of the screen, with and without dist, against the definition; returns the
    counts of the call"""
    torch, codec, ctx = gpu
    n, d = x.shape
    buf = torch.full((n, ld_x), float("nan"), device="cuda")
    buf[:, :d] = torch.from_numpy(x)
    xd = buf[:, :d]
    coarse = codec.Coarse(ctx, c)
    if world == "non_finite":   # numpy's argmin and the kernel's `<` treat NaN differently
        dd = torch.empty(n, device="cuda")
        want_l = coarse.assign(xd, dist=dd, metric=metric).cpu().numpy()
        want_d = dd.cpu().numpy()
    else:
        with np.errstate(over="ignore", invalid="ignore"):
            want_l, want_d = (metric_ref if metric == "ip" else ivf_ref).assign(x, c)
    dist = torch.full((n,), -1.0, device="cuda")
    got = coarse.assign(xd, dist=dist, metric=metric, method="screen")
    counts = coarse.screen_counts()
    alone = coarse.assign(xd, metric=metric, method="screen")
    assert coarse.screen_counts() == counts
    assert np.array_equal(got.cpu().numpy(), want_l)
    assert np.array_equal(dist.cpu().numpy().view(np.uint32), want_d.view(np.uint32))
    assert np.array_equal(alone.cpu().numpy(), want_l)
    coarse.close()
    return counts


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("world", sorted(WORLDS))
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_screen_equals_the_definition(gpu, metric, world, shape):
    n, d, nlist, ld_x = shape
    rng = np.random.default_rng(1000 * n + d + len(world))
    x, c = WORLDS[world](n, d, nlist, rng)
    reranked, fallback = _check(gpu, metric, world, x, c, ld_x)
    if world == "normal":      # the screen separates: it is not the all-lists path in disguise
        assert fallback <= n // 100 and reranked < 0.1 * n, (reranked, fallback)
    # nothing is separated where tau (about 2^-10 * d * 10^6 at these d) is far above the spread
    # of the scores (about 10^3 * sqrt(2 d) for the inner product) and a row's two lanes cannot
    # hold the lists: d >= 128, hundreds of lists
    if world == "offset" and nlist > 256 and d <= SCREEN_MAX_D:
        assert fallback > 0, (reranked, fallback)


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_values_whose_scores_overflow(gpu, metric):
    """d = 4, values near 2^62: ||x||^2 is finite and a screening score is not"""
    rng = np.random.default_rng(62)
    x, c = _normal(100, 4, 40, rng)
    x, c = (np.float32(2.0 ** 62) * (1 + x / 16)).astype(np.float32), \
        (np.float32(2.0 ** 62) * (1 + c / 16)).astype(np.float32)
    assert _check(gpu, metric, "huge", x, c, 4)[1] == 100


def test_no_rows(gpu):
    torch, codec, ctx = gpu
    coarse = codec.Coarse(ctx, np.ones((3, 8), np.float32))
    out = coarse.assign(torch.empty((0, 8), device="cuda"), method="screen")
    assert out.shape == (0,) and out.dtype == torch.int32
    coarse.close()


def test_the_index_of_a_screened_build_and_add_is_the_index(gpu):
    torch, codec, ctx = gpu
    import datagen
    x = datagen.sift_like(2000, 128, seed=31)
    cc = datagen.lloyd_centroids(x, 1, 40, iters=2, sample=2000)[0]
    pq = codec.PQ(ctx, datagen.lloyd_centroids(x, 8, 256, iters=1, sample=2000))
    coarse = codec.Coarse(ctx, cc)
    xd = torch.from_numpy(x).cuda()
    built = []
    for method in ("direct", "screen"):
        ivf = codec.IVF.build(ctx, pq, coarse, xd[:1500], assign=method)
        assert ivf.assign_method == method and ivf.add(xd[1500:]) == 1500
        built.append(ivf)
    a, b = built
    assert torch.equal(a.perm, b.perm) and torch.equal(a.offsets, b.offsets)
    assert a.enc.nbytes == b.enc.nbytes
    assert torch.equal(a.enc.stream[:a.enc.nbytes], b.enc.stream[:b.enc.nbytes])
    assert torch.equal(a.enc.chunk_offsets, b.enc.chunk_offsets)
