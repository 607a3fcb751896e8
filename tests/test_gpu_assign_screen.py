"""PQ assignment mode 2 (the LDS-resident MFMA screen, pqh_assign_screen.hip) on the GPU: the
codes equal the definition's (oracle.pq_assign) bit for bit, whatever the screen separates.  No
tolerance anywhere: the screen only chooses which codes the definition's chain is run for."""
import numpy as np
import pytest

import test_gpu_coarse_screen as cs

pytestmark = pytest.mark.gpu

# (n, m, K, dsub, ld_x) and the form the LDS budget rule gives it (image = 64 P bytes and a norm
# per padded code; resident where image + 2 waves' 16 KB of lists fit 160 KB).  u8 codes mean
# K <= 256 and so an image of at most 132 KB: only u16 shapes can be streamed.
SHAPES = [
    (1, 1, 1, 1, 1),             # resident, u8: the smallest case
    (33, 3, 16, 4, 13),          # resident, u8: one half-empty tile, unaligned rows, 4-bit
    (129, 2, 33, 5, 10),         # resident, u8: K crosses a tile, a padded pass
    (300, 2, 256, 48, 96),       # resident, u8: P = 3, 49 KB
    (257, 16, 256, 8, 128),      # resident, u8: a shape mode 0 also serves
    (130, 2, 1024, 16, 32),      # resident, u16: 68 KB
    (200, 1, 300, 128, 131),     # streamed, u16: the register limit, 161 KB
    (70, 1, 4100, 8, 8),         # streamed, u16: K neither 4096 nor a multiple of 32, 274 KB
    (5, 2, 4, 130, 260),         # the exact kernel, counts (0, 0)
]
WORLDS = {w: cs.WORLDS[w] for w in ("normal", "near_ties", "offset", "up", "down", "mixed_exact",
                                    "non_finite")}
LAYOUTS = ("rows", "parts")
_ids = dict(ids=lambda s: "x".join(map(str, s)))


@pytest.fixture(scope="module")
def gpu():
    import torch
    from pq_huffman_amd import codec
    assert torch.cuda.is_available()
    return torch, codec, codec.Context(0)


def _world(world, n, m, k, dsub, rng):
    """the world's generator per subspace: x (n, m * dsub), centroids (m, k, dsub)"""
    parts = [WORLDS[world](n, dsub, k, rng) for _ in range(m)]
    return np.hstack([p[0] for p in parts]), np.stack([p[1] for p in parts])


def _poisoned(torch, x, ld_x):
    buf = torch.full((x.shape[0], ld_x), float("nan"), device="cuda")
    buf[:, :x.shape[1]] = torch.from_numpy(x)
    return buf[:, :x.shape[1]]


def _run(pq, xd, layout, mode, counts=None):
    out = pq.assign(xd, counts=counts, mode=mode) if layout == "rows" else \
        pq.assign_parts(xd, counts=counts, mode=mode).t().contiguous()
    out = out.cpu().numpy()
    return out.view(np.uint16) if out.dtype == np.int16 else out


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("world", sorted(WORLDS))
@pytest.mark.parametrize("shape", SHAPES, **_ids)
def test_codes_equal_the_definition(gpu, oracle, shape, world, layout):
    torch, codec, ctx = gpu
    n, m, k, dsub, ld_x = shape
    x, cent = _world(world, n, m, k, dsub, np.random.default_rng(1000 * n + dsub))
    xd = _poisoned(torch, x, ld_x)
    pq = codec.PQ(ctx, cent)
    got = _run(pq, xd, layout, 2)
    reranked, fallback = pq.screen_counts()
    assert pq.rerank_count() == reranked + fallback
    if world == "non_finite":   # numpy's argmin and the kernel's `<` treat NaN differently
        want = _run(pq, xd, layout, 1)
    else:
        want = oracle.pq_assign(np.ascontiguousarray(x), cent, threads=0)[0]
    pq.close()
    assert got.dtype == want.dtype and np.array_equal(got, want)
    if dsub > 128:
        assert (reranked, fallback) == (0, 0)
    elif world == "normal":    # the screen separates: it is not the all-codes chain in disguise
        assert fallback <= n * m / 100 and reranked < 0.1 * n * m, (reranked, fallback)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_values_whose_scores_overflow(gpu, layout):
    """dsub = 4, values near 2^62: ||x||^2 is finite and a screening score is not"""
    torch, codec, ctx = gpu
    x, c = _world("normal", 100, 2, 40, 4, np.random.default_rng(62))
    x, c = (np.float32(2.0 ** 62) * (1 + x / 16)).astype(np.float32), \
        (np.float32(2.0 ** 62) * (1 + c / 16)).astype(np.float32)
    xd = _poisoned(torch, x, 9)
    pq = codec.PQ(ctx, c)
    got = _run(pq, xd, layout, 2)
    assert pq.screen_counts() == (0, 200)
    assert np.array_equal(got, _run(pq, xd, layout, 1))
    pq.close()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", [(300, 2, 256, 48), (130, 2, 1024, 16)], **_ids)
def test_fused_histogram(gpu, shape, layout):
    torch, codec, ctx = gpu
    n, m, k, dsub = shape
    x, cent = _world("normal", n, m, k, dsub, np.random.default_rng(n))
    pq = codec.PQ(ctx, cent, assign_mode=2)
    counts = torch.zeros((m, k), dtype=torch.int32, device="cuda")
    got = _run(pq, torch.from_numpy(x).cuda(), layout, None, counts)
    pq.close()
    want = np.stack([np.bincount(got[:, i], minlength=k) for i in range(m)])
    assert np.array_equal(counts.cpu().numpy(), want)


@pytest.mark.parametrize("shape", [(2000, 1, 40, 128), (2000, 4, 16, 8)], **_ids)
def test_kmeans_through_the_screen_is_kmeans(gpu, shape):
    torch, codec, ctx = gpu
    n, m, k, dsub = shape
    x, init = _world("normal", n, m, k, dsub, np.random.default_rng(k))
    xd = torch.from_numpy(x).cuda()
    a, b = (codec.kmeans_train(ctx, xd, init, 3, mode=mode) for mode in (0, 2))
    assert a.tobytes() == b.tobytes() and a.tobytes() != init.tobytes()


def test_the_index_of_a_screened_pq_is_the_index(gpu):
    torch, codec, ctx = gpu
    import datagen
    x = datagen.sift_like(2000, 128, seed=31)
    cc = datagen.lloyd_centroids(x, 1, 40, iters=2, sample=2000)[0]
    cent = datagen.lloyd_centroids(x, 8, 16, iters=1, sample=2000)
    coarse = codec.Coarse(ctx, cc)
    xd = torch.from_numpy(x).cuda()
    a, b = (codec.IVF.build(ctx, codec.PQ(ctx, cent, assign_mode=mode), coarse, xd, context=False)
            for mode in (0, 2))   # (context coding is for K = 256)
    assert b.pq.screen_counts()[0] + b.pq.screen_counts()[1] < 2000 * 8
    assert torch.equal(a.perm, b.perm) and a.enc.nbytes == b.enc.nbytes
    assert torch.equal(a.enc.stream[:a.enc.nbytes], b.enc.stream[:b.enc.nbytes])
    assert torch.equal(a.enc.chunk_offsets, b.enc.chunk_offsets)
    none = b.pq.assign(xd[:0])
    assert none.shape == (0, 8) and none.dtype == torch.uint8
