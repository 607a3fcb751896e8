"""The assignment kernel's deferred re-rank (batches of 32 queued vectors, the hand-over of a
wave's leftover entries to its partner wave, skipped candidate slots): codes from pq.assign
and pq.assign_parts against the CPU oracle at shapes that sit on batch boundaries.  A 64-row
chunk belongs to one wave, so with every row tying the row count sets that wave's queue."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    from pq_huffman_amd import codec
    assert torch.cuda.is_available()
    ctx = codec.Context(0)
    return torch, codec, ctx


def _codes(gpu, x, cent, layout="rows", counts=None):
    """(codes (n, m) as numpy, re-rank count) through either code layout"""
    torch, codec, ctx = gpu
    pq = codec.PQ(ctx, cent)
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    if layout == "rows":
        out = pq.assign(xd, counts=counts).cpu().numpy()
    else:   # part-major, ld padded to 128 codes
        out = pq.assign_parts(xd, counts=counts).t().contiguous().cpu().numpy()
    if out.dtype == np.int16:   # (torch keeps u16 codes as int16)
        out = out.view(np.uint16)
    return out, pq.rerank_count()


def _dup_centroids(rng, m, k, dsub, hi):
    """integer centroids, the upper half a copy of the lower: every row ties"""
    cent = rng.integers(0, hi, (m, k, dsub)).astype(np.float32)
    cent[:, k // 2:] = cent[:, :k // 2]
    return cent


ALL_TIE_N = (1, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 256 + 17)


@pytest.fixture(scope="module")
def all_tie(oracle):
    rng = np.random.default_rng(71)
    x = rng.integers(0, 50, (max(ALL_TIE_N), 32)).astype(np.float32)
    cent = _dup_centroids(rng, 2, 256, 16, 50)
    want, _ = oracle.pq_assign(x, cent, threads=0)   # (row by row: a prefix's codes are a prefix)
    assert (want < 128).all()
    return x, cent, want


@pytest.mark.parametrize("layout", ["rows", "parts"])
@pytest.mark.parametrize("n", ALL_TIE_N)
def test_all_rows_tie(gpu, all_tie, n, layout):
    """d = 32, m = 2, K = 256, dsub 16, every row a tie: an empty tail, exactly one full batch,
    one full plus one partial batch, several waves of a workgroup finishing with leftovers."""
    x, cent, want = all_tie
    got, rr = _codes(gpu, x[:n], cent, layout)
    assert np.array_equal(got, want[:n]), (got != want[:n]).sum()
    assert rr > 0


def _nearest_other(cent_p):
    """index of every centroid's nearest other centroid (one part, (k, dsub))"""
    d2 = ((cent_p[:, None, :] - cent_p[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d2, np.inf)
    return d2.argmin(1)


@pytest.mark.parametrize("lo", [False, True])
def test_some_rows_tie(gpu, oracle, lo):
    """n = 4,096 + 17; rows r % 7 == 0 are exact midpoints of a centroid and its nearest
    neighbour (integer centroids below 100: the .5 midpoints are bf16-exact), the others random
    integer rows.  `lo`: a few rows carry a value that is not bf16-exact, so their chunks run
    the tile loop with the lo pass and the others the one without."""
    torch, codec, ctx = gpu
    rng = np.random.default_rng(72)
    n, m, dsub = 4096 + 17, 2, 16
    cent = rng.integers(0, 100, (m, 256, dsub)).astype(np.float32)
    x = rng.integers(0, 100, (n, m * dsub)).astype(np.float32)
    tie_rows = np.arange(0, n, 7)
    for p in range(m):
        a = rng.integers(0, 256, tie_rows.size)
        b = _nearest_other(cent[p])[a]
        x[tie_rows, p * dsub:(p + 1) * dsub] = (cent[p][a] + cent[p][b]) / 2
    if lo:
        x[1::500, 3] += np.float32(0.001)
        assert (x.view(np.uint32) & 0xFFFF).any()
    else:
        assert not (x.view(np.uint32) & 0xFFFF).any()
    want, _ = oracle.pq_assign(x, cent, threads=0)
    counts = torch.zeros((m, 256), dtype=torch.int32, device="cuda")
    got, rr = _codes(gpu, x, cent, "rows", counts)
    assert np.array_equal(got, want), (got != want).sum()
    assert rr > 0
    assert np.array_equal(codec.counts_to_host(counts), oracle.histogram(want, 256, False))
    got_p, rr_p = _codes(gpu, x, cent, "parts")
    assert np.array_equal(got_p, want) and rr_p > 0


def _spread_centroids(rng, m, dsub):
    """distinct centroids on a grid of pitch 8 (two of them differ by >= 8 in some dim)"""
    while True:
        cent = (rng.integers(0, 12, (m, 256, dsub)) * 8).astype(np.float32)
        if all(np.unique(cent[p], axis=0).shape[0] == 256 for p in range(m)):
            return cent


# centroid indices in different 32-row tiles and both half-waves (accumulator row
# (i & 3) + 8 (i >> 2) + 4 h: bit 2 of the row within the tile is the half-wave)
EQUI_IDX = (5, 40, 100, 250, 33, 70, 135, 172, 201, 238)


@pytest.mark.parametrize("ncand", [4, 10])
def test_equidistant_candidates_first_index(gpu, oracle, ncand):
    """One row with `ncand` centroids at the same distance, in different tiles and half-waves
    (4: two candidate slots of both half-waves; 10: more than one candidate round); the first
    index must win.  Every other row sits on a centroid of its own, far from all others."""
    rng = np.random.default_rng(73)
    n, m, dsub = 64 + 9, 2, 16
    cent = _spread_centroids(rng, m, dsub) + 200.0   # (the grid lies away from the tie row)
    base = rng.integers(20, 60, dsub).astype(np.float32)
    idx = EQUI_IDX[:ncand]
    for j, k in enumerate(idx):   # base +- 2 e_(j / 2): all at squared distance 4
        c = base.copy()
        c[j // 2] += 2.0 if j % 2 == 0 else -2.0
        cent[0, k] = c
    assert len({(k >> 5, (k >> 2) & 1) for k in idx}) >= 4
    pick = rng.integers(0, 256, (n, m))
    x = np.concatenate([cent[p][pick[:, p]] for p in range(m)], axis=1)
    x = x + rng.integers(-1, 2, x.shape).astype(np.float32)
    row = 37
    x[row, :dsub] = base
    want, _ = oracle.pq_assign(x, cent, threads=0)
    assert want[row, 0] == min(idx)
    for layout in ("rows", "parts"):
        got, rr = _codes(gpu, x, cent, layout)
        assert np.array_equal(got, want), (layout, np.argwhere(got != want))
        assert rr > 0


def test_single_tying_row_in_its_wave(gpu, oracle):
    """One exact midpoint among rows that screen far from any tie: its batch holds one entry
    with one candidate per half-wave slot at most, and the later slots are skipped."""
    rng = np.random.default_rng(74)
    n, m, dsub = 64 * 4 + 11, 2, 16
    cent = _spread_centroids(rng, m, dsub)
    cent[0, 200] = cent[0, 17]
    cent[0, 200, 0] += 8.0 if cent[0, 17, 0] < 48 else -8.0
    assert np.unique(cent[0], axis=0).shape[0] == 256
    pick = rng.integers(0, 256, (n, m))
    x = np.concatenate([cent[p][pick[:, p]] for p in range(m)], axis=1)
    x = x + rng.integers(-1, 2, x.shape).astype(np.float32)
    row = 64 + 21
    x[row, :dsub] = (cent[0, 17] + cent[0, 200]) / 2
    want, _ = oracle.pq_assign(x, cent, threads=0)
    assert want[row, 0] == 17
    for layout in ("rows", "parts"):
        got, rr = _codes(gpu, x, cent, layout)
        assert np.array_equal(got, want), (layout, np.argwhere(got != want))
        assert rr > 0


def test_deep_shaped_all_rows_tie(gpu, oracle):
    """d = 96, m = 16, dsub 6 (the instantiation without the half-wave split), n = 2,049."""
    rng = np.random.default_rng(75)
    x = rng.integers(0, 30, (2049, 96)).astype(np.float32)
    cent = _dup_centroids(rng, 16, 256, 6, 30)
    want, _ = oracle.pq_assign(x, cent, threads=0)
    for layout in ("rows", "parts"):
        got, rr = _codes(gpu, x, cent, layout)
        assert np.array_equal(got, want), (layout, (got != want).sum())
        assert rr > 0


def test_k4096_all_rows_tie(gpu, oracle):
    """K = 4,096 (dsub 16, u16 codes, tiles streamed from L2), n = 257, every row a tie."""
    rng = np.random.default_rng(76)
    x = rng.integers(0, 50, (257, 32)).astype(np.float32)
    cent = _dup_centroids(rng, 2, 4096, 16, 50)
    want, _ = oracle.pq_assign(x, cent, threads=0)
    want = want.astype(np.uint16)
    for layout in ("rows", "parts"):
        got, rr = _codes(gpu, x, cent, layout)
        assert np.array_equal(got, want), (layout, (got != want).sum())
        assert rr > 0


def test_smallest_grid_all_rows_tie(gpu, oracle):
    """One workgroup per subspace (the smallest grid the tuning gives: workgroups per CU
    below 1 / CUs), n = 64 * 4 * 3 + 5, every row a tie: the four waves share 13 chunks through
    the work queue, so some take several chunks (full batches in the loop, a leftover at its
    end) and some may take none and only hand over an empty queue."""
    torch, codec, ctx = gpu
    rng = np.random.default_rng(77)
    n = 64 * 4 * 3 + 5
    x = rng.integers(0, 50, (n, 32)).astype(np.float32)
    cent = _dup_centroids(rng, 2, 256, 16, 50)
    want, _ = oracle.pq_assign(x, cent, threads=0)
    counts = torch.zeros((2, 256), dtype=torch.int32, device="cuda")
    ctx.set_tuning(assign_wgs_per_cu=1.0 / 4096)
    try:
        got, rr = _codes(gpu, x, cent, "rows", counts)
        got_p, rr_p = _codes(gpu, x, cent, "parts")
    finally:
        ctx.set_tuning(assign_wgs_per_cu=0)   # the default
    assert np.array_equal(got, want), (got != want).sum()
    assert rr > 0
    assert np.array_equal(codec.counts_to_host(counts), oracle.histogram(want, 256, False))
    assert np.array_equal(got_p, want) and rr_p > 0
