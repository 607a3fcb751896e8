"""PQ assignment at the inputs where its two decisions matter: the acceptance test
`gap > tau` of pq_assign_mfma (rows below, inside and above the band, at other magnitudes and
offsets, overflowing norms) and the host's choice of path in assign_impl (strided rows,
unaligned rows, non-finite centroids, another context, the exact kernel's shapes, the argument
checks); then pqh_pq_error and pqh_pq_reconstruct at the shapes their one golden case misses.
Codes are compared bit for bit with the CPU oracle run on contiguous copies at the same scale
(test_assign_cpu.py: the oracle's codes change under extreme scales)."""
import ctypes

import numpy as np
import pytest

import assign_ref as ar

pytestmark = pytest.mark.gpu

PQH_ERR_ARG, PQH_ERR_UNSUPPORTED = -1, -4
LAYOUTS = ("rows", "parts")


@pytest.fixture(scope="module")
def gpu():
    import torch
    from pq_huffman_amd import codec
    assert torch.cuda.is_available()
    ctx = codec.Context(0)
    return torch, codec, ctx


def _dev(gpu, x):
    torch = gpu[0]
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _host(codes, layout):
    """codes (n, m) as numpy, u16 for K > 256 (torch keeps them as int16)"""
    out = (codes if layout == "rows" else codes.t().contiguous()).cpu().numpy()
    return out.view(np.uint16) if out.dtype == np.int16 else out


def _run(pq, xd, layout, counts=None, mode=0, ctx=None):
    """(codes (n, m) as numpy, re-rank count of the context that ran) through either layout"""
    if layout == "rows":
        out = pq.assign(xd, counts=counts, mode=mode, ctx=ctx)
    else:   # part-major, ld padded to 128 codes
        out = pq.assign_parts(xd, counts=counts, mode=mode, ctx=ctx)
    rr = pq.rerank_count(ctx=ctx)   # (synchronises the stream)
    return _host(out, layout), rr


def _want(oracle, x, cent):
    w, _ = oracle.pq_assign(np.ascontiguousarray(x), cent, threads=0)
    return w   # (u8, or u16 for K > 256)


def _zero_counts(gpu, m, k):
    return gpu[0].zeros((m, k), dtype=gpu[0].int32, device="cuda")


def _dup_centroids(rng, m, k, dsub, hi):
    """integer centroids, the upper half a copy of the lower: every row ties"""
    cent = rng.integers(0, hi, (m, k, dsub)).astype(np.float32)
    cent[:, k // 2:] = cent[:, :k // 2]
    return cent


# ---- B1: near ties across the band, scales and offsets --------------------------------------
@pytest.fixture(scope="module")
def band():
    cache = {}

    def get(dsub, offset):
        if (dsub, offset) not in cache:   # (test_assign_cpu.py asserts what these rows cover)
            cache[(dsub, offset)] = ar.near_tie(ar.N_BAND, ar.parts_of(dsub), dsub,
                                                seed=100 + dsub, offset=offset)
        return cache[(dsub, offset)]
    return get


@pytest.mark.parametrize("s", [0, 40, -40, -60, -75, 62])
@pytest.mark.parametrize("offset", [0.0, 64.0])
@pytest.mark.parametrize("dsub", ar.DSUBS)
def test_near_ties_scales_offsets(gpu, oracle, band, dsub, offset, s):
    """K = 256, n = 2,085: rows at +-2^-2 .. 2^-30 of a centroid pair's midpoint, x and the
    centroids times 2^s.  At 2^62 the norms overflow or tau comes within 2^110 of it (at dsub 4
    ||x||^2 and tau stay finite while a score can overflow); either way the inline path runs.
    2^-60 puts every gap below the bound's 1e-30 floors, 2^-75 underflows the squares (all
    ties); offset 64 cancels (nearly every row is re-ranked)."""
    torch, codec, ctx = gpu
    x0, c0 = band(dsub, offset)
    x, cent = ar.scaled(x0, s), ar.scaled(c0, s)
    assert np.isfinite(x).all() and np.isfinite(cent).all()
    want = _want(oracle, x, cent)
    pq = codec.PQ(ctx, cent)
    xd = _dev(gpu, x)
    for layout in LAYOUTS:
        got, rr = _run(pq, xd, layout)
        assert np.array_equal(got, want), (layout, (got != want).sum())
        if s == 0:
            assert rr > 0


@pytest.mark.parametrize("dsub", [6, 16])
def test_near_ties_mixed_scales_per_part(gpu, oracle, band, dsub):
    """part 0 times 2^40, part 1 times 2^-40: the bound's coefficients are per subspace"""
    torch, codec, ctx = gpu
    x0, c0 = band(dsub, 0.0)
    x, cent = x0.copy(), c0.copy()
    x[:, :dsub], cent[0] = ar.scaled(x0[:, :dsub], 40), ar.scaled(c0[0], 40)
    x[:, dsub:], cent[1] = ar.scaled(x0[:, dsub:], -40), ar.scaled(c0[1], -40)
    want = _want(oracle, x, cent)
    assert np.array_equal(want, _want(oracle, x0, c0))   # (each part alone is a pure scale)
    pq = codec.PQ(ctx, cent)
    for layout in LAYOUTS:
        got, rr = _run(pq, _dev(gpu, x), layout)
        assert np.array_equal(got, want), (layout, (got != want).sum())
        assert rr > 0


@pytest.mark.parametrize("s", [0, 40])
def test_near_ties_k4096(gpu, oracle, s):
    """K = 4,096, dsub 16, m = 2, n = 257: 2,048 centroids and their copies plus N(0, 2^-12),
    rows between a centroid and its twin"""
    torch, codec, ctx = gpu
    x0, c0 = ar.near_tie(257, 2, 16, seed=131, cent=ar.dup_k4096(16, 2, seed=130))
    x, cent = ar.scaled(x0, s), ar.scaled(c0, s)
    want = _want(oracle, x, cent)
    assert want.dtype == np.uint16 and (want >= 2048).any() and (want < 2048).any()
    pq = codec.PQ(ctx, cent)
    for layout in LAYOUTS:
        got, rr = _run(pq, _dev(gpu, x), layout)
        assert np.array_equal(got, want), (layout, (got != want).sum())
        assert rr > 0


def test_near_ties_fused_histogram_scaled(gpu, oracle, band):
    """the fused histogram (counts=) at 2^40: every row counted once under its final code,
    whether the screen or the re-rank decided it"""
    torch, codec, ctx = gpu
    x0, c0 = band(16, 0.0)
    x, cent = ar.scaled(x0, 40), ar.scaled(c0, 40)
    want = _want(oracle, x, cent)
    pq = codec.PQ(ctx, cent)
    for layout in LAYOUTS:
        counts = _zero_counts(gpu, 2, 256)
        got, _ = _run(pq, _dev(gpu, x), layout, counts)
        assert np.array_equal(got, want)
        assert np.array_equal(codec.counts_to_host(counts), oracle.histogram(want, 256, False))


# ---- B2: strided rows on the MFMA path -------------------------------------------------------
def _all_tie(seed, n, m, k, dsub):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 50, (n, m * dsub)).astype(np.float32)
    return x, _dup_centroids(rng, m, k, dsub, 50)


@pytest.mark.parametrize("k,dsub", [(256, d) for d in ar.DSUBS] + [(4096, 16)])
def test_strided_rows_mfma(gpu, oracle, k, dsub):
    """x = wide[:, :d] of a NaN-filled (n, d + 4) tensor (16-byte aligned rows: the MFMA
    kernel's vector loads), n = 64 * 4 + 33, every row a tie: the lane offsets, the clamped last
    block and the re-rank tail's row address all use ld_x = d + 4; a NaN read from the gap
    would change codes or counts."""
    torch, codec, ctx = gpu
    n, m = 64 * 4 + 33, 2
    x, cent = _all_tie(200 + dsub + k, n, m, k, dsub)
    want = _want(oracle, x, cent)
    pq = codec.PQ(ctx, cent)
    xd = ar.strided(torch, x, 4)
    assert xd.stride(0) == m * dsub + 4 and xd.data_ptr() % 16 == 0
    for layout in LAYOUTS:
        counts = None if (layout == "parts" and k > 256) else _zero_counts(gpu, m, k)
        got, rr = _run(pq, xd, layout, counts)
        assert np.array_equal(got, want), (layout, (got != want).sum())
        assert rr > 0   # (the screen and the re-rank tail ran)
        if counts is not None:
            assert np.array_equal(codec.counts_to_host(counts), oracle.histogram(want, k, False))


# ---- B3: the alignment fallback --------------------------------------------------------------
def _unaligned(gpu, x, how):
    """the same rows (a) with ld_x = d + 3, NaN gaps; (b) one float into an allocation"""
    torch = gpu[0]
    n, d = x.shape
    if how == "ld":
        xd = ar.strided(torch, x, 3)
        assert xd.stride(0) % 4 != 0
        return xd
    flat = torch.full((n * d + 8,), float("nan"), dtype=torch.float32, device="cuda")
    flat[1:1 + n * d] = torch.from_numpy(x.reshape(-1)).cuda()
    xd = flat[1:1 + n * d].view(n, d)
    assert xd.data_ptr() % 16 == 4 and xd.stride(0) == d
    return xd


@pytest.mark.parametrize("how", ["ld", "ptr"])
@pytest.mark.parametrize("dsub", [4, 8, 12, 16, 32])
def test_unaligned_rows_take_the_exact_kernel(gpu, oracle, dsub, how):
    """dsub % 4 == 0 and rows that are not 16-byte aligned: assign_impl sends the call to the
    exact kernel (the MFMA kernel would load 16 bytes at a time), which re-ranks nothing"""
    torch, codec, ctx = gpu
    n, m = 64 * 4 + 33, 2
    x, cent = _all_tie(300 + dsub, n, m, 256, dsub)
    want = _want(oracle, x, cent)
    pq = codec.PQ(ctx, cent)
    _, rr_aligned = _run(pq, _dev(gpu, x), "rows")
    assert rr_aligned > 0   # (aligned, the same call screens)
    xd = _unaligned(gpu, x, how)
    for layout in LAYOUTS:
        counts = _zero_counts(gpu, m, 256)
        got, rr = _run(pq, xd, layout, counts)
        assert np.array_equal(got, want), (layout, (got != want).sum())
        assert rr == 0
        assert np.array_equal(codec.counts_to_host(counts), oracle.histogram(want, 256, False))


@pytest.mark.parametrize("how", ["ld", "ptr"])
def test_unaligned_rows_dsub6_stay_on_mfma(gpu, oracle, how):
    """dsub 6 (d = 96, m = 16) loads its slices one float at a time, so unaligned rows stay on
    the MFMA kernel: the re-rank count shows it ran"""
    torch, codec, ctx = gpu
    n, m = 64 * 4 + 33, 16
    x, cent = _all_tie(306, n, m, 256, 6)
    want = _want(oracle, x, cent)
    pq = codec.PQ(ctx, cent)
    xd = _unaligned(gpu, x, how)
    for layout in LAYOUTS:
        got, rr = _run(pq, xd, layout)
        assert np.array_equal(got, want), (layout, (got != want).sum())
        assert rr > 0


# ---- B4: centroid and row magnitudes -----------------------------------------------------------
def test_nonfinite_centroids_take_the_exact_kernel(gpu, oracle, band):
    """one NaN and one inf entry in part 0: no MFMA fragments are built, the exact kernel runs"""
    torch, codec, ctx = gpu
    x, c0 = band(16, 0.0)
    cent = c0.copy()
    cent[0, 5, 3] = np.nan
    cent[0, 77, 0] = np.inf
    want = _want(oracle, x, cent)
    assert not np.array_equal(want, _want(oracle, x, c0))   # (rows of centroids 5 and 77 move)
    pq = codec.PQ(ctx, cent)
    for layout in LAYOUTS:
        got, rr = _run(pq, _dev(gpu, x), layout)
        assert np.array_equal(got, want), (layout, (got != want).sum())
        assert rr == 0


def test_centroid_norm_overflows(gpu, oracle, band):
    """finite entries of about 2^64 in one centroid of part 1: ||c||^2 overflows, so Cmax and
    tau are inf for the subspace and its accumulator starts at inf for that centroid"""
    torch, codec, ctx = gpu
    x, c0 = band(16, 0.0)
    cent = c0.copy()
    cent[1, 200, ::3] = np.float32(2.0 ** 64) * np.float32(1.25)
    cent[1, 200, 1] = -np.float32(2.0 ** 64)
    assert np.isfinite(cent).all()
    want = _want(oracle, x, cent)
    pq = codec.PQ(ctx, cent)
    for layout in LAYOUTS:
        got, _ = _run(pq, _dev(gpu, x), layout)
        assert np.array_equal(got, want), (layout, (got != want).sum())


def test_row_norm_overflows(gpu, oracle, band):
    """the mirror image: rows with finite entries of 2^64 (||x||^2 = inf, every distance inf:
    code 0) among ordinary rows, in full blocks and in the clamped last block"""
    torch, codec, ctx = gpu
    x0, cent = band(16, 0.0)
    x = x0.copy()
    rows = np.array([0, 31, 32, 700, 1033, x.shape[0] - 1])
    x[rows, 2] = np.float32(2.0 ** 64)
    x[rows[::2], 20] = -np.float32(2.0 ** 64) * np.float32(1.5)
    assert np.isfinite(x).all()
    want = _want(oracle, x, cent)
    assert (want[rows, 0] == 0).all()
    pq = codec.PQ(ctx, cent)
    for layout in LAYOUTS:
        got, rr = _run(pq, _dev(gpu, x), layout)
        assert np.array_equal(got, want), (layout, np.argwhere(got != want)[:8])
        assert rr > 0


# ---- B5: another context ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_books(oracle):
    """d = 128 twice: m = 16 (dsub 8) and m = 8 (dsub 16), near-tie rows"""
    n = 4096 + 37
    x16, c16 = ar.near_tie(n, 16, 8, seed=501)
    x8, c8 = ar.near_tie(n, 8, 16, seed=502)
    return (x16, c16, _want(oracle, x16, c16)), (x8, c8, _want(oracle, x8, c8))


def test_assign_on_another_context(gpu, oracle, two_books):
    """PQ prepared on context A, assign(..., ctx=B) with B on a stream of its own, in the order
    A, B, B, A, B with codebooks of m = 16 and m = 8 interleaved: B's work-queue heads (reset by
    its own previous launch, for every subspace) and B's re-rank counter serve the launch.  One
    workgroup per subspace on both contexts, so its four waves share the 65 chunks through the
    work queue."""
    torch, codec, A = gpu
    B = codec.Context(0, stream=torch.cuda.Stream())
    (x16, c16, w16), (x8, c8, w8) = two_books
    pq16, pq8 = codec.PQ(A, c16), codec.PQ(A, c8)
    xd16, xd8 = _dev(gpu, x16), _dev(gpu, x8)
    n = x16.shape[0]
    try:
        A.set_tuning(assign_wgs_per_cu=1.0 / 4096)
        B.set_tuning(assign_wgs_per_cu=1.0 / 4096)
        alone = {}   # re-rank counts of runs on A alone
        for name, pq, xd, want in (("16", pq16, xd16, w16), ("8", pq8, xd8, w8)):
            got, alone[name] = _run(pq, xd, "rows")
            assert np.array_equal(got, want) and alone[name] > 0
        torch.cuda.synchronize()   # (the uploads and A's runs are done before B's stream starts)
        # outputs allocated up front and kept: nothing is freed while another stream may run
        outs = [torch.full((n, m), 255, dtype=torch.uint8, device="cuda")
                for m in (16, 8, 16, 8, 16)]
        torch.cuda.synchronize()
        plan = ((A, pq16, xd16, w16, "16"), (B, pq8, xd8, w8, "8"), (B, pq16, xd16, w16, "16"),
                (A, pq8, xd8, w8, "8"), (B, pq16, xd16, w16, "16"))
        for out, (c, pq, xd, want, name) in zip(outs, plan):
            pq.assign(xd, codes=out, ctx=c)
            assert pq.rerank_count(ctx=c) == alone[name], (name, c is B)
        A.sync()
        B.sync()
        for out, (c, pq, xd, want, name) in zip(outs, plan):
            assert np.array_equal(out.cpu().numpy(), want), (name, c is B)
        for layout in LAYOUTS:   # and the part-major layout on B
            got, rr = _run(pq8, xd8, layout, ctx=B)
            assert np.array_equal(got, w8) and rr == alone["8"]
    finally:
        A.set_tuning(assign_wgs_per_cu=0)
        B.set_tuning(assign_wgs_per_cu=0)
        torch.cuda.synchronize()


# n of the concurrent case.  Judged by the events the test records on both streams (printed,
# not asserted: a timing).  With one workgroup per subspace a launch of 8 workgroups took
# 0.49 ms at this n on an MI355X (48 ns per row), and the two streams' spans, 0.021 - 1.500 ms
# and 0.025 - 1.505 ms after the common start, overlapped for 1.475 ms: all three launches of
# each ran beside the other's.  A launch has to outlast the host's issue of the other
# stream's next launch (the six are issued alternately, 5 us apart here, tens of us on a
# loaded host); 10 K rows keep that margin above ten, 2 K rows (0.1 ms) would leave three.
# This is the one n that was timed: no smaller n was tried, so it is not shown to be the
# smallest that overlaps, only one that does with room to spare.
# The two grids take 16 of the 256 CUs, so neither waits for the other to drain.
N_CONCURRENT = 10240 + 37


def test_two_streams_assign_concurrently(gpu, oracle):
    """Two side streams, each a context of its own, three back-to-back assign launches of the
    same codebook each into separate outputs, no synchronisation between the streams until the
    end: all six outputs equal the oracle."""
    torch, codec, A = gpu
    x, cent = ar.near_tie(N_CONCURRENT, 8, 16, seed=503)
    want = _want(oracle, x, cent)
    pq = codec.PQ(A, cent)
    xd = _dev(gpu, x)
    side = [codec.Context(0, stream=torch.cuda.Stream()) for _ in range(2)]
    outs = [[torch.full((N_CONCURRENT, 8), 255, dtype=torch.uint8, device="cuda")
             for _ in range(3)] for _ in range(2)]
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(2)]
    t0 = torch.cuda.Event(enable_timing=True)
    try:
        for c in side:
            c.set_tuning(assign_wgs_per_cu=1.0 / 4096)
        torch.cuda.synchronize()
        t0.record()
        for c in side:
            c.stream.wait_event(t0)
        for i, c in enumerate(side):
            ev[i][0].record(c.stream)
        for j in range(3):
            for i, c in enumerate(side):
                pq.assign(xd, codes=outs[i][j], ctx=c)
        for i, c in enumerate(side):
            ev[i][1].record(c.stream)
        for c in side:
            c.sync()
        spans = [(t0.elapsed_time(ev[i][0]), t0.elapsed_time(ev[i][1])) for i in range(2)]
        overlap = min(spans[0][1], spans[1][1]) - max(spans[0][0], spans[1][0])
        print(f"stream spans (ms from the start): {spans}, overlap {overlap:.3f} ms")
        for i in range(2):
            for j in range(3):
                got = outs[i][j].cpu().numpy()
                assert np.array_equal(got, want), (i, j, (got != want).sum())
    finally:
        for c in side:
            c.set_tuning(assign_wgs_per_cu=0)
        torch.cuda.synchronize()


# ---- B6: the exact kernel's matrix and the argument checks ---------------------------------------
@pytest.fixture(scope="module")
def plain():
    rng = np.random.default_rng(601)
    return rng.normal(0.0, 1.0, (500, 32)).astype(np.float32)


@pytest.mark.parametrize("k", [16, 300, 1000])
def test_exact_kernel_parts_layout(gpu, oracle, plain, k):
    """K the MFMA kernel has no form for, part-major codes (u8 up to 256, u16 above), with
    counts for K <= 256"""
    torch, codec, ctx = gpu
    x = plain
    cent = np.ascontiguousarray(
        x[np.random.default_rng(k).choice(500, k, replace=k > 500)].reshape(k, 4, 8)
        .transpose(1, 0, 2)) + np.float32(0.25)
    want = _want(oracle, x, cent)
    pq = codec.PQ(ctx, cent)
    for layout in LAYOUTS:
        counts = _zero_counts(gpu, 4, k) if k <= 256 else None
        got, rr = _run(pq, _dev(gpu, x), layout, counts)
        assert got.dtype == want.dtype and np.array_equal(got, want), (layout, k)
        assert rr == 0
        if counts is not None:
            assert np.array_equal(codec.counts_to_host(counts), oracle.histogram(want, k, False))


def test_exact_mode_parts_counts_k256(gpu, oracle, band):
    """mode = 1 (the exact kernel on a shape the MFMA kernel serves) with part-major codes and
    counts"""
    torch, codec, ctx = gpu
    x, cent = band(8, 0.0)
    want = _want(oracle, x, cent)
    pq = codec.PQ(ctx, cent)
    counts = _zero_counts(gpu, 2, 256)
    got, rr = _run(pq, _dev(gpu, x), "parts", counts, mode=1)
    assert np.array_equal(got, want) and rr == 0
    assert np.array_equal(codec.counts_to_host(counts), oracle.histogram(want, 256, False))


def test_argument_checks(gpu, plain):
    """parts + K > 256 + counts is unsupported; ld_x < d and ld_codes < n are argument errors;
    n = 0 is OK, writes nothing and reports no re-rank"""
    from pq_huffman_amd.capi import lib
    torch, codec, ctx = gpu
    x = plain
    n, d = x.shape
    xd = _dev(gpu, x)
    big = codec.PQ(ctx, np.random.default_rng(602).normal(0, 1, (4, 300, 8)).astype(np.float32))
    with pytest.raises(codec.PqhError) as e:
        big.assign_parts(xd, counts=_zero_counts(gpu, 4, 300))
    assert e.value.status == PQH_ERR_UNSUPPORTED
    pq = codec.PQ(ctx, np.random.default_rng(603).normal(0, 1, (4, 256, 8)).astype(np.float32))
    codes = torch.full((4, n + 11), 201, dtype=torch.uint8, device="cuda")
    P = ctypes.c_void_p
    assert lib().pqh_pq_assign(ctx.ptr, pq.ptr, P(xd.data_ptr()), n, d - 1, P(codes.data_ptr()),
                               None, 0) == PQH_ERR_ARG
    assert lib().pqh_pq_assign_parts(ctx.ptr, pq.ptr, P(xd.data_ptr()), n, d, P(codes.data_ptr()),
                                     n - 1, None, 0) == PQH_ERR_ARG
    pq.assign(xd)   # (a launch that re-ranks or not: the n = 0 call below must report 0)
    assert lib().pqh_pq_assign(ctx.ptr, pq.ptr, P(xd.data_ptr()), 0, d, P(codes.data_ptr()),
                               None, 0) == 0
    assert pq.rerank_count() == 0
    assert lib().pqh_pq_assign_parts(ctx.ptr, pq.ptr, P(xd.data_ptr()), 0, d, P(codes.data_ptr()),
                                     n + 11, None, 0) == 0
    assert pq.rerank_count() == 0
    ctx.sync()
    assert (codes == 201).all().item()


# ---- C: error and reconstruct ----------------------------------------------------------------------
ERR_SHAPES = ((256, 6, 16), (300, 8, 4), (4096, 16, 2))   # (K, dsub, m)


@pytest.fixture(scope="module")
def err_cases(oracle):
    out = {}
    for k, dsub, m in ERR_SHAPES:
        rng = np.random.default_rng(700 + k)
        x = rng.normal(0.0, 1.0, (1000, m * dsub)).astype(np.float32)
        cent = rng.normal(0.0, 1.0, (m, k, dsub)).astype(np.float32)
        codes = rng.integers(0, k, (1000, m)).astype(np.uint8 if k <= 256 else np.uint16)
        codes[::3] = _want(oracle, x[::3], cent)   # (some nearest, some arbitrary: both are codes)
        codes[-1, :], codes[0, :] = k - 1, 0
        out[(k, dsub, m)] = (x, cent, codes)
    return out


def _codes_dev(gpu, codes):
    torch = gpu[0]
    c = np.ascontiguousarray(codes)
    return torch.from_numpy(c.view(np.int16) if c.dtype == np.uint16 else c).cuda()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
@pytest.mark.parametrize("shape", ERR_SHAPES)
def test_error_shapes(gpu, oracle, err_cases, shape, n):
    """pq.error against the oracle's compute_error at relative 1e-12 (the 256-row block sums
    are added in another order): u8 and u16 codes, dsub 6, the partial-block boundary"""
    torch, codec, ctx = gpu
    x, cent, codes = err_cases[shape]
    pq = codec.PQ(ctx, cent)
    got = pq.error(_dev(gpu, x[:n]), _codes_dev(gpu, codes[:n]))
    want = oracle.compute_error(x[:n], cent, codes[:n])
    assert want > 0 and abs(got - want) <= 1e-12 * abs(want)


def test_error_strided_rows(gpu, oracle, err_cases):
    """ld_x = d + 3 with NaN gaps (u16 codes): a gap float read would make the sum NaN"""
    torch, codec, ctx = gpu
    x, cent, codes = err_cases[(4096, 16, 2)]
    pq = codec.PQ(ctx, cent)
    got = pq.error(ar.strided(torch, x, 3), _codes_dev(gpu, codes))
    want = oracle.compute_error(x, cent, codes)
    assert abs(got - want) <= 1e-12 * abs(want)


@pytest.mark.parametrize("shape", ERR_SHAPES)
def test_reconstruct_padded_output(gpu, err_cases, shape):
    """pqh_pq_reconstruct into a sentinel-filled (n, d + 3) buffer: the d columns are the
    gathered centroids bit for bit, the pad columns keep the sentinel"""
    from pq_huffman_amd.capi import lib
    torch, codec, ctx = gpu
    x, cent, codes = err_cases[shape]
    k, dsub, m = shape
    n, d = 257, m * dsub
    pq = codec.PQ(ctx, cent)
    out = torch.full((n, d + 3), -7.5, dtype=torch.float32, device="cuda")
    cd = _codes_dev(gpu, codes[:n])
    P = ctypes.c_void_p
    assert lib().pqh_pq_reconstruct(ctx.ptr, pq.ptr, P(cd.data_ptr()), n, P(out.data_ptr()),
                                    d + 3) == 0
    assert lib().pqh_pq_reconstruct(ctx.ptr, pq.ptr, P(cd.data_ptr()), n, P(out.data_ptr()),
                                    d - 1) == PQH_ERR_ARG
    ctx.sync()
    got = out.cpu().numpy()
    ref = np.concatenate([cent[i][codes[:n, i]] for i in range(m)], axis=1)
    assert np.array_equal(got[:, :d].view(np.uint32), ref.view(np.uint32))
    assert (got[:, d:] == -7.5).all()
