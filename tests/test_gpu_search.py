"""ADC search of a compressed stream (pqh_adc_tables, pqh_search_stream, pqh_search_codes).
Expected values come from numpy in this file -- the distance summed part by part in float32,
the order np.lexsort((ids, dist)) -- never from the calls under test.  The order is total and
the arithmetic fixed, so every comparison is array_equal on the ids and on the raw float bits."""
import ctypes

import numpy as np
import pytest

import datagen

pytestmark = pytest.mark.gpu

N = 1003   # not a multiple of any chunk size below
CHUNKS = [1, 4, 7, 32, 64]
NQ = 9     # crosses one query batch at either batch size (8 or 4)
# name: (m, k, context)
MODES = {"ctx_m8": (8, 256, True), "noctx_m8": (8, 256, False), "ctx_m16": (16, 256, True),
         "noctx_m3": (3, 256, False)}
POISON = (0xFFFFFFFF, 0xA5A5A5A5, 0x00000001)


@pytest.fixture(scope="module")
def gpu():
    import torch
    from pq_huffman_amd import codec
    assert torch.cuda.is_available()
    return torch, codec, codec.Context(0)


@pytest.fixture(scope="module")
def coded(gpu):
    """mode -> (host codes, device codes, tables), built once"""
    torch, codec, ctx = gpu
    made = {}

    def get(mode):
        if mode not in made:
            m, k, ctxm = MODES[mode]
            codes = datagen.skewed_codes(N, m, k=k, seed=100 + m + k)
            cd = torch.from_numpy(codes).cuda()
            counts = codec.histogram(ctx, cd, k, ctxm)
            cbs = codec.Codebooks(codec.counts_to_host(counts), k, ctxm)
            made[mode] = (codes, cd, codec.Tables.from_codebooks(ctx, cbs))
        return made[mode]
    return get


def _lut(nq, m, seed, k=256):
    return np.random.default_rng(seed).normal(0.0, 100.0, size=(nq, m, k)).astype(np.float32)


def _ties_lut(nq, m, seed):
    """only the values 0, 1, 2: hundreds of rows share each distance, the ids decide"""
    return np.random.default_rng(seed).integers(0, 3, size=(nq, m, 256)).astype(np.float32)


def _dists(lut, codes):
    """[nq][n] float32, parts added left to right"""
    out = np.empty((lut.shape[0], codes.shape[0]), np.float32)
    for q in range(lut.shape[0]):
        dist = lut[q, 0, codes[:, 0]]
        for i in range(1, codes.shape[1]):
            dist = dist + lut[q, i, codes[:, i]]
        assert dist.dtype == np.float32
        out[q] = dist
    return out


def _want(lut, codes, k, id_base=0, first=0):
    """the top k of rows [first, n) by (dist, id), padded with (+inf, -1)"""
    d = _dists(lut, codes)
    wd = np.full((lut.shape[0], k), np.inf, np.float32)
    wi = np.full((lut.shape[0], k), -1, np.int64)
    ids = np.arange(first, codes.shape[0], dtype=np.int64)
    for q in range(lut.shape[0]):
        dist = d[q, first:]
        order = np.lexsort((ids, dist))[:k]
        wd[q, :len(order)] = dist[order]
        wi[q, :len(order)] = ids[order] - first + id_base
    return wd, wi


def _check(got, want, what=""):
    gd, gi = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert gd.dtype == np.float32 and gi.dtype == np.int64
    assert np.array_equal(gi, want[1]), what
    assert np.array_equal(gd.view(np.uint32), want[0].view(np.uint32)), what


def _status(fn):
    from pq_huffman_amd.capi import PqhError
    try:
        fn()
    except PqhError as err:
        return err.status
    return 0


@pytest.mark.parametrize("m,dsub,kind", [(8, 16, "sift"), (16, 6, "deep")])
def test_tables(gpu, m, dsub, kind):
    torch, codec, ctx = gpu
    d = m * dsub
    x = datagen.sift_like(3000, d) if kind == "sift" else datagen.deep_like(3000, d)
    cent = datagen.lloyd_centroids(x, m, 256, iters=2, sample=3000)
    queries = (datagen.sift_like(3, d, seed=77) if kind == "sift"
               else datagen.deep_like(3, d, seed=77)).astype(np.float32)
    pq = codec.PQ(ctx, cent)
    want = np.empty((3, m, 256), np.float32)
    c = np.ascontiguousarray(cent, np.float32)
    for q in range(3):
        for i in range(m):
            acc = np.zeros(256, np.float32)
            for j in range(dsub):
                t = queries[q, i * dsub + j] - c[i, :, j]
                acc = acc + t * t
            want[q, i] = acc
    assert want.dtype == np.float32
    got = codec.adc_tables(ctx, pq, torch.from_numpy(queries).cuda())
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    # query rows further apart than their length
    wide = torch.zeros((3, d + 5), dtype=torch.float32, device="cuda")
    wide[:, :d] = torch.from_numpy(queries).cuda()
    got = codec.adc_tables(ctx, pq, wide)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("mode", list(MODES))
def test_exact_topk_over_the_stream(gpu, coded, mode, chunk):
    torch, codec, ctx = gpu
    codes, cd, tabs = coded(mode)
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=chunk)
    lut = _lut(NQ, codes.shape[1], chunk)
    ld = torch.from_numpy(lut).cuda()
    for k in (1, 10, 64):
        _check(codec.search(ctx, tabs, enc, ld, k), _want(lut, codes, k), k)
    codec.decode_status(ctx)


@pytest.mark.parametrize("mode,chunk", [("ctx_m8", 200), ("ctx_m16", 250), ("noctx_m3", N)])
def test_chunks_too_long_for_a_64_chunk_stage(gpu, coded, mode, chunk):
    """64 chunks of C * m > 1.5 KB do not fit a wave's stage: fewer lanes walk per step, from
    the global stream"""
    torch, codec, ctx = gpu
    codes, cd, tabs = coded(mode)
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=chunk)
    lut = _lut(NQ, codes.shape[1], chunk)
    _check(codec.search(ctx, tabs, enc, torch.from_numpy(lut).cuda(), 64), _want(lut, codes, 64))
    codec.decode_status(ctx)


@pytest.mark.parametrize("chunk", [4, 7])
def test_ties_are_decided_by_the_id(gpu, coded, chunk):
    torch, codec, ctx = gpu
    codes, cd, tabs = coded("ctx_m8")
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=chunk)
    lut = _ties_lut(NQ, 8, 5)
    want = _want(lut, codes, 64)
    d = _dists(lut, codes)   # the 64th distance is shared with rows that stay outside
    assert any((d[q] == want[0][q, -1]).sum() > (want[0][q] == want[0][q, -1]).sum() for q in range(NQ))
    assert all(len(np.unique(want[0][q])) < 16 for q in range(NQ))
    _check(codec.search(ctx, tabs, enc, torch.from_numpy(lut).cuda(), 64), want)
    codec.decode_status(ctx)


def test_grid_independence(gpu, coded):
    """one workgroup looping over every chunk group, three with uneven spans, the default"""
    torch, codec, ctx = gpu
    codes, cd, tabs = coded("ctx_m8")
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=4)
    lut = _ties_lut(NQ, 8, 6)
    want = _want(lut, codes, 64)
    ld = torch.from_numpy(lut).cuda()
    try:
        for g in (1, 3, 0):
            ctx.set_tuning(search_groups=g)
            _check(codec.search(ctx, tabs, enc, ld, 64), want, g)
            _check(codec.search_codes(ctx, cd, ld, 64), want, g)
    finally:
        ctx.set_tuning(search_groups=0)
    codec.decode_status(ctx)


def test_edges(gpu, coded):
    torch, codec, ctx = gpu
    codes, cd, tabs = coded("ctx_m8")
    lut = _lut(NQ, 8, 21)
    ld = torch.from_numpy(lut).cuda()
    for n, k in ((1, 1), (1, 10), (5, 10), (256, 64), (257, 64)):   # 64 chunks of 4, and one more
        enc = codec.encode(ctx, tabs, cd[:n], chunk_vectors=4)
        want = _want(lut, codes[:n], k)
        if n == 5:
            assert np.isinf(want[0][:, 5:]).all() and (want[1][:, 5:] == -1).all()
        _check(codec.search(ctx, tabs, enc, ld, k), want, (n, k))
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=4)
    # no queries: nothing is written
    dist = torch.full((2, 10), 7.0, dtype=torch.float32, device="cuda")
    ids = torch.full((2, 10), 7, dtype=torch.int64, device="cuda")
    codec.search(ctx, tabs, enc, ld[:0], 10, out=(dist, ids))
    assert bool((dist == 7.0).all()) and bool((ids == 7).all())
    # a table of negative values (inner products)
    neg = -np.abs(lut) - 1.0
    _check(codec.search(ctx, tabs, enc, torch.from_numpy(neg).cuda(), 10), _want(neg, codes, 10))
    # ids come back with the base added
    _check(codec.search(ctx, tabs, enc, ld, 10, id_base=10**10), _want(lut, codes, 10, id_base=10**10))
    codec.decode_status(ctx)


@pytest.mark.parametrize("chunk", [7, 64])
def test_search_a_shard(gpu, coded, chunk):
    """rows [500, N) encoded as a shard (raw_first = 0, the halo row as context), searched
    with id_base = 500: the search of the whole stream restricted to ids >= 500"""
    torch, codec, ctx = gpu
    codes, cd, tabs = coded("ctx_m8")
    enc = codec.encode(ctx, tabs, cd[500:], chunk_vectors=chunk, raw_first=0, prev_row=cd[499])
    lut = _lut(NQ, 8, 31)
    got = codec.search(ctx, tabs, enc, torch.from_numpy(lut).cuda(), 10, id_base=500)
    _check(got, _want(lut, codes, 10, id_base=500, first=500))
    assert int(got[1].min()) >= 500
    codec.decode_status(ctx)


@pytest.mark.parametrize("mode", ["ctx_m8", "noctx_m3"])
def test_search_codes_equals_search(gpu, coded, mode):
    torch, codec, ctx = gpu
    codes, cd, tabs = coded(mode)
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=7)
    lut = _lut(NQ, codes.shape[1], 41)
    ld = torch.from_numpy(lut).cuda()
    want = _want(lut, codes, 64)
    a = codec.search(ctx, tabs, enc, ld, 64)
    b = codec.search_codes(ctx, cd, ld, 64)
    _check(a, want)
    _check(b, want)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    # rows that do not start on a 4-byte boundary
    off = cd.flatten()[codes.shape[1]:].view(N - 1, codes.shape[1]) if codes.shape[1] % 4 else None
    if off is not None:
        _check(codec.search_codes(ctx, off, ld, 10), _want(lut, codes[1:], 10))
    codec.decode_status(ctx)


def test_errors(gpu, coded):
    torch, codec, ctx = gpu
    codes, cd, tabs = coded("ctx_m8")
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=7)
    lut = _lut(2, 8, 51)
    ld = torch.from_numpy(lut).cuda()
    out = (torch.empty((2, 65), dtype=torch.float32, device="cuda"),
           torch.empty((2, 65), dtype=torch.int64, device="cuda"))
    for k in (65, 0):
        assert _status(lambda: codec.search(ctx, tabs, enc, ld, k, out=out)) == -1       # PQH_ERR_ARG
        assert _status(lambda: codec.search_codes(ctx, cd, ld, k, out=out)) == -1
    # a K = 4096 table set
    big = datagen.skewed_codes(N, 8, k=4096, seed=3)
    bd = torch.from_numpy(big.view(np.int16)).cuda()
    bt = codec.Tables.from_codebooks(
        ctx, codec.Codebooks(codec.counts_to_host(codec.histogram(ctx, bd, 4096, False)), 4096, False))
    benc = codec.encode(ctx, bt, bd, chunk_vectors=7)
    wide = torch.zeros((1, 8, 4096), dtype=torch.float32, device="cuda")
    assert _status(lambda: codec.search(ctx, bt, benc, wide, 10)) == -4                   # PQH_ERR_UNSUPPORTED
    codec.decode_status(ctx)
    # the stream cut to half its whole words
    half = enc.stream.numel() // 4 // 2 * 4
    cut = codec.Encoded(enc.stream[:half], enc.bits, 7, enc.chunk_offsets, enc.chunk_prev, N, 1)
    got = codec.search(ctx, tabs, cut, ld, 64)
    assert _status(lambda: codec.decode_status(ctx)) == -6                                # PQH_ERR_CORRUPT
    gi = got[1].cpu().numpy()
    assert gi.min() >= -1 and gi.max() < N
    # the chunks that lie wholly inside the cut stream are all there is to find
    off = enc.chunk_offsets.cpu().numpy()
    sound = int((off[1:] <= half * 8).sum()) * 7          # rows of the chunks that end inside it
    assert 0 < sound < N
    _check(got, _want(lut, codes[:sound], 64))
    # read once, then clean: a good call on the same context
    _check(codec.search(ctx, tabs, enc, ld, 64), _want(lut, codes, 64))
    codec.decode_status(ctx)


@pytest.fixture(scope="module")
def large(gpu):
    """200,000 rows in chunks of 4: 782 chunk groups, many waves' lists to merge"""
    torch, codec, ctx = gpu
    n = 200_000
    codes = datagen.skewed_codes(n, 8, seed=61, stay=0)
    cd = torch.from_numpy(codes).cuda()
    tabs = codec.Tables(ctx, 8, 256, True).build(codec.histogram(ctx, cd, 256, True))
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=4)
    lut = _lut(8, 8, 62)
    return tabs, enc, torch.from_numpy(lut).cuda(), _want(lut, codes, 64)


def test_large_run(gpu, large):
    torch, codec, ctx = gpu
    tabs, enc, ld, want = large
    _check(codec.search(ctx, tabs, enc, ld, 64), want)
    codec.decode_status(ctx)


def test_large_run_after_lds_poison(gpu, large):
    """every CU's LDS filled with a pattern first: a read of LDS the kernel did not write
    (the window's pad, a stage slot, a table entry) shows as a wrong result"""
    from pq_huffman_amd.capi import lib
    torch, codec, ctx = gpu
    tabs, enc, ld, want = large
    for value in POISON:
        assert lib().pqh_debug_poison_lds(ctx.ptr, ctypes.c_uint(value)) == 0
        _check(codec.search(ctx, tabs, enc, ld, 64), want, hex(value))
    codec.decode_status(ctx)
