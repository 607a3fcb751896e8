"""Probe search: ADC top-k over per-query row ranges of a stream (pqh_search_stream_ranges,
pqh_search_codes_ranges) and the two helpers that make a probe list (ivf_layout, probe_ranges).
Expected values come from numpy in this file -- the distance summed part by part in float32
over the concatenated ranges of a query, the order np.lexsort((ids, dist)) -- never from the
calls under test.  Every comparison is array_equal on the ids and on the raw float bits."""
import ctypes

import numpy as np
import pytest

import datagen

pytestmark = pytest.mark.gpu

N = 1003   # not a multiple of any chunk size below
CHUNKS = [1, 4, 7, 64]
NQ = 9
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
    """the plain search of tests/test_gpu_search.py: the top k of rows [first, n)"""
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


def _csr(per_query):
    """a list of (first, count) lists, one per query -> (range_ptr, ranges) as numpy int64"""
    ptr = np.zeros(len(per_query) + 1, np.int64)
    ptr[1:] = np.cumsum([len(p) for p in per_query])
    flat = [r for p in per_query for r in p]
    return ptr, np.array(flat, np.int64).reshape(len(flat), 2)


def _rows_of(ranges, n):
    """the candidate rows of one query: its good ranges concatenated, bad ones skipped"""
    rows = [np.arange(f, f + c, dtype=np.int64) for f, c in ranges
            if 0 <= f <= n and 0 <= c <= n - f]
    return np.concatenate(rows) if rows else np.zeros(0, np.int64)


def _want_ranges(lut, codes, k, per_query, id_base=0, d=None, keep=None):
    """the top k by (dist, id) of every query's concatenated ranges, padded with (+inf, -1);
    keep: a row -> bool mask of the rows that take part at all"""
    n = codes.shape[0]
    d = _dists(lut, codes) if d is None else d
    wd = np.full((lut.shape[0], k), np.inf, np.float32)
    wi = np.full((lut.shape[0], k), -1, np.int64)
    for q, ranges in enumerate(per_query):
        if ranges is None:      # a query whose range_ptr entries are bad
            continue
        rows = _rows_of(ranges, n)
        if keep is not None:
            rows = rows[keep[rows]]
        dist = d[q, rows]
        order = np.lexsort((rows, dist))[:k]
        wd[q, :len(order)] = dist[order]
        wi[q, :len(order)] = rows[order] + id_base
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


def _dev(torch, ptr, ranges):
    return torch.from_numpy(ptr).cuda(), torch.from_numpy(ranges).cuda()


def _mix(chunk):
    """nine queries, each with its own mix of ranges"""
    C = chunk
    two_steps = (3 * C + C // 2, min(64 * C + 1, N - (3 * C + C // 2)))   # (the stream is shorter
    #                                                                       than 64 * 64 + 1 rows)
    return [
        [(0, N)],                                        # the whole stream
        [(17, 1)],                                       # one row
        [(5, 2)],                                        # inside one chunk, cut at both ends
        [(1, 40)],                                       # chunk 0 decoded, row 0 not scored
        [(N - 30, 30), (5, 2), (1, 1)],                  # ends at N
        [two_steps],                                     # 65 chunks from the middle of one
        [(100, 50), (300, 0), (600, 25)],                # an empty range between two real ones
        [],                                              # no ranges at all
        [(10, 3), (990, 4), two_steps[:1] + (0,)],       # fewer rows than k
    ]


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("mode", list(MODES))
def test_exact_topk_over_ranges(gpu, coded, mode, chunk):
    torch, codec, ctx = gpu
    codes, cd, tabs = coded(mode)
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=chunk)
    lut = _lut(NQ, codes.shape[1], chunk)
    ld = torch.from_numpy(lut).cuda()
    per_query = _mix(chunk)
    assert len(per_query) == NQ
    if chunk < 64:   # 65 chunks, the first and the last one cut
        f, c = per_query[5][0]
        assert c == 64 * chunk + 1 and (f + c - 1) // chunk - f // chunk + 1 == 65
    ptr, ranges = _dev(torch, *_csr(per_query))
    d = _dists(lut, codes)
    for k in (1, 10, 64):
        want = _want_ranges(lut, codes, k, per_query, d=d)
        plain = _want(lut, codes, k)
        assert np.array_equal(want[1][0], plain[1][0]) and np.array_equal(want[0][0], plain[0][0])
        assert (want[1][7] == -1).all() and np.isinf(want[0][7]).all()
        assert (want[1][8] >= 0).sum() == min(k, 7) and 0 not in want[1][3]
        _check(codec.search_ranges(ctx, tabs, enc, ld, ptr, ranges, k), want, k)
    codec.decode_status(ctx)


def test_overlapping_ranges_offer_a_row_twice(gpu, coded):
    torch, codec, ctx = gpu
    codes, cd, tabs = coded("ctx_m8")
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=4)
    lut = _lut(2, 8, 71)
    per_query = [[(100, 50), (130, 40)], [(130, 40), (100, 50), (140, 1)]]   # rows 130..149 shared
    want = _want_ranges(lut, codes, 64, per_query)
    for q in range(2):
        ids, times = np.unique(want[1][q], return_counts=True)
        assert set(ids[times >= 2]) <= set(range(130, 150)) and (times >= 2).any()
    assert (want[1][1] == 140).sum() == 3
    ptr, ranges = _dev(torch, *_csr(per_query))
    ld = torch.from_numpy(lut).cuda()
    _check(codec.search_ranges(ctx, tabs, enc, ld, ptr, ranges, 64), want)
    _check(codec.search_codes_ranges(ctx, cd, ld, ptr, ranges, 64), want)
    codec.decode_status(ctx)


@pytest.mark.parametrize("chunk", [4, 7])
def test_ties_are_decided_by_the_id(gpu, coded, chunk):
    torch, codec, ctx = gpu
    codes, cd, tabs = coded("ctx_m8")
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=chunk)
    lut = _ties_lut(NQ, 8, 5)
    per_query = [[(3 + 11 * q, 150), (500 - 7 * q, 120 + q), (800, 0), (990 - 30 * q, 13 + 30 * q)]
                 for q in range(NQ)]
    want = _want_ranges(lut, codes, 64, per_query)
    d = _dists(lut, codes)   # the 64th distance is shared with candidates that stay outside
    assert any((d[q, _rows_of(per_query[q], N)] == want[0][q, -1]).sum() >
               (want[0][q] == want[0][q, -1]).sum() for q in range(NQ))
    assert all(len(np.unique(want[0][q])) < 16 for q in range(NQ))
    ptr, ranges = _dev(torch, *_csr(per_query))
    _check(codec.search_ranges(ctx, tabs, enc, torch.from_numpy(lut).cuda(), ptr, ranges, 64), want)
    codec.decode_status(ctx)


def test_grid_independence(gpu, coded):
    """one workgroup per query looping over every step, three with uneven spans, the default:
    one query with 16 ranges and one with a single range in the same call"""
    torch, codec, ctx = gpu
    codes, cd, tabs = coded("ctx_m8")
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=1)   # 1,003 chunks: 16 steps in one range
    lut = _ties_lut(2, 8, 6)
    per_query = [[(57 * r + (r * r) % 7, 5 + 37 * (r % 5)) for r in range(16)], [(2, N - 3)]]
    assert all(0 <= f and f + c <= N for p in per_query for f, c in p)
    want = _want_ranges(lut, codes, 64, per_query)
    ptr, ranges = _dev(torch, *_csr(per_query))
    ld = torch.from_numpy(lut).cuda()
    try:
        for g in (1, 3, 0):
            ctx.set_tuning(search_groups=g)
            _check(codec.search_ranges(ctx, tabs, enc, ld, ptr, ranges, 64), want, g)
            _check(codec.search_codes_ranges(ctx, cd, ld, ptr, ranges, 64), want, g)
    finally:
        ctx.set_tuning(search_groups=0)
    codec.decode_status(ctx)


@pytest.mark.parametrize("mode", ["ctx_m8", "noctx_m3"])
def test_search_codes_ranges_equals_search_ranges(gpu, coded, mode):
    torch, codec, ctx = gpu
    codes, cd, tabs = coded(mode)
    m = codes.shape[1]
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=7)
    lut = _lut(NQ, m, 41)
    ld = torch.from_numpy(lut).cuda()
    per_query = _mix(7)
    want = _want_ranges(lut, codes, 64, per_query)
    ptr, ranges = _dev(torch, *_csr(per_query))
    a = codec.search_ranges(ctx, tabs, enc, ld, ptr, ranges, 64)
    b = codec.search_codes_ranges(ctx, cd, ld, ptr, ranges, 64)
    _check(a, want)
    _check(b, want)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    if m % 4:   # rows that do not start on a 4-byte boundary
        off = cd.flatten()[m:].view(N - 1, m)
        per_query = [[(0, N - 1)], [(1, 1)], [(2, 3), (N - 6, 5)], [(300, 301)]]
        ptr, ranges = _dev(torch, *_csr(per_query))
        _check(codec.search_codes_ranges(ctx, off, ld[:4], ptr, ranges, 10),
               _want_ranges(lut[:4], codes[1:], 10, per_query))
    codec.decode_status(ctx)


@pytest.mark.parametrize("mode,chunk", [("ctx_m8", 200), ("noctx_m3", N)])
def test_cut_ranges_over_chunks_too_long_for_a_64_chunk_stage(gpu, coded, mode, chunk):
    torch, codec, ctx = gpu
    codes, cd, tabs = coded(mode)
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=chunk)
    lut = _lut(3, codes.shape[1], chunk)
    per_query = [[(150, 700)], [(1, 10), (399, 2), (N - 1, 1)], [(0, N), (200, 200)]]
    ptr, ranges = _dev(torch, *_csr(per_query))
    _check(codec.search_ranges(ctx, tabs, enc, torch.from_numpy(lut).cuda(), ptr, ranges, 64),
           _want_ranges(lut, codes, 64, per_query))
    codec.decode_status(ctx)


@pytest.mark.parametrize("chunk", [7, 64])
def test_search_ranges_of_a_shard(gpu, coded, chunk):
    """rows [500, N) encoded as a shard (raw_first = 0, the halo row as context), searched
    with id_base = 500 and ranges in the shard's own rows"""
    torch, codec, ctx = gpu
    codes, cd, tabs = coded("ctx_m8")
    enc = codec.encode(ctx, tabs, cd[500:], chunk_vectors=chunk, raw_first=0, prev_row=cd[499])
    lut = _lut(3, 8, 31)
    per_query = [[(0, N - 500)], [(0, 1), (3, 9)], [(100, 300), (N - 500 - 5, 5)]]
    ptr, ranges = _dev(torch, *_csr(per_query))
    want = _want_ranges(lut, codes[500:], 10, per_query, id_base=500)
    plain = _want(lut, codes, 10, id_base=500, first=500)
    assert np.array_equal(want[1][0], plain[1][0])
    got = codec.search_ranges(ctx, tabs, enc, torch.from_numpy(lut).cuda(), ptr, ranges, 10,
                              id_base=500)
    _check(got, want)
    assert int(got[1].min()) >= 500
    codec.decode_status(ctx)


def test_errors(gpu, coded):
    torch, codec, ctx = gpu
    codes, cd, tabs = coded("ctx_m8")
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=7)
    lut = _lut(7, 8, 51)
    ld = torch.from_numpy(lut).cuda()
    ptr, ranges = _dev(torch, *_csr([[(0, N)], [(3, 4)]]))
    out = (torch.empty((2, 65), dtype=torch.float32, device="cuda"),
           torch.empty((2, 65), dtype=torch.int64, device="cuda"))
    for k in (65, 0):
        assert _status(lambda: codec.search_ranges(ctx, tabs, enc, ld[:2], ptr, ranges, k,
                                                   out=out)) == -1                        # PQH_ERR_ARG
        assert _status(lambda: codec.search_codes_ranges(ctx, cd, ld[:2], ptr, ranges, k,
                                                         out=out)) == -1
    # a K = 4096 table set
    big = datagen.skewed_codes(N, 8, k=4096, seed=3)
    bd = torch.from_numpy(big.view(np.int16)).cuda()
    bt = codec.Tables.from_codebooks(
        ctx, codec.Codebooks(codec.counts_to_host(codec.histogram(ctx, bd, 4096, False)), 4096, False))
    benc = codec.encode(ctx, bt, bd, chunk_vectors=7)
    wide = torch.zeros((2, 8, 4096), dtype=torch.float32, device="cuda")
    assert _status(lambda: codec.search_ranges(ctx, bt, benc, wide, ptr, ranges, 10)) == -4   # UNSUPPORTED
    codec.decode_status(ctx)

    # one bad range of each kind among good ones, and bad range_ptr entries: every good range
    # and query still exact
    per_query = [[(10, 50), (-5, 10), (100, 20)],          # first < 0
                 [(10, -3), (200, 30)],                    # count < 0
                 [(N - 10, 20), (300, 5)],                 # first + count > n
                 [(5, 2 ** 62), (400, 10)],                # first + count overflows
                 [(0, N), (N + 1, 0), (N, 0)]]             # first > n; (N, 0) is merely empty
    ptr_h, ranges_h = _csr(per_query)
    nr = ranges_h.shape[0]
    # query 5 reversed (its end before its start), query 6 reaching past nr
    ptr_h = np.concatenate([ptr_h, [nr - 4, nr + 5]]).astype(np.int64)
    ptr, ranges = _dev(torch, ptr_h, ranges_h)
    for fn in (lambda: codec.search_ranges(ctx, tabs, enc, ld, ptr, ranges, 64),
               lambda: codec.search_codes_ranges(ctx, cd, ld, ptr, ranges, 64)):
        got = fn()
        assert _status(lambda: codec.decode_status(ctx)) == -1
        _check(got, _want_ranges(lut, codes, 64, per_query + [None, None]))
    # a reversed query alone flags the error too
    ptr2, ranges2 = _dev(torch, np.array([0, 2, 1], np.int64), np.array([[0, 9], [20, 9]], np.int64))
    got = codec.search_ranges(ctx, tabs, enc, ld[:2], ptr2, ranges2, 10)
    assert _status(lambda: codec.decode_status(ctx)) == -1
    _check(got, _want_ranges(lut[:2], codes, 10, [[(0, 9), (20, 9)], None]))
    # read once, then clean: a good call on the same context
    ptr, ranges = _dev(torch, *_csr([[(0, N)]]))
    _check(codec.search_ranges(ctx, tabs, enc, ld[:1], ptr, ranges, 64),
           _want_ranges(lut[:1], codes, 64, [[(0, N)]]))
    codec.decode_status(ctx)

    # the stream cut to half its whole words: the sound half is searchable
    half = enc.stream.numel() // 4 // 2 * 4
    cut = codec.Encoded(enc.stream[:half], enc.bits, 7, enc.chunk_offsets, enc.chunk_prev, N, 1)
    off = enc.chunk_offsets.cpu().numpy()
    sound = int((off[1:] <= half * 8).sum()) * 7          # rows of the chunks that end inside it
    assert 100 < sound < N - 100
    per_query = [[(0, sound)], [(3, 9), (sound - 40, 40)], [(sound - 1, 1), (1, 1)]]
    ptr, ranges = _dev(torch, *_csr(per_query))
    _check(codec.search_ranges(ctx, tabs, cut, ld[:3], ptr, ranges, 64),
           _want_ranges(lut[:3], codes, 64, per_query))
    codec.decode_status(ctx)
    # a range reaching into the cut half: its sound chunks are all there is to find
    per_query = [[(3, 9), (sound - 40, 40)], [(20, 30), (sound - 20, 200)], [(sound + 70, 10)]]
    ptr, ranges = _dev(torch, *_csr(per_query))
    got = codec.search_ranges(ctx, tabs, cut, ld[:3], ptr, ranges, 64)
    assert _status(lambda: codec.decode_status(ctx)) == -6                                # PQH_ERR_CORRUPT
    _check(got, _want_ranges(lut[:3], codes, 64, per_query, keep=np.arange(N) < sound))
    # CORRUPT before ARG when both happen
    ptr, ranges = _dev(torch, *_csr([[(sound - 20, 200), (-1, 5)]]))
    codec.search_ranges(ctx, tabs, cut, ld[:1], ptr, ranges, 64)
    assert _status(lambda: codec.decode_status(ctx)) == -6
    codec.decode_status(ctx)


def test_empty_inputs(gpu, coded):
    torch, codec, ctx = gpu
    codes, cd, tabs = coded("ctx_m8")
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=4)
    lut = _lut(2, 8, 81)
    ld = torch.from_numpy(lut).cuda()
    # no ranges at all: the padding
    ptr = torch.zeros(3, dtype=torch.int64, device="cuda")
    none = torch.zeros((0, 2), dtype=torch.int64, device="cuda")
    pad = (np.full((2, 10), np.inf, np.float32), np.full((2, 10), -1, np.int64))
    _check(codec.search_ranges(ctx, tabs, enc, ld, ptr, none, 10), pad)
    _check(codec.search_codes_ranges(ctx, cd, ld, ptr, none, 10), pad)
    # no queries: nothing is written
    dist = torch.full((2, 10), 7.0, dtype=torch.float32, device="cuda")
    ids = torch.full((2, 10), 7, dtype=torch.int64, device="cuda")
    one = torch.tensor([[0, 5]], dtype=torch.int64, device="cuda")
    codec.search_ranges(ctx, tabs, enc, ld[:0], ptr[:1], one, 10, out=(dist, ids))
    assert bool((dist == 7.0).all()) and bool((ids == 7).all())
    codec.decode_status(ctx)


def test_ivf_end_to_end(gpu, coded):
    """rows grouped by a list id, encoded in list order, probed three lists a query and the
    ids mapped back: numpy brute force over the original rows whose list is probed (ties are
    broken by the stream row)"""
    torch, codec, ctx = gpu
    codes, cd, _ = coded("ctx_m8")
    nlist = 16
    lists = codes[:, 0].astype(np.int64) % nlist
    perm, offsets = codec.ivf_layout(torch.from_numpy(lists).cuda(), nlist)
    pcd = cd[perm].contiguous()
    tabs = codec.Tables.from_codebooks(
        ctx, codec.Codebooks(codec.counts_to_host(codec.histogram(ctx, pcd, 256, True)), 256, True))
    enc = codec.encode(ctx, tabs, pcd, chunk_vectors=4)
    rng = np.random.default_rng(91)
    probes = np.stack([rng.permutation(nlist)[:3] for _ in range(NQ)]).astype(np.int64)
    probes[np.arange(NQ), np.arange(NQ) % 3] = -1            # one entry of each query probes nothing
    ptr, ranges = codec.probe_ranges(offsets, torch.from_numpy(probes).cuda())
    lut = _ties_lut(NQ, 8, 92)
    got = codec.search_ranges(ctx, tabs, enc, torch.from_numpy(lut).cuda(), ptr, ranges, 64)
    # brute force over the original rows
    perm_h = np.argsort(lists, kind="stable")
    assert np.array_equal(perm.cpu().numpy(), perm_h)
    stream_row = np.empty(N, np.int64)
    stream_row[perm_h] = np.arange(N)
    d = _dists(lut, codes)
    wd = np.full((NQ, 64), np.inf, np.float32)
    ws = np.full((NQ, 64), -1, np.int64)
    wo = np.full((NQ, 64), -1, np.int64)
    for q in range(NQ):
        rows = np.flatnonzero(np.isin(lists, probes[q][probes[q] >= 0]))
        order = np.lexsort((stream_row[rows], d[q, rows]))[:64]
        wd[q, :len(order)] = d[q, rows[order]]
        ws[q, :len(order)] = stream_row[rows[order]]
        wo[q, :len(order)] = rows[order]
    _check(got, (wd, ws))
    mapped = torch.where(got[1] >= 0, perm[got[1].clamp(min=0)], got[1])
    assert np.array_equal(mapped.cpu().numpy(), wo)
    codec.decode_status(ctx)


@pytest.fixture(scope="module")
def large(gpu):
    """200,000 rows in chunks of 4; eight queries with 16 disjoint ranges each of 1 to 20,000
    rows, in no order"""
    torch, codec, ctx = gpu
    n = 200_000
    codes = datagen.skewed_codes(n, 8, seed=61, stay=0)
    cd = torch.from_numpy(codes).cuda()
    tabs = codec.Tables(ctx, 8, 256, True).build(codec.histogram(ctx, cd, 256, True))
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=4)
    lut = _lut(8, 8, 62)
    rng = np.random.default_rng(63)
    per_query = []
    for _ in range(8):
        lens = rng.integers(1, 20_001, size=16)
        while lens.sum() > n:
            lens = rng.integers(1, 20_001, size=16)
        # the slack dealt out as the gaps before the ranges
        cuts = np.sort(rng.integers(0, n - lens.sum() + 1, size=16))
        firsts = cuts + np.concatenate([[0], np.cumsum(lens)[:-1]])
        assert (firsts[1:] >= firsts[:-1] + lens[:-1]).all() and firsts[-1] + lens[-1] <= n
        order = rng.permutation(16)
        per_query.append([(int(firsts[i]), int(lens[i])) for i in order])
    ptr, ranges = _dev(torch, *_csr(per_query))
    want = _want_ranges(lut, codes, 64, per_query)
    return tabs, enc, torch.from_numpy(lut).cuda(), ptr, ranges, want


def test_large_run(gpu, large):
    torch, codec, ctx = gpu
    tabs, enc, ld, ptr, ranges, want = large
    _check(codec.search_ranges(ctx, tabs, enc, ld, ptr, ranges, 64), want)
    codec.decode_status(ctx)


def test_large_run_after_lds_poison(gpu, large):
    """every CU's LDS filled with a pattern first: a read of LDS the kernel did not write
    (the window's pad, a stage slot, a table entry) shows as a wrong result"""
    from pq_huffman_amd.capi import lib
    torch, codec, ctx = gpu
    tabs, enc, ld, ptr, ranges, want = large
    for value in POISON:
        assert lib().pqh_debug_poison_lds(ctx.ptr, ctypes.c_uint(value)) == 0
        _check(codec.search_ranges(ctx, tabs, enc, ld, ptr, ranges, 64), want, hex(value))
    codec.decode_status(ctx)
