"""The list-major probe search on the GPU: pqh_search_stream_lists, pqh_search_codes_lists and
codec.IVF.search(schedule="list" / "auto").  Expected values come from numpy
(tests/search_lists_ref.py, which tests/test_search_lists_cpu.py pins to the definition of the
probe search), never from the calls under test: floats are compared on their raw bits, ids with
array_equal -- and every result is also the range calls' on the same inputs."""
import ctypes

import numpy as np
import pytest

import datagen
import ivf_ref
import ivf_residual_ref as ref
import search_lists_ref as lref

pytestmark = pytest.mark.gpu

POISON = (0xFFFFFFFF, 0xA5A5A5A5, 0x00000001)   # (the patterns of tests/test_gpu_search.py)
NPROBE = lref.NPROBE


@pytest.fixture(scope="module")
def gpu():
    import torch
    from pq_huffman_amd import codec
    assert torch.cuda.is_available()
    return torch, codec, codec.Context(0)


def _bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


def _status(fn):
    from pq_huffman_amd.capi import PqhError
    try:
        fn()
    except PqhError as err:
        return err.status
    return 0


def _check(got, want, what=""):
    gd, gi = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert gd.dtype == np.float32 and gi.dtype == np.int64
    assert np.array_equal(gi, want[1]), what
    assert np.array_equal(_bits(gd), _bits(want[0])), what


def _same(torch, a, b, what=""):
    assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)), what


def _first(want, k):
    """the result for a smaller k is the head of every row (the order is total)"""
    return want[0][:, :k], want[1][:, :k]


def _encoded(gpu, codes, chunk, context=True):
    torch, codec, ctx = gpu
    cd = torch.from_numpy(codes).cuda()
    m = codes.shape[1]
    tabs = codec.Tables(ctx, m, 256, context).build(codec.histogram(ctx, cd, 256, context))
    return cd, tabs, codec.encode(ctx, tabs, cd, chunk_vectors=chunk)


# ------------------------------------------------------------------------------ the sweep
@pytest.mark.parametrize("m", [8, 16, 3])
@pytest.mark.parametrize("chunk", [1, 7, 64])
@pytest.mark.parametrize("context", [True, False])
def test_lists_sweep(gpu, context, chunk, m):
    """the stream and the codes form, a table per query and one per pair, k in {1, 10, 64},
    one workgroup row per unit, three, 64 (most of them without a step) and the default"""
    torch, codec, ctx = gpu
    codes, offsets, probes, lut_q, lut_pair = lref.sweep_case(m, chunk, 100 * m + chunk)
    lref.check_sweep_inputs(chunk, offsets, probes, m)
    cd, tabs, enc = _encoded(gpu, codes, chunk, context)
    od, pd = torch.from_numpy(offsets).cuda(), torch.from_numpy(probes).cuda()
    ptr, ranges = lref.probe_ranges(offsets, probes)
    rpd, rd = torch.from_numpy(ptr).cuda(), torch.from_numpy(ranges).cuda()
    for lut in (lut_q, lut_pair):
        ld = torch.from_numpy(lut).cuda()
        w64 = lref.search(lut, codes, 64, offsets, probes)[:2]
        assert (w64[1][5] == -1).all() and (w64[1][3] == -1).all() and (w64[1][2] >= 0).sum() == 1
        if lut is lut_pair:
            assert np.isnan(lut[ranges[:, 1] == 0]).all() and not np.isnan(w64[0]).any()
        # a stale or mis-indexed table (every pair scored with its predecessor's) would show
        stale = lref.search(np.nan_to_num(np.roll(lut, 1, axis=0), nan=1e9), codes, 64, offsets, probes)
        assert not np.array_equal(stale[1][0], w64[1][0]) and not np.array_equal(stale[1][4], w64[1][4])
        try:
            for g in (1, 3, 64, 0):
                ctx.set_tuning(search_groups=g)
                for k in (1, 10, 64):
                    want = _first(w64, k)
                    _check(codec.search_lists(ctx, tabs, enc, ld, od, pd, k), want, (g, k, "stream"))
                    _check(codec.search_codes_lists(ctx, cd, ld, od, pd, k), want, (g, k, "codes"))
        finally:
            ctx.set_tuning(search_groups=0)
        # the range calls on the same inputs
        if lut is lut_q:
            a = codec.search_ranges(ctx, tabs, enc, ld, rpd, rd, 64)
            b = codec.search_codes_ranges(ctx, cd, ld, rpd, rd, 64)
        else:
            a = codec.search_range_tables(ctx, tabs, enc, ld, rpd, rd, 64)
            b = codec.search_codes_range_tables(ctx, cd, ld, rpd, rd, 64)
        _check(a, w64)
        _check(b, w64)
        _same(torch, codec.search_lists(ctx, tabs, enc, ld, od, pd, 64), a)
        # id_base, and an out pair to fill
        out = (torch.empty((lref.NQ, 10), dtype=torch.float32, device="cuda"),
               torch.empty((lref.NQ, 10), dtype=torch.int64, device="cuda"))
        got = codec.search_lists(ctx, tabs, enc, ld, od, pd, 10, id_base=1000, out=out)
        assert got[0] is out[0]
        _check(got, lref.search(lut, codes, 10, offsets, probes, id_base=1000)[:2])
    codec.decode_status(ctx)


def test_lists_on_the_default_grid_of_a_larger_index(gpu):
    """20,011 rows in chunks of 4 as 37 lists of very unequal size, 70 queries of 5 probes:
    more units than one per list, lists of one step and of many, both table forms"""
    torch, codec, ctx = gpu
    n, m, nlist, nq, nprobe = 20_011, 8, 37, 70, 5
    rng = np.random.default_rng(63)
    codes = datagen.skewed_codes(n, m, seed=61, stay=0)
    cuts = np.sort(rng.choice(np.arange(400, n), size=nlist - 1, replace=False))
    cuts[:8] = np.arange(1, 9) * 37                        # some lists shorter than a step
    cuts[20] = cuts[19]                                    # and an empty one
    offsets = np.concatenate([[0], np.sort(cuts), [n]]).astype(np.int64)
    sizes = np.diff(offsets)
    assert sizes.max() > 40 * sizes[sizes > 0].min() and (sizes == 0).sum() == 1
    probes = np.stack([rng.permutation(nlist)[:nprobe] for _ in range(nq)])
    probes[:, 3] = np.arange(nq) % 8                       # every query a short list too
    probes[::7, 1] = int(np.argmax(sizes))                 # the longest list ten times
    cd, tabs, enc = _encoded(gpu, codes, 4)
    od, pd = torch.from_numpy(offsets).cuda(), torch.from_numpy(probes).cuda()
    ptr, ranges = lref.probe_ranges(offsets, probes)
    rpd, rd = torch.from_numpy(ptr).cuda(), torch.from_numpy(ranges).cuda()
    for tables in (nq, nq * nprobe):
        lut = rng.normal(0.0, 100.0, size=(tables, m, 256)).astype(np.float32)
        ld = torch.from_numpy(lut).cuda()
        wd, wi, units = lref.search(lut, codes, 64, offsets, probes)
        assert units > nlist
        got = codec.search_lists(ctx, tabs, enc, ld, od, pd, 64)
        _check(got, (wd, wi))
        _check(codec.search_codes_lists(ctx, cd, ld, od, pd, 64), (wd, wi))
        fn = codec.search_ranges if tables == nq else codec.search_range_tables
        _same(torch, got, fn(ctx, tabs, enc, ld, rpd, rd, 64))
    codec.decode_status(ctx)


def test_lists_after_lds_poison(gpu):
    """every CU's LDS filled with a pattern first: a table entry or a stage slot read before
    it was written shows as a wrong result"""
    from pq_huffman_amd.capi import lib
    torch, codec, ctx = gpu
    codes, offsets, probes, lut_q, lut_pair = lref.sweep_case(8, 7, 5)
    cd, tabs, enc = _encoded(gpu, codes, 7)
    od, pd, ld = (torch.from_numpy(a).cuda() for a in (offsets, probes, lut_pair))
    want = lref.search(lut_pair, codes, 64, offsets, probes)[:2]
    for value in POISON:
        assert lib().pqh_debug_poison_lds(ctx.ptr, ctypes.c_uint(value)) == 0
        _check(codec.search_lists(ctx, tabs, enc, ld, od, pd, 64), want, hex(value))
        assert lib().pqh_debug_poison_lds(ctx.ptr, ctypes.c_uint(value)) == 0
        _check(codec.search_codes_lists(ctx, cd, ld, od, pd, 64), want, hex(value))
    codec.decode_status(ctx)


# ------------------------------------------------------------------------------ errors
def test_lists_errors(gpu):
    """bad probes and a bad offsets pair are skipped and reported, every other query exact; the
    sound half of a stream cut in two is searchable without an error"""
    from pq_huffman_amd.capi import lib
    torch, codec, ctx = gpu
    n, m, chunk, nlist = 1003, 8, 7, 6
    codes = datagen.skewed_codes(n, m, seed=108)
    cd, tabs, enc = _encoded(gpu, codes, chunk)
    offsets = np.array([0, 100, 100, 350, 600, 900, n], np.int64)
    good = np.array([[0, 3, 5], [2, 4, 1], [5, -1, 0], [3, 3, 2]], np.int64)
    rng = np.random.default_rng(51)
    lut = rng.normal(0.0, 100.0, size=(12, m, 256)).astype(np.float32)
    ld, od = torch.from_numpy(lut).cuda(), torch.from_numpy(offsets).cuda()
    clean = lref.search(lut, codes, 64, offsets, good)[:2]
    _check(codec.search_lists(ctx, tabs, enc, ld, od, torch.from_numpy(good).cuda(), 64), clean)
    codec.decode_status(ctx)
    # a probe of nlist and one of -2: no rows from them, the other queries as they were
    broken = good.copy()
    broken[1, 1], broken[3, 0] = nlist, -2
    assert lref.invert(offsets, broken, n)[1]
    want = lref.search(lut, codes, 64, offsets, broken)[:2]
    assert np.array_equal(want[1][[0, 2]], clean[1][[0, 2]])
    assert not np.array_equal(want[1][1], clean[1][1])
    bd = torch.from_numpy(broken).cuda()
    for fn in (lambda: codec.search_lists(ctx, tabs, enc, ld, od, bd, 64),
               lambda: codec.search_codes_lists(ctx, cd, ld, od, bd, 64)):
        got = fn()
        assert _status(lambda: codec.decode_status(ctx)) == -1                  # PQH_ERR_ARG
        _check(got, want)
    codec.decode_status(ctx)                                                    # read once, then clean
    # a reversed offsets pair of a probed list (list 3: [600, 350)), and one past n (list 5)
    for at, value in ((3, 700), (6, n + 1)):
        rev = offsets.copy()
        rev[at] = value
        want = lref.search(lut, codes, 64, rev, good)[:2]
        assert lref.invert(rev, good, n)[1]
        rvd = torch.from_numpy(rev).cuda()
        gd = torch.from_numpy(good).cuda()
        for fn in (lambda: codec.search_lists(ctx, tabs, enc, ld, rvd, gd, 64),
                   lambda: codec.search_codes_lists(ctx, cd, ld, rvd, gd, 64)):
            got = fn()
            assert _status(lambda: codec.decode_status(ctx)) == -1
            _check(got, want, (at, value))
    # a bad pair of a list nobody probes is nobody's error
    rev = offsets.copy()
    rev[1] = 50
    rev[2] = 40                                            # list 1 = [50, 40)
    only = np.array([[3, 4, 5], [5, -1, 3]], np.int64)
    _check(codec.search_lists(ctx, tabs, enc, ld[:6], torch.from_numpy(rev).cuda(),
                              torch.from_numpy(only).cuda(), 64),
           lref.search(lut[:6], codes, 64, rev, only)[:2])
    codec.decode_status(ctx)

    # the argument checks
    gd = torch.from_numpy(good).cuda()
    out = (torch.empty((4, 65), dtype=torch.float32, device="cuda"),
           torch.empty((4, 65), dtype=torch.int64, device="cuda"))
    for k in (65, 0):
        assert _status(lambda: codec.search_lists(ctx, tabs, enc, ld, od, gd, k, out=out)) == -1
        assert _status(lambda: codec.search_codes_lists(ctx, cd, ld, od, gd, k, out=out)) == -1
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    L = lib()

    def codes_call(nl=nlist, nq=4, nprobe=3, off=p(od), pr=p(gd), lt=p(ld), mm=m, kk=256, nn=n):
        return L.pqh_search_codes_lists(ctx.ptr, p(cd), nn, mm, kk, off, nl, pr, nq, nprobe, lt, 1,
                                        10, 0, p(out[0]), p(out[1]))

    def stream_call(nl=nlist, nq=4, nprobe=3, off=p(od), pr=p(gd), lt=p(ld), tp=tabs.ptr):
        return L.pqh_search_stream_lists(ctx.ptr, tp, p(enc.stream), enc.stream.numel(), n, 1,
                                         chunk, p(enc.chunk_offsets), p(enc.chunk_prev), off, nl,
                                         pr, nq, nprobe, lt, 1, 10, 0, p(out[0]), p(out[1]))

    assert codes_call() == 0 and stream_call() == 0
    for call in (codes_call, stream_call):
        assert call(nl=0) == -1 and call(nprobe=0) == -1 and call(nq=-1) == -1
        assert call(off=None) == -1 and call(pr=None) == -1 and call(lt=None) == -1
        assert call(nq=1 << 20, nprobe=1 << 11) == -4                           # 2^31 pairs
        assert call(nq=(1 << 31) - 1, nprobe=2) == -4
    assert stream_call(tp=None) == -1
    assert codes_call(mm=0) == -1 and codes_call(nn=-1) == -1
    assert codes_call(mm=17) == -4 and codes_call(kk=257) == -4                 # PQH_ERR_UNSUPPORTED
    codec.decode_status(ctx)

    # empty inputs: no query, no row, no probe that is a list -- the padding
    none = codec.search_lists(ctx, tabs, enc, ld[:0], od, gd[:0], 10)
    assert none[0].shape == (0, 10) and none[1].shape == (0, 10)
    pad = (np.full((4, 10), np.inf, np.float32), np.full((4, 10), -1, np.int64))
    zero = torch.zeros(nlist + 1, dtype=torch.int64, device="cuda")
    _check(codec.search_codes_lists(ctx, cd[:0], ld, zero, gd, 10), pad)
    minus = torch.full((4, 3), -1, dtype=torch.int64, device="cuda")
    _check(codec.search_lists(ctx, tabs, enc, ld, od, minus, 10), pad)
    _check(codec.search_codes_lists(ctx, cd, ld, od, minus, 10), pad)
    codec.decode_status(ctx)

    # the stream cut to half its whole words
    half = enc.stream.numel() // 4 // 2 * 4
    cut = codec.Encoded(enc.stream[:half], enc.bits, chunk, enc.chunk_offsets, enc.chunk_prev, n, 1)
    off = enc.chunk_offsets.cpu().numpy()
    sound = int((off[1:] <= half * 8).sum()) * chunk      # rows of the chunks that end inside it
    assert 100 < sound < n - 250
    offsets = np.array([0, 50, sound - 40, sound - 20, sound + 180, n], np.int64)
    od = torch.from_numpy(offsets).cuda()
    probes = np.array([[0, 1, 2], [2, -1, 1], [1, 0, -1], [2, 2, 0]], np.int64)
    _check(codec.search_lists(ctx, tabs, cut, ld, od, torch.from_numpy(probes).cuda(), 64),
           lref.search(lut, codes, 64, offsets, probes)[:2])
    codec.decode_status(ctx)
    # lists reaching into the cut half: their sound chunks are all there is to find
    probes = np.array([[0, 3, 2], [4, -1, 1], [1, 0, -1], [3, 4, 0]], np.int64)
    got = codec.search_lists(ctx, tabs, cut, ld, od, torch.from_numpy(probes).cuda(), 64)
    assert _status(lambda: codec.decode_status(ctx)) == -6                      # PQH_ERR_CORRUPT
    _check(got, lref.search(lut, codes, 64, offsets, probes, keep=np.arange(n) < sound)[:2])
    codec.decode_status(ctx)


# ------------------------------------------------------------------------------ end to end
N, NL, M, NQ = 1003, 13, 8, 9


@pytest.fixture(scope="module")
def world(gpu):
    """x with 50 rows twice, a 13-list coarse codebook, an 8 x 256 PQ trained on the
    residuals, nine queries near rows of x (the world of tests/test_gpu_ivf_residual.py)"""
    torch, codec, ctx = gpu
    x = datagen.sift_like(N, 128, seed=31)
    x[900:950] = x[100:150]
    rng = np.random.default_rng(32)
    cc = (x[rng.choice(N, NL, replace=False)] + np.float32(0.5)).astype(np.float32)
    lists, _ = ivf_ref.assign(x, cc)
    perm, offsets = ivf_ref.layout(lists, NL)
    res, bad = ref.residuals(x, cc, lists, perm)
    assert not bad.any()
    cent = datagen.lloyd_centroids(res, M, 256, iters=2, sample=N)
    q = (x[[100, 101, 120, 149, 7, 300, 555, 800, 1002]] +
         rng.normal(0.0, 3.0, size=(NQ, 128))).astype(np.float32)
    return dict(x=x, cc=cc, cent=cent, q=q, perm=perm, offsets=offsets, res=res,
                cdist=ivf_ref.dists(q, cc), xd=torch.from_numpy(x).cuda(),
                qd=torch.from_numpy(q).cuda(), pq=codec.PQ(ctx, cent), coarse=codec.Coarse(ctx, cc))


@pytest.mark.parametrize("residual", [False, True])
def test_ivf_list_schedule_gives_the_bits_of_the_query_schedule(gpu, world, residual, monkeypatch):
    torch, codec, ctx = gpu
    w = world
    ivf = codec.IVF.build(ctx, w["pq"], w["coarse"], w["xd"], chunk_vectors=7, residual=residual)
    codec.ivf_status(ctx)
    calls = []
    inner = codec.search_lists
    monkeypatch.setattr(codec, "search_lists", lambda *a, **kw: calls.append(1) or inner(*a, **kw))
    codes = codec.decode(ctx, ivf.tables, ivf.enc).cpu().numpy()
    for nprobe in (1, 4, 16):                                   # (16 > 13 lists: padding)
        # numpy, from the queries on: the probes, the tables, the list-major search
        _, _, probes, _ = ivf_ref.probe(w["q"], w["cc"], nprobe, w["offsets"], w["cdist"])
        if residual:
            lut = ref.tables(w["q"], w["cc"], probes, w["cent"])
            if nprobe == 1:
                lut = lut[:NQ]
        else:
            lut = np.stack([np.stack([ivf_ref.dists(w["q"][qi:qi + 1, i * 16:(i + 1) * 16], w["cent"][i])[0]
                                      for i in range(M)]) for qi in range(NQ)])
        for k in (1, 10, 64):
            wd, rows, _ = lref.search(lut, codes, k, w["offsets"], probes)
            wi = np.where(rows >= 0, w["perm"][np.maximum(rows, 0)], -1)
            before = len(calls)
            by_query = ivf.search(w["qd"], nprobe, k)
            assert len(calls) == before
            by_list = ivf.search(w["qd"], nprobe, k, schedule="list")
            assert len(calls) == before + 1
            _check(by_list, (wd, wi), (nprobe, k))
            _same(torch, by_list, by_query, (nprobe, k))
            _same(torch, ivf.search(w["qd"], nprobe, k, schedule="query"), by_query)
    codec.decode_status(ctx)
    codec.ivf_status(ctx)

    one = ivf.search(w["qd"], 4, 10)
    if residual:
        # three slabs give what one gives
        ivf.table_budget = 3 * 4 * M * 256 * 4                  # the tables of three queries
        before = len(calls)
        three = ivf.search(w["qd"], 4, 10, schedule="list")
        assert len(calls) == before + 3
        del ivf.table_budget
        _same(torch, three, one)

    # auto: on both sides of the ratio (9 queries * 4 probes = 36 pairs, 13 lists)
    assert codec.IVF.list_major_ratio > 0
    for ratio, by_list in ((2.75, True), (2.8, False), (0.5, True), (float("inf"), False)):
        ivf.list_major_ratio = ratio
        before = len(calls)
        _same(torch, ivf.search(w["qd"], 4, 10, schedule="auto"), one, ratio)
        assert (len(calls) > before) == by_list, ratio
    del ivf.list_major_ratio
    assert ivf.list_major_ratio == codec.IVF.list_major_ratio
    assert _status(lambda: ivf.search(w["qd"], 4, 10, schedule="lists")) == -1
    codec.decode_status(ctx)
    codec.ivf_status(ctx)
