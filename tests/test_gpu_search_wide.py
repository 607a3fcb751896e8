"""The wide search on the GPU: top_k and re-rank candidates in (64, 256] on a context whose limit
pqh_ctx_set_search_max_k raised -- every scan form, the merge, the fused re-rank, codec.IVF.
Expected values come from numpy (the references tests/search_wide_ref.py names), never from
the calls under test; every comparison is array_equal on the ids and on the raw float bits.
The tests use a context of their own with the limit at 256; test_the_limit makes another."""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest

import refine_ref as rr
import search_filter_ref as fref
import search_lists_ref as lref
import search_shapes_ref as sref
import search_wide_ref as wref

pytestmark = pytest.mark.gpu

POISON = (0xFFFFFFFF, 0xA5A5A5A5, 0x00000001)
WIDE = wref.WIDE_K


@pytest.fixture(scope="module")
def gpu():
    import torch
    from pq_huffman_amd import codec
    assert torch.cuda.is_available()
    ctx = codec.Context(0).set_search_max_k(WIDE)
    assert ctx.search_max_k == WIDE
    return torch, codec, ctx


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


def _dev(torch, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _encoded(gpu, cd, K, chunk, context):
    """(tables, stream) of device codes, and the decoder's word on them"""
    torch, codec, ctx = gpu
    tabs = codec.Tables(ctx, cd.shape[1], K, context).build(codec.histogram(ctx, cd, K, context))
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=chunk)
    assert torch.equal(codec.decode(ctx, tabs, enc), cd), "the decoder, not the search"
    codec.decode_status(ctx)
    return tabs, enc


def _poison(ctx, value):
    from pq_huffman_amd.capi import lib
    assert lib().pqh_debug_poison_lds(ctx.ptr, ctypes.c_uint(value)) == 0


# ------------------------------------------------------------------------------ 1. the limit
def test_the_limit():
    import torch
    from pq_huffman_amd import codec
    ctx = codec.Context(0)
    assert ctx.search_max_k == 64
    codes = wref.codes_of("ctx_m8")
    cd, ld = _dev(torch, codes, wref.lut_of("ctx_m8", 2, nq=2))
    tabs = codec.Tables(ctx, 8, 256, True).build(codec.histogram(ctx, cd, 256, True))
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=7)
    w = rr.sweep_world(rr.SHAPES[1], 256)
    plain = ((codec.PQ(ctx, w["cent1"]), torch.from_numpy(w["codes1"]).cuda()),
             (codec.PQ(ctx, w["cent2"]), torch.from_numpy(w["codes2"]).cuda()))
    qd = torch.from_numpy(w["q"][:2]).cuda()

    def searches(k):
        return (_status(lambda: codec.search(ctx, tabs, enc, ld, k)),
                _status(lambda: codec.search_codes(ctx, cd, ld, k)))

    def refines(ncand):
        rows = torch.zeros((2, ncand), dtype=torch.int64, device="cuda")
        return _status(lambda: codec.refine(ctx, *plain, qd, rows, 10))

    assert searches(64) == (0, 0) and searches(65) == (-1, -1) and refines(64) == 0 and refines(65) == -1
    assert _status(lambda: ctx.set_search_max_k(63)) == -1 and ctx.search_max_k == 64
    assert _status(lambda: ctx.set_search_max_k(257)) == -1 and ctx.search_max_k == 64
    assert ctx.set_search_max_k(256) is ctx and ctx.search_max_k == 256
    for k in (65, 256):
        assert searches(k) == (0, 0) and refines(k) == 0
        _check(codec.search(ctx, tabs, enc, ld, k), wref.want(wref.lut_of("ctx_m8", 2, nq=2), codes, k), k)
    assert searches(257) == (-1, -1) and refines(257) == -1
    ctx.set_search_max_k(100)
    assert ctx.search_max_k == 100 and searches(100) == (0, 0) and searches(101) == (-1, -1)
    ctx.set_search_max_k(64)
    assert searches(65) == (-1, -1) and refines(65) == -1 and searches(64) == (0, 0)
    codec.decode_status(ctx)


# ------------------------------------------------------------------------------ 2. the whole stream
@functools.lru_cache(maxsize=None)
def _whole(shape):
    codes, lut = wref.codes_of(shape), wref.lut_of(shape, 11)
    return codes, lut, wref.want(lut, codes, WIDE)


@pytest.mark.parametrize("chunk", wref.CHUNKS)
@pytest.mark.parametrize("shape", list(wref.SHAPES))
def test_whole_stream_sweep(gpu, shape, chunk):
    """N = 1,003 rows, nine queries (three batches of four tables, the last part-filled), every
    top_k of the sweep: the stream and the plain codes equal numpy and each other"""
    torch, codec, ctx = gpu
    m, K, context = wref.SHAPES[shape]
    codes, lut, want = _whole(shape)
    cd, ld = _dev(torch, codes, lut)
    tabs, enc = _encoded(gpu, cd, K, chunk, context)
    for k in wref.TOP_KS:
        a = codec.search(ctx, tabs, enc, ld, k)
        b = codec.search_codes(ctx, cd, ld, k)
        _check(a, sref.head(want, k), (k, "stream"))
        _check(b, sref.head(want, k), (k, "codes"))
        _same(torch, a, b, k)
    codec.decode_status(ctx)


@pytest.mark.parametrize("shape", ["ctx_m8", "m12_k16"])
def test_fewer_rows_than_k_and_none(gpu, shape):
    torch, codec, ctx = gpu
    m, K, context = wref.SHAPES[shape]
    codes, lut, _ = _whole(shape)
    n = wref.SHORT_N
    cd, ld = _dev(torch, codes[:n], lut)
    tabs, enc = _encoded(gpu, cd, K, 7, context)
    for k in (128, 255, WIDE):
        want = wref.want(lut, codes[:n], k)
        assert (want[1][:, n:] == -1).all() and (want[1][:, :n] >= 0).all()
        _check(codec.search(ctx, tabs, enc, ld, k), want, k)
        _check(codec.search_codes(ctx, cd, ld, k), want, k)
    pad = (np.full((wref.NQ, WIDE), np.inf, np.float32), np.full((wref.NQ, WIDE), -1, np.int64))
    _check(codec.search_codes(ctx, cd[:0], ld, WIDE), pad)
    _check(codec.search(ctx, tabs, dataclasses.replace(enc, n=0), ld, WIDE), pad)
    codec.decode_status(ctx)


# ------------------------------------------------------------------------------ 3. ties
@pytest.mark.parametrize("chunk", [4, 7])
def test_ties_are_decided_by_the_id(gpu, chunk):
    torch, codec, ctx = gpu
    codes, lut = wref.codes_of("ctx_m8"), wref.ties_lut()
    wref.check_ties(lut, codes)
    want = wref.want(lut, codes, WIDE)
    cd, ld = _dev(torch, codes, lut)
    tabs, enc = _encoded(gpu, cd, 256, chunk, True)
    for k in wref.TOP_KS:
        _check(codec.search(ctx, tabs, enc, ld, k), sref.head(want, k), k)
        _check(codec.search_codes(ctx, cd, ld, k), sref.head(want, k), k)
    codec.decode_status(ctx)


# ------------------------------------------------------------------------------ 4. the offer paths
def _offers(gpu, run):
    torch, codec, ctx = gpu
    codes = wref.offer_codes()
    cd, = _dev(torch, codes)
    src = run(cd)
    try:
        ctx.set_tuning(search_groups=1)
        for top_k, j, order, landing, seed in wref.offer_cases():
            lut, dist = wref.offer_table(top_k, j, order, landing, seed)
            wref.check_offer_case(codes, lut, dist, top_k, j, order, landing)
            ld, = _dev(torch, lut)
            _check(src(ld, top_k), wref.want(lut, codes, top_k), (top_k, j, order, landing))
    finally:
        ctx.set_tuning(search_groups=0)
    codec.decode_status(ctx)


def test_offer_paths_stream(gpu):
    """512 rows in chunks of 8, one workgroup: 64 chunks are one step of one wave, which offers
    its rows 64 at a time in row order -- four offers fill the list, of the fifth and the
    seventh exactly j beat the threshold (ascending, descending, shuffled by lane), landing
    inside the threshold's block, across a block boundary, before everything"""
    torch, codec, ctx = gpu

    def run(cd):
        tabs, enc = _encoded(gpu, cd, 256, 8, True)
        return lambda ld, k: codec.search(ctx, tabs, enc, ld, k)
    _offers(gpu, run)


def test_offer_paths_codes(gpu):
    """512 rows are two steps of search_codes (four rows a lane) for the one wave"""
    torch, codec, ctx = gpu
    _offers(gpu, lambda cd: lambda ld, k: codec.search_codes(ctx, cd, ld, k))


# ------------------------------------------------------------------------------ 5. the grid
def test_grid_independence(gpu):
    """16,700 rows on the ties table at k = 256: one workgroup, three with uneven spans, 17 and
    65 -- more partial lists than adc_merge_wide has waves, and its loop's second round"""
    torch, codec, ctx = gpu
    codes, lut = wref.grid_case()
    wref.check_grid_case(codes, lut)
    want = wref.want(lut, codes, WIDE)
    cd, ld = _dev(torch, codes, lut)
    tabs, enc = _encoded(gpu, cd, 256, wref.GRID_CHUNK, True)
    try:
        for g in wref.GRID_GROUPS + (0,):
            ctx.set_tuning(search_groups=g)
            _check(codec.search(ctx, tabs, enc, ld, WIDE), want, g)
            _check(codec.search_codes(ctx, cd, ld, WIDE), want, g)
            _check(codec.search(ctx, tabs, enc, ld, 200), sref.head(want, 200), g)
    finally:
        ctx.set_tuning(search_groups=0)
    codec.decode_status(ctx)


# ------------------------------------------------------------------------------ 6. the probe forms
@pytest.mark.parametrize("source", ["stream", "codes"])
@pytest.mark.parametrize("m,K", wref.PROBE_SHAPES)
def test_probe_forms(gpu, m, K, source):
    """search_ranges, search_range_tables and search_lists with a table per query and per pair,
    with and without keep=, at k = 65 and 256, over the stream or the codes"""
    torch, codec, ctx = gpu
    case, keep = wref.probe_case(m, K)
    wref.check_probe_case(case, keep)
    codes, offsets, probes, lut_q, lut_pair = case
    cd, lq, lp, od, bd = _dev(torch, codes, lut_q, lut_pair, offsets, probes)
    pd, rd = _dev(torch, *lref.probe_ranges(offsets, probes))
    kd, = _dev(torch, fref.pack(keep))
    src = _encoded(gpu, cd, K, wref.PROBE_CHUNK, True) if source == "stream" else None
    for mask, words in ((None, None), (keep, kd)):
        per_query, per_pair = fref.probe_want(case, mask, WIDE)
        by_lists = lref.search(lut_pair, codes, WIDE, offsets, probes, keep=mask)[:2]
        assert np.array_equal(by_lists[1], per_pair[1])           # the two references agree
        for k in wref.PROBE_KS:
            wq, wp = sref.head(per_query, k), sref.head(per_pair, k)
            what = (k, mask is not None)
            if src is not None:
                tabs, enc = src
                _check(codec.search_ranges(ctx, tabs, enc, lq, pd, rd, k, keep=words), wq, what)
                _check(codec.search_range_tables(ctx, tabs, enc, lp, pd, rd, k, keep=words), wp, what)
                _check(codec.search_lists(ctx, tabs, enc, lq, od, bd, k, keep=words), wq, what)
                _check(codec.search_lists(ctx, tabs, enc, lp, od, bd, k, keep=words), wp, what)
            else:
                _check(codec.search_codes_ranges(ctx, cd, lq, pd, rd, k, keep=words), wq, what)
                _check(codec.search_codes_range_tables(ctx, cd, lp, pd, rd, k, keep=words), wp, what)
                _check(codec.search_codes_lists(ctx, cd, lq, od, bd, k, keep=words), wq, what)
                _check(codec.search_codes_lists(ctx, cd, lp, od, bd, k, keep=words), wp, what)
    codec.decode_status(ctx)


# ------------------------------------------------------------------------------ 7. the re-rank
def _enc2(gpu, codes, k, context, chunk):
    torch, codec, ctx = gpu
    cd = torch.from_numpy(codes).cuda()
    tabs = codec.Tables(ctx, codes.shape[1], k, context).build(codec.histogram(ctx, cd, k, context))
    return tabs, codec.encode(ctx, tabs, cd, chunk_vectors=chunk)


def _streams(gpu, w, pq1, pq2, chunks=(4, 7)):
    """both levels of a K = 256 world as context streams"""
    t1, e1 = _enc2(gpu, w["codes1"], 256, True, chunks[0])
    t2, e2 = _enc2(gpu, w["codes2"], 256, True, chunks[1])
    return (t1, pq1, e1), (t2, pq2, e2)


def _out(torch, nq, k, value):
    def poisoned(dtype):
        t = torch.empty((nq, k), dtype=dtype, device="cuda")
        t.view(torch.int32).fill_(value - (1 << 32) if value >= 1 << 31 else value)
        return t
    return poisoned(torch.float32), poisoned(torch.int64)


@pytest.mark.parametrize("k", rr.KS)
@pytest.mark.parametrize("shape", rr.SHAPES)
def test_refine_stream_equals_codes_equals_numpy(gpu, shape, k):
    """every pair of chunk sizes x nq x (ncand, top_k) with 65 to 256 candidates of
    refine_ref.candidates: padding, a duplicate, chunk-first and chunk-last rows"""
    torch, codec, ctx = gpu
    w = rr.sweep_world(shape, k)
    pq1, pq2 = codec.PQ(ctx, w["cent1"]), codec.PQ(ctx, w["cent2"])
    c1d, c2d, qd = _dev(torch, w["codes1"], w["codes2"], w["q"])
    context = k == 256
    case = 0
    for chunks in rr.CHUNKS:
        t1, e1 = _enc2(gpu, w["codes1"], k, context, chunks[0])
        t2, e2 = _enc2(gpu, w["codes2"], k, context, chunks[1])
        for nq in wref.REFINE_NQS:
            for ncand, top_k in wref.REFINE_CANDS:
                rows = rr.candidates(nq, ncand, chunks, 17 * nq + ncand)
                rr.check_candidates(rows, chunks)
                want = rr.refine(w["q"][:nq], rows, top_k, w["cent1"], w["codes1"], w["cent2"],
                                 w["codes2"])
                rd, = _dev(torch, rows)
                value = POISON[case % 3]
                case += 1
                a = codec.refine(ctx, (pq1, c1d), (pq2, c2d), qd[:nq], rd, top_k,
                                 out=_out(torch, nq, top_k, value))
                b = codec.refine(ctx, (t1, pq1, e1), (t2, pq2, e2), qd[:nq], rd, top_k,
                                 out=_out(torch, nq, top_k, value))
                _check(a, want, (chunks, nq, ncand, top_k, "codes"))
                _check(b, want, (chunks, nq, ncand, top_k, "streams"))
                _same(torch, a, b)
    codec.decode_status(ctx)                              # -1 and a duplicate are no errors


@pytest.mark.parametrize("d", [15, 128])
def test_refine_residual_form_and_a_bad_row(gpu, d):
    """200 candidates over 37 lists, several empty; then a row outside [0, n): dropped and
    reported"""
    torch, codec, ctx = gpu
    w = rr.residual_world(d)
    rows = wref.residual_rows(w)
    wref.check_residual_rows(w, rows)
    pq1, pq2 = codec.PQ(ctx, w["cent1"]), codec.PQ(ctx, w["cent2"])
    plain = ((pq1, torch.from_numpy(w["codes1"]).cuda()), (pq2, torch.from_numpy(w["codes2"]).cuda()))
    streams = _streams(gpu, w, pq1, pq2)
    cq = codec.Coarse(ctx, w["coarse"])
    qd, od = _dev(torch, w["q"], w["offsets"])
    codec.decode_status(ctx)
    bad = rows.copy()
    bad[1, 130], bad[3, 5] = rr.N, 2 ** 40
    for cand, status in ((rows, 0), (bad, -1)):
        rd, = _dev(torch, cand)
        for k in (1, 10, cand.shape[1]):
            want = rr.refine(w["q"], cand, k, w["cent1"], w["codes1"], w["cent2"], w["codes2"],
                             w["coarse"], w["offsets"])
            for levels in (streams, plain):
                got = codec.refine(ctx, *levels, qd, rd, k, coarse=cq, offsets=od,
                                   out=_out(torch, 5, k, POISON[k % 3]))
                _check(got, want, (d, k, status))
                assert _status(lambda: codec.decode_status(ctx)) == status        # PQH_ERR_ARG
    codec.decode_status(ctx)
    cq.close()


# ------------------------------------------------------------------------------ 8. the index
@pytest.mark.parametrize("kind", ["plain", "residual"])
def test_ivf_wide(gpu, kind):
    torch, codec, ctx = gpu
    w = fref.ivf_world()
    wref.check_ivf_world(w)
    r2 = rr.ivf_refine_world(w, kind)
    xd, qd = _dev(torch, w["x"], w["q"])
    pq, pq2, coarse = codec.PQ(ctx, w["cent"]), codec.PQ(ctx, r2["cent2"]), codec.Coarse(ctx, w["cc"])
    res = kind == "residual"
    ivf = codec.IVF.build(ctx, pq, coarse, xd, chunk_vectors=4, residual=res, refine_pq=pq2,
                          refine_chunk_vectors=7)
    codec.ivf_status(ctx)
    nprobe, perm = fref.IVF_NPROBE, w["perm"]

    @functools.lru_cache(maxsize=None)
    def cands(kept, removed):
        return rr.ivf_candidates(w, kind, WIDE, w["keep"] if kept else None,
                                 None if removed is None else np.array(removed))

    def want(k, refine, kept=False, removed=None):
        wd, cand = cands(kept, removed)
        if refine:
            wd, rows = rr.ivf_refined(w, kind, r2, cand[:, :refine], k)
        else:
            wd, rows = wd[:, :k], cand[:, :k]
        return wd, np.where(rows >= 0, perm[np.maximum(rows, 0)], -1)

    keep, = _dev(torch, w["keep"])
    assert (want(WIDE, 0)[1] >= 0).all() and (want(WIDE, 0, kept=True)[1][:, -1] == -1).all()

    def sweep(removed, tag):
        for schedule in ("query", "list"):
            for k, refine in wref.IVF_KS:
                for kept in (False, True):
                    got = ivf.search(qd, nprobe, k, schedule=schedule, refine=refine,
                                     keep=keep if kept else None)
                    _check(got, want(k, refine, kept, removed), (schedule, k, refine, kept, tag))
    sweep(None, "")
    if res:                                               # slab by slab
        ivf.table_budget = 2 * nprobe * fref.IVF_M * 256 * 4
        for k, refine in wref.IVF_KS:
            _check(ivf.search(qd, nprobe, k, refine=refine), want(k, refine), ("slabs", k, refine))
        del ivf.table_budget
    assert _status(lambda: ivf.search(qd, nprobe, 10, refine=257)) == -1
    assert _status(lambda: ivf.search(qd, nprobe, 257)) == -1
    first = tuple(int(v) for v in want(10, 256)[1][0])
    ivf.remove(torch.tensor(first, device="cuda"))
    sweep(first, "removed")
    got = ivf.search(qd, nprobe, WIDE, refine=WIDE)
    assert not np.isin(got[1].cpu().numpy(), first).any()
    codec.decode_status(ctx)
    codec.ivf_status(ctx)
    for h in (pq2, coarse, pq):
        h.close()


# ------------------------------------------------------------------------------ 9. a cut stream
def test_a_cut_stream(gpu):
    torch, codec, ctx = gpu
    codes, lut, _ = _whole("ctx_m8")
    lut = lut[:2]
    cd, ld = _dev(torch, codes, lut)
    tabs, enc = _encoded(gpu, cd, 256, 7, True)
    half = enc.stream.numel() // 4 // 2 * 4
    cut = codec.Encoded(enc.stream[:half], enc.bits, 7, enc.chunk_offsets, enc.chunk_prev, wref.N, 1)
    got = codec.search(ctx, tabs, cut, ld, WIDE)
    assert _status(lambda: codec.decode_status(ctx)) == -6                                # PQH_ERR_CORRUPT
    gi = got[1].cpu().numpy()
    assert gi.min() >= -1 and gi.max() < wref.N
    off = enc.chunk_offsets.cpu().numpy()
    sound = int((off[1:] <= half * 8).sum()) * 7          # rows of the chunks that end inside it
    assert WIDE < sound < wref.N
    _check(got, wref.want(lut, codes[:sound], WIDE))
    _check(codec.search(ctx, tabs, enc, ld, WIDE), wref.want(lut, codes, WIDE))
    codec.decode_status(ctx)                              # read once, then clean


# ------------------------------------------------------------------------------ 10. stale LDS
def test_after_lds_poison(gpu):
    """the end-of-kernel exchange of the wide lists reuses the tables' and the stages' LDS, and
    the wide re-rank hands its keys through LDS: each equal to the unpoisoned result"""
    torch, codec, ctx = gpu
    codes, lut = wref.grid_case()
    want = wref.want(lut, codes, WIDE)
    cd, ld = _dev(torch, codes, lut)
    tabs, enc = _encoded(gpu, cd, 256, wref.GRID_CHUNK, True)
    case, _ = wref.probe_case(8, 256)
    pcodes, offsets, probes, lut_q, lut_pair = case
    pcd, lq, lp, od, bd = _dev(torch, pcodes, lut_q, lut_pair, offsets, probes)
    ptabs, penc = _encoded(gpu, pcd, 256, wref.PROBE_CHUNK, True)
    per_query, per_pair = fref.probe_want(case, None, WIDE)
    w = rr.sweep_world(rr.SHAPES[1], 256)
    pq1, pq2 = codec.PQ(ctx, w["cent1"]), codec.PQ(ctx, w["cent2"])
    levels = _streams(gpu, w, pq1, pq2)
    rows = rr.candidates(5, WIDE, (4, 7), 9)
    rwant = rr.refine(w["q"], rows, WIDE, w["cent1"], w["codes1"], w["cent2"], w["codes2"])
    qd, rd = _dev(torch, w["q"], rows)
    for value in POISON:
        _poison(ctx, value)
        _check(codec.search(ctx, tabs, enc, ld, WIDE), want, hex(value))
        _poison(ctx, value)
        _check(codec.search_lists(ctx, ptabs, penc, lq, od, bd, WIDE), per_query, hex(value))
        _poison(ctx, value)
        _check(codec.search_lists(ctx, ptabs, penc, lp, od, bd, WIDE), per_pair, hex(value))
        _poison(ctx, value)
        _check(codec.refine(ctx, *levels, qd, rd, WIDE), rwant, hex(value))
    codec.decode_status(ctx)
