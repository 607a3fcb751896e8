"""The refinement codes on the GPU: pqh_refine_stream and pqh_refine_codes (codec.refine), and
codec.IVF built with refine_pq from vectors and queries to re-ranked neighbour ids.  Expected
values come from numpy (tests/refine_ref.py), never from the calls under test: floats are
compared on their raw bits, ids with array_equal."""
import numpy as np
import pytest

import refine_ref as rr
import search_filter_ref as fref

pytestmark = pytest.mark.gpu

POISON = (0xFFFFFFFF, 0xA5A5A5A5, 0x00000001)   # (the patterns of tests/test_gpu_ivf_residual.py)


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


def _poisoned(torch, shape, dtype, value):
    """a device tensor whose every 32-bit word is `value`"""
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.int32).fill_(value - (1 << 32) if value >= 1 << 31 else value)
    return t


def _out(torch, nq, k, value):
    return (_poisoned(torch, (nq, k), torch.float32, value),
            _poisoned(torch, (nq, k), torch.int64, value))


def _check(got, want, what=""):
    gd, gi = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert gd.dtype == np.float32 and gi.dtype == np.int64
    assert np.array_equal(gi, want[1]), what
    assert np.array_equal(_bits(gd), _bits(want[0])), what


def _encode(gpu, codes, k, context, chunk):
    """(tables, enc) of host codes"""
    torch, codec, ctx = gpu
    cd = torch.from_numpy(codes).cuda()
    tabs = codec.Tables(ctx, codes.shape[1], k, context).build(codec.histogram(ctx, cd, k, context))
    return tabs, codec.encode(ctx, tabs, cd, chunk_vectors=chunk)


def _levels(gpu, w, k=256, context=(True, True), chunks=(4, 7)):
    """the two levels of a world as streams and as plain codes"""
    torch, codec, ctx = gpu
    pq1, pq2 = codec.PQ(ctx, w["cent1"]), codec.PQ(ctx, w["cent2"])
    t1, e1 = _encode(gpu, w["codes1"], k, context[0], chunks[0])
    t2, e2 = _encode(gpu, w["codes2"], k, context[1], chunks[1])
    plain = ((pq1, torch.from_numpy(w["codes1"]).cuda()), (pq2, torch.from_numpy(w["codes2"]).cuda()))
    return ((t1, pq1, e1), (t2, pq2, e2)), plain


def _want(w, rows, k, residual=False):
    return rr.refine(w["q"][:rows.shape[0]], rows, k, w["cent1"], w["codes1"], w["cent2"],
                     w["codes2"], w["coarse"] if residual else None,
                     w["offsets"] if residual else None)


# ------------------------------------------------------------------------------ the sweep
@pytest.mark.parametrize("k", rr.KS)
@pytest.mark.parametrize("shape", rr.SHAPES)
def test_stream_equals_codes_equals_numpy(gpu, shape, k):
    """every pair of chunk sizes x context on or off per level x nq x (ncand, top_k); the
    candidates of rr.candidates: the raw row, the last row, chunk ends, a duplicate, -1s.
    (Context coding exists at K = 256 only -- pqh_tables_alloc refuses it otherwise -- so the
    K = 16 streams are coded without.)"""
    torch, codec, ctx = gpu
    w = rr.sweep_world(shape, k)
    pq1, pq2 = codec.PQ(ctx, w["cent1"]), codec.PQ(ctx, w["cent2"])
    c1d, c2d = torch.from_numpy(w["codes1"]).cuda(), torch.from_numpy(w["codes2"]).cuda()
    qd = torch.from_numpy(w["q"]).cuda()
    contexts = (True, False) if k == 256 else (False,)
    streams = {}
    for level, codes in ((1, w["codes1"]), (2, w["codes2"])):
        for chunk in {c[level - 1] for c in rr.CHUNKS}:
            for context in contexts:
                streams[level, chunk, context] = _encode(gpu, codes, k, context, chunk)
    codec.decode_status(ctx)
    case = 0
    for chunks in rr.CHUNKS:
        for nq in rr.NQS:
            for ncand, top_k in rr.CANDS:
                rows = rr.candidates(nq, ncand, chunks, 17 * nq + ncand)
                rr.check_candidates(rows, chunks)
                want = _want(w, rows, top_k)
                assert np.isfinite(want[0][:, 0]).all()
                rd = torch.from_numpy(rows).cuda()
                value = POISON[case % 3]
                case += 1
                got = codec.refine(ctx, (pq1, c1d), (pq2, c2d), qd[:nq], rd, top_k,
                                   out=_out(torch, nq, top_k, value))
                _check(got, want, (chunks, nq, ncand, top_k, "codes"))
                for cx1 in contexts:
                    for cx2 in contexts:
                        t1, e1 = streams[1, chunks[0], cx1]
                        t2, e2 = streams[2, chunks[1], cx2]
                        got = codec.refine(ctx, (t1, pq1, e1), (t2, pq2, e2), qd[:nq], rd, top_k,
                                           out=_out(torch, nq, top_k, value))
                        _check(got, want, (chunks, nq, ncand, top_k, cx1, cx2))
    codec.decode_status(ctx)                              # -1 and a duplicate are no errors


@pytest.fixture(scope="module")
def small(gpu):
    """the (8, 4, 16, 2) world at K = 256, context on, chunks (4, 7): streams and codes"""
    w = rr.sweep_world(rr.SHAPES[1], 256)
    streams, plain = _levels(gpu, w)
    return w, streams, plain


def test_no_queries_launch_nothing(gpu, small):
    torch, codec, ctx = gpu
    w, streams, plain = small
    qd = torch.from_numpy(w["q"]).cuda()
    rows = torch.zeros((0, 10), dtype=torch.int64, device="cuda")
    for levels in (streams, plain):
        out = _out(torch, 1, 10, POISON[1])
        got = codec.refine(ctx, *levels, qd[:0], rows, 10, out=(out[0][:0], out[1][:0]))
        assert got[0].shape == (0, 10) and got[1].shape == (0, 10)
        assert (_bits(out[0].cpu().numpy()) == POISON[1]).all()
    # the entry points themselves: PQH_OK without queries, candidates or outputs
    from pq_huffman_amd.capi import lib
    p = codec._ptr
    args = [(t.ptr, pq.ptr, p(e.stream), e.stream.numel(), e.raw_first, e.chunk_vectors,
             p(e.chunk_offsets), p(e.chunk_prev)) for t, pq, e in streams]
    tail = (rr.N, None, None, None, 0, 32, None, 10, 10, None, None, 10)
    assert lib().pqh_refine_stream(ctx.ptr, *args[0], *args[1], *tail) == 0
    assert lib().pqh_refine_codes(ctx.ptr, plain[0][0].ptr, p(plain[0][1]), plain[1][0].ptr,
                                  p(plain[1][1]), *tail) == 0
    codec.decode_status(ctx)


def test_argument_checks(gpu, small):
    torch, codec, ctx = gpu
    w, streams, plain = small
    qd = torch.from_numpy(w["q"]).cuda()
    rows = torch.zeros((5, 10), dtype=torch.int64, device="cuda")
    assert _status(lambda: codec.refine(ctx, *plain, qd, rows, 11)) == -1          # top_k > ncand
    assert _status(lambda: codec.refine(ctx, *plain, qd, rows, 0)) == -1
    wide = torch.zeros((5, 65), dtype=torch.int64, device="cuda")
    assert _status(lambda: codec.refine(ctx, *plain, qd, wide, 10)) == -1          # ncand > 64
    short = qd[:, :31].contiguous()                                                # ld_q < d
    assert _status(lambda: codec.refine(ctx, *plain, short, rows, 10)) == -1
    other = codec.PQ(ctx, np.zeros((4, 256, 4), np.float32))                       # d = 16, not 32
    codes = torch.zeros((rr.N, 4), dtype=torch.uint8, device="cuda")
    assert _status(lambda: codec.refine(ctx, plain[0], (other, codes), qd, rows, 10)) == -1
    assert _status(lambda: codec.refine(ctx, streams[0], plain[1], qd, rows, 10)) == -1
    codec.decode_status(ctx)
    other.close()


def test_an_all_padding_query_and_its_neighbours(gpu, small):
    torch, codec, ctx = gpu
    w, streams, plain = small
    rows = rr.candidates(5, 64, (4, 7), 3)
    rows[2] = -1
    want = _want(w, rows, 10)
    assert (want[1][2] == -1).all() and np.isposinf(want[0][2]).all() and (want[1][[1, 3]] >= 0).all()
    qd, rd = torch.from_numpy(w["q"]).cuda(), torch.from_numpy(rows).cuda()
    for i, levels in enumerate((streams, plain)):
        _check(codec.refine(ctx, *levels, qd, rd, 10, out=_out(torch, 5, 10, POISON[i])), want)
    codec.decode_status(ctx)


def test_query_and_output_layout(gpu, small):
    """queries d + 3 floats apart with NaN between them; outputs with gaps between their rows,
    the gaps as they were; out=None: fresh tensors"""
    torch, codec, ctx = gpu
    w, streams, plain = small
    nq, d = w["q"].shape
    wide = np.full((nq, d + 3), np.nan, np.float32)
    wide[:, :d] = w["q"]
    qd = torch.from_numpy(wide).cuda()[:, :d]
    assert qd.stride(0) == d + 3
    rows = rr.candidates(nq, 64, (4, 7), 4)
    rd = torch.from_numpy(rows).cuda()
    want = _want(w, rows, 10)
    for i, levels in enumerate((streams, plain)):
        value = POISON[i]
        bd = _poisoned(torch, (nq + 1, 13), torch.float32, value)
        bi = _poisoned(torch, (nq + 1, 13), torch.int64, value)
        got = codec.refine(ctx, *levels, qd, rd, 10, out=(bd[:nq, :10], bi[:nq, :10]))
        _check(got, want, i)
        hd, hi = bd.cpu().numpy(), bi.cpu().numpy()
        assert (_bits(hd[:nq, 10:]) == value).all() and (_bits(hd[nq:]) == value).all()
        assert (hi.view(np.uint32)[:nq, 20:] == value).all() and (hi.view(np.uint32)[nq:] == value).all()
        _check(codec.refine(ctx, *levels, qd, rd, 10), want, i)
    codec.decode_status(ctx)


@pytest.mark.parametrize("d", [15, 128])
def test_residual_form(gpu, d):
    """37 lists, several empty, candidates in the lists right after an empty one"""
    torch, codec, ctx = gpu
    w = rr.residual_world(d)
    rr.check_residual_world(w)
    streams, plain = _levels(gpu, w)
    cq = codec.Coarse(ctx, w["coarse"])
    qd, rd = torch.from_numpy(w["q"]).cuda(), torch.from_numpy(w["rows"]).cuda()
    od = torch.from_numpy(w["offsets"]).cuda()
    ncand = w["rows"].shape[1]
    case = 0
    for k in (1, 10, ncand):
        want = _want(w, w["rows"], k, residual=True)
        if k == 10:                                       # the centroid matters
            assert not np.array_equal(want[1], _want(w, w["rows"], k)[1])
        for levels in (streams, plain):
            got = codec.refine(ctx, *levels, qd, rd, k, coarse=cq, offsets=od,
                               out=_out(torch, 5, k, POISON[case % 3]))
            case += 1
            _check(got, want, (d, k))
    # one of the two without the other is refused
    assert _status(lambda: codec.refine(ctx, *plain, qd, rd, 1, coarse=cq)) == -1
    assert _status(lambda: codec.refine(ctx, *plain, qd, rd, 1, offsets=od)) == -1
    codec.decode_status(ctx)
    cq.close()


def test_ties_come_out_in_row_order(gpu):
    torch, codec, ctx = gpu
    w = rr.ties_world()
    streams, plain = _levels(gpu, w, k=16, context=(False, False), chunks=(4, 7))
    qd, rd = torch.from_numpy(w["q"]).cuda(), torch.from_numpy(w["rows"]).cuda()
    for k in (10, 64):
        want = _want(w, w["rows"], k)
        assert all((np.diff(want[0][i]) == 0).any() for i in range(4))
        for i, levels in enumerate((streams, plain)):
            _check(codec.refine(ctx, *levels, qd, rd, k, out=_out(torch, 4, k, POISON[i])), want, k)
    codec.decode_status(ctx)


# ------------------------------------------------------------------------------ errors
def test_a_row_outside_the_stream_is_dropped_and_reported(gpu, small):
    torch, codec, ctx = gpu
    w, streams, plain = small
    rows = rr.candidates(5, 10, (4, 7), 5)
    rows[1, 0], rows[3, 9] = rr.N, 2 ** 40
    want = _want(w, rows, 10)
    assert want[1][1][-1] == -1 and (want[1][0] >= 0).sum() == 8
    qd, rd = torch.from_numpy(w["q"]).cuda(), torch.from_numpy(rows).cuda()
    codec.decode_status(ctx)
    for levels in (streams, plain):
        _check(codec.refine(ctx, *levels, qd, rd, 10, out=_out(torch, 5, 10, POISON[0])), want)
        assert _status(lambda: codec.decode_status(ctx)) == -1                   # PQH_ERR_ARG
        codec.decode_status(ctx)                                                 # read once, then clean


@pytest.mark.parametrize("extra", [0, 100])
def test_a_row_past_the_last_list_is_dropped_and_reported(gpu, extra):
    """a residual re-rank whose offsets do not cover the stream: the offsets of rr.residual_world(15)
    from the end of the last non-empty list on (offsets[nlist] and the empty lists before it, so
    that they still ascend) lowered by three rows.  That list keeps a row and every row below the
    new end keeps its list; a candidate at or above it is inside [0, n) and is decoded, finds no
    list, is dropped and sets PQH_ERR_ARG, in a query's first and last slot too.  Expected: the
    mirrors with those candidates as rows outside the stream.  extra = 0: about 30 candidates,
    refine_rows; extra = 100: about 130, refine_rows_wide on a context whose limit is raised."""
    import metric_ref as mref
    torch, codec, ctx = gpu
    w = rr.residual_world(15)
    rr.check_residual_world(w)
    off, nlist = w["offsets"], len(w["offsets"]) - 1
    cut = rr.N - 3
    low = np.minimum(off, cut)
    last = int(np.flatnonzero(np.diff(off) > 0)[-1])      # the last non-empty list
    assert low[nlist] == cut < off[nlist] and (np.diff(low) >= 0).all()
    assert low[last] == off[last] < cut and np.array_equal(low[:last + 1], off[:last + 1])
    below = np.arange(cut)
    assert np.array_equal(rr.lists_of(low, below), rr.lists_of(off, below))
    assert (rr.lists_of(low, np.arange(cut, rr.N)) >= nlist).all()

    rng = np.random.default_rng(77 + extra)
    rows = np.concatenate([w["rows"], rng.integers(0, rr.N, size=(5, extra))], axis=1)
    ncand = rows.shape[1]
    assert (ncand <= 64) if extra == 0 else (64 < ncand <= 256)
    rows[0, 0], rows[2, -1], rows[4, 0], rows[4, -1] = cut, rr.N - 1, cut + 1, cut
    assert (rows[1] >= cut).any() and (rows[3] >= cut).any()     # (rr.N - 1 is in every query)
    outside = np.where(rows >= cut, rr.N, rows)
    streams, plain = _levels(gpu, w)
    cq = codec.Coarse(ctx, w["coarse"])
    qd, rd = torch.from_numpy(w["q"]).cuda(), torch.from_numpy(rows).cuda()
    od = torch.from_numpy(low).cuda()
    limit = ctx.search_max_k
    if ncand > limit:
        ctx.set_search_max_k(256)
    try:
        codec.decode_status(ctx)
        case = 0
        for fn, mirror in ((codec.refine, rr.refine), (codec.refine_ip, mref.refine)):
            for k in (10, ncand):
                want = mirror(w["q"], outside, k, w["cent1"], w["codes1"], w["cent2"], w["codes2"],
                              w["coarse"], off)
                if k == ncand:                            # the dropped ones are the padding
                    assert ((want[1] == -1).sum(axis=1) == (rows >= cut).sum(axis=1)).all()
                for levels in (streams, plain):
                    got = fn(ctx, *levels, qd, rd, k, coarse=cq, offsets=od,
                             out=_out(torch, 5, k, POISON[case % 3]))
                    case += 1
                    _check(got, want, (fn.__name__, extra, k))
                    assert _status(lambda: codec.decode_status(ctx)) == -1       # PQH_ERR_ARG
                    codec.decode_status(ctx)                                     # read once, then clean
    finally:
        ctx.set_search_max_k(limit)
    cq.close()


def test_a_corrupt_level_two_chunk_drops_its_candidates_only(gpu, small):
    """a level-2 chunk offset past the stream's end: the candidate in that chunk is dropped and
    PQH_ERR_CORRUPT reported (before a bad row's PQH_ERR_ARG); the other queries' results are the
    reference's; with no candidate in the chunk nothing is reported"""
    import dataclasses
    torch, codec, ctx = gpu
    w, streams, plain = small
    (t1, pq1, e1), (t2, pq2, e2) = streams
    j = 60                                                # level-2 rows 420 ... 426
    offs = e2.chunk_offsets.clone()
    offs[j] = e2.stream.numel() * 8 + 64
    broken = dataclasses.replace(e2, chunk_offsets=offs)
    rows = rr.candidates(5, 10, (4, 7), 6)
    assert not ((rows >= 7 * j) & (rows < 7 * j + 7)).any()
    qd = torch.from_numpy(w["q"]).cuda()
    codec.decode_status(ctx)
    _check(codec.refine(ctx, (t1, pq1, e1), (t2, pq2, broken), qd, torch.from_numpy(rows).cuda(), 10),
           _want(w, rows, 10))
    codec.decode_status(ctx)                              # the chunk was not walked: clean
    hit = rows.copy()
    hit[2, 0] = 7 * j + 3
    hit[4, 1] = rr.N + 5                                  # and a bad row elsewhere
    dropped = hit.copy()
    dropped[2, 0] = -1
    want = _want(w, dropped, 10)
    assert np.array_equal(want[1][[0, 1, 3]], _want(w, hit, 10)[1][[0, 1, 3]])
    _check(codec.refine(ctx, (t1, pq1, e1), (t2, pq2, broken), qd, torch.from_numpy(hit).cuda(), 10,
                        out=_out(torch, 5, 10, POISON[1])), want)
    assert _status(lambda: codec.decode_status(ctx)) == -6                       # PQH_ERR_CORRUPT
    codec.decode_status(ctx)


# ------------------------------------------------------------------------------ the index
@pytest.fixture(scope="module")
def world(gpu):
    torch, codec, ctx = gpu
    w = fref.ivf_world()
    w.update(xd=torch.from_numpy(w["x"]).cuda(), qd=torch.from_numpy(w["q"]).cuda(),
             pq=codec.PQ(ctx, w["cent"]), coarse=codec.Coarse(ctx, w["cc"]))
    return w


@pytest.mark.parametrize("kind", ["plain", "residual"])
def test_ivf_end_to_end(gpu, world, kind):
    torch, codec, ctx = gpu
    w = world
    r2 = rr.ivf_refine_world(w, kind)
    pq2 = codec.PQ(ctx, r2["cent2"])
    res = kind == "residual"
    ivf = codec.IVF.build(ctx, w["pq"], w["coarse"], w["xd"], chunk_vectors=4, residual=res,
                          refine_pq=pq2, refine_chunk_vectors=7)
    codec.ivf_status(ctx)
    assert ivf.enc.chunk_vectors == 4 and ivf.refine_enc.chunk_vectors == 7 and ivf.refine_pq is pq2
    assert np.array_equal(codec.decode(ctx, ivf.tables, ivf.enc).cpu().numpy(), w[kind]["codes"])
    assert np.array_equal(codec.decode(ctx, ivf.refine_tables, ivf.refine_enc).cpu().numpy(),
                          r2["codes2"])
    # pq_residuals: what the second codebook was trained on
    rows = w["coarse"].residuals(w["xd"], w["coarse"].assign(w["xd"]), ivf.perm) if res \
        else w["xd"][ivf.perm]
    assert np.array_equal(_bits(codec.pq_residuals(ctx, w["pq"], rows).cpu().numpy()), _bits(r2["left"]))
    nprobe, perm = fref.IVF_NPROBE, w["perm"]

    def want(k, c=64, keep=None, removed=None):
        _, cand = rr.ivf_candidates(w, kind, c, keep, removed)
        wd, rows = rr.ivf_refined(w, kind, r2, cand, k)
        return wd, np.where(rows >= 0, perm[np.maximum(rows, 0)], -1)

    keep = torch.from_numpy(w["keep"]).cuda()
    plain_ivf = codec.IVF.build(ctx, w["pq"], w["coarse"], w["xd"], chunk_vectors=4, residual=res)
    for schedule in ("query", "list"):
        def search(k, **kw):
            return ivf.search(w["qd"], nprobe, k, schedule=schedule, **kw)
        _check(search(10, refine=64), want(10), (schedule, 64))
        assert not np.array_equal(want(10)[1], fref.ivf_want(w, kind, 10)[1])
        _check(search(10, refine=10), want(10, 10), (schedule, 10))
        _check(search(64, refine=64), want(64), (schedule, "all"))
        _check(search(10, refine=64, keep=keep), want(10, keep=w["keep"]), (schedule, "keep"))
        # refine=0 and an index without refine_pq: the bits of a call without the new arguments
        for k in (10, 64):
            free = fref.ivf_want(w, kind, k)
            _check(search(k), free, k)
            _check(search(k, refine=0), free, k)
            _check(plain_ivf.search(w["qd"], nprobe, k, schedule=schedule), free, k)
    if res:                                               # slab by slab
        ivf.table_budget = 2 * nprobe * fref.IVF_M * 256 * 4
        _check(ivf.search(w["qd"], nprobe, 10, refine=64), want(10), "slabs")
        del ivf.table_budget
    assert _status(lambda: plain_ivf.search(w["qd"], nprobe, 10, refine=64)) == -1
    assert _status(lambda: ivf.search(w["qd"], nprobe, 10, refine=9)) == -1
    assert _status(lambda: ivf.search(w["qd"], nprobe, 10, refine=65)) == -1
    assert _status(lambda: plain_ivf.fetch(torch.arange(3, device="cuda"), refined=True)) == -1

    # fetch(refined=True): (c1 + c2), then + centroid
    ids = np.array([0, 5, 100, 900, 1002, 5], np.int64)
    srow = np.argsort(perm)[ids]
    y = rr.reconstruct(w["cent"], w[kind]["codes"][srow]) + rr.reconstruct(r2["cent2"], r2["codes2"][srow])
    if res:
        y = y + w["cc"][rr.lists_of(w["offsets"], srow)]
    idd = torch.from_numpy(ids).cuda()
    assert np.array_equal(_bits(ivf.fetch(idd, refined=True).cpu().numpy()), _bits(y))
    assert torch.equal(ivf.fetch(idd), plain_ivf.fetch(idd))

    # after remove(): the first query's refined result taken out
    first = want(10)[1][0]
    ivf.remove(torch.from_numpy(first).cuda())
    for schedule in ("query", "list"):
        got = ivf.search(w["qd"], nprobe, 10, schedule=schedule, refine=64)
        assert not np.isin(got[1].cpu().numpy(), first).any()
        _check(got, want(10, removed=first), (schedule, "removed"))
        _check(ivf.search(w["qd"], nprobe, 10, schedule=schedule, refine=64, keep=keep),
               want(10, keep=w["keep"], removed=first), (schedule, "removed, keep"))
    codec.decode_status(ctx)
    codec.ivf_status(ctx)
    pq2.close()
