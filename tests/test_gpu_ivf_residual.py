"""The residual inverted file on the GPU: pqh_ivf_residuals, pqh_adc_tables_residual, the probe
search with one table per range (pqh_search_stream_range_tables,
pqh_search_codes_range_tables) and codec.IVF with residual=True from vectors and queries to
neighbour ids.  Expected values come from numpy (tests/ivf_residual_ref.py, tests/ivf_ref.py),
never from the calls under test: floats are compared on their raw bits, ids with array_equal."""
import ctypes

import numpy as np
import pytest

import datagen
import ivf_ref
import ivf_residual_ref as ref

pytestmark = pytest.mark.gpu

POISON = (0xFFFFFFFF, 0xA5A5A5A5, 0x00000001)   # (the patterns of tests/test_gpu_search.py)


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


def _check(got, want, what=""):
    gd, gi = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert gd.dtype == np.float32 and gi.dtype == np.int64
    assert np.array_equal(gi, want[1]), what
    assert np.array_equal(_bits(gd), _bits(want[0])), what


# ------------------------------------------------------------------------------ residuals
def _residuals_case(gpu, cq, x, c, lists, perm, pad_x, pad_o, value, what):
    """x with NaN between its rows, out poisoned with gaps between its rows: the rows exact,
    the gaps as they were"""
    torch, codec, ctx = gpu
    n, d = x.shape
    wide = np.full((max(n, 1), d + pad_x), np.nan, np.float32)
    wide[:n, :d] = x
    xd = torch.from_numpy(wide).cuda()[:n, :d]
    assert n < 2 or xd.stride(0) == d + pad_x
    want, bad = ref.residuals(x, c, lists, perm)
    assert not np.isnan(want).any()
    buf = _poisoned(torch, (max(n, 1), d + pad_o), torch.float32, value)
    out = buf[:n, :d]
    got = cq.residuals(xd, torch.from_numpy(lists).cuda(),
                       None if perm is None else torch.from_numpy(perm).cuda(), out=out)
    assert got is out
    host = buf.cpu().numpy()
    assert np.array_equal(_bits(host[:n, :d]), _bits(want)), what
    assert (_bits(host[:n, d:]) == value).all() and (_bits(host[n:]) == value).all(), what
    return want, bad


@pytest.mark.parametrize("d", [1, 5, 128, 130])
def test_residuals_sweep(gpu, d):
    """n in {0, 1, 1003} (more than one workgroup), perm given and None, rows 16 bytes apart
    (the float4 steps, where d allows them) and not"""
    torch, codec, ctx = gpu
    nlist = 37
    rng = np.random.default_rng(2000 + d)
    x = rng.normal(0.0, 30.0, size=(1003, d)).astype(np.float32)
    c = rng.normal(0.0, 30.0, size=(nlist, d)).astype(np.float32)
    cq = codec.Coarse(ctx, c)
    case = 0
    for n in (0, 1, 1003):
        lists = rng.integers(0, nlist, size=n).astype(np.int32)
        perm = rng.permutation(n).astype(np.int64)
        for pad_x, pad_o in ((3, 2), (4, 8)):
            for p in (perm, None):
                _residuals_case(gpu, cq, x[:n], c, lists, p, pad_x, pad_o, POISON[case % 3],
                                (d, n, pad_x, p is None))
                case += 1
    # out = None: a fresh (n, d) tensor
    lists = rng.integers(0, nlist, size=1003).astype(np.int32)
    got = cq.residuals(torch.from_numpy(x).cuda(), torch.from_numpy(lists).cuda())
    assert got.shape == (1003, d)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(ref.residuals(x, c, lists)[0]))
    codec.ivf_status(ctx)
    cq.close()


@pytest.mark.parametrize("d,pad", [(128, 4), (130, 3)])
def test_residuals_flag_a_bad_list_id_and_a_bad_perm_entry(gpu, d, pad):
    """a zero row each, PQH_ERR_ARG from the status once, every other row exact"""
    torch, codec, ctx = gpu
    n, nlist = 1003, 37
    rng = np.random.default_rng(d)
    x = rng.normal(0.0, 30.0, size=(n, d)).astype(np.float32)
    c = rng.normal(0.0, 30.0, size=(nlist, d)).astype(np.float32)
    cq = codec.Coarse(ctx, c)
    lists = rng.integers(0, nlist, size=n).astype(np.int32)
    perm = rng.permutation(n).astype(np.int64)
    good = ref.residuals(x, c, lists, perm)[0]
    codec.ivf_status(ctx)
    broken_l, broken_p = lists.copy(), perm.copy()
    broken_l[77], broken_l[500] = nlist, -1
    broken_p[5], broken_p[9], broken_p[1000] = n, -1, 2 ** 40
    want, bad = _residuals_case(gpu, cq, x, c, broken_l, broken_p, pad, pad, POISON[1], "bad")
    assert _status(lambda: codec.ivf_status(ctx)) == -1                      # PQH_ERR_ARG
    rows = set(np.flatnonzero(bad).tolist())
    assert {5, 9, 1000} <= rows and 3 <= len(rows) <= 5 and not want[bad].any()
    assert np.array_equal(want[~bad], good[~bad])
    codec.ivf_status(ctx)                                                    # read once, then clean
    _residuals_case(gpu, cq, x, c, lists, perm, pad, pad, POISON[2], "good")
    codec.ivf_status(ctx)
    # the argument checks: rows closer than d floats
    from pq_huffman_amd.capi import lib
    xd = torch.from_numpy(x).cuda()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    ld = torch.from_numpy(lists).cuda()
    assert lib().pqh_ivf_residuals(ctx.ptr, cq.ptr, p(xd), n, d - 1, p(ld), None, p(xd), d) == -1
    assert lib().pqh_ivf_residuals(ctx.ptr, cq.ptr, p(xd), n, d, p(ld), None, p(xd), d - 1) == -1
    assert lib().pqh_ivf_residuals(ctx.ptr, None, p(xd), n, d, p(ld), None, p(xd), d) == -1
    cq.close()


# ------------------------------------------------------------------------------ tables
@pytest.mark.parametrize("m,k,dsub", [(8, 256, 16), (16, 256, 8), (3, 16, 5), (1, 256, 4)])
def test_tables_sweep(gpu, m, k, dsub):
    """nq in {1, 9} x nprobe in {1, 5, 64}: probes with -1 and with repeated lists, the
    queries ld_q > d apart; bit-equal to numpy and to adc_tables run on the residual query"""
    torch, codec, ctx = gpu
    d, nlist = m * dsub, 13
    rng = np.random.default_rng(m * 1000 + k + dsub)
    cent = rng.normal(0.0, 20.0, size=(m, k, dsub)).astype(np.float32)
    c = rng.normal(0.0, 30.0, size=(nlist, d)).astype(np.float32)
    wide = np.full((9, d + 3), np.nan, np.float32)
    wide[:, :d] = rng.normal(0.0, 30.0, size=(9, d))
    q = wide[:, :d]
    qd = torch.from_numpy(wide).cuda()[:, :d]
    pq, cq = codec.PQ(ctx, cent), codec.Coarse(ctx, c)
    case = 0
    for nq in (1, 9):
        for nprobe in (1, 5, 64):
            probes = rng.integers(0, nlist, size=(nq, nprobe)).astype(np.int64)
            if nprobe > 1:
                probes[:, nprobe // 2] = -1
                probes[:, -1] = probes[:, 0]            # a list probed twice
                if nq > 1:
                    probes[nq - 1, 1:] = -1             # as after nprobe > nlist
            want = ref.tables(q[:nq], c, probes, cent)
            assert not np.isnan(want).any()
            value = POISON[case % 3]
            case += 1
            out = _poisoned(torch, (nq * nprobe + 1, m, k), torch.float32, value)
            got = codec.adc_tables_residual(ctx, pq, cq, qd[:nq], torch.from_numpy(probes).cuda(),
                                            out=out[:-1])
            host = out.cpu().numpy()
            assert np.array_equal(_bits(host[:-1]), _bits(want)), (nq, nprobe)
            assert (_bits(host[-1]) == value).all()
            flat = probes.reshape(-1)
            assert np.isinf(want[flat < 0]).all() and np.isfinite(want[flat >= 0]).all()
            # the same bits as the plain tables of the residual queries
            valid = np.flatnonzero(flat >= 0)
            rq = (q[valid // nprobe] - c[flat[valid]]).astype(np.float32)
            plain = codec.adc_tables(ctx, pq, torch.from_numpy(rq).cuda())
            assert torch.equal(plain.view(torch.int32), got[torch.from_numpy(valid).cuda()].view(torch.int32))
    # out = None
    probes = torch.from_numpy(rng.integers(0, nlist, size=(9, 5)).astype(np.int64)).cuda()
    got = codec.adc_tables_residual(ctx, pq, cq, qd, probes)
    assert got.shape == (45, m, k)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(ref.tables(q, c, probes.cpu().numpy(), cent)))
    codec.ivf_status(ctx)
    pq.close()
    cq.close()


def test_tables_errors(gpu):
    torch, codec, ctx = gpu
    rng = np.random.default_rng(77)
    m, k, dsub, nlist = 4, 16, 8, 5
    cent = rng.normal(0.0, 20.0, size=(m, k, dsub)).astype(np.float32)
    c = rng.normal(0.0, 30.0, size=(nlist, 32)).astype(np.float32)
    q = rng.normal(0.0, 30.0, size=(3, 33)).astype(np.float32)
    qd = torch.from_numpy(q).cuda()
    pq, cq = codec.PQ(ctx, cent), codec.Coarse(ctx, c)
    probes = np.array([[0, 4], [1, 1], [2, 3]], np.int64)
    pd = torch.from_numpy(probes).cuda()
    # pq's m * dsub must be the coarse quantizer's d
    other = codec.Coarse(ctx, rng.normal(0.0, 30.0, size=(nlist, 33)).astype(np.float32))
    assert _status(lambda: codec.adc_tables_residual(ctx, pq, other, qd, pd)) == -1   # PQH_ERR_ARG
    other.close()
    from pq_huffman_amd.capi import lib
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    out = torch.empty((6, m, k), dtype=torch.float32, device="cuda")
    assert lib().pqh_adc_tables_residual(ctx.ptr, pq.ptr, cq.ptr, p(qd), 3, 31, p(pd), 2, p(out)) == -1
    assert lib().pqh_adc_tables_residual(ctx.ptr, pq.ptr, cq.ptr, p(qd), 3, 33, p(pd), 0, p(out)) == -1
    assert lib().pqh_adc_tables_residual(ctx.ptr, pq.ptr, None, p(qd), 3, 33, p(pd), 2, p(out)) == -1
    wide = codec.PQ(ctx, rng.normal(0.0, 20.0, size=(4, 4096, 8)).astype(np.float32))
    assert _status(lambda: codec.adc_tables_residual(ctx, wide, cq, qd, pd)) == -4    # UNSUPPORTED
    wide.close()
    codec.ivf_status(ctx)
    # a list outside [0, nlist) that is not the padding: a table of +inf and the sticky bit
    for bad in (nlist, -2, 2 ** 40):
        broken = probes.copy()
        broken[1, 0] = bad
        got = codec.adc_tables_residual(ctx, pq, cq, qd, torch.from_numpy(broken).cuda())
        assert _status(lambda: codec.ivf_status(ctx)) == -1
        want = ref.tables(q[:, :32], c, broken, cent)
        assert np.isinf(want[2]).all() and np.isfinite(want[3]).all()
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))
        codec.ivf_status(ctx)
    # the padding alone is no error
    broken = probes.copy()
    broken[1, 0] = -1
    codec.adc_tables_residual(ctx, pq, cq, qd, torch.from_numpy(broken).cuda())
    codec.ivf_status(ctx)
    pq.close()
    cq.close()


# ------------------------------------------------------------------------------ range tables
NLIST, NPROBE = 9, 12
# the lists every query probes, in probe order (padded with -1 to NPROBE > NLIST)
PROBES = [[3, 0, 2, 1, 4],                        # the long list first, an empty and a single one
          [3, 5, 6, 8, 7, 4],                     # shares lists 3 and 4 with query 0
          [2],                                    # one row: fewer than k
          [1, 7],                                 # empty lists only: the padding
          [0, 1, 2, 3, 4, 5, 6, 7, 8, 0, 3],      # lists 0 and 3 twice, each time its own table
          [6, 3, 0]]                              # one table for all three: ties by stream row


def _list_sizes(C):
    """list 1 and 7 empty, list 2 a single row, list 3 longer than 64 chunks and cut at both
    ends, the others of sizes that are no multiple of C (unless C = 1)"""
    return [3 * C + C // 2 + 1, 0, 1, 64 * C + C + 3, 37, 2 * C + 1, 150, 0, 5]


def _range_case(m, chunk, seed):
    """codes in list order, the CSR probe list and one table per range"""
    sizes = _list_sizes(chunk)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(offsets[-1])
    codes = datagen.skewed_codes(n, m, seed=seed)
    # the first 20 rows of list 0 again in lists 3 and 6: equal distances under one table
    for l in (3, 6):
        codes[offsets[l]:offsets[l] + 20] = codes[:20]
    probes = np.full((len(PROBES), NPROBE), -1, np.int64)
    for qi, row in enumerate(PROBES):
        probes[qi, :len(row)] = row
    flat = probes.reshape(-1)
    ranges = np.zeros((flat.size, 2), np.int64)
    ranges[flat >= 0, 0] = offsets[flat[flat >= 0]]
    ranges[flat >= 0, 1] = (offsets[1:] - offsets[:-1])[flat[flat >= 0]]
    ptr = np.arange(len(PROBES) + 1, dtype=np.int64) * NPROBE
    rng = np.random.default_rng(seed + 1)
    lut = rng.normal(0.0, 100.0, size=(flat.size, m, 256)).astype(np.float32)
    lut[5 * NPROBE:5 * NPROBE + 3] = rng.integers(0, 3, size=(m, 256)).astype(np.float32)
    lut[ranges[:, 1] == 0] = np.nan        # the table of a range without rows is never read
    return codes, offsets, ptr, ranges, lut


@pytest.mark.parametrize("m", [8, 16, 3])
@pytest.mark.parametrize("chunk", [1, 7, 64])
@pytest.mark.parametrize("context", [True, False])
def test_range_tables_sweep(gpu, context, chunk, m):
    """the stream and the codes form, k in {1, 10, 64}, one workgroup per query, three, 64
    (most of them without a step) and the default grid"""
    torch, codec, ctx = gpu
    codes, offsets, ptr, ranges, lut = _range_case(m, chunk, 100 * m + chunk)
    n = codes.shape[0]
    # the inputs' own properties: a range of more than 64 chunks cut at both ends
    f, c = ranges[0]
    assert (f + c - 1) // chunk - f // chunk + 1 > 64
    assert chunk == 1 or (f % chunk and (f + c) % chunk)
    cd = torch.from_numpy(codes).cuda()
    tabs = codec.Tables(ctx, m, 256, context).build(codec.histogram(ctx, cd, 256, context))
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=chunk)
    ld, pd, rd = (torch.from_numpy(a).cuda() for a in (lut, ptr, ranges))
    want = {k: ref.search(lut, codes, k, ptr, ranges) for k in (1, 10, 64)}
    w64 = want[64]
    assert (w64[1][2] >= 0).sum() == 1 and (w64[1][3] == -1).all()
    ids, times = np.unique(w64[1][4], return_counts=True)
    assert (times[ids >= 0] <= 2).all()
    # query 5: equal distances across lists, in stream-row order
    d5, i5 = w64[0][5], w64[1][5]
    tie = np.flatnonzero(d5[1:] == d5[:-1])
    assert len(tie) > 8 and (i5[tie + 1] > i5[tie]).all()
    lists5 = np.searchsorted(offsets[1:], i5, side="right")
    assert (lists5[tie + 1] != lists5[tie]).any()
    # a stale table (every range scored with its predecessor's) would change the ids
    stale = ref.search(np.nan_to_num(np.roll(lut, 1, axis=0), nan=1e9), codes, 64, ptr, ranges)
    assert not np.array_equal(stale[1][0], w64[1][0]) and not np.array_equal(stale[1][4], w64[1][4])
    try:
        for g in (1, 3, 64, 0):
            ctx.set_tuning(search_groups=g)
            for k in (1, 10, 64):
                _check(codec.search_range_tables(ctx, tabs, enc, ld, pd, rd, k), want[k], (g, k))
                _check(codec.search_codes_range_tables(ctx, cd, ld, pd, rd, k), want[k], (g, k))
    finally:
        ctx.set_tuning(search_groups=0)
    # id_base, and an out pair to fill
    out = (torch.empty((6, 10), dtype=torch.float32, device="cuda"),
           torch.empty((6, 10), dtype=torch.int64, device="cuda"))
    got = codec.search_range_tables(ctx, tabs, enc, ld, pd, rd, 10, id_base=1000, out=out)
    assert got[0] is out[0]
    _check(got, ref.search(lut, codes, 10, ptr, ranges, id_base=1000))
    codec.decode_status(ctx)

    # against the existing kernel: every range with the table of the query that owns it
    own = np.random.default_rng(chunk).normal(0.0, 100.0, size=(6, m, 256)).astype(np.float32)
    per_range = np.repeat(own, NPROBE, axis=0)
    od, prd = torch.from_numpy(own).cuda(), torch.from_numpy(per_range).cuda()
    w = ref.search(per_range, codes, 64, ptr, ranges)
    a = codec.search_ranges(ctx, tabs, enc, od, pd, rd, 64)
    b = codec.search_range_tables(ctx, tabs, enc, prd, pd, rd, 64)
    e = codec.search_codes_range_tables(ctx, cd, prd, pd, rd, 64)
    _check(a, w)
    _check(b, w)
    _check(e, w)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    codec.decode_status(ctx)


def test_range_tables_after_lds_poison(gpu):
    """every CU's LDS filled with a pattern first: a table entry or a stage slot read before
    it was written shows as a wrong result"""
    from pq_huffman_amd.capi import lib
    torch, codec, ctx = gpu
    codes, offsets, ptr, ranges, lut = _range_case(8, 7, 5)
    cd = torch.from_numpy(codes).cuda()
    tabs = codec.Tables(ctx, 8, 256, True).build(codec.histogram(ctx, cd, 256, True))
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=7)
    ld, pd, rd = (torch.from_numpy(a).cuda() for a in (lut, ptr, ranges))
    want = ref.search(lut, codes, 64, ptr, ranges)
    for value in POISON:
        assert lib().pqh_debug_poison_lds(ctx.ptr, ctypes.c_uint(value)) == 0
        _check(codec.search_range_tables(ctx, tabs, enc, ld, pd, rd, 64), want, hex(value))
        assert lib().pqh_debug_poison_lds(ctx.ptr, ctypes.c_uint(value)) == 0
        _check(codec.search_codes_range_tables(ctx, cd, ld, pd, rd, 64), want, hex(value))
    codec.decode_status(ctx)


def test_range_tables_errors(gpu):
    """bad ranges and bad range_ptr entries are skipped and reported, every other query exact;
    the sound half of a stream cut in two is searchable without an error"""
    torch, codec, ctx = gpu
    n, m, chunk = 1003, 8, 7
    codes = datagen.skewed_codes(n, m, seed=108)
    cd = torch.from_numpy(codes).cuda()
    tabs = codec.Tables(ctx, m, 256, True).build(codec.histogram(ctx, cd, 256, True))
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=chunk)
    per_query = [[(10, 50), (-5, 10), (100, 20)],          # first < 0
                 [(10, -3), (200, 30)],                    # count < 0
                 [(n - 10, 20), (300, 5)],                 # first + count > n
                 [(5, 2 ** 62), (400, 10)],                # first + count overflows
                 [(0, n), (n + 1, 0), (n, 0)]]             # first > n; (n, 0) is merely empty
    ranges = np.array([r for p in per_query for r in p], np.int64)
    nr = len(ranges)
    ptr = np.concatenate([[0], np.cumsum([len(p) for p in per_query])]).astype(np.int64)
    # query 5 reversed (its end before its start), query 6 reaching past nr
    ptr = np.concatenate([ptr, [nr - 4, nr + 5]]).astype(np.int64)
    lut = np.random.default_rng(51).normal(0.0, 100.0, size=(nr, m, 256)).astype(np.float32)
    ld, pd, rd = (torch.from_numpy(a).cuda() for a in (lut, ptr, ranges))
    want = ref.search(lut, codes, 64, ptr, ranges)
    assert (want[1][5:] == -1).all() and (want[1][:5, 0] >= 0).all()
    for fn in (lambda: codec.search_range_tables(ctx, tabs, enc, ld, pd, rd, 64),
               lambda: codec.search_codes_range_tables(ctx, cd, ld, pd, rd, 64)):
        got = fn()
        assert _status(lambda: codec.decode_status(ctx)) == -1                  # PQH_ERR_ARG
        _check(got, want)
    codec.decode_status(ctx)                                                    # read once, then clean
    # the argument checks of the range calls
    out = (torch.empty((7, 65), dtype=torch.float32, device="cuda"),
           torch.empty((7, 65), dtype=torch.int64, device="cuda"))
    for k in (65, 0):
        assert _status(lambda: codec.search_range_tables(ctx, tabs, enc, ld, pd, rd, k, out=out)) == -1
        assert _status(lambda: codec.search_codes_range_tables(ctx, cd, ld, pd, rd, k, out=out)) == -1
    # no ranges at all: the padding
    none = torch.zeros((0, 2), dtype=torch.int64, device="cuda")
    zero = torch.zeros(3, dtype=torch.int64, device="cuda")
    pad = (np.full((2, 10), np.inf, np.float32), np.full((2, 10), -1, np.int64))
    _check(codec.search_range_tables(ctx, tabs, enc, ld, zero, none, 10), pad)
    _check(codec.search_codes_range_tables(ctx, cd, ld, zero, none, 10), pad)
    codec.decode_status(ctx)

    # the stream cut to half its whole words
    half = enc.stream.numel() // 4 // 2 * 4
    cut = codec.Encoded(enc.stream[:half], enc.bits, chunk, enc.chunk_offsets, enc.chunk_prev, n, 1)
    off = enc.chunk_offsets.cpu().numpy()
    sound = int((off[1:] <= half * 8).sum()) * chunk      # rows of the chunks that end inside it
    assert 100 < sound < n - 100
    ranges = np.array([(0, sound), (3, 9), (sound - 40, 40), (sound - 1, 1), (1, 1)], np.int64)
    ptr = np.array([0, 1, 3, 5], np.int64)
    pd, rd = torch.from_numpy(ptr).cuda(), torch.from_numpy(ranges).cuda()
    _check(codec.search_range_tables(ctx, tabs, cut, ld, pd, rd, 64),
           ref.search(lut, codes, 64, ptr, ranges))
    codec.decode_status(ctx)
    # a range reaching into the cut half: its sound chunks are all there is to find
    ranges = np.array([(3, 9), (sound - 40, 40), (20, 30), (sound - 20, 200), (sound + 70, 10)], np.int64)
    ptr = np.array([0, 2, 4, 5], np.int64)
    pd, rd = torch.from_numpy(ptr).cuda(), torch.from_numpy(ranges).cuda()
    got = codec.search_range_tables(ctx, tabs, cut, ld, pd, rd, 64)
    assert _status(lambda: codec.decode_status(ctx)) == -6                      # PQH_ERR_CORRUPT
    _check(got, ref.search(lut, codes, 64, ptr, ranges, keep=np.arange(n) < sound))
    codec.decode_status(ctx)


def test_range_tables_on_the_default_grid_of_a_larger_index(gpu):
    """60,000 rows in chunks of 4 as 64 lists, eight queries of 16 probes each with its own
    table: many workgroups per query, lists of one step and of many"""
    torch, codec, ctx = gpu
    n, m, nlist, nq, nprobe = 60_000, 8, 64, 8, 16
    rng = np.random.default_rng(63)
    codes = datagen.skewed_codes(n, m, seed=61, stay=0)
    cuts = np.sort(rng.choice(np.arange(1, n), size=nlist - 1, replace=False))
    cuts[:8] = np.arange(1, 9) * 37                        # some lists shorter than a step
    offsets = np.concatenate([[0], np.sort(cuts), [n]]).astype(np.int64)
    probes = np.stack([rng.permutation(nlist)[:nprobe] for _ in range(nq)])
    probes[:, 3] = np.arange(nq) % 8                       # every query a short list too
    flat = probes.reshape(-1)
    ranges = np.stack([offsets[flat], offsets[flat + 1] - offsets[flat]], axis=1)
    ptr = np.arange(nq + 1, dtype=np.int64) * nprobe
    lut = rng.normal(0.0, 100.0, size=(nq * nprobe, m, 256)).astype(np.float32)
    cd = torch.from_numpy(codes).cuda()
    tabs = codec.Tables(ctx, m, 256, True).build(codec.histogram(ctx, cd, 256, True))
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=4)
    ld, pd, rd = (torch.from_numpy(a).cuda() for a in (lut, ptr, ranges))
    want = ref.search(lut, codes, 64, ptr, ranges)
    _check(codec.search_range_tables(ctx, tabs, enc, ld, pd, rd, 64), want)
    _check(codec.search_codes_range_tables(ctx, cd, ld, pd, rd, 64), want)
    codec.decode_status(ctx)


# ------------------------------------------------------------------------------ end to end
N, NL, M, NQ = 1003, 13, 8, 9


@pytest.fixture(scope="module")
def world(gpu):
    """x with 50 rows twice, a 13-list coarse codebook, an 8 x 256 PQ trained on the
    residuals, nine queries near rows of x"""
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
    return dict(x=x, cc=cc, cent=cent, q=q, lists=lists, perm=perm, offsets=offsets, res=res,
                cdist=ivf_ref.dists(q, cc), xd=torch.from_numpy(x).cuda(),
                qd=torch.from_numpy(q).cuda(), pq=codec.PQ(ctx, cent), coarse=codec.Coarse(ctx, cc))


@pytest.mark.parametrize("chunk", [7, 64])
@pytest.mark.parametrize("context", [True, False])
def test_residual_ivf_equals_numpy(gpu, world, context, chunk):
    torch, codec, ctx = gpu
    w = world
    ivf = codec.IVF.build(ctx, w["pq"], w["coarse"], w["xd"], chunk_vectors=chunk, context=context,
                          residual=True)
    codec.ivf_status(ctx)
    assert ivf.residual
    assert np.array_equal(ivf.perm.cpu().numpy(), w["perm"])
    assert np.array_equal(ivf.offsets.cpu().numpy(), w["offsets"])
    inv = np.empty(N, np.int64)
    inv[w["perm"]] = np.arange(N)
    assert np.array_equal(ivf.inv.cpu().numpy(), inv)
    # build: the stream holds the codes of the residuals in list order
    codes = codec.decode(ctx, ivf.tables, ivf.enc).cpu().numpy()
    codec.decode_status(ctx)
    assert np.array_equal(codes, ref.pq_codes(w["res"], w["cent"]))
    assert np.array_equal(codes, w["pq"].assign(torch.from_numpy(w["res"]).cuda()).cpu().numpy())
    # search: ids are caller rows
    for nprobe in (1, 4, 16):                                   # (16 > 13 lists: padding)
        ptr, ranges, probes, _ = ivf_ref.probe(w["q"], w["cc"], nprobe, w["offsets"], w["cdist"])
        lut = ref.tables(w["q"], w["cc"], probes, w["cent"])
        for k in (1, 10, 64):
            wd, rows = ref.search(lut, codes, k, ptr, ranges)
            wi = np.where(rows >= 0, w["perm"][np.maximum(rows, 0)], -1)
            gd, gi = ivf.search(w["qd"], nprobe, k)
            assert np.array_equal(gi.cpu().numpy(), wi), (nprobe, k)
            assert np.array_equal(_bits(gd.cpu().numpy()), _bits(wd)), (nprobe, k)
            if nprobe == 4 and k == 64:
                # the doubled rows tie, in (dist, list, caller row) order: the same list, so
                # the smaller caller row first
                tie = np.flatnonzero((wd[0][1:] == wd[0][:-1]) & np.isfinite(wd[0][1:]))
                pairs = [(wi[0][t], wi[0][t + 1]) for t in tie]
                assert any(b == a + 800 for a, b in pairs), pairs
                for qi in range(NQ):
                    key = [(wd[qi][j], w["lists"][wi[qi][j]], wi[qi][j]) for j in range(64)
                           if wi[qi][j] >= 0]
                    assert all(key[j] < key[j + 1] for j in range(len(key) - 1))
    codec.decode_status(ctx)
    codec.ivf_status(ctx)

    # three slabs give what one gives
    one = ivf.search(w["qd"], 4, 10)
    ivf.table_budget = 3 * 4 * M * 256 * 4                      # the tables of three queries
    three = ivf.search(w["qd"], 4, 10)
    ivf.table_budget = 1                                        # (never less than a query a slab)
    nine = ivf.search(w["qd"], 4, 10)
    del ivf.table_budget
    assert ivf.table_budget == codec.IVF.table_budget
    for got in (three, nine):
        assert torch.equal(got[1], one[1]) and torch.equal(got[0].view(torch.int32), one[0].view(torch.int32))

    # fetch: the centroid of the row's list plus the decoded residual
    ids = one[1].reshape(-1)
    assert int(ids.min()) >= 0
    ids_h = ids.cpu().numpy()
    rhat = np.concatenate([w["cent"][i][codes[inv[ids_h], i]] for i in range(M)], axis=1)
    want = w["cc"][w["lists"][ids_h]] + rhat
    assert want.dtype == np.float32
    got = ivf.fetch(ids)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))
    # and nearer to x than the centroid alone
    err = ((got.cpu().numpy() - w["x"][ids_h]) ** 2).sum()
    assert err < ((w["cc"][w["lists"][ids_h]] - w["x"][ids_h]) ** 2).sum()
    codec.decode_status(ctx)


def test_the_plain_index_is_unchanged_by_the_flag(gpu, world):
    """residual=False is the default and the path of before: the stream holds the codes of
    x[perm], and fetch adds nothing"""
    torch, codec, ctx = gpu
    w = world
    a = codec.IVF.build(ctx, w["pq"], w["coarse"], w["xd"], chunk_vectors=7)
    b = codec.IVF.build(ctx, w["pq"], w["coarse"], w["xd"], chunk_vectors=7, residual=False)
    assert not a.residual and not b.residual
    codes = codec.decode(ctx, a.tables, a.enc)
    assert torch.equal(codes, w["pq"].assign(w["xd"][a.perm]))
    assert torch.equal(codes, codec.decode(ctx, b.tables, b.enc))
    ra, rb = a.search(w["qd"], 4, 10), b.search(w["qd"], 4, 10)
    assert torch.equal(ra[1], rb[1]) and torch.equal(ra[0].view(torch.int32), rb[0].view(torch.int32))
    ids = ra[1].reshape(-1)
    assert torch.equal(a.fetch(ids), w["pq"].reconstruct(w["pq"].assign(w["xd"])[ids]))
    codec.decode_status(ctx)
    codec.ivf_status(ctx)
