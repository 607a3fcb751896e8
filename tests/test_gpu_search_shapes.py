"""The search kernels (pqh_search.hip, pqh_topk_dev.h) at the shapes, plan sizes and list paths
the other search tests never run.  Expected values come from numpy (tests/search_shapes_ref.py,
which tests/test_search_shapes_cpu.py pins to the definition), never from the calls under test:
every comparison is array_equal on the ids and on the uint32 view of the distances.

What runs what -- scan_launch picks adc_scan<SRC, NW, CTX, QB, RG, RT, LM>: SRC = 1 for the
*_codes* calls; NW = m / 8 for m in {8, 16} (a stream: and chunk_prev 8-byte aligned), else 0,
the byte-wise walk; QB = 1 for the range forms, else 8 if m <= 8 and m * K <= 2048, else 4.

  path                                          reached by                             test
  --------------------------------------------  -------------------------------------  ----------------------------
  scan_plan, second and later rounds (carry,    nr = 1,025 (two rounds, the second of  test_ranges_plan_rounds
  wsum written again after the closing          one range) and 2,111 (three); 1,024 is
  barrier)                                      exactly one
  lists_plan, the same (carry_p, carry_u,       nlist = 1,025 and 2,111, hot lists of  test_lists_plan_rounds,
  cnt[l] = p0, units past the first round)      ten pairs in the second and the third  test_coarse_probe_feeds_
                                                round; m = 8: units of 8, m = 12: of 4 both_schedules
  adc_scan<*, NW = 0, *, QB = 4>, plain and     m in {9, 12, 15} (m > 8: qb = 4, m no  test_shape_sweep,
  list-major                                    multiple of 8: nw = 0); m = 16 with    test_unaligned_chunk_contexts
                                                chunk_prev at byte 4 (packed = false)
  NW = 0, QB = 8                                m in {1, 2, 3, 5} (m * K <= 2048);     test_shape_sweep,
                                                m = 8 with chunk_prev at byte 4        test_unaligned_chunk_contexts
  K < 256: the stride i * k + c, the clamp      K in {2, 5, 16, 100} at m in {5, 12},  test_shape_sweep
  min(c, k - 1), qb from m * k <= 2048          (8, 16), (16, 16), (3, 5), (1, 2)
  RT form, scalar table load                    m * K no multiple of 4: (5, 5) = 25,   test_shape_sweep,
                                                (3, 5) = 15, (5, 2) = 10, (1, 2) = 2;  test_unaligned_tables
                                                or the table one float into its
                                                buffer (base & 15)
  probe form, m * K * 4 no multiple of 16:      the same four: 100, 60, 40 and 8       test_shape_sweep
  stage and window 4-byte aligned               bytes of table before the stages
                                                (rg: qb = 1)
  list_offer, serial inserts (<= 6 passing      one wave, one step; of the second      test_offer_boundary_stream,
  lanes) against list_merge (>= 7)              offer exactly j in {0, 1, 6, 7, 63,    test_offer_boundary_codes
                                                64} lanes pass, in three lane orders
  top_k other than 1, 10, 64 (kth,              top_k in {1, 2, 7, 33, 63, 64}; 3 in   test_shape_sweep,
  lane < top_k)                                 the offer tests                        test_offer_boundary_*
  adc_merge with more lists than its waves,     search_groups = 17, 40: the plain      test_merge_width,
  plain form, equal distances across them       form caps the groups at the steps, so  test_merge_width_of_a_
                                                N = 1,003 gives at most 16 (chunk 1:   longer_stream
                                                4 waves of the merge busy); 16,700
                                                rows give 17, 40 and 65 (the merge
                                                loop's second round, which the plain
                                                form otherwise sees only on the
                                                default grid of test_large_run)

Every K < 256 stream is a non-context one (context tables exist only at K = 256); the *_codes*
calls take any K.  Each sweep case also checks that codec.decode gives the codes back, so a
failure says whether the decoder or the scoring is at fault."""
import dataclasses
import functools

import numpy as np
import pytest

import datagen
import ivf_residual_ref as ref
import search_lists_ref as lref
import search_shapes_ref as sref

pytestmark = pytest.mark.gpu

NPROBE = sref.NPROBE


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


def _at_byte(torch, t, nbytes):
    """an equal copy of t that starts nbytes into a larger, 16-byte aligned buffer"""
    flat = t.contiguous().view(torch.uint8).reshape(-1)
    buf = torch.zeros(flat.numel() + 16, dtype=torch.uint8, device=t.device)
    assert buf.data_ptr() % 16 == 0
    view = buf[nbytes:nbytes + flat.numel()]
    view.copy_(flat)
    out = view.view(t.dtype).view(t.shape)
    assert out.data_ptr() % 16 == nbytes and out.dtype == t.dtype and out.shape == t.shape
    assert torch.equal(out.contiguous().view(torch.uint8).reshape(-1), flat)   # (NaN tables too)
    return out


def _all_forms(codec, ctx, src, k, ldq, ldp, od, pd, rpd, rd):
    """the five forms on one probe list: src = (tables, stream) or the device codes.  Returns
    [(name, result, which reference)]: 0 the plain search, 1 a table per query, 2 one per pair"""
    if isinstance(src, tuple):
        tabs, enc = src
        return [("search", codec.search(ctx, tabs, enc, ldq, k), 0),
                ("search_ranges", codec.search_ranges(ctx, tabs, enc, ldq, rpd, rd, k), 1),
                ("search_range_tables", codec.search_range_tables(ctx, tabs, enc, ldp, rpd, rd, k), 2),
                ("search_lists/query", codec.search_lists(ctx, tabs, enc, ldq, od, pd, k), 1),
                ("search_lists/pair", codec.search_lists(ctx, tabs, enc, ldp, od, pd, k), 2)]
    return [("search_codes", codec.search_codes(ctx, src, ldq, k), 0),
            ("search_codes_ranges", codec.search_codes_ranges(ctx, src, ldq, rpd, rd, k), 1),
            ("search_codes_range_tables", codec.search_codes_range_tables(ctx, src, ldp, rpd, rd, k), 2),
            ("search_codes_lists/query", codec.search_codes_lists(ctx, src, ldq, od, pd, k), 1),
            ("search_codes_lists/pair", codec.search_codes_lists(ctx, src, ldp, od, pd, k), 2)]


# ------------------------------------------------------------------------------ a. the shape sweep
@functools.lru_cache(maxsize=2)
def _sweep(m, K, chunk):
    """a sweep case and its references, made once for the tests that share it"""
    case = sref.sweep_case(m, K, chunk, 100 * m + K + chunk)
    sref.check_sweep_case(m, K, chunk, case)
    return case, sref.sweep_want(case, 64)


# every shape over the codes and as a stream without contexts, a K = 256 shape as a context
# stream too; the tests of a shape follow one another and share _sweep
SWEEP = [(m, K, chunk, source) for chunk in sref.CHUNKS for m, K in sref.SHAPES
         for source in (("codes", "noctx", "ctx") if K == 256 else ("codes", "noctx"))]


@pytest.mark.parametrize("m,K,chunk,source", SWEEP)
def test_shape_sweep(gpu, m, K, chunk, source):
    """all five forms on the probe list of search_lists_ref.sweep_case with K symbols a part,
    over the codes, the stream without contexts or the context stream: top_k in {1, 2, 7, 33,
    63, 64} at search_groups in {1, 3, default}"""
    torch, codec, ctx = gpu
    case, wants = _sweep(m, K, chunk)
    codes, offsets, probes, lut_q, lut_pair = case
    assert (wants[2][1][5] == -1).all() and not np.isnan(wants[2][0]).any()
    cd, ldq, ldp, od, pd = _dev(torch, codes, lut_q, lut_pair, offsets, probes)
    rpd, rd = _dev(torch, *lref.probe_ranges(offsets, probes))
    srcs = [(source, cd if source == "codes" else _encoded(gpu, cd, K, chunk, source == "ctx"))]
    try:
        for g in (1, 3, 0):
            ctx.set_tuning(search_groups=g)
            for k in sref.TOP_KS:
                for tag, src in srcs:
                    for name, got, which in _all_forms(codec, ctx, src, k, ldq, ldp, od, pd, rpd, rd):
                        _check(got, sref.head(wants[which], k), (tag, name, g, k))
    finally:
        ctx.set_tuning(search_groups=0)
    codec.decode_status(ctx)


# ------------------------------------------------------------------------------ b. unaligned operands
@pytest.mark.parametrize("m", [8, 16])
def test_unaligned_chunk_contexts(gpu, m):
    """chunk_prev at byte 4 of its buffer: not readable as u64 words, so the byte-wise walk with
    eight (m = 8) or four (m = 16) query tables -- the bits of the aligned index, and numpy's"""
    torch, codec, ctx = gpu
    chunk = 7
    case = sref.sweep_case(m, 256, chunk, 300 + m)
    codes, offsets, probes, lut_q, lut_pair = case
    wants = sref.sweep_want(case, 64)
    cd, ldq, ldp, od, pd = _dev(torch, codes, lut_q, lut_pair, offsets, probes)
    rpd, rd = _dev(torch, *lref.probe_ranges(offsets, probes))
    tabs, enc = _encoded(gpu, cd, 256, chunk, True)
    assert enc.chunk_prev.data_ptr() % 8 == 0
    moved = dataclasses.replace(enc, chunk_prev=_at_byte(torch, enc.chunk_prev, 4))
    assert moved.chunk_prev.data_ptr() % 8 == 4 and moved.stream is enc.stream
    try:
        for g in (1, 0):
            ctx.set_tuning(search_groups=g)
            for k in (64, 7):
                aligned = _all_forms(codec, ctx, (tabs, enc), k, ldq, ldp, od, pd, rpd, rd)
                byte_wise = _all_forms(codec, ctx, (tabs, moved), k, ldq, ldp, od, pd, rpd, rd)
                for (name, a, which), (_, b, _) in zip(aligned, byte_wise):
                    _same(torch, a, b, (name, g, k))
                    _check(b, sref.head(wants[which], k), (name, g, k))
    finally:
        ctx.set_tuning(search_groups=0)
    codec.decode_status(ctx)


@pytest.mark.parametrize("m,K", [(8, 256), (16, 256), (12, 256), (5, 5), (8, 16)])
def test_unaligned_tables(gpu, m, K):
    """the tables a view that starts one float into a larger buffer: every form, stream and
    codes (the per-range form then loads its tables entry by entry)"""
    torch, codec, ctx = gpu
    chunk = 7
    case = sref.sweep_case(m, K, chunk, 400 + m + K)
    codes, offsets, probes, lut_q, lut_pair = case
    wants = sref.sweep_want(case, 64)
    cd, ldq, ldp, od, pd = _dev(torch, codes, lut_q, lut_pair, offsets, probes)
    rpd, rd = _dev(torch, *lref.probe_ranges(offsets, probes))
    ldq, ldp = _at_byte(torch, ldq, 4), _at_byte(torch, ldp, 4)
    assert ldq.data_ptr() % 16 == 4 and ldp.data_ptr() % 16 == 4
    enc = _encoded(gpu, cd, K, chunk, K == 256)
    for k in (64, 7):
        for src in (enc, cd):
            for name, got, which in _all_forms(codec, ctx, src, k, ldq, ldp, od, pd, rpd, rd):
                _check(got, sref.head(wants[which], k), (name, k))
    codec.decode_status(ctx)


@pytest.mark.parametrize("m,K", [(8, 256), (16, 256), (12, 256), (3, 5)])
def test_codes_at_byte_one(gpu, m, K):
    """the codes start at byte 1 of their buffer: no row group is 4-byte aligned unless its
    first row happens to be, in the range and the list forms"""
    torch, codec, ctx = gpu
    case = sref.sweep_case(m, K, 7, 500 + m + K)
    codes, offsets, probes, lut_q, lut_pair = case
    wants = sref.sweep_want(case, 64)
    cd, ldq, ldp, od, pd = _dev(torch, codes, lut_q, lut_pair, offsets, probes)
    rpd, rd = _dev(torch, *lref.probe_ranges(offsets, probes))
    moved = _at_byte(torch, cd, 1)
    assert moved.data_ptr() % 4 == 1
    for k in (64, 2):
        for name, got, which in _all_forms(codec, ctx, moved, k, ldq, ldp, od, pd, rpd, rd):
            _check(got, sref.head(wants[which], k), (name, k))
    codec.decode_status(ctx)


# ------------------------------------------------------------------------------ c. the plan rounds
@pytest.mark.parametrize("form", ["query", "range"])
@pytest.mark.parametrize("nr", [1024, 1025, 2111])
def test_ranges_plan_rounds(gpu, nr, form):
    """scan_plan over one round exactly, one range more, and three rounds: a table per query on
    a K = 256 context stream, a table per range at K = 16.  Then the same ranges with
    out-of-bounds ones in every round: skipped, reported, every other range as it was."""
    torch, codec, ctx = gpu
    K = 256 if form == "query" else 16
    case = sref.ranges_case(nr, nr, m=8, K=K)
    sref.check_ranges_case(nr, case)
    sref.check_ranges_carry(nr, case)
    codes, ptr = case["codes"], case["ptr"]
    lut = case["lut_q"] if form == "query" else case["lut_r"]
    tables = sref.per_range(lut, ptr, nr) if form == "query" else lut
    cd, ld, pd = _dev(torch, codes, lut, ptr)
    tabs, enc = _encoded(gpu, cd, K, case["C"], K == 256)
    by_stream = codec.search_ranges if form == "query" else codec.search_range_tables
    by_codes = codec.search_codes_ranges if form == "query" else codec.search_codes_range_tables
    for ranges, status in ((case["ranges"], 0), (case["bad"], -1)):      # -1: PQH_ERR_ARG
        rd, = _dev(torch, ranges)
        want = ref.search(tables, codes, 64, ptr, ranges)
        assert (want[1][:2] >= 0).all() and (want[1][2] == -1).all()     # (query 2 has no range)
        try:
            for g in (0, 3):
                ctx.set_tuning(search_groups=g)
                for k in (64, 7):
                    got = by_stream(ctx, tabs, enc, ld, pd, rd, k)
                    assert _status(lambda: codec.decode_status(ctx)) == status, (g, k)
                    _check(got, sref.head(want, k), ("stream", g, k, status))
                    got = by_codes(ctx, cd, ld, pd, rd, k)
                    assert _status(lambda: codec.decode_status(ctx)) == status, (g, k)
                    _check(got, sref.head(want, k), ("codes", g, k, status))
        finally:
            ctx.set_tuning(search_groups=0)
    codec.decode_status(ctx)


@pytest.mark.parametrize("m", [8, 12])
@pytest.mark.parametrize("nlist", [1024, 1025, 2111])
def test_lists_plan_rounds(gpu, nlist, m):
    """lists_plan over one round exactly, one list more, and three rounds, in units of eight
    pairs (m = 8) and of four (m = 12): a table per query and one per pair, and the range calls
    on the same probes"""
    torch, codec, ctx = gpu
    case = sref.lists_case(nlist, m, nlist + m)
    sref.check_lists_carry(nlist, m, case)
    codes, offsets, probes = case["codes"], case["offsets"], case["probes"]
    ptr, ranges = lref.probe_ranges(offsets, probes)
    cd, od, pd, rpd, rd = _dev(torch, codes, offsets, probes, ptr, ranges)
    tabs, enc = _encoded(gpu, cd, 256, case["C"], True)
    for lut in (case["lut_q"], case["lut_pair"]):
        per_query = lut is case["lut_q"]
        ld, = _dev(torch, lut)
        want = ref.search(np.repeat(lut, probes.shape[1], axis=0) if per_query else lut,
                          codes, 64, ptr, ranges)
        try:
            for g in (0, 3):
                ctx.set_tuning(search_groups=g)
                for k in (64, 7):
                    _check(codec.search_lists(ctx, tabs, enc, ld, od, pd, k), sref.head(want, k),
                           ("stream", per_query, g, k))
                    _check(codec.search_codes_lists(ctx, cd, ld, od, pd, k), sref.head(want, k),
                           ("codes", per_query, g, k))
        finally:
            ctx.set_tuning(search_groups=0)
        fn = codec.search_ranges if per_query else codec.search_range_tables
        _same(torch, codec.search_lists(ctx, tabs, enc, ld, od, pd, 64),
              fn(ctx, tabs, enc, ld, rpd, rd, 64), per_query)
    codec.decode_status(ctx)


def test_coarse_probe_feeds_both_schedules(gpu):
    """pqh_coarse_probe at nlist = 1,025: its probes into the *_lists calls and its ranges into
    the *_ranges calls, device to device; the two equal each other and numpy"""
    torch, codec, ctx = gpu
    case = sref.coarse_case(1025)
    sref.check_coarse_case(case)
    cd, ld, od, qd = _dev(torch, case["codes"], case["lut_q"], case["offsets"], case["q"])
    tabs, enc = _encoded(gpu, cd, 256, 4, True)
    coarse = codec.Coarse(ctx, case["cc"])
    nprobe = case["probes"].shape[1]
    want = ref.search(np.repeat(case["lut_q"], nprobe, axis=0), case["codes"], 64, case["ptr"],
                      case["ranges"])
    for k in (64, 7):
        rpd, rd, pd, _ = coarse.probe(qd, nprobe, od)
        by_list = codec.search_lists(ctx, tabs, enc, ld, od, pd, k)
        by_query = codec.search_ranges(ctx, tabs, enc, ld, rpd, rd, k)
        codes_list = codec.search_codes_lists(ctx, cd, ld, od, pd, k)
        codes_query = codec.search_codes_ranges(ctx, cd, ld, rpd, rd, k)
        _same(torch, by_list, by_query, k)
        _same(torch, codes_list, codes_query, k)
        for got in (by_list, by_query, codes_list, codes_query):
            _check(got, sref.head(want, k), k)
        assert np.array_equal(pd.cpu().numpy(), case["probes"])
        assert np.array_equal(rd.cpu().numpy(), case["ranges"])
    codec.ivf_status(ctx)
    codec.decode_status(ctx)


# ------------------------------------------------------------------------------ d. the offer boundary
def _offers(gpu, n, run):
    torch, codec, ctx = gpu
    codes = sref.offer_codes(n, 8, n)
    cd, = _dev(torch, codes)
    src = run(cd)
    seed = 0
    try:
        ctx.set_tuning(search_groups=1)
        for top_k in sref.OFFER_TOP_KS:
            for j in sref.OFFER_J:
                for order in sref.OFFER_ORDERS:
                    seed += 1                       # (the seeds of tests/test_search_shapes_cpu.py)
                    lut = sref.offer_table(n, 8, top_k, j, order, seed)
                    sref.check_offer_case(n, codes, lut, top_k, j, order)
                    ld, = _dev(torch, lut)
                    _check(src(ld, top_k), sref.want(lut, codes, top_k), (top_k, j, order))
    finally:
        ctx.set_tuning(search_groups=0)
    codec.decode_status(ctx)


def test_offer_boundary_stream(gpu):
    """128 rows in chunks of 2, one workgroup: 64 chunks are one step of one wave, rows 0-63
    its first offer (which fills the list) and rows 64-127 the second, of which exactly j beat
    the threshold -- ascending, descending and shuffled by lane"""
    torch, codec, ctx = gpu

    def run(cd):
        tabs, enc = _encoded(gpu, cd, 256, 2, True)
        return lambda ld, k: codec.search(ctx, tabs, enc, ld, k)
    _offers(gpu, 128, run)


def test_offer_boundary_codes(gpu):
    """256 rows are one step of search_codes (four rows a lane): four offers, the second and
    the fourth with j passing lanes, the third with none"""
    torch, codec, ctx = gpu
    _offers(gpu, 256, lambda cd: lambda ld, k: codec.search_codes(ctx, cd, ld, k))


# ------------------------------------------------------------------------------ e. the merge width
def _ties_lut(nq, m, seed, values=3):
    """only the values 0, 1, 2 (or 0 ... values - 1): many rows share each distance, the ids
    decide"""
    return np.random.default_rng(seed).integers(0, values, size=(nq, m, 256)).astype(np.float32)


@pytest.mark.parametrize("chunk", [1, 4])
def test_merge_width(gpu, chunk):
    """the N = 1,003 shape of tests/test_gpu_search.py with the ties table at search_groups 17
    and 40.  The plain form caps the groups at the steps -- 16 at chunk 1, 4 at chunk 4 and for
    the codes -- so this reaches 16 partial lists, four waves of adc_merge; the next test has
    the steps for more."""
    torch, codec, ctx = gpu
    codes = datagen.skewed_codes(1003, 8, k=256, seed=100 + 8 + 256)
    lut = _ties_lut(9, 8, 6)
    want = sref.want(lut, codes, 64)
    assert all(len(np.unique(want[0][q])) < 16 for q in range(9))
    cd, ld = _dev(torch, codes, lut)
    tabs, enc = _encoded(gpu, cd, 256, chunk, True)
    try:
        for g in (17, 40):
            ctx.set_tuning(search_groups=g)
            for k in (64, 33):
                _check(codec.search(ctx, tabs, enc, ld, k), sref.head(want, k), (g, k))
                _check(codec.search_codes(ctx, cd, ld, k), sref.head(want, k), (g, k))
    finally:
        ctx.set_tuning(search_groups=0)
    codec.decode_status(ctx)


def test_merge_width_of_a_longer_stream(gpu):
    """16,700 rows: 261 steps of the stream in chunks of 1 and 66 of the codes, so
    search_groups 17, 40 and 65 are what runs -- more partial lists than adc_merge has waves,
    and at 65 * 64 entries the second round of its loop -- with equal distances across them"""
    torch, codec, ctx = gpu
    n = 16_700
    assert -(-n // 64) >= 65 and -(-n // 256) >= 65 and 65 * 64 > 16 * 4 * 64
    codes = datagen.skewed_codes(n, 8, seed=77, stay=0)
    lut = _ties_lut(9, 8, 7, values=40)
    want = sref.want(lut, codes, 64)
    assert all(len(np.unique(want[0][q])) < 32 for q in range(9))
    # the best 64 come from far more than 16 of 65 equal spans of the rows
    assert all(len(np.unique(want[1][q] * 65 // n)) > 20 for q in range(9))
    cd, ld = _dev(torch, codes, lut)
    tabs, enc = _encoded(gpu, cd, 256, 1, True)
    try:
        for g in (17, 40, 65):
            ctx.set_tuning(search_groups=g)
            for k in (64, 33):
                _check(codec.search(ctx, tabs, enc, ld, k), sref.head(want, k), (g, k))
                _check(codec.search_codes(ctx, cd, ld, k), sref.head(want, k), (g, k))
    finally:
        ctx.set_tuning(search_groups=0)
    codec.decode_status(ctx)
