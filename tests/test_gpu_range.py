"""Range search on the GPU: pqh_range_count_* / pqh_range_fill_* behind codec.range_search*,
and codec.IVF.range_search.  Expected values come from numpy (tests/range_ref.py:
ivf_residual_ref.adc, d < r in scan order), never from the calls under test.  lims and ids are
compared with array_equal, dist on the raw float bits."""
import ctypes

import numpy as np
import pytest

import range_ref as rref
import search_filter_ref as fref
import search_shapes_ref as sref

pytestmark = pytest.mark.gpu

POISON = (0xFFFFFFFF, 0xA5A5A5A5, 0x00000001)   # (the patterns of tests/test_gpu_search.py)
SENTINEL_D, SENTINEL_I, PAD = np.float32(-7.25), -77, 64


@pytest.fixture(scope="module")
def gpu():
    import torch
    from pq_huffman_amd import codec
    assert torch.cuda.is_available()
    return torch, codec, codec.Context(0)


@pytest.fixture(scope="module")
def coded(gpu):
    """mode -> (host codes, device codes, tables, device lut, its distances, the radii), once"""
    torch, codec, ctx = gpu
    made = {}

    def get(mode):
        if mode not in made:
            m, k, ctxm = rref.MODES[mode]
            codes = fref.codes_of(mode)
            cd = torch.from_numpy(codes).cuda()
            counts = codec.histogram(ctx, cd, k, ctxm)
            cbs = codec.Codebooks(codec.counts_to_host(counts), k, ctxm)
            lut = rref.lut_of(mode)
            d = sref.dists(lut, codes)
            rad = rref.radii(d)
            rref.check_radii(mode, d, rad)
            made[mode] = (codes, cd, codec.Tables.from_codebooks(ctx, cbs),
                          torch.from_numpy(lut).cuda(), d, rad)
        return made[mode]
    return get


def _bits(a):
    return a.view(np.uint32)


def _host(got):
    return tuple(t.cpu().numpy() for t in got)


def _check(got, want, what=""):
    lims, dist, ids = _host(got)
    assert lims.dtype == np.int64 and dist.dtype == np.float32 and ids.dtype == np.int64
    assert np.array_equal(lims, want[0]), what
    assert np.array_equal(ids, want[2]), what
    assert np.array_equal(_bits(dist), _bits(want[1])), what


def _status(fn):
    from pq_huffman_amd.capi import PqhError
    try:
        fn()
    except PqhError as err:
        return err.status
    return 0


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _words(torch, keep, stale=False):
    return torch.from_numpy(fref.pack(keep, stale)).cuda()


@pytest.mark.parametrize("chunk", rref.CHUNKS)
@pytest.mark.parametrize("mode", list(rref.MODES))
def test_stream_and_codes(gpu, coded, mode, chunk):
    torch, codec, ctx = gpu
    codes, cd, tabs, ld, d, rad = coded(mode)
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=chunk)
    for kind, r in rad.items():
        want = rref.want(d, r)
        rd = _dev(torch, r)
        _check(codec.range_search(ctx, tabs, enc, ld, rd), want, (kind, "stream"))
        _check(codec.range_search_codes(ctx, cd, ld, rd), want, (kind, "codes"))
    # a float is every query's radius
    r = float(rad["median"][0])
    want = rref.want(d, np.full(rref.NQ, r, np.float32))
    _check(codec.range_search(ctx, tabs, enc, ld, r), want)
    _check(codec.range_search_codes(ctx, cd, ld, r), want)
    codec.decode_status(ctx)


@pytest.mark.parametrize("chunk", rref.CHUNKS)
def test_ties_at_the_radius(gpu, coded, chunk):
    torch, codec, ctx = gpu
    _, cd, tabs, _, _, _ = coded("ctx_m8")
    codes, lut, d = rref.ties_case()
    rref.check_ties(d)
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=chunk)
    ld = _dev(torch, lut)
    for r in (8.0, 8.5):
        want = rref.want(d, np.full(rref.NQ, r, np.float32))
        _check(codec.range_search(ctx, tabs, enc, ld, r), want, r)
        _check(codec.range_search_codes(ctx, cd, ld, r), want, r)
    codec.decode_status(ctx)


@pytest.mark.parametrize("mode", list(rref.MODES))
def test_the_same_bits_at_every_grid(gpu, coded, mode):
    torch, codec, ctx = gpu
    codes, cd, tabs, ld, d, rad = coded(mode)
    try:
        for chunk in rref.CHUNKS:
            enc = codec.encode(ctx, tabs, cd, chunk_vectors=chunk)
            for kind in ("median", "mixed"):
                want = rref.want(d, rad[kind])
                rd = _dev(torch, rad[kind])
                for g in rref.GROUPS:
                    ctx.set_tuning(search_groups=g)
                    _check(codec.range_search(ctx, tabs, enc, ld, rd), want, (chunk, kind, g))
                    _check(codec.range_search_codes(ctx, cd, ld, rd), want, (chunk, kind, g))
    finally:
        ctx.set_tuning(search_groups=0)
    codec.decode_status(ctx)


@pytest.mark.parametrize("chunk", rref.CHUNKS)
@pytest.mark.parametrize("mode", ["ctx_m8", "ctx_m16", "noctx_m3"])
def test_masks(gpu, coded, mode, chunk):
    torch, codec, ctx = gpu
    codes, cd, tabs, ld, d, rad = coded(mode)
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=chunk)
    first, last = fref.chunk_end_masks(rref.N, chunk)
    fref.check_chunk_ends(chunk)
    masks = {"half": fref.random_mask(rref.N, 0.5, 11), "first": first, "last": last,
             "zeros": np.zeros(rref.N, bool), "ones": np.ones(rref.N, bool)}
    for kind in ("median", "pos_inf"):
        rd = _dev(torch, rad[kind])
        for name, keep in masks.items():
            want = rref.want(d, rad[kind], keep)
            rref.check_order(want, keep)
            for stale in (False, True):
                kd = _words(torch, keep, stale)
                what = (kind, name, stale)
                _check(codec.range_search(ctx, tabs, enc, ld, rd, keep=kd), want, what)
                _check(codec.range_search_codes(ctx, cd, ld, rd, keep=kd), want, what)
        # keep=None is all ones
        _check(codec.range_search(ctx, tabs, enc, ld, rd, keep=None),
               rref.want(d, rad[kind], masks["ones"]), kind)
    want = rref.want(d, rad["median"], masks["half"], id_base=10 ** 12)
    kd, rd = _words(torch, masks["half"]), _dev(torch, rad["median"])
    _check(codec.range_search(ctx, tabs, enc, ld, rd, keep=kd, id_base=10 ** 12), want)
    _check(codec.range_search_codes(ctx, cd, ld, rd, keep=kd, id_base=10 ** 12), want)
    codec.decode_status(ctx)


def _raw(gpu, src, tabs, enc, cd, ld, rd, capacity, count=True, plan=None, lims=None):
    """the C calls on buffers of this test: outputs of capacity + PAD sentinel entries.
    Returns (plan, lims, dist, ids) as device tensors."""
    from pq_huffman_amd import capi
    torch, codec, ctx = gpu
    lib = capi.lib()
    nq = ld.shape[0]
    if src == "stream":
        head = (tabs.ptr, *codec._index_args(enc))
        shape = (enc.n, tabs.m, tabs.k, enc.chunk_vectors)
    else:
        head = (cd.data_ptr(), cd.shape[0], cd.shape[1], ld.shape[2])
        shape = (cd.shape[0], cd.shape[1], ld.shape[2], 0)
    if plan is None:
        nbytes = ctypes.c_ulonglong(0)
        assert lib.pqh_range_plan_bytes(ctx.ptr, *shape, nq, -1, 0, ctypes.byref(nbytes)) == 0
        assert nbytes.value >= 8 * (nq + 1)
        plan = torch.zeros(nbytes.value // 8 + 1, dtype=torch.int64, device="cuda")
        lims = torch.full((nq + 1,), -5, dtype=torch.int64, device="cuda")
    args = (ctx.ptr, *head, ld.data_ptr(), nq, None, None, -1, 0, rd.data_ptr(), None,
            plan.data_ptr(), plan.numel() * 8, lims.data_ptr())
    if count:
        assert getattr(lib, f"pqh_range_count_{src}")(*args) == 0
    dist = torch.full((capacity + PAD,), float(SENTINEL_D), dtype=torch.float32, device="cuda")
    ids = torch.full((capacity + PAD,), SENTINEL_I, dtype=torch.int64, device="cuda")
    assert getattr(lib, f"pqh_range_fill_{src}")(*args, capacity, 0, dist.data_ptr(),
                                                 ids.data_ptr()) == 0
    return plan, lims, dist, ids


@pytest.mark.parametrize("src", ["stream", "codes"])
def test_capacity(gpu, coded, src):
    """a buffer that is too small holds the first entries of the full result, nothing past
    them is touched, and lims tells the truth"""
    torch, codec, ctx = gpu
    codes, cd, tabs, ld, d, rad = coded("ctx_m16")
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=7)
    want = rref.want(d, rad["median"])
    total = int(want[0][-1])
    rd = _dev(torch, rad["median"])
    assert total == rref.NQ * (rref.N // 2)
    for capacity in (0, int(want[0][3]), total - 1, total, total + 64):
        plan, lims, dist, ids = _raw(gpu, src, tabs, enc, cd, ld, rd, capacity)
        have = min(capacity, total)
        dist, ids = dist.cpu().numpy(), ids.cpu().numpy()
        assert np.array_equal(lims.cpu().numpy(), want[0]), capacity
        assert np.array_equal(ids[:have], want[2][:have]), capacity
        assert np.array_equal(_bits(dist[:have]), _bits(want[1][:have])), capacity
        assert (ids[have:] == SENTINEL_I).all() and (dist[have:] == SENTINEL_D).all(), capacity
        # the Python layer: outputs of that length, (+inf, -1) behind the result, no wait
        fn = codec.range_search if src == "stream" else codec.range_search_codes
        head = (ctx, tabs, enc, ld) if src == "stream" else (ctx, cd, ld)
        got = _host(fn(*head, rd, capacity=capacity))
        assert len(got[1]) == capacity and len(got[2]) == capacity
        assert np.array_equal(got[0], want[0])
        assert np.array_equal(got[2][:have], want[2][:have])
        assert np.array_equal(_bits(got[1][:have]), _bits(want[1][:have]))
        assert (got[2][have:] == -1).all() and np.isposinf(got[1][have:]).all()
    codec.decode_status(ctx)


def test_a_plan_of_another_geometry_is_refused(gpu, coded):
    """counted at search_groups = 1, filled at 3: PQH_ERR_ARG from decode_status, nothing
    written; the fill at the count's tuning then gives the result"""
    torch, codec, ctx = gpu
    codes, cd, tabs, ld, d, rad = coded("ctx_m8")
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=1)
    want = rref.want(d, rad["median"])
    total = int(want[0][-1])
    rd = _dev(torch, rad["median"])
    codec.decode_status(ctx)
    try:
        # (the plan of one group is the larger one: eight waves a workgroup against 3 * 2)
        ctx.set_tuning(search_groups=1)
        plan, lims, dist, ids = _raw(gpu, "stream", tabs, enc, cd, ld, rd, total)
        assert np.array_equal(ids.cpu().numpy()[:total], want[2])
        codec.decode_status(ctx)
        ctx.set_tuning(search_groups=3)
        _, _, dist, ids = _raw(gpu, "stream", tabs, enc, cd, ld, rd, total, count=False,
                               plan=plan, lims=lims)
        assert _status(lambda: codec.decode_status(ctx)) == -1
        assert (ids.cpu().numpy() == SENTINEL_I).all() and (dist.cpu().numpy() == SENTINEL_D).all()
        assert np.array_equal(lims.cpu().numpy(), want[0])
        ctx.set_tuning(search_groups=1)
        _, _, dist, ids = _raw(gpu, "stream", tabs, enc, cd, ld, rd, total, count=False,
                               plan=plan, lims=lims)
        assert np.array_equal(ids.cpu().numpy()[:total], want[2])
        assert np.array_equal(_bits(dist.cpu().numpy()[:total]), _bits(want[1]))
    finally:
        ctx.set_tuning(search_groups=0)
    codec.decode_status(ctx)


@pytest.mark.parametrize("m,K", fref.PROBE_SHAPES)
@pytest.mark.parametrize("chunk", fref.PROBE_CHUNKS)
@pytest.mark.parametrize("context", [True, False])
def test_probe_forms(gpu, context, chunk, m, K):
    torch, codec, ctx = gpu
    case, ptr, ranges = rref.probe_case(m, K, chunk)
    rref.check_probe_case(case, ptr, ranges)
    codes = case[0]
    cd = torch.from_numpy(codes).cuda()
    counts = codec.histogram(ctx, cd, K, context)
    tabs = codec.Tables.from_codebooks(ctx, codec.Codebooks(codec.counts_to_host(counts), K, context))
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=chunk)
    pd, gd = _dev(torch, ptr), _dev(torch, ranges)
    bad = rref.bad_ranges(ranges, ptr, len(codes))
    bd = _dev(torch, bad)
    keep = fref.random_mask(len(codes), 0.5, 21)
    kd = _words(torch, keep)
    codec.decode_status(ctx)
    # a table per query (lut_q), and one per range (lut_pair, NaN where a range has no rows)
    for per_range, lut_dev, lut in ((False, case[3], rref.probe_luts(case)[0]),
                                    (True, case[4], rref.probe_luts(case)[1])):
        ld = _dev(torch, lut_dev)
        for name, r in rref.probe_radii(lut, codes, ptr, ranges).items():
            rd = _dev(torch, r)
            what = (per_range, name)
            want = rref.want_ranges(lut, codes, ptr, ranges, r)
            _check(codec.range_search_ranges(ctx, tabs, enc, ld, pd, gd, rd, per_range), want, what)
            _check(codec.range_search_codes_ranges(ctx, cd, ld, pd, gd, rd, per_range), want, what)
            want = rref.want_ranges(lut, codes, ptr, ranges, r, keep=keep, id_base=5)
            _check(codec.range_search_ranges(ctx, tabs, enc, ld, pd, gd, rd, per_range, keep=kd,
                                             id_base=5), want, what)
            _check(codec.range_search_codes_ranges(ctx, cd, ld, pd, gd, rd, per_range, keep=kd,
                                                   id_base=5), want, what)
            codec.decode_status(ctx)
            # a bad range: reported, skipped, and no other query the worse for it
            want = rref.want_ranges(lut, codes, ptr, bad, r)
            got = codec.range_search_ranges(ctx, tabs, enc, ld, pd, bd, rd, per_range)
            assert _status(lambda: codec.decode_status(ctx)) == -1
            _check(got, want, what)
            got = codec.range_search_codes_ranges(ctx, cd, ld, pd, bd, rd, per_range)
            assert _status(lambda: codec.decode_status(ctx)) == -1
            _check(got, want, what)
    codec.decode_status(ctx)


def test_after_lds_poison(gpu, coded):
    """every CU's LDS filled with a pattern first: a read of LDS the kernel did not write
    (the window's pad, a stage slot, a table entry) shows as a wrong result"""
    from pq_huffman_amd.capi import lib
    torch, codec, ctx = gpu
    codes, cd, tabs, ld, d, rad = coded("ctx_m8")
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=7)
    want = rref.want(d, rad["mixed"])
    rd = _dev(torch, rad["mixed"])
    for value in POISON:
        assert lib().pqh_debug_poison_lds(ctx.ptr, ctypes.c_uint(value)) == 0
        _check(codec.range_search(ctx, tabs, enc, ld, rd), want, hex(value))
        assert lib().pqh_debug_poison_lds(ctx.ptr, ctypes.c_uint(value)) == 0
        _check(codec.range_search_codes(ctx, cd, ld, rd), want, hex(value))
    codec.decode_status(ctx)


# ------------------------------------------------------------------------------ the index
@pytest.fixture(scope="module")
def world(gpu):
    torch, codec, ctx = gpu
    w = fref.ivf_world()
    rref.check_ivf(w)
    w.update(xd=torch.from_numpy(w["x"]).cuda(), qd=torch.from_numpy(w["q"]).cuda(),
             pq=codec.PQ(ctx, w["cent"]), coarse=codec.Coarse(ctx, w["cc"]))
    return w


@pytest.mark.parametrize("kind", ["plain", "residual"])
def test_ivf_range_search(gpu, world, kind):
    """N, NLIST, M, NQ = 1003, 13, 8, 9 (search_filter_ref.ivf_world): the index as built, with
    keep=, after remove(), after add() and after compact(), against the numpy references"""
    torch, codec, ctx = gpu
    w = world
    nprobe = fref.IVF_NPROBE
    ivf = codec.IVF.build(ctx, w["pq"], w["coarse"], w["xd"][:600], chunk_vectors=7,
                          residual=kind == "residual")
    ivf.add(w["xd"][600:])                                # (the index build() makes of all rows)
    codec.ivf_status(ctx)
    assert np.array_equal(ivf.perm.cpu().numpy(), w["perm"])
    assert np.array_equal(codec.decode(ctx, ivf.tables, ivf.enc).cpu().numpy(), w[kind]["codes"])
    rad = rref.ivf_radii(w, kind)
    rd = _dev(torch, rad)
    keep = torch.from_numpy(w["keep"]).cuda()
    _check(ivf.range_search(w["qd"], nprobe, rd), rref.ivf_want(w, kind, rad))
    _check(ivf.range_search(w["qd"], nprobe, rd, keep=keep), rref.ivf_want(w, kind, rad, w["keep"]))
    r = float(rad[6])                                     # one radius for all
    _check(ivf.range_search(w["qd"], nprobe, r),
           rref.ivf_want(w, kind, np.full(fref.IVF_NQ, r, np.float32)))
    if kind == "residual":                                # slabs of two queries
        ivf.table_budget = 2 * nprobe * fref.IVF_M * 256 * 4
        _check(ivf.range_search(w["qd"], nprobe, rd, keep=keep),
               rref.ivf_want(w, kind, rad, w["keep"]), "slabs")
        del ivf.table_budget

    # the top-k search agrees: its entries below the radius are the head of the range result
    # in its own order, (dist, stream row)
    top = _host(ivf.search(w["qd"], nprobe, 64))
    heads = rref.topk_of(_host(ivf.range_search(w["qd"], nprobe, rd)), rref.inverse(w["perm"]))
    for q, (hd, hi) in enumerate(heads):
        below = top[0][q] < rad[q]
        assert below.sum() == min(64, len(hd)) == len(hi)
        assert np.array_equal(top[1][q][below], hi), q
        assert np.array_equal(_bits(top[0][q][below]), _bits(hd)), q

    # remove the rows of query 8's result (the longest), with and without keep=
    gone = rref.ivf_want(w, kind, rad)
    gone = np.unique(gone[2][gone[0][8]:gone[0][9]])
    assert len(gone) > 64
    ivf.remove(torch.from_numpy(gone).cuda())
    got = ivf.range_search(w["qd"], nprobe, rd)
    assert not np.isin(got[2].cpu().numpy(), gone).any()
    _check(got, rref.ivf_want(w, kind, rad, removed=gone))
    _check(ivf.range_search(w["qd"], nprobe, rd, keep=keep),
           rref.ivf_want(w, kind, rad, w["keep"], removed=gone))
    # compact(): the same hits from the shorter stream, the ids what they were
    assert ivf.compact() == len(gone)
    assert ivf.perm.numel() == fref.IVF_N - len(gone)
    _check(ivf.range_search(w["qd"], nprobe, rd), rref.ivf_want(w, kind, rad, removed=gone))
    _check(ivf.range_search(w["qd"], nprobe, rd, keep=keep),
           rref.ivf_want(w, kind, rad, w["keep"], removed=gone))
    codec.decode_status(ctx)
    codec.ivf_status(ctx)


def test_nothing_to_scan(gpu, coded):
    """nq == 0, n == 0 and nr == 0: lims of zeros and empty outputs"""
    torch, codec, ctx = gpu
    codes, cd, tabs, ld, d, rad = coded("ctx_m8")
    got = _host(codec.range_search_codes(ctx, cd[:0], ld, 1.0))
    assert np.array_equal(got[0], np.zeros(rref.NQ + 1, np.int64)) and len(got[1]) == len(got[2]) == 0
    got = _host(codec.range_search_codes(ctx, cd, ld[:0], 1.0))
    assert np.array_equal(got[0], [0]) and len(got[1]) == 0
    ptr = torch.zeros(rref.NQ + 1, dtype=torch.int64, device="cuda")
    none = torch.zeros((0, 2), dtype=torch.int64, device="cuda")
    got = _host(codec.range_search_codes_ranges(ctx, cd, ld, ptr, none, 1.0))
    assert np.array_equal(got[0], np.zeros(rref.NQ + 1, np.int64)) and len(got[2]) == 0
    codec.decode_status(ctx)
