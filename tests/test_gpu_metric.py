"""The inner-product metric on the GPU, call by call: pqh_adc_tables_ip, pqh_coarse_assign_ip,
pqh_coarse_probe_ip, pqh_adc_tables_residual_ip (codec's metric="ip") and pqh_refine_*_ip
(codec.refine_ip).
Expected values come from numpy (tests/metric_ref.py), never from the calls under test: floats
are compared on their raw bits, ids with array_equal, and every output is a slice of a poisoned
buffer whose other words must come back as they were."""
import ctypes

import numpy as np
import pytest

import ivf_ref
import metric_ref as mr
import refine_ref as rr
import search_wide_ref as wref

pytestmark = pytest.mark.gpu

POISON = (0xFFFFFFFF, 0xA5A5A5A5, 0x00000001)   # (the patterns of tests/test_gpu_search.py)


@pytest.fixture(scope="module")
def gpu():
    """a context whose limit was raised: calls up to 64 launch what they launch on any context"""
    import torch
    from pq_huffman_amd import codec
    assert torch.cuda.is_available()
    return torch, codec, codec.Context(0).set_search_max_k(256)


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


def _signed(value):
    return value - (1 << 32) if value >= 1 << 31 else value


def _poisoned(torch, shape, dtype, value):
    """a device tensor whose every 32-bit word is `value`"""
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.int32).fill_(_signed(value))
    return t


def _untouched(t, value):
    """every 32-bit word of the host array t is still the poison"""
    return (np.ascontiguousarray(t).view(np.uint32) == value).all()


def _gapped(torch, a, pad):
    """a on the device, its rows `pad` NaN floats apart"""
    n, d = a.shape
    wide = np.full((max(n, 1), d + pad), np.nan, np.float32)
    wide[:n, :d] = a
    return torch.from_numpy(wide).cuda()[:n, :d]


def _check(got, want, what=""):
    gd, gi = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert gd.dtype == np.float32 and gi.dtype == np.int64
    assert np.array_equal(gi, want[1]), what
    assert np.array_equal(_bits(gd), _bits(want[0])), what


# ------------------------------------------------------------------------------ tables
@pytest.mark.parametrize("m,k,dsub", [(1, 2, 1), (8, 256, 16), (16, 256, 6), (3, 17, 5)])
def test_tables(gpu, m, k, dsub):
    torch, codec, ctx = gpu
    rng = np.random.default_rng(100 * m + k + dsub)
    cent = rng.normal(0.0, 20.0, size=(m, k, dsub)).astype(np.float32)
    q = rng.normal(0.0, 30.0, size=(3, m * dsub)).astype(np.float32)
    q[0, 0] = 0.0                                             # a product that is a zero
    qd = _gapped(torch, q, 3)
    pq = codec.PQ(ctx, cent)
    for case, nq in enumerate((1, 3)):
        want = mr.tables(q[:nq], cent)
        assert not np.isnan(want).any()
        value = POISON[(case + m) % 3]
        out = _poisoned(torch, (nq + 1, m, k), torch.float32, value)
        got = codec.adc_tables(ctx, pq, qd[:nq], out=out[:nq], metric="ip")
        host = out.cpu().numpy()
        assert np.array_equal(_bits(host[:nq]), _bits(want)), nq
        assert _untouched(host[nq], value)
        assert got.data_ptr() == out.data_ptr()
    # out = None, and the default metric is the L2 table of before
    got = codec.adc_tables(ctx, pq, qd, metric="ip")
    assert got.shape == (3, m, k) and np.array_equal(_bits(got.cpu().numpy()), _bits(mr.tables(q, cent)))
    l2 = np.stack([ivf_ref.dists(q[:, i * dsub:(i + 1) * dsub], cent[i]) for i in range(m)], axis=1)
    assert np.array_equal(_bits(codec.adc_tables(ctx, pq, qd).cpu().numpy()), _bits(l2))
    assert np.array_equal(_bits(codec.adc_tables(ctx, pq, qd, metric="l2").cpu().numpy()), _bits(l2))
    pq.close()


# ------------------------------------------------------------------------------ assignment
# (n, nlist, d): one row, one list, one dimension; each side of a tile of 128 rows, of 128
# centroids and of 32 staged dimensions; several tiles and stages
ASSIGN = [(1, 1, 1), (127, 127, 31), (128, 129, 32), (129, 300, 33), (300, 129, 100), (300, 1, 33),
          (1, 300, 32)]


@pytest.mark.parametrize("n,nlist,d", ASSIGN)
def test_assign(gpu, n, nlist, d):
    """rows ld_x > d apart with NaN between them; list and score outputs inside poisoned buffers"""
    torch, codec, ctx = gpu
    rng = np.random.default_rng(n + 7 * nlist + d)
    x = rng.normal(0.0, 30.0, size=(n, d)).astype(np.float32)
    c = rng.normal(0.0, 30.0, size=(nlist, d)).astype(np.float32)
    cq = codec.Coarse(ctx, c)
    want_l, want_s = mr.assign(x, c)
    value = POISON[n % 3]
    lists = _poisoned(torch, (n + 2,), torch.int32, value)
    score = _poisoned(torch, (n + 2,), torch.float32, value)
    got = cq.assign(_gapped(torch, x, 3), out=lists[1:n + 1], dist=score[1:n + 1], metric="ip")
    assert got.data_ptr() == lists[1:].data_ptr()
    hl, hs = lists.cpu().numpy(), score.cpu().numpy()
    assert np.array_equal(hl[1:n + 1], want_l)
    assert np.array_equal(_bits(hs[1:n + 1]), _bits(want_s))
    assert _untouched(hl[[0, n + 1]], value) and _untouched(hs[[0, n + 1]], value)
    # without the score, into a fresh tensor
    assert np.array_equal(cq.assign(_gapped(torch, x, 1), metric="ip").cpu().numpy(), want_l)
    if nlist > 1 and n > 1:
        assert not np.array_equal(want_l, ivf_ref.assign(x, c)[0])     # not the L2 answer
    codec.ivf_status(ctx)
    cq.close()


def test_assign_ties_go_to_the_smaller_list(gpu):
    """an integer grid, every sum exact: rows with several maxima, in one tile and across tiles"""
    torch, codec, ctx = gpu
    x, c = ivf_ref.integer_grid(300, 5, 300, seed=12)
    c[150:] = c[:150]                  # every centroid twice, 150 apart: never in the same tile
    c[140] = c[3]
    exact = mr.nip_int64(x, c)
    ties = (exact == exact.min(axis=1, keepdims=True)).sum(axis=1)
    first = np.array([np.flatnonzero(exact[v] == exact[v].min())[0] for v in range(300)])
    assert (ties > 1).all() and (ties > 2).any() and (first < 150).all() and (first >= 128).any()
    cq = codec.Coarse(ctx, c)
    score = torch.empty(300, dtype=torch.float32, device="cuda")
    lists = cq.assign(torch.from_numpy(x).cuda(), dist=score, metric="ip").cpu().numpy()
    assert np.array_equal(lists, first) and np.array_equal(lists, mr.assign(x, c)[0])
    assert np.array_equal(score.cpu().numpy().astype(np.int64), exact.min(axis=1))
    codec.ivf_status(ctx)
    cq.close()


# ------------------------------------------------------------------------------ probe
def _probe_case(gpu, q, c, nprobe, offsets, value, what):
    torch, codec, ctx = gpu
    cq = codec.Coarse(ctx, c)
    want = mr.probe(q, c, nprobe, offsets)
    got = cq.probe(_gapped(torch, q, 5), nprobe, torch.from_numpy(offsets).cuda(), metric="ip")
    for g, w, name in zip(got, want, ("range_ptr", "ranges", "probes", "probe_dist")):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        assert np.array_equal(_bits(g), _bits(w)) if name == "probe_dist" else np.array_equal(g, w), \
            (what, name)
    # the raw call: the optional outputs left out, the others inside poisoned buffers
    from pq_huffman_amd.capi import lib
    nq = q.shape[0]
    ptr = _poisoned(torch, (nq + 2,), torch.int64, value)
    ranges = _poisoned(torch, (nq * nprobe + 1, 2), torch.int64, value)
    qd, od = torch.from_numpy(q).cuda(), torch.from_numpy(offsets).cuda()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib().pqh_coarse_probe_ip(ctx.ptr, cq.ptr, p(qd), nq, q.shape[1], nprobe, p(od), p(ptr),
                                     p(ranges), None, None) == 0
    hp, hr = ptr.cpu().numpy(), ranges.cpu().numpy()
    assert np.array_equal(hp[:nq + 1], want[0]) and _untouched(hp[nq + 1:], value), what
    assert np.array_equal(hr[:-1], want[1]) and _untouched(hr[-1], value), what
    if nprobe == 1:          # the probe's score is the assignment's, bit for bit
        score = torch.empty(nq, dtype=torch.float32, device="cuda")
        lists = cq.assign(qd, dist=score, metric="ip")
        assert torch.equal(lists.long(), got[2][:, 0]), what
        assert torch.equal(score.view(torch.int32), got[3][:, 0].contiguous().view(torch.int32)), what
    codec.ivf_status(ctx)
    cq.close()
    return want


@pytest.mark.parametrize("nlist", [1, 64, 65, 1025])
def test_probe(gpu, nlist):
    """nprobe 1 and 64 (more than nlist at 1: the padding); floats of d = 33, and an integer grid
    of d = 5 whose many equal scores must come out in list order"""
    rng = np.random.default_rng(nlist)
    sizes = rng.integers(0, 5, size=nlist)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    q = rng.normal(0.0, 30.0, size=(3, 33)).astype(np.float32)
    c = rng.normal(0.0, 30.0, size=(nlist, 33)).astype(np.float32)
    qi, ci = ivf_ref.integer_grid(3, 5, nlist, seed=nlist + 1)
    if nlist > 1:
        ci[nlist - 1] = ci[0]                                  # a certain tie, far apart
    for case, nprobe in enumerate((1, 64)):
        _probe_case(gpu, q, c, nprobe, offsets, POISON[case], (nlist, nprobe, "float"))
        want = _probe_case(gpu, qi, ci, nprobe, offsets, POISON[2], (nlist, nprobe, "grid"))
        if nprobe > nlist:
            assert (want[2][:, nlist:] == -1).all() and np.isposinf(want[3][:, nlist:]).all()
            assert (want[1].reshape(3, nprobe, 2)[:, nlist:] == 0).all()
        if nprobe == 64 and nlist >= 64:
            tie = (want[3][:, 1:] == want[3][:, :-1]) & (want[2][:, 1:] >= 0)
            assert tie.sum() > 10 and (want[2][:, 1:][tie] > want[2][:, :-1][tie]).all()


# ------------------------------------------------------------------------------ residual tables
@pytest.mark.parametrize("m,k,dsub", [(8, 256, 16), (13, 17, 10), (16, 256, 8)])
def test_residual_tables(gpu, m, k, dsub):
    """d = 128 and d = 130; the probes are the probe selection's own (with its -1 padding,
    nprobe > nlist) and then hand-made ones: repeated lists, -1, 257 probes (two rounds of the
    workgroup).  The bias is the probe's score on every bit."""
    torch, codec, ctx = gpu
    d, nlist, nq = m * dsub, 11, 3
    rng = np.random.default_rng(m * 1000 + k + dsub)
    cent = rng.normal(0.0, 20.0, size=(m, k, dsub)).astype(np.float32)
    c = rng.normal(0.0, 30.0, size=(nlist, d)).astype(np.float32)
    q = rng.normal(0.0, 30.0, size=(nq, d)).astype(np.float32)
    qd = _gapped(torch, q, 3)
    pq, cq = codec.PQ(ctx, cent), codec.Coarse(ctx, c)
    offsets = torch.arange(nlist + 1, dtype=torch.int64, device="cuda")
    plain = codec.adc_tables(ctx, pq, qd, metric="ip").cpu().numpy()
    for case, nprobe in enumerate((1, 5, 16)):
        _, _, probes, pdist = cq.probe(qd, nprobe, offsets, metric="ip")
        hp, hd = probes.cpu().numpy(), pdist.cpu().numpy()
        want = mr.tables_residual(q, c, hp, cent)
        value = POISON[case]
        out = _poisoned(torch, (nq * nprobe + 1, m, k), torch.float32, value)
        got = codec.adc_tables_residual(ctx, pq, cq, qd, probes, out=out[:-1], metric="ip")
        host = out.cpu().numpy()
        assert np.array_equal(_bits(host[:-1]), _bits(want)), nprobe
        assert _untouched(host[-1], value)
        assert got.data_ptr() == out.data_ptr()
        # part 0 = the probe's own score + the plain table, the other parts the plain table
        lut = host[:-1].reshape(nq, nprobe, m, k)
        live = hp >= 0
        assert (live.sum(axis=1) == min(nprobe, nlist)).all()
        part0 = hd[:, :, None] + plain[:, None, 0, :]
        assert part0.dtype == np.float32
        assert np.array_equal(_bits(lut[:, :, 0][live]), _bits(part0[live]))
        rest = np.broadcast_to(plain[:, None, 1:], lut[:, :, 1:].shape)
        assert np.array_equal(_bits(lut[:, :, 1:][live]), _bits(rest[live]))
        assert np.isposinf(lut[~live]).all()
    for nprobe in (4, 257):
        probes = rng.integers(0, nlist, size=(nq, nprobe)).astype(np.int64)
        probes[:, 1] = -1
        probes[:, -1] = probes[:, 0]
        probes[nq - 1, 2:] = -1
        want = mr.tables_residual(q, c, probes, cent)
        got = codec.adc_tables_residual(ctx, pq, cq, qd, torch.from_numpy(probes).cuda(), metric="ip")
        assert got.shape == (nq * nprobe, m, k)
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), nprobe
    codec.ivf_status(ctx)
    # a list that does not exist: a table of +inf and the sticky error, once
    for bad in (nlist, -2, 2 ** 40):
        probes = np.array([[0, 1], [bad, 2], [3, 3]], np.int64)
        got = codec.adc_tables_residual(ctx, pq, cq, qd, torch.from_numpy(probes).cuda(), metric="ip")
        assert _status(lambda: codec.ivf_status(ctx)) == -1                    # PQH_ERR_ARG
        want = mr.tables_residual(q, c, probes, cent)
        assert np.isposinf(want[2]).all() and np.isfinite(want[3]).all()
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))
        codec.ivf_status(ctx)
    pq.close()
    cq.close()


# ------------------------------------------------------------------------------ re-rank
def _encode(gpu, codes, k, context, chunk):
    torch, codec, ctx = gpu
    cd = torch.from_numpy(codes).cuda()
    tabs = codec.Tables(ctx, codes.shape[1], k, context).build(codec.histogram(ctx, cd, k, context))
    return tabs, codec.encode(ctx, tabs, cd, chunk_vectors=chunk)


def _out(torch, nq, k, value):
    """a (dist, ids) pair whose rows lie k + 3 apart inside poisoned buffers"""
    return (_poisoned(torch, (nq, k + 3), torch.float32, value),
            _poisoned(torch, (nq, k + 3), torch.int64, value))


def _refine_check(gpu, levels, qd, rows, k, want, value, what, **kw):
    torch, codec, ctx = gpu
    nq = rows.shape[0]
    bd, bi = _out(torch, nq, k, value)
    got = codec.refine_ip(ctx, *levels, qd[:nq], torch.from_numpy(np.ascontiguousarray(rows)).cuda(),
                          k, out=(bd[:, :k], bi[:, :k]), **kw)
    _check(got, want, what)
    assert _untouched(bd.cpu().numpy()[:, k:], value), what
    assert _untouched(bi.cpu().numpy()[:, k:], value), what


# (m1, dsub1, m2, dsub2), K: the 16-byte loads; m1 != m2 and a dsub of 2; dsub 5 and 3
@pytest.mark.parametrize("shape,k", [((8, 4, 8, 4), 256), ((8, 4, 16, 2), 256), ((3, 5, 5, 3), 16)])
def test_refine_plain(gpu, shape, k):
    """refine_ref's candidates: the raw row, the last row, chunk ends, a duplicate, -1s.  The
    stream form and the codes form against numpy, so against each other"""
    torch, codec, ctx = gpu
    w = rr.sweep_world(shape, k)
    pq1, pq2 = codec.PQ(ctx, w["cent1"]), codec.PQ(ctx, w["cent2"])
    chunks = (4, 7)
    t1, e1 = _encode(gpu, w["codes1"], k, k == 256, chunks[0])
    t2, e2 = _encode(gpu, w["codes2"], k, False, chunks[1])
    forms = {"codes": ((pq1, torch.from_numpy(w["codes1"]).cuda()),
                       (pq2, torch.from_numpy(w["codes2"]).cuda())),
             "stream": ((t1, pq1, e1), (t2, pq2, e2))}
    qd = _gapped(torch, w["q"], 3)
    for case, (nq, ncand, top_k) in enumerate(((1, 1, 1), (5, 64, 64), (5, 64, 10), (5, 200, 200),
                                                 (1, 200, 1))):
        rows = rr.candidates(nq, ncand, chunks, 17 * nq + ncand)
        rr.check_candidates(rows, chunks)
        want = mr.refine(w["q"][:nq], rows, top_k, w["cent1"], w["codes1"], w["cent2"], w["codes2"])
        assert np.isfinite(want[0][:, 0]).all()
        l2 = rr.refine(w["q"][:nq], rows, top_k, w["cent1"], w["codes1"], w["cent2"], w["codes2"])
        assert not np.array_equal(want[0], l2[0])
        for name, levels in forms.items():
            _refine_check(gpu, levels, qd, rows, top_k, want, POISON[case % 3],
                          (shape, nq, ncand, top_k, name))
    codec.decode_status(ctx)                                  # -1 and a duplicate are no errors
    for h in (pq1, pq2):
        h.close()


@pytest.mark.parametrize("d", [15, 128])
def test_refine_residual(gpu, d):
    """37 lists, several of them empty: the centroid of the row's list is added to the
    reconstruction; up to 64 candidates and 200"""
    torch, codec, ctx = gpu
    w = rr.residual_world(d)
    wide = wref.residual_rows(w)
    wref.check_residual_rows(w, wide)
    pq1, pq2 = codec.PQ(ctx, w["cent1"]), codec.PQ(ctx, w["cent2"])
    t1, e1 = _encode(gpu, w["codes1"], 256, True, 4)
    t2, e2 = _encode(gpu, w["codes2"], 256, True, 7)
    forms = {"codes": ((pq1, torch.from_numpy(w["codes1"]).cuda()),
                       (pq2, torch.from_numpy(w["codes2"]).cuda())),
             "stream": ((t1, pq1, e1), (t2, pq2, e2))}
    cq = codec.Coarse(ctx, w["coarse"])
    od = torch.from_numpy(w["offsets"]).cuda()
    qd = _gapped(torch, w["q"], 1)
    for case, (rows, top_k) in enumerate(((w["rows"], 10), (w["rows"], w["rows"].shape[1]),
                                           (wide, 200), (wide[:, :1], 1))):
        want = mr.refine(w["q"], rows, top_k, w["cent1"], w["codes1"], w["cent2"], w["codes2"],
                         w["coarse"], w["offsets"])
        plain = mr.refine(w["q"], rows, top_k, w["cent1"], w["codes1"], w["cent2"], w["codes2"])
        assert not np.array_equal(want[0], plain[0])          # the centroid matters
        for name, levels in forms.items():
            _refine_check(gpu, levels, qd, rows, top_k, want, POISON[case % 3],
                          (d, rows.shape[1], top_k, name), coarse=cq, offsets=od)
    codec.decode_status(ctx)
    # a row outside the stream is dropped and reported, as by the L2 form
    bad = w["rows"].copy()
    bad[1, 5] = rr.N
    want = mr.refine(w["q"], bad, 10, w["cent1"], w["codes1"], w["cent2"], w["codes2"],
                     w["coarse"], w["offsets"])
    _refine_check(gpu, forms["stream"], qd, bad, 10, want, POISON[0], "bad row", coarse=cq, offsets=od)
    assert _status(lambda: codec.decode_status(ctx)) == -1
    codec.decode_status(ctx)
    for h in (pq1, pq2, cq):
        h.close()


# ------------------------------------------------------------------------------ argument errors
def test_argument_errors(gpu):
    torch, codec, ctx = gpu
    from pq_huffman_amd.capi import lib
    rng = np.random.default_rng(77)
    m, k, dsub, nlist = 4, 16, 8, 5
    cent = rng.normal(0.0, 20.0, size=(m, k, dsub)).astype(np.float32)
    c = rng.normal(0.0, 30.0, size=(nlist, 32)).astype(np.float32)
    qd = torch.from_numpy(rng.normal(0.0, 30.0, size=(3, 33)).astype(np.float32)).cuda()
    pq, cq = codec.PQ(ctx, cent), codec.Coarse(ctx, c)
    pd = torch.from_numpy(np.array([[0, 4], [1, 1], [2, 3]], np.int64)).cuda()
    offsets = torch.arange(nlist + 1, dtype=torch.int64, device="cuda")
    # an unknown metric, at every entry
    for fn in (lambda: codec.adc_tables(ctx, pq, qd, metric="cosine"),
               lambda: codec.adc_tables_residual(ctx, pq, cq, qd, pd, metric="IP"),
               lambda: cq.assign(qd, metric="dot"),
               lambda: cq.probe(qd, 2, offsets, metric=""),
               lambda: codec.IVF.build(ctx, pq, cq, qd[:, :32], metric="mips")):
        assert _status(fn) == -1
    # pq's m * dsub must be the coarse quantizer's d
    other = codec.Coarse(ctx, rng.normal(0.0, 30.0, size=(nlist, 33)).astype(np.float32))
    assert _status(lambda: codec.adc_tables_residual(ctx, pq, other, qd, pd, metric="ip")) == -1
    assert _status(lambda: codec.IVF.build(ctx, pq, other, qd, metric="ip")) == -1
    other.close()
    # K > 256
    big = codec.PQ(ctx, rng.normal(0.0, 20.0, size=(4, 4096, 8)).astype(np.float32))
    assert _status(lambda: codec.adc_tables(ctx, big, qd, metric="ip")) == -4   # UNSUPPORTED
    assert _status(lambda: codec.adc_tables_residual(ctx, big, cq, qd, pd, metric="ip")) == -4
    assert _status(lambda: codec.IVF.build(ctx, big, cq, qd[:, :32], metric="ip")) == -4
    big.close()
    # the raw calls: rows closer than d floats, no probes, a null quantizer
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    out = torch.empty((6, m, k), dtype=torch.float32, device="cuda")
    li = torch.empty(3, dtype=torch.int32, device="cuda")
    L = lib()
    assert L.pqh_adc_tables_ip(ctx.ptr, pq.ptr, p(qd), 3, 31, p(out)) == -1
    assert L.pqh_adc_tables_residual_ip(ctx.ptr, pq.ptr, cq.ptr, p(qd), 3, 31, p(pd), 2, p(out)) == -1
    assert L.pqh_adc_tables_residual_ip(ctx.ptr, pq.ptr, cq.ptr, p(qd), 3, 33, p(pd), 0, p(out)) == -1
    assert L.pqh_adc_tables_residual_ip(ctx.ptr, pq.ptr, None, p(qd), 3, 33, p(pd), 2, p(out)) == -1
    assert L.pqh_coarse_assign_ip(ctx.ptr, cq.ptr, p(qd), 3, 31, p(li), None) == -1
    assert L.pqh_coarse_assign_ip(ctx.ptr, None, p(qd), 3, 33, p(li), None) == -1
    assert _status(lambda: cq.probe(qd, 0, offsets, metric="ip")) == -1
    assert _status(lambda: cq.probe(qd, 65, offsets, metric="ip")) == -1
    # nothing to do launches nothing and is no error
    assert L.pqh_adc_tables_ip(ctx.ptr, pq.ptr, None, 0, 33, None) == 0
    assert L.pqh_coarse_assign_ip(ctx.ptr, cq.ptr, None, 0, 33, None, None) == 0
    assert L.pqh_adc_tables_residual_ip(ctx.ptr, pq.ptr, cq.ptr, None, 0, 33, None, 2, None) == 0
    codec.ivf_status(ctx)
    codec.decode_status(ctx)
    pq.close()
    cq.close()
