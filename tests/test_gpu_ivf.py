"""The inverted-file front end on the GPU: pqh_coarse_assign, pqh_ivf_layout, pqh_coarse_probe
and codec.IVF from vectors and queries to neighbour ids.  Expected values come from numpy
(tests/ivf_ref.py and this file), never from the calls under test: distances are compared on
their raw float bits, ids with array_equal."""
import ctypes

import numpy as np
import pytest

import datagen
import ivf_ref

pytestmark = pytest.mark.gpu

POISON = (0xFFFFFFFF, 0xA5A5A5A5, 0x00000001)   # (the patterns of tests/test_gpu_search.py)
NS = (1, 63, 1003)
DS = (1, 5, 96, 128, 130)
NLISTS = (1, 3, 70, 257, 1030)


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


def _check_assign(gpu, cq, xd, want_lists, want_dist, what, value=POISON[0]):
    torch, codec, ctx = gpu
    n = xd.shape[0]
    out = _poisoned(torch, (n,), torch.int32, value)
    dist = _poisoned(torch, (n,), torch.float32, value)
    got = cq.assign(xd, out=out, dist=dist)
    assert got is out
    assert np.array_equal(out.cpu().numpy(), want_lists), what
    assert np.array_equal(_bits(dist.cpu().numpy()), _bits(want_dist)), what


# ------------------------------------------------------------------------------ assign
@pytest.mark.parametrize("d", DS)
def test_assign_sweep(gpu, d):
    """every n, nlist of the sweep at this d: d odd, nlist no multiple of a tile, one list,
    more than one workgroup (1003 rows) and more than one centroid tile (257, 1030 lists)"""
    torch, codec, ctx = gpu
    rng = np.random.default_rng(1000 + d)
    x = rng.normal(0.0, 30.0, size=(max(NS), d)).astype(np.float32)
    c = rng.normal(0.0, 30.0, size=(max(NLISTS), d)).astype(np.float32)
    dist = ivf_ref.dists(x, c)          # once: a subset's distances are a slice of it
    xd = torch.from_numpy(x).cuda()
    for i, nlist in enumerate(NLISTS):
        cq = codec.Coarse(ctx, c[:nlist])
        assert (cq.nlist, cq.d) == (nlist, d)
        wl, wd = ivf_ref.assign(None, None, dist[:, :nlist])
        for n in NS:
            _check_assign(gpu, cq, xd[:n], wl[:n], wd[:n], (d, nlist, n), POISON[i % 3])
        # d_dist = NULL
        assert np.array_equal(cq.assign(xd[:63]).cpu().numpy(), wl[:63]), (d, nlist)
        cq.close()
    codec.ivf_status(ctx)


def test_assign_rows_apart_with_nan_between(gpu):
    """ld_x = d + 3 and the three floats between rows NaN: they are not read"""
    torch, codec, ctx = gpu
    rng = np.random.default_rng(5)
    n, d, nlist = 1003, 130, 257
    x = rng.normal(0.0, 10.0, size=(n, d)).astype(np.float32)
    c = rng.normal(0.0, 10.0, size=(nlist, d)).astype(np.float32)
    wide = np.full((n, d + 3), np.nan, np.float32)
    wide[:, :d] = x
    xd = torch.from_numpy(wide).cuda()[:, :d]
    assert xd.stride(0) == d + 3
    cq = codec.Coarse(ctx, c)
    wl, wd = ivf_ref.assign(x, c)
    assert not np.isnan(wd).any()
    _check_assign(gpu, cq, xd, wl, wd, "ld_x")
    cq.close()


@pytest.mark.parametrize("d,nlist", [(5, 257), (96, 1030), (2, 70)])
def test_assign_ties_on_the_integer_grid(gpu, d, nlist):
    """integers in [-8, 8]: every sum exact in fp32 and many lists at the same distance, so
    the first of them has to win"""
    torch, codec, ctx = gpu
    x, c = ivf_ref.integer_grid(1003, d, nlist, seed=d)
    dist = ivf_ref.dists(x, c)
    assert np.array_equal(dist.astype(np.int64), ivf_ref.dists_int64(x, c))
    tied = ((dist == dist.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum()
    if d <= 5:          # (the input's own property: rows whose minimum is shared by several lists)
        assert tied >= 20
    wl, wd = ivf_ref.assign(x, c, dist)
    cq = codec.Coarse(ctx, c)
    _check_assign(gpu, cq, torch.from_numpy(x).cuda(), wl, wd, (d, nlist))
    cq.close()


def test_assign_never_picks_the_copy_of_a_list(gpu):
    torch, codec, ctx = gpu
    rng = np.random.default_rng(8)
    n, d, nlist = 1003, 96, 70
    c = rng.normal(0.0, 10.0, size=(nlist, d)).astype(np.float32)
    c[7] = c[3]
    x = rng.normal(0.0, 10.0, size=(n, d)).astype(np.float32)
    x[::5] = c[3] + rng.normal(0.0, 1.0, size=(len(x[::5]), d)).astype(np.float32)
    wl, wd = ivf_ref.assign(x, c)
    assert (wl == 3).sum() >= 200 and not (wl == 7).any()
    cq = codec.Coarse(ctx, c)
    _check_assign(gpu, cq, torch.from_numpy(x).cuda(), wl, wd, "copy")
    got = cq.assign(torch.from_numpy(x).cuda()).cpu().numpy()
    assert not (got == 7).any()
    cq.close()


# ------------------------------------------------------------------------------ layout
def _layout(gpu, ids, nlist, value=POISON[1]):
    from pq_huffman_amd.capi import check, lib
    torch, codec, ctx = gpu
    idd = torch.from_numpy(np.asarray(ids, np.int32)).cuda()
    perm = _poisoned(torch, (len(ids),), torch.int64, value)
    offsets = _poisoned(torch, (nlist + 1,), torch.int64, value)
    check(lib().pqh_ivf_layout(ctx.ptr, ctypes.c_void_p(idd.data_ptr()), len(ids), nlist,
                               ctypes.c_void_p(perm.data_ptr()) if len(ids) else None,
                               ctypes.c_void_p(offsets.data_ptr())), "pqh_ivf_layout")
    return perm.cpu().numpy(), offsets.cpu().numpy()


def _layout_ids(n, nlist, seed):
    ids = np.random.default_rng(seed).integers(0, nlist, size=n)
    ids[ids == 4] = 5               # an empty list in the middle
    ids[ids == nlist - 1] = 0       # and an empty last one
    ids[ids == nlist - 2] = 1
    return ids


@pytest.mark.parametrize("n,nlist", [(0, 5), (1, 3), (1003, 70), (70_001, 1030)])
def test_layout_is_the_stable_sort_by_list(gpu, n, nlist):
    torch, codec, ctx = gpu
    ids = _layout_ids(n, nlist, n) if n > 100 else np.full(n, nlist - 1, np.int64)
    perm, offsets = _layout(gpu, ids, nlist)
    want = np.zeros(nlist + 1, np.int64)
    want[1:] = np.cumsum(np.bincount(ids, minlength=nlist))
    assert np.array_equal(offsets, want)
    assert np.array_equal(perm, np.argsort(ids, kind="stable"))
    if n > 100:
        assert want[4] == want[5] and want[-1] == want[-2] == want[-3] == n
    rp, ro = ivf_ref.layout(ids, nlist)
    assert np.array_equal(perm, rp) and np.array_equal(offsets, ro)
    codec.ivf_status(ctx)
    # the same through codec.Coarse
    if n == 1003:
        cq = codec.Coarse(ctx, np.zeros((nlist, 2), np.float32))
        p2, o2 = cq.layout(torch.from_numpy(ids.astype(np.int32)).cuda())
        assert np.array_equal(p2.cpu().numpy(), perm) and np.array_equal(o2.cpu().numpy(), offsets)
        cq.close()


def test_layout_flags_a_list_id_outside_the_lists(gpu):
    """an argument check on the device: nothing is written out of bounds, the status says
    PQH_ERR_ARG once, and the next good call is clean"""
    torch, codec, ctx = gpu
    nlist = 70
    ids = _layout_ids(1003, nlist, 3)
    for bad in (nlist, -1):
        broken = ids.copy()
        broken[500] = bad
        perm, offsets = _layout(gpu, broken, nlist)
        assert _status(lambda: codec.ivf_status(ctx)) == -1                    # PQH_ERR_ARG
        assert np.array_equal(np.sort(perm), np.arange(1003))                  # still a permutation
        codec.ivf_status(ctx)                                                  # read once, then clean
        perm, offsets = _layout(gpu, ids, nlist)
        codec.ivf_status(ctx)
        rp, ro = ivf_ref.layout(ids, nlist)
        assert np.array_equal(perm, rp) and np.array_equal(offsets, ro)


# ------------------------------------------------------------------------------ probe
def _probe(gpu, cq, qd, nprobe, offsets_d, value, lists=True):
    """pqh_coarse_probe into poisoned buffers -> numpy (range_ptr, ranges, probes, dist)"""
    from pq_huffman_amd.capi import check, lib
    torch, codec, ctx = gpu
    nq = qd.shape[0]
    ptr = _poisoned(torch, (nq + 1,), torch.int64, value)
    ranges = _poisoned(torch, (nq * nprobe, 2), torch.int64, value)
    probes = _poisoned(torch, (nq, nprobe), torch.int64, value)
    pdist = _poisoned(torch, (nq, nprobe), torch.float32, value)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    check(lib().pqh_coarse_probe(ctx.ptr, cq.ptr, p(qd), nq, qd.stride(0), nprobe, p(offsets_d),
                                 p(ptr), p(ranges), p(probes) if lists else None,
                                 p(pdist) if lists else None), "pqh_coarse_probe")
    return ptr, ranges, probes, pdist


def _check_probe(got, want, what):
    ptr, ranges, probes, pdist = (t.cpu().numpy() for t in got)
    assert np.array_equal(ptr, want[0]), what
    assert np.array_equal(probes, want[2]), what
    assert np.array_equal(_bits(pdist), _bits(want[3])), what
    assert np.array_equal(ranges, want[1]), what


@pytest.mark.parametrize("nlist", [3, 70, 1030])
def test_probe_sweep(gpu, nlist):
    """nq in {1, 9} x nprobe in {1, 5, 64}; nprobe > nlist pads with (-1, +inf, (0, 0)); list 7
    is a copy of list 3 (a tie decided by the id) and some lists are empty"""
    torch, codec, ctx = gpu
    d = 37
    rng = np.random.default_rng(nlist)
    c = rng.normal(0.0, 10.0, size=(nlist, d)).astype(np.float32)
    if nlist > 7:
        c[7] = c[3]
    q = (c[rng.integers(0, nlist, size=9)] + rng.normal(0.0, 4.0, size=(9, d))).astype(np.float32)
    ids = _layout_ids(1003, nlist, 7) if nlist > 7 else np.array([0] * 5 + [2] * 4)
    _, offsets = ivf_ref.layout(ids, nlist)
    assert (np.diff(offsets) == 0).any()
    od = torch.from_numpy(offsets).cuda()
    dist = ivf_ref.dists(q, c)
    cq = codec.Coarse(ctx, c)
    qd = torch.from_numpy(q).cuda()
    case = 0
    for nq in (1, 9):
        for nprobe in (1, 5, 64):
            want = ivf_ref.probe(q[:nq], c, nprobe, offsets, dist[:nq])
            got = _probe(gpu, cq, qd[:nq], nprobe, od, POISON[case % 3])
            case += 1
            _check_probe(got, want, (nlist, nq, nprobe))
            assert np.array_equal(got[0].cpu().numpy(), np.arange(nq + 1) * nprobe)
            # the ranges are probe_ranges of the lists that were returned
            ptr2, ranges2 = codec.probe_ranges(od, got[2])
            assert torch.equal(ptr2, got[0]) and torch.equal(ranges2, got[1])
            if nprobe > nlist:
                assert (want[2][:, nlist:] == -1).all() and (want[1].reshape(nq, nprobe, 2)[:, nlist:] == 0).all()
            if nlist > 7 and nprobe == 64:
                for row in want[2]:
                    row = row.tolist()
                    if 3 in row[:-1]:
                        assert row[row.index(3) + 1] == 7
    # the optional outputs left out: the buffers stay as they were, the rest is the same
    want = ivf_ref.probe(q, c, 5, offsets, dist)
    got = _probe(gpu, cq, qd, 5, od, POISON[1], lists=False)
    assert np.array_equal(got[1].cpu().numpy(), want[1])
    assert (got[2].cpu().numpy().view(np.uint32) == POISON[1]).all()
    # and through codec.Coarse
    _check_probe(cq.probe(qd, 5, od), want, "Coarse.probe")
    assert cq.probe(qd, 5, od, lists=False)[2] is None
    codec.ivf_status(ctx)
    cq.close()


def test_probe_flags_a_reversed_offsets_pair(gpu):
    torch, codec, ctx = gpu
    rng = np.random.default_rng(2)
    c = rng.normal(0.0, 10.0, size=(3, 5)).astype(np.float32)
    q = rng.normal(0.0, 10.0, size=(9, 5)).astype(np.float32)
    cq = codec.Coarse(ctx, c)
    qd = torch.from_numpy(q).cuda()
    bad = np.array([0, 9, 4, 20], np.int64)           # list 1 = [9, 4)
    want = ivf_ref.probe(q, c, 5, bad)
    assert (want[1].reshape(9, 5, 2)[want[2] == 1] == 0).all()
    got = _probe(gpu, cq, qd, 5, torch.from_numpy(bad).cuda(), POISON[0])
    assert _status(lambda: codec.ivf_status(ctx)) == -1
    _check_probe(got, want, "reversed")
    good = np.array([0, 4, 9, 20], np.int64)
    got = _probe(gpu, cq, qd, 5, torch.from_numpy(good).cuda(), POISON[2])
    codec.ivf_status(ctx)
    _check_probe(got, ivf_ref.probe(q, c, 5, good), "good")
    # the argument checks
    from pq_huffman_amd.capi import PqhError
    for nprobe in (0, 65):
        with pytest.raises(PqhError) as err:
            cq.probe(qd, nprobe, torch.from_numpy(good).cuda())
        assert err.value.status == -1
    cq.close()


# ------------------------------------------------------------------------------ end to end
N, NLIST, M, NQ = 1003, 13, 8, 9


@pytest.fixture(scope="module")
def world(gpu):
    """x, a 13-list coarse codebook, an 8 x 256 PQ, nine queries and their numpy ADC tables"""
    torch, codec, ctx = gpu
    x = datagen.sift_like(N, 128, seed=21)
    rng = np.random.default_rng(22)
    cc = (x[rng.choice(N, NLIST, replace=False)] + np.float32(0.5)).astype(np.float32)
    cent = datagen.lloyd_centroids(x, M, 256, iters=2, sample=N)
    q = (x[rng.choice(N, NQ, replace=False)] +
         rng.normal(0.0, 3.0, size=(NQ, 128))).astype(np.float32)
    lut = np.stack([ivf_ref.dists(q[:, 16 * i:16 * i + 16], cent[i]) for i in range(M)], axis=1)
    assert lut.shape == (NQ, M, 256) and lut.dtype == np.float32
    lists, _ = ivf_ref.assign(x, cc)
    perm, offsets = ivf_ref.layout(lists, NLIST)
    return dict(x=x, cc=cc, cent=cent, q=q, lut=lut, perm=perm, offsets=offsets,
                cdist=ivf_ref.dists(q, cc), xd=torch.from_numpy(x).cuda(),
                qd=torch.from_numpy(q).cuda(), pq=codec.PQ(ctx, cent), coarse=codec.Coarse(ctx, cc))


def _adc(lut_q, codes):
    dist = lut_q[0, codes[:, 0]]
    for i in range(1, codes.shape[1]):
        dist = dist + lut_q[i, codes[:, i]]
    assert dist.dtype == np.float32
    return dist


@pytest.mark.parametrize("chunk", [7, 64])
@pytest.mark.parametrize("context", [True, False])
def test_ivf_search_equals_numpy(gpu, world, context, chunk):
    torch, codec, ctx = gpu
    w = world
    ivf = codec.IVF.build(ctx, w["pq"], w["coarse"], w["xd"], chunk_vectors=chunk, context=context)
    codec.ivf_status(ctx)
    assert np.array_equal(ivf.perm.cpu().numpy(), w["perm"])
    assert np.array_equal(ivf.offsets.cpu().numpy(), w["offsets"])
    assert (np.diff(w["offsets"]) % chunk != 0).any()        # lists cut chunks
    inv = np.empty(N, np.int64)
    inv[w["perm"]] = np.arange(N)
    assert np.array_equal(ivf.inv.cpu().numpy(), inv)
    codes = codec.decode(ctx, ivf.tables, ivf.enc).cpu().numpy()      # the index's own codes
    codec.decode_status(ctx)
    assert codes.shape == (N, M)
    for nprobe in (1, 4):
        _, ranges, probes, _ = ivf_ref.probe(w["q"], w["cc"], nprobe, w["offsets"], w["cdist"])
        for k in (1, 10, 64):
            wd = np.full((NQ, k), np.inf, np.float32)
            wi = np.full((NQ, k), -1, np.int64)
            for qi in range(NQ):
                rows = np.concatenate([np.arange(f, f + cnt, dtype=np.int64)
                                       for f, cnt in ranges[qi * nprobe:(qi + 1) * nprobe]])
                dist = _adc(w["lut"][qi], codes[rows])
                order = np.lexsort((rows, dist))[:k]
                wd[qi, :len(order)] = dist[order]
                wi[qi, :len(order)] = w["perm"][rows[order]]
            gd, gi = ivf.search(w["qd"], nprobe, k)
            assert np.array_equal(gi.cpu().numpy(), wi), (nprobe, k)
            assert np.array_equal(_bits(gd.cpu().numpy()), _bits(wd)), (nprobe, k)
    codec.decode_status(ctx)
    codec.ivf_status(ctx)

    # every list probed: the plain search of the whole stream, mapped through perm
    lut_d = codec.adc_tables(ctx, w["pq"], w["qd"])
    assert np.array_equal(_bits(lut_d.cpu().numpy()), _bits(w["lut"]))
    for k in (1, 10, 64):
        pd, rows = codec.search(ctx, ivf.tables, ivf.enc, lut_d, k)
        gd, gi = ivf.search(w["qd"], NLIST, k)
        assert torch.equal(gi, ivf.perm[rows]) and torch.equal(gd.view(torch.int32), pd.view(torch.int32))

    # fetch: the reconstruction of caller rows
    ids = ivf.search(w["qd"], 4, 10)[1].reshape(-1)
    assert int(ids.min()) >= 0
    want = np.concatenate([w["cent"][i][codes[inv[ids.cpu().numpy()], i]] for i in range(M)], axis=1)
    got = ivf.fetch(ids)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))
    caller_codes = w["pq"].assign(w["xd"])
    assert torch.equal(got, w["pq"].reconstruct(caller_codes[ids]))
    codec.decode_status(ctx)


def test_ivf_with_a_trained_coarse_codebook(gpu, world):
    """kmeans_train with m = 1, k = nlist, dsub = d trains the coarse centroids as it trains
    any codebook: the index builds and searches, and every list is the nearest one's"""
    torch, codec, ctx = gpu
    w = world
    init = w["x"][np.random.default_rng(4).choice(N, NLIST, replace=False)][None]
    trained = codec.kmeans_train(ctx, w["xd"], init, 3)
    assert trained.shape == (1, NLIST, 128)
    coarse = codec.Coarse(ctx, trained)
    assert (coarse.nlist, coarse.d) == (NLIST, 128)
    ivf = codec.IVF.build(ctx, w["pq"], coarse, w["xd"])
    dist, ids = ivf.search(w["qd"], 4, 10)
    codec.ivf_status(ctx)
    codec.decode_status(ctx)
    ids = ids.cpu().numpy()
    assert ((ids >= 0) & (ids < N)).all() and np.isfinite(dist.cpu().numpy()).all()
    lists, _ = ivf_ref.assign(w["x"], trained[0])
    perm, offsets = ivf_ref.layout(lists, NLIST)
    assert np.array_equal(ivf.perm.cpu().numpy(), perm)
    assert np.array_equal(ivf.offsets.cpu().numpy(), offsets)
    coarse.close()
