"""codec.IVF with metric="ip" on the GPU, from vectors and queries to neighbour ids: both
schedules, plain and residual, keep=, remove, refine=, k above 64, range_search, compress_ids,
add and compact.  Expected values are the brute force of tests/metric_ref.py over the probed
lists, never the calls under test: floats are compared on their raw bits, ids with array_equal."""
import numpy as np
import pytest

import datagen
import ivf_ref
import metric_ref as mr
import refine_ref as rr

pytestmark = pytest.mark.gpu

N, D, NLIST, M, NQ, NPROBE = 1500, 32, 24, 8, 7, 8
KINDS = ("plain", "residual")


@pytest.fixture(scope="module")
def gpu():
    import torch
    from pq_huffman_amd import codec
    assert torch.cuda.is_available()
    return torch, codec, codec.Context(0).set_search_max_k(256)


def _bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


def _check(got, want, what=""):
    gd, gi = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert gd.dtype == np.float32 and gi.dtype == np.int64
    assert np.array_equal(gi, want[1]), what
    assert np.array_equal(_bits(gd), _bits(want[0])), what


def make_world(kind):
    """1,500 centred SIFT-like rows of spread norms, 24 lists, the last two with a centroid
    of zeros (a score of +0 for every row, and every row has a centroid it points towards, so
    they stay empty; the long centroids draw rows from others, which leaves more lists empty),
    an 8 x 256 PQ trained on what the stream holds and a 16 x 256 PQ on what that leaves over;
    seven queries"""
    rng = np.random.default_rng(41)
    x = datagen.sift_like(N, D, seed=40)
    x = ((x - x.mean(axis=0)) * rng.lognormal(0.0, 0.5, size=(N, 1))).astype(np.float32)
    cc = datagen.lloyd_centroids(x, 1, NLIST - 2, iters=3, sample=N)[0]
    cc = np.concatenate([cc, np.zeros((1, D), np.float32), np.zeros((1, D), np.float32)])
    residual = kind == "residual"
    lists = mr.assign(x, cc)[0]
    stored = x - cc[lists] if residual else x
    cent = datagen.lloyd_centroids(stored, M, 256, iters=2, sample=N)
    left = stored - rr.reconstruct(cent, mr.pq_codes(stored, cent))
    cent2 = datagen.lloyd_centroids(left, 16, 256, iters=2, sample=N)
    q = (x[rng.choice(N, NQ, replace=False)] + rng.normal(0.0, 3.0, size=(NQ, D))).astype(np.float32)
    keep = rng.random(N) < 0.5
    w = mr.build(x, cc, cent, residual, "ip", cent2)
    w.update(x=x, q=q, keep=keep)
    return w


def check_world(w):
    sizes = np.diff(w["offsets"])
    assert (sizes == 0).sum() >= 1 and len(sizes) == NLIST <= 40 and N <= 4096 and NQ <= 9
    # every query probes more than 256 rows, so k = 200 is filled; under keep one query at
    # least finds fewer than 200, so its result (and its candidates for the re-rank) end in
    # padding, and every query finds more than 64
    wd, wi = mr.search(w, w["q"], NPROBE, 256)
    assert (wi >= 0).all() and np.isfinite(wd).all()
    found = (mr.search(w, w["q"], NPROBE, 256, keep=w["keep"])[1] >= 0).sum(axis=1)
    assert (found < 200).any() and (found > 64).all(), found
    # and the index is no L2 index
    assert not np.array_equal(w["lists"], ivf_ref.assign(w["x"], w["cc"])[0])


@pytest.fixture(scope="module", params=KINDS)
def world(request, gpu):
    torch, codec, ctx = gpu
    w = make_world(request.param)
    check_world(w)
    w.update(kind=request.param, xd=torch.from_numpy(w["x"]).cuda(),
             qd=torch.from_numpy(w["q"]).cuda(), keepd=torch.from_numpy(w["keep"]).cuda(),
             pq=codec.PQ(ctx, w["cent"]), pq2=codec.PQ(ctx, w["cent2"]),
             coarse=codec.Coarse(ctx, w["cc"]))
    return w


def _build(gpu, w, xd, **kw):
    torch, codec, ctx = gpu
    return codec.IVF.build(ctx, w["pq"], w["coarse"], xd, chunk_vectors=7,
                           residual=w["residual"], refine_pq=w["pq2"], refine_chunk_vectors=5,
                           metric="ip", **kw)


def _sweep(ivf, w, removed=None, tag=""):
    """both schedules x (k, refine) x keep, and the range search, against the brute force;
    removed: caller rows taken out"""
    alive = np.ones(N, bool)
    if removed is not None:
        alive[removed] = False
    for kept in (False, True):
        mask = alive & w["keep"] if kept else (alive if removed is not None else None)
        keepd = w["keepd"] if kept else None
        cands = {c: mr.search(w, w["q"], NPROBE, c, keep=mask) for c in (10, 64, 200)}
        fine = {(k, c): mr.search(w, w["q"], NPROBE, c, keep=mask, refine_k=k)
                for k, c in ((10, 64), (10, 200), (200, 200))}
        for schedule in ("query", "list"):
            for k in (10, 200):
                _check(ivf.search(w["qd"], NPROBE, k, schedule=schedule, keep=keepd), cands[k],
                       (tag, schedule, k, kept))
            for (k, c), want in fine.items():
                _check(ivf.search(w["qd"], NPROBE, k, schedule=schedule, keep=keepd, refine=c),
                       want, (tag, schedule, k, c, kept))
        # every row below each query's 10th score: nine rows, and the rows that tie with them
        radius = cands[10][0][:, 9].copy()
        assert np.isfinite(radius).all()
        want = mr.range_search(w, w["q"], NPROBE, radius, keep=mask)
        assert (np.diff(want[0]) >= 1).all() and (np.diff(want[0]) <= 9).all()
        import torch
        lims, dist, ids = ivf.range_search(w["qd"], NPROBE, torch.from_numpy(radius).cuda(),
                                           keep=keepd)
        assert np.array_equal(lims.cpu().numpy(), want[0]), (tag, kept)
        assert np.array_equal(ids.cpu().numpy(), want[2]), (tag, kept)
        assert np.array_equal(_bits(dist.cpu().numpy()), _bits(want[1])), (tag, kept)


def test_ip_index_equals_the_brute_force(gpu, world):
    torch, codec, ctx = gpu
    w = world
    ivf = _build(gpu, w, w["xd"])
    codec.ivf_status(ctx)
    assert ivf.metric == "ip" and ivf.residual == w["residual"]
    assert np.array_equal(ivf.perm.cpu().numpy(), w["perm"])
    assert np.array_equal(ivf.offsets.cpu().numpy(), w["offsets"])
    # the stream holds L2 codes of the rows (residual: of x - c[list]) whatever the metric
    assert np.array_equal(codec.decode(ctx, ivf.tables, ivf.enc).cpu().numpy(), w["codes"])
    assert np.array_equal(codec.decode(ctx, ivf.refine_tables, ivf.refine_enc).cpu().numpy(),
                          w["codes2"])
    codec.decode_status(ctx)
    _sweep(ivf, w)
    if w["residual"]:                                         # slab by slab
        one = ivf.search(w["qd"], NPROBE, 10)
        ivf.table_budget = 2 * NPROBE * M * 256 * 4
        _check(ivf.search(w["qd"], NPROBE, 10), mr.search(w, w["q"], NPROBE, 10), "slabs")
        del ivf.table_budget
        assert torch.equal(one[1], ivf.search(w["qd"], NPROBE, 10)[1])
    # scores = -dist: the best row's score is its inner product with what the index stores
    dist, ids = ivf.search(w["qd"], NPROBE, 1)
    got = ivf.fetch(ids.reshape(-1)).cpu().numpy().astype(np.float64)
    ip = (got * w["q"].astype(np.float64)).sum(axis=1)
    assert np.allclose(-dist.cpu().numpy()[:, 0], ip, rtol=1e-4, atol=1e-2)
    # remove: the best rows of the first query go, everywhere
    first = mr.search(w, w["q"], NPROBE, 10)[1][0]
    ivf.remove(torch.from_numpy(first).cuda())
    _sweep(ivf, w, removed=first, tag="removed")
    # compress_ids: the same bits through the id map
    assert ivf.compress_ids() > 0 and ivf.perm is None
    _sweep(ivf, w, removed=first, tag="idmap")
    codec.decode_status(ctx)
    codec.ivf_status(ctx)


def _same_stream(torch, a_tables, a, b_tables, b, what):
    assert (a.n, a.bits, a.chunk_vectors, a.raw_first) == (b.n, b.bits, b.chunk_vectors, b.raw_first), what
    assert torch.equal(a.stream[:a.nbytes], b.stream[:b.nbytes]), what
    assert torch.equal(a.chunk_offsets, b.chunk_offsets), what
    assert a_tables.codebooks().file_bytes() == b_tables.codebooks().file_bytes(), what


def _same_index(gpu, got, want, ids=None, what=""):
    torch, codec, ctx = gpu
    assert got.metric == want.metric == "ip"
    assert torch.equal(got.offsets, want.offsets), what
    _same_stream(torch, got.tables, got.enc, want.tables, want.enc, what)
    _same_stream(torch, got.refine_tables, got.refine_enc, want.refine_tables, want.refine_enc, what)
    assert torch.equal(got.perm, want.perm if ids is None else ids[want.perm]), what
    codec.decode_status(ctx)
    codec.ivf_status(ctx)


def test_add_then_compact_equals_build(gpu, world):
    """build of the first half, add of the second: the index build() gives for all rows, which
    it is only if add() sends its rows to the lists of the index's own metric.  Then 300 rows
    removed and compact(): the index of the rows that are left."""
    torch, codec, ctx = gpu
    w = world
    ivf = _build(gpu, w, w["xd"][:N // 2])
    assert ivf.add(w["xd"][N // 2:]) == N // 2 and ivf.n_ids == N
    whole = _build(gpu, w, w["xd"])
    assert np.array_equal(whole.offsets.cpu().numpy(), w["offsets"])
    _same_index(gpu, ivf, whole, what="add")
    _check(ivf.search(w["qd"], NPROBE, 10), mr.search(w, w["q"], NPROBE, 10), "added")
    gone = np.sort(np.random.default_rng(3).choice(N, 300, replace=False))
    ivf.remove(torch.from_numpy(gone).cuda())
    assert ivf.compact() == 300
    left = np.setdiff1d(np.arange(N), gone)
    ld = torch.from_numpy(left).cuda()
    _same_index(gpu, ivf, _build(gpu, w, w["xd"][ld]), ids=ld, what="compact")
    alive = np.ones(N, bool)
    alive[gone] = False
    _check(ivf.search(w["qd"], NPROBE, 10), mr.search(w, w["q"], NPROBE, 10, keep=alive), "compacted")


def test_an_exact_world_gives_the_exact_inner_products(gpu):
    """rows that are the codebook's own reconstructions on an integer grid: the stream loses
    nothing and every sum is exact, so -dist is the int64 inner product and the ids are the
    exact top k (every list probed; equal scores in stream order)"""
    torch, codec, ctx = gpu
    rng = np.random.default_rng(17)
    m, k, dsub, nlist, n, nq = 4, 16, 4, 9, 600, 5
    cent = rng.integers(-4, 5, size=(m, k, dsub)).astype(np.float32)
    x = rr.reconstruct(cent, rng.integers(0, k, size=(n, m)).astype(np.uint8))
    q, cc = ivf_ref.integer_grid(nq, m * dsub, nlist, seed=18)
    pq, coarse = codec.PQ(ctx, cent), codec.Coarse(ctx, cc)
    ivf = codec.IVF.build(ctx, pq, coarse, torch.from_numpy(x).cuda(), chunk_vectors=4,
                          context=False, metric="ip")
    perm = ivf.perm.cpu().numpy()
    lists = mr.assign(x, cc)[0]
    assert np.array_equal(perm, ivf_ref.layout(lists, nlist)[0])
    exact = mr.nip_int64(q, x[perm])                           # [nq][stream row]
    for top in (1, 10, 64):
        dist, ids = ivf.search(torch.from_numpy(q).cuda(), nlist, top)
        for i in range(nq):
            order = np.lexsort((np.arange(n), exact[i]))[:top]
            assert np.array_equal(ids.cpu().numpy()[i], perm[order]), (top, i)
            assert np.array_equal(-dist.cpu().numpy()[i].astype(np.int64), -exact[i][order]), (top, i)
    assert (np.diff(np.sort(exact[0])[:64]) == 0).any()       # there are equal scores
    codec.decode_status(ctx)
    codec.ivf_status(ctx)
    pq.close()
    coarse.close()


def test_the_default_metric_is_the_l2_index_of_before(gpu, world):
    """no metric given: the L2 mirror of tests/ivf_ref.py and ivf_residual_ref.py, bit for bit"""
    torch, codec, ctx = gpu
    w = world
    l2 = mr.build(w["x"], w["cc"], w["cent"], w["residual"], "l2", w["cent2"])
    ivf = codec.IVF.build(ctx, w["pq"], w["coarse"], w["xd"], chunk_vectors=7,
                          residual=w["residual"], refine_pq=w["pq2"])
    assert ivf.metric == "l2"
    assert np.array_equal(ivf.offsets.cpu().numpy(), l2["offsets"])
    assert np.array_equal(ivf.perm.cpu().numpy(), l2["perm"])
    for schedule in ("query", "list"):
        _check(ivf.search(w["qd"], NPROBE, 10, schedule=schedule), mr.search(l2, w["q"], NPROBE, 10),
               schedule)
        _check(ivf.search(w["qd"], NPROBE, 10, schedule=schedule, refine=64),
               mr.search(l2, w["q"], NPROBE, 64, refine_k=10), (schedule, "refine"))
    explicit = codec.IVF.build(ctx, w["pq"], w["coarse"], w["xd"], chunk_vectors=7,
                               residual=w["residual"], refine_pq=w["pq2"], metric="l2")
    a, b = ivf.search(w["qd"], NPROBE, 10), explicit.search(w["qd"], NPROBE, 10)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    codec.decode_status(ctx)
    codec.ivf_status(ctx)
