"""codec.IVF with rotation= on the GPU, from vectors and queries to neighbour ids: the world of
tests/test_gpu_ivf_metric.py's shape (1,500 rows, d = 32, 24 lists, a level-2 codebook), plain
and residual, "l2" and "ip", behind a dense orthonormal R.  Expected values are the existing
brute force of tests/metric_ref.py on inputs rotated by tests/opq_ref.py, never the calls under
test: floats are compared on their raw bits, ids with array_equal."""
import numpy as np
import pytest

import datagen
import ivf_ref
import metric_ref as mr
import opq_ref
import refine_ref as rr

pytestmark = pytest.mark.gpu

N, D, NLIST, M, NQ, NPROBE = 1500, 32, 24, 8, 7, 8
KINDS = [("plain", "l2"), ("residual", "l2"), ("plain", "ip"), ("residual", "ip")]


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


def make_world(kind, metric):
    """1,500 centred SIFT-like rows of spread norms and seven queries in the caller's axes; R a
    Procrustes of a random matrix (orthonormal and dense); everything the index holds -- 24
    coarse centroids, an 8 x 256 PQ of what the stream stores, a 16 x 256 PQ of what that leaves
    over -- trained on the rotated rows, and the numpy index of the rotated rows"""
    rng = np.random.default_rng(51)
    x = datagen.sift_like(N, D, seed=50)
    x = ((x - x.mean(axis=0)) * rng.lognormal(0.0, 0.5, size=(N, 1))).astype(np.float32)
    R = opq_ref.procrustes(rng.normal(size=(D, D)))
    assert (np.abs(R) > 1e-3).mean() > 0.9              # dense: no axis is left alone
    xr = opq_ref.rotate(x, R)
    cc = datagen.lloyd_centroids(xr, 1, NLIST, iters=3, sample=N)[0]
    residual = kind == "residual"
    lists = mr.assign(xr, cc)[0] if metric == "ip" else ivf_ref.assign(xr, cc)[0]
    stored = xr - cc[lists] if residual else xr
    cent = datagen.lloyd_centroids(stored, M, 256, iters=2, sample=N)
    left = stored - rr.reconstruct(cent, mr.pq_codes(stored, cent))
    cent2 = datagen.lloyd_centroids(left, 16, 256, iters=2, sample=N)
    q = (x[rng.choice(N, NQ, replace=False)] + rng.normal(0.0, 3.0, size=(NQ, D))).astype(np.float32)
    w = mr.build(xr, cc, cent, residual, metric, cent2)
    w.update(x=x, q=q, qr=opq_ref.rotate(q, R), R=R, keep=rng.random(N) < 0.5)
    # the rotation matters: the index of the unrotated rows is another one
    assert not np.array_equal(mr.build(x, cc, cent, residual, metric)["lists"], w["lists"])
    return w


@pytest.fixture(scope="module", params=KINDS, ids=lambda p: "-".join(p))
def world(request, gpu):
    torch, codec, ctx = gpu
    w = make_world(*request.param)
    w.update(xd=torch.from_numpy(w["x"]).cuda(), qd=torch.from_numpy(w["q"]).cuda(),
             keepd=torch.from_numpy(w["keep"]).cuda(), pq=codec.PQ(ctx, w["cent"]),
             pq2=codec.PQ(ctx, w["cent2"]), coarse=codec.Coarse(ctx, w["cc"]),
             rot=codec.Rotation(ctx, w["R"]))
    return w


def _build(gpu, w, xd, **kw):
    torch, codec, ctx = gpu
    return codec.IVF.build(ctx, w["pq"], w["coarse"], xd, chunk_vectors=7, residual=w["residual"],
                           refine_pq=w["pq2"], refine_chunk_vectors=5, metric=w["metric"],
                           rotation=w["rot"], **kw)


def _sweep(ivf, w, removed=None, tag=""):
    """both schedules x (k, refine) x keep, and the range search, against the brute force over
    the rotated rows and the rotated queries; removed: caller rows taken out"""
    import torch
    alive = np.ones(N, bool)
    if removed is not None:
        alive[removed] = False
    for kept in (False, True):
        mask = alive & w["keep"] if kept else (alive if removed is not None else None)
        keepd = w["keepd"] if kept else None
        cands = {c: mr.search(w, w["qr"], NPROBE, c, keep=mask) for c in (10, 64, 200)}
        fine = {(k, c): mr.search(w, w["qr"], NPROBE, c, keep=mask, refine_k=k)
                for k, c in ((10, 64), (10, 200))}
        for schedule in ("query", "list"):
            for k in (10, 200):
                _check(ivf.search(w["qd"], NPROBE, k, schedule=schedule, keep=keepd), cands[k],
                       (tag, schedule, k, kept))
            for (k, c), want in fine.items():
                _check(ivf.search(w["qd"], NPROBE, k, schedule=schedule, keep=keepd, refine=c),
                       want, (tag, schedule, k, c, kept))
        radius = cands[10][0][:, 9].copy()
        assert np.isfinite(radius).all()
        want = mr.range_search(w, w["qr"], NPROBE, radius, keep=mask)
        assert (np.diff(want[0]) >= 1).all()
        lims, dist, ids = ivf.range_search(w["qd"], NPROBE, torch.from_numpy(radius).cuda(),
                                           keep=keepd)
        assert np.array_equal(lims.cpu().numpy(), want[0]), (tag, kept)
        assert np.array_equal(ids.cpu().numpy(), want[2]), (tag, kept)
        assert np.array_equal(_bits(dist.cpu().numpy()), _bits(want[1])), (tag, kept)


def test_rotated_index_equals_the_brute_force_on_rotated_rows(gpu, world):
    torch, codec, ctx = gpu
    w = world
    ivf = _build(gpu, w, w["xd"])
    codec.ivf_status(ctx)
    assert ivf.rotation is w["rot"] and ivf.metric == w["metric"]
    assert np.array_equal(ivf.perm.cpu().numpy(), w["perm"])
    assert np.array_equal(ivf.offsets.cpu().numpy(), w["offsets"])
    assert np.array_equal(codec.decode(ctx, ivf.tables, ivf.enc).cpu().numpy(), w["codes"])
    assert np.array_equal(codec.decode(ctx, ivf.refine_tables, ivf.refine_enc).cpu().numpy(),
                          w["codes2"])
    codec.decode_status(ctx)
    _sweep(ivf, w)
    # remove: the best rows of the first query go, everywhere
    first = mr.search(w, w["qr"], NPROBE, 10)[1][0]
    ivf.remove(torch.from_numpy(first).cuda())
    _sweep(ivf, w, removed=first, tag="removed")
    # compress_ids: the same bits through the id map
    assert ivf.compress_ids() > 0 and ivf.perm is None
    _sweep(ivf, w, removed=first, tag="idmap")
    codec.decode_status(ctx)
    codec.ivf_status(ctx)


def test_fetch_rotates_the_reconstruction_back(gpu, world):
    """fetch and fetch(refined=True): what the index reconstructs in its own space (c1, + c2
    first when refined, then + the list's centroid on a residual index, one add each), taken
    back by R's transpose"""
    torch, codec, ctx = gpu
    w = world
    ivf = _build(gpu, w, w["xd"])
    ids = np.random.default_rng(4).choice(N, 90, replace=False)
    inv = np.empty(N, np.int64)
    inv[w["perm"]] = np.arange(N)
    rows = inv[ids]
    for refined in (False, True):
        y = rr.reconstruct(w["cent"], w["codes"][rows])
        if refined:
            y = y + rr.reconstruct(w["cent2"], w["codes2"][rows])
        if w["residual"]:
            y = y + w["cc"][rr.lists_of(w["offsets"], rows)]
        assert y.dtype == np.float32
        want = opq_ref.rotate(y, w["R"], transpose=True)
        got = ivf.fetch(torch.from_numpy(ids).cuda(), refined=refined)
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), refined
        out = torch.full((90, D + 2), -7.0, dtype=torch.float32, device="cuda")
        assert ivf.fetch(torch.from_numpy(ids).cuda(), out=out, refined=refined) is out
        assert np.array_equal(_bits(out[:, :D].cpu().numpy()), _bits(want))
        assert (out[:, D:] == -7.0).all()
    # and that is near the caller's rows: the refined reconstruction nearer than the plain one
    plain = ivf.fetch(torch.from_numpy(ids).cuda()).cpu().numpy().astype(np.float64)
    fine = ivf.fetch(torch.from_numpy(ids).cuda(), refined=True).cpu().numpy().astype(np.float64)
    x64 = w["x"][ids].astype(np.float64)
    assert ((fine - x64) ** 2).sum() < ((plain - x64) ** 2).sum() < (x64 ** 2).sum()
    codec.decode_status(ctx)


def _same_stream(torch, a_tables, a, b_tables, b, what):
    assert (a.n, a.bits, a.chunk_vectors, a.raw_first) == (b.n, b.bits, b.chunk_vectors, b.raw_first), what
    assert torch.equal(a.stream[:a.nbytes], b.stream[:b.nbytes]), what
    assert torch.equal(a.chunk_offsets, b.chunk_offsets), what
    assert a_tables.codebooks().file_bytes() == b_tables.codebooks().file_bytes(), what


def _same_index(gpu, got, want, ids=None, what=""):
    torch, codec, ctx = gpu
    assert got.rotation is want.rotation and got.metric == want.metric
    assert torch.equal(got.offsets, want.offsets), what
    _same_stream(torch, got.tables, got.enc, want.tables, want.enc, what)
    _same_stream(torch, got.refine_tables, got.refine_enc, want.refine_tables, want.refine_enc, what)
    assert torch.equal(got.perm, want.perm if ids is None else ids[want.perm]), what
    codec.decode_status(ctx)
    codec.ivf_status(ctx)


def test_add_then_compact_equals_build(gpu, world):
    """build of the first half, add of the second: the index build() gives for all rows, which it
    is only if add() rotates its batch.  Then 300 rows removed and compact()."""
    torch, codec, ctx = gpu
    w = world
    ivf = _build(gpu, w, w["xd"][:N // 2])
    assert ivf.add(w["xd"][N // 2:]) == N // 2 and ivf.n_ids == N
    whole = _build(gpu, w, w["xd"])
    assert np.array_equal(whole.offsets.cpu().numpy(), w["offsets"])
    _same_index(gpu, ivf, whole, what="add")
    _check(ivf.search(w["qd"], NPROBE, 10), mr.search(w, w["qr"], NPROBE, 10), "added")
    gone = np.sort(np.random.default_rng(3).choice(N, 300, replace=False))
    ivf.remove(torch.from_numpy(gone).cuda())
    assert ivf.compact() == 300
    left = np.setdiff1d(np.arange(N), gone)
    ld = torch.from_numpy(left).cuda()
    _same_index(gpu, ivf, _build(gpu, w, w["xd"][ld]), ids=ld, what="compact")
    alive = np.ones(N, bool)
    alive[gone] = False
    _check(ivf.search(w["qd"], NPROBE, 10), mr.search(w, w["qr"], NPROBE, 10, keep=alive), "compacted")


def test_build_refuses_a_rotation_that_does_not_fit(gpu, world):
    torch, codec, ctx = gpu
    w = world
    small = codec.Rotation(ctx, np.eye(D - 1, dtype=np.float32))
    twice = codec.Rotation(ctx, 2.0 * w["R"])
    assert w["rot"].defect() < 1e-4 and twice.defect() > 1.0
    for bad in (small, twice):
        with pytest.raises(codec.PqhError):
            codec.IVF.build(ctx, w["pq"], w["coarse"], w["xd"], residual=w["residual"],
                            metric=w["metric"], rotation=bad)
    small.close()
    twice.close()
    # no rotation: the index of before, of the unrotated rows
    plain = codec.IVF.build(ctx, w["pq"], w["coarse"], w["xd"], chunk_vectors=7,
                            residual=w["residual"], metric=w["metric"])
    assert plain.rotation is None
    ref = mr.build(w["x"], w["cc"], w["cent"], w["residual"], w["metric"])
    assert np.array_equal(plain.perm.cpu().numpy(), ref["perm"])
    _check(plain.search(w["qd"], NPROBE, 10), mr.search(ref, w["q"], NPROBE, 10), "unrotated")


def test_a_trained_rotation_finds_more_of_the_exact_neighbours(gpu, oracle):
    """spectrum_world(mix=True) with the reference's R and codebooks (the PCA start), every list
    probed: the rotated index returns the reference's ids, so its recall@10 against the exact
    float64 neighbours is the reference's, and that exceeds the unrotated reference's with a
    codebook of as many Lloyd iterations.  The reference gives 0.8325 against 0.6525 (0.715 from
    the identity start; a numpy prototype of the procedure gave 0.85 against 0.64)."""
    torch, codec, ctx = gpu
    n, nq, m, k, nlist = 4000, 40, 8, 64, 8
    rows = opq_ref.spectrum_world(n + nq, 32, 0.85, 3, True)
    x, q = rows[:n], rows[n:]
    truth = opq_ref.exact_knn(x, q, 10)
    start = opq_ref.pca_rotation(x, m)
    R, cent, errors = opq_ref.train(oracle, x, m, k, opq_ref.init_rows(x, m, k, 11, start),
                                    init="pca")
    init = opq_ref.init_rows(x, m, k, 11)
    plain_cent = oracle.kmeans(x, init, 18)
    cc = datagen.lloyd_centroids(x, 1, nlist, iters=3, sample=n)[0]
    ccr = opq_ref.rotate(cc, R)
    plain = mr.build(x, cc, plain_cent, False, "l2")
    turned = mr.build(opq_ref.rotate(x, R), ccr, cent, False, "l2")
    want = mr.search(turned, opq_ref.rotate(q, R), nlist, 10)
    rot, pq, coarse = codec.Rotation(ctx, R), codec.PQ(ctx, cent), codec.Coarse(ctx, ccr)
    # the coarse centroids taken to the rotated space on the device are the same
    assert torch.equal(rot.apply(torch.from_numpy(cc).cuda()), coarse.centroids)
    # (context coding takes K = 256: this stream is coded without)
    ivf = codec.IVF.build(ctx, pq, coarse, torch.from_numpy(x).cuda(), context=False,
                          rotation=rot)
    _check(ivf.search(torch.from_numpy(q).cuda(), nlist, 10), want, "trained")
    recall = mr.recall(want[1], truth)
    recall_plain = mr.recall(mr.search(plain, q, nlist, 10)[1], truth)
    print("recall@10 rotated", recall, "unrotated", recall_plain)
    assert recall > recall_plain
    for o in (rot, pq, coarse):
        o.close()
