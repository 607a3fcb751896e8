"""codec.IVF.add and codec.IVF.compact on the GPU.  The yardstick is IVF.build itself: an index
that was added to or compacted must be, stream for stream and table for table, the index that
build() makes of the same rows -- the layout is a stable sort by list and every assignment a
per-row fp32 argmin, so a difference is a bug, not rounding -- and its searches the same bits."""
import numpy as np
import pytest

import datagen

pytestmark = pytest.mark.gpu

N, NLIST, M, NQ = 1003, 13, 8, 9
KINDS = ("plain", "residual", "refine")


@pytest.fixture(scope="module")
def gpu():
    import torch
    from pq_huffman_amd import codec
    assert torch.cuda.is_available()
    return torch, codec, codec.Context(0)


@pytest.fixture(scope="module")
def world(gpu):
    """1,003 SIFT-like rows, an 8 x 256 PQ, a 16 x 256 second codebook, nine queries and a
    coarse codebook of 13 rows of x and two centroids far from the data: two empty lists"""
    torch, codec, ctx = gpu
    x = datagen.sift_like(N, 128, seed=21)
    rng = np.random.default_rng(22)
    cc = (x[rng.choice(N, NLIST, replace=False)] + np.float32(0.5)).astype(np.float32)
    far = np.stack([np.full(128, -5000.0, np.float32), np.full(128, 9000.0, np.float32)])
    cc = np.concatenate([cc[:4], far[:1], cc[4:], far[1:]])
    cent = datagen.lloyd_centroids(x, M, 256, iters=2, sample=N)
    cent2 = datagen.lloyd_centroids((x - x.mean(axis=0)) * np.float32(0.25), 16, 256, iters=1, sample=N)
    q = (x[rng.choice(N, NQ, replace=False)] +
         rng.normal(0.0, 3.0, size=(NQ, 128))).astype(np.float32)
    return dict(x=x, xd=torch.from_numpy(x).cuda(), qd=torch.from_numpy(q).cuda(),
                pq=codec.PQ(ctx, cent), pq2=codec.PQ(ctx, cent2), coarse=codec.Coarse(ctx, cc))


def _build(gpu, w, xd, kind, chunk, context):
    torch, codec, ctx = gpu
    return codec.IVF.build(ctx, w["pq"], w["coarse"], xd, chunk_vectors=chunk, context=context,
                           residual=kind == "residual",
                           refine_pq=w["pq2"] if kind == "refine" else None,
                           refine_chunk_vectors=5 if kind == "refine" else None)


def _same_stream(torch, a_tables, a, b_tables, b, what):
    assert (a.n, a.bits, a.chunk_vectors, a.raw_first) == (b.n, b.bits, b.chunk_vectors, b.raw_first), what
    assert torch.equal(a.stream[:a.nbytes], b.stream[:b.nbytes]), what
    assert torch.equal(a.chunk_offsets, b.chunk_offsets), what
    assert (a.chunk_prev is None) == (b.chunk_prev is None), what
    if a.chunk_prev is not None:
        assert torch.equal(a.chunk_prev, b.chunk_prev), what
    assert a_tables.context == b_tables.context
    assert a_tables.codebooks().file_bytes() == b_tables.codebooks().file_bytes(), what


def _same_index(gpu, got, want, ids=None, what=""):
    """got is the index build() made (want), whose rows are the ids `ids` of got (None: 0 ... n - 1)"""
    torch, codec, ctx = gpu
    _same_stream(torch, got.tables, got.enc, want.tables, want.enc, what)
    assert (got.refine_enc is None) == (want.refine_enc is None)
    if got.refine_enc is not None:
        _same_stream(torch, got.refine_tables, got.refine_enc, want.refine_tables, want.refine_enc,
                     (what, "level 2"))
    assert torch.equal(got.offsets, want.offsets), what
    perm = want.perm if ids is None else ids[want.perm]
    assert torch.equal(got.perm, perm), what
    inv = torch.full((got.n_ids,), -1, dtype=torch.int64, device="cuda")
    inv[perm] = torch.arange(perm.numel(), dtype=torch.int64, device="cuda")
    assert torch.equal(got.inv, inv), what
    assert got.inv.numel() == got.n_ids
    codec.decode_status(ctx)
    codec.ivf_status(ctx)


def _searches(ivf, qd, kind, keep=None):
    """every schedule, k and refine of the issue, as raw bits"""
    out = []
    for schedule in ("query", "list"):
        for k in (1, 64):
            for refine in ((0, 64) if kind == "refine" else (0,)):
                dist, ids = ivf.search(qd, 4, k, schedule=schedule, refine=refine, keep=keep)
                out.append((dist.cpu().numpy().view(np.uint32), ids.cpu().numpy()))
    return out


def _same_results(a, b, ids=None, what=""):
    assert len(a) == len(b)
    for (ad, ai), (bd, bi) in zip(a, b):
        if ids is not None:
            bi = np.where(bi >= 0, ids[np.maximum(bi, 0)], bi)
        assert np.array_equal(ai, bi), what
        assert np.array_equal(ad, bd), what


# ------------------------------------------------------------------------------ add
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("context", [True, False])
@pytest.mark.parametrize("chunk", [7, 64])
def test_add_equals_build(gpu, world, chunk, context, kind):
    """build(x[:400]) then add(x[400:1002]), add of one row and add of none: the index of
    build(x).  (No test or document says that build() takes an empty x, so the first batch has
    rows; the next test starts from one.)"""
    torch, codec, ctx = gpu
    w = world
    ivf = _build(gpu, w, w["xd"][:400], kind, chunk, context)
    assert ivf.n_ids == 400
    assert ivf.add(w["xd"][400:1002]) == 400 and ivf.n_ids == 1002
    assert ivf.add(w["xd"][1002:]) == 1002 and ivf.n_ids == N
    before = (ivf.enc, ivf.perm, ivf.offsets)
    assert ivf.add(w["xd"][:0]) == N and ivf.n_ids == N
    assert all(a is b for a, b in zip(before, (ivf.enc, ivf.perm, ivf.offsets)))   # nothing touched
    want = _build(gpu, w, w["xd"], kind, chunk, context)
    assert (np.diff(want.offsets.cpu().numpy()) == 0).sum() >= 2       # the two far lists
    _same_index(gpu, ivf, want, what=(chunk, context, kind))
    assert ivf.live is None and ivf.live_count() == N
    _same_results(_searches(ivf, w["qd"], kind), _searches(want, w["qd"], kind))
    ids = torch.tensor([0, 399, 400, 1001, 1002], dtype=torch.int64, device="cuda")
    assert torch.equal(ivf.fetch(ids), want.fetch(ids))
    codec.decode_status(ctx)


def test_add_to_a_one_row_index(gpu, world):
    """the smallest first batch: one row, then all the others"""
    torch, codec, ctx = gpu
    w = world
    for kind in KINDS:
        ivf = _build(gpu, w, w["xd"][:1], kind, 7, True)
        assert ivf.add(w["xd"][1:]) == 1
        _same_index(gpu, ivf, _build(gpu, w, w["xd"], kind, 7, True), what=kind)


# ------------------------------------------------------------------------------ compact
def _removed(torch, ivf, seed):
    """300 random ids, every id of the longest list, the first and the last stream row"""
    rng = np.random.default_rng(seed)
    offsets = ivf.offsets.cpu().numpy()
    l = int(np.argmax(np.diff(offsets)))
    perm = ivf.perm.cpu().numpy()
    ids = np.concatenate([rng.choice(ivf.n_ids, 300, replace=False), perm[offsets[l]:offsets[l + 1]],
                          perm[[0, -1]]])
    return np.unique(ids)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("chunk,context", [(7, True), (64, False)])
def test_compact_equals_build_of_the_live_rows(gpu, world, chunk, context, kind):
    torch, codec, ctx = gpu
    w = world
    ivf = _build(gpu, w, w["xd"], kind, chunk, context)
    assert ivf.compact() == 0 and ivf.live is None                    # nothing removed: untouched
    gone = _removed(torch, ivf, 3)
    gone_d = torch.from_numpy(gone).cuda()
    ivf.remove(gone_d)
    alive = np.setdiff1d(np.arange(N), gone)
    alive_d = torch.from_numpy(alive).cuda()
    keep = torch.from_numpy(np.random.default_rng(4).random(N) < 0.5).cuda()
    before = _searches(ivf, w["qd"], kind), _searches(ivf, w["qd"], kind, keep)
    vectors = ivf.fetch(alive_d, refined=kind == "refine")
    nbytes, count = ivf.enc.nbytes, ivf.live_count()
    assert count == len(alive)

    assert ivf.compact() == len(gone)
    assert ivf.n_ids == N and ivf.live is None and ivf._live_words is None
    assert ivf.enc.nbytes < nbytes and ivf.enc.n == len(alive) and ivf.live_count() == count
    assert ivf.compact() == 0
    # the same bits from every search, and none of the removed ids
    after = _searches(ivf, w["qd"], kind), _searches(ivf, w["qd"], kind, keep)
    _same_results(after[0], before[0], what="compact")
    _same_results(after[1], before[1], what="compact, keep=")
    assert not np.isin(np.concatenate([ids.ravel() for _, ids in after[0]]), gone).any()
    # the index build() makes of the live rows, its rows carrying their old ids
    want = _build(gpu, w, w["xd"][alive_d], kind, chunk, context)
    _same_index(gpu, ivf, want, ids=alive_d, what=(chunk, context, kind))
    _same_results(after[0], _searches(want, w["qd"], kind), ids=alive)
    # a dropped id: remove() passes over it, fetch() reports it
    ivf.remove(gone_d[:5])
    assert ivf.live_count() == count
    _same_results(_searches(ivf, w["qd"], kind), after[0], what="remove of a dropped id")
    assert torch.equal(ivf.fetch(alive_d, refined=kind == "refine"), vectors)
    codec.decode_status(ctx)
    ivf.fetch(torch.cat([alive_d[:3], gone_d[:1]]))
    with pytest.raises(codec.PqhError) as err:
        codec.decode_status(ctx)
    assert err.value.status == -1
    codec.decode_status(ctx)

    # add after compact: ids go on from n_ids, and the index is build() of live + new
    more = torch.from_numpy(datagen.sift_like(77, 128, seed=33)).cuda()
    assert ivf.add(more) == N and ivf.n_ids == N + 77
    ids = torch.cat([alive_d, torch.arange(N, N + 77, dtype=torch.int64, device="cuda")])
    want = _build(gpu, w, torch.cat([w["xd"][alive_d], more]), kind, chunk, context)
    _same_index(gpu, ivf, want, ids=ids, what="add after compact")
    _same_results(_searches(ivf, w["qd"], kind), _searches(want, w["qd"], kind), ids=ids.cpu().numpy())


@pytest.mark.parametrize("kind", KINDS)
def test_remove_then_add_without_compact(gpu, world, kind):
    """add() drops nothing: the stream is build() of all rows, the removed ones stay out of
    every search and can still be fetched"""
    torch, codec, ctx = gpu
    w = world
    ivf = _build(gpu, w, w["xd"][:700], kind, 7, True)
    gone = np.unique(np.random.default_rng(5).choice(700, 200, replace=False))
    gone_d = torch.from_numpy(gone).cuda()
    ivf.remove(gone_d)
    assert ivf.add(w["xd"][700:]) == 700
    want = _build(gpu, w, w["xd"], kind, 7, True)
    _same_index(gpu, ivf, want, what=kind)
    assert ivf.live_count() == N - len(gone)
    live = np.ones(N, bool)
    live[gone] = False
    assert np.array_equal(ivf.live.cpu().numpy(), live[ivf.perm.cpu().numpy()])
    got = _searches(ivf, w["qd"], kind)
    assert not np.isin(np.concatenate([ids.ravel() for _, ids in got]), gone).any()
    _same_results(got, _searches(want, w["qd"], kind, torch.from_numpy(live).cuda()))
    assert torch.equal(ivf.fetch(gone_d), want.fetch(gone_d))
    codec.decode_status(ctx)
    # ... and a compact() afterwards is build() of the live rows
    assert ivf.compact() == len(gone)
    alive_d = torch.from_numpy(np.flatnonzero(live)).cuda()
    _same_index(gpu, ivf, _build(gpu, w, w["xd"][alive_d], kind, 7, True), ids=alive_d, what=kind)


# ------------------------------------------------------------------------------ failure
@pytest.mark.parametrize("kind", KINDS)
def test_a_failed_add_leaves_the_index_as_it_was(gpu, world, kind):
    torch, codec, ctx = gpu
    w = world
    ivf = _build(gpu, w, w["xd"][:500], kind, 7, True)
    ivf.remove(torch.tensor([3, 77], dtype=torch.int64, device="cuda"))
    fields = ("tables", "enc", "perm", "inv", "offsets", "refine_tables", "refine_enc", "live",
              "_live_words", "n_ids")
    state = {f: getattr(ivf, f) for f in fields}
    before = _searches(ivf, w["qd"], kind)
    for bad in (torch.zeros((5, 64), device="cuda"), torch.zeros((5, 130), device="cuda")):
        with pytest.raises(codec.PqhError):
            ivf.add(bad)
        for f in fields:
            assert getattr(ivf, f) is state[f], f
    _same_results(_searches(ivf, w["qd"], kind), before)
    codec.decode_status(ctx)
    codec.ivf_status(ctx)
