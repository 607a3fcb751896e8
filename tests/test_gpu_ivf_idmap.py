"""codec.IVF with compressed ids on the GPU.  The yardstick is the index itself with its int64
perm and inv: twins are built from the same data, one of them with compress_ids=True and one
converted by compress_ids(), and every call must return the same bits on all three -- ids are
integers and the scans do not look at them, so a difference is a bug.  After every step of a
life cycle the compressed twin's blob is the IdMap of the plain twin's perm, byte for byte."""
import numpy as np
import pytest

import datagen
import idmap_ref as ref

pytestmark = pytest.mark.gpu

N, N0, NLIST, M, NQ = 2300, 1800, 16, 8, 9
KINDS = ("plain", "residual", "refine")


@pytest.fixture(scope="module")
def gpu():
    import torch
    from pq_huffman_amd import codec
    assert torch.cuda.is_available()
    return torch, codec, codec.Context(0)


@pytest.fixture(scope="module")
def world(gpu):
    """2,300 SIFT-like rows, an 8 x 256 PQ, a 16 x 256 second codebook, nine queries and 16
    lists, one of them far from the data: an empty list"""
    torch, codec, ctx = gpu
    x = datagen.sift_like(N, 128, seed=41)
    rng = np.random.default_rng(42)
    cc = (x[rng.choice(N0, NLIST - 1, replace=False)] + np.float32(0.5)).astype(np.float32)
    cc = np.concatenate([cc[:6], np.full((1, 128), -5000.0, np.float32), cc[6:]])
    cent = datagen.lloyd_centroids(x, M, 256, iters=2, sample=N)
    cent2 = datagen.lloyd_centroids((x - x.mean(axis=0)) * np.float32(0.25), 16, 256, iters=1, sample=N)
    q = (x[rng.choice(N, NQ, replace=False)] +
         rng.normal(0.0, 3.0, size=(NQ, 128))).astype(np.float32)
    return dict(xd=torch.from_numpy(x).cuda(), qd=torch.from_numpy(q).cuda(),
                pq=codec.PQ(ctx, cent), pq2=codec.PQ(ctx, cent2), coarse=codec.Coarse(ctx, cc))


def _build(gpu, w, xd, kind, chunk, **kw):
    torch, codec, ctx = gpu
    return codec.IVF.build(ctx, w["pq"], w["coarse"], xd, chunk_vectors=chunk,
                           residual=kind == "residual",
                           refine_pq=w["pq2"] if kind == "refine" else None, **kw)


def _twins(gpu, w, xd, kind, chunk):
    """(plain, built compressed, converted)"""
    plain = _build(gpu, w, xd, kind, chunk)
    built = _build(gpu, w, xd, kind, chunk, compress_ids=True)
    converted = _build(gpu, w, xd, kind, chunk)
    before = converted.id_bytes()
    assert before == 16 * xd.shape[0]
    assert converted.compress_ids() == before - converted.id_bytes() > 0
    assert converted.compress_ids() == 0                      # already compressed: untouched
    return plain, built, converted


def _same(torch, a, b, what):
    assert len(a) == len(b), what
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and torch.equal(x, y), what


def _check_state(gpu, plain, twin, what):
    """the compressed twin holds the map of the plain twin's perm and nothing else"""
    torch, codec, ctx = gpu
    assert twin.perm is None and twin.inv is None, what
    want = codec.IdMap(ctx, plain.perm, plain.offsets, plain.n_ids)
    assert torch.equal(twin.idmap.blob, want.blob), what
    assert torch.equal(twin.offsets, plain.offsets), what
    assert (twin.n_ids, twin.live_count(), twin.enc.n) == (plain.n_ids, plain.live_count(), plain.enc.n)
    n, n_ids = plain.enc.n, plain.n_ids
    assert plain.id_bytes() == 8 * n + 8 * n_ids
    assert twin.id_bytes() == twin.idmap.nbytes <= codec.idmap_bytes(n, n_ids, NLIST)
    # derived: L + 3 bits a row and 16 bits an id against 64 + 64, L <= 5 at these sizes
    assert ref.shape(n, n_ids, NLIST)["L"] <= 5
    assert twin.id_bytes() == ref.idmap_bytes(n, n_ids, NLIST)
    if n >= 1024:
        assert 4 * twin.id_bytes() < plain.id_bytes(), what
    codec.ivf_status(ctx)
    codec.decode_status(ctx)


def _searches(torch, ivf, qd, kind, keep=None):
    out = []
    for schedule in ("query", "list", "auto"):
        for k in (1, 64):
            out += ivf.search(qd, 4, k, schedule=schedule, keep=keep)
            if kind == "refine":
                out += ivf.search(qd, 4, k, schedule=schedule, keep=keep, refine=64)
    # nq * nprobe >= 4 * nlist: "auto" takes the list-major form
    out += ivf.search(torch.cat([qd] * 8), 4, 10, schedule="auto", keep=keep)
    return out


def _range_searches(torch, ivf, qd, radius, keep=None):
    out = list(ivf.range_search(qd, 4, radius, keep=keep))
    out += ivf.range_search(qd, 4, float(radius.max().item()), keep=keep)
    return out


def _everything(gpu, w, ivf, kind, keep, radius, ids):
    torch, codec, ctx = gpu
    out = _searches(torch, ivf, w["qd"], kind) + _searches(torch, ivf, w["qd"], kind, keep)
    out += _range_searches(torch, ivf, w["qd"], radius) + _range_searches(torch, ivf, w["qd"], radius, keep)
    out.append(ivf.fetch(ids))
    if kind == "refine":
        out.append(ivf.fetch(ids, refined=True))
    return out


def _radius(torch, ivf, qd):
    dist, _ = ivf.search(qd, 4, 64)
    return dist[:, 20].contiguous()


# ------------------------------------------------------------------------------ call by call
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("chunk", [4, 64])
def test_every_call_gives_the_plain_index_bits(gpu, world, chunk, kind):
    torch, codec, ctx = gpu
    w = world
    plain, built, converted = _twins(gpu, w, w["xd"][:N0], kind, chunk)
    for twin in (built, converted):
        _check_state(gpu, plain, twin, (kind, chunk))
    keep = torch.from_numpy(np.random.default_rng(43).random(N0) < 0.4).cuda()
    radius = _radius(torch, plain, w["qd"])
    ids = torch.tensor([0, 1, 999, N0 - 1, 5, 5], dtype=torch.int64, device="cuda")
    want = _everything(gpu, w, plain, kind, keep, radius, ids)
    assert int(want[-1].numel()) > 0
    lims = plain.range_search(w["qd"], 4, radius)[0]
    assert int(lims[-1].item()) >= NQ                        # the range searches return rows
    for twin in (built, converted):
        _same(torch, _everything(gpu, w, twin, kind, keep, radius, ids), want, (kind, chunk))
    codec.ivf_status(ctx)
    codec.decode_status(ctx)


def test_range_search_in_slabs(gpu, world):
    """a residual index whose tables do not fit the budget: the queries go slab by slab, the
    rows of all slabs through one lookup"""
    torch, codec, ctx = gpu
    w = world
    plain, built, _ = _twins(gpu, w, w["xd"][:N0], "residual", 64)
    radius = _radius(torch, plain, w["qd"])
    keep = torch.from_numpy(np.random.default_rng(44).random(N0) < 0.5).cuda()
    for ivf in (plain, built):
        ivf.table_budget = 2 * 4 * M * 256 * 4                # two queries a slab: five slabs
    for kp in (None, keep):
        _same(torch, built.range_search(w["qd"], 4, radius, keep=kp),
              plain.range_search(w["qd"], 4, radius, keep=kp), "slabs")
        _same(torch, built.search(w["qd"], 4, 64, keep=kp), plain.search(w["qd"], 4, 64, keep=kp),
              "slabs")
    empty = built.range_search(w["qd"][:0], 4, 1.0)
    assert empty[2].numel() == 0 and empty[2].dtype == torch.int64
    codec.ivf_status(ctx)


# ------------------------------------------------------------------------------ life cycle
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("chunk", [4, 64])
def test_life_cycle(gpu, world, chunk, kind):
    """remove -> search -> add -> search -> compact -> add -> search, the twins side by side"""
    torch, codec, ctx = gpu
    w = world
    plain, built, converted = _twins(gpu, w, w["xd"][:N0], kind, chunk)
    twins = (built, converted)
    rng = np.random.default_rng(45)
    fetch_ids = torch.tensor([0, 7, N0 - 1], dtype=torch.int64, device="cuda")

    def compare(step):
        keep = torch.from_numpy(rng.random(plain.n_ids) < 0.5).cuda()
        radius = _radius(torch, plain, w["qd"])
        want = _everything(gpu, w, plain, kind, keep, radius, fetch_ids)
        for twin in twins:
            _check_state(gpu, plain, twin, (step, kind, chunk))
            _same(torch, _everything(gpu, w, twin, kind, keep, radius, fetch_ids), want,
                  (step, kind, chunk))
            assert (twin.live is None) == (plain.live is None)
            if plain.live is not None:
                assert torch.equal(twin.live, plain.live) and \
                    torch.equal(twin._live_words, plain._live_words)

    gone = torch.from_numpy(np.unique(rng.choice(np.arange(10, N0 - 10), 700, replace=False))).cuda()
    for ivf in (plain,) + twins:
        ivf.remove(gone)
    compare("remove")
    firsts = [ivf.add(w["xd"][N0:N - 77]) for ivf in (plain,) + twins]
    assert firsts == [N0] * 3
    compare("add")
    dropped = [ivf.compact() for ivf in (plain,) + twins]
    assert dropped == [gone.numel()] * 3
    assert plain.enc.n == N - 77 - gone.numel() >= 1024
    compare("compact")
    for ivf in (plain,) + twins:                               # a dropped id: passed over
        ivf.remove(gone[:5])
    compare("remove of a dropped id")
    # a dropped id is fetched as on the plain index: the same vectors and the decode status
    got = []
    for ivf in (plain,) + twins:
        got.append(ivf.fetch(torch.cat([fetch_ids, gone[:1]])))
        with pytest.raises(codec.PqhError) as err:
            codec.decode_status(ctx)
        assert err.value.status == -1
    assert torch.equal(got[1], got[0]) and torch.equal(got[2], got[0])
    firsts = [ivf.add(w["xd"][N - 77:]) for ivf in (plain,) + twins]
    assert firsts == [N - 77] * 3 and plain.n_ids == N
    compare("add after compact")
    assert [ivf.compact() for ivf in (plain,) + twins] == [0] * 3       # nothing removed since


@pytest.mark.parametrize("kind", KINDS)
def test_a_failed_add_leaves_the_compressed_index_as_it_was(gpu, world, kind):
    torch, codec, ctx = gpu
    w = world
    ivf = _build(gpu, w, w["xd"][:500], kind, 4, compress_ids=True)
    ivf.remove(torch.tensor([3, 77], dtype=torch.int64, device="cuda"))
    fields = ("tables", "enc", "perm", "inv", "idmap", "offsets", "refine_tables", "refine_enc",
              "live", "_live_words", "n_ids")
    state = {f: getattr(ivf, f) for f in fields}
    blob = ivf.idmap.blob.clone()
    before = _searches(torch, ivf, w["qd"], kind)
    for bad in (torch.zeros((5, 64), device="cuda"), torch.zeros((5, 130), device="cuda")):
        with pytest.raises(codec.PqhError):
            ivf.add(bad)
        for f in fields:
            assert getattr(ivf, f) is state[f], f
    assert ivf.perm is None and ivf.inv is None and torch.equal(ivf.idmap.blob, blob)
    _same(torch, _searches(torch, ivf, w["qd"], kind), before, kind)
    codec.decode_status(ctx)
    codec.ivf_status(ctx)
