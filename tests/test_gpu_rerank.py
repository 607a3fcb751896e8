"""The exact re-rank on the GPU (codec.rerank, IVF.search(rerank=)) against tests/rerank_ref.py:
ids equal and dist equal bit for bit, for fp32, fp16, bf16 and SQ8 stores and both metrics."""
import numpy as np
import pytest

import datagen
import rerank_ref
import sq_ref

pytestmark = pytest.mark.gpu
STORES = ["f32", "f16", "bf16", "sq8"]
DTYPE = {"f32": "float32", "f16": "float16", "bf16": "bfloat16", "sq8": "uint8"}
N = 300
# A segment is 128 bytes of a row: d below one, at the fp32 edge, one past it, several with a ragged
# last one, and ("edge") one element past each type's own first segment.
EDGE = {"f32": 33, "f16": 65, "bf16": 65, "sq8": 129}
DS = [1, 3, 32, 33, 130, "edge"]
# "vec": rows and base on 4 bytes (the 16-byte loads); "odd": an odd distance between rows (fp32
# rows stay on 4 bytes, the others take the element loads); "shift": the base one element on
LAYOUTS = ["vec", "odd", "shift"]
# name: (ncand, k, d, nq, layout).  ncand up to 64 runs one wave on the default context, above it
# the wide form on a context raised to 256; k is 1, ncand and a value between; d, nq and the
# layout walk their lists so that every d meets every layout.
CASES = {"extremes": (64, 64, 32, 5, "vec")}
for a, ncand in enumerate([1, 63, 64, 65, 200, 256]):
    for b, k in enumerate(sorted({1, (ncand + 1) // 2, ncand})):
        i = 3 * a + b
        CASES[f"c{ncand}_k{k}"] = (ncand, k, DS[i % 6], (1, 5)[i % 2], LAYOUTS[(i + i // 6) % 3])


@pytest.fixture(scope="module")
def gpu():
    import torch
    from pq_huffman_amd import codec
    assert torch.cuda.is_available()
    return torch, codec, codec.Context(0), codec.Context(0).set_search_max_k(256)


def _device(torch, a, store, layout):
    """a as a device tensor of the store's type in the layout: NaN (255 for codes) everywhere
    between the rows, past d and in front of a shifted base"""
    n, d = a.shape
    ld = {"vec": (d + 3) // 4 * 4 + 4, "odd": (d + 2) | 1, "shift": (d + 3) // 4 * 4}[layout]
    shift = 1 if layout == "shift" else 0
    fill = 255 if store == "sq8" else float("nan")
    flat = torch.full((n * ld + shift,), fill, dtype=getattr(torch, DTYPE[store]), device="cuda")
    buf = flat[shift:].view(n, ld)
    buf[:, :d] = torch.from_numpy(a).to(buf.dtype)
    return buf


def _world(store, d, nq, ncand, rng, extremes=False):
    """(rows as the reference sees them, the store's own array, sq, queries, candidates):
    duplicated rows, a query that is a copy of a row, an id named twice, -1 in the middle and at
    the end, and a last query of -1 alone"""
    x = rng.standard_normal((N, d)).astype(np.float32)
    if extremes:   # the ends of fp16: +-65504, the smallest subnormal, -0.0
        for v in (65504.0, -65504.0, 2.0 ** -24, -2.0 ** -24, -0.0):
            x[rng.integers(0, N, 40), rng.integers(0, d, 40)] = v
    if store == "f16":   # every value one of the store's type
        x = x.astype(np.float16).astype(np.float32)
    if store == "bf16":
        x = (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    x[N // 2:] = x[:N // 2]
    q = rng.standard_normal((nq, d)).astype(np.float32)
    cand = rng.integers(0, N, (nq, ncand)).astype(np.int64)
    q[0] = x[cand[0, 0]]
    if ncand >= 4:
        cand[:, 1] = cand[:, 0]
        cand[:, 2] = (cand[:, 0] + N // 2) % N   # the same row under another id
        cand[:, ncand // 2] = -1
        cand[::2, -1] = -1
    if nq > 1:
        cand[-1] = -1
    sq = sq_ref.train(x) if store == "sq8" else None
    return x, (sq_ref.encode(x, *sq) if sq else x), sq, q, cand


def _store(gpu, store, own, sq, layout):
    t = _device(gpu[0], own, store, layout)
    return t if sq is None else (gpu[1].SQ(gpu[2], *(gpu[0].from_numpy(v).cuda() for v in sq)), t)


def _equal(got, want):
    got = [t.cpu().numpy() for t in got[:2]]
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("store", STORES)
def test_rerank(gpu, store, metric, case):
    torch, codec, ctx, wide = gpu
    ncand, k, d, nq, layout = CASES[case]
    d = EDGE[store] if d == "edge" else d
    rng = np.random.default_rng(1000 * ncand + k)
    x, own, sq, q, cand = _world(store, d, nq, ncand, rng, extremes=case == "extremes")
    c = wide if ncand > 64 else ctx
    got = codec.rerank(c, _store(gpu, store, own, sq, layout), torch.from_numpy(q).cuda(),
                       torch.from_numpy(cand).cuda(), k, metric=metric, d=d)
    codec.ivf_status(c)
    want = rerank_ref.rerank(q, own, cand, k, metric, sq)
    assert not want[2]
    _equal(got, want)


@pytest.mark.parametrize("store", STORES)
def test_bad_ids_are_dropped_and_reported(gpu, store):
    torch, codec, ctx, _ = gpu
    x, own, sq, q, cand = _world(store, 33, 5, 64, np.random.default_rng(7))
    cand[1, 5], cand[3, 60] = -2, N
    st, qd = _store(gpu, store, own, sq, "vec"), torch.from_numpy(q).cuda()
    got = codec.rerank(ctx, st, qd, torch.from_numpy(cand).cuda(), 64, d=33)
    with pytest.raises(codec.PqhError):
        codec.ivf_status(ctx)
    want = rerank_ref.rerank(q, own, cand, 64, "l2", sq)
    assert want[2] == {-2, N}
    _equal(got, want)
    cand[1, 5], cand[3, 60] = -1, 0
    out = tuple(t[:, :64] for t in (torch.empty((5, 70), device="cuda"),
                                    torch.empty((5, 70), dtype=torch.int64, device="cuda")))
    _equal(codec.rerank(ctx, st, qd, torch.from_numpy(cand).cuda(), 64, d=33, out=out),
           rerank_ref.rerank(q, own, cand, 64, "l2", sq))
    codec.ivf_status(ctx)   # the next clean call: nothing to report


@pytest.mark.parametrize("form", ["plain", "residual", "compressed"])
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_index_reranks_its_candidates(gpu, metric, form):
    torch, codec, ctx, _ = gpu
    n, d, nlist, nq, k, c = 3000, 16, 8, 12, 10, 64
    x = datagen.sift_like(n + 200, d, seed=3)
    q = datagen.sift_like(nq, d, seed=4)
    xd, qd = torch.from_numpy(x).cuda(), torch.from_numpy(q).cuda()
    pq = codec.PQ(ctx, datagen.lloyd_centroids(x, 4, 256, iters=1, sample=n))
    coarse = codec.Coarse(ctx, x[:nlist].copy())
    ivf = codec.IVF.build(ctx, pq, coarse, xd[:n], chunk_vectors=7, metric=metric,
                          residual=form == "residual", compress_ids=form == "compressed")

    def check(store, **kw):
        cand = ivf.search(qd, nlist, c, **kw)[1].cpu().numpy()
        _equal(ivf.search(qd, nlist, k, rerank=c, **kw), rerank_ref.rerank(q, store, cand, k, metric))

    with pytest.raises(codec.PqhError):   # no store yet
        ivf.search(qd, nlist, k, rerank=c)
    ivf.set_rows(xd[:n])
    check(x)
    check(x, schedule="list")
    keep = torch.from_numpy(np.random.default_rng(5).random(n) < 0.5).cuda()
    check(x, keep=keep)
    ivf.remove(ivf.search(qd, nlist, 1)[1][:, 0])
    assert ivf.add(xd[n:]) == n
    with pytest.raises(codec.PqhError):   # the store of before add(): fewer rows than ids
        ivf.search(qd, nlist, k, rerank=c)
    ivf.set_rows(xd)
    check(x)
    for bad in (dict(rerank=k - 1), dict(rerank=65), dict(rerank=c, refine=c)):
        with pytest.raises(codec.PqhError):
            ivf.search(qd, nlist, k, **bad)
    ivf.set_rows(None)
    with pytest.raises(codec.PqhError):
        ivf.search(qd, nlist, k, rerank=c)
    codec.ivf_status(ctx)
