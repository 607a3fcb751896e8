"""The numpy restatement of the top-k merge (pqh_topk_merge, codec.merge_topk) and of the search
over a row-sharded index (shard.ShardedIVF), shared by tests/test_shard_search_cpu.py,
tests/test_gpu_merge.py, tests/test_gpu_zz_shard_search.py and tests/shard_search_worker.py,
with the data they use.  Nothing here calls the library.

A block's search is the references' that the single-GPU tests already use: ivf_ref (lists,
layout, probes), ivf_residual_ref (codes, tables, the scan) and refine_ref (the re-rank); the
merge is np.lexsort((id, dist)) per query."""
import numpy as np

import datagen
import ivf_ref
import ivf_residual_ref as ref
import refine_ref


def merge_topk_ref(dist, ids, id_base, k):
    """(dist float32 [nq][k], ids int64 [nq][k]) from dist / ids [parts][nq][k_in]: per query
    the entries with id >= 0, each id moved by its part's base (None: zeros), the k smallest by
    (dist, id), padded with (+inf, -1)"""
    dist = np.asarray(dist, np.float32)
    ids = np.asarray(ids, np.int64)
    parts, nq, _ = dist.shape
    base = np.zeros(parts, np.int64) if id_base is None else np.asarray(id_base, np.int64)
    wd = np.full((nq, k), np.inf, np.float32)
    wi = np.full((nq, k), -1, np.int64)
    for q in range(nq):
        d = dist[:, q, :].reshape(-1)
        i = (ids[:, q, :] + base[:, None]).reshape(-1)
        ok = ids[:, q, :].reshape(-1) >= 0
        d, i = d[ok], i[ok]
        order = np.lexsort((i, d))[:k]
        wd[q, :len(order)] = d[order]
        wi[q, :len(order)] = i[order]
    return wd, wi


def brute_topk(dist, ids, id_base, k):
    """merge_topk_ref said another way: a Python sort of (dist, id) tuples of the concatenation"""
    parts, nq, k_in = np.shape(dist)
    base = [0] * parts if id_base is None else [int(b) for b in id_base]
    wd = np.full((nq, k), np.inf, np.float32)
    wi = np.full((nq, k), -1, np.int64)
    for q in range(nq):
        cand = sorted((float(dist[p][q][j]), int(ids[p][q][j]) + base[p])
                      for p in range(parts) for j in range(k_in) if ids[p][q][j] >= 0)[:k]
        for j, (d, i) in enumerate(cand):
            wd[q, j], wi[q, j] = d, i
    return wd, wi


def tied_parts(parts, nq, k_in, seed, bases=None):
    """dist, ids [parts][nq][k_in] for the merge alone: distances from 8 distinct values, ids
    unique per query across the parts after the bases, a third of the entries padding at random
    positions, and some entries (finite, -1)"""
    rng = np.random.default_rng(seed)
    values = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 5.0, 8.0], np.float32)
    dist = values[rng.integers(0, 8, size=(parts, nq, k_in))]
    base = np.zeros(parts, np.int64) if bases is None else np.asarray(bases, np.int64)
    ids = np.empty((parts, nq, k_in), np.int64)
    for q in range(nq):
        g = rng.permutation(parts * k_in * 3)[:parts * k_in].reshape(parts, k_in).astype(np.int64)
        g = g * 7 + int(base.max())           # global ids, above every base
        ids[:, q, :] = g - base[:, None]
    pad = rng.random((parts, nq, k_in)) < 1.0 / 3.0
    dist[pad] = np.inf
    ids[pad] = -1
    ghost = rng.random((parts, nq, k_in)) < 0.05        # (finite, -1): to be ignored
    ids[ghost] = -1
    return dist, ids


# ------------------------------------------------------------------------------ a block's search
def block_search_ref(x, q, cc, cent, nprobe, k, residual=False, keep=None, removed=None,
                     refine=0, cent2=None):
    """(dist, ids) of codec.IVF.build(pq, coarse, x, residual=...).search(q, nprobe, k, ...):
    keep a bool over x's rows, removed the rows taken out, refine = c > 0 with the level-2
    codebook cent2: the c best of the scan re-ranked to k.  ids are rows of x."""
    n, nlist = x.shape[0], cc.shape[0]
    m, _, dsub = cent.shape
    lists, _ = ivf_ref.assign(x, cc)
    perm, offsets = ivf_ref.layout(lists, nlist)
    ptr, ranges, probes, _ = ivf_ref.probe(q, cc, nprobe, offsets)
    if residual:
        rows, bad = ref.residuals(x, cc, lists, perm)
        assert not bad.any()
        lut = ref.tables(q, cc, probes, cent)
    else:
        rows = x[perm]
        lut_q = np.stack([ivf_ref.dists(q[:, dsub * i:dsub * (i + 1)], cent[i]) for i in range(m)],
                         axis=1)
        lut = np.repeat(lut_q, nprobe, axis=0)
    codes = ref.pq_codes(rows, cent)
    ok = np.ones(n, bool) if keep is None else np.asarray(keep, bool).copy()
    if removed is not None:
        ok[np.asarray(removed, np.int64)] = False
    wd, srows = ref.search(lut, codes, refine or k, ptr, ranges, keep=ok[perm])
    if refine:
        left = rows - refine_ref.reconstruct(cent, codes)
        assert left.dtype == np.float32
        codes2 = ref.pq_codes(left, cent2)
        wd, srows = refine_ref.refine(q, srows, k, cent, codes, cent2, codes2,
                                      cc if residual else None, offsets if residual else None)
    return wd, np.where(srows >= 0, perm[np.maximum(srows, 0)], -1)


def sharded_search_ref(x, starts, q, cc, cent, nprobe, k, keep=None, removed=None, **kw):
    """(dist, ids) of ShardedIVF.search over the row blocks x[starts[r]:starts[r + 1]]: every
    block's block_search_ref, then merge_topk_ref with the block starts.  keep and removed are
    over the global ids."""
    ds, is_ = [], []
    for b, e in zip(starts[:-1], starts[1:]):
        kp = None if keep is None else keep[b:e]
        rm = None
        if removed is not None:
            removed = np.asarray(removed, np.int64)
            rm = removed[(removed >= b) & (removed < e)] - b
        d, i = block_search_ref(x[b:e], q, cc, cent, nprobe, k, keep=kp, removed=rm, **kw)
        ds.append(d)
        is_.append(i)
    return merge_topk_ref(np.stack(ds), np.stack(is_), starts[:-1], k)


def distinct_mask(dist):
    """bool [nq][k]: the positions whose distance differs from both neighbours' -- where the ids
    of a merged result and of one index must agree"""
    d = np.asarray(dist)
    m = np.ones(d.shape, bool)
    eq = d[:, 1:] == d[:, :-1]
    m[:, 1:] &= ~eq
    m[:, :-1] &= ~eq
    return m


# ------------------------------------------------------------------------------ the data
def search_world(n, d, nlist, nq, m, residual=False, seed=41, m2=0, spread=False):
    """rows, a coarse codebook of rows moved by 0.5, an m x 256 PQ trained on the rows (on the
    residuals for a residual index), queries near rows; m2 > 0: an m2 x 256 level-2 codebook
    trained on what the first leaves over.  The rows are datagen.sift_like's, or with spread
    independent normal ones: sift_like's heavy clusters give some 7 % of 3,001 rows the PQ code
    of another row at m = 4, and so equal distances, which a test of the ids has to avoid."""
    rng = np.random.default_rng(seed + 1)
    if spread:
        x = rng.normal(0.0, 30.0, size=(n, d)).astype(np.float32)
    else:
        x = datagen.sift_like(n, d, seed=seed)
    cc = (x[rng.choice(n, nlist, replace=False)] + np.float32(0.5)).astype(np.float32)
    lists, _ = ivf_ref.assign(x, cc)
    rows = ref.residuals(x, cc, lists)[0] if residual else x
    cent = datagen.lloyd_centroids(rows, m, 256, iters=2, sample=n)
    q = (x[rng.choice(n, nq, replace=False)] + rng.normal(0.0, 3.0, size=(nq, d))).astype(np.float32)
    w = dict(x=x, cc=cc, cent=cent, q=q)
    if m2:
        left = rows - refine_ref.reconstruct(cent, ref.pq_codes(rows, cent))
        w["cent2"] = datagen.lloyd_centroids(left, m2, 256, iters=2, sample=n)
    return w


def block_starts(n, sizes=None, world=None):
    """[0, ..., n]: the starts of `world` even row blocks (the sizes of pqh_shard_block), or of
    blocks of the given sizes"""
    if sizes is None:
        base, extra = divmod(n, world)
        sizes = [base + (1 if r < extra else 0) for r in range(world)]
    assert sum(sizes) == n
    return [0] + list(np.cumsum(sizes))
