"""The numpy reference of the refinement codes (pqh_refine_stream, pqh_refine_codes,
codec.refine, codec.IVF with refine_pq), shared by tests/test_refine_cpu.py and
tests/test_gpu_refine.py, with the inputs both use.  Nothing here calls the library.

Every value is a float32 array operation of numpy, which rounds each operation to float32 and
fuses nothing.  A row has two codes, a (level 1) and b (level 2):
    y = concat_i cent1[i][a_i] + concat_i cent2[i][b_i]          one add per dimension
    t = q - y                  residual index: t = (q - c[l]) - y, l the list of the row
    dist = ivf_ref.dists' chain over all d dimensions: acc = 0; acc = acc + t_j * t_j
and every order is np.lexsort((row, dist))."""
import numpy as np

import datagen
import ivf_ref
import ivf_residual_ref as ref


def reconstruct(cent, codes):
    """float32 [rows][m * dsub]: concat_i cent[i][codes[:, i]]"""
    return np.concatenate([cent[i][codes[:, i]] for i in range(cent.shape[0])], axis=1)


def lists_of(offsets, rows):
    """the last list l with offsets[l] <= row: the rule of IVF.fetch, which passes over the
    empty lists that end where the row's list begins"""
    return np.searchsorted(np.asarray(offsets)[1:], rows, side="right")


def dists(q, cent1, a, cent2, b, c=None):
    """float32 [rows]: the distance of one query q [d] to the rows with codes a [rows][m1] and
    b [rows][m2]; c: float32 [rows][d], the coarse centroid of every row's list, or None"""
    q = np.asarray(q, np.float32)
    y = reconstruct(cent1, a) + reconstruct(cent2, b)
    d = y.shape[1]
    ql = np.broadcast_to(q[None, :d], y.shape) if c is None else q[None, :d] - c
    t = ql - y
    assert y.dtype == np.float32 and t.dtype == np.float32
    acc = np.zeros(y.shape[0], np.float32)
    for j in range(d):
        acc = acc + t[:, j] * t[:, j]
    assert acc.dtype == np.float32
    return acc


def refine(q, rows, top_k, cent1, codes1, cent2, codes2, coarse=None, offsets=None):
    """(dist float32 [nq][top_k], ids int64 [nq][top_k]): of the candidates rows[q] (-1 is
    padding, rows outside [0, n) are dropped, a row given twice counts twice) the top_k smallest
    by (dist, row), padded with (+inf, -1)"""
    rows = np.asarray(rows, np.int64)
    n = codes1.shape[0]
    nq = rows.shape[0]
    wd = np.full((nq, top_k), np.inf, np.float32)
    wi = np.full((nq, top_k), -1, np.int64)
    for i in range(nq):
        r = rows[i][(rows[i] >= 0) & (rows[i] < n)]
        c = None if coarse is None else coarse[lists_of(offsets, r)]
        dist = dists(q[i], cent1, codes1[r], cent2, codes2[r], c)
        order = np.lexsort((r, dist))[:top_k]
        wd[i, :len(order)] = dist[order]
        wi[i, :len(order)] = r[order]
    return wd, wi


def dists_int64(q, cent1, a, cent2, b, c=None):
    """the same distance in int64 arithmetic, for integer-valued inputs"""
    y = reconstruct(cent1, a).astype(np.int64) + reconstruct(cent2, b).astype(np.int64)
    t = np.asarray(q).astype(np.int64)[None, :y.shape[1]] - y
    if c is not None:
        t = t - np.asarray(c).astype(np.int64)
    return (t * t).sum(axis=1)


# ------------------------------------------------------------------------------ the sweep
N = 1003                                        # no multiple of a chunk, of 32 or of 64
SHAPES = ((8, 4, 8, 4), (8, 4, 16, 2), (3, 5, 5, 3))   # (m1, dsub1, m2, dsub2)
KS = (256, 16)
CHUNKS = ((1, 1), (4, 7), (64, 4))              # (C1, C2)
NQS = (1, 5)
CANDS = ((1, 1), (10, 1), (10, 10), (64, 1), (64, 64))   # (ncand, top_k)


def sweep_world(shape, k):
    """codes of both levels (datagen.skewed_codes), random float codebooks, five queries"""
    m1, ds1, m2, ds2 = shape
    rng = np.random.default_rng(1000 * m1 + 10 * m2 + k)
    return dict(codes1=datagen.skewed_codes(N, m1, k=k, seed=300 + m1 + k),
                codes2=datagen.skewed_codes(N, m2, k=k, seed=400 + m2 + k),
                cent1=rng.normal(0.0, 20.0, size=(m1, k, ds1)).astype(np.float32),
                cent2=rng.normal(0.0, 5.0, size=(m2, k, ds2)).astype(np.float32),
                q=rng.normal(0.0, 25.0, size=(max(NQS), m1 * ds1)).astype(np.float32))


def candidates(nq, ncand, chunks, seed):
    """int64 [nq][ncand].  From ten candidates on every query has: row 0 (the raw row in context
    mode), row N - 1, the first and the last row of a level-1 chunk and of a level-2 chunk (two
    rows of one chunk where a chunk has two), a duplicate, and -1 at positions 3 and 6.  A list
    of one candidate is one of those rows, another one for every query."""
    c1, c2 = chunks
    rng = np.random.default_rng(seed)
    special = [0, N - 1, 3 * c1, 3 * c1 + c1 - 1, 5 * c2, 5 * c2 + c2 - 1]
    out = np.empty((nq, ncand), np.int64)
    for i in range(nq):
        if ncand < 10:
            out[i] = [special[(i + j) % len(special)] for j in range(ncand)]
            continue
        body = special + [special[3]] + rng.integers(0, N, size=ncand - 9).tolist()
        body = [body[j] for j in rng.permutation(len(body))]
        out[i] = body[:3] + [-1] + body[3:5] + [-1] + body[5:]
    return out


def check_candidates(rows, chunks):
    c1, c2 = chunks
    if rows.shape[1] < 10:
        return
    for r in rows:
        assert r[3] == -1 and r[6] == -1 and (np.delete(r, [3, 6]) >= 0).all()
        assert {0, N - 1, 3 * c1, 4 * c1 - 1, 5 * c2, 6 * c2 - 1} <= set(r.tolist())
        assert len(set(r.tolist())) < len(r) - 1          # a duplicate beside the two -1
        if c1 > 1:
            assert 3 * c1 != 4 * c1 - 1                   # two rows of one chunk


# ------------------------------------------------------------------------------ ties
def ties_world(seed=5):
    """integer-grid data: codebooks with entries in [-4, 4] (their sum in [-8, 8]), queries in
    [-8, 8], d = 16 -- every partial sum an integer below 2^24, so float32 is exact -- and the
    rows 200 ... 399 copies of the rows 0 ... 199, so equal distances are certain"""
    rng = np.random.default_rng(seed)
    m1, ds1, m2, ds2, k = 4, 4, 8, 2, 16
    w = dict(cent1=rng.integers(-4, 5, size=(m1, k, ds1)).astype(np.float32),
             cent2=rng.integers(-4, 5, size=(m2, k, ds2)).astype(np.float32),
             codes1=rng.integers(0, k, size=(400, m1)).astype(np.uint8),
             codes2=rng.integers(0, k, size=(400, m2)).astype(np.uint8),
             q=ivf_ref.integer_grid(4, 16, 1, seed + 1)[0])
    w["codes1"][200:] = w["codes1"][:200]
    w["codes2"][200:] = w["codes2"][:200]
    base = rng.permutation(200)[:32]
    w["rows"] = np.stack([rng.permutation(np.concatenate([base, base + 200])) for _ in range(4)])
    return w


# ------------------------------------------------------------------------------ the residual form
def residual_world(d, seed=0):
    """37 lists, several of them empty, over N rows; m1 = 5 or 8 parts and m2 = 3 or 16; the
    candidates of every query hold the first row of each list that follows an empty one"""
    rng = np.random.default_rng(700 + d + seed)
    nlist = 37
    m1, m2 = (5, 3) if d == 15 else (8, 16)
    sizes = rng.multinomial(N, np.ones(nlist) / nlist)
    for l in (0, 7, 8, 20, 36):                  # empty lists: the first, two in a row, the last
        sizes[l + 1 if l < 36 else 35] += sizes[l]
        sizes[l] = 0
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    assert offsets[-1] == N
    after_empty = [int(offsets[l]) for l in range(1, nlist) if sizes[l - 1] == 0 and sizes[l] > 0]
    rows = np.stack([np.concatenate([after_empty, [a - 1 for a in after_empty if a > 0], [0, N - 1],
                                     rng.integers(0, N, size=20)]) for _ in range(5)])
    return dict(offsets=offsets, after_empty=after_empty, rows=rows.astype(np.int64),
                coarse=rng.normal(0.0, 30.0, size=(nlist, d)).astype(np.float32),
                cent1=rng.normal(0.0, 20.0, size=(m1, 256, d // m1)).astype(np.float32),
                cent2=rng.normal(0.0, 5.0, size=(m2, 256, d // m2)).astype(np.float32),
                codes1=datagen.skewed_codes(N, m1, seed=31 + d),
                codes2=datagen.skewed_codes(N, m2, seed=32 + d),
                q=rng.normal(0.0, 25.0, size=(5, d)).astype(np.float32))


def check_residual_world(w):
    off = w["offsets"]
    assert (np.diff(off) == 0).sum() >= 5 and len(w["after_empty"]) >= 3
    for r in w["after_empty"]:
        l = lists_of(off, r)
        assert off[l] == r and off[l - 1] == r and off[l + 1] > r      # the list after an empty one
        assert np.isin(r, w["rows"]).all()
    assert w["rows"].shape[1] <= 64


# ------------------------------------------------------------------------------ the index
def ivf_refine_world(w, kind):
    """for search_filter_ref.ivf_world() and a kind ("plain", "residual"): the level-2 codebook
    trained on what the 8 x 256 PQ leaves over of the stream's rows, and its codes"""
    x, perm, cent = w["x"], w["perm"], w["cent"]
    if kind == "residual":
        rows = (x[perm] - w["cc"][lists_of(w["offsets"], np.arange(len(perm)))]).astype(np.float32)
    else:
        rows = x[perm]
    left = rows - reconstruct(cent, w[kind]["codes"])
    assert left.dtype == np.float32
    cent2 = datagen.lloyd_centroids(left, 16, 256, iters=2, sample=1003)
    return dict(left=left, cent2=cent2, codes2=ref.pq_codes(left, cent2))


def ivf_candidates(w, kind, c=64, keep=None, removed=None):
    """(dist, stream rows): the c best rows of the ADC scan, ivf_residual_ref.search; keep a bool
    over the caller's rows or None, removed the caller rows taken out"""
    ok = np.ones(len(w["perm"]), bool) if keep is None else np.asarray(keep, bool).copy()
    if removed is not None:
        ok[removed] = False
    return ref.search(w[kind]["lut"], w[kind]["codes"], c, w["ptr"], w["ranges"],
                      keep=ok[w["perm"]])


def ivf_refined(w, kind, r2, cand, k):
    """(dist, stream rows) of the refinement of the candidates `cand`"""
    res = kind == "residual"
    return refine(w["q"], cand, k, w["cent"], w[kind]["codes"], r2["cent2"], r2["codes2"],
                  w["cc"] if res else None, w["offsets"] if res else None)
