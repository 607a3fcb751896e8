"""The numpy reference of the inner-product metric (pqh_adc_tables_ip, pqh_coarse_assign_ip,
pqh_coarse_probe_ip, pqh_adc_tables_residual_ip, pqh_refine_*_ip, codec.IVF with metric="ip"),
shared by tests/test_metric_cpu.py, tests/test_gpu_metric.py and tests/test_gpu_ivf_metric.py.
Nothing here calls the library.

A score is the negated inner product, smaller is nearer:
    nip(x, y):  acc = +0.0;  for j ascending:  acc = acc - x[j] * y[j]
Every step is a float32 array operation of numpy, which rounds the multiply and the subtract to
float32 each and fuses nothing -- a sequential chain, never a vectorised dot -- so the bits are
those of the definition, the sign of a zero included.  Every order is np.lexsort((ids, score)).
The L2 twins of everything here are ivf_ref, ivf_residual_ref and refine_ref."""
import numpy as np

import ivf_ref
import ivf_residual_ref as rref
import range_ref
import refine_ref


# ------------------------------------------------------------------------------ the chain
def nip(x, c):
    """float32 [n][nlist]: nip(x[v], c[l]) over all the columns of x"""
    x = np.ascontiguousarray(x, np.float32)
    c = np.ascontiguousarray(c, np.float32)
    acc = np.zeros((x.shape[0], c.shape[0]), np.float32)
    for j in range(x.shape[1]):
        acc = acc - x[:, j:j + 1] * c[None, :, j]
    assert acc.dtype == np.float32
    return acc


def nip_int64(x, c):
    """the same in int64 arithmetic, for integer-valued inputs"""
    return -(np.asarray(x).astype(np.int64) @ np.asarray(c).astype(np.int64).T)


def assign(x, c, s=None):
    """(list int32 [n], score float32 [n]): the first minimum of every row"""
    return ivf_ref.assign(x, c, nip(x, c) if s is None else s)


def probe(q, c, nprobe, offsets, s=None):
    """ivf_ref.probe by (nip, list): (range_ptr, ranges, probes, probe_dist)"""
    return ivf_ref.probe(q, c, nprobe, offsets, nip(q, c) if s is None else s)


# ------------------------------------------------------------------------------ the tables
def tables(q, cent):
    """float32 [nq][m][K]: lut[q][i][c] = nip(q_i, cent[i][c]), cent [m][K][dsub]"""
    q = np.asarray(q, np.float32)
    m, k, dsub = cent.shape
    return np.stack([nip(q[:, i * dsub:(i + 1) * dsub], cent[i]) for i in range(m)], axis=1)


def tables_residual(q, c, probes, cent):
    """float32 [nq * nprobe][m][K]: the plain table of the query, part 0 with
    bias = nip(q, c[l]) added (one add); a list outside [0, nlist) (-1 is the padding) gives
    +inf"""
    q = np.asarray(q, np.float32)
    m, k, dsub = cent.shape
    nq, nprobe = probes.shape
    plain = tables(q[:, :m * dsub], cent)
    bias = nip(q[:, :m * dsub], c)
    lut = np.full((nq * nprobe, m, k), np.inf, np.float32)
    for o, l in enumerate(probes.reshape(-1)):
        if 0 <= l < c.shape[0]:
            lut[o] = plain[o // nprobe]
            lut[o, 0] = bias[o // nprobe, l] + plain[o // nprobe, 0]
    assert lut.dtype == np.float32
    return lut


# ------------------------------------------------------------------------------ the re-rank
def refine_dists(q, cent1, a, cent2, b, c=None):
    """float32 [rows]: nip(q, y), y = cent1[a] + cent2[b] (one add), then c + y where c
    (float32 [rows][d], the coarse centroid of every row's list) is given"""
    q = np.asarray(q, np.float32)
    y = refine_ref.reconstruct(cent1, a) + refine_ref.reconstruct(cent2, b)
    if c is not None:
        y = c + y
    assert y.dtype == np.float32
    acc = np.zeros(y.shape[0], np.float32)
    for j in range(y.shape[1]):
        acc = acc - q[j] * y[:, j]
    assert acc.dtype == np.float32
    return acc


def refine_int64(q, cent1, a, cent2, b, c=None):
    y = refine_ref.reconstruct(cent1, a).astype(np.int64) + refine_ref.reconstruct(cent2, b).astype(np.int64)
    if c is not None:
        y = y + np.asarray(c).astype(np.int64)
    return -(y @ np.asarray(q).astype(np.int64)[:y.shape[1]])


def refine(q, rows, top_k, cent1, codes1, cent2, codes2, coarse=None, offsets=None):
    """refine_ref.refine with refine_dists: (dist [nq][top_k], rows [nq][top_k])"""
    rows = np.asarray(rows, np.int64)
    n = codes1.shape[0]
    nq = rows.shape[0]
    wd = np.full((nq, top_k), np.inf, np.float32)
    wi = np.full((nq, top_k), -1, np.int64)
    for i in range(nq):
        r = rows[i][(rows[i] >= 0) & (rows[i] < n)]
        c = None if coarse is None else coarse[refine_ref.lists_of(offsets, r)]
        dist = refine_dists(q[i], cent1, codes1[r], cent2, codes2[r], c)
        order = np.lexsort((r, dist))[:top_k]
        wd[i, :len(order)] = dist[order]
        wi[i, :len(order)] = r[order]
    return wd, wi


# ------------------------------------------------------------------------------ the index
def pq_codes(x, cent):
    """the stream's codes are L2 assignments whatever the metric (ivf_residual_ref.pq_codes)"""
    return rref.pq_codes(x, cent)


def build(x, cc, cent, residual, metric="ip", cent2=None):
    """the index as numpy sees it: lists, perm, offsets, the stream's codes in list order (and
    the level-2 codes of what they leave over)"""
    x = np.asarray(x, np.float32)
    lists = assign(x, cc)[0] if metric == "ip" else ivf_ref.assign(x, cc)[0]
    perm, offsets = ivf_ref.layout(lists, cc.shape[0])
    rows = x[perm] - cc[lists[perm]] if residual else x[perm]
    assert rows.dtype == np.float32
    codes = pq_codes(rows, cent)
    w = dict(lists=lists, perm=perm, offsets=offsets, codes=codes, residual=residual,
             metric=metric, cc=cc, cent=cent, cent2=cent2, codes2=None)
    if cent2 is not None:
        left = rows - refine_ref.reconstruct(cent, codes)
        assert left.dtype == np.float32
        w["codes2"] = pq_codes(left, cent2)
    return w


def range_tables(w, q, nprobe):
    """(ptr, ranges, probes, one table per range) of the index w for the queries q"""
    if w["metric"] == "ip":
        ptr, ranges, probes, _ = probe(q, w["cc"], nprobe, w["offsets"])
        lut = (tables_residual(q, w["cc"], probes, w["cent"]) if w["residual"]
               else np.repeat(tables(q, w["cent"]), nprobe, axis=0))
    else:
        ptr, ranges, probes, _ = ivf_ref.probe(q, w["cc"], nprobe, w["offsets"])
        if w["residual"]:
            lut = rref.tables(q, w["cc"], probes, w["cent"])
        else:
            m, k, dsub = w["cent"].shape
            plain = np.stack([ivf_ref.dists(q[:, i * dsub:(i + 1) * dsub], w["cent"][i])
                              for i in range(m)], axis=1)
            lut = np.repeat(plain, nprobe, axis=0)
    return ptr, ranges, probes, lut


def _ids(w, rows):
    return np.where(rows >= 0, w["perm"][np.maximum(rows, 0)], -1)


def search(w, q, nprobe, k, keep=None, refine_k=0):
    """(dist, ids): the brute force over the probed lists -- every row of every probed list
    scored with its range's table, the k smallest by (dist, stream row), ids the caller's rows.
    keep: bool over the caller's rows.  refine_k: the k candidates re-ranked to refine_k."""
    ptr, ranges, _, lut = range_tables(w, q, nprobe)
    keep_rows = None if keep is None else np.asarray(keep, bool)[w["perm"]]
    dist, rows = rref.search(lut, w["codes"], k, ptr, ranges, keep=keep_rows)
    if refine_k:
        coarse = (w["cc"], w["offsets"]) if w["residual"] else (None, None)
        fn = refine if w["metric"] == "ip" else refine_ref.refine
        dist, rows = fn(q, rows, refine_k, w["cent"], w["codes"], w["cent2"], w["codes2"], *coarse)
    return dist, _ids(w, rows)


def range_search(w, q, nprobe, radius, keep=None):
    """(lims, dist, ids): range_ref.want_ranges over the same tables, ids the caller's rows"""
    ptr, ranges, _, lut = range_tables(w, q, nprobe)
    keep_rows = None if keep is None else np.asarray(keep, bool)[w["perm"]]
    lims, dist, rows = range_ref.want_ranges(lut, w["codes"], ptr, ranges,
                                             np.asarray(radius, np.float32), keep=keep_rows)
    return lims, dist, w["perm"][rows]


def exact_mips(x, q, k):
    """ids int64 [nq][k]: the exact maximum-inner-product rows in float64, ties to the smaller id"""
    s = -(np.asarray(q, np.float64) @ np.asarray(x, np.float64).T)
    ids = np.arange(x.shape[0])
    return np.stack([np.lexsort((ids, s[i]))[:k] for i in range(len(q))])


def recall(ids, truth):
    """the mean share of truth's ids found in ids, row by row"""
    return float(np.mean([len(set(a.tolist()) & set(b.tolist())) / len(b)
                          for a, b in zip(ids, truth)]))


def spread_world(n=4000, d=32, nlist=32, m=8, k=64, nq=40, seed=5):
    """rows whose norms are spread: datagen.sift_like rows, centred, each scaled by a fixed-seed
    log-normal factor.  Returns x, queries, a coarse codebook and a PQ trained on x."""
    import datagen
    rng = np.random.default_rng(seed)
    x = datagen.sift_like(n, d, seed=seed)
    x = ((x - x.mean(axis=0)) * rng.lognormal(0.0, 0.6, size=(n, 1))).astype(np.float32)
    q = ((datagen.sift_like(nq, d, seed=seed + 1) - datagen.sift_like(n, d, seed=seed).mean(axis=0))
         ).astype(np.float32)
    cc = datagen.lloyd_centroids(x, 1, nlist, iters=4, sample=n)[0]
    cent = datagen.lloyd_centroids(x, m, k, iters=4, sample=n)
    return x, q, cc, cent
