"""The numpy reference of the residual inverted file (pqh_ivf_residuals,
pqh_adc_tables_residual, pqh_search_*_range_tables, codec.IVF with residual=True), shared by
tests/test_ivf_residual_cpu.py and tests/test_gpu_ivf_residual.py.  Nothing here calls the
library.

Every value is a float32 array operation of numpy, which rounds each operation to float32 and
fuses nothing: the residual is one subtract, a table entry is ivf_ref.dists' sum
(acc = acc + t * t, j ascending) over the residual, a distance is the parts' entries added left
to right, and every order is np.lexsort((ids, dist))."""
import numpy as np

import ivf_ref


def residuals(x, c, lists, perm=None):
    """float32 [n][d]: row s = x[p] - c[lists[p]], p = perm[s] (None: s).  A perm entry
    outside [0, n) or a list id outside [0, nlist) gives a row of zeros; bad[s] says so."""
    x = np.asarray(x, np.float32)
    c = np.asarray(c, np.float32)
    n = x.shape[0]
    p = np.arange(n, dtype=np.int64) if perm is None else np.asarray(perm, np.int64)
    ok = (p >= 0) & (p < n)
    l = np.where(ok, np.asarray(lists, np.int64)[np.where(ok, p, 0)] if n else 0, -1)
    ok &= (l >= 0) & (l < c.shape[0])
    out = np.zeros((n, x.shape[1]), np.float32)
    out[ok] = x[p[ok]] - c[l[ok]]
    assert out.dtype == np.float32
    return out, ~ok


def tables(q, c, probes, cent):
    """float32 [nq * nprobe][m][K]: the table of q - c[probes[q][p]] against the PQ centroids
    cent [m][K][dsub]; a list outside [0, nlist) (-1 is the padding) gives +inf"""
    q = np.asarray(q, np.float32)
    m, k, dsub = cent.shape
    nq, nprobe = probes.shape
    lut = np.full((nq * nprobe, m, k), np.inf, np.float32)
    for o, l in enumerate(probes.reshape(-1)):
        if 0 <= l < c.shape[0]:
            r = (q[o // nprobe, :m * dsub] - c[l])[None]
            assert r.dtype == np.float32
            for i in range(m):
                lut[o, i] = ivf_ref.dists(r[:, i * dsub:(i + 1) * dsub], cent[i])[0]
    return lut


def adc(table, codes):
    """float32 [rows]: the parts' entries of one table added left to right"""
    dist = table[0, codes[:, 0]]
    for i in range(1, codes.shape[1]):
        dist = dist + table[i, codes[:, i]]
    assert dist.dtype == np.float32
    return dist


def search(lut, codes, k, ptr, ranges, id_base=0, keep=None):
    """(dist float32 [nq][k], ids int64 [nq][k]): query q scores the rows of its ranges
    r in [ptr[q], ptr[q + 1]) with table lut[r], a row once per range that holds it; the k
    smallest by (dist, row), padded with (+inf, -1).  A range that leaves [0, n] is skipped, a
    query whose ptr pair is reversed or leaves [0, nr] has no ranges; keep: a row -> bool mask
    of the rows that take part at all."""
    n = codes.shape[0]
    nq, nr = len(ptr) - 1, len(ranges)
    wd = np.full((nq, k), np.inf, np.float32)
    wi = np.full((nq, k), -1, np.int64)
    for q in range(nq):
        if not 0 <= ptr[q] <= ptr[q + 1] <= nr:
            continue
        rows, dist = [np.zeros(0, np.int64)], [np.zeros(0, np.float32)]
        for r in range(ptr[q], ptr[q + 1]):
            f, c = int(ranges[r][0]), int(ranges[r][1])
            if not (0 <= f <= n and 0 <= c <= n - f):
                continue
            rr = np.arange(f, f + c, dtype=np.int64)
            if keep is not None:
                rr = rr[keep[rr]]
            rows.append(rr)
            dist.append(adc(lut[r], codes[rr]))
        rows, dist = np.concatenate(rows), np.concatenate(dist)
        order = np.lexsort((rows, dist))[:k]
        wd[q, :len(order)] = dist[order]
        wi[q, :len(order)] = rows[order] + id_base
    return wd, wi


def pq_codes(x, cent):
    """uint8 [n][m]: the nearest centroid of every part, the first minimum of ivf_ref.dists"""
    m, k, dsub = cent.shape
    return np.stack([np.argmin(ivf_ref.dists(x[:, i * dsub:(i + 1) * dsub], cent[i]), axis=1)
                     for i in range(m)], axis=1).astype(np.uint8)


def quantization_error(x, cent):
    """mean over the rows of ||x - its reconstruction||^2 in float64"""
    m, k, dsub = cent.shape
    codes = pq_codes(x, cent)
    rec = np.concatenate([cent[i][codes[:, i]] for i in range(m)], axis=1)
    return float(((x.astype(np.float64) - rec.astype(np.float64)) ** 2).sum(axis=1).mean())


def plain_and_residual_error(datagen, n, d, nlist, m, k, seed):
    """(plain, residual): the quantization error of an m x k PQ trained on x, and of one
    trained on x - c[list] for a Lloyd coarse codebook of nlist centroids -- at the same code
    size, on datagen.sift_like rows"""
    x = datagen.sift_like(n, d, seed=seed)
    coarse = datagen.lloyd_centroids(x, 1, nlist, iters=4, sample=n)[0]
    lists, _ = ivf_ref.assign(x, coarse)
    res, bad = residuals(x, coarse, lists)
    assert not bad.any()
    plain = quantization_error(x, datagen.lloyd_centroids(x, m, k, iters=4, sample=n))
    resid = quantization_error(res, datagen.lloyd_centroids(res, m, k, iters=4, sample=n))
    return plain, resid
