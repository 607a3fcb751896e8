"""The numpy reference of the inverted-file front end (coarse assignment, list layout, probe
selection), shared by tests/test_ivf_cpu.py and tests/test_gpu_ivf.py.  Nothing here calls the
library.

The distance is the definition of pqh_coarse_assign: a loop over j of float32 array operations,
acc = acc + (x_j - c_j) * (x_j - c_j).  numpy rounds each of the three operations to float32
and fuses nothing, so the bits are those of the direct form with j ascending.  Every order is
np.lexsort((ids, dist)): by distance, then by id."""
import numpy as np


def dists(x, c):
    """float32 [n][nlist]"""
    x = np.ascontiguousarray(x, np.float32)
    c = np.ascontiguousarray(c, np.float32)
    acc = np.zeros((x.shape[0], c.shape[0]), np.float32)
    for j in range(x.shape[1]):
        t = x[:, j:j + 1] - c[None, :, j]
        acc = acc + t * t
    assert acc.dtype == np.float32
    return acc


def assign(x, c, d=None):
    """(list int32 [n], dist float32 [n]): the first minimum of every row"""
    d = dists(x, c) if d is None else d
    lists = np.argmin(d, axis=1)          # (numpy returns the first of equal minima)
    return lists.astype(np.int32), d[np.arange(d.shape[0]), lists]


def layout(list_ids, nlist):
    """(perm int64 [n], offsets int64 [nlist + 1])"""
    list_ids = np.asarray(list_ids)
    perm = np.argsort(list_ids, kind="stable").astype(np.int64)
    offsets = np.zeros(nlist + 1, np.int64)
    offsets[1:] = np.cumsum(np.bincount(list_ids, minlength=nlist))
    return perm, offsets


def probe(q, c, nprobe, offsets, d=None):
    """(range_ptr [nq + 1], ranges [nq * nprobe][2], probes [nq][nprobe], dist [nq][nprobe]):
    the nprobe lists nearest to every query by (dist, list), padded with (-1, +inf, (0, 0));
    a reversed pair of offsets gives the range (0, 0)"""
    d = dists(q, c) if d is None else d
    nq, nlist = d.shape
    ids = np.arange(nlist, dtype=np.int64)
    probes = np.full((nq, nprobe), -1, np.int64)
    pdist = np.full((nq, nprobe), np.inf, np.float32)
    ranges = np.zeros((nq * nprobe, 2), np.int64)
    for i in range(nq):
        order = np.lexsort((ids, d[i]))[:nprobe]
        probes[i, :len(order)] = order
        pdist[i, :len(order)] = d[i, order]
        for p, l in enumerate(order):
            if offsets[l + 1] >= offsets[l]:
                ranges[i * nprobe + p] = offsets[l], offsets[l + 1] - offsets[l]
    return np.arange(nq + 1, dtype=np.int64) * nprobe, ranges, probes, pdist


def integer_grid(n, d, nlist, seed):
    """x and centroids with integer entries in [-8, 8]: every partial sum is an integer below
    2^24 (d * 16^2 <= 2^24 for d <= 65536), so float32 holds it exactly and many lists tie"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-8, 9, size=(n, d)).astype(np.float32)
    c = rng.integers(-8, 9, size=(nlist, d)).astype(np.float32)
    return x, c


def dists_int64(x, c):
    """the same distances in int64 arithmetic, for integer-valued inputs"""
    xi = np.asarray(x).astype(np.int64)
    ci = np.asarray(c).astype(np.int64)
    return ((xi[:, None, :] - ci[None, :, :]) ** 2).sum(axis=2)
