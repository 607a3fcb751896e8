"""The numpy restatement of the flat search (pqh_flat_search*, codec.Flat): the definition's
chains of every (query, row) pair and the k smallest by (dist, id), shared by
tests/test_flat_cpu.py and tests/test_gpu_flat.py."""
import numpy as np

import ivf_ref
import metric_ref


def topk(dist, k, keep=None, id_base=0):
    """(dist float32 [nq][k], ids int64 [nq][k]) of dist [nq][n]: per query the k smallest by
    (dist, id) among the kept rows, ids moved by id_base, padded with (+inf, -1)"""
    nq, n = dist.shape
    rows = np.arange(n, dtype=np.int64) if keep is None else np.flatnonzero(keep).astype(np.int64)
    wd = np.full((nq, k), np.inf, np.float32)
    wi = np.full((nq, k), -1, np.int64)
    for i in range(nq):
        order = np.lexsort((rows, dist[i, rows]))[:k]
        wd[i, :len(order)] = dist[i, rows[order]]
        wi[i, :len(order)] = rows[order] + id_base
    return wd, wi


def search(q, x, k, metric="l2", keep=None, id_base=0):
    with np.errstate(over="ignore", invalid="ignore"):
        dist = metric_ref.nip(q, x) if metric == "ip" else ivf_ref.dists(q, x)
    return topk(dist, k, keep, id_base)
