"""The numpy restatement of the exact re-rank (pqh_rerank_rows, pqh_rerank_sq, codec.rerank): per
query the definition's chains (ivf_ref.dists, metric_ref.nip) of its valid candidates against
their stored rows, the k smallest by (dist, id).  Nothing calls the library."""
import numpy as np

import ivf_ref
import metric_ref
import sq_ref


def rerank(q, x, cand, k, metric="l2", sq=None):
    """(dist float32 [nq][k], ids int64 [nq][k], the set of bad ids).  x: the stored rows as
    float32 values [n][d], or with sq = (vmin, step) the uint8 codes; cand int64 [nq][ncand],
    -1 = padding, an id below -1 or >= n dropped and returned among the bad ones; an id named
    twice is scored twice; padded with (+inf, -1)"""
    q, cand = np.asarray(q, np.float32), np.asarray(cand, np.int64)
    n = x.shape[0]
    wd = np.full((len(q), k), np.inf, np.float32)
    wi = np.full((len(q), k), -1, np.int64)
    bad = set(cand[(cand < -1) | (cand >= n)].tolist())
    for i in range(len(q)):
        ids = cand[i][(cand[i] >= 0) & (cand[i] < n)]
        if not len(ids):
            continue
        rows = x[ids] if sq is None else sq_ref.decode(x[ids], *sq)
        with np.errstate(over="ignore", invalid="ignore"):
            dist = (metric_ref.nip if metric == "ip" else ivf_ref.dists)(q[i:i + 1], rows)[0]
        order = np.lexsort((ids, dist))[:k]
        wd[i, :len(order)], wi[i, :len(order)] = dist[order], ids[order]
    return wd, wi, bad
