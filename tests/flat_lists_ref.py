"""The numpy restatement of pqh_flat_search_lists (codec.flat_search_lists): per query
flat_ref.topk over the definition's chains, the keep mask being (rows of the query's valid probed
lists) AND (the caller's keep).  Probes are distinct per query here.  Nothing calls the library."""
import numpy as np

import flat_ref
import ivf_ref
import metric_ref


def search(q, x_sorted, offsets, probes, k, metric="l2", keep=None, id_base=0):
    """(dist float32 [nq][k], rows int64 [nq][k]): rows of x_sorted + id_base"""
    n, nlist = len(x_sorted), len(offsets) - 1
    with np.errstate(over="ignore", invalid="ignore"):
        dist = metric_ref.nip(q, x_sorted) if metric == "ip" else ivf_ref.dists(q, x_sorted)
    wd = np.empty((len(q), k), np.float32)
    wi = np.empty((len(q), k), np.int64)
    for i, row in enumerate(probes):
        mask = np.zeros(n, bool) if keep is None else np.asarray(keep, bool).copy()
        inside = np.zeros(n, bool)
        for l in row:
            if 0 <= l < nlist and 0 <= offsets[l] <= offsets[l + 1] <= n:
                inside[offsets[l]:offsets[l + 1]] = True
        mask = inside if keep is None else mask & inside
        wd[i], wi[i] = (a[0] for a in flat_ref.topk(dist[i:i + 1], k, mask, id_base))
    return wd, wi
