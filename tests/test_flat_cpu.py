"""tests/flat_ref.py (the reference of tests/test_gpu_flat.py) against an int64 brute force on
the integer grid, where every fp32 chain is exact; and what the flat calls answer without a GPU."""
import numpy as np
import pytest

import flat_ref
import ivf_ref
import metric_ref
from pq_huffman_amd.capi import lib


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_ref_equals_int64_brute_force(metric):
    x, q = ivf_ref.integer_grid(300, 9, 17, 4)
    keep = np.random.default_rng(1).random(300) < 0.5
    exact = metric_ref.nip_int64(q, x) if metric == "ip" else ivf_ref.dists_int64(q, x)
    for kp in (None, keep):
        rows = np.arange(300) if kp is None else np.flatnonzero(kp)
        wd, wi = flat_ref.search(q, x, 200, metric, keep=kp, id_base=7)
        for i in range(17):
            order = sorted(rows, key=lambda v: (exact[i, v], v))[:200]
            assert wi[i, :len(order)].tolist() == [v + 7 for v in order]
            assert wd[i, :len(order)].tolist() == [float(exact[i, v]) for v in order]
            assert (wi[i, len(order):] == -1).all() and np.isinf(wd[i, len(order):]).all()


def test_null_context():
    L = lib()
    want = L.pqh_coarse_assign(None, None, None, 0, 1, None, None)
    assert want < 0
    assert L.pqh_flat_create(None, None, 0, 1, 1, None) == want
    assert L.pqh_flat_search(None, None, None, 0, 1, 1, None, 0, None, None) == want
    assert L.pqh_flat_search_ip(None, None, None, 0, 1, 1, None, 0, None, None) == want
    assert L.pqh_flat_last_counts(None, None, None) == want
    assert L.pqh_flat_destroy(None) == 0
