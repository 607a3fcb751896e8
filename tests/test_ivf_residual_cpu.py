"""Host-side parts of the residual inverted file (pqh_ivf_residuals, pqh_adc_tables_residual,
pqh_search_stream_range_tables, pqh_search_codes_range_tables): the calls are exported,
declared and bound, a process that sees no GPU gets PQH_ERR_NO_DEVICE from each, and the numpy
reference (tests/ivf_residual_ref.py) shows what the feature is for: at the same code size the
residual form has the strictly lower quantization error."""
import os
import subprocess
import sys

import numpy as np
import pytest

import datagen
import ivf_ref
import ivf_residual_ref as ref
from conftest import ROOT
from pq_huffman_amd import capi, codec

NEW_CALLS = ["pqh_ivf_residuals", "pqh_adc_tables_residual", "pqh_search_stream_range_tables",
             "pqh_search_codes_range_tables"]


def test_residual_calls_are_exported_declared_and_bound():
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    header = open(os.path.join(ROOT, "include", "pqh.h")).read()
    bound = {name for name, _, _ in capi.SIGNATURES}
    for name in NEW_CALLS:
        assert name in exported and name in bound and f"int {name}(" in header, name
        assert getattr(capi.lib(), name).argtypes
    # the range-table calls take the arguments of the range calls
    sig = {name: args for name, _, args in capi.SIGNATURES}
    assert sig["pqh_search_stream_range_tables"] == sig["pqh_search_stream_ranges"]
    assert sig["pqh_search_codes_range_tables"] == sig["pqh_search_codes_ranges"]
    for name in ("adc_tables_residual", "search_range_tables", "search_codes_range_tables"):
        assert callable(getattr(codec, name))
    assert callable(codec.Coarse.residuals)
    import inspect
    assert inspect.signature(codec.IVF.build).parameters["residual"].default is False
    assert codec.IVF.table_budget == 256 << 20


PROBE = """
from pq_huffman_amd import capi
L = capi.lib()
print(L.pqh_ivf_residuals(None, None, None, 10, 8, None, None, None, 8),
      L.pqh_adc_tables_residual(None, None, None, None, 1, 8, None, 2, None),
      L.pqh_search_stream_range_tables(None, None, None, 0, 10, 1, 4, None, None, None, 1, None,
                                       None, 1, 10, 0, None, None),
      L.pqh_search_codes_range_tables(None, None, 10, 8, 256, None, 1, None, None, 1, 10, 0, None,
                                      None))
"""


def test_residual_calls_without_a_device():
    """the devices hidden: no context can exist, and every call says why before it looks at
    any other argument"""
    env = dict(os.environ)
    env["HIP_VISIBLE_DEVICES"] = ""
    env["ROCR_VISIBLE_DEVICES"] = ""
    r = subprocess.run([sys.executable, "-c", PROBE], capture_output=True, text=True, env=env,
                       cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["-2"] * 4, r.stdout + r.stderr


def test_null_context_is_no_device_or_arg():
    """in this process, whatever it sees: PQH_ERR_NO_DEVICE (-2) or PQH_ERR_ARG (-1)"""
    L = capi.lib()
    got = [L.pqh_ivf_residuals(None, None, None, 0, 0, None, None, None, 0),
           L.pqh_adc_tables_residual(None, None, None, None, 0, 0, None, 0, None),
           L.pqh_search_stream_range_tables(None, None, None, 0, 0, 1, 0, None, None, None, 0,
                                            None, None, 0, 0, 0, None, None),
           L.pqh_search_codes_range_tables(None, None, 0, 0, 0, None, 0, None, None, 0, 0, 0,
                                           None, None)]
    assert len(set(got)) == 1 and got[0] in (-1, -2), got


# n, d, lists, m, K: the table of the issue this feature answers
SHAPES = [(4000, 32, 16, 4, 16), (6000, 128, 37, 8, 256), (3000, 16, 7, 8, 16)]


@pytest.mark.parametrize("n,d,nlist,m,k", SHAPES)
def test_residual_form_has_the_lower_quantization_error(n, d, nlist, m, k):
    plain, resid = ref.plain_and_residual_error(datagen, n, d, nlist, m, k, seed=n + d)
    print(f"n={n} d={d} lists={nlist} m={m} K={k}: plain {plain:.1f} residual {resid:.1f}")
    assert resid < plain


def test_reference_pieces_agree_with_each_other():
    """the residual of the reference is x - c[list] in list order; a table is ivf_ref.dists of
    the residual query; the range search with every range given its query's table is the
    search of the concatenated ranges"""
    rng = np.random.default_rng(3)
    n, d, nlist, m, k = 200, 12, 5, 3, 16
    x = rng.normal(0.0, 10.0, size=(n, d)).astype(np.float32)
    c = rng.normal(0.0, 10.0, size=(nlist, d)).astype(np.float32)
    cent = rng.normal(0.0, 5.0, size=(m, k, d // m)).astype(np.float32)
    lists, _ = ivf_ref.assign(x, c)
    perm, offsets = ivf_ref.layout(lists, nlist)
    res, bad = ref.residuals(x, c, lists, perm)
    assert not bad.any()
    for s in (0, 17, n - 1):
        assert np.array_equal(res[s], x[perm[s]] - c[lists[perm[s]]])
    broken = perm.copy()
    broken[3] = n
    lists2 = lists.copy()
    lists2[perm[9]] = nlist
    res2, bad2 = ref.residuals(x, c, lists2, broken)
    assert np.flatnonzero(bad2).tolist() == [3, 9] and not res2[[3, 9]].any()
    keep = np.ones(n, bool)
    keep[[3, 9]] = False
    assert np.array_equal(res2[keep], res[keep])

    q = rng.normal(0.0, 10.0, size=(2, d)).astype(np.float32)
    probes = np.array([[1, -1, 4], [4, 4, 0]], np.int64)
    lut = ref.tables(q, c, probes, cent)
    assert lut.shape == (6, m, k) and np.isinf(lut[1]).all() and np.array_equal(lut[3], lut[4])
    r = (q[1] - c[0])[None]
    assert np.array_equal(lut[5, 2], ivf_ref.dists(r[:, 8:12], cent[2])[0])

    codes = ref.pq_codes(res, cent)
    ptr, ranges, _, _ = ivf_ref.probe(q, c, 3, offsets)
    own = np.repeat(rng.normal(0.0, 50.0, size=(2, m, k)).astype(np.float32), 3, axis=0)
    wd, wi = ref.search(own, codes, 10, ptr, ranges)
    for qi in range(2):
        rows = np.concatenate([np.arange(f, f + cnt) for f, cnt in ranges[3 * qi:3 * qi + 3]])
        dist = ref.adc(own[3 * qi], codes[rows])
        order = np.lexsort((rows, dist))[:10]
        assert np.array_equal(wi[qi, :len(order)], rows[order])
        assert np.array_equal(wd[qi, :len(order)], dist[order])
