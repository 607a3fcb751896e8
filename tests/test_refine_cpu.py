"""The refinement codes without a GPU: the numpy reference (tests/refine_ref.py) against exact
integer arithmetic and on its edge cases, what the refinement is worth on the nine-query world
of the filtered search's tests, and the interface -- the C entry points declared, exported and
bound, their NULL-context rule, the new arguments of codec.IVF."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import ivf_ref
import refine_ref as rr
import search_filter_ref as fref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


# ------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("residual", [False, True])
def test_reference_is_exact_on_the_integer_grid(residual):
    """integer codebooks, queries and coarse centroids: every fp32 operation is exact, so the
    distances are those of int64 arithmetic"""
    rng = np.random.default_rng(3)
    (m1, ds1), (m2, ds2), k, n, nlist = (3, 5), (5, 3), 16, 300, 7
    cent1 = rng.integers(-3, 4, size=(m1, k, ds1)).astype(np.float32)
    cent2 = rng.integers(-3, 4, size=(m2, k, ds2)).astype(np.float32)
    a = rng.integers(0, k, size=(n, m1)).astype(np.uint8)
    b = rng.integers(0, k, size=(n, m2)).astype(np.uint8)
    q, cc = ivf_ref.integer_grid(6, 15, nlist, 4)
    offsets = np.array([0, 0, 50, 50, 50, 120, 300, 300], np.int64)
    rows = rng.integers(0, n, size=(6, 40)).astype(np.int64)
    wd, wi = rr.refine(q, rows, 40, cent1, a, cent2, b, cc if residual else None,
                       offsets if residual else None)
    for i in range(6):
        c = cc[rr.lists_of(offsets, rows[i])] if residual else None
        exact = rr.dists_int64(q[i], cent1, a[rows[i]], cent2, b[rows[i]], c)
        order = np.lexsort((rows[i], exact))
        assert np.array_equal(wi[i], rows[i][order])
        assert np.array_equal(wd[i].astype(np.int64), exact[order]) and (wd[i] == np.floor(wd[i])).all()


def test_reference_decides_ties_by_the_row():
    w = rr.ties_world()
    wd, wi = rr.refine(w["q"], w["rows"], 64, w["cent1"], w["codes1"], w["cent2"], w["codes2"])
    for i in range(4):
        assert (wi[i] >= 0).all()
        # a row and its copy 200 further on are neighbours in the result, the smaller one first
        pos = {int(r): p for p, r in enumerate(wi[i])}
        low = [r for r in pos if r < 200]
        assert len(low) == 32
        for r in low:
            assert wd[i][pos[r]] == wd[i][pos[r + 200]] and pos[r] < pos[r + 200]
        same = np.diff(wd[i]) == 0
        assert same.sum() >= 32 and (np.diff(wi[i])[same] > 0).all()
    # a row given twice appears twice
    twice = np.array([[5, 9, 5, -1]], np.int64)
    wd, wi = rr.refine(w["q"][:1], twice, 4, w["cent1"], w["codes1"], w["cent2"], w["codes2"])
    assert sorted(wi[0].tolist()) == [-1, 5, 5, 9] and wi[0][3] == -1 and np.isinf(wd[0][3])


def test_reference_padding_and_rows_outside():
    w = rr.ties_world()
    args = (w["cent1"], w["codes1"], w["cent2"], w["codes2"])
    plain = rr.refine(w["q"][:1], np.array([[7, 3, 11]], np.int64), 3, *args)
    for rows in ([-1, 7, 3, 11], [7, -1, 3, -1, 11], [7, 3, 11, -1, -1], [400, 7, 3, -5, 11, 2 ** 40]):
        wd, wi = rr.refine(w["q"][:1], np.array([rows], np.int64), len(rows), *args)
        assert np.array_equal(wi[0][:3], plain[1][0]) and np.array_equal(_bits(wd[0][:3]), _bits(plain[0][0]))
        assert (wi[0][3:] == -1).all() and np.isposinf(wd[0][3:]).all()
    wd, wi = rr.refine(w["q"][:2], np.array([[-1, -1, -1], [7, 3, 11]], np.int64), 2, *args)
    assert (wi[0] == -1).all() and np.isposinf(wd[0]).all()
    own = rr.refine(w["q"][1:2], np.array([[7, 3, 11]], np.int64), 2, *args)
    assert np.array_equal(wi[1], own[1][0]) and np.array_equal(_bits(wd[1]), _bits(own[0][0]))


def test_reference_list_rule_passes_over_empty_lists():
    offsets = np.array([0, 0, 0, 4, 4, 9, 9], np.int64)       # lists 0, 1, 3 and 5 are empty
    assert rr.lists_of(offsets, np.arange(9)).tolist() == [2] * 4 + [4] * 5
    # the rule of IVF.fetch, and the distance uses that list's centroid
    rng = np.random.default_rng(8)
    cc = rng.normal(size=(6, 4)).astype(np.float32)
    cent = rng.normal(size=(2, 4, 2)).astype(np.float32)
    codes = rng.integers(0, 4, size=(9, 2)).astype(np.uint8)
    q = rng.normal(size=(1, 4)).astype(np.float32)
    wd, wi = rr.refine(q, np.arange(9)[None], 9, cent, codes, cent, codes, cc, offsets)
    for dist, r in zip(wd[0], wi[0]):
        y = rr.reconstruct(cent, codes[r:r + 1])[0]
        t = (q[0] - cc[2 if r < 4 else 4]) - (y + y)
        acc = np.float32(0)
        for j in range(4):
            acc = acc + t[j] * t[j]
        assert _bits(np.float32(dist)) == _bits(np.float32(acc))


# ------------------------------------------------------------------------------ what it is worth
@pytest.fixture(scope="module")
def world():
    return fref.ivf_world()


@pytest.mark.parametrize("kind", ["plain", "residual"])
def test_refinement_improves_the_top_ten(world, kind):
    """per query the overlap of the top 10 with the exact top 10 among the 64 candidates: the
    refined one is never worse than the ADC one, better in sum, and differs for every query"""
    w = world
    r2 = rr.ivf_refine_world(w, kind)
    _, cand = rr.ivf_candidates(w, kind, 64)
    assert (cand >= 0).all()
    _, fine = rr.ivf_refined(w, kind, r2, cand, 10)
    adc_sum = fine_sum = 0
    for i in range(fref.IVF_NQ):
        exact = ivf_ref.dists(w["q"][i:i + 1], w["x"][w["perm"][cand[i]]])[0]
        best = set(cand[i][np.lexsort((cand[i], exact))[:10]].tolist())
        adc, got = len(best & set(cand[i][:10].tolist())), len(best & set(fine[i].tolist()))
        assert got >= adc, (kind, i, adc, got)
        assert not np.array_equal(fine[i], cand[i][:10]), (kind, i)   # (as ordered lists)
        adc_sum += adc
        fine_sum += got
    print(f"{kind}: overlap with the exact top 10 among 64 candidates {adc_sum} -> {fine_sum} of 90")
    assert fine_sum > adc_sum
    # the second code shrinks what is left over
    err1 = (r2["left"].astype(np.float64) ** 2).sum(axis=1).mean()
    left2 = r2["left"] - rr.reconstruct(r2["cent2"], r2["codes2"])
    assert (left2.astype(np.float64) ** 2).sum(axis=1).mean() < 0.5 * err1


# ------------------------------------------------------------------------------ the interface
def test_entry_points_are_declared_exported_and_bound():
    from pq_huffman_amd import capi
    header = open(os.path.join(ROOT, "include", "pqh.h")).read()
    bound = {name: args for name, _, args in capi.SIGNATURES}
    for name in ("pqh_refine_stream", "pqh_refine_codes"):
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert decl, name
        assert len(bound[name]) == decl.group(1).count(",") + 1, name
        assert hasattr(capi.lib(), name)
    # per level the stream and index arguments of pqh_fetch_vectors but n, which both share
    fetch = len(bound["pqh_fetch_vectors"])
    assert len(bound["pqh_refine_stream"]) == 1 + 2 * (fetch - 1 - 5) + 12


def test_null_context_is_refused_first():
    from pq_huffman_amd import capi
    lib = capi.lib()
    n = ctypes.c_int(0)
    lib.pqh_device_count(ctypes.byref(n))
    want = -1 if n.value > 0 else -2
    z = [None, None, None, 0, 0, 0, None, None]
    assert lib.pqh_refine_stream(None, *z, *z, -5, None, None, None, -1, 0, None, 0, 0, None, None,
                                 0) == want
    assert lib.pqh_refine_codes(None, None, None, None, None, -5, None, None, None, -1, 0, None, 0,
                                0, None, None, 0) == want


def test_codec_has_the_new_arguments():
    from pq_huffman_amd import codec
    p = inspect.signature(codec.IVF.build).parameters
    assert p["refine_pq"].default is None and p["refine_chunk_vectors"].default is None
    assert inspect.signature(codec.IVF.search).parameters["refine"].default == 0
    assert inspect.signature(codec.IVF.fetch).parameters["refined"].default is False
    assert list(inspect.signature(codec.refine).parameters) == [
        "ctx", "level1", "level2", "queries", "rows", "k", "coarse", "offsets", "out"]
    assert list(inspect.signature(codec.pq_residuals).parameters) == ["ctx", "pq", "x", "codes"]
