"""The inputs of the range-search tests have the properties their cases rely on, the numpy
reference does what the definition says, and the library declares, exports and binds the new
entry points (tests/range_ref.py; the GPU half is tests/test_gpu_range.py)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import range_ref as rref
import search_filter_ref as fref
import search_shapes_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("pqh_range_plan_bytes", "pqh_range_count_stream", "pqh_range_fill_stream",
         "pqh_range_count_codes", "pqh_range_fill_codes")


@pytest.mark.parametrize("mode", list(rref.MODES))
def test_radii(mode):
    d = sref.dists(rref.lut_of(mode), fref.codes_of(mode))
    rad = rref.radii(d)
    rref.check_radii(mode, d, rad)
    for kind in rad:
        rref.check_order(rref.want(d, rad[kind]))


def test_ties_at_the_radius():
    rref.check_ties(rref.ties_case()[2])


def test_masks_and_id_base():
    d = sref.dists(rref.lut_of("ctx_m8"), fref.codes_of("ctx_m8"))
    rad = rref.radii(d)["median"]
    free = rref.want(d, rad)
    keep = fref.random_mask(rref.N, 0.5, 11)
    half = rref.want(d, rad, keep)
    rref.check_order(half, keep)
    assert 0 < half[0][-1] < free[0][-1]
    ones = rref.want(d, rad, np.ones(rref.N, bool))
    assert all(np.array_equal(a, b) for a, b in zip(free, ones))
    assert rref.want(d, rad, np.zeros(rref.N, bool))[0][-1] == 0
    moved = rref.want(d, rad, keep, id_base=10 ** 12)
    assert np.array_equal(moved[2] - 10 ** 12, half[2]) and np.array_equal(moved[0], half[0])
    for chunk in rref.CHUNKS:
        fref.check_chunk_ends(chunk)
    w = rref.prefix(free, int(free[0][3]))
    assert len(w[1]) == free[0][3] and np.array_equal(w[0], free[0])


@pytest.mark.parametrize("m,K", fref.PROBE_SHAPES)
@pytest.mark.parametrize("chunk", fref.PROBE_CHUNKS)
def test_probe_cases(m, K, chunk):
    case, ptr, ranges = rref.probe_case(m, K, chunk)
    rref.check_probe_case(case, ptr, ranges)
    # a bad range is skipped, and only its query's result changes
    codes = case[0]
    lut = rref.probe_luts(case)[0]
    inf = np.full(len(ptr) - 1, np.inf, np.float32)
    good = rref.want_ranges(lut, codes, ptr, ranges, inf)
    bad = rref.want_ranges(lut, codes, ptr, rref.bad_ranges(ranges, ptr, len(codes)), inf)
    diff = rref.counts(good) != rref.counts(bad)
    assert diff[rref.BAD_Q] and diff.sum() == 1


def test_the_reference_agrees_with_the_top_k_reference():
    """the hits below the k-th distance are the head of ivf_residual_ref.search"""
    w = fref.ivf_world()
    rref.check_ivf(w)
    for kind in ("plain", "residual"):
        rad = rref.ivf_radii(w, kind)
        top = fref.ivf_want(w, kind, 64)
        heads = rref.topk_of(rref.ivf_want(w, kind, rad), rref.inverse(w["perm"]))
        for q, (d, ids) in enumerate(heads):
            below = top[0][q] < rad[q]
            assert np.array_equal(top[1][q][below], ids) and np.array_equal(top[0][q][below], d)


def test_the_calls_are_declared_exported_and_bound():
    from pq_huffman_amd import capi
    header = open(os.path.join(ROOT, "include", "pqh.h")).read()
    bound = {name: args for name, _, args in capi.SIGNATURES}
    lib = capi.lib()
    for name in CALLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in bound and hasattr(lib, name), name
    # the fill takes the count's arguments, then capacity, id_base, dist and ids
    tail = [capi.LL, capi.LL, capi.P, capi.P]
    for src in ("stream", "codes"):
        assert bound[f"pqh_range_fill_{src}"] == bound[f"pqh_range_count_{src}"] + tail
    # the count's are the top-k call's up to nr, without top_k, id_base and the outputs
    assert bound["pqh_range_count_stream"][:14] == bound["pqh_search_stream_ranges"][:14]
    assert bound["pqh_range_count_codes"][:10] == bound["pqh_search_codes_ranges"][:10]


def test_the_python_layer():
    from pq_huffman_amd import codec
    for name in ("range_search", "range_search_codes", "range_search_ranges",
                 "range_search_codes_ranges"):
        p = inspect.signature(getattr(codec, name)).parameters
        assert p["keep"].default is None and p["id_base"].default == 0, name
        assert p["capacity"].default is None and "radius" in p, name
    assert inspect.signature(codec.range_search_ranges).parameters["tables_per_range"].default is False
    p = inspect.signature(codec.IVF.range_search).parameters
    assert list(p) == ["self", "queries", "nprobe", "radius", "keep"] and p["keep"].default is None


def test_a_null_context_is_refused_before_anything_else():
    """as the searches (PQH_ERR_ARG or PQH_ERR_NO_DEVICE): no GPU is needed to be told"""
    from pq_huffman_amd import capi
    lib = capi.lib()
    nbytes = ctypes.c_ulonglong(0)
    assert lib.pqh_range_plan_bytes(None, 1000, 8, 256, 64, 9, -1, 0, ctypes.byref(nbytes)) in (-1, -2)
    got = lib.pqh_range_count_codes(None, None, 0, 8, 256, None, 0, None, None, -1, 0, None, None,
                                    None, 0, None)
    assert got in (-1, -2)
    got = lib.pqh_range_fill_codes(None, None, 0, 8, 256, None, 0, None, None, -1, 0, None, None,
                                   None, 0, None, 0, 0, None, None)
    assert got in (-1, -2)
    got = lib.pqh_range_count_stream(None, None, None, 0, 0, 1, 64, None, None, None, 0, None, None,
                                     -1, 0, None, None, None, 0, None)
    assert got in (-1, -2)
    got = lib.pqh_range_fill_stream(None, None, None, 0, 0, 1, 64, None, None, None, 0, None, None,
                                    -1, 0, None, None, None, 0, None, 0, 0, None, None)
    assert got in (-1, -2)
