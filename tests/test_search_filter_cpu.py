"""The inputs of the filtered-search tests have the properties their cases rely on, the numpy
reference does what a filter has to, and the library declares, exports and binds the new
entry points (tests/search_filter_ref.py; the GPU half is tests/test_gpu_search_filter.py)."""
import inspect
import os
import re

import numpy as np
import pytest

import search_filter_ref as fref
import search_shapes_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEARCHES = ("pqh_search_stream", "pqh_search_codes", "pqh_search_stream_ranges",
            "pqh_search_codes_ranges", "pqh_search_stream_range_tables",
            "pqh_search_codes_range_tables", "pqh_search_stream_lists", "pqh_search_codes_lists")


def test_pack_is_little_endian_bit_order():
    fref.check_pack()


@pytest.mark.parametrize("mode", list(fref.MODES))
def test_plain_masks(mode):
    codes = fref.codes_of(mode)
    lut = fref.lut_of(fref.NQ, codes.shape[1], 7)
    d = sref.dists(lut, codes)
    for chunk in fref.CHUNKS:
        fref.check_plain_masks(chunk, lut, codes, fref.plain_masks(chunk, lut, codes, d), d)


def test_ties_are_decided_by_the_ids():
    codes = fref.codes_of("ctx_m8")
    fref.check_ties(fref.ties_lut(fref.NQ, 8, 9), codes, fref.random_mask(fref.N, 0.5, 11))


def test_a_filter_after_the_selection_is_wrong():
    """the reason the mask is inside the scan: dropping rows from the unfiltered top 64 leaves
    nothing where the definition has 64 rows"""
    codes = fref.codes_of("noctx_m3")
    lut = fref.lut_of(fref.NQ, 3, 7)
    keep = fref.complement_of_top(lut, codes)
    fref.check_not_top(lut, codes, keep)
    top = sref.want(lut, codes, 64)[1]
    assert not keep[top].any()


@pytest.mark.parametrize("m,K", fref.PROBE_SHAPES)
@pytest.mark.parametrize("chunk", fref.PROBE_CHUNKS)
def test_probe_masks(m, K, chunk):
    case = sref.sweep_case(m, K, chunk, seed=40 + m + chunk)
    if chunk == 7:
        sref.check_sweep_case(m, K, chunk, case)
    fref.check_probe_masks(chunk, case, fref.probe_masks(case))
    assert {sref.qb_of(m, K) for m, K in fref.PROBE_SHAPES} == {8, 4}


def test_pack_cases():
    for n in fref.PACK_NS:
        for permuted in (False, True):
            keep, perm, words = fref.pack_case(n, n + 1, permuted)
            assert words.dtype == np.int32 and len(words) == (n + 31) // 32
            if n > 1:
                assert (keep > 1).any() or n < 4          # nonzero, not one: still kept
            if permuted and n > 1:
                assert sorted(perm) == list(range(n))
    keep, perm, words = fref.bad_perm_case()
    assert (perm == -1).sum() == 1 and (perm == len(keep)).sum() == 1
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:len(keep)]
    assert bits.sum() == len(keep) - 2 and not bits[40] and not bits[len(keep) - 2]


def test_ivf_world():
    fref.check_ivf_world(fref.ivf_world())


def test_the_masked_calls_are_declared_exported_and_bound():
    from pq_huffman_amd import capi
    header = open(os.path.join(ROOT, "include", "pqh.h")).read()
    bound = {name: args for name, _, args in capi.SIGNATURES}
    for name in SEARCHES:
        assert re.search(r"\b%s_masked\(" % name, header), name
        # the unfiltered call's arguments and the mask words behind them
        assert bound[name + "_masked"] == bound[name] + [capi.P], name
    assert re.search(r"\bpqh_mask_pack\(", header) and len(bound["pqh_mask_pack"]) == 5
    lib = capi.lib()
    for name in [s + "_masked" for s in SEARCHES] + ["pqh_mask_pack"]:
        assert hasattr(lib, name), name


def test_the_python_layer_takes_keep():
    from pq_huffman_amd import codec
    for name in ("search", "search_codes", "search_ranges", "search_codes_ranges",
                 "search_range_tables", "search_codes_range_tables", "search_lists",
                 "search_codes_lists"):
        p = inspect.signature(getattr(codec, name)).parameters
        assert "keep" in p and p["keep"].default is None, name
    p = inspect.signature(codec.IVF.search).parameters
    assert p["keep"].default is None
    assert list(inspect.signature(codec.pack_mask).parameters) == ["ctx", "keep", "perm", "out"]
    assert callable(codec.IVF.remove) and callable(codec.IVF.live_count)


def test_a_null_context_is_refused_before_anything_else():
    """as the unfiltered calls (PQH_ERR_ARG or PQH_ERR_NO_DEVICE): no GPU is needed to be told"""
    from pq_huffman_amd import capi
    lib = capi.lib()
    assert lib.pqh_mask_pack(None, None, None, 0, None) in (-1, -2)
    got = lib.pqh_search_codes_masked(None, None, 0, 8, 256, None, 0, 1, 0, None, None, None)
    assert got in (-1, -2)
