"""Host-side parts of the list-major probe search (pqh_search_stream_lists,
pqh_search_codes_lists): the numpy restatement of the schedule (tests/search_lists_ref.py)
gives what the probe search is defined to give (tests/ivf_residual_ref.py on probe_ranges), the
calls are exported, declared and bound, and a process that sees no GPU gets PQH_ERR_NO_DEVICE
from each before any other argument is looked at."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

import ivf_residual_ref as ref
import search_lists_ref as lref
from conftest import ROOT
from pq_huffman_amd import capi, codec

NEW_CALLS = ["pqh_search_stream_lists", "pqh_search_codes_lists"]


def _bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


@pytest.mark.parametrize("m,chunk", [(8, 7), (16, 1), (3, 64)])
def test_the_schedule_restated_gives_the_probe_search(m, chunk):
    """both table forms, k in {1, 10, 64}: ids and float bits of the range search of
    probe_ranges(offsets, probes); the inputs have the properties the GPU sweep relies on"""
    codes, offsets, probes, lut_q, lut_pair = lref.sweep_case(m, chunk, 100 * m + chunk)
    n_units = lref.check_sweep_inputs(chunk, offsets, probes, m)
    ptr, ranges = lref.probe_ranges(offsets, probes)
    assert np.isnan(lut_pair[ranges[:, 1] == 0]).all() and not np.isnan(lut_q).any()
    for lut, per_range in ((lut_q, np.repeat(lut_q, lref.NPROBE, axis=0)), (lut_pair, lut_pair)):
        for k in (1, 10, 64):
            wd, wi = ref.search(per_range, codes, k, ptr, ranges)
            gd, gi, units = lref.search(lut, codes, k, offsets, probes)
            assert units == n_units
            assert np.array_equal(gi, wi) and np.array_equal(_bits(gd), _bits(wd)), (m, chunk, k)
            assert not np.isnan(wd).any()
        assert (wi[5] == -1).all() and (wi[3] == -1).all() and (wi[2] >= 0).sum() == 1
        # the list probed twice offers its rows twice
        ids, times = np.unique(wi[4], return_counts=True)
        assert (times[ids >= 0] <= 2).all() and ((times == 2).any() or lut is lut_pair)
        # the shared integer table: equal distances across lists, in stream-row order
        d6, i6 = wd[6], wi[6]
        tie = np.flatnonzero(d6[1:] == d6[:-1])
        assert len(tie) > 8 and (i6[tie + 1] > i6[tie]).all()
        lists6 = np.searchsorted(offsets[1:], i6, side="right")
        assert (lists6[tie + 1] != lists6[tie]).any()
        # tables rolled by one pair (or query) change the result: a stale table would show
        rolled = np.nan_to_num(np.roll(lut, 1, axis=0), nan=1e9)
        sd, si, _ = lref.search(rolled, codes, 64, offsets, probes)
        assert not np.array_equal(si[0], wi[0]) and not np.array_equal(si[4], wi[4])
    # id_base, and a mask of rows that take no part
    keep = np.arange(codes.shape[0]) % 3 != 0
    wd, wi = ref.search(lut_pair, codes, 10, ptr, ranges, id_base=1000, keep=keep)
    gd, gi, _ = lref.search(lut_pair, codes, 10, offsets, probes, id_base=1000, keep=keep)
    assert np.array_equal(gi, wi) and np.array_equal(_bits(gd), _bits(wd))


def test_bad_probes_and_bad_offsets_have_no_pairs():
    offsets = np.array([0, 5, 5, 9, 7, 12], np.int64)         # list 3 reversed, list 1 empty
    probes = np.array([[0, 5, -2], [3, 1, 4], [-1, 2, 0]], np.int64)
    pairs, bad = lref.invert(offsets, probes, 12)
    assert bad and pairs == [[0, 8], [], [7], [], [5]]
    assert not lref.invert(offsets, np.array([[0, -1, 2]], np.int64), 12)[1]
    assert lref.units(pairs, 1) == [(0, [0]), (0, [8]), (2, [7]), (4, [5])]
    assert lref.units([list(range(17)), [], [3]], 8) == [(0, list(range(8))), (0, list(range(8, 16))),
                                                         (0, [16]), (2, [3])]


def test_list_calls_are_exported_declared_and_bound():
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    header = open(os.path.join(ROOT, "include", "pqh.h")).read()
    bound = {name for name, _, _ in capi.SIGNATURES}
    for name in NEW_CALLS:
        assert name in exported and name in bound and f"int {name}(" in header, name
        assert getattr(capi.lib(), name).argtypes
    sig = {name: args for name, _, args in capi.SIGNATURES}
    # the stream and index arguments of the range call, then offsets, nlist, probes, nq, nprobe,
    # lut, tables_per_probe and the range call's tail
    rng = sig["pqh_search_stream_ranges"]
    P, LL, I = rng[0], rng[4], rng[5]
    assert sig["pqh_search_stream_lists"] == rng[:9] + [P, LL, P, LL, I, P, I] + rng[14:]
    crng = sig["pqh_search_codes_ranges"]
    assert sig["pqh_search_codes_lists"] == crng[:5] + [P, LL, P, LL, I, P, I] + crng[10:]
    for name in ("search_lists", "search_codes_lists"):
        assert callable(getattr(codec, name))
    assert inspect.signature(codec.IVF.search).parameters["schedule"].default == "query"
    assert float(codec.IVF.list_major_ratio) > 0


PROBE = """
from pq_huffman_amd import capi
L = capi.lib()
print(L.pqh_search_stream_lists(None, None, None, 0, 10, 1, 4, None, None, None, 3, None, 1, 2,
                                None, 0, 10, 0, None, None),
      L.pqh_search_codes_lists(None, None, 10, 8, 256, None, 3, None, 1, 2, None, 1, 10, 0, None,
                               None),
      # arguments that are bad in themselves (no list, no probe, top_k = 0): the context first
      L.pqh_search_stream_lists(None, None, None, 0, 10, 1, 0, None, None, None, 0, None, 1, 0,
                                None, 0, 0, 0, None, None),
      L.pqh_search_codes_lists(None, None, -1, 0, 0, None, 0, None, 1, 0, None, 1, 0, 0, None,
                               None))
"""


def test_list_calls_without_a_device():
    """the devices hidden: no context can exist, and every call says why before it looks at
    any other argument, good or bad -- the family's order of checks"""
    env = dict(os.environ)
    env["HIP_VISIBLE_DEVICES"] = ""
    env["ROCR_VISIBLE_DEVICES"] = ""
    r = subprocess.run([sys.executable, "-c", PROBE], capture_output=True, text=True, env=env,
                       cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["-2"] * 4, r.stdout + r.stderr


def test_null_context_is_no_device_or_arg():
    """in this process, whatever it sees: PQH_ERR_NO_DEVICE (-2) or PQH_ERR_ARG (-1), the same
    for good and for bad arguments"""
    L = capi.lib()
    got = [L.pqh_search_stream_lists(None, None, None, 0, 0, 1, 0, None, None, None, 0, None, 0, 0,
                                     None, 0, 0, 0, None, None),
           L.pqh_search_codes_lists(None, None, 0, 0, 0, None, 0, None, 0, 0, None, 0, 0, 0, None,
                                    None),
           L.pqh_search_codes_lists(None, None, 10, 8, 256, None, 3, None, 1, 2, None, 1, 10, 0,
                                    None, None)]
    assert len(set(got)) == 1 and got[0] in (-1, -2), got


def test_the_table_form_is_taken_from_the_tables():
    """nq tables: shared; nq * nprobe: one per pair; anything else raises before the library is
    called (no context needed)"""
    import torch
    probes = torch.zeros((4, 3), dtype=torch.int64)
    offsets = torch.zeros(6, dtype=torch.int64)
    nlist, _, nq, nprobe, per_probe, dist, ids = codec._lists_args(
        torch.zeros((4, 8, 256)), offsets, probes, 5, None)
    assert (nlist, nq, nprobe, per_probe) == (5, 4, 3, 0) and dist.shape == ids.shape == (4, 5)
    assert codec._lists_args(torch.zeros((12, 8, 256)), offsets, probes, 5, None)[4] == 1
    for tables in (5, 8, 13, 0):
        with pytest.raises(capi.PqhError):
            codec._lists_args(torch.zeros((tables, 8, 256)), offsets, probes, 5, None)
