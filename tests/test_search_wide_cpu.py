"""The wide search without a GPU: the two new context calls exported, declared and bound, their
NULL-context rule, the header's two limits; that the inputs of tests/search_wide_ref.py cover
what tests/test_gpu_search_wide.py claims for them; and the recall experiment the width is
for, in the float32 arithmetic of tests/refine_ref.py."""
import os
import subprocess
import sys

import numpy as np

from conftest import ROOT
from pq_huffman_amd import capi, codec

import refine_ref as rr
import search_filter_ref as fref
import search_wide_ref as wref

NEW_CALLS = ["pqh_ctx_set_search_max_k", "pqh_ctx_search_max_k"]


def test_limit_calls_are_exported_declared_and_bound():
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    header = open(os.path.join(ROOT, "include", "pqh.h")).read()
    bound = {name for name, _, _ in capi.SIGNATURES}
    for name in NEW_CALLS:
        assert name in exported and name in bound and f"int {name}(" in header, name
        assert getattr(capi.lib(), name).argtypes
    assert "#define PQH_SEARCH_MAX_K 64" in header
    assert "#define PQH_SEARCH_MAX_K_WIDE 256" in header
    assert "#define PQH_IVF_MAX_NPROBE 64" in header
    assert callable(codec.Context.set_search_max_k)
    assert isinstance(codec.Context.search_max_k, property)
    assert "search_max_k" not in codec.Context.TUNE          # a limit, not a tuning key


PROBE = """
from pq_huffman_amd import capi
L = capi.lib()
print(L.pqh_ctx_set_search_max_k(None, 256), L.pqh_ctx_set_search_max_k(None, 1000),
      L.pqh_ctx_search_max_k(None))
"""


def test_limit_calls_without_a_device():
    """the devices hidden: no context can exist, and a NULL one is refused before the value"""
    env = dict(os.environ)
    env["HIP_VISIBLE_DEVICES"] = ""
    env["ROCR_VISIBLE_DEVICES"] = ""
    r = subprocess.run([sys.executable, "-c", PROBE], capture_output=True, text=True, env=env,
                       cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["-2", "-2", "-2"], r.stdout + r.stderr


# ------------------------------------------------------------------------------ the inputs
def test_whole_stream_inputs():
    wref.check_whole_stream()


def test_ties_fall_on_every_block_boundary_and_threshold():
    wref.check_ties(wref.ties_lut(), wref.codes_of("ctx_m8"))


def test_offer_cases_pass_counts_and_landings():
    """of every later offer exactly j candidates beat the threshold, and they land where the
    case says: inside the threshold's block, across a block boundary, before everything"""
    codes = wref.offer_codes()
    seen = set()
    for top_k, j, order, landing, seed in wref.offer_cases():
        lut, dist = wref.offer_table(top_k, j, order, landing, seed)
        wref.check_offer_case(codes, lut, dist, top_k, j, order, landing)
        seen.add((top_k, j, order, landing))
    assert len(seen) == 4 * 6 * 3 * 2
    # the widened count agrees with search_shapes_ref's where both hold 64 entries
    import search_shapes_ref as sref
    d = np.random.default_rng(1).permutation(512).astype(np.float32)
    assert wref.offers_passing(d, 64) == sref.offers_passing(d, 64)


def test_grid_inputs():
    wref.check_grid_case(*wref.grid_case())


def test_probe_inputs_have_long_and_short_queries():
    for m, K in wref.PROBE_SHAPES:
        wref.check_probe_case(*wref.probe_case(m, K))


def test_refine_inputs():
    wref.check_refine_cands()
    for d in (15, 128):
        w = rr.residual_world(d)
        wref.check_residual_rows(w, wref.residual_rows(w))


def test_index_inputs():
    wref.check_ivf_world(fref.ivf_world())


# ------------------------------------------------------------------------------ what it is for
def test_recall_rises_with_the_candidates():
    """20,000 SIFT-shaped rows, 200 queries, an 8 x 256 first and a 16 x 256 second code: with 256
    candidates instead of 64 more of the exact top 10 are among them, and more of them come out
    of the re-rank"""
    got = wref.recall_experiment((64, 256))
    print(got)
    (share64, recall64), (share256, recall256) = got[64], got[256]
    assert share256 > share64
    assert recall256 > recall64
