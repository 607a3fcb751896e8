"""The IVF-SQ8 calls without a GPU: exported, declared and bound, the argument errors answered
before the context is looked at, and the reference's own round trip within its error bound."""
import os
import subprocess

import numpy as np
import pytest

import sq_ref
from pq_huffman_amd import capi, codec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEARCHES = ["pqh_sq_search_lists", "pqh_sq_search_lists_ip"]
CALLS = ["pqh_sq_train", "pqh_sq_encode", "pqh_sq_decode"] + SEARCHES


def test_calls_are_exported_declared_and_bound():
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    header = open(os.path.join(ROOT, "include", "pqh.h")).read()
    bound = {name for name, _, _ in capi.SIGNATURES}
    for name in CALLS:
        assert name in exported and name in bound and f"int {name}(" in header, name
    assert callable(codec.sq_search_lists)
    assert all(hasattr(codec.SQ, f) for f in ("train", "encode", "decode"))
    assert all(hasattr(codec.IVFSQ, f) for f in ("build", "search", "remove", "live_count", "fetch", "nbytes"))


# the arguments in pqh.h's order, 1 standing for a pointer that is never followed
GOOD = {
    "pqh_sq_train": dict(x=1, n=10, ld_x=4, d=4, vmin=1, step=1),
    "pqh_sq_encode": dict(x=1, n=10, ld_x=4, d=4, perm=None, vmin=1, step=1, codes=1, ld_c=4),
    "pqh_sq_decode": dict(codes=1, n=10, ld_c=4, d=4, vmin=1, step=1, rows=None, first=2, count=8,
                          out=1, ld_out=4),
    "search": dict(codes=1, n=10, ld_c=4, d=4, vmin=1, step=1, offsets=1, nlist=2, probes=1, queries=1,
                   nq=3, ld_q=4, nprobe=2, top_k=5, keep=None, id_base=0, dist=1, ids=1),
}
BAD = {
    "pqh_sq_train": {"d_0": dict(d=0), "ld_x_below_d": dict(ld_x=3), "null_step": dict(step=None),
                     "null_x": dict(x=None), "negative_n": dict(n=-1)},
    "pqh_sq_encode": {"ld_c_below_d": dict(ld_c=3), "ld_x_below_d": dict(ld_x=3),
                      "null_codes": dict(codes=None), "null_vmin": dict(vmin=None)},
    "pqh_sq_decode": {"ld_c_below_d": dict(ld_c=3), "ld_out_below_d": dict(ld_out=3),
                      "range_past_n": dict(count=9), "negative_first": dict(first=-1),
                      "null_out": dict(out=None)},
    "search": {"top_k_0": dict(top_k=0), "nprobe_0": dict(nprobe=0), "ld_c_below_d": dict(ld_c=3),
               "null_queries": dict(queries=None), "null_ids": dict(ids=None), "null_step": dict(step=None),
               "negative_id_base": dict(id_base=-1), "misaligned_keep": dict(keep=2)},
}


@pytest.mark.parametrize("name", CALLS)
def test_argument_errors_need_no_device(name):
    fn = getattr(capi.lib(), name)
    kind = "search" if name in SEARCHES else name
    no_ctx = capi.lib().pqh_coarse_assign(None, None, None, 0, 1, None, None)
    assert no_ctx < 0
    assert fn(None, *GOOD[kind].values()) == no_ctx   # good arguments: the NULL context is the answer
    for what, change in BAD[kind].items():
        assert fn(None, *{**GOOD[kind], **change}.values()) == -1, what   # PQH_ERR_ARG
    if kind == "search":
        assert fn(None, *{**GOOD[kind], "nq": 0, "queries": None, "ids": None}.values()) == no_ctx


@pytest.mark.parametrize("offset,scale", [(0, 1), (-5, 100), (30000, 7)])
def test_reference_round_trip_is_within_its_bound(offset, scale):
    """|x - decode(encode(x))| <= step / 2 + 2^-22 (max(|vmin|, |vmax|) + 255 step) per dimension:
    half a step of the rounding to a code, and the four roundings of encode and decode"""
    x = (offset + scale * np.random.default_rng(5).standard_normal((4000, 6))).astype(np.float32)
    vmin, step = sq_ref.train(x)
    codes = sq_ref.encode(x, vmin, step)
    assert codes.min() == 0 and codes.max() == 255
    err = np.abs(x.astype(np.float64) - sq_ref.decode(codes, vmin, step)).max(axis=0)
    s = step.astype(np.float64)
    bound = 0.5 * s + 2.0 ** -22 * (np.maximum(np.abs(vmin), np.abs(x.max(axis=0))) + 255 * s)
    assert (err <= bound).all(), (err / bound).max()
