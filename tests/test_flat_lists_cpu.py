"""pqh_flat_search_lists / _ip without a GPU: exported, declared and bound, and the argument
errors answered before the context is looked at."""
import os
import subprocess

import pytest

from pq_huffman_amd import capi, codec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["pqh_flat_search_lists", "pqh_flat_search_lists_ip"]


def test_calls_are_exported_declared_and_bound():
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    header = open(os.path.join(ROOT, "include", "pqh.h")).read()
    bound = {name for name, _, _ in capi.SIGNATURES}
    for name in CALLS:
        assert name in exported and name in bound and f"int {name}(" in header, name
    assert callable(codec.flat_search_lists)
    assert all(hasattr(codec.IVFFlat, f) for f in ("build", "search", "remove", "live_count"))


# x, n, ld_x, d, offsets, nlist, probes, queries, nq, ld_q, nprobe, top_k, keep, id_base, dist, ids
# with 1 standing for a pointer that is never followed
GOOD = dict(x=1, n=10, ld_x=4, d=4, offsets=1, nlist=2, probes=1, queries=1, nq=3, ld_q=4, nprobe=2,
            top_k=5, keep=None, id_base=0, dist=1, ids=1)
BAD = {"top_k_0": dict(top_k=0), "nprobe_0": dict(nprobe=0), "ld_x_below_d": dict(ld_x=3),
       "null_queries": dict(queries=None), "null_ids": dict(ids=None),
       "negative_id_base": dict(id_base=-1), "misaligned_keep": dict(keep=2)}


@pytest.mark.parametrize("name", CALLS)
def test_argument_errors_need_no_device(name):
    fn = getattr(capi.lib(), name)
    no_ctx = capi.lib().pqh_coarse_assign(None, None, None, 0, 1, None, None)
    assert no_ctx < 0
    assert fn(None, *GOOD.values()) == no_ctx   # good arguments: the NULL context is the answer
    for what, change in BAD.items():
        assert fn(None, *{**GOOD, **change}.values()) == -1, what   # PQH_ERR_ARG
    assert fn(None, *{**GOOD, "nq": 0, "queries": None, "ids": None}.values()) == no_ctx
