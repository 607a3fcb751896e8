"""The calls that take a row type (pqh_flat_create_rows, pqh_flat_search_lists_rows / _ip) without
a GPU: exported, declared and bound, and the argument errors answered before the context is
looked at."""
import os
import subprocess

import pytest

from pq_huffman_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LISTS = ["pqh_flat_search_lists_rows", "pqh_flat_search_lists_rows_ip"]
CALLS = ["pqh_flat_create_rows"] + LISTS
F32, F16, BF16 = 0, 1, 2


def test_calls_are_exported_declared_and_bound():
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    header = open(os.path.join(ROOT, "include", "pqh.h")).read()
    bound = {name for name, _, _ in capi.SIGNATURES}
    for name in CALLS:
        assert name in exported and name in bound and f"int {name}(" in header, name
    for name, value in (("PQH_ROWS_F32", F32), ("PQH_ROWS_F16", F16), ("PQH_ROWS_BF16", BF16)):
        assert f"#define {name} {value}\n" in header


# x, rows, n, ld_x, d, offsets, nlist, probes, queries, nq, ld_q, nprobe, top_k, keep, id_base,
# dist, ids with small numbers standing for pointers that are never followed
GOOD = dict(x=8, rows=F16, n=10, ld_x=4, d=4, offsets=8, nlist=2, probes=8, queries=8, nq=3, ld_q=4,
            nprobe=2, top_k=5, keep=None, id_base=0, dist=8, ids=8)
BAD = {"rows_3": dict(rows=3), "ld_x_below_d": dict(ld_x=3), "odd_address": dict(x=9),
       "f32_off_4_bytes": dict(rows=F32, x=10), "top_k_0": dict(top_k=0), "null_ids": dict(ids=None)}


@pytest.mark.parametrize("name", LISTS)
def test_list_scan_argument_errors_need_no_device(name):
    fn = getattr(capi.lib(), name)
    no_ctx = capi.lib().pqh_coarse_assign(None, None, None, 0, 1, None, None)
    assert no_ctx < 0
    for rows, x in ((F32, 8), (F16, 8), (BF16, 6)):   # good arguments: the NULL context is the answer
        assert fn(None, *{**GOOD, "rows": rows, "x": x}.values()) == no_ctx
    for what, change in BAD.items():
        assert fn(None, *{**GOOD, **change}.values()) == -1, what   # PQH_ERR_ARG


def test_create_argument_errors_need_no_device():
    fn = capi.lib().pqh_flat_create_rows
    no_ctx = capi.lib().pqh_coarse_assign(None, None, None, 0, 1, None, None)
    assert fn(None, 8, BF16, 10, 4, 4, 8) == no_ctx
    assert fn(None, 8, 3, 10, 4, 4, 8) == -1     # an unknown row type
    assert fn(None, 9, F16, 10, 4, 4, 8) == -1   # 16-bit rows on an odd address
