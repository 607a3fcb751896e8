"""The exact re-rank without a GPU: the four calls exported, declared and bound, every argument
error of the contract answered before the context is looked at, and the reference against a
double-loop chain."""
import os
import subprocess

import numpy as np
import pytest

import rerank_ref
import sq_ref
from pq_huffman_amd import capi, codec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["pqh_rerank_rows", "pqh_rerank_rows_ip", "pqh_rerank_sq", "pqh_rerank_sq_ip"]


def test_calls_are_exported_declared_and_bound():
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    header = open(os.path.join(ROOT, "include", "pqh.h")).read()
    bound = {name for name, _, _ in capi.SIGNATURES}
    for name in CALLS:
        assert name in exported and name in bound and f"int {name}(" in header, name
    assert callable(codec.rerank) and hasattr(codec.IVF, "set_rows")


# the arguments in pqh.h's order, 4 standing for a pointer that is never followed
TAIL = dict(queries=4, nq=3, ld_q=4, cand=4, ncand=8, top_k=5, dist=4, ids=4, ld_out=5)
GOOD = {"rows": dict(x=4, rows=0, n=10, ld_x=4, d=4, **TAIL),
        "sq": dict(x=4, n=10, ld_x=4, d=4, vmin=4, step=4, **TAIL)}
BAD = {"negative_n": dict(n=-1), "d_0": dict(d=0), "ld_x_below_d": dict(ld_x=3), "negative_nq": dict(nq=-1),
       "ld_q_below_d": dict(ld_q=3), "ncand_0": dict(ncand=0), "ncand_257": dict(ncand=257, top_k=5),
       "top_k_0": dict(top_k=0), "top_k_above_ncand": dict(top_k=9, ld_out=9),
       "ld_out_below_top_k": dict(ld_out=4), "null_queries": dict(queries=None),
       "null_cand": dict(cand=None), "null_dist": dict(dist=None), "null_ids": dict(ids=None),
       "null_store": dict(x=None)}
BAD_ROWS = {"unknown_type": dict(rows=3), "x_off_its_element": dict(rows=1, x=5), "f32_off_4": dict(x=6)}
BAD_SQ = {"null_vmin": dict(vmin=None), "null_step": dict(step=None)}


@pytest.mark.parametrize("name", CALLS)
def test_argument_errors_need_no_device(name):
    fn = getattr(capi.lib(), name)
    kind = "sq" if "_sq" in name else "rows"
    good = GOOD[kind]
    no_ctx = capi.lib().pqh_coarse_assign(None, None, None, 0, 1, None, None)
    assert no_ctx < 0
    assert fn(None, *good.values()) == no_ctx   # good arguments: the NULL context is the answer
    for what, change in {**BAD, **(BAD_SQ if kind == "sq" else BAD_ROWS)}.items():
        assert fn(None, *{**good, **change}.values()) == -1, what   # PQH_ERR_ARG
    # nothing to do, no rows: the pointers are not looked at
    assert fn(None, *{**good, "nq": 0, "queries": None, "cand": None, "ids": None}.values()) == no_ctx
    assert fn(None, *{**good, "n": 0, "x": None}.values()) == no_ctx


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_reference_is_the_double_loop_chain(metric):
    rng = np.random.default_rng(2)
    x, q = rng.standard_normal((9, 5)).astype(np.float32), rng.standard_normal((2, 5)).astype(np.float32)
    x[4] = x[1]
    vmin, step = sq_ref.train(x)
    codes = sq_ref.encode(x, vmin, step)
    cand = np.array([[4, -1, 1, 9, 7, 7], [-1, -1, -2, -1, -1, -1]], np.int64)
    for store, sq, rows in ((x, None, x), (codes, (vmin, step), sq_ref.decode(codes, vmin, step))):
        dist, ids, bad = rerank_ref.rerank(q, store, cand, 5, metric, sq)
        assert bad == {9, -2} and ids[0].tolist() == sorted([1, 4, 7, 7], key=lambda r: (chain(q[0], rows[r], metric), r)) + [-1]
        for j, r in enumerate(ids[0][:4]):
            assert dist[0, j].view(np.uint32) == chain(q[0], rows[r], metric).view(np.uint32)
        assert np.isinf(dist[0, 4]) and np.isinf(dist[1]).all() and (ids[1] == -1).all()


def chain(q, row, metric):
    acc = np.float32(0)
    for qv, xv in zip(q, row):   # (float32 scalars: every operation rounds to float32)
        acc = acc - qv * xv if metric == "ip" else acc + (qv - xv) * (qv - xv)
    assert acc.dtype == np.float32
    return acc
