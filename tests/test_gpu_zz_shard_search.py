"""The sharded search (shard.ShardedIVF over pqh_shard_search_merge) with two ranks on one GPU
(gloo hooks, fresh child processes; tests/shard_search_worker.py): every rank's merged result
must be the same, equal the numpy restatement of the sharded procedure
(merge_ref.sharded_search_ref) exactly, and equal the single-process reference over all rows in
its distances, bit for bit, and in its ids wherever a query's distances are distinct.  A failing
rank must leave nobody waiting in the collective."""
import os
import subprocess
import sys

import numpy as np
import pytest

import merge_ref as mref
import shard_search_worker as worker
from conftest import ROOT, run_fail_msg

pytestmark = pytest.mark.gpu

# torchrun's own c10d store binds port 0 and the ranks reuse it (TORCHELASTIC_USE_AGENT_STORE):
# no port is picked here and released before the launcher binds it.
_LAUNCH = ["--standalone", "--local-addr=127.0.0.1"]


def _run(case, tmp_path):
    dump = tmp_path / "search.npz"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           *_LAUNCH,
           os.path.join(ROOT, "tests", "shard_search_worker.py"), "--case", case,
           "--out", str(dump)]
    r = subprocess.run(cmd, env=dict(os.environ, MASTER_ADDR="127.0.0.1"), capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, run_fail_msg(r)
    return np.load(dump, allow_pickle=False)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("case", ["plain", "residual", "wide", "masked", "removed"])
def test_two_rank_sharded_search(tmp_path, case):
    got = _run(case, tmp_path)
    gd, gi = got["dist"], got["ids"]
    assert gd.shape[0] == 2
    assert np.array_equal(_bits(gd[0]), _bits(gd[1])) and np.array_equal(gi[0], gi[1])
    w = worker.world_of(case)
    starts = mref.block_starts(worker.N, world=2)
    keep, gone = worker.masks(starts)
    k = 100 if case == "wide" else 10
    kw = dict(residual=case == "residual")
    if case == "masked":
        kw["keep"] = keep
    if case == "removed":
        kw["removed"] = gone
        assert int(got["live"]) == worker.N - len(gone)
    args = (w["q"], w["cc"], w["cent"], worker.NPROBE, k)
    wd, wi = mref.sharded_search_ref(w["x"], starts, *args, **kw)
    assert np.array_equal(_bits(gd[0]), _bits(wd)) and np.array_equal(gi[0], wi)
    od, oi = mref.block_search_ref(w["x"], *args, **kw)
    assert np.array_equal(_bits(gd[0]), _bits(od))
    sure = mref.distinct_mask(od)
    assert np.array_equal(gi[0][sure], oi[sure]) and (~sure).sum() <= 0.01 * sure.size
    assert (gi[0] >= 0).all()
    if case == "masked":
        assert keep[gi[0]].all() and (gi[0] < starts[1]).all()
    if case == "removed":
        assert not np.isin(gi[0], gone).any()
        assert (gone < starts[1]).any() and (gone >= starts[1]).any()


def test_two_rank_sharded_search_one_rank_fails(tmp_path):
    """rank 1 passes a non-zero status: both ranks return from the collective, both see
    PQH_ERR_REMOTE from search_status (asserted in the worker), both outputs are padding"""
    got = _run("fail", tmp_path)
    assert int(got["failed"]) == 1
    assert np.isinf(got["dist"]).all() and (got["dist"] > 0).all() and (got["ids"] == -1).all()
