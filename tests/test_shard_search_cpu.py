"""The sharded search without a GPU: the interface of the four new calls, the numpy merge
(tests/merge_ref.py) against a brute-force statement, the torch half of the protocol
(shard.gather_topk) over gloo with 2 and 3 ranks against the single-process reference, and the
Python arithmetic of shard.ShardedIVF (id bases, the keep= slice, the routing of removed ids)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import merge_ref as mref
from conftest import ROOT
from pq_huffman_amd import shard

CALLS = ("pqh_topk_merge", "pqh_shard_search_scratch_bytes", "pqh_shard_search_merge",
         "pqh_shard_search_status")


# ------------------------------------------------------------------------------ the interface
def test_entry_points_are_declared_exported_and_bound():
    from pq_huffman_amd import capi
    header = open(os.path.join(ROOT, "include", "pqh.h")).read()
    bound = {name: args for name, _, args in capi.SIGNATURES}
    for name in CALLS:
        decl = re.search(r"\b(?:int|unsigned long long) " + name + r"\(([^;]*)\);", header)
        assert decl, name
        args = re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S)
        assert len(bound[name]) == args.count(",") + 1, name
        assert hasattr(capi.lib(), name)
    makefile = open(os.path.join(ROOT, "pq_huffman_amd", "csrc", "Makefile")).read()
    assert re.search(r"^HIP_SRC\s*:=.*\bpqh_merge\.hip\b", makefile, flags=re.M)


def test_null_context_is_refused_first():
    from pq_huffman_amd import capi
    lib = capi.lib()
    n = ctypes.c_int(0)
    lib.pqh_device_count(ctypes.byref(n))
    want = -1 if n.value > 0 else -2
    assert lib.pqh_topk_merge(None, None, None, 0, -1, 0, None, 0, None, None) == want
    assert lib.pqh_shard_search_merge(None, None, None, None, -1, 0, 0, 0, None, 0, None, None,
                                      None) == want
    assert lib.pqh_shard_search_status(None, None) == want


def test_python_has_the_new_names():
    from pq_huffman_amd import codec
    assert list(inspect.signature(codec.merge_topk).parameters) == [
        "ctx", "dist", "ids", "k", "id_base", "out"]
    assert list(inspect.signature(shard.search_merge).parameters) == [
        "ctx", "comm", "dist", "ids", "id_base", "status", "check"]
    assert list(inspect.signature(shard.gather_topk).parameters) == [
        "dist", "ids", "world", "rank", "group"]
    assert list(inspect.signature(shard.search_status).parameters) == ["ctx", "state"]
    for name in ("build", "search", "remove", "live_count"):
        assert callable(getattr(shard.ShardedIVF, name))


def test_scratch_bytes():
    from pq_huffman_amd import capi
    f = capi.lib().pqh_shard_search_scratch_bytes
    record = lambda nq, k: 16 + (nq * k * 4 + 7) // 8 * 8 + nq * k * 8
    for world in (1, 2, 3, 8):
        for nq in (0, 1, 5, 33, 512):
            for k in (1, 10, 63, 64, 65, 256):
                got = f(world, nq, k)
                assert got >= world * record(nq, k) and got % 8 == 0, (world, nq, k)
                assert f(world + 1, nq, k) >= got and f(world, nq + 1, k) >= got
                if k < 256:
                    assert f(world, nq, k + 1) >= got
    # what the collective refuses at once has no size
    assert f(0, 1, 1) == 0 and f(1, -1, 1) == 0 and f(1, 1, 0) == 0 and f(1, 1, 257) == 0
    assert f(1, 2 ** 31, 1) == 0


# ------------------------------------------------------------------------------ the numpy merge
@pytest.mark.parametrize("parts,nq,k_in,k,bases", [
    (1, 1, 1, 1, None), (2, 3, 10, 10, [0, 100]), (3, 4, 7, 30, [5, 1 << 40, 77]),
    (5, 2, 20, 6, None)])
def test_merge_ref_against_brute_force(parts, nq, k_in, k, bases):
    d, i = mref.tied_parts(parts, nq, k_in, seed=parts * 100 + k_in, bases=bases)
    if parts * k_in > 8:
        assert (i < 0).any() and (np.isfinite(d) & (i < 0)).any()      # padding and (finite, -1)
        live = d[i >= 0]
        assert len(np.unique(live)) < len(live)                         # ties
    wd, wi = mref.merge_topk_ref(d, i, bases, k)
    bd, bi = mref.brute_topk(d, i, bases, k)
    assert np.array_equal(wd.view(np.uint32), bd.view(np.uint32)) and np.array_equal(wi, bi)
    base = np.zeros(parts, np.int64) if bases is None else np.asarray(bases, np.int64)
    for q in range(nq):                                      # ids unique after the bases
        g = (i[:, q, :] + base[:, None])[i[:, q, :] >= 0]
        assert len(np.unique(g)) == len(g)
    assert ((wi >= 0) == np.isfinite(wd)).all()


def test_distinct_mask():
    d = np.array([[1, 2, 2, 3, 4, 4, 4, 5]], np.float32)
    assert mref.distinct_mask(d).tolist() == [[True, False, False, True, False, False, False, True]]


# ------------------------------------------------------------------------------ Python arithmetic
def test_id_bases_are_the_exclusive_sum():
    assert shard.id_bases([1, 3000]) == [0, 1]
    assert shard.id_bases([3000, 1]) == [0, 3000]
    assert shard.id_bases([5]) == [0]
    assert shard.id_bases([0, 7, 0, 2]) == [0, 0, 7, 7]
    for n in (601, 3001):
        for world in (2, 3, 5):
            ranges = [shard.row_range(n, world, r) for r in range(world)]
            assert shard.id_bases([e - b for b, e in ranges]) == [b for b, _ in ranges]


def test_keep_slices_and_remove_routing():
    n, world = 601, 3
    rng = np.random.default_rng(3)
    keep = torch.from_numpy(rng.random(n) < 0.4)
    gone = torch.from_numpy(rng.choice(n, 50, replace=False).astype(np.int64))
    pieces, routed = [], []
    for r in range(world):
        b, e = shard.row_range(n, world, r)
        pieces.append(shard.keep_slice(keep, b, e - b))
        assert pieces[-1].shape == (e - b,)
        mine = shard.local_ids(gone, b, e - b)
        assert ((mine >= 0) & (mine < e - b)).all()
        routed.append(mine + b)
    assert torch.equal(torch.cat(pieces), keep)
    assert sorted(torch.cat(routed).tolist()) == sorted(gone.tolist())      # each id to one rank


# ------------------------------------------------------------------------------ over gloo
N, D, M, NLIST, NPROBE, NQ, K = 601, 16, 4, 8, 3, 5, 10


def _world():
    return mref.search_world(N, D, NLIST, NQ, M, seed=51)


def _masks():
    rng = np.random.default_rng(9)
    keep = rng.random(N) < 0.5
    return keep, rng.choice(N, 80, replace=False).astype(np.int64)


def _worker(rank, world, store_file, q):
    dist.init_process_group("gloo", init_method=f"file://{store_file}", rank=rank,
                            world_size=world)
    try:
        w = _world()
        keep, gone = _masks()
        b, e = shard.row_range(N, world, rank)
        counts = [None] * world
        dist.all_gather_object(counts, e - b)
        bases = shard.id_bases(counts)
        assert bases[rank] == b
        out = {}
        for name in ("free", "filtered"):
            kw = {}
            if name == "filtered":       # the slices of ShardedIVF.search and .remove
                kw = dict(keep=shard.keep_slice(torch.from_numpy(keep), b, e - b).numpy(),
                          removed=shard.local_ids(torch.from_numpy(gone), b, e - b).numpy())
            d, i = mref.block_search_ref(w["x"][b:e], w["q"], w["cc"], w["cent"], NPROBE, K, **kw)
            all_d, all_i = shard.gather_topk(torch.from_numpy(d), torch.from_numpy(i), world, rank)
            assert all_d.shape == (world, NQ, K) and all_i.dtype == torch.int64
            out[name] = mref.merge_topk_ref(all_d.numpy(), all_i.numpy(), bases, K)
        if rank == 0:
            q.put(out)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_search_matches_single_process(world, tmp_path):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    store_file = tmp_path / "store"
    procs = [ctx.Process(target=_worker, args=(r, world, str(store_file), q))
             for r in range(world)]
    for p in procs:
        p.start()
    got = q.get(timeout=120)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    w = _world()
    keep, gone = _masks()
    for name, kw in (("free", {}), ("filtered", dict(keep=keep, removed=gone))):
        wd, wi = mref.block_search_ref(w["x"], w["q"], w["cc"], w["cent"], NPROBE, K, **kw)
        assert (wi >= 0).all()
        for row in wd:                        # continuous data: no ties, so ids must agree too
            assert len(np.unique(row)) == K
        assert np.array_equal(got[name][0].view(np.uint32), wd.view(np.uint32)), name
        assert np.array_equal(got[name][1], wi), name
    assert not np.array_equal(got["free"][1], got["filtered"][1])
    assert keep[got["filtered"][1]].all() and not np.isin(got["filtered"][1], gone).any()


def test_gather_topk_one_rank():
    d, i = torch.rand(3, 4), torch.arange(12).reshape(3, 4)
    all_d, all_i = shard.gather_topk(d, i, 1, 0)
    assert all_d.shape == (1, 3, 4) and torch.equal(all_d[0], d) and torch.equal(all_i[0], i)
