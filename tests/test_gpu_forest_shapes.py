"""GPU parity of the forest builder's kNN (pqh_knn_blocks_info / pqh_knn_fast through
pq_huffman_amd.forest) at every kernel instantiation, block-size edge, list path, magnitude and
input layout of csrc/hip/pqh_knn.hip, on the default path and -- each in one fresh child
process (tests/knn_worker.py) -- under PQH_KNN_IMPL=valu and PQH_KNN_SELECT=lane.  Every
comparison is exact and against the oracle (oracle.knn_blocks_info / oracle.knn_fast): block
ranges, block sizes, indices as uint32 (0xFFFFFFFF slots included) and distances (+inf slots
included).  The inputs are the named cases of tests/forest_shapes_ref.py; that they have the
properties relied on here is shown without a GPU by tests/test_forest_shapes_cpu.py.

Case -> instantiation.  Every grid block holds more than 64 rows, so kmax = num_nn + 1 and

    num_nn   7     8, 15    16, 31    32, 51    52, 63
    KMAX     8     16       32        52        64

    test_grid[grid_d{d}_nn{nn}]     d     1, 16    17, 32    33, 64    65, 96, 128
      knn_split<DP>, knn_screen<DP, KMAX>, knn_select_wave<DP>:
                                    DP    16       32        64        128
    test_child[valu] (knn_block_topk<DMAX, KMAX>)
                                    d     8     9, 16    32    64    96    97, 128
                                    DMAX  8     16       32    64    96    128
    test_child[lane] (knn_screen<DP, KMAX> then knn_select<DP, KMAX>)
                                    d     1     17    64    96
                                    DP    16    32    64    128

  so test_grid reaches the 20 knn_screen and the 4 knn_select_wave instantiations (the fifth
  dispatch of the selection, the lane form, is test_child[lane]), the valu child the 30
  knn_block_topk and the lane child the 20 knn_select ones, each from both sides of every
  step of num_nn and d; grid_d16_* and grid_d128_* at num_nn 7, 15, 31, 51, 63 also feed the MST.
  test_block_sizes   block populations 0, 1, 2, 31, 32, 33, 63 .. 66, 127, 128, 129 (asserted on
                     the sizes read back), num_nn = 40 and 63: blocks with kk < kmax beside
                     full ones in one call; (DP 32; KMAX 8 .. 64 as the largest block allows)
  test_paths         path_sep: lists that cannot overflow; path_dups: 100 identical rows whose
                     lists must overflow beside block-mates whose lists must not (equal
                     distances in position order through the full scan); path_offset: every
                     coordinate + 4096, E of the order of the distances
  test_scales        grid_d16_nn15 / grid_d128_nn32 (/ grid_d96_nn16) times a power of two;
                     deep_like rows times 2^-68 (products rounded at 2^-149)
  test_strided       d = 40 and 128 as big[:, :d] of a NaN-padded (n, d + 24) tensor
  test_argument_errors
Both children also run the block-size and path cases, the valu child the strided and the
scaled ones too (a tiny scale that fails here and passes there blames the screen's bound).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import datagen
import forest_shapes_ref as fs
import knn_worker

pytestmark = pytest.mark.gpu

# the default path is the one under test here; the variants run in children only
assert "PQH_KNN_IMPL" not in os.environ and "PQH_KNN_SELECT" not in os.environ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_REF = {}    # case name -> the oracle's result, computed once and shared with the children's checks
_GPU = {}    # case name -> the default path's result (the scales' and strides' base runs)


@pytest.fixture(scope="module")
def gpu():
    import torch
    from pq_huffman_amd import codec, forest
    assert torch.cuda.is_available()
    return torch, forest, codec.Context(0)


def _ref(oracle, name):
    if name not in _REF:
        c = fs.build(name)
        st, en = oracle.knn_blocks_info(c["x"], c["ns"], c["nb"], c["ov"])
        oi, od, osz = oracle.knn_fast(c["x"], c["nn"], *(c["geo"] or (st, en)))
        for a in (st, en, oi, od, osz):
            a.setflags(write=False)
        _REF[name] = dict(starts=st, ends=en, idx=oi, dist=od, sizes=osz)
    return _REF[name]


def _same(got, want, name):
    for key in ("starts", "ends", "sizes", "idx", "dist"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=f"{name}: {key}")


def _run(gpu, name):
    """the default path's result of a case (host arrays) and its device lists"""
    torch, forest, ctx = gpu
    st, en, idx, dist, sizes = knn_worker.run_case(torch, forest, ctx, fs.build(name))
    got = dict(starts=st, ends=en, idx=idx.cpu().numpy().view(np.uint32),
               dist=dist.cpu().numpy(), sizes=sizes)
    _GPU[name] = got
    return got, idx, dist


def _mst(gpu, oracle, name, idx, dist, want):
    """the lists as the MST's input (as test_gpu_forest.py): the reference's mst_builder cannot
    read never-filled slots, so there the call must raise"""
    torch, forest, ctx = gpu
    nn = fs.build(name)["nn"]
    if (want["idx"] == 0xFFFFFFFF).any():
        with pytest.raises(Exception):
            forest.mst(ctx, idx, dist, 3)
        return
    codes = datagen.skewed_codes(len(want["idx"]), 8, seed=7)
    pq = torch.from_numpy(codes).cuda()
    for take, pen in ((min(5, nn), 0.0), (min(3, nn), 1.5), (nn, float("inf"))):
        tg, cn = forest.mst(ctx, idx, dist, take, pq, pen)
        otg, ocn = oracle.mst(want["idx"], want["dist"], take, codes, pen)
        np.testing.assert_array_equal(cn, ocn)
        np.testing.assert_array_equal(tg, otg)


# ------------------------------------------------------------------ 1. the instantiation grid
@pytest.mark.parametrize("name", fs.GRID)
def test_grid(gpu, oracle, name):
    c = fs.build(name)
    got, idx, dist = _run(gpu, name)
    assert got["sizes"].max() - 1 >= c["nn"] and got["sizes"].min() > 64   # kmax = num_nn + 1
    want = _ref(oracle, name)
    _same(got, want, name)
    if name in fs.GRID_MST:
        _mst(gpu, oracle, name, idx, dist, want)


# ------------------------------------------------------------------ 2. the two other implementations
@pytest.mark.parametrize("variant,var", [("valu", "PQH_KNN_IMPL"), ("lane", "PQH_KNN_SELECT")])
def test_child(oracle, tmp_path, variant, var):
    """one fresh process per variant runs all of its cases; its death, a non-zero status or
    the timeout fails the test, and nothing is started again"""
    names = fs.child_cases(variant)
    lst = tmp_path / "cases.json"
    lst.write_text(json.dumps(names))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "knn_worker.py"), str(lst),
                        str(tmp_path)], env={**os.environ, var: variant}, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, (r.stdout or "")[-2000:], (r.stderr or "")[-4000:])
    bad = []
    for name in names:
        got = np.load(tmp_path / (name + ".npz"), allow_pickle=False)
        want = _ref(oracle, name)
        if name.startswith("grid"):
            assert want["sizes"].max() - 1 >= fs.build(name)["nn"]
        try:
            _same(got, want, f"{variant}: {name}")
        except AssertionError as e:
            bad.append(str(e).strip().splitlines()[-1] if not bad else name)
    assert not bad, bad


# ------------------------------------------------------------------ 3. controlled block sizes
def test_block_sizes(gpu, oracle):
    seen = set()
    unfilled = 0
    for name in fs.SIZES:
        got, idx, dist = _run(gpu, name)
        want = _ref(oracle, name)
        _same(got, want, name)
        seen |= set(int(s) for s in got["sizes"])
        unfilled += bool((want["idx"] == 0xFFFFFFFF).any())
        _mst(gpu, oracle, name, idx, dist, want)
    assert set(fs.WANTED_SIZES) <= seen, sorted(set(fs.WANTED_SIZES) - seen)
    assert 0 < unfilled < len(fs.SIZES)   # both of _mst's branches ran


# ------------------------------------------------------------------ 4. both list paths
@pytest.mark.parametrize("name", fs.PATHS)
def test_paths(gpu, oracle, name):
    """which path every (block, query) pair of these inputs must take is proved by
    forest_shapes_ref.path_model (test_forest_shapes_cpu.py); here the result"""
    got, idx, dist = _run(gpu, name)
    want = _ref(oracle, name)
    _same(got, want, name)
    if name == "path_dups":   # every neighbour of a copy is another copy
        dups = fs.dups_rows(fs.build(name))
        assert (got["dist"][dups] == 0).all() and np.isin(got["idx"][dups], dups).all()
    _mst(gpu, oracle, name, idx, dist, want)


# ------------------------------------------------------------------ 5. magnitudes
@pytest.mark.parametrize("name", list(fs.scale_cases()))
def test_scales(gpu, oracle, name):
    """The rows of a grid case times 2^s, on that case's block ranges times 2^s.  Every
    product and sum scales exactly while nothing overflows or underflows: at the mid scales,
    and at the top of the range (where the distances of the lists are finite and, in the
    overflow cases, every block's Cmax is +inf, so the screen must list everything), the
    indices are the unscaled run's and the distances its distances times 4^s.  At the tiny
    scales (squares of some, or of all, coordinates below 2^-126) the bound E, a relative one,
    says nothing about an absolute flush: only the oracle decides.  (On an MI355X every scale
    matches: the MFMA keeps the denormal products, see test_forest_shapes_cpu.py's flush model.)"""
    base, s, kind = fs.scale_cases()[name]
    got, _, _ = _run(gpu, name)
    want = _ref(oracle, name)
    assert np.isfinite(want["dist"]).all() and (want["dist"] > 0).any()
    print(f"{name}: {kind}, rows differing from the oracle: "
          f"{int((got['idx'] != want['idx']).any(1).sum())} of {len(want['idx'])}")
    _same(got, want, name)
    if kind != "tiny":
        b = _GPU[base] if base in _GPU else _run(gpu, base)[0]
        np.testing.assert_array_equal(got["idx"], b["idx"])
        np.testing.assert_array_equal(got["dist"], b["dist"] * np.float32(4.0 ** s))
        np.testing.assert_array_equal(got["sizes"], b["sizes"])


# ------------------------------------------------------------------ 6. strided rows
@pytest.mark.parametrize("name", fs.STRIDED)
def test_strided(gpu, oracle, name):
    """a read past column d meets NaN: the bits must be the contiguous call's"""
    torch, forest, ctx = gpu
    c = fs.build(name)
    got, _, _ = _run(gpu, name)
    _same(got, _ref(oracle, name), name)
    st, en, idx, dist, sizes = knn_worker.run_case(torch, forest, ctx, dict(c, pad=0))
    _same(got, dict(starts=st, ends=en, idx=idx.cpu().numpy().view(np.uint32),
                    dist=dist.cpu().numpy(), sizes=sizes), name + " against contiguous")


# ------------------------------------------------------------------ 7. argument errors
@pytest.mark.parametrize("what,d,ns,nb,nn,status,msg", [
    ("num_nn_0", 8, 1, 2, 0, -1, None),
    ("num_nn_64", 8, 1, 2, 64, -1, None),
    ("d_129", 129, 1, 2, 5, -4, "d = 129 > 128"),
    ("num_split_0", 8, 0, 2, 5, -1, None),
    ("num_split_gt_d", 2, 3, 2, 5, -1, None),
    ("num_split_9", 12, 9, 2, 5, -1, None),
    ("blocks_per_dim_33", 8, 1, 33, 5, -1, None),
], ids=["num_nn_0", "num_nn_64", "d_129", "num_split_0", "num_split_gt_d", "num_split_9",
        "blocks_per_dim_33"])
def test_argument_errors(gpu, oracle, what, d, ns, nb, nn, status, msg):
    torch, forest, ctx = gpu
    from pq_huffman_amd.capi import PqhError
    x = datagen.sift_like(200, d, seed=5)
    xd = torch.from_numpy(x).cuda()
    geo_ok = 0 < ns <= min(d, 8) and 0 < nb <= 32
    if geo_ok:
        st, en = forest.blocks_info(ctx, xd, ns, nb, 0.1)
    else:
        with pytest.raises(PqhError) as e:
            forest.blocks_info(ctx, xd, ns, nb, 0.1)
        assert e.value.status == -1
        st = en = np.zeros((ns, nb), np.float32)
    with pytest.raises(PqhError) as e:
        forest.knn_fast(ctx, xd, nn, st, en)
    assert e.value.status == status
    if msg:
        assert msg in ctx.last_error()
    # the context is still usable
    name = "sizeA_n80_b2_nn40"
    _same(_run(gpu, name)[0], _ref(oracle, name), name + " after " + what)
