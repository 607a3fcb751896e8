"""The inputs of tests/test_gpu_forest_shapes.py have the properties that file relies on, shown
without a GPU: the case table reaches every kernel instantiation of pqh_knn_fast's three
dispatches, the controlled block populations are the ones intended, the list-path model
(forest_shapes_ref.path_model) proves both selection paths on the inputs built for them, and
the scales of the magnitude cases sit where they are meant to."""
import numpy as np
import pytest

import forest_shapes_ref as fs


def _sizes(oracle, c):
    st, en = oracle.knn_blocks_info(c["x"], c["ns"], c["nb"], c["ov"])
    mst, men = fs.blocks_info_model(c["x"], c["ns"], c["nb"], c["ov"])
    np.testing.assert_array_equal(st, mst)
    np.testing.assert_array_equal(en, men)
    return np.array([len(r) for r in fs.members(c["x"], st, en)], np.int64)


def test_every_instantiation_has_a_named_case():
    big = 400   # (every block of the grid is larger than 64 rows: test_grid_geometry)
    grid = {(fs.dp_of(d), fs.kmax_of(nn, big)[1]) for d in fs.GRID_D for nn in fs.GRID_NN}
    assert grid == {(dp, k) for dp in fs.DPS for k in fs.KMAXS}            # knn_screen: 20
    assert {fs.dp_of(d) for d in fs.GRID_D} == set(fs.DPS)                # knn_select_wave
    valu = {(fs.dmax_of(d), fs.kmax_of(nn, big)[1]) for d in fs.VALU_D for nn in fs.GRID_NN}
    assert valu == {(m, k) for m in fs.DMAXS for k in fs.KMAXS}            # knn_block_topk: 30
    lane = {(fs.dp_of(d), fs.kmax_of(nn, big)[1]) for d in fs.LANE_D for nn in fs.GRID_NN}
    assert lane == {(dp, k) for dp in fs.DPS for k in fs.KMAXS}            # knn_select: 20
    assert set(fs.LANE_GRID) <= set(fs.GRID)
    # both sides of every KMAX step, and of every DP and DMAX step
    for lo, hi in ((7, 8), (15, 16), (31, 32), (51, 52)):
        assert fs.kmax_of(lo, big)[1] < fs.kmax_of(hi, big)[1]
    for lo, hi in ((16, 17), (32, 33), (64, 65)):
        assert fs.dp_of(lo) < fs.dp_of(hi) and {lo, hi} <= set(fs.GRID_D)
    for lo, hi in ((8, 9), (96, 97)):
        assert fs.dmax_of(lo) < fs.dmax_of(hi) and {lo, hi} <= set(fs.VALU_D)
    assert {fs.kmax_of(nn, big)[1] for nn in fs.MST_NN} == set(fs.KMAXS)
    assert fs.GRID_MST <= set(fs.GRID) and len(fs.GRID_MST) == 10


@pytest.mark.parametrize("d", sorted(set(fs.GRID_D + fs.VALU_D + (40,))))
def test_grid_geometry(oracle, d):
    """three blocks, each larger than 64 rows (kmax = num_nn + 1 for every num_nn <= 63), and
    rows that lie in two blocks (the merge sees both lists)"""
    c = fs.build(fs.grid_name(d, 63))
    sizes = _sizes(oracle, c)
    assert len(sizes) == 3 and sizes.min() > 64
    assert sizes.sum() >= len(c["x"]) + 100


def test_members_model_is_the_oracles(oracle):
    c = fs.build("sizeB_two_n200_nn40")
    st, en = oracle.knn_blocks_info(c["x"], c["ns"], c["nb"], c["ov"])
    for a, b in zip(fs.members(c["x"], st, en), oracle.knn_members(c["x"], st, en)):
        np.testing.assert_array_equal(a, b)


def test_controlled_block_sizes(oracle):
    seen = set()
    mixed = {nn: 0 for nn in fs.SIZE_NN}
    for name in fs.SIZES:
        c = fs.build(name)
        sizes = _sizes(oracle, c)
        if name.startswith("sizeA"):
            n, nb = len(c["x"]), c["nb"]
            assert list(sizes) == fs.sizes_a(n, nb), name
            assert len(np.unique(c["x"][:, 0])) == n and (np.diff(c["x"][:, 0]) < 0).any()
        else:
            assert list(sizes) == fs.sizes_b(len(c["x"]), "two" in name), name
        np.testing.assert_array_equal(oracle.knn_fast(c["x"], c["nn"],
                                                      *oracle.knn_blocks_info(c["x"], c["ns"], c["nb"], c["ov"]))[2],
                                      sizes)
        seen |= set(int(s) for s in sizes)
        pop = sizes[sizes > 0]
        if (pop - 1 < c["nn"]).any() and (pop - 1 >= c["nn"]).any():
            mixed[c["nn"]] += 1
    assert set(fs.WANTED_SIZES) <= seen, sorted(set(fs.WANTED_SIZES) - seen)
    # blocks with never-filled slots (kk < kmax) beside blocks without, in one call
    assert all(v >= 2 for v in mixed.values()), mixed


def _counts(model):
    n = sum(len(r) for r, _, _ in model)
    return n, sum(int(l.sum()) for _, l, _ in model), sum(int(f.sum()) for _, _, f in model)


def test_path_model_separated_rows():
    n, listed, full = _counts(fs.path_model(fs.build("path_sep")))
    print(f"path_sep: {n} pairs, {listed} surely listed, {full} surely full")
    assert 2 * listed >= n


def test_path_model_identical_rows():
    c = fs.build("path_dups")
    dups = fs.dups_rows(c)
    assert len(dups) == fs.PATH_DUPS > 2 * fs.ch_of(c["nn"] + 1) + 8
    hit = 0
    for rows, listed, full in fs.path_model(c):
        isd = np.isin(rows, dups)
        if not isd.any():
            continue
        hit += 1
        assert isd.sum() == fs.PATH_DUPS           # all of them share the block ...
        assert full[isd].all()                     # ... and every one must scan it whole
        assert listed[~isd].any()                  # beside lists that must not overflow
        # the copies are not one run of positions: equal distances across both halves
        pos = np.flatnonzero(isd)
        assert (np.diff(pos) > 1).any()
    assert hit >= 1


def test_path_model_offset_rows():
    """E is of the order of the distances: the model proves neither path for any pair (the
    lists' lengths are then decided by the real error, far below E) -- a plain parity case"""
    c = fs.build("path_offset")
    n, listed, full = _counts(fs.path_model(c))
    print(f"path_offset: {n} pairs, {listed} surely listed, {full} surely full")
    x = c["x"].astype(np.float64)
    e = (3 * 2.0 ** -18 + (3 * 128 + 3 * 128 + 8) * 2.0 ** -24) * 1.25 * 2 * (x * x).sum(1).min()
    dist = fs.pair_dist64(x[:400])
    assert e > np.median(dist)
    assert listed == 0 and full == 0


@pytest.mark.parametrize("d,nn", fs.SCALE_BASE + fs.OVERFLOW_ONLY)
def test_scale_choices(oracle, d, nn):
    base = fs.build(fs.grid_name(d, nn))
    st, en = oracle.knn_blocks_info(base["x"], base["ns"], base["nb"], base["ov"])
    bi, bd, _ = oracle.knn_fast(base["x"], nn, st, en)
    kinds = {}
    for name, (_, s, kind) in fs.scale_cases().items():
        if not name.startswith(f"scale_d{d}_nn{nn}_"):
            continue
        kinds.setdefault(kind, []).append(s)
        c = fs.build(name)
        x = c["x"]
        sst, sen = c["geo"]
        mem = fs.members(x, sst, sen)
        for a, b in zip(mem, fs.members(base["x"], st, en)):
            np.testing.assert_array_equal(a, b)      # the same blocks at every scale
        oi, od, _ = oracle.knn_fast(x, nn, sst, sen)
        assert np.isfinite(od).all() and (od > 0).any(), name
        sq = x * x
        with np.errstate(over="ignore"):
            nrm = sq.sum(1, dtype=np.float32)
        if kind == "mid":
            # a power of two scales every product and sum exactly
            np.testing.assert_array_equal(x, base["x"] * np.float32(2.0 ** s))
            np.testing.assert_array_equal(oi, bi)
            np.testing.assert_array_equal(od, bd * np.float32(4.0 ** s))
        elif kind in ("overflow", "top"):
            dk = fs.pair_stats(d, nn)[0]
            assert dk * 4.0 ** s < fs.FP32_MAX <= dk * 4.0 ** (s + 1) * (1 + 2.0 ** -10)
            # Cmax = +inf in every block, or (top) nowhere, with the next power of two
            # already past the lists' distances
            assert all(np.isinf(nrm[r]).any() for r in mem) == (kind == "overflow"), name
            assert kind == "overflow" or (np.isfinite(nrm).all() and nrm.max() * 2 > fs.FP32_MAX / 2)
            np.testing.assert_array_equal(oi, bi)
        else:
            nz = sq[x != 0]
            tiny = np.float32(2.0 ** -126)
            assert (nz < tiny).any() and (nz > 0).all()
            if s == min(fs.tiny_exps(d, nn)):
                assert (nz < tiny).all()
            else:
                assert (nz >= tiny).any()
    if (d, nn) in fs.OVERFLOW_ONLY:
        assert sorted(kinds) == ["overflow"]
        return
    assert set(kinds) == {"mid", "overflow" if d == 16 else "top", "tiny"}
    assert len(kinds["tiny"]) == 2 and sorted(kinds["mid"]) == sorted(fs.MID_EXPS)


@pytest.mark.parametrize("d,nn", fs.SCALE_BASE)
def test_a_flushing_screen_fails_the_smallest_scale(d, nn):
    """At the smaller tiny scale every product of two coordinates is below 2^-126.  A screen
    whose MFMA returned 0 for the dot products there (denormals flushed) would order the
    candidates by their norms alone and, for most queries, drop a true neighbour from a list
    short enough to be trusted: parity of test_gpu_forest_shapes.py::test_scales at that scale
    therefore shows that v_mfma_f32_32x32x16_bf16 keeps them."""
    s = min(fs.tiny_exps(d, nn))
    c = fs.build(fs.scale_name(d, nn, s))
    assert (np.abs(c["x"]).max().astype(np.float64)) ** 2 < 2.0 ** -126
    pairs, wrong = fs.flush_model(c)
    print(f"{fs.scale_name(d, nn, s)}: a flushing screen fails {wrong} of {pairs} (block, query) pairs")
    assert 2 * wrong > pairs


def test_deep_tiny_scale(oracle):
    """float rows whose squares are denormals with few bits left: the products are rounded at
    2^-149 (the integer rows' never are) and the oracle keeps them.  (Rows of one norm say
    nothing about a flush: d' without the dot product is the same for every candidate.)"""
    base, s, kind = fs.scale_cases()[fs.DEEP_TINY]
    b, c = fs.build(base), fs.build(fs.DEEP_TINY)
    assert kind == "tiny" and c["x"].shape == (1200, 96)
    st, en = oracle.knn_blocks_info(b["x"], b["ns"], b["nb"], b["ov"])
    np.testing.assert_array_equal(st * np.float32(2.0 ** s), c["geo"][0])
    np.testing.assert_array_equal(en * np.float32(2.0 ** s), c["geo"][1])
    sizes = np.array([len(r) for r in fs.members(c["x"], *c["geo"])])
    assert sizes.min() > 64
    x = c["x"]
    np.testing.assert_array_equal(x.astype(np.float64), b["x"].astype(np.float64) * 2.0 ** s)
    sq32 = (x * x).astype(np.float64)
    sq64 = x.astype(np.float64) ** 2
    assert sq64.max() < 2.0 ** -126
    assert np.median(sq64) > 2.0 ** -145 and (sq32 != sq64).mean() > 0.8    # rounded, not lost
    oi, od, _ = oracle.knn_fast(x, c["nn"], *c["geo"])
    assert np.isfinite(od).all() and (od > 0).all() and len(np.unique(od)) > 100
