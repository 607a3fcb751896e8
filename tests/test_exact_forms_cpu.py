"""CPU pins for tests/exact_forms_cases.py: every case's numpy reference runs, and every case
has the property tests/test_gpu_exact_forms.py names it for -- the kernel form its shape selects
(a mirror of flat_search's dispatch in pqh_flat.hip), the number of non-finite queries, the pair
counts of the units its probe table makes, the dead tiles of its mask -- so that a change of a
generator cannot silently empty a case.  The expected output of every case is unique: no
candidate distance of a compared query is NaN and no candidate id is named twice, so the order by
(dist, id) is total."""
import numpy as np
import pytest

import exact_forms_cases as cases
from exact_forms_cases import FLAT, LISTS, METRICS, RERANK, TILE

CUS = 256   # the compute units of an MI355X: the slabs of Flat depend on them


def flat_plan(n, d, nq, k, cus=CUS):
    """(form, wide, query groups, slabs) as flat_search (pqh_flat.hip) chooses them"""
    wide = k > 64
    screen = d <= 1024 and n > 0
    form = "valu" if not screen else "panel" if d > 128 else "reg"
    groups = -(-nq // (32 if wide else 128)) if screen else nq
    target = max(1, cus * (1 if screen else 8) // groups)
    slab_rows = max(1024, (-(-n // target) + 31) // 32 * 32)
    return form, wide, groups, -(-n // slab_rows)


def flat_vec(c, rows):
    """(vec_x, vec_q, vec_chain) of a Flat case (buffers start on 16 bytes)"""
    d, per16 = c["d"], 4 if rows == "f32" else 8
    layout = c.get("x_layout", "plain")
    ld_x, ld_q = (d + 1 if layout == "stride1" else d), d + c.get("q_pad", 0)
    x16 = ld_x % per16 == 0 and layout != "shift"
    q16 = ld_q % 4 == 0
    return d % 16 == 0 and x16, d % 16 == 0 and q16, d % per16 == 0 and x16 and q16


def _total_order(dist, ids):
    assert not np.isnan(dist).any()
    assert len(np.unique(ids)) == len(ids)


@pytest.mark.parametrize("case,rows", cases.flat_ids())
def test_flat_cases(case, rows):
    c, w = FLAT[case], cases.flat_world(case, rows)
    n, d, nq, k = c["n"], c["d"], c["nq"], c["k"]
    form, wide, groups, slabs = flat_plan(n, d, nq, k)
    bad = int((~w["compared"]).sum())
    assert bad == (3 if c.get("bad_q") else 1 if c.get("nan_q") else 0)
    assert np.isfinite(w["q"]).all() and np.array_equal(w["q"][w["compared"]], w["q_sent"][w["compared"]])
    assert np.array_equal(cases.exact(w["x"], rows).view(np.uint32), w["x"].view(np.uint32))
    # the fallback count the GPU test asserts is the one the inputs give
    if form == "valu" or c.get("inf_row"):
        assert c["fallback"] == "nq"
    else:
        assert c["fallback"] == bad
    if c.get("inf_row"):
        assert np.isinf(w["x"]).sum() == 1 and not w["keep"][40] and form != "valu"
    else:
        assert np.isfinite(w["x"]).all()
    keep = w["keep"]
    if c.get("keep") == "half":   # an empty tile among kept ones, and rows enough for every k
        tiles = np.add.reduceat(keep, np.arange(0, n, 32))
        # (the last tile may be a few rows only)
        assert tiles[5] == 0 and (np.delete(tiles, 5)[:-1] > 0).all() and keep.sum() > k
        assert w["id_base"] == cases.ID_BASE
    if c.get("keep") == "none":
        assert not keep.any()
    for metric in METRICS:
        wd, wi = cases.flat_want(case, rows, metric)
        assert wd.shape == wi.shape == (nq, k) and wd.dtype == np.float32 and wi.dtype == np.int64
        if c.get("keep") == "none":
            assert np.isinf(wd).all() and (wd > 0).all() and (wi == -1).all()
        else:
            full = min(k, n if keep is None else int(keep.sum()))
            assert (wi[:, :full] >= w["id_base"]).all() and (wi[:, full:] == -1).all()
            assert np.isfinite(wd[w["compared"]][:, :full]).all()


# the form every Flat case is named for: (form, wide, groups, slabs)
FLAT_FORMS = {
    "wide_panels_k129": ("panel", True, 2, 1), "wide_panels_k256": ("panel", True, 2, 1),
    "wide_valu_k65": ("valu", True, 3, 1), "wide_valu_k256": ("valu", True, 3, 1),
    **{f"k_edges_k{k}": ("reg", True, 2, 3) for k in (65, 128, 129, 256)},
    "groups_x_slabs_k5": ("reg", False, 2, 3), "groups_x_slabs_k70": ("reg", True, 5, 3),
    "mask_panel": ("panel", False, 1, 1), "mask_wide_reg": ("reg", True, 2, 3),
    "mask_wide_panel": ("panel", True, 2, 1), "mask_valu_k5": ("valu", False, 3, 1),
    "mask_valu_k65": ("valu", True, 3, 1), "none_wide_panel": ("panel", True, 2, 1),
    "none_valu": ("valu", True, 3, 1),
    "fb_reg_mask": ("reg", False, 1, 3), "fb_wide_reg": ("reg", True, 2, 3),
    "fb_panel": ("panel", False, 1, 1), "fb_wide_panel_mask": ("panel", True, 2, 1),
    "inf_row_wide": ("reg", True, 2, 3), "inf_row_panel": ("panel", False, 1, 1),
    **{f"elem_d32_{lay}": ("reg", False, 1, 1) for lay in ("stride1", "shift", "q_stride1")},
    **{f"elem_d144_{lay}": ("panel", False, 1, 1) for lay in ("stride1", "shift", "q_stride1")},
    **{f"qstride_{f}_pad{p}": v for p in (3, 4)
       for f, v in (("reg", ("reg", False, 1, 3)), ("panel", ("panel", False, 1, 1)),
                    ("valu", ("valu", False, 3, 1)), ("fallback", ("reg", False, 1, 3)))},
}


def test_flat_cases_select_the_forms_they_name():
    assert set(FLAT_FORMS) == set(FLAT)
    for name, c in FLAT.items():
        assert flat_plan(c["n"], c["d"], c["nq"], c["k"]) == FLAT_FORMS[name], name
    # two panels with a short last one; a query wave of one query beside a full one
    assert -(-136 // 16) == 9 and 33 % 32 == 1
    # the loads: element loads of rows and queries at d % 16 == 0, and the two mixed settings
    for rows in cases.ROWS:
        for d in (32, 144):
            assert flat_vec(FLAT[f"elem_d{d}_stride1"], rows) == (False, True, False)
            assert flat_vec(FLAT[f"elem_d{d}_shift"], rows) == (False, True, False)
            assert flat_vec(FLAT[f"elem_d{d}_q_stride1"], rows) == (True, False, False)
        assert flat_vec(FLAT["qstride_reg_pad3"], rows) == (True, False, False)
        assert flat_vec(FLAT["qstride_reg_pad4"], rows) == (True, True, True)
        assert flat_vec(FLAT["qstride_valu_pad4"], rows)[2] and not flat_vec(FLAT["qstride_valu_pad3"], rows)[2]


@pytest.mark.parametrize("case,store", cases.list_ids())
def test_list_cases(case, store):
    lengths, d, ld, nq, nprobe, k, opt = LISTS[case]
    w = cases.list_world(case, store)
    offsets, probes, keep = w["offsets"], w["probes"], w["keep"]
    n, nlist = int(offsets[-1]), len(lengths)
    assert probes.shape == (nq, nprobe) and ((probes >= -1) & (probes < nlist)).all()
    assert np.isfinite(w["x"]).all() and w["x"].shape == (n, d) and ld >= d
    if store == "sq8":
        assert w["own"].dtype == np.uint8 and len(np.unique(w["own"])) > 200
    else:
        assert np.array_equal(cases.exact(w["x"], store).view(np.uint32), w["x"].view(np.uint32))
    for i, row in enumerate(probes):   # distinct lists, -1 only behind them; no tie, no NaN
        valid = row[row >= 0]
        assert len(set(valid)) == len(valid) and (row[:len(valid)] >= 0).all()
    for metric in METRICS:
        wd, wi = cases.list_want(case, store, metric)
        assert wd.shape == wi.shape == (nq, k)
        assert not np.isnan(wd).any()
        for i in range(nq):
            _total_order(wd[i][wi[i] >= 0], wi[i][wi[i] >= 0])
        assert (wi >= 0).any()


def test_list_cases_have_the_units_and_loads_they_name():
    sweep = cases.list_world("pairs_sweep", "f32")["probes"]
    lengths = LISTS["pairs_sweep"][0]
    assert [int((sweep == l).sum()) for l in range(16)] == list(range(1, 17))
    assert sorted(cases.unit_sizes(sweep, lengths, 16)) == list(range(1, 17))   # u_cnt 1 .. 16
    assert {(u + 3) // 4 for u in range(1, 17)} == {1, 2, 3, 4}                 # every ng
    wide = cases.unit_sizes(cases.list_world("pairs_sweep_wide", "f32")["probes"], lengths, 4)
    assert set(wide) == {1, 2, 3, 4} and len(wide) == sum(-(-c // 4) for c in range(1, 17))
    assert sorted(lengths) == [70] * 15 + [300]
    for name in ("qstride_pad3", "qstride_pad4"):   # a second unit on each list
        w = cases.list_world(name, "f32")
        assert cases.unit_sizes(w["probes"], LISTS[name][0], 16) == [16, 1, 16, 1]
    # many_units: more units than any other case, fewer than the grid's bound, empty lists probed
    units = {}
    for name, store in cases.list_ids():
        lengths, d, ld, nq, nprobe, k, opt = LISTS[name]
        qb = 16 if k <= 64 else 4
        w = cases.list_world(name, store)
        units[name] = (len(cases.unit_sizes(w["probes"], lengths, qb)),
                       min(nq * nprobe, len(lengths) + nq * nprobe // qb))
    many = units.pop("many_units")
    assert many[0] > max(u for u, _ in units.values()) and many[0] < many[1]
    w = cases.list_world("many_units", "f32")
    assert any(LISTS["many_units"][0][l] == 0 for l in w["probes"].ravel())
    # the loads of the fp32 scan: 16-byte loads past one chunk of 32, ragged and whole last chunks
    for d in (36, 64, 100, 128, 132):
        lengths, dd, ld, *_ , opt = LISTS[f"vec_d{d}"]
        assert dd == ld == d and d % 4 == 0 and d > 32 and "shift" not in opt
    assert {d % 32 for d in (36, 64, 100, 128, 132)} == {4, 0}
    assert LISTS["vec_d64_shift"][2] % 4 == 0 and LISTS["vec_d64_shift"][6]["shift"] == 1
    assert LISTS["vec_d64_gap"][2] == 68
    for d in (40, 64, 72):   # 16-bit rows: a whole 16-byte piece in the second chunk of 32
        assert LISTS[f"vec_d{d}"][2] % 2 == 0 and d >= 32 + 8
    assert LISTS["qstride_pad3"][1] == 40   # two chunks of 32, one chunk of 64 codes


@pytest.mark.parametrize("store", cases.STORES)
def test_masked_groups_start_and_end_on_a_dead_tile(store):
    lengths, d, ld, nq, nprobe, k, opt = LISTS["masked_groups"]
    keep = cases.list_world("masked_groups", store)["keep"]
    groups, nt = opt["groups"], -(-lengths[0] // TILE)
    live = [bool(keep[t * TILE:min((t + 1) * TILE, lengths[0])].any()) for t in range(nt)]
    assert live == [False, True, True, True, False]
    spans = [(g * nt // groups, (g + 1) * nt // groups) for g in range(groups)]
    assert spans == [(0, 1), (1, 3), (3, 5)]
    assert not live[spans[0][0]] and not live[spans[2][1] - 1] and live[spans[2][0]]
    assert keep[lengths[0]:].any()


@pytest.mark.parametrize("store", cases.STORES)
@pytest.mark.parametrize("case", sorted(RERANK))
def test_rerank_cases(case, store):
    ncand, k, d, nq, opt = RERANK[case]
    w = cases.rerank_world(case, store)
    cand = w["cand"]
    assert cand.shape == (nq, ncand) and (cand[-1] == -1).all() and (ncand > 64) == ("wide" in case)
    for metric in METRICS:
        wd, wi = cases.rerank_want(case, store, metric)
        assert wd.shape == (nq, k) and not np.isnan(wd).any()
        for i in range(nq):
            valid = cand[i][cand[i] >= 0]
            assert len(set(valid)) == len(valid)   # no candidate twice: (dist, id) never ties
            _total_order(wd[i][wi[i] >= 0], wi[i][wi[i] >= 0])
        assert (wi[:-1, :min(k, ncand - 2)] >= 0).all() and (wi[-1] == -1).all()
