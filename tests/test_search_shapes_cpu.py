"""The inputs of tests/test_gpu_search_shapes.py have the properties that file relies on
(every check_* of tests/search_shapes_ref.py), and the references it compares with give, at the
new shapes, what the search is defined to give: brute force over all rows of a query's ranges,
fp32 parts summed left to right, np.lexsort((rows, dist)).  No GPU, no library call."""
import numpy as np
import pytest

import ivf_residual_ref as ref
import search_lists_ref as lref
import search_shapes_ref as sref


def _bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


def _equal(a, b, what=""):
    assert np.array_equal(a[1], b[1]), what
    assert np.array_equal(_bits(a[0]), _bits(b[0])), what


def _brute(tables, codes, k, ptr, ranges):
    """the definition, row by row: every row of every good range of a query, its table's
    entries added left to right in float32, the k first by (dist, row)"""
    n, m = codes.shape
    nq = len(ptr) - 1
    wd = np.full((nq, k), np.inf, np.float32)
    wi = np.full((nq, k), -1, np.int64)
    for q in range(nq):
        rows, dist = [], []
        for r in range(ptr[q], ptr[q + 1]):
            f, c = int(ranges[r, 0]), int(ranges[r, 1])
            if not (0 <= f <= n and 0 <= c <= n - f):
                continue
            for row in range(f, f + c):
                acc = tables[r][0][codes[row, 0]]
                for i in range(1, m):
                    acc = np.float32(acc + tables[r][i][codes[row, i]])
                rows.append(row)
                dist.append(acc)
        rows, dist = np.array(rows, np.int64), np.array(dist, np.float32)
        order = np.lexsort((rows, dist))[:k]
        wd[q, :len(order)] = dist[order]
        wi[q, :len(order)] = rows[order]
    return wd, wi


def test_the_sweep_takes_the_subset_and_reaches_every_walk():
    sref.check_shapes()
    assert sref.qb_of(8, 256) == 8 and sref.qb_of(9, 2) == 4 and sref.qb_of(16, 16) == 4
    assert sref.walk_of(8) == 1 and sref.walk_of(16) == 2
    assert sref.walk_of(8, aligned=False) == 0 and sref.walk_of(16, aligned=False) == 0


@pytest.mark.parametrize("m,K", sref.SHAPES)
def test_sweep_inputs(m, K):
    for chunk in sref.CHUNKS:
        sref.check_sweep_case(m, K, chunk, sref.sweep_case(m, K, chunk, 100 * m + K + chunk))


@pytest.mark.parametrize("m,K,chunk", [(5, 5, 7), (12, 256, 1), (3, 5, 1)])
def test_sweep_references_are_the_definition(m, K, chunk):
    """K = 5 and m = 12: the references the GPU sweep uses against the row-by-row brute force,
    and against the list-major restatement"""
    case = sref.sweep_case(m, K, chunk, 100 * m + K + chunk)
    codes, offsets, probes, lut_q, lut_pair = case
    ptr, ranges = lref.probe_ranges(offsets, probes)
    plain, by_query, by_pair = sref.sweep_want(case, 64)
    whole = np.array([[0, len(codes)]], np.int64)
    for q in (0, 6, sref.NQ - 1):
        one = _brute(lut_q[q:q + 1], codes, 64, np.array([0, 1]), whole)
        _equal(one, (plain[0][q:q + 1], plain[1][q:q + 1]), q)
    _equal(by_query, _brute(np.repeat(lut_q, sref.NPROBE, axis=0), codes, 64, ptr, ranges), "query")
    _equal(by_pair, _brute(lut_pair, codes, 64, ptr, ranges), "pair")
    for lut, w in ((lut_q, by_query), (lut_pair, by_pair)):
        for k in sref.TOP_KS:
            got = lref.search(lut, codes, k, offsets, probes)[:2]
            _equal(got, sref.head(w, k), k)
    assert (by_pair[1][5] == -1).all() and (by_pair[1][3] == -1).all() and not np.isnan(by_pair[0]).any()
    # a table read with another K's stride, or one symbol off, gives something else
    if m > 1:
        flat = lut_q.reshape(sref.NQ, -1)
        wrong = np.stack([np.roll(flat[q], 1) for q in range(sref.NQ)]).reshape(lut_q.shape)
        assert not np.array_equal(sref.want(wrong, codes, 64)[1][0], plain[1][0])


@pytest.mark.parametrize("nr", [1024, 1025, 2111])
def test_ranges_plan_inputs_and_the_dropped_carry(nr):
    case = sref.ranges_case(nr, nr)
    steps = sref.check_ranges_case(nr, case)
    sref.check_ranges_carry(nr, case)
    # the prefix restated in numpy twice, with and without the carry between rounds
    good, broken = sref.prefix(steps), sref.prefix(steps, carry=False)
    assert good[nr] == steps.sum() > nr // 2
    if nr > sref.ROUND:
        r = sref.ROUND + int(np.flatnonzero(steps[sref.ROUND:] > 0)[0])
        assert good[r] != broken[r] and case["ranges"][r, 1] > 0
        assert broken[sref.ROUND] == 0 and good[sref.ROUND] == steps[:sref.ROUND].sum() > 0


def test_ranges_reference_is_the_definition_past_two_rounds():
    """nr > 2,048: the per-query and the per-range table form, bad ranges skipped"""
    nr = 2111
    case = sref.ranges_case(nr, nr)
    tables = sref.per_range(case["lut_q"], case["ptr"], nr)
    owner = np.repeat(np.arange(len(case["ptr"]) - 1), np.diff(case["ptr"]))
    assert np.array_equal(_bits(tables), _bits(case["lut_q"][owner]))
    for ranges in (case["ranges"], case["bad"]):
        for lut in (tables, case["lut_r"]):
            _equal(ref.search(lut, case["codes"], 33, case["ptr"], ranges),
                   _brute(lut, case["codes"], 33, case["ptr"], ranges))
    # the bad ranges took rows away from some query
    a = ref.search(tables, case["codes"], 64, case["ptr"], case["ranges"])
    b = ref.search(tables, case["codes"], 64, case["ptr"], case["bad"])
    assert not np.array_equal(a[1], b[1])


@pytest.mark.parametrize("m", [8, 12])
@pytest.mark.parametrize("nlist", [1024, 1025, 2111])
def test_lists_plan_inputs_and_the_dropped_carry(nlist, m):
    case = sref.lists_case(nlist, m, nlist + m)
    pairs, units = sref.check_lists_carry(nlist, m, case)
    work = lref.units(lref.invert(case["offsets"], case["probes"], case["n"])[0], sref.qb_of(m, 256))
    assert len(work) == units[-1] and sum(len(b) for _, b in work) == pairs[-1]
    if nlist > sref.ROUND:
        # the first unit of the hot list of a later round: where the right prefix puts it
        for l in case["hot"][1:]:
            assert work[units[l]][0] == l and work[units[l] + 1][0] == l
            assert sref.prefix(np.diff(units), carry=False)[l] != units[l]
    if nlist == 2111 and m == 12:
        ptr, ranges = lref.probe_ranges(case["offsets"], case["probes"])
        for lut in (case["lut_q"], case["lut_pair"]):
            per = lut if len(lut) == len(ranges) else np.repeat(lut, case["probes"].shape[1], axis=0)
            want = ref.search(per, case["codes"], 7, ptr, ranges)
            _equal(want, _brute(per, case["codes"], 7, ptr, ranges))
            _equal(lref.search(lut, case["codes"], 7, case["offsets"], case["probes"])[:2], want)


def test_coarse_probe_inputs():
    sref.check_coarse_case(sref.coarse_case(1025))


@pytest.mark.parametrize("n", [128, 256])
def test_offer_inputs(n):
    """every (top_k, j, order): the counts of passing lanes offer by offer, and the order of
    the passing candidates by lane"""
    codes = sref.offer_codes(n, 8, n)
    seed = 0
    for top_k in sref.OFFER_TOP_KS:
        for j in sref.OFFER_J:
            for order in sref.OFFER_ORDERS:
                seed += 1
                lut = sref.offer_table(n, 8, top_k, j, order, seed)
                sref.check_offer_case(n, codes, lut, top_k, j, order)
                w = sref.want(lut, codes, top_k)
                if order == "ascending" and top_k == 1 and j > 0:
                    # the first passing lane is the best: every later one fails the re-filter
                    second = lut[0, 0, 64:128]
                    assert w[1][0, 0] == (64 + int(np.argmin(second)) if n == 128 else w[1][0, 0])
                    assert np.argmin(second) == np.flatnonzero(second < sref.FAIL)[0]
