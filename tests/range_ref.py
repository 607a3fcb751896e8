"""Inputs and the numpy reference of the range search (pqh_range_count_*, pqh_range_fill_*,
codec.range_search*, codec.IVF.range_search), shared by tests/test_range_cpu.py and
tests/test_gpu_range.py, each input with a check_* function that asserts the properties its case
relies on.  Nothing here calls the library.

A result is every scanned row with dist < radius[q] (strict; a NaN on either side is no hit), dist
ivf_residual_ref.adc's sum, in scan order: ascending row for the whole stream, range by range in
the order of the query's list and ascending row inside a range for the probe forms.  The output
is CSR: lims int64 [nq + 1], dist float32 and ids int64 [lims[nq]]."""
import numpy as np

import ivf_residual_ref as ref
import search_filter_ref as fref
import search_lists_ref as lref
import search_shapes_ref as sref

N, NQ = fref.N, fref.NQ
MODES = fref.MODES
CHUNKS = (1, 7, 64)           # 16 steps of 64 chunks, three, one
LUT_SEED = 7
KINDS = ("neg_inf", "pos_inf", "nan", "min", "d10", "d10_next", "median", "max_next")
GROUPS = (1, 3, 0)            # search_groups: one workgroup a batch, three, the default


def lut_of(mode):
    return fref.lut_of(NQ, MODES[mode][0], LUT_SEED)


def _below(dist, r):
    with np.errstate(invalid="ignore"):
        return dist < r


def _csr(per_query):
    lims = np.zeros(len(per_query) + 1, np.int64)
    lims[1:] = np.cumsum([len(d) for d, _ in per_query])
    dist = np.concatenate([d for d, _ in per_query] + [np.zeros(0, np.float32)]).astype(np.float32)
    ids = np.concatenate([i for _, i in per_query] + [np.zeros(0, np.int64)]).astype(np.int64)
    return lims, dist, ids


def want(d, radius, keep=None, id_base=0):
    """(lims, dist, ids) of the whole-stream form: d float32 [nq][n] (search_shapes_ref.dists),
    radius float32 [nq], keep a bool per row or None"""
    rows = np.arange(d.shape[1], dtype=np.int64)
    if keep is not None:
        rows = rows[np.asarray(keep, bool)]
    out = []
    for q in range(d.shape[0]):
        hit = _below(d[q, rows], radius[q])
        out.append((d[q, rows][hit], rows[hit] + id_base))
    return _csr(out)


def want_ranges(lut, codes, ptr, ranges, radius, keep=None, id_base=0):
    """(lims, dist, ids) of the probe forms, lut one table per range [nr][m][K] (np.repeat a
    table per query): the loop of ivf_residual_ref.search without its sort.  A range that
    leaves [0, n] is skipped, a query whose ptr pair is reversed or leaves [0, nr] has none."""
    n = codes.shape[0]
    nq, nr = len(ptr) - 1, len(ranges)
    out = []
    for q in range(nq):
        rows, dist = [np.zeros(0, np.int64)], [np.zeros(0, np.float32)]
        if 0 <= ptr[q] <= ptr[q + 1] <= nr:
            for r in range(ptr[q], ptr[q + 1]):
                f, c = int(ranges[r][0]), int(ranges[r][1])
                if not (0 <= f <= n and 0 <= c <= n - f):
                    continue
                rr = np.arange(f, f + c, dtype=np.int64)
                if keep is not None:
                    rr = rr[keep[rr]]
                dd = ref.adc(lut[r], codes[rr])
                hit = _below(dd, radius[q])
                rows.append(rr[hit])
                dist.append(dd[hit])
        out.append((np.concatenate(dist), np.concatenate(rows) + id_base))
    return _csr(out)


def prefix(w, capacity):
    """what a fill into buffers of `capacity` entries leaves: lims as they are, the first
    `capacity` entries"""
    return w[0], w[1][:capacity], w[2][:capacity]


# ------------------------------------------------------------------------------ the radii
def radii(d):
    """kind -> float32 [nq], and "mixed": query q takes kind q % 8 -- every kind in one call"""
    nq = d.shape[0]
    up = np.float32(np.inf)
    d10 = np.array([np.unique(d[q])[9] for q in range(nq)], np.float32)
    out = {"neg_inf": np.full(nq, -np.inf, np.float32), "pos_inf": np.full(nq, np.inf, np.float32),
           "nan": np.full(nq, np.nan, np.float32), "min": d.min(axis=1), "d10": d10,
           "d10_next": np.nextafter(d10, up), "median": np.sort(d, axis=1)[:, d.shape[1] // 2],
           "max_next": np.nextafter(d.max(axis=1), up)}
    assert tuple(out) == KINDS and all(v.dtype == np.float32 for v in out.values())
    out["mixed"] = np.array([out[KINDS[q % len(KINDS)]][q] for q in range(nq)], np.float32)
    return out


def counts(w):
    return np.diff(w[0])


def check_radii(mode, d, rad):
    """the table of the issue: the hits of every kind of radius on the data of `mode`"""
    assert d.shape == (NQ, N) and np.isfinite(d).all()
    got = {kind: counts(want(d, rad[kind])) for kind in rad}
    assert (got["neg_inf"] == 0).all() and (got["nan"] == 0).all() and (got["min"] == 0).all()
    assert (got["pos_inf"] == N).all() and (got["max_next"] == N).all()
    # nine distinct distances below the tenth: nine rows, and one more for every row that
    # repeats one of them.  Only the three-part codes have such rows (query 0 among them).
    ties = np.array([(np.sort(d[q]) < rad["d10"][q]).sum() - 9 for q in range(NQ)])
    if mode == "noctx_m3":
        assert ties[0] == 1 and set(ties) == {0, 1}
    else:
        assert not ties.any()
    assert np.array_equal(got["d10"], 9 + ties)
    # the next float above it takes in the rows at d10 itself: one, but for a three-part row
    # that repeats
    at = np.array([(d[q] == rad["d10"][q]).sum() for q in range(NQ)])
    assert (at == 1).all() or (mode == "noctx_m3" and at.min() == 1)
    assert np.array_equal(got["d10_next"], got["d10"] + at)
    assert (got["median"] == N // 2).all()
    ids = want(d, rad["median"])[2]
    assert (ids == 0).any() and (ids == N - 1).any()
    assert np.array_equal(got["mixed"], [got[KINDS[q % len(KINDS)]][q] for q in range(NQ)])
    assert len(set(got["mixed"])) >= 5


def ties_case():
    """(codes, lut, d): search_filter_ref.ties_lut on the codes of ctx_m8 -- small integers"""
    codes = fref.codes_of("ctx_m8")
    lut = fref.ties_lut(NQ, 8, 9)
    return codes, lut, sref.dists(lut, codes)


def check_ties(d):
    """150 to 195 rows a query at 8.0 (154 ... 193): none of them below 8.0, all of them below
    8.5"""
    at = (d == 8.0).sum(axis=1)
    assert (at >= 150).all() and (at <= 195).all()
    a = want(d, np.full(NQ, 8.0, np.float32))
    b = want(d, np.full(NQ, 8.5, np.float32))
    assert not (a[1] == 8.0).any() and np.array_equal(counts(b) - counts(a), at)
    for q in range(NQ):
        assert (b[1][b[0][q]:b[0][q + 1]] == 8.0).sum() == at[q]


def check_order(w, keep=None):
    """ascending rows per query, every one kept"""
    for q in range(len(w[0]) - 1):
        ids = w[2][w[0][q]:w[0][q + 1]]
        assert (np.diff(ids) > 0).all()
        assert keep is None or keep[ids].all()


# ------------------------------------------------------------------------------ the probe forms
REPEAT_Q, REPEAT_LIST = 4, 3          # search_lists_ref.PROBES: query 4 probes list 3 twice
BAD_Q = 2


def probe_case(m, K, chunk):
    """search_shapes_ref.sweep_case as the filtered search's tests take it, with the probe list"""
    case = sref.sweep_case(m, K, chunk, seed=40 + m + chunk)
    ptr, ranges = lref.probe_ranges(case[1], case[2])
    return case, ptr, ranges


def probe_luts(case):
    """(a table per range from the queries' tables, the pairs' tables with their NaN ones)"""
    return np.repeat(case[3], sref.NPROBE, axis=0), case[4]


def probe_radii(lut, codes, ptr, ranges):
    """name -> float32 [nq]: +inf, and per query the median of the distances it scans (0 for a
    query without rows)"""
    everything = want_ranges(lut, codes, ptr, ranges, np.full(len(ptr) - 1, np.inf, np.float32))
    med = np.zeros(len(ptr) - 1, np.float32)
    for q in range(len(med)):
        dd = everything[1][everything[0][q]:everything[0][q + 1]]
        if len(dd):
            med[q] = np.sort(dd)[len(dd) // 2]
    return {"pos_inf": np.full(len(med), np.inf, np.float32), "median": med}


def check_probe_case(case, ptr, ranges):
    codes, offsets, probes = case[0], case[1], case[2]
    assert (probes[REPEAT_Q] == REPEAT_LIST).sum() == 2
    size = offsets[REPEAT_LIST + 1] - offsets[REPEAT_LIST]
    rows = np.arange(offsets[REPEAT_LIST], offsets[REPEAT_LIST + 1])
    for lut in probe_luts(case):
        rad = probe_radii(lut, codes, ptr, ranges)
        w = want_ranges(lut, codes, ptr, ranges, rad["pos_inf"])
        ids = w[2][w[0][REPEAT_Q]:w[0][REPEAT_Q + 1]]
        at = np.flatnonzero(ids == rows[0])
        assert len(at) == 2 and all(np.array_equal(ids[a:a + size], rows) for a in at)
        c = counts(w)
        assert (c == 0).any() and (c > 64 * 7).any()          # nothing at all; more than a step
        half = counts(want_ranges(lut, codes, ptr, ranges, rad["median"]))
        assert ((half > 0) & (half < c)).any()
        # a NaN table (a pair without rows) gives no hit and spoils none
        assert not np.isnan(w[1]).any()


def bad_ranges(ranges, ptr, n):
    """the first range of query BAD_Q leaves the rows"""
    out = ranges.copy()
    out[ptr[BAD_Q]] = (n - 1, 5)
    return out


# ------------------------------------------------------------------------------ the index
def ivf_radii(w, kind):
    """float32 [nq]: per query the distance at a rank of its scanned rows -- 0, 1, 10, 63, 64,
    65, 150, the middle, the last: results shorter and longer than a top-64 list"""
    inf = np.full(fref.IVF_NQ, np.inf, np.float32)
    every = want_ranges(w[kind]["lut"], w[kind]["codes"], w["ptr"], w["ranges"], inf)
    rad = np.zeros(fref.IVF_NQ, np.float32)
    for q in range(fref.IVF_NQ):
        dd = np.sort(every[1][every[0][q]:every[0][q + 1]])
        rank = (0, 1, 10, 63, 64, 65, 150, len(dd) // 2, len(dd) - 1)[q]
        rad[q] = dd[min(rank, len(dd) - 1)]
    return rad


def ivf_want(w, kind, radius, keep=None, removed=None):
    """(lims, dist, caller ids) of IVF.range_search: keep a bool over the caller's rows or None,
    removed the caller rows taken out"""
    ok = np.ones(fref.IVF_N, bool) if keep is None else np.asarray(keep, bool).copy()
    if removed is not None:
        ok[removed] = False
    lims, dist, rows = want_ranges(w[kind]["lut"], w[kind]["codes"], w["ptr"], w["ranges"], radius,
                                   keep=ok[w["perm"]])
    return lims, dist, w["perm"][rows]


def check_ivf(w):
    for kind in ("plain", "residual"):
        rad = ivf_radii(w, kind)
        c = counts(ivf_want(w, kind, rad))
        assert c[0] == 0 and (c[:3] < 64).all() and (c[5:] > 64).all() and c[4] >= 64
        kept = counts(ivf_want(w, kind, rad, w["keep"]))
        assert (kept <= c).all() and (kept < c).any() and kept.sum() > 0


def topk_of(w3, inv, k=64):
    """per query the first k of a range result sorted by (dist, stream row), the order of
    IVF.search: (dist, ids) lists.  inv: caller row -> stream row.  (A stable sort by the
    distance alone keeps rows of one distance in probe order, which is the order of the stream
    inside a list only: query 7 of the plain index has four rows of one distance in lists that
    it probes in another order than the stream holds them.)"""
    out = []
    for q in range(len(w3[0]) - 1):
        d, i = w3[1][w3[0][q]:w3[0][q + 1]], w3[2][w3[0][q]:w3[0][q + 1]]
        order = np.lexsort((inv[i], d))[:k]
        out.append((d[order], i[order]))
    return out


def inverse(perm):
    inv = np.empty(len(perm), np.int64)
    inv[perm] = np.arange(len(perm))
    return inv
