"""Inputs for the search kernels at the shapes, plan sizes and list paths the other search tests
never reach (tests/test_search_shapes_cpu.py, tests/test_gpu_search_shapes.py), each with a
check_* function that asserts the properties its case relies on.  Nothing here calls the
library.

The references are the ones the neighbouring files pin to the definition, all general in m and
K: ivf_residual_ref.adc / search (brute force over a query's ranges, fp32 parts summed left to
right, np.lexsort((rows, dist))), search_lists_ref.search / probe_ranges / invert, and want()
below, the plain search of tests/test_gpu_search.py restated."""
import numpy as np

import datagen
import ivf_ref
import ivf_residual_ref as ref
import search_lists_ref as lref

ROUND = 1024          # the ranges (scan_plan) or lists (lists_plan) of one round of a plan kernel
LANES = 64            # a step is up to 64 chunks; an offer is 64 candidates, one per lane
SERIAL_MAX = 6        # list_offer: up to six passing lanes are inserted one by one


# ------------------------------------------------------------------------------ the plain search
def dists(lut, codes):
    """[nq][n] float32, parts added left to right"""
    out = np.empty((lut.shape[0], codes.shape[0]), np.float32)
    for q in range(lut.shape[0]):
        out[q] = ref.adc(lut[q], codes)
    return out


def want(lut, codes, k, id_base=0):
    """the top k of all rows by (dist, id), padded with (+inf, -1)"""
    d = dists(lut, codes)
    wd = np.full((lut.shape[0], k), np.inf, np.float32)
    wi = np.full((lut.shape[0], k), -1, np.int64)
    ids = np.arange(codes.shape[0], dtype=np.int64)
    for q in range(lut.shape[0]):
        order = np.lexsort((ids, d[q]))[:k]
        wd[q, :len(order)] = d[q, order]
        wi[q, :len(order)] = ids[order] + id_base
    return wd, wi


def head(w, k):
    """the result for a smaller k is the head of every row (the order is total)"""
    return w[0][:, :k], w[1][:, :k]


# ------------------------------------------------------------------------------ the shape sweep
MS = (1, 2, 5, 8, 9, 12, 15, 16)
KS = (2, 5, 16, 100, 256)
SHAPES = ([(m, 256) for m in MS] + [(m, K) for m in (5, 12) for K in KS if K != 256] +
          [(8, 16), (16, 16), (3, 5), (1, 2)])
CHUNKS = (1, 7, 64)
TOP_KS = (1, 2, 7, 33, 63, 64)
NQ, NPROBE = lref.NQ, lref.NPROBE


def qb_of(m, K):
    """the query tables of a workgroup (scan_launch): eight when m <= 8 and they fit 64 KB"""
    return 8 if m <= 8 and m * K <= 2048 else 4


def walk_of(m, aligned=True):
    """the row's u64 words of the packed walk (search_stream, search_codes), 0: the byte-wise
    one.  aligned: the chunk contexts of a stream start on an 8-byte boundary."""
    return m // 8 if m in (8, 16) and aligned else 0


def check_shapes():
    """the subset the sweep takes, and the instantiations (walk, tables) it selects"""
    assert all((m, 256) in SHAPES for m in MS)
    assert all((m, K) in SHAPES for m in (5, 12) for K in KS)
    assert all(s in SHAPES for s in ((8, 16), (16, 16), (3, 5), (1, 2)))
    assert len(SHAPES) == len(set(SHAPES)) == 20
    forms = {(walk_of(m), qb_of(m, K)) for m, K in SHAPES}
    assert forms == {(0, 8), (0, 4), (1, 8), (2, 4)}
    assert {m for m, K in SHAPES if (walk_of(m), qb_of(m, K)) == (0, 4)} == {9, 12, 15}
    assert {m for m, K in SHAPES if (walk_of(m), qb_of(m, K)) == (0, 8)} == {1, 2, 3, 5}
    # the scalar table load of the per-range form, and tables that are no multiple of 16 bytes
    assert any((m * K) % 4 for m, K in SHAPES)
    assert sum((m * K * 4) % 16 != 0 for m, K in SHAPES) >= 3
    assert {K for m, K in SHAPES} == set(KS)


def sweep_case(m, K, chunk, seed):
    """search_lists_ref.sweep_case with K symbols a part: (codes, offsets, probes,
    lut_q [NQ][m][K], lut_pair [NQ * NPROBE][m][K])"""
    offsets = np.concatenate([[0], np.cumsum(lref.list_sizes(chunk))]).astype(np.int64)
    codes = datagen.skewed_codes(int(offsets[-1]), m, k=K, seed=seed)
    for l in (3, 6):
        codes[offsets[l]:offsets[l] + 20] = codes[:20]
    probes = np.array(lref.PROBES, np.int64)
    rng = np.random.default_rng(seed + 1)
    whole = rng.integers(0, 3, size=(m, K)).astype(np.float32)
    lut_q = rng.normal(0.0, 100.0, size=(NQ, m, K)).astype(np.float32)
    lut_pair = rng.normal(0.0, 100.0, size=(NQ * NPROBE, m, K)).astype(np.float32)
    for q in lref.SHARED:
        lut_q[q] = whole
        lut_pair[q * NPROBE:(q + 1) * NPROBE] = whole
    lut_pair[lref.probe_ranges(offsets, probes)[1][:, 1] == 0] = np.nan
    return codes, offsets, probes, lut_q, lut_pair


def check_sweep_case(m, K, chunk, case):
    codes, offsets, probes, lut_q, lut_pair = case
    lref.check_sweep_inputs(chunk, offsets, probes, m)
    assert probes.shape == (NQ, NPROBE)
    assert codes.dtype == np.uint8 and codes.shape == (offsets[-1], m) and codes.max() < K
    # every part uses more than one symbol, some part the last one: the stride i * K + c
    # and the clamp at K - 1 both matter
    assert all(len(np.unique(codes[:, i])) > 1 for i in range(m))
    assert K > 100 or codes.max() == K - 1
    assert lut_q.shape == (NQ, m, K) and lut_pair.shape == (NQ * NPROBE, m, K)
    ranges = lref.probe_ranges(offsets, probes)[1]
    assert np.isnan(lut_pair[ranges[:, 1] == 0]).all() and not np.isnan(lut_q).any()
    assert not np.isnan(lut_pair[ranges[:, 1] > 0]).any()


def sweep_want(case, k=64):
    """(plain, per query, per pair): the plain search of all rows with lut_q, the probe search
    with a table per query and with one per pair"""
    codes, offsets, probes, lut_q, lut_pair = case
    ptr, ranges = lref.probe_ranges(offsets, probes)
    return (want(lut_q, codes, k),
            ref.search(np.repeat(lut_q, NPROBE, axis=0), codes, k, ptr, ranges),
            ref.search(lut_pair, codes, k, ptr, ranges))


# ------------------------------------------------------------------------------ the plans
def prefix(counts, carry=True):
    """the exclusive prefix of counts as a plan kernel computes it, ROUND entries a round;
    carry=False: what it would give if the sum of the rounds before were dropped"""
    counts = np.asarray(counts, np.int64)
    out = np.zeros(len(counts) + 1, np.int64)
    out[1:] = np.cumsum(counts)
    if not carry:
        for base in range(ROUND, len(counts) + 1, ROUND):
            out[base:base + ROUND] -= out[base]
    return out


def range_steps(ranges, n, C, L=LANES):
    """scan_plan's steps of every range: ceil(its chunks / L), none for an empty or a bad one"""
    f, c = ranges[:, 0], ranges[:, 1]
    good = (f >= 0) & (c > 0) & (f <= n) & (c <= n - f)
    last = np.where(good, f + c - 1, 0)
    return np.where(good, (last // C - np.where(good, f, 0) // C + L) // L, 0)


RANGES_N, RANGES_C = 3001, 4
EMPTY_AT, BAD_AT = (3, 100, 511), (5, 200, 777)          # offsets inside every round
QUERY_CUTS = (0, 40, 700, 700, 1000, 1030, 1500, 2047, 2049, 2060, 2100)


def ranges_case(nr, seed, m=8, K=16):
    """nr ranges over RANGES_N rows in chunks of RANGES_C: mostly 1-12 rows, every 301st longer
    than 64 chunks, empty ones (EMPTY_AT) in every round, ranges with rows on both sides of
    every round boundary.  Returns dict(codes, ptr, ranges, bad, lut_q, lut_r): bad is ranges
    with an out-of-bounds range at BAD_AT of every round; the queries' spans are QUERY_CUTS up
    to nr (one of them empty), lut_q a table per query and lut_r one per range."""
    n, C = RANGES_N, RANGES_C
    rng = np.random.default_rng(seed)
    ranges = np.stack([rng.integers(0, n - 12, size=nr), rng.integers(1, 13, size=nr)], axis=1)
    for r in range(7, nr, 301):
        ranges[r] = rng.integers(0, n - 700), LANES * C + rng.integers(2, 300)
    for base in range(0, nr, ROUND):
        for o in EMPTY_AT:
            if base + o < nr:
                ranges[base + o, 1] = 0
        if base + EMPTY_AT[1] < nr:
            ranges[base + EMPTY_AT[1], 0] = n            # (n, 0): empty, not bad
    for b in range(ROUND, nr + 1, ROUND):
        ranges[b - 1] = 17 + b // ROUND, 5
        if b < nr:
            ranges[b] = 1200 + b // ROUND, 6
    ranges = ranges.astype(np.int64)
    bad = ranges.copy()
    kinds = [(-3, 4), (n - 2, 10), (4, -1), (n + 1, 0), (5, 2 ** 62)]
    at = 0
    for base in range(0, nr, ROUND):
        for o in BAD_AT:
            if base + o < nr:
                bad[base + o] = kinds[at % len(kinds)]
                at += 1
    cuts = [c for c in QUERY_CUTS if c < nr] + [nr]
    ptr = np.array(cuts, np.int64)
    nq = len(ptr) - 1
    return dict(codes=datagen.skewed_codes(n, m, k=K, seed=seed + 1), ptr=ptr, ranges=ranges,
                bad=bad, n=n, C=C,
                lut_q=rng.normal(0.0, 100.0, size=(nq, m, K)).astype(np.float32),
                lut_r=rng.normal(0.0, 100.0, size=(nr, m, K)).astype(np.float32))


def per_range(lut_q, ptr, nr):
    """the table of every range's query, for ivf_residual_ref.search"""
    owner = np.searchsorted(ptr[1:], np.arange(nr), side="right")
    return lut_q[np.minimum(owner, len(lut_q) - 1)]


def check_ranges_case(nr, case):
    ptr, ranges, bad, n, C = (case[key] for key in ("ptr", "ranges", "bad", "n", "C"))
    assert ranges.shape == bad.shape == (nr, 2) and ptr[0] == 0 and ptr[-1] == nr
    assert (np.diff(ptr) >= 0).all() and (np.diff(ptr) == 0).any()      # a query with no range
    ok = lambda r: (r[:, 0] >= 0) & (r[:, 1] >= 0) & (r[:, 0] <= n) & (r[:, 1] <= n - r[:, 0])
    assert ok(ranges).all()
    steps = range_steps(ranges, n, C)
    for base in range(0, nr, ROUND):
        here = slice(base, min(base + ROUND, nr))
        if nr - base > BAD_AT[-1]:                       # (the one-entry round of nr = 1,025
            assert (ranges[here, 1] == 0).sum() == 3     #  is the range after the boundary)
            assert (~ok(bad[here])).sum() == 3
            assert (steps[here] >= 2).any() and (steps[here] == 1).any()
    # bad differs from ranges at the bad entries alone, and none of them was an empty one
    differ = np.flatnonzero((bad != ranges).any(axis=1))
    assert len(differ) and (~ok(bad[differ])).all() and (ranges[differ, 1] > 0).all()
    assert np.array_equal(range_steps(bad, n, C)[ok(bad)], steps[ok(bad)])
    assert (range_steps(bad, n, C)[~ok(bad)] == 0).all()
    # rows directly before and after every round boundary
    for b in range(ROUND, nr + 1, ROUND):
        assert ranges[b - 1, 1] > 0 and (b == nr or ranges[b, 1] > 0)
    spans = list(zip(ptr[:-1], ptr[1:]))
    if nr > ROUND:
        assert any(lo < ROUND < hi for lo, hi in spans)                  # straddles entry 1,024
    if nr > 2 * ROUND:
        assert any(lo < 2 * ROUND < hi for lo, hi in spans)
        assert sum(lo >= 2 * ROUND and hi > lo for lo, hi in spans) >= 2   # inside the third round
    return steps


def check_ranges_carry(nr, case):
    """the plan with the carry between rounds dropped differs from the plan, at a range with
    rows and at the first range of some query: a kernel without the carry could not pass"""
    for ranges in (case["ranges"], case["bad"]):
        steps = range_steps(ranges, case["n"], case["C"])
        good, broken = prefix(steps), prefix(steps, carry=False)
        assert good[-1] == steps.sum() and (np.diff(good) == steps).all()
        assert np.array_equal(good[:ROUND], broken[:ROUND])
        if nr <= ROUND:
            assert np.array_equal(good[:nr], broken[:nr])     # one round: nothing to carry
            continue
        differ = good != broken
        assert differ[ROUND:].all() and not differ[:ROUND].any()
        assert (steps[ROUND:] > 0).any()
        # a query with ranges whose span of the plan begins or ends in a later round
        spans = [(lo, hi) for lo, hi in zip(case["ptr"][:-1], case["ptr"][1:]) if hi > lo]
        assert any(lo < ROUND <= hi for lo, hi in spans)
        if nr > 2 * ROUND:
            assert any(lo >= ROUND and differ[lo] for lo, hi in spans)
            assert any(lo >= 2 * ROUND and differ[lo] for lo, hi in spans)


LISTS_C = 4


def lists_case(nlist, m, seed, nq=24, nprobe=6):
    """nlist lists over about 5,000 rows in chunks of LISTS_C: mostly 0-8 rows, up to three
    long ones (the hot lists: list 5, one in the middle of the second round, one 30 into the
    third, where there are such rounds; the last of them longer than 64 chunks), and lists
    with rows on both sides of every round boundary.  Every hot list is probed by at least ten
    pairs.  Returns dict(codes, offsets, probes, hot, lut_q, lut_pair) with K = 256."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(0, 9, size=nlist) * (rng.random(nlist) < min(1.0, 4400 / (4.0 * nlist)))
    hot = [5]
    if nlist > ROUND:
        hot.append(ROUND + (nlist - ROUND) // 2)
    if nlist > 2 * ROUND + 30:
        hot.append(2 * ROUND + 30)
    for l, size in zip(hot, (70, 150, 150)):
        sizes[l] = size
    sizes[hot[-1]] = 64 * LISTS_C + 44                   # the last hot list: more than one step
    for b in range(ROUND, nlist + 1, ROUND):
        sizes[b - 1] = max(sizes[b - 1], 3)
        if b < nlist:
            sizes[b] = max(sizes[b], 2)
    sizes[7] = 0                                         # an empty list that is probed
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(offsets[-1])
    probes = rng.integers(0, nlist, size=(nq, nprobe)).astype(np.int64)
    probes[rng.random((nq, nprobe)) < 0.1] = -1
    for i, l in enumerate(hot):
        probes[4 * i:4 * i + 10, i] = l                  # ten pairs each
    probes[20:, 4] = hot[0]                              # (list 5: fourteen)
    probes[0, 5], probes[1, 5], probes[2, 5] = 7, -1, nlist - 1
    at = 12
    for b in range(ROUND, nlist + 1, ROUND):             # the lists at the round boundaries
        probes[at, 3] = b - 1
        probes[at + 1, 3] = min(b, nlist - 1)
        at += 2
    return dict(codes=datagen.skewed_codes(n, m, seed=seed + 1), offsets=offsets, probes=probes,
                hot=hot, n=n, C=LISTS_C,
                lut_q=rng.normal(0.0, 100.0, size=(nq, m, 256)).astype(np.float32),
                lut_pair=rng.normal(0.0, 100.0, size=(nq * nprobe, m, 256)).astype(np.float32))


def check_lists_case(nlist, m, case):
    offsets, probes, hot, n, C = (case[key] for key in ("offsets", "probes", "hot", "n", "C"))
    sizes = np.diff(offsets)
    assert len(sizes) == nlist and 3500 < n < 6500 and (sizes >= 0).all()
    assert np.median(sizes) <= 8 and (sizes == 0).sum() > nlist // 20
    assert len(hot) == (nlist + ROUND - 1) // ROUND          # one in every round
    pairs, bad = lref.invert(offsets, probes, n)
    assert not bad
    count = np.array([len(p) for p in pairs])
    qb = lref.qb_of(m)
    assert qb == qb_of(m, 256)
    for l in hot:
        assert count[l] >= 10 and -(-count[l] // qb) >= 2      # more than one unit
    f, c = offsets[hot[-1]], sizes[hot[-1]]
    assert (f + c - 1) // C - f // C + 1 > LANES                 # more than one step
    flat = probes.reshape(-1)
    assert (flat == -1).any() and sizes[7] == 0 and (flat == 7).any()
    for base in range(0, nlist, ROUND):                          # probes reach every round
        assert (count[base:base + ROUND] > 0).any()
    for b in range(ROUND, nlist + 1, ROUND):
        assert count[b - 1] > 0 and (b == nlist or count[b] > 0)
    return count


def check_lists_carry(nlist, m, case):
    """lists_plan's two prefixes (the pairs and the units of every list) with the carry between
    rounds dropped differ from the right ones at lists that have pairs"""
    count = check_lists_case(nlist, m, case)
    units = -(-count // qb_of(m, 256))
    for per_list in (count, units):
        good, broken = prefix(per_list), prefix(per_list, carry=False)
        assert np.array_equal(good[:ROUND], broken[:ROUND])
        if nlist <= ROUND:
            continue
        later = np.arange(nlist) >= ROUND
        assert (good[:nlist] != broken[:nlist])[later].all()
        assert (count[later] > 0).any()
        for l in case["hot"][1:]:
            assert good[l] != broken[l]
    # units and pairs carry differently: a unit is not a pair
    assert prefix(units)[-1] < prefix(count)[-1]
    return prefix(count), prefix(units)


def coarse_case(seed, nlist=1025, d=16, n=5000, nq=16, nprobe=5, m=8):
    """a coarse codebook of nlist centroids and queries near some of them -- the last list,
    the only one of the second round, among them -- with the rows' layout from numpy"""
    rng = np.random.default_rng(seed)
    cc = rng.normal(0.0, 10.0, size=(nlist, d)).astype(np.float32)
    x = (cc[rng.integers(0, nlist, size=n)] + rng.normal(0.0, 2.0, size=(n, d))).astype(np.float32)
    x[:6] = cc[nlist - 1] + rng.normal(0.0, 0.5, size=(6, d)).astype(np.float32)
    lists, _ = ivf_ref.assign(x, cc)
    _, offsets = ivf_ref.layout(lists, nlist)
    near = np.concatenate([[nlist - 1, nlist - 1, 0, ROUND - 1], rng.integers(0, nlist, size=nq - 4)])
    q = (cc[near] + rng.normal(0.0, 1.0, size=(nq, d))).astype(np.float32)
    ptr, ranges, probes, _ = ivf_ref.probe(q, cc, nprobe, offsets)
    return dict(cc=cc, q=q, offsets=offsets, ptr=ptr, ranges=ranges, probes=probes, n=n,
                codes=datagen.skewed_codes(n, m, seed=seed + 1),
                lut_q=rng.normal(0.0, 100.0, size=(nq, m, 256)).astype(np.float32))


def check_coarse_case(case):
    nlist = len(case["cc"])
    assert nlist == ROUND + 1 and case["offsets"][-1] == case["n"]
    probes = case["probes"]
    assert (probes[:2, 0] == nlist - 1).all() and (probes >= 0).all()
    assert case["offsets"][nlist] - case["offsets"][nlist - 1] >= 6
    count = np.array([len(p) for p in lref.invert(case["offsets"], probes, case["n"])[0]])
    assert count[nlist - 1] >= 2 and (count[:ROUND] > 0).sum() > 20
    ptr, ranges = lref.probe_ranges(case["offsets"], probes)
    assert np.array_equal(ptr, case["ptr"]) and np.array_equal(ranges, case["ranges"])


# ------------------------------------------------------------------------------ the offer boundary
OFFER_J = (0, 1, 6, 7, 63, 64)
OFFER_TOP_KS = (1, 3, 10, 64)
OFFER_ORDERS = ("ascending", "descending", "shuffled")
FAIL = np.float32(5000.0)


def offer_codes(n, m, seed):
    """code[0] = the row, the other parts anything: with a table whose parts 1 ... m - 1 are
    zero, row r's distance is lut[0][r]"""
    codes = datagen.skewed_codes(n, m, seed=seed)
    codes[:, 0] = np.arange(n)
    return codes


def _passing(rng, j, order, values, fail=FAIL):
    """[64] float32: `values` (ascending, j of them) on j lanes in `order` by lane, fail + lane
    on the others"""
    lanes = np.sort(rng.choice(LANES, size=j, replace=False))
    values = np.asarray(values, np.float32)
    if order == "descending":
        values = values[::-1]
    elif order == "shuffled":
        values = rng.permutation(values)
    out = fail + np.arange(LANES, dtype=np.float32)
    out[lanes] = values
    return out


def offer_table(n, m, top_k, j, order, seed):
    """[1][m][256]: rows 0-63 get 1000 + 10 * a permutation of 0 ... 63 (the list after them
    holds the top_k smallest, threshold T = 1000 + 10 * (top_k - 1)); of rows 64-127 exactly j
    beat T, with values T - 5, T - 15, ... that fall between the list's entries; n = 256: of
    rows 128-191 none does, and of rows 192-255 again j, all below everything before"""
    rng = np.random.default_rng(seed)
    row = np.zeros(256, np.float32)
    row[:LANES] = 1000 + 10 * rng.permutation(LANES)
    t = 1000 + 10 * (top_k - 1)
    row[LANES:2 * LANES] = _passing(rng, j, order, t - 5 - 10 * np.arange(j)[::-1])
    if n > 2 * LANES:
        row[2 * LANES:3 * LANES] = 2 * FAIL + np.arange(LANES)
        row[3 * LANES:4 * LANES] = _passing(rng, j, order, -1000 + 10 * np.arange(j), 3 * FAIL)
    lut = np.zeros((1, m, 256), np.float32)
    lut[0, 0] = row
    return lut


def offers_passing(dist, top_k):
    """how many candidates of every offer of 64 rows precede the list's threshold (its entry
    top_k - 1, +inf while it has fewer) when the offer comes"""
    held = np.zeros(0, np.int64)                         # the rows of the list
    counts = []
    ids = np.arange(len(dist), dtype=np.int64)
    for base in range(0, len(dist), LANES):
        rows = ids[base:base + LANES]
        if len(held) < top_k:
            counts.append(len(rows))
        else:
            td, tid = dist[held[top_k - 1]], held[top_k - 1]
            counts.append(int(((dist[rows] < td) | ((dist[rows] == td) & (rows < tid))).sum()))
        both = np.concatenate([held, rows])
        held = both[np.lexsort((both, dist[both]))][:LANES]
    return counts


def check_offer_case(n, codes, lut, top_k, j, order):
    assert n in (2 * LANES, 4 * LANES) and codes.shape[0] == n
    assert np.array_equal(codes[:, 0], np.arange(n)) and not lut[0, 1:].any()
    dist = ref.adc(lut[0], codes)
    assert np.array_equal(dist, lut[0, 0, :n]) and len(np.unique(dist)) == n
    assert offers_passing(dist, top_k) == [LANES, j] + ([0, j] if n == 4 * LANES else [])
    for base in range(LANES, n, 2 * LANES):
        d = dist[base:base + LANES]
        mine = d[d < FAIL]
        assert len(mine) == j
        if order == "ascending":
            assert (np.diff(mine) > 0).all()
        elif order == "descending":
            assert (np.diff(mine) < 0).all()
        elif j > 6:
            assert (np.diff(mine) > 0).any() and (np.diff(mine) < 0).any()
    # on both sides of the boundary between serial inserts and the merge network
    assert SERIAL_MAX in OFFER_J and SERIAL_MAX + 1 in OFFER_J
