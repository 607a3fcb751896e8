"""Inputs of the wide search (top_k and re-rank candidates in (64, 256] on a context whose limit
pqh_ctx_set_search_max_k raised), shared by tests/test_search_wide_cpu.py and
tests/test_gpu_search_wide.py, each with a check_* function that asserts the properties its
case relies on.  Nothing here calls the library.

The references are the existing ones, which take any k: search_filter_ref.want (the plain
search), ivf_residual_ref.search and search_lists_ref.search (the probe forms), refine_ref.refine
(the re-rank) -- fp32 parts summed left to right, np.lexsort((rows, dist)), padded with
(+inf, -1)."""
import numpy as np

import datagen
import ivf_ref
import ivf_residual_ref as ref
import refine_ref as rr
import search_filter_ref as fref
import search_lists_ref as lref
import search_shapes_ref as sref

MAX_K, WIDE_K = 64, 256       # PQH_SEARCH_MAX_K, PQH_SEARCH_MAX_K_WIDE
LANES = 64                    # an offer is 64 candidates; a block of the wide list 64 entries
SERIAL_MAX = sref.SERIAL_MAX

# ------------------------------------------------------------------------------ the whole stream
N = 1003
NQ = 9                        # four tables a workgroup: three batches, one of them part-filled
CHUNKS = (1, 7, 64)
TOP_KS = (65, 100, 128, 129, 192, 255, 256)
# name: (m, K, context) -- the packed walk of one and of two words, the byte-wise walk
SHAPES = {"ctx_m8": (8, 256, True), "noctx_m8": (8, 256, False), "ctx_m16": (16, 256, True),
          "noctx_m16": (16, 256, False), "m12_k16": (12, 16, False), "m5_k16": (5, 16, False)}
SHORT_N = 100                 # fewer rows than k: the tail is padding


def codes_of(shape):
    m, K, _ = SHAPES[shape]
    return datagen.skewed_codes(N, m, k=K, seed=100 + m + K)


def lut_of(shape, seed, nq=NQ):
    m, K, _ = SHAPES[shape]
    return fref.lut_of(nq, m, seed, k=K)


want = fref.want


def check_whole_stream():
    assert NQ % 4 and NQ > 8                       # three batches of four, the last part-filled
    assert all(MAX_K < k <= WIDE_K for k in TOP_KS)
    assert {k % LANES for k in TOP_KS} >= {0, 1, 63}
    assert {(k - 1) // LANES for k in TOP_KS} == {1, 2, 3}   # the threshold in every later block
    assert {sref.walk_of(m) for m, K, c in SHAPES.values()} == {0, 1, 2}
    assert MAX_K < SHORT_N < 128 and N > 3 * WIDE_K    # padding from k = 128 on, none at 65
    for shape in SHAPES:
        codes = codes_of(shape)
        wd, wi = want(lut_of(shape, 1), codes[:SHORT_N], WIDE_K)
        assert (wi[:, :SHORT_N] >= 0).all() and (wi[:, SHORT_N:] == -1).all()
        assert np.isposinf(wd[:, SHORT_N:]).all()


# ------------------------------------------------------------------------------ ties
TIES_SEED = 9                 # (the first seed at which check_ties holds for every query)
TIE_EDGES = (64, 128, 192)    # the first entry of every block but the first


def ties_lut(nq=NQ, m=8, seed=TIES_SEED):
    return fref.ties_lut(nq, m, seed)


def check_ties(lut, codes, top_ks=TOP_KS):
    """equal distances across every block boundary of the list and across the threshold of
    every top_k: there (dist, row) has to decide"""
    wd, wi = want(lut, codes, WIDE_K + 1)
    for q in range(lut.shape[0]):
        for e in TIE_EDGES + tuple(top_ks):
            assert wd[q, e - 1] == wd[q, e] and wi[q, e - 1] < wi[q, e], (q, e)


# ------------------------------------------------------------------------------ the offer paths
# 512 rows in four groups of 128: part g of a row of group g is 1 + (r % 128), every other part
# 0, and every table has a zero at symbol 0 -- so dist(r) = lut[r // 128][1 + r % 128] is chosen
# row by row and is exact.  One workgroup of one wave offers the rows 64 at a time, in row
# order: offers 0-3 fill the list, 4 and 6 have j passing lanes, 5 and 7 none.
OFFER_N, OFFER_M, OFFER_GROUP = 512, 8, 128
OFFER_J = (0, 1, 6, 7, 63, 64)
OFFER_TOP_KS = (65, 128, 200, 256)
OFFER_ORDERS = sref.OFFER_ORDERS
OFFER_LANDINGS = ("tail", "boundary")      # of offer 4; offer 6 lands before everything
FAIL = np.float32(50000.0)


def offer_codes():
    codes = np.zeros((OFFER_N, OFFER_M), np.uint8)
    r = np.arange(OFFER_N)
    codes[r, r // OFFER_GROUP] = 1 + r % OFFER_GROUP
    return codes


def offer_start(top_k, j, landing):
    """the rank of the first passing candidate of offer 4 among the 256 rows before it: `tail`
    the last j ranks below the threshold; `boundary` j ranks around the last block boundary
    below the threshold's entry (moved down as far as it takes for all of them to pass)"""
    if landing == "tail":
        return top_k - j
    edge = LANES * ((top_k - 1) // LANES)
    return max(0, min(edge - j // 2, top_k - j))


def offer_table(top_k, j, order, landing, seed):
    """[1][8][256].  Rows 0-255: 1000 + 10 * a permutation of 0 ... 255, so the list after them
    holds the ranks 0 ... top_k - 1 and its threshold is T = 1000 + 10 * (top_k - 1).  Offer 4
    (rows 256-319): exactly j lanes beat T, with values 1000 + 10 * (s + i) - 5 that fall
    between the entries of ranks s + i - 1 and s + i, s = offer_start; offer 5: nobody; offer 6:
    again j, below everything before (the whole list shifts); offer 7: nobody."""
    rng = np.random.default_rng(seed)
    dist = np.empty(OFFER_N, np.float32)
    dist[:WIDE_K] = 1000 + 10 * rng.permutation(WIDE_K)
    s = offer_start(top_k, j, landing)
    dist[256:320] = sref._passing(rng, j, order, 1000 + 10 * (s + np.arange(j)) - 5, FAIL)
    dist[320:384] = 2 * FAIL + np.arange(LANES)
    dist[384:448] = sref._passing(rng, j, order, -1000 + 10 * np.arange(j), 3 * FAIL)
    dist[448:512] = 4 * FAIL + np.arange(LANES)
    lut = np.zeros((1, OFFER_M, 256), np.float32)
    r = np.arange(OFFER_N)
    lut[0, r // OFFER_GROUP, 1 + r % OFFER_GROUP] = dist
    return lut, dist


def offers_passing(dist, top_k):
    """search_shapes_ref.offers_passing with a list of top_k entries: how many candidates of
    every offer of 64 rows precede the threshold (entry top_k - 1, +inf while the list has
    fewer) when the offer comes"""
    held = np.zeros(0, np.int64)
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
        held = both[np.lexsort((both, dist[both]))][:top_k]
    return counts


def check_offer_case(codes, lut, dist, top_k, j, order, landing):
    assert np.array_equal(ref.adc(lut[0], codes), dist) and len(np.unique(dist)) == OFFER_N
    assert not lut[0, :, 0].any() and not lut[0, 4:].any()
    counts = offers_passing(dist, top_k)
    assert counts[0] == LANES and counts[4:] == [j, 0, j, 0], (counts, top_k, j)
    # where offer 4 lands: ranks [s, s + j) of the list as it will be, s its first
    s = offer_start(top_k, j, landing)
    mine = np.sort(dist[256:320][dist[256:320] < FAIL])
    before = np.sort(dist[:WIDE_K])
    assert len(mine) == j and 0 <= s and s + j <= top_k
    if j:
        assert np.array_equal(np.searchsorted(before, mine), s + np.arange(j))
        edge = LANES * ((top_k - 1) // LANES)
        if landing == "boundary" and j > 1:
            # passing rows on both sides of a block boundary, entries too: an entry moves from
            # lane 63 of a block to lane 0 of the next
            assert s < edge < s + j
        if landing == "tail" and j <= top_k - edge:
            assert s >= edge                                   # inside the threshold's block
    for base in (256, 384):
        d = dist[base:base + LANES]
        got = d[d < FAIL]
        if order == "ascending":
            assert (np.diff(got) > 0).all()
        elif order == "descending":
            assert (np.diff(got) < 0).all()
        elif j > SERIAL_MAX:
            assert (np.diff(got) > 0).any() and (np.diff(got) < 0).any()
    assert (dist[384:448][dist[384:448] < FAIL] < dist[:384].min()).all()   # before everything
    assert SERIAL_MAX in OFFER_J and SERIAL_MAX + 1 in OFFER_J


def offer_cases():
    """(top_k, j, order, landing, seed) of every case, the seeds both test files use"""
    seed = 0
    for top_k in OFFER_TOP_KS:
        for j in OFFER_J:
            for order in OFFER_ORDERS:
                for landing in OFFER_LANDINGS:
                    seed += 1
                    yield top_k, j, order, landing, seed


# ------------------------------------------------------------------------------ the grid
GRID_N, GRID_CHUNK, GRID_NQ = 16_700, 4, 5
GRID_GROUPS = (1, 3, 17, 65)


def grid_case():
    codes = datagen.skewed_codes(GRID_N, 8, k=256, seed=7)
    return codes, fref.ties_lut(GRID_NQ, 8, 6)


def check_grid_case(codes, lut):
    steps = -(-(-(-GRID_N // GRID_CHUNK)) // LANES)
    assert steps >= max(GRID_GROUPS)               # the grid is not capped below 65 groups
    assert max(GRID_GROUPS) > 16 * 4               # the merge loop's second round (16 waves, 4 ahead)
    wd, _ = want(lut, codes, WIDE_K)
    assert all((np.diff(wd[q]) == 0).sum() > 200 for q in range(GRID_NQ))


# ------------------------------------------------------------------------------ the probe forms
PROBE_SHAPES = fref.PROBE_SHAPES           # (8, 256): the packed walk; (12, 256): the byte-wise
PROBE_CHUNK = 7
PROBE_KS = (65, 256)


def probe_case(m, K):
    case = sref.sweep_case(m, K, PROBE_CHUNK, 900 + m)
    return case, fref.probe_masks(case)["half"]


def check_probe_case(case, keep):
    codes, offsets, probes = case[0], case[1], case[2]
    sref.check_sweep_case(codes.shape[1], 256, PROBE_CHUNK, case)
    ptr, ranges = lref.probe_ranges(offsets, probes)
    for mask in (None, keep):
        wd, wi = ref.search(np.repeat(case[3], probes.shape[1], axis=0), codes, WIDE_K + 1, ptr,
                            ranges, keep=mask)
        found = (wi >= 0).sum(axis=1)
        # a query with more rows than the list holds, and one with fewer: its tail is padding
        assert (found > WIDE_K).any() and ((found > 0) & (found < MAX_K)).any(), found


# ------------------------------------------------------------------------------ the re-rank
REFINE_CANDS = ((65, 1), (65, 65), (128, 10), (200, 200), (256, 1), (256, 10), (256, 256))
REFINE_NQS = (1, 5)


def check_refine_cands():
    assert all(MAX_K < c <= WIDE_K and 1 <= k <= c for c, k in REFINE_CANDS)
    assert {-(-c // LANES) for c, k in REFINE_CANDS} == {2, 4}      # two and four wave pairs
    assert any(c % LANES for c, k in REFINE_CANDS)                  # a part-filled pair
    for chunks in rr.CHUNKS:
        for ncand, _ in REFINE_CANDS:
            rows = rr.candidates(5, ncand, chunks, 17 + ncand)
            rr.check_candidates(rows, chunks)
            assert (rows[:, LANES:] >= 0).any()


def residual_rows(w, ncand=200, seed=3):
    """the candidates of refine_ref.residual_world made wider: its rows (the first row of every
    list after an empty one among them), random rows behind them, a -1 and the last row in the
    later wave pairs"""
    rng = np.random.default_rng(seed)
    base = w["rows"]
    extra = rng.integers(0, rr.N, size=(base.shape[0], ncand - base.shape[1])).astype(np.int64)
    rows = np.concatenate([base, extra], axis=1)
    rows[:, 70] = -1
    rows[:, 150] = rr.N - 1
    return rows


def check_residual_rows(w, rows):
    rr.check_residual_world(w)
    assert rows.shape[1] > 3 * LANES and (rows[:, 70] == -1).all()
    assert all(np.isin(w["after_empty"], r).all() for r in rows)


# ------------------------------------------------------------------------------ the index
IVF_KS = ((200, 0), (10, 256), (256, 256))      # (k, refine) of IVF.search


def check_ivf_world(w):
    """every query probes more than 256 rows, so the unfiltered search fills the list; under
    the world's keep it finds fewer, so the filtered one ends in padding"""
    for kind in ("plain", "residual"):
        free = rr.ivf_candidates(w, kind, WIDE_K + 1)[1]
        kept = rr.ivf_candidates(w, kind, WIDE_K + 1, w["keep"])[1]
        assert (free >= 0).all()
        found = (kept >= 0).sum(axis=1)
        assert (found > MAX_K).all() and (found < WIDE_K).all(), found


# ------------------------------------------------------------------------------ recall
def recall_experiment(cands=(64, 256), n=20000, nq=200, d=32):
    """DESIGN.md section 4.5.8's experiment with a 16 x 256 second code, in the float32
    arithmetic of refine_ref: for every candidate count c the share of the exact top 10 among
    the c best rows by ADC distance, and recall@10 after the re-rank of those c"""
    x = datagen.sift_like(n + nq, d, seed=3, centers=256)
    base, q = x[:n], x[n:]
    cent1 = datagen.lloyd_centroids(base, 8, 256, iters=4)
    codes1 = ref.pq_codes(base, cent1)
    left = base - rr.reconstruct(cent1, codes1)
    cent2 = datagen.lloyd_centroids(left, 16, 256, iters=4)
    codes2 = ref.pq_codes(left, cent2)
    exact = np.empty((nq, 10), np.int64)
    for i in range(nq):
        t = base.astype(np.float64) - q[i].astype(np.float64)
        exact[i] = np.argsort((t * t).sum(axis=1), kind="stable")[:10]
    dsub = d // 8
    lut = np.stack([ivf_ref.dists(q[:, dsub * i:dsub * (i + 1)], cent1[i]) for i in range(8)], axis=1)
    cand = want(lut, codes1, max(cands))[1]
    out = {}
    for c in cands:
        rows = cand[:, :c]
        _, ids = rr.refine(q, rows, 10, cent1, codes1, cent2, codes2)
        share = np.mean([np.isin(exact[i], rows[i]).mean() for i in range(nq)])
        recall = np.mean([np.isin(exact[i], ids[i]).mean() for i in range(nq)])
        out[c] = (float(share), float(recall))
    return out
