"""Inputs and the numpy reference of the filtered search (the *_masked calls, codec.pack_mask,
the keep= of the search functions and of IVF.search, IVF.remove), shared by
tests/test_search_filter_cpu.py and tests/test_gpu_search_filter.py, each input with a check_*
function that asserts the properties its case relies on.  Nothing here calls the library.

A filtered result is the unfiltered definition over the kept rows: ivf_residual_ref.adc's sum,
np.lexsort((rows, dist)) over the rows that are kept (and inside the query's ranges), padded
with (+inf, -1).  A mask's words are np.packbits(..., bitorder="little")."""
import numpy as np

import datagen
import ivf_ref
import ivf_residual_ref as ref
import search_lists_ref as lref
import search_shapes_ref as sref

N = 1003                      # no multiple of a chunk, of 32 or of 64
CHUNKS = (1, 4, 7, 64)
NQ = 9                        # two batches of eight tables, one of them part-filled
TOP_KS = (1, 10, 64)
# name: (m, k, context) -- the modes of tests/test_gpu_search_ranges.py: all three walks
MODES = {"ctx_m8": (8, 256, True), "noctx_m8": (8, 256, False), "ctx_m16": (16, 256, True),
         "noctx_m3": (3, 256, False)}
LANES = 64                    # a step is 64 chunks
CODES_ROWS = 4                # the rows of a lane of the scan over plain codes
SINGLE_ROWS = (0, 31, 32, 63, 64, N - 1)


def codes_of(mode):
    m, k, _ = MODES[mode]
    return datagen.skewed_codes(N, m, k=k, seed=100 + m + k)


def lut_of(nq, m, seed, k=256):
    return np.random.default_rng(seed).normal(0.0, 100.0, size=(nq, m, k)).astype(np.float32)


def ties_lut(nq, m, seed):
    """only the values 0, 1, 2: hundreds of rows share each distance, the ids decide"""
    return np.random.default_rng(seed).integers(0, 3, size=(nq, m, 256)).astype(np.float32)


# ------------------------------------------------------------------------------ the mask
def pack(keep, stale=False):
    """int32 [ceil(n / 32)]: bit r & 31 of word r >> 5 = keep[r]; stale: the bits from n on in
    the last word all set (they may hold anything)"""
    keep = np.asarray(keep, bool)
    n = len(keep)
    bits = np.zeros(((n + 31) // 32) * 32, bool)
    bits[:n] = keep
    if stale:
        bits[n:] = True
    return np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32).view(np.int32)


def check_pack():
    keep = np.zeros(70, bool)
    keep[[0, 31, 32, 69]] = True
    w = pack(keep).view(np.uint32)
    assert w.tolist() == [0x80000001, 1, 1 << 5]
    assert pack(keep, stale=True).view(np.uint32).tolist() == [0x80000001, 1, 0xFFFFFFE0]
    assert len(pack(np.zeros(0, bool))) == 0 and len(pack(np.ones(64, bool))) == 2
    assert len(pack(np.ones(65, bool))) == 3


def want(lut, codes, k, keep=None, id_base=0, d=None):
    """the top k by (dist, id) of the kept rows, padded with (+inf, -1)"""
    d = sref.dists(lut, codes) if d is None else d
    rows = np.arange(codes.shape[0], dtype=np.int64)
    if keep is not None:
        rows = rows[np.asarray(keep, bool)]
    wd = np.full((lut.shape[0], k), np.inf, np.float32)
    wi = np.full((lut.shape[0], k), -1, np.int64)
    for q in range(lut.shape[0]):
        dist = d[q, rows]
        order = np.lexsort((rows, dist))[:k]
        wd[q, :len(order)] = dist[order]
        wi[q, :len(order)] = rows[order] + id_base
    return wd, wi


def random_mask(n, fraction, seed):
    return np.random.default_rng(seed).random(n) < fraction


def chunk_end_masks(n, chunk):
    """(first, last): only the first row of every chunk kept (a lane stops after one row), only
    the last one (it cannot stop early)"""
    first = np.zeros(n, bool)
    first[::chunk] = True
    last = np.zeros(n, bool)
    last[chunk - 1::chunk] = True
    last[n - 1] = True
    return first, last


def single(n, row):
    keep = np.zeros(n, bool)
    keep[row] = True
    return keep


def complement_of_top(lut, codes, d=None):
    """every row but those of some query's unfiltered top 64"""
    top = want(lut, codes, 64, d=d)[1]
    keep = np.ones(codes.shape[0], bool)
    keep[top[top >= 0]] = False
    return keep


def plain_masks(chunk, lut, codes, d=None):
    """name -> bool [N], every mask of the plain search but the ties case"""
    first, last = chunk_end_masks(N, chunk)
    masks = {"ones": np.ones(N, bool), "zeros": np.zeros(N, bool), "half": random_mask(N, 0.5, 11),
             "sparse": random_mask(N, 0.01, 10), "first": first, "last": last,
             "not_top": complement_of_top(lut, codes, d)}
    for r in SINGLE_ROWS:
        masks[f"row{r}"] = single(N, r)
    return masks


def steps_kept(keep, rows_per_step):
    """the kept rows of every step of the plain scan"""
    n = len(keep)
    return [int(keep[s:s + rows_per_step].sum()) for s in range(0, n, rows_per_step)]


def check_sparse(keep):
    """about ten rows, fewer than k = 64; at chunks 1 and 4 (and over plain codes, lanes of
    CODES_ROWS rows) a whole step of 64 chunks without a kept row, and one with one"""
    assert 5 <= keep.sum() < 20
    for chunk in (1, 4, CODES_ROWS):
        per_step = steps_kept(keep, LANES * chunk)
        assert min(per_step) == 0 and max(per_step) > 0, (chunk, per_step)


def check_chunk_ends(chunk):
    first, last = chunk_end_masks(N, chunk)
    chunks = -(-N // chunk)
    assert first.sum() == chunks and last.sum() == chunks
    for j in range(chunks):
        rows = np.arange(j * chunk, min((j + 1) * chunk, N))
        assert first[rows[0]] and last[rows[-1]]
        assert first[rows].sum() == 1 and last[rows].sum() == 1


def check_not_top(lut, codes, keep, d=None):
    """a filter applied after the selection returns the padding alone, the reference k rows"""
    top = want(lut, codes, 64, d=d)[1]
    assert (top >= 0).all() and not keep[top].any() and keep.sum() >= 64
    wd, wi = want(lut, codes, 64, keep, d=d)
    assert np.isfinite(wd).all() and (wi >= 0).all() and keep[wi].all()
    assert not np.isin(wi, top).any()


def check_plain_masks(chunk, lut, codes, masks, d=None):
    assert masks["ones"].all() and not masks["zeros"].any()
    assert 400 < masks["half"].sum() < 600
    check_sparse(masks["sparse"])
    check_chunk_ends(chunk)
    check_not_top(lut, codes, masks["not_top"], d)
    for r in SINGLE_ROWS:
        assert masks[f"row{r}"].sum() == 1 and masks[f"row{r}"][r]
    wd, wi = want(lut, codes, 64, masks["sparse"], d=d)
    assert (wi[:, -1] == -1).all() and np.isinf(wd[:, -1]).all() and (wi[:, 0] >= 0).all()
    wd, wi = want(lut, codes, 64, masks["zeros"], d=d)
    assert (wi == -1).all() and np.isinf(wd).all()
    a, b = want(lut, codes, 64, masks["ones"], d=d), sref.want(lut, codes, 64)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


def check_ties(lut, codes, keep):
    """ids decide: inside the top 64 of the kept rows, runs of equal distances"""
    wd, wi = want(lut, codes, 64, keep)
    assert all((np.diff(wd[q]) == 0).sum() > 32 for q in range(lut.shape[0]))
    assert keep[wi].all()


def embedded(words, fill):
    """(buffer, slice): the words from an odd int32 index on in a larger buffer of `fill`"""
    buf = np.full(len(words) + 8, fill, np.uint32).view(np.int32)
    buf[3:3 + len(words)] = words
    return buf, slice(3, 3 + len(words))


# ------------------------------------------------------------------------------ the probe forms
PROBE_SHAPES = ((8, 256), (12, 256))      # the packed walk with eight tables, the byte-wise with four
PROBE_CHUNKS = (4, 7)
OUT_LIST, ONLY_LIST = 3, 6                # the list of more than one step; a list of 150 rows


def probe_masks(case):
    """name -> bool [n] for a search_shapes_ref.sweep_case"""
    codes, offsets = case[0], case[1]
    n = codes.shape[0]
    out = np.ones(n, bool)
    out[offsets[OUT_LIST]:offsets[OUT_LIST + 1]] = False
    only = np.zeros(n, bool)
    only[offsets[ONLY_LIST]:offsets[ONLY_LIST + 1]] = True
    return {"half": random_mask(n, 0.5, 21), "sparse": random_mask(n, 0.01, 22), "list_out": out,
            "list_only": only}


def check_probe_masks(chunk, case, masks):
    """(search_lists_ref.check_sweep_inputs holds at chunk 7; at chunk 4 list 3 happens to begin
    on a chunk boundary and is cut at its end alone, so what the filter's cases need of the
    sweep's lists is asserted here for both)"""
    codes, offsets, probes = case[0], case[1], case[2]
    flat = probes.reshape(-1)
    f, c = offsets[OUT_LIST], offsets[OUT_LIST + 1] - offsets[OUT_LIST]
    assert (f + c - 1) // chunk - f // chunk + 1 > LANES and (f + c) % chunk   # steps to pass over
    assert (flat == -1).any() and (np.diff(offsets) == 0).any()
    assert (flat == OUT_LIST).sum() > 8 and (flat == ONLY_LIST).sum() >= 8   # more than one unit
    assert offsets[ONLY_LIST + 1] - offsets[ONLY_LIST] == 150
    assert 1 <= masks["sparse"].sum() < 20
    # a query that probes only the list that is masked out, or none of the kept one: padding
    ptr, ranges = lref.probe_ranges(offsets, probes)
    lut = np.repeat(case[3], probes.shape[1], axis=0)
    wd, wi = ref.search(lut, codes, 64, ptr, ranges, keep=masks["list_only"])
    has = (probes == ONLY_LIST).any(axis=1)
    assert has.any() and not has.all()
    assert (wi[~has] == -1).all() and (wi[has, 0] >= 0).all()
    wd, wi = ref.search(lut, codes, 64, ptr, ranges, keep=masks["list_out"])
    inside = (wi >= offsets[OUT_LIST]) & (wi < offsets[OUT_LIST + 1])
    assert not inside.any()
    plain = ref.search(lut, codes, 64, ptr, ranges)[1]
    assert ((plain >= offsets[OUT_LIST]) & (plain < offsets[OUT_LIST + 1])).any()


def probe_want(case, keep, k=64):
    """(per query, per pair): ivf_residual_ref.search with a table per query and one per pair"""
    codes, offsets, probes, lut_q, lut_pair = case
    ptr, ranges = lref.probe_ranges(offsets, probes)
    return (ref.search(np.repeat(lut_q, probes.shape[1], axis=0), codes, k, ptr, ranges, keep=keep),
            ref.search(lut_pair, codes, k, ptr, ranges, keep=keep))


# ------------------------------------------------------------------------------ pack_mask
PACK_NS = (0, 1, 63, 64, 65, 1003)


def pack_case(n, seed, permuted):
    """(keep u8 [n] with values 0, 1 and others, perm int64 [n] or None, the words)"""
    rng = np.random.default_rng(seed)
    keep = (rng.integers(0, 4, size=n) * (rng.random(n) < 0.6)).astype(np.uint8)
    perm = rng.permutation(n).astype(np.int64) if permuted else None
    by_row = keep if perm is None else keep[perm]
    return keep, perm, pack(by_row != 0)


def bad_perm_case(n=1003, seed=5):
    """every row kept, a permutation with one entry -1 and one entry n: their bits are zero"""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n).astype(np.int64)
    perm[40], perm[n - 2] = -1, n
    bits = np.ones(n, bool)
    bits[[40, n - 2]] = False
    return np.ones(n, np.uint8), perm, pack(bits)


# ------------------------------------------------------------------------------ the index
IVF_N, IVF_NL, IVF_M, IVF_NQ, IVF_NPROBE = 1003, 13, 8, 9, 4


def ivf_world():
    """the data of tests/test_gpu_ivf_residual.py: x with 50 rows twice, 13 lists, an 8 x 256 PQ
    trained on the residuals, nine queries near rows of x -- and for the plain and the residual
    index the stream's codes, the probes and the tables of every (query, probe) pair"""
    x = datagen.sift_like(IVF_N, 128, seed=31)
    x[900:950] = x[100:150]
    rng = np.random.default_rng(32)
    cc = (x[rng.choice(IVF_N, IVF_NL, replace=False)] + np.float32(0.5)).astype(np.float32)
    lists, _ = ivf_ref.assign(x, cc)
    perm, offsets = ivf_ref.layout(lists, IVF_NL)
    res, bad = ref.residuals(x, cc, lists, perm)
    assert not bad.any()
    cent = datagen.lloyd_centroids(res, IVF_M, 256, iters=2, sample=IVF_N)
    q = (x[[100, 101, 120, 149, 7, 300, 555, 800, 1002]] +
         rng.normal(0.0, 3.0, size=(IVF_NQ, 128))).astype(np.float32)
    ptr, ranges, probes, _ = ivf_ref.probe(q, cc, IVF_NPROBE, offsets)
    dsub = 128 // IVF_M
    lut_q = np.stack([ivf_ref.dists(q[:, dsub * i:dsub * (i + 1)], cent[i]) for i in range(IVF_M)],
                     axis=1)
    keep = random_mask(IVF_N, 0.3, 33)                   # over the caller's rows
    return dict(x=x, cc=cc, cent=cent, q=q, perm=perm, offsets=offsets, ptr=ptr, ranges=ranges,
                keep=keep,
                plain=dict(codes=ref.pq_codes(x[perm], cent), lut=np.repeat(lut_q, IVF_NPROBE, axis=0)),
                residual=dict(codes=ref.pq_codes(res, cent), lut=ref.tables(q, cc, probes, cent)))


def ivf_want(w, kind, k, keep=None, removed=None):
    """(dist, caller ids) of IVF.search: keep a bool over the caller's rows or None, removed the
    caller rows taken out"""
    ok = np.ones(IVF_N, bool) if keep is None else np.asarray(keep, bool).copy()
    if removed is not None:
        ok[removed] = False
    wd, rows = ref.search(w[kind]["lut"], w[kind]["codes"], k, w["ptr"], w["ranges"],
                          keep=ok[w["perm"]])
    return wd, np.where(rows >= 0, w["perm"][np.maximum(rows, 0)], -1)


def check_ivf_world(w):
    assert 200 < w["keep"].sum() < 400
    for kind in ("plain", "residual"):
        free = ivf_want(w, kind, 10)
        kept = ivf_want(w, kind, 10, w["keep"])
        assert (free[1] >= 0).all() and (kept[1] >= 0).all()
        assert w["keep"][kept[1]].all() and not w["keep"][free[1]].all()   # the filter matters
        first = free[1][0]
        gone = ivf_want(w, kind, 10, removed=first)
        assert not np.isin(gone[1], first).any() and (gone[1][0] >= 0).all()
        assert not np.array_equal(gone[1][0], first)
        both = ivf_want(w, kind, 10, w["keep"], removed=first)
        assert w["keep"][both[1][both[1] >= 0]].all() and not np.isin(both[1], first).any()
