"""The case table of tests/test_gpu_forest_shapes.py and the CPU models it relies on (checked
without a GPU by tests/test_forest_shapes_cpu.py).  numpy and datagen only: tests/knn_worker.py
imports this module in a child process that has neither the oracle nor pytest.

A case is a name; ``build(name)`` gives its input: x (n, d) float32, num_split, blocks_per_dim,
overlap, num_nn, ``pad`` (> 0: the rows are handed to the library as ``big[:, :d]`` of an
(n, d + pad) tensor whose extra columns hold NaN) and ``geo`` (None: the kNN runs on the block
ranges that blocks_info gives for x; else the (starts, ends) to use instead).

  grid_d{d}_nn{nn}     the instantiation grid: 1,200 sift_like rows, one split, three blocks
                       of about 430 rows (overlap 0.05), so kmax = num_nn + 1
  sizeA_n{N}_b{nb}_nn{nn}   one split, overlap 0, column 0 a permuted arange: block b holds the
                       sorted positions [N b/nb, min(N (b+1)/nb, N - 1)] (``sizes_a``)
  sizeB_{one,two}_n{N}_nn{nn}   two splits over two equal columns, three blocks per split: full
                       diagonal blocks, neighbours that share only the boundary value's rows
                       (one row, or two where every value occurs twice), empty far corners
  path_sep / path_dups / path_offset   the three inputs of the list-path model
  scale_d{d}_nn{nn}_e{s}    grid_d{d}_nn{nn} times 2^s (``m`` for a minus sign), on the grid
                       case's block ranges times 2^s -- blocks_info of the scaled rows is not
                       that: below 2^-22 two of these values are within the reference
                       comparator's 1e-9 and its sort leaves them where they are
  deep_d96_nn20        1,200 deep_like rows in the grid's geometry, the base of the scaled
                       case scale_deep_d96_nn20_em68
  strided_d{d}         grid rows inside a wider NaN-padded tensor
"""
from __future__ import annotations

import functools
import re

import numpy as np

import datagen

# ------------------------------------------------------------------ dispatch (pqh_knn_fast)
GRID_D = (1, 16, 17, 32, 33, 64, 65, 96, 128)
GRID_NN = (7, 8, 15, 16, 31, 32, 51, 52, 63)
VALU_D = (8, 9, 16, 32, 64, 96, 97, 128)      # every DMAX of knn_block_topk, both sides of 8|9, 96|97
LANE_D = (1, 17, 64, 96)                      # one d per DP of knn_select
MST_D = (16, 128)
MST_NN = (7, 15, 31, 51, 63)                  # one num_nn per KMAX
DPS = (16, 32, 64, 128)
DMAXS = (8, 16, 32, 64, 96, 128)
KMAXS = (8, 16, 32, 52, 64)


def dp_of(d):
    """knn_screen / knn_select / knn_select_wave's DP"""
    return 16 if d <= 16 else 32 if d <= 32 else 64 if d <= 64 else 128


def dmax_of(d):
    """knn_block_topk's DMAX"""
    return next(m for m in DMAXS if d <= m)


def kmax_of(num_nn, max_s):
    """(kmax, KMAX): the longest list of the call and the template argument it selects"""
    kmax = min(num_nn, max_s - 1) + 1
    return kmax, next(k for k in KMAXS if kmax <= k)


def ch_of(kmax):
    """listed candidates per half-wave lane before the selection scans the whole block"""
    return 2 * kmax + 16


def grid_name(d, nn):
    return f"grid_d{d}_nn{nn}"


GRID = [grid_name(d, nn) for d in GRID_D for nn in GRID_NN]
GRID_MST = {grid_name(d, nn) for d in MST_D for nn in MST_NN}
VALU_GRID = [grid_name(d, nn) for d in VALU_D for nn in GRID_NN]
LANE_GRID = [grid_name(d, nn) for d in LANE_D for nn in GRID_NN]

# ------------------------------------------------------------------ controlled block sizes
SIZE_A = ((62, 2), (64, 2), (80, 2), (126, 2), (128, 2), (130, 2), (195, 3), (254, 2), (256, 2))
SIZE_NN = (40, 63)
SIZE_D = 20
WANTED_SIZES = (0, 1, 2, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129)
SIZES = ([f"sizeA_n{n}_b{nb}_nn{nn}" for n, nb in SIZE_A for nn in SIZE_NN] +
         [f"sizeB_{k}_n{n}_nn{nn}" for k, n in (("one", 300), ("two", 200)) for nn in SIZE_NN])


def sizes_a(n, nb):
    """construction A's block sizes: sorted positions [n b/nb, min(n (b+1)/nb, n - 1)], both
    ends included (dimension_info_build reads the value AT each end)"""
    return [min(n * (b + 1) // nb, n - 1) - n * b // nb + 1 for b in range(nb)]


def sizes_b(n, twice):
    """construction B (three blocks per split, block id = 3 * (range of column 1) + (range of
    column 0), both columns equal): diagonal blocks as construction A over the sorted values,
    neighbours hold the rows of the shared boundary value, the far corners nothing"""
    srt = np.sort(np.arange(n) // 2 if twice else np.arange(n))
    lo = [srt[n * b // 3] for b in range(3)]
    hi = [srt[min(n * (b + 1) // 3, n - 1)] for b in range(3)]
    lo[0] -= 1
    hi[2] += 1
    out = []
    for b0 in range(3):
        for b1 in range(3):
            s, e = max(lo[b0], lo[b1]), min(hi[b0], hi[b1])
            out.append(int(((srt >= s) & (srt <= e)).sum()))
    return out


# ------------------------------------------------------------------ magnitudes
SCALE_BASE = ((16, 15), (128, 32))
# grid_d128_*'s largest list distance is 2^18.3 .. 2^18.6 and its largest ||x||^2 is 2^19.0: no
# power of two puts the first below and the second above fp32's maximum (the same holds for
# twenty other seeds), so its top scale is kind "top" (everything finite, ||q||^2 + Cmax a
# factor 2 below the maximum) and the padded d = 96 cell supplies DP = 128's overflow case
OVERFLOW_ONLY = ((96, 16),)
FP32_MAX = float(np.finfo(np.float32).max)


def scale_name(d, nn, s):
    return f"scale_d{d}_nn{nn}_e{'m' if s < 0 else ''}{abs(s)}"


@functools.lru_cache(maxsize=None)
def pair_stats(d, nn):
    """(the largest distance any in-block list of grid_d{d}_nn{nn} holds -- the largest
    kk-th smallest squared distance over its (block, query) pairs --, smallest and largest
    non-zero |coordinate|), in float64"""
    c = build(grid_name(d, nn))
    x = c["x"].astype(np.float64)
    st, en = blocks_info_model(c["x"], c["ns"], c["nb"], c["ov"])
    dk = 0.0
    for rows in members(c["x"], st, en):
        kk = min(nn, len(rows) - 1) + 1
        dk = max(dk, float(np.sort(pair_dist64(x[rows]), axis=1)[:, kk - 1].max()))
    nz = np.abs(x[x != 0])
    return dk, float(nz.min()), float(nz.max())


def overflow_exp(d, nn):
    """the largest s at which every distance of every in-block list (hence every distance the
    oracle returns) is still finite in fp32: the direct form's partial sums are non-negative
    and grow, so the last is the largest, and rounding moves it by at most (d + 2) 2^-24 of
    itself.  Distances of pairs further apart may be +inf there."""
    dk = pair_stats(d, nn)[0] * (1.0 + (d + 2) * 2.0 ** -24)
    s = int(np.floor(np.log2(FP32_MAX / dk) / 2))
    assert dk * 4.0 ** s <= FP32_MAX < dk * 4.0 ** (s + 1)
    return s


def tiny_exps(d, nn):
    """(s1, s2): at 2^s1 only the smallest non-zero coordinates' squares are below 2^-126 (the
    largest's are not); at 2^s2 every coordinate's square is, and none is below 2^-149"""
    _, lo, hi = pair_stats(d, nn)
    s2 = int(np.floor((-126 - 2 * np.log2(hi)) / 2 - 1e-9))
    s1 = int(np.floor((-126 - 2 * np.log2(lo)) / 2 - 1e-9)) - 2
    assert (lo * 2.0 ** s1) ** 2 < 2.0 ** -126 <= (hi * 2.0 ** s1) ** 2
    assert 2.0 ** -149 <= (lo * 2.0 ** s2) ** 2 and (hi * 2.0 ** s2) ** 2 < 2.0 ** -126
    return s1, s2


MID_EXPS = (-40, 20)
# unit-norm float rows (coordinates around 0.1) times 2^-68: every square is a denormal with a
# handful of significant bits, so -- unlike the integer rows above, whose scaled products are
# exact multiples of 4^s -- every product is rounded at 2^-149, an absolute error that E, a
# relative bound, does not count
DEEP_TINY, DEEP_TINY_EXP = "scale_deep_d96_nn20_em68", -68


@functools.lru_cache(maxsize=None)
def scale_cases():
    """{case name: (base grid case, exponent, kind)}; kind in mid / overflow / top / tiny"""
    out = {}
    for d, nn in SCALE_BASE:
        for s in MID_EXPS:
            out[scale_name(d, nn, s)] = (grid_name(d, nn), s, "mid")
        s = overflow_exp(d, nn)
        out[scale_name(d, nn, s)] = (grid_name(d, nn), s, "overflow" if norms_overflow(d, nn, s) else "top")
        for s in tiny_exps(d, nn):
            out[scale_name(d, nn, s)] = (grid_name(d, nn), s, "tiny")
    for d, nn in OVERFLOW_ONLY:
        s = overflow_exp(d, nn)
        out[scale_name(d, nn, s)] = (grid_name(d, nn), s, "overflow")
    out[DEEP_TINY] = ("deep_d96_nn20", DEEP_TINY_EXP, "tiny")
    return out


def norms_overflow(d, nn, s):
    """every block of grid_d{d}_nn{nn} times 2^s holds a row whose fp32 ||x||^2 is +inf"""
    c = build(grid_name(d, nn))
    x = c["x"] * np.float32(2.0 ** s)
    with np.errstate(over="ignore"):
        nrm = (x * x).sum(1, dtype=np.float32)
    st, en = blocks_info_model(c["x"], c["ns"], c["nb"], c["ov"])
    return all(np.isinf(nrm[r]).any() for r in members(c["x"], st, en))


# ------------------------------------------------------------------ the rest of the table
PATHS = ("path_sep", "path_dups", "path_offset")
STRIDED = ("strided_d40", "strided_d128")
STRIDED_BASE = {"strided_d40": (40, 25), "strided_d128": (128, 50)}
STRIDE_PAD = 24
PATH_DUPS = 100      # identical rows of path_dups (> 2 ch + 8 = 92 at num_nn = 12)


def _case(x, ns, nb, ov, nn, pad=0, geo=None):
    x = np.ascontiguousarray(x, np.float32)
    x.setflags(write=False)
    return dict(x=x, ns=ns, nb=nb, ov=ov, nn=nn, pad=pad, geo=geo)


def _perm_column(n, seed, twice=False):
    v = np.random.default_rng(seed).permutation(n)
    return (v // 2 if twice else v).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _sift(n, d, seed):
    return datagen.sift_like(n, d, seed=seed)


@functools.lru_cache(maxsize=None)
def build(name):
    m = re.fullmatch(r"grid_d(\d+)_nn(\d+)", name)
    if m:
        d, nn = int(m[1]), int(m[2])
        return _case(_sift(1200, d, 1000 + d), 1, 3, 0.05, nn)
    m = re.fullmatch(r"sizeA_n(\d+)_b(\d+)_nn(\d+)", name)
    if m:
        n, nb, nn = int(m[1]), int(m[2]), int(m[3])
        x = _sift(n, SIZE_D, 2000 + n).copy()
        x[:, 0] = _perm_column(n, 2100 + n)
        return _case(x, 1, nb, 0.0, nn)
    m = re.fullmatch(r"sizeB_(one|two)_n(\d+)_nn(\d+)", name)
    if m:
        n, nn = int(m[2]), int(m[3])
        x = _sift(n, SIZE_D, 2200 + n).copy()
        x[:, 0] = _perm_column(n, 2300 + n, twice=m[1] == "two")
        x[:, 1] = x[:, 0]
        return _case(x, 2, 3, 0.0, nn)
    if name == "deep_d96_nn20":
        return _case(datagen.deep_like(1200, 96, seed=3005), 1, 3, 0.05, 20)
    if name == "path_sep":
        return _case(_sift(1200, 16, 3001), 1, 3, 0.1, 10)
    if name == "path_dups":
        # 100 copies of one row (its column 0 well inside block 0) scattered among 600
        # ordinary rows: the copies' lists overflow, their block-mates' need not
        x = _sift(700, 16, 3002).copy()
        at = np.sort(np.random.default_rng(3003).choice(700, PATH_DUPS, replace=False))
        row = x[at[0]].copy()
        row[0] = np.sort(x[:, 0])[120]
        x[at] = row
        return _case(x, 1, 2, 0.1, 12)
    if name == "path_offset":
        return _case(_sift(1200, 128, 3004) + np.float32(4096), 1, 3, 0.1, 20)
    if name in scale_cases():
        base, s, _ = scale_cases()[name]
        c = build(base)
        f = np.float32(2.0 ** s)
        st, en = blocks_info_model(c["x"], c["ns"], c["nb"], c["ov"])
        return _case(c["x"] * f, c["ns"], c["nb"], c["ov"], c["nn"], geo=(st * f, en * f))
    if name in STRIDED_BASE:
        d, nn = STRIDED_BASE[name]
        return _case(_sift(1200, d, 1000 + d), 1, 3, 0.05, nn, pad=STRIDE_PAD)
    raise KeyError(name)


def dups_rows(c):
    """the identical rows of path_dups"""
    x = c["x"]
    same = (x[:, None, :] == x[None, :, :]).all(-1).sum(1)
    return np.flatnonzero(same == PATH_DUPS)


# ------------------------------------------------------------------ geometry in numpy
def blocks_info_model(x, ns, nb, ov):
    """blocks_info_init for columns without two distinct values closer than 1e-9 (every
    column of this table): a plain sort"""
    n = len(x)
    st = np.zeros((ns, nb), np.float32)
    en = np.zeros_like(st)
    o = int(n * ov / 2)
    for i in range(ns):
        col = np.sort(x[:, ns - 1 - i])
        for b in range(nb):
            s = min(max(n * b // nb - o, 0), n)
            e = min(min(max(n * (b + 1) // nb + o, 0), n), n - 1)
            st[i, b] = col[min(s, n - 1)]
            en[i, b] = col[e]
        st[i, 0] = np.float32(np.float64(col[0]) - 1.0)
        en[i, nb - 1] = np.float32(np.float64(col[-1]) + 1.0)
    return st, en


def members(x, st, en):
    """rows of every block in block-id order (split 0 is the most significant digit and reads
    coordinate ns - 1)"""
    ns, nb = st.shape
    out = []
    for B in range(nb ** ns):
        ok = np.ones(len(x), bool)
        for i in range(ns):
            b = B // nb ** (ns - 1 - i) % nb
            v = x[:, ns - 1 - i]
            ok &= ~((v < st[i, b]) | (v > en[i, b]))
        out.append(np.flatnonzero(ok))
    return out


def pair_dist64(xb):
    """all squared distances of a block's rows (float64, summed over the dimensions)"""
    acc = np.zeros((len(xb), len(xb)))
    for j in range(xb.shape[1]):
        t = xb[:, j, None] - xb[None, :, j]
        acc += t * t
    return acc


# ------------------------------------------------------------------ the list-path model
def path_model(c):
    """For every (block, query) pair of case c what the screen MUST do, from its documented
    guarantee alone.  Returns a list over the blocks of (rows, listed, full): bool arrays over
    the block's positions.

    listed: at most ch candidates have D_c <= D_(2kk-1) + 4 E.  One of the two halves holds kk
      of the 2kk-1 smallest d', so T <= d'_(2kk-1) <= D_(2kk-1) + E; a candidate on the list
      has d'_c <= T + 2 E, hence D_c <= d'_c + E <= D_(2kk-1) + 4 E.  (A block of fewer than
      2kk-1 rows may leave T = +inf: then every row is listed, and no half of the block may
      hold more than ch.)
    full:   more than ch candidates of one half ((position >> 2) & 1) have D_c <= D_(kk): the
      screen lists every one of them, so that half overflows.

    E is the kernel's formula with the norms in float64 pushed up by 2^-20 (the kernel's fp32
    norms are within d 2^-24 of them): a larger E only makes `listed` harder to prove."""
    x = c["x"]
    d = x.shape[1]
    st, en = blocks_info_model(x, c["ns"], c["nb"], c["ov"])
    mem = members(x, st, en)
    kmax = min(c["nn"], max(len(r) for r in mem) - 1) + 1
    ch = ch_of(kmax)
    coef = (3.0 * 2.0 ** -18 + (3 * dp_of(d) + 3 * d + 8) * 2.0 ** -24) * 1.25 * (1 + 2.0 ** -20)
    out = []
    for rows in mem:
        S = len(rows)
        if S == 0:
            out.append((rows, np.zeros(0, bool), np.zeros(0, bool)))
            continue
        xb = x[rows].astype(np.float64)
        D = pair_dist64(xb)
        nrm = (xb * xb).sum(1)
        E = coef * (nrm + nrm.max())
        kk = min(c["nn"], S - 1) + 1
        srt = np.sort(D, axis=1)
        half = (np.arange(S) >> 2) & 1
        if S >= 2 * kk - 1:
            listed = (D <= (srt[:, 2 * kk - 2] + 4 * E)[:, None]).sum(1) <= ch
        else:
            listed = np.full(S, max((half == 0).sum(), (half == 1).sum()) <= ch)
        near = D <= srt[:, kk - 1][:, None]
        full = np.maximum(near[:, half == 0].sum(1), near[:, half == 1].sum(1)) > ch
        assert not (listed & full).any()
        out.append((rows, listed, full))
    return out


def flush_model(c):
    """What a screen would return on case c if its MFMA gave 0 for every dot product (as one
    that flushes fp32 denormals would where every product of two coordinates is below 2^-126):
    d' = ||q||^2 + ||c||^2, T at most the block's (2kk-1)-th smallest d' (see path_model), the
    list every candidate with d' <= T + 2 E.  Returns (pairs, wrong): wrong counts the pairs
    whose list surely stays within ch slots -- no full scan comes to the rescue -- and misses
    a candidate strictly closer than the kk-th neighbour."""
    x = c["x"]
    d = x.shape[1]
    st, en = c["geo"] or blocks_info_model(x, c["ns"], c["nb"], c["ov"])
    mem = members(x, st, en)
    ch = ch_of(min(c["nn"], max(len(r) for r in mem) - 1) + 1)
    coef = (3.0 * 2.0 ** -18 + (3 * dp_of(d) + 3 * d + 8) * 2.0 ** -24) * 1.25 * (1 + 2.0 ** -20)
    pairs = wrong = 0
    for rows in mem:
        S = len(rows)
        kk = min(c["nn"], S - 1) + 1
        if S < 2 * kk - 1:
            continue
        xb = x[rows].astype(np.float64)
        D = pair_dist64(xb)
        nrm = (xb * xb).sum(1)
        dflush = (nrm[:, None] + nrm[None, :]) * (1 - 2.0 ** -20)
        U = np.sort(dflush, axis=1)[:, 2 * kk - 2] + 2 * coef * (nrm + nrm.max())
        listed = dflush <= U[:, None]
        must = D < np.sort(D, axis=1)[:, kk - 1][:, None]
        wrong += int(((listed.sum(1) <= ch) & (must & ~listed).any(1)).sum())
        pairs += S
    return pairs, wrong


# ------------------------------------------------------------------ the children's case lists
EXTRA = SIZES + list(PATHS)


def child_cases(variant):
    if variant == "valu":
        return VALU_GRID + EXTRA + list(STRIDED) + list(scale_cases())
    assert variant == "lane"
    return LANE_GRID + EXTRA
