"""Generators and numpy references for the PQ-assignment and k-means edge tests
(test_assign_cpu.py, test_gpu_assign_edges.py, test_gpu_kmeans.py) -- test infrastructure.

Nothing here is imported from the kernel: `tau_doc` and `bf16_split` restate DESIGN.md
section 4.1 on the test side, `direct_gap` the oracle's fp32 direct form.
"""
from __future__ import annotations

import numpy as np

DSUBS = (4, 6, 8, 12, 16, 32)
N_BAND = 2048 + 37
# e range of near_tie at which the conditions of test_assign_cpu hold (rows below, inside and
# above the band 0.1 tau .. 10 tau)
E_LO, E_HI = 2, 30


def parts_of(dsub: int) -> int:
    """m of the near-tie cases: two subspaces, one at dsub 32"""
    return 1 if dsub == 32 else 2


def nearest_other(cent_p: np.ndarray) -> np.ndarray:
    """index of every centroid's nearest other centroid (one part, (k, dsub)), in float64"""
    c = cent_p.astype(np.float64)
    sq = (c ** 2).sum(1)
    out = np.empty(c.shape[0], np.int64)
    for r0 in range(0, c.shape[0], 512):   # (row blocks: 16 MB at k = 4,096, not (k, k))
        d2 = sq[r0:r0 + 512, None] + sq[None, :] - 2.0 * (c[r0:r0 + 512] @ c.T)
        rows = np.arange(d2.shape[0])
        d2[rows, r0 + rows] = np.inf
        out[r0:r0 + 512] = d2.argmin(1)
    return out


def near_tie(n: int, m: int, dsub: int, seed: int, offset: float = 0.0, e_lo: int = E_LO,
             e_hi: int = E_HI, k: int = 256, cent: np.ndarray = None):
    """(x (n, m dsub), cent (m, k, dsub)), both float32.  Centroids are N(0, 1) + offset (not
    bf16-exact).  Row r of part p lies on the segment between a random centroid a and a's
    nearest other centroid b, eps_r (c_b - c_a) past their midpoint, eps_r = +-2^-e with e a
    uniform integer of [e_lo, e_hi]; computed in float64, then rounded to float32.  The
    real gap between a and b is 2 |eps_r| ||c_b - c_a||^2.  `cent`: these centroids instead."""
    rng = np.random.default_rng(seed)
    if cent is None:
        cent = (rng.normal(0.0, 1.0, (m, k, dsub)) + offset).astype(np.float32)
    k = cent.shape[1]
    x = np.empty((n, m * dsub), np.float32)
    for p in range(m):
        c = cent[p].astype(np.float64)
        a = rng.integers(0, k, n)
        b = nearest_other(cent[p])[a]
        e = rng.integers(e_lo, e_hi + 1, n)
        eps = np.ldexp(1.0, -e) * rng.choice((-1.0, 1.0), n)
        row = (c[a] + c[b]) / 2 + eps[:, None] * (c[b] - c[a])
        x[:, p * dsub:(p + 1) * dsub] = row.astype(np.float32)
    return x, cent


def dup_k4096(dsub: int, m: int, seed: int):
    """(m, 4096, dsub) centroids: 2,048 N(0, 1) rows and their copies plus N(0, 2^-12)"""
    rng = np.random.default_rng(seed)
    base = rng.normal(0.0, 1.0, (m, 2048, dsub))
    twin = base + rng.normal(0.0, 2.0 ** -12, base.shape)
    return np.ascontiguousarray(np.concatenate([base, twin], axis=1).astype(np.float32))


def scaled(a: np.ndarray, s: int) -> np.ndarray:
    """a 2^s in float32 (exact unless it overflows or leaves the normal range)"""
    with np.errstate(over="ignore", under="ignore"):
        return np.ldexp(a, s).astype(np.float32)


def direct_dists(x_part: np.ndarray, cent_part: np.ndarray) -> np.ndarray:
    """(n, k) fp32 direct-form distances as the oracle forms them: the difference, its
    square and the running sum each rounded to fp32, j ascending"""
    x = np.ascontiguousarray(x_part, np.float32)
    c = np.ascontiguousarray(cent_part, np.float32)
    acc = np.zeros((x.shape[0], c.shape[0]), np.float32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for j in range(x.shape[1]):
            diff = x[:, j, None] - c[None, :, j]
            acc = acc + diff * diff
    return acc


def direct_gap(x_part: np.ndarray, cent_part: np.ndarray):
    """(fp32 first-minimum argmin, gap between the two smallest fp32 distances) per row"""
    d = direct_dists(x_part, cent_part)
    two = np.partition(d, 1, axis=1)[:, :2]
    return d.argmin(1), (two[:, 1].astype(np.float64) - two[:, 0].astype(np.float64))


def argmin64(x_part: np.ndarray, cent_part: np.ndarray) -> np.ndarray:
    """argmin of the float64 distances of the same float32 inputs"""
    x = x_part.astype(np.float64)
    c = cent_part.astype(np.float64)
    return ((x[:, None, :] - c[None, :, :]) ** 2).sum(-1).argmin(1)


def tau_doc(x_part: np.ndarray, cent_part: np.ndarray, any_lo: bool) -> np.ndarray:
    """DESIGN.md section 4.1 in float64, per row: tau = 2.2 E0,
    E0 = (any_lo ? 2^-13 : 2^-15) P + 2^-22 Cmax + 2^-17 (2.02 P + 1.01 Cmax + 1.05 X),
    P = sqrt(X) sqrt(Cmax), X = ||x||^2, Cmax = max_k ||c_k||^2."""
    X = (x_part.astype(np.float64) ** 2).sum(1)
    cmax = (cent_part.astype(np.float64) ** 2).sum(1).max()
    P = np.sqrt(X) * np.sqrt(cmax)
    split = (2.0 ** -13 if any_lo else 2.0 ** -15) * P
    e0 = split + 2.0 ** -22 * cmax + 2.0 ** -17 * (2.02 * P + 1.01 * cmax + 1.05 * X)
    return 2.2 * e0


def bf16_rne(a: np.ndarray) -> np.ndarray:
    """float32 -> the nearest bf16 (ties to even), returned as float32; finite inputs"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16
    return u.astype(np.uint32).view(np.float32)


def bf16_split(a: np.ndarray):
    """(hi, lo) as float32: hi = RNE bf16(a), lo = RNE bf16(a - hi)"""
    a = np.ascontiguousarray(a, np.float32)
    hi = bf16_rne(a)
    lo = bf16_rne(a - hi)   # (a - hi is exact in fp32: hi holds a's leading bits)
    return hi, lo


def screen_scores(x_part: np.ndarray, cent_part: np.ndarray, with_lo: bool) -> np.ndarray:
    """(n, k) screening scores ||c||^2 - 2 (xh.ch + xh.cl + xl.ch) from float64 products of
    the split halves (a product of two bf16 values is exact in float64; their sum over dsub
    is rounded at 2^-53 relative).  with_lo False: the xl.ch term is left out."""
    xh, xl = bf16_split(x_part)
    ch, cl = bf16_split(cent_part)
    xh, xl, ch, cl = (v.astype(np.float64) for v in (xh, xl, ch, cl))
    dot = xh @ ch.T + xh @ cl.T
    if with_lo:
        dot = dot + xl @ ch.T
    return (cent_part.astype(np.float64) ** 2).sum(1)[None, :] - 2.0 * dot


def real_scores(x_part: np.ndarray, cent_part: np.ndarray) -> np.ndarray:
    """(n, k) D_real - X = ||c||^2 - 2 x.c in float64"""
    x = x_part.astype(np.float64)
    c = cent_part.astype(np.float64)
    return (c ** 2).sum(1)[None, :] - 2.0 * (x @ c.T)


def split_remainder(cent_part: np.ndarray) -> float:
    """R = max_k ||c_k - ch_k - cl_k|| in float64"""
    ch, cl = bf16_split(cent_part)
    r = cent_part.astype(np.float64) - ch.astype(np.float64) - cl.astype(np.float64)
    return float(np.sqrt((r ** 2).sum(1).max()))


# ---- k-means cases (test_gpu_kmeans.py; the empty-cluster count in test_assign_cpu.py) ----
def kmeans_case(n: int, d: int, m: int, k: int, seed: int = 4):
    """(x (n, d), init (m, k, dsub)): N(0, 1) rows with negative values; the initial
    centroids are rows of x (drawn with replacement when k > n, plus N(0, 0.5) then, so
    that they differ)"""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1.0, (n, d)).astype(np.float32)
    rows = rng.choice(n, k, replace=k > n)
    ds = d // m
    init = x[rows].reshape(k, m, ds).transpose(1, 0, 2).astype(np.float64)
    if k > n:
        init = init + rng.normal(0.0, 0.5, init.shape)
    return x, np.ascontiguousarray(init.astype(np.float32))


def kmeans_lds_bytes(k: int, dsub: int) -> int:
    """what kmeans_accum's LDS form needs: k dsub 8-byte sums and k 4-byte counts; the host
    takes the LDS form up to 48 KB = 49,152 B"""
    return k * dsub * 8 + k * 4


def cluster_sizes(codes: np.ndarray, k: int) -> np.ndarray:
    """(m, k) members per cluster"""
    return np.stack([np.bincount(codes[:, i], minlength=k) for i in range(codes.shape[1])])


def strided(torch, x: np.ndarray, pad: int, fill=float("nan")):
    """x as the first d columns of a `fill`-filled (n, d + pad) device tensor"""
    n, d = x.shape
    wide = torch.full((n, d + pad), fill, dtype=torch.float32, device="cuda")
    wide[:, :d] = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    view = wide[:, :d]
    assert view.stride(0) == d + pad
    return view
