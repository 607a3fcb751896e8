"""The numpy reference of the rotated index (pqh_rotate, pqh_cross_moments, codec.procrustes,
codec.pca_rotation, codec.opq_train), shared by tests/test_opq_cpu.py, tests/test_gpu_opq.py and
tests/test_gpu_ivf_rotated.py.  Nothing here calls the library; train() takes the CPU oracle
(oracle/oracle_ctypes.py) for the k-means and the assignment.

    rotate(x, R):   acc = +0.0;  for t ascending:  acc = acc + x[t] * R[t][j]
Every step is a float32 array operation of numpy, which rounds the multiply and the add to
float32 each and fuses nothing -- a sequential chain, never a vectorised dot -- so the bits are
those of the definition (metric_ref.nip is the same chain with a subtract).
    moments(x, y):  every product one float32 multiply p, f = rint(p * 2^s) as int64, the f
added as integers, the sum times 2^-s: nothing depends on an order."""
import math

import numpy as np


# ------------------------------------------------------------------------------ the map
def rotate(x, R, transpose=False):
    """float32 [n][d]: out[v][j] = sum_t x[v][t] * R[t][j] (transpose: R[j][t]), one column of
    x a step"""
    x = np.ascontiguousarray(x, np.float32)
    R = np.ascontiguousarray(R, np.float32)
    if transpose:
        R = np.ascontiguousarray(R.T)
    acc = np.zeros((x.shape[0], R.shape[1]), np.float32)
    for t in range(R.shape[0]):
        acc = acc + x[:, t:t + 1] * R[t][None, :]
    assert acc.dtype == np.float32
    return acc


def rotate_int64(x, R, transpose=False):
    """the same in int64 arithmetic, for integer-valued inputs"""
    R = np.asarray(R).astype(np.int64)
    return np.asarray(x).astype(np.int64) @ (R.T if transpose else R)


# ------------------------------------------------------------------------------ the sums
def moments_shift(max_x, max_y, n):
    """61 - ceil(log2(max|x| * max|y| * n)) on doubles, clamped to [-126, 100]; 40 when the
    product is 0 (pqh_kmeans_train's exponent with max|x| * max|y| for max|x|)"""
    p = float(max_x) * float(max_y)
    if not p > 0.0 or n <= 0:
        return 40
    if math.isinf(p):
        return -126
    return max(-126, min(100, 61 - math.ceil(math.log2(p * float(n)))))


def moments(x, y):
    """float64 [dx][dy]: M[a][b] = sum_v x[v][a] * y[v][b] in 64-bit fixed point"""
    x = np.ascontiguousarray(x, np.float32)
    y = np.ascontiguousarray(y, np.float32)
    n = x.shape[0]
    if n == 0:
        return np.zeros((x.shape[1], y.shape[1]), np.float64)
    s = moments_shift(np.abs(x).max(), np.abs(y).max(), n)
    total = np.zeros((x.shape[1], y.shape[1]), np.int64)
    for v0 in range(0, n, 256):   # (in slabs of rows: integer sums, so the split is free)
        p = x[v0:v0 + 256, :, None] * y[v0:v0 + 256, None, :]
        assert p.dtype == np.float32
        total += np.rint(np.ldexp(p.astype(np.float64), s)).astype(np.int64).sum(axis=0)
    return np.ldexp(total.astype(np.float64), -s)


def moments_int64(x, y):
    return np.asarray(x).astype(np.int64).T @ np.asarray(y).astype(np.int64)


# ------------------------------------------------------------------------------ the host steps
def procrustes(M):
    """float32 [d][d]: U @ Vt of M's singular value decomposition"""
    u, _, vt = np.linalg.svd(np.asarray(M, np.float64))
    return (u @ vt).astype(np.float32)


def allocate(lam, m):
    """the eigenvalue allocation: the indices of lam, subspace by subspace.  Eigenvalues
    descending (stable), each to the subspace with room whose sum of log max(lam, tiny) is
    smallest so far, ties to the lower subspace"""
    lam = np.asarray(lam, np.float64)
    dsub = len(lam) // m
    tiny = np.finfo(np.float64).tiny
    taken = [[] for _ in range(m)]
    logs = np.zeros(m, np.float64)
    for e in np.argsort(-lam, kind="stable"):
        room = [i for i in range(m) if len(taken[i]) < dsub]
        best = min(room, key=lambda i: (logs[i], i))
        taken[best].append(int(e))
        logs[best] += np.log(max(lam[e], tiny))
    return taken


def pca_rotation(x, m, second=None, sums=None):
    """float32 [d][d] from the reference's own moments; second / sums: moments computed
    elsewhere (X^T X and the column sums), to compare the host steps alone"""
    x = np.ascontiguousarray(x, np.float32)
    n = x.shape[0]
    if sums is None:
        sums = moments(x, np.ones((n, 1), np.float32))[:, 0]
    if second is None:
        second = moments(x, x)
    mu = sums / n
    cov = second / n - np.outer(mu, mu)
    lam, vec = np.linalg.eigh(cov)
    cols = [e for t in allocate(lam, m) for e in t]
    return np.ascontiguousarray(vec[:, cols]).astype(np.float32)


def reconstruct(cent, codes):
    """float32 [n][m * dsub]: the gather of every part's centroid"""
    return np.concatenate([cent[i][codes[:, i]] for i in range(cent.shape[0])], axis=1)


def train(oracle, x, m, k, cent_init, outer=8, inner=2, init="identity", trace=None):
    """(R, centroids, errors): codec.opq_train's loop over oracle.kmeans, oracle.pq_assign and
    a gather"""
    x = np.ascontiguousarray(x, np.float32)
    d = x.shape[1]
    if isinstance(init, str):
        R = np.eye(d, dtype=np.float32) if init == "identity" else pca_rotation(x, m)
    else:
        R = np.ascontiguousarray(init, np.float32)
    cent = np.ascontiguousarray(cent_init, np.float32)
    errors = []
    for it in range(outer + 1):
        xr = rotate(x, R)
        cent = oracle.kmeans(xr, cent, inner)
        codes, _ = oracle.pq_assign(xr, cent)
        errors.append(oracle.compute_error(xr, cent, codes))
        if trace is not None:
            trace.append(dict(R=R, cent=cent, err=errors[-1], M=None))
        if it == outer:
            break
        M = moments(x, reconstruct(cent, codes))
        if trace is not None:
            trace[-1]["M"] = M
        R = procrustes(M)
    return R, cent, errors


# ------------------------------------------------------------------------------ the world
def spectrum_world(n, d, decay, seed, mix):
    """float32 [n][d]: 64 Gaussian centres plus 0.7 * N(0, 1) noise, column j scaled by
    decay**j, times a fixed-seed orthonormal Q (np.linalg.qr of a Gaussian matrix) when mix,
    times 64"""
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, 1.0, size=(64, d))
    x = centres[rng.integers(0, 64, size=n)] + 0.7 * rng.normal(0.0, 1.0, size=(n, d))
    x = x * decay ** np.arange(d)
    if mix:
        q, _ = np.linalg.qr(np.random.default_rng(1234).normal(0.0, 1.0, size=(d, d)))
        x = x @ q
    return (x * 64.0).astype(np.float32)


def init_rows(x, m, k, seed, R=None):
    """[m][k][dsub]: k rows of x chosen by seed, rotated by R (None: as they are), cut into m
    parts -- centroids of the rotated space to start opq_train from"""
    rows = np.random.default_rng(seed).choice(x.shape[0], k, replace=False)
    start = x[rows] if R is None else rotate(x[rows], R)
    return np.ascontiguousarray(start.reshape(k, m, x.shape[1] // m).transpose(1, 0, 2))


def exact_knn(x, q, k):
    """ids int64 [nq][k]: the exact L2 neighbours in float64, ties to the smaller id"""
    x64, q64 = np.asarray(x, np.float64), np.asarray(q, np.float64)
    ids = np.arange(x.shape[0])
    out = []
    for v in q64:
        dist = ((x64 - v) ** 2).sum(axis=1)
        out.append(np.lexsort((ids, dist))[:k])
    return np.stack(out)
