"""GPU Lloyd k-means (pqh_kmeans_train, pq_train_rows) against the oracle's sequential
restatement, bit for bit, at the shapes the suite did not reach: both kmeans_accum forms
without LDS sums, the block split of the accumulation, strided rows, the clamp of the
fixed-point shift, clusters that stay empty, and the trivial calls."""
import ctypes

import numpy as np
import pytest

import assign_ref as ar

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    from pq_huffman_amd import codec
    assert torch.cuda.is_available()
    ctx = codec.Context(0)
    return torch, codec, ctx


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _train(gpu, x, init, iters):
    torch, codec, ctx = gpu
    return codec.kmeans_train(ctx, torch.from_numpy(np.ascontiguousarray(x)).cuda(), init, iters)


# (n, d, m, k, iters, LDS form?)
TABLE = [(5000, 46, 2, 256, 2, True), (5000, 48, 2, 256, 2, False), (5000, 64, 2, 256, 2, False),
         (3000, 32, 2, 4096, 2, False), (9000, 128, 1, 64, 3, False)]


@pytest.mark.parametrize("n,d,m,k,iters,lds", TABLE)
def test_kmeans_accum_forms(gpu, oracle, n, d, m, k, iters, lds):
    """kmeans_accum<CodeT, LDS> keeps its sums in LDS while k dsub 8 + k 4 <= 49,152 B:
      (5000, 46, 2, 256)   dsub 23: 48,128 B, the last LDS shape          <u8, true>
      (5000, 48, 2, 256)   dsub 24: 50,176 B, the first without           <u8, false>
      (5000, 64, 2, 256)   dsub 32: 66,560 B, MFMA assignment             <u8, false>
      (3000, 32, 2, 4096)  dsub 16: 540,672 B, u16 codes, MFMA assignment <u16, false>
      (9000, 128, 1, 64)   dsub 128: 65,792 B, the coarse-codebook shape  <u8, false>
    (<u16, true> is (2500, 64, 8, 300) of test_gpu_pq.py.)  n < k in the fourth leaves
    clusters empty at every iteration; they keep their bits (test_assign_cpu.py counts them)."""
    assert (ar.kmeans_lds_bytes(k, d // m) <= 48 * 1024) == lds
    x, init = ar.kmeans_case(n, d, m, k)
    want = oracle.kmeans(x, init, iters, threads=0)
    got = _train(gpu, x, init, iters)
    assert np.array_equal(_bits(got), _bits(want)), (_bits(got) != _bits(want)).sum()
    if n < k:
        last = oracle.kmeans(x, init, iters - 1, threads=0)
        empty = ar.cluster_sizes(oracle.pq_assign(x, last, threads=0)[0], k) == 0
        assert empty.sum() > 1000
        assert np.array_equal(_bits(got[empty]), _bits(last[empty]))


@pytest.mark.parametrize("n", [4095, 8191, 8192, 12289])
def test_kmeans_block_split(gpu, oracle, n):
    """the accumulation's grid is bx = clamp(n / 4096, 1, 256) blocks per subspace, each over
    ceil(n / bx) rows: 1 block below 8,192 rows, 2 at 8,192, 3 with a short last one at 12,289"""
    x, init = ar.kmeans_case(n, 32, 4, 16, seed=n)
    want = oracle.kmeans(x, init, 2, threads=0)
    got = _train(gpu, x, init, 2)
    assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("d,m,k", [(32, 2, 256), (48, 2, 256)])
def test_kmeans_strided_rows(gpu, oracle, d, m, k):
    """ld_x = d + 3 with NaN gaps, through the absmax, assignment and accumulation kernels (LDS
    sums at dsub 16, global ones at dsub 24): a gap float read would make the shift -126"""
    torch, codec, ctx = gpu
    x, init = ar.kmeans_case(5000, d, m, k, seed=9)
    want = oracle.kmeans(x, init, 2, threads=0)
    got = codec.kmeans_train(ctx, ar.strided(torch, x, 3), init, 2)
    assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("s", [-120, 100])
def test_kmeans_shift_clamp(gpu, oracle, s):
    """pqh_kmeans_fixed_shift clamps to [-126, 100].  x 2^-120: the shift clamps at 100, every
    fixed-point term rounds to 0 and every square underflows (all rows in cluster 0, whose
    mean is 0).  x 2^100: a negative shift, and every squared distance but a row's to itself
    overflows, so nearly all rows go to code 0.  The data has negative values; the oracle's
    centroids are finite for both (test_assign_cpu.py)."""
    x0, i0 = ar.kmeans_case(3000, 32, 2, 256)
    x, init = ar.scaled(x0, s), ar.scaled(i0, s)
    assert (x < 0).any()
    want = oracle.kmeans(x, init, 2, threads=0)
    assert np.isfinite(want).all()
    got = _train(gpu, x, init, 2)
    assert np.array_equal(_bits(got), _bits(want)), (_bits(got) != _bits(want)).sum()


def test_kmeans_trivial_calls(gpu):
    """iters = 0 and n = 0 return the initial centroids unchanged"""
    torch, codec, ctx = gpu
    x, init = ar.kmeans_case(300, 32, 2, 256)
    assert np.array_equal(_bits(_train(gpu, x, init, 0)), _bits(init))
    none = torch.empty((0, 32), dtype=torch.float32, device="cuda")
    assert np.array_equal(_bits(codec.kmeans_train(ctx, none, init, 3)), _bits(init))


def _cb_struct():
    class CB(ctypes.Structure):   # pq.h centroids_codebook_t
        _fields_ = [("num_clusters", ctypes.c_int), ("num_dimensions", ctypes.c_int),
                    ("num_parts", ctypes.c_int), ("centroids_pool", ctypes.c_void_p),
                    ("centroids", ctypes.c_void_p)]
    return CB


@pytest.mark.parametrize("chunk", [1000, 1024])
def test_streamed_trainer_without_lds_sums(gpu, oracle, chunk):
    """pq_train_rows on the (5000, 64, 2, 256) shape (sums in global memory): a chunk is
    rounded down to whole 256-row blocks, so 1,000 asks for 768 rows (a last chunk of 392)
    and 1,024 ends on a short chunk of 904; either way the sums are exact integers and the
    result is the one-shot trainer's bit for bit."""
    from pq_huffman_amd.capi import lib
    n, d, m, k = 5000, 64, 2, 256
    x, init = ar.kmeans_case(n, d, m, k)
    cent = init.copy()
    cb = _cb_struct()(k, d // m, m, cent.ctypes.data, None)
    seen = []
    fn_t = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_longlong,
                            ctypes.c_void_p)

    def read(_user, row0, rows, dst):
        ctypes.memmove(dst, x[row0:row0 + rows].ctypes.data, rows * d * 4)
        seen.append(rows)
        return 0
    assert lib().pq_train_rows(ctypes.byref(cb), d, n, fn_t(read), None, 2, chunk) == 0
    assert sum(seen) == 3 * n and max(seen) == chunk // 256 * 256   # absmax + 2 iterations
    assert seen[-1] == n % (chunk // 256 * 256)
    one = _train(gpu, x, init, 2)
    assert np.array_equal(_bits(cent), _bits(one))
    assert np.array_equal(_bits(cent), _bits(oracle.kmeans(x, init, 2, threads=0)))
