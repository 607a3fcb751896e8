"""Host-side parts of the rotated index (pqh_rotation_*, pqh_rotate, pqh_cross_moments,
codec.Rotation / opq_train): the calls are exported, declared and bound, the argument errors
that need no device are told without one, and the numpy reference the GPU tests compare against
(tests/opq_ref.py) is checked against integer arithmetic, against its own host steps and against
the conditions the training is built for.  No GPU calls."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import opq_ref
from conftest import ROOT
from pq_huffman_amd import capi, codec

NEW_CALLS = ["pqh_rotation_create", "pqh_rotation_destroy", "pqh_rotate", "pqh_cross_moments"]
WORLD = dict(n=4000, d=32, decay=0.85, seed=3, mix=True)
M, K, OUTER, INNER = 8, 64, 8, 2


def test_opq_calls_are_exported_declared_and_bound():
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    header = open(os.path.join(ROOT, "include", "pqh.h")).read()
    bound = {name for name, _, _ in capi.SIGNATURES}
    for name in NEW_CALLS:
        assert name in exported and name in bound and f"int {name}(" in header, name
        assert getattr(capi.lib(), name).argtypes
    assert "#define PQH_ROT_MAX_D 1024" in header
    for name in ("Rotation", "cross_moments", "procrustes", "pca_rotation", "opq_train"):
        assert callable(getattr(codec, name))
    for name in ("apply", "defect", "close"):
        assert callable(getattr(codec.Rotation, name))
    assert "rotation" in codec.IVF.build.__code__.co_varnames


def test_argument_errors_need_no_device():
    """pqh.h: the argument checks of these calls come before the context is looked at, so a
    process with or without a GPU is told the same"""
    L = capi.lib()
    rot = ctypes.c_void_p()
    R = np.eye(4, dtype=np.float32)
    rp = R.ctypes.data_as(ctypes.c_void_p)
    assert L.pqh_rotation_create(None, rp, 0, ctypes.byref(rot)) == -1
    assert L.pqh_rotation_create(None, rp, -3, ctypes.byref(rot)) == -1
    assert L.pqh_rotation_create(None, rp, 1025, ctypes.byref(rot)) == -4
    assert L.pqh_rotation_create(None, None, 4, ctypes.byref(rot)) == -1
    assert L.pqh_rotation_create(None, rp, 4, None) == -1
    assert not rot.value
    # with nothing wrong but the context: as every call that takes one
    assert L.pqh_rotation_create(None, rp, 4, ctypes.byref(rot)) in (-1, -2)
    assert L.pqh_rotation_destroy(None) == 0
    assert L.pqh_rotate(None, None, rp, 1, 4, rp, 4, 0) == -1          # no rotation
    out = np.zeros((4, 4), np.float64)
    op = out.ctypes.data_as(ctypes.c_void_p)
    f = L.pqh_cross_moments
    assert f(None, rp, 4, 4, 4, rp, 4, 4, None) == -1                   # no output
    assert f(None, None, 4, 4, 4, rp, 4, 4, op) == -1                   # rows but no x
    assert f(None, rp, 4, 4, 4, None, 4, 4, op) == -1
    assert f(None, rp, -1, 4, 4, rp, 4, 4, op) == -1
    assert f(None, rp, 4, 3, 4, rp, 4, 4, op) == -1                     # ld_x < dx
    assert f(None, rp, 4, 4, 4, rp, 3, 4, op) == -1                     # ld_y < dy
    assert f(None, rp, 4, 4, 0, rp, 4, 4, op) == -1
    assert f(None, rp, 4, 4, 4, rp, 4, 0, op) == -1
    assert f(None, rp, 4, 1025, 1025, rp, 4, 4, op) == -4
    assert f(None, rp, 4, 4, 4, rp, 1025, 1025, op) == -4
    assert f(None, rp, 4, 4, 4, rp, 4, 4, op) in (-1, -2)
    assert not out.any()


def test_reference_is_exact_on_the_integer_grid():
    """small integers: every product and every partial sum is an integer below 2^24, so the
    float32 chain and the fixed-point sums are the int64 results"""
    rng = np.random.default_rng(5)
    for n, d in ((1, 1), (9, 3), (70, 33)):
        x = rng.integers(-8, 9, size=(n, d)).astype(np.float32)
        R = rng.integers(-8, 9, size=(d, d)).astype(np.float32)
        for tr in (False, True):
            got = opq_ref.rotate(x, R, tr)
            assert got.dtype == np.float32
            assert np.array_equal(got.astype(np.int64), opq_ref.rotate_int64(x, R, tr)), (n, d, tr)
    assert not np.array_equal(opq_ref.rotate(x, R), opq_ref.rotate(x, R, True))
    for n, dx, dy in ((1, 1, 1), (50, 7, 3), (600, 16, 20)):
        x = rng.integers(-8, 9, size=(n, dx)).astype(np.float32)
        y = rng.integers(-8, 9, size=(n, dy)).astype(np.float32)
        got = opq_ref.moments(x, y)
        assert got.dtype == np.float64 and got.shape == (dx, dy)
        assert np.array_equal(got, opq_ref.moments_int64(x, y).astype(np.float64)), (n, dx, dy)
    assert not opq_ref.moments(np.zeros((0, 3), np.float32), np.zeros((0, 2), np.float32)).any()
    assert not opq_ref.moments(x, np.zeros_like(y)).any()
    # the exponent: n values of the largest product stay below 2^61, and a zero product has one
    assert opq_ref.moments_shift(0.0, 3.0, 10) == 40
    assert opq_ref.moments_shift(2.0, 4.0, 8) == 61 - 6
    assert opq_ref.moments_shift(3.0, 1.0, 1) == 61 - 2
    assert opq_ref.moments_shift(1e-30, 1e-30, 1) == 100
    assert opq_ref.moments_shift(3e38, 3e38, 1 << 40) == -126


def test_procrustes_gives_the_rotation_back():
    rng = np.random.default_rng(6)
    for d in (3, 32, 64):
        x = rng.normal(size=(500, d))
        q, _ = np.linalg.qr(rng.normal(size=(d, d)))
        for fn in (opq_ref.procrustes, codec.procrustes):
            R = fn(x.T @ (x @ q))                           # X^T X R
            assert R.dtype == np.float32 and R.shape == (d, d)
            assert np.abs(R - q).max() < 1e-5, d
            r64 = R.astype(np.float64)
            assert np.abs(r64.T @ r64 - np.eye(d)).max() < 1e-5


def test_eigenvalue_allocation_fills_every_subspace():
    rng = np.random.default_rng(7)
    for d, m in ((32, 8), (12, 3), (8, 8), (6, 1)):
        for lam in (rng.random(d) * 10, np.zeros(d), 0.5 ** np.arange(d), np.ones(d)):
            taken = opq_ref.allocate(lam, m)
            assert [len(t) for t in taken] == [d // m] * m
            assert sorted(e for t in taken for e in t) == list(range(d))
    # eigenvalues of 1 add log 1 = 0: every sum ties, and ties go to the lower subspace with room
    assert opq_ref.allocate(np.ones(4), 2) == [[0, 1], [2, 3]]
    assert opq_ref.allocate(np.full(4, 2.0), 2) == [[0, 2], [1, 3]]
    # a decaying spectrum: the largest goes with the smallest
    assert opq_ref.allocate([8.0, 4.0, 2.0, 1.0], 2) == [[0, 3], [1, 2]]
    x = opq_ref.spectrum_world(**WORLD)
    R = opq_ref.pca_rotation(x, M)
    r64 = R.astype(np.float64)
    assert np.abs(r64.T @ r64 - np.eye(32)).max() < 1e-5
    # the rotated columns are the principal axes in the allocated order: their variances are the
    # eigenvalues, column by column (float32 rows and a float32 R: far inside 1e-3)
    x64 = x.astype(np.float64)
    lam = np.linalg.eigvalsh(np.cov(x64.T, bias=True))
    cols = [e for t in opq_ref.allocate(lam, M) for e in t]
    var = opq_ref.rotate(x, R).astype(np.float64).var(axis=0)
    assert np.allclose(var, lam[cols], rtol=1e-3), np.abs(var / lam[cols] - 1).max()


@pytest.fixture(scope="module")
def trained(oracle):
    x = opq_ref.spectrum_world(**WORLD)
    init = opq_ref.init_rows(x, M, K, 11)
    plain = oracle.kmeans(x, init, (OUTER + 1) * INNER)
    plain_err = oracle.compute_error(x, plain, oracle.pq_assign(x, plain)[0])
    ident = opq_ref.train(oracle, x, M, K, init, OUTER, INNER, "identity")
    start = opq_ref.pca_rotation(x, M)
    pca = opq_ref.train(oracle, x, M, K, opq_ref.init_rows(x, M, K, 11, start), OUTER, INNER, "pca")
    return plain_err, ident, pca


def test_reference_training_meets_its_conditions(trained):
    """the world of the prototype: 0.40 from the identity and 0.125 from the PCA start there;
    this reference gives 0.413 and 0.126"""
    plain_err, ident, pca = trained
    for R, cent, errors in (ident, pca):
        assert len(errors) == OUTER + 1 and cent.shape == (M, K, 4)
        for a, b in zip(errors, errors[1:]):
            assert b <= a * (1 + 1e-4), errors
        r64 = R.astype(np.float64)
        assert np.abs(r64.T @ r64 - np.eye(32)).max() < 1e-4
    print("ratios", ident[2][-1] / plain_err, pca[2][-1] / plain_err)
    assert ident[2][-1] <= 0.6 * plain_err, (ident[2][-1], plain_err)
    assert pca[2][-1] <= 0.25 * plain_err, (pca[2][-1], plain_err)
