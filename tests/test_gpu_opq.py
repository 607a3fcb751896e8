"""pqh_rotate, pqh_cross_moments, codec.pca_rotation and codec.opq_train on the GPU against the
numpy reference of tests/opq_ref.py: floats are compared on their raw bits, the float64 moments
with array_equal (they are exact integers times a power of two)."""
import numpy as np
import pytest

import opq_ref

pytestmark = pytest.mark.gpu

WORLD = dict(n=4000, d=32, decay=0.85, seed=3, mix=True)
M, K, INNER = 8, 64, 2


@pytest.fixture(scope="module")
def gpu():
    import torch
    from pq_huffman_amd import codec
    assert torch.cuda.is_available()
    return torch, codec, codec.Context(0)


def _bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


# the row tile of the kernel is 128: 127, 128 and 129 rows, several tiles, one column tile and
# more (d > 128), d no multiple of the 32 staged steps, the widest map
ROTATE_SHAPES = [(0, 8), (1, 1), (127, 3), (128, 64), (129, 33), (300, 63), (300, 65), (300, 128),
                 (130, 129), (70, 1024)]


@pytest.mark.parametrize("n,d", ROTATE_SHAPES)
def test_rotate_equals_the_chain(gpu, n, d):
    torch, codec, ctx = gpu
    rng = np.random.default_rng(1000 * n + d)
    x = rng.normal(size=(n, d)).astype(np.float32)
    R = rng.normal(size=(d, d)).astype(np.float32)       # dense, not orthonormal
    rot = codec.Rotation(ctx, R)
    assert rot.d == d and np.array_equal(rot.R, R)
    xd = torch.from_numpy(x).cuda()
    for tr in (False, True):
        got = rot.apply(xd, transpose=tr)
        assert got.shape == (n, d) and got.dtype == torch.float32
        want = opq_ref.rotate(x, R, tr)
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), (n, d, tr)
    if d > 1 and n > 0:
        assert not np.array_equal(opq_ref.rotate(x, R), opq_ref.rotate(x, R, True))
    rot.close()


def test_rotate_leaves_the_gaps_between_rows_alone(gpu):
    """ld_x = d + 5 with NaN between the rows of x (never read), ld_out = d + 3 with a sentinel
    between the rows of out (never written)"""
    torch, codec, ctx = gpu
    n, d = 257, 100
    rng = np.random.default_rng(8)
    x = rng.normal(size=(n, d)).astype(np.float32)
    R = rng.normal(size=(d, d)).astype(np.float32)
    wide = torch.full((n, d + 5), float("nan"), dtype=torch.float32, device="cuda")
    wide[:, :d] = torch.from_numpy(x).cuda()
    rot = codec.Rotation(ctx, R)
    for tr in (False, True):
        out = torch.full((n, d + 3), 12345.0, dtype=torch.float32, device="cuda")
        assert rot.apply(wide[:, :d], out=out[:, :d], transpose=tr).data_ptr() == out.data_ptr()
        got = out.cpu().numpy()
        assert (got[:, d:] == 12345.0).all()
        assert np.array_equal(_bits(got[:, :d]), _bits(opq_ref.rotate(x, R, tr))), tr
    rot.close()


def test_rotate_is_exact_on_the_integer_grid(gpu):
    torch, codec, ctx = gpu
    rng = np.random.default_rng(9)
    x = rng.integers(-8, 9, size=(200, 40)).astype(np.float32)
    R = rng.integers(-8, 9, size=(40, 40)).astype(np.float32)
    rot = codec.Rotation(ctx, R)
    for tr in (False, True):
        got = rot.apply(torch.from_numpy(x).cuda(), transpose=tr).cpu().numpy()
        assert np.array_equal(got.astype(np.int64), opq_ref.rotate_int64(x, R, tr))
    assert rot.defect() > 1.0
    # rows nearer than d floats, a direction that is none, rows but no buffer: refused at once
    from pq_huffman_amd import capi
    xd, out = torch.from_numpy(x).cuda(), torch.empty((200, 40), dtype=torch.float32, device="cuda")
    f, xp, op = capi.lib().pqh_rotate, xd.data_ptr(), out.data_ptr()
    assert f(ctx.ptr, rot.ptr, xp, 200, 39, op, 40, 0) == -1
    assert f(ctx.ptr, rot.ptr, xp, 200, 40, op, 39, 0) == -1
    assert f(ctx.ptr, rot.ptr, xp, 200, 40, op, 40, 2) == -1
    assert f(ctx.ptr, rot.ptr, xp, -1, 40, op, 40, 0) == -1
    assert f(ctx.ptr, rot.ptr, None, 200, 40, op, 40, 0) == -1
    assert f(ctx.ptr, rot.ptr, xp, 200, 40, None, 40, 0) == -1
    assert f(ctx.ptr, rot.ptr, None, 0, 40, None, 40, 0) == 0
    rot.close()
    eye = codec.Rotation(ctx, np.eye(7, dtype=np.float32))
    assert eye.defect() == 0.0
    eye.close()
    with pytest.raises(codec.PqhError):
        codec.Rotation(ctx, np.zeros((1025, 1025), np.float32))
    with pytest.raises(codec.PqhError):
        codec.Rotation(ctx, np.zeros((3, 4), np.float32))


MOMENT_SHAPES = [(1, 1, 1), (257, 33, 1), (5000, 32, 32), (300, 128, 100), (64, 1024, 3)]


@pytest.mark.parametrize("n,dx,dy", MOMENT_SHAPES)
def test_cross_moments_equal_the_fixed_point_sums(gpu, n, dx, dy):
    torch, codec, ctx = gpu
    rng = np.random.default_rng(n + dx + dy)
    x = (rng.normal(size=(n, dx)) * 37.0).astype(np.float32)
    y = (rng.normal(size=(n, dy)) * 0.3).astype(np.float32)
    want = opq_ref.moments(x, y)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    got = codec.cross_moments(ctx, xd, yd)
    assert got.dtype == np.float64 and got.shape == (dx, dy)
    assert np.array_equal(got, want), np.abs(got - want).max()
    assert np.array_equal(codec.cross_moments(ctx, xd, yd), got)       # twice: equal bits
    # rows further apart, NaN between them
    xw = torch.full((n, dx + 3), float("nan"), dtype=torch.float32, device="cuda")
    yw = torch.full((n, dy + 7), float("nan"), dtype=torch.float32, device="cuda")
    xw[:, :dx], yw[:, :dy] = xd, yd
    assert np.array_equal(codec.cross_moments(ctx, xw[:, :dx], yw[:, :dy]), want)
    if dx == dy:                                                       # X^T X from one buffer
        assert np.array_equal(codec.cross_moments(ctx, xd, xd), opq_ref.moments(x, x))


def test_cross_moments_edges(gpu):
    torch, codec, ctx = gpu
    rng = np.random.default_rng(12)
    x = rng.integers(-8, 9, size=(700, 70)).astype(np.float32)
    y = rng.integers(-8, 9, size=(700, 5)).astype(np.float32)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    got = codec.cross_moments(ctx, xd, yd)
    assert np.array_equal(got, opq_ref.moments_int64(x, y).astype(np.float64))
    assert np.array_equal(got, opq_ref.moments(x, y))
    zero = codec.cross_moments(ctx, xd, torch.zeros_like(yd))
    assert zero.shape == (70, 5) and not zero.any() and not np.signbit(zero).any()
    none = codec.cross_moments(ctx, xd[:0], yd[:0])
    assert none.shape == (70, 5) and not none.any()
    # the column sums, as pca_rotation takes them
    ones = torch.ones((700, 1), dtype=torch.float32, device="cuda")
    assert np.array_equal(codec.cross_moments(ctx, xd, ones)[:, 0], x.astype(np.float64).sum(axis=0))
    with pytest.raises(codec.PqhError):
        codec.cross_moments(ctx, xd, yd[:10])


@pytest.fixture(scope="module")
def world(gpu):
    torch, codec, ctx = gpu
    x = opq_ref.spectrum_world(**WORLD)
    return x, torch.from_numpy(x).cuda()


def test_opq_train_follows_the_reference_step_by_step(gpu, oracle, world):
    """every traced round against the oracle's k-means of the reference's rotation, the
    reference's moments and the same numpy Procrustes on bit-equal input"""
    torch, codec, ctx = gpu
    x, xd = world
    init = opq_ref.init_rows(x, M, K, 11)
    trace = []
    R, cent, errors = codec.opq_train(ctx, xd, M, K, init, outer=3, inner=INNER, trace=trace)
    assert len(trace) == len(errors) == 4
    assert np.array_equal(trace[0]["R"], np.eye(32, dtype=np.float32))
    assert np.array_equal(R, trace[-1]["R"]) and np.array_equal(cent, trace[-1]["cent"])
    prev = init
    for it, step in enumerate(trace):
        xr = opq_ref.rotate(x, step["R"])
        want = oracle.kmeans(xr, prev, INNER)
        assert np.array_equal(_bits(step["cent"]), _bits(want)), it
        codes = oracle.pq_assign(xr, want)[0]
        err = oracle.compute_error(xr, want, codes)
        # the device adds 256-row partial sums in double, the oracle row by row: 4,000 roundings
        # of 2^-53 at the most, the tolerance of test_gpu_pq.test_error_and_reconstruct
        assert abs(step["err"] - err) <= 1e-12 * err and errors[it] == step["err"], it
        if it == 3:
            assert step["M"] is None
            break
        assert np.array_equal(step["M"], opq_ref.moments(x, opq_ref.reconstruct(want, codes))), it
        assert np.array_equal(_bits(trace[it + 1]["R"]), _bits(opq_ref.procrustes(step["M"]))), it
        prev = want
    for step in trace:
        rot = codec.Rotation(ctx, step["R"])
        assert rot.defect() < 1e-4
        rot.close()
    for a, b in zip(errors, errors[1:]):
        assert b <= a * (1 + 1e-4), errors


def test_pca_rotation_equals_the_reference(gpu, oracle, world):
    torch, codec, ctx = gpu
    x, xd = world
    second = codec.cross_moments(ctx, xd, xd)
    sums = codec.cross_moments(ctx, xd, torch.ones((len(x), 1), dtype=torch.float32, device="cuda"))
    assert np.array_equal(second, opq_ref.moments(x, x))
    assert np.array_equal(sums, opq_ref.moments(x, np.ones((len(x), 1), np.float32)))
    want = opq_ref.pca_rotation(x, M)
    got = codec.pca_rotation(ctx, xd, M)
    assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(want))
    # and it is where opq_train(init="pca") starts
    trace = []
    start = opq_ref.init_rows(x, M, K, 11, want)
    R, cent, errors = codec.opq_train(ctx, xd, M, K, start, outer=0, inner=INNER, init="pca",
                                      trace=trace)
    assert np.array_equal(_bits(R), _bits(want)) and len(errors) == 1
    assert np.array_equal(_bits(cent), _bits(oracle.kmeans(opq_ref.rotate(x, want), start, INNER)))
    with pytest.raises(codec.PqhError):
        codec.opq_train(ctx, xd, M, K, start, init="nothing")
    with pytest.raises(codec.PqhError):
        codec.opq_train(ctx, xd, 5, K, start)
