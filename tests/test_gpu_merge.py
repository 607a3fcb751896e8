"""The top-k merge on the GPU (pqh_topk_merge through codec.merge_topk) and, in one process, the
search over row blocks of one data set merged with it: the kernel against the numpy merge
(tests/merge_ref.py) with exact equality of both outputs, the merged search against one index
over all rows -- distances on their raw bits, ids wherever a query's distances are distinct --
and shard.ShardedIVF on one rank against its local index."""
import numpy as np
import pytest

import merge_ref as mref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    from pq_huffman_amd import codec
    assert torch.cuda.is_available()
    return torch, codec, codec.Context(0), codec.Context(0).set_search_max_k(256)


def _bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


def _status(fn):
    from pq_huffman_amd.capi import PqhError
    try:
        fn()
    except PqhError as err:
        return err.status
    return 0


def _same(got, want, what):
    gd, gi = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert np.array_equal(_bits(gd), _bits(want[0])), what
    assert np.array_equal(gi, want[1]), what


# ------------------------------------------------------------------------------ the kernel
# (parts, nq, k_in, top_k, bases, a context raised to 256)
SHAPES = [
    (1, 1, 1, 1, None, False),
    (1, 5, 64, 64, [1 << 40], False),
    (2, 5, 64, 64, [0, 1000], False),
    (3, 7, 10, 64, [0, 50, 1 << 33], False),       # fewer valid entries than top_k: padding out
    (5, 3, 63, 17, [3, 0, 9, 1, 7], False),
    (17, 2, 64, 64, list(range(0, 1700, 100)), False),
    (2, 1, 300, 64, [0, 5000], False),
    (2, 33, 64, 10, [0, 1 << 32], False),            # more than one workgroup, a wave without a query
    (2, 4, 65, 65, [0, 700], True),
    (4, 2, 256, 256, [0, 1 << 35, 9, 100000], True),
    (3, 3, 100, 200, [10, 0, 1 << 31], True),
]


@pytest.mark.parametrize("parts,nq,k_in,top_k,bases,wide", SHAPES)
def test_kernel_equals_numpy(gpu, parts, nq, k_in, top_k, bases, wide):
    torch, codec, ctx, ctx_wide = gpu
    d, i = mref.tied_parts(parts, nq, k_in, seed=1000 * parts + k_in + top_k, bases=bases)
    if parts * k_in >= 60:      # the input's own properties: padding, (finite, -1), ties
        assert (np.isinf(d) & (i < 0)).any() and (np.isfinite(d) & (i < 0)).any()
        assert len(np.unique(d[i >= 0])) <= 8
    want = mref.merge_topk_ref(d, i, bases, top_k)
    if (parts, k_in, top_k) == (3, 10, 64):
        assert (want[1] < 0).any()
    dd, di = torch.from_numpy(d).cuda(), torch.from_numpy(i).cuda()
    c = ctx_wide if wide else ctx
    _same(codec.merge_topk(c, dd, di, top_k, bases), want, "a sequence of bases")
    bt = torch.tensor(bases, dtype=torch.int64, device="cuda") if bases is not None else None
    out = (torch.full((nq, top_k), -7.0, dtype=torch.float32, device="cuda"),
           torch.full((nq, top_k), -7, dtype=torch.int64, device="cuda"))
    got = codec.merge_topk(c, dd, di, top_k, bt, out=out)
    assert got[0] is out[0] and got[1] is out[1]
    _same(got, want, "a tensor of bases, out=")
    if not wide:                # top_k <= 64 is the same kernel whatever the limit is
        _same(codec.merge_topk(ctx_wide, dd, di, top_k, bases), want, "raised limit")
    if top_k == k_in:
        _same(codec.merge_topk(c, dd, di, id_base=bases), want, "k defaults to k_in")


def test_no_bases_and_a_part_of_padding(gpu):
    torch, codec, ctx, _ = gpu
    d, i = mref.tied_parts(3, 5, 40, seed=5)
    d[1], i[1] = np.inf, -1
    i[2, :, ::2] = -1                   # (finite, -1) at every other entry of a part
    want = mref.merge_topk_ref(d, i, None, 16)
    assert (want[1] >= 0).all()
    # ids unique per query only with bases: without them this input still is (tied_parts)
    _same(codec.merge_topk(ctx, torch.from_numpy(d).cuda(), torch.from_numpy(i).cuda(), 16), want,
          "NULL bases")
    d[:], i[:] = np.inf, -1             # nothing valid at all
    got = codec.merge_topk(ctx, torch.from_numpy(d).cuda(), torch.from_numpy(i).cuda(), 64)
    assert np.isinf(got[0].cpu().numpy()).all() and (got[1].cpu().numpy() == -1).all()


def test_limits_and_no_queries(gpu):
    torch, codec, ctx, ctx_wide = gpu
    d, i = mref.tied_parts(2, 3, 70, seed=6)
    dd, di = torch.from_numpy(d).cuda(), torch.from_numpy(i).cuda()
    assert _status(lambda: codec.merge_topk(ctx, dd, di, 65)) == -1            # PQH_ERR_ARG
    assert _status(lambda: codec.merge_topk(ctx, dd, di, 0)) == -1
    assert _status(lambda: codec.merge_topk(ctx_wide, dd, di, 257)) == -1
    _same(codec.merge_topk(ctx_wide, dd, di, 65), mref.merge_topk_ref(d, i, None, 65), "65")
    got = codec.merge_topk(ctx, dd[:, :0], di[:, :0], 10)
    assert got[0].shape == (0, 10) and got[1].shape == (0, 10)
    assert _status(lambda: codec.merge_topk(ctx, dd, di[:, :2], 10)) == -1    # shapes disagree
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------ end to end
N, D, NLIST, NPROBE = 3001, 32, 16, 4
KINDS = {"plain": dict(m=4, residual=False, metric="l2"),
         "residual": dict(m=8, residual=True, metric="l2"),
         "ip": dict(m=4, residual=False, metric="ip")}
SPLITS = {"1": mref.block_starts(N, world=1), "2": mref.block_starts(N, world=2),
          "3": mref.block_starts(N, world=3), "5": mref.block_starts(N, world=5),
          "3000+1": mref.block_starts(N, sizes=[3000, 1])}
_built = {}


def _indices(gpu, kind):
    """the data of a kind, its PQ and coarse quantizer, and one IVF per row block of every split
    (the split "1" is the single index over all rows)"""
    if kind in _built:
        return _built[kind]
    torch, codec, _, ctx = gpu
    spec = KINDS[kind]
    w = mref.search_world(N, D, NLIST, 33, spec["m"], residual=spec["residual"], spread=True)
    w["xd"], w["qd"] = torch.from_numpy(w["x"]).cuda(), torch.from_numpy(w["q"]).cuda()
    w["pq"], w["coarse"] = codec.PQ(ctx, w["cent"]), codec.Coarse(ctx, w["cc"])
    w["ivf"] = {name: [codec.IVF.build(ctx, w["pq"], w["coarse"], w["xd"][b:e], chunk_vectors=8,
                                       residual=spec["residual"], metric=spec["metric"])
                       for b, e in zip(starts[:-1], starts[1:])]
                for name, starts in SPLITS.items()}
    codec.ivf_status(ctx)
    _built[kind] = w
    return w


def _merged(gpu, w, split, nq, k, **kw):
    """(merged GPU result, the per-block GPU results stacked)"""
    torch, codec, _, ctx = gpu
    starts = SPLITS[split]
    keep = kw.pop("keep", None)
    res = []
    for ivf, b, e in zip(w["ivf"][split], starts[:-1], starts[1:]):
        kp = None if keep is None else keep[b:e]
        res.append(ivf.search(w["qd"][:nq], NPROBE, k, keep=kp, **kw))
    ds, is_ = torch.stack([r[0] for r in res]), torch.stack([r[1] for r in res])
    return codec.merge_topk(ctx, ds, is_, k, starts[:-1]), (ds, is_)


def _check_split(gpu, w, split, nq, k, tally, **kw):
    torch, codec, _, ctx = gpu
    got, (ds, is_) = _merged(gpu, w, split, nq, k, **dict(kw))
    what = (split, nq, k, sorted(kw))
    # the kernel: the numpy merge of the very results it was given
    _same(got, mref.merge_topk_ref(ds.cpu().numpy(), is_.cpu().numpy(), SPLITS[split][:-1], k), what)
    # one index over all rows: its distances bit for bit, its ids where distances are distinct
    one = w["ivf"]["1"][0].search(w["qd"][:nq], NPROBE, k, **kw)
    od, oi = one[0].cpu().numpy(), one[1].cpu().numpy()
    gd, gi = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert np.array_equal(_bits(gd), _bits(od)), what
    sure = mref.distinct_mask(od)
    assert np.array_equal(gi[sure], oi[sure]), what
    assert ((gi >= 0) == (oi >= 0)).all(), what
    tally[0] += int((~sure).sum())
    tally[1] += sure.size


@pytest.mark.parametrize("nq", [5, 33])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_blocks_merged_equal_one_index(gpu, kind, nq):
    torch, codec, _, ctx = gpu
    w = _indices(gpu, kind)
    tally = [0, 0]
    for split in SPLITS:
        for k in (1, 10, 64):
            _check_split(gpu, w, split, nq, k, tally)
        _check_split(gpu, w, split, nq, 10, tally, schedule="list")
    _check_split(gpu, w, "3", nq, 200, tally)                  # the wide list, a raised context
    _check_split(gpu, w, "3000+1", nq, 200, tally, schedule="list")
    # keep= that leaves the second of three blocks nothing
    keep = torch.from_numpy(np.random.default_rng(12).random(N) < 0.6).cuda()
    keep[SPLITS["3"][1]:SPLITS["3"][2]] = False
    _check_split(gpu, w, "3", nq, 10, tally, keep=keep)
    _check_split(gpu, w, "3", nq, 64, tally, keep=keep, schedule="list")
    got, (ds, is_) = _merged(gpu, w, "3", nq, 10, keep=keep)
    assert (is_[1] == -1).all() and keep[got[1].reshape(-1)].all()
    # the positions whose ids are not compared (a distance equal to a neighbour's): at most 1 %
    assert tally[0] <= 0.01 * tally[1], tally
    codec.decode_status(ctx)
    codec.ivf_status(ctx)


def test_refined_blocks_equal_the_numpy_procedure(gpu):
    """refine=32 with a 4 x 256 second code: every block re-ranks its own 32 candidates and the
    merge takes the top 10 of 3 * 32 -- the CPU restatement of exactly that"""
    torch, codec, _, ctx = gpu
    w = mref.search_world(N, D, NLIST, 5, 4, m2=4, spread=True)
    pq, pq2, coarse = codec.PQ(ctx, w["cent"]), codec.PQ(ctx, w["cent2"]), codec.Coarse(ctx, w["cc"])
    xd, qd = torch.from_numpy(w["x"]).cuda(), torch.from_numpy(w["q"]).cuda()
    starts = SPLITS["3"]
    res = [codec.IVF.build(ctx, pq, coarse, xd[b:e], chunk_vectors=8, refine_pq=pq2)
           .search(qd, NPROBE, 10, refine=32) for b, e in zip(starts[:-1], starts[1:])]
    got = codec.merge_topk(ctx, torch.stack([r[0] for r in res]), torch.stack([r[1] for r in res]),
                           10, starts[:-1])
    want = mref.sharded_search_ref(w["x"], starts, w["q"], w["cc"], w["cent"], NPROBE, 10,
                                   refine=32, cent2=w["cent2"])
    _same(got, want, "refined")
    codec.decode_status(ctx)


@pytest.mark.parametrize("kind", ["plain", "residual"])
def test_one_rank_sharded_ivf_is_its_local_index(gpu, kind):
    torch, codec, _, ctx = gpu
    from pq_huffman_amd import shard
    w = _indices(gpu, kind)
    spec = KINDS[kind]
    sh = shard.ShardedIVF.build(ctx, None, w["pq"], w["coarse"], w["xd"], chunk_vectors=8,
                                residual=spec["residual"])
    ivf = codec.IVF.build(ctx, w["pq"], w["coarse"], w["xd"], chunk_vectors=8,
                          residual=spec["residual"])
    assert (sh.world, sh.id_base, sh.n_total, sh.local.n_ids) == (1, 0, N, N)
    assert sh.live_count() == N
    keep = torch.from_numpy(np.random.default_rng(13).random(N) < 0.5).cuda()
    gone = torch.from_numpy(np.random.default_rng(14).choice(N, 300, replace=False)).cuda()
    for step in range(2):
        for kw in (dict(), dict(schedule="list"), dict(keep=keep)):
            a, b = sh.search(w["qd"], NPROBE, 10, **kw), ivf.search(w["qd"], NPROBE, 10, **kw)
            assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
        # the collective on one rank: a gather that is a copy, then the merge of one part
        d, i = ivf.search(w["qd"], NPROBE, 10)
        md, mi, state = shard.search_merge(ctx, sh.comm, d, i, 0, check=True)
        want = mref.merge_topk_ref(d.cpu().numpy()[None], i.cpu().numpy()[None], [0], 10)
        _same((md, mi), want, "search_merge on one rank")
        assert int(state.item()) == 0
        sh.remove(gone)
        ivf.remove(gone)
        assert sh.live_count() == ivf.live_count() == N - 300
    assert _status(lambda: sh.search(w["qd"], NPROBE, 10, keep=keep[:-1])) == -1


# ------------------------------------------------------------------------------ the collective
def test_collective_through_a_raw_pointer_hook(gpu):
    """pqh_shard_search_merge on one rank with a hook that is handed raw device pointers (a
    device-to-device copy on the call's stream): the good call, and the failures that keep the
    rank in the gather -- a passed-in status, k above the context's limit, a scratch too small
    (the gather then lands in the context's own scratch, which no tensor covers)"""
    import ctypes
    torch, codec, ctx, ctx_wide = gpu
    from pq_huffman_amd import capi
    lib = capi.lib()
    copy = lib.hipMemcpyAsync          # (found through the library's own dependency on HIP)
    copy.restype = ctypes.c_int
    copy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    calls = []

    def gather(user, send, recv, nbytes, stream):
        calls.append(nbytes)
        return copy(recv, send, nbytes, 3, stream)          # hipMemcpyDeviceToDevice

    hook = capi.ALL_GATHER(gather)
    comm = capi.ShardComm(None, 1, 0, capi.ALL_REDUCE_U32(lambda *a: 1), hook)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())

    def run(c, d, i, base, status=0, scratch_bytes=None):
        nq, k = d.shape
        need = lib.pqh_shard_search_scratch_bytes(1, nq, k)
        scratch = torch.empty(max(need, 8), dtype=torch.uint8, device="cuda")
        out = (torch.full((nq, k), -7.0, dtype=torch.float32, device="cuda"),
               torch.full((nq, k), -7, dtype=torch.int64, device="cuda"))
        state = torch.full((1,), -7, dtype=torch.int64, device="cuda")
        rc = lib.pqh_shard_search_merge(c.ptr, ctypes.byref(comm), ptr(d), ptr(i), nq, k, base,
                                        status, ptr(scratch),
                                        need if scratch_bytes is None else scratch_bytes,
                                        ptr(out[0]), ptr(out[1]), ptr(state))
        torch.cuda.synchronize()
        return rc, out, int(state.item()), lib.pqh_shard_search_status(c.ptr, ptr(state))

    def padding(out):
        return bool(torch.isinf(out[0]).all() and (out[0] > 0).all() and (out[1] == -1).all())

    for nq, k, c in ((5, 10, ctx), (3, 7, ctx), (4, 100, ctx_wide)):   # 3 * 7: the odd count's pad
        d, i = mref.tied_parts(1, nq, k, seed=nq + k)
        dd, di = torch.from_numpy(d[0]).cuda(), torch.from_numpy(i[0]).cuda()
        rc, out, state, st = run(c, dd, di, 1 << 36)
        assert (rc, state, st) == (0, 0, 0)
        _same(out, mref.merge_topk_ref(d, i, [1 << 36], k), (nq, k))
        assert calls[-1] == 16 + (nq * k * 4 + 7) // 8 * 8 + nq * k * 8
        for kw, want in ((dict(status=-3), -3), (dict(scratch_bytes=64), -8)):
            n_calls = len(calls)
            rc, out, state, st = run(c, dd, di, 0, **kw)
            assert (rc, state, st) == (want, 1, -9) and padding(out), kw       # PQH_ERR_REMOTE
            assert len(calls) == n_calls + 1                                    # it did gather
    d, i = mref.tied_parts(1, 2, 65, seed=3)
    rc, out, state, st = run(ctx, torch.from_numpy(d[0]).cuda(), torch.from_numpy(i[0]).cuda(), 0)
    assert (rc, state, st) == (-1, 1, -9) and padding(out)                      # k above the limit
    rc, out, state, st = run(ctx, torch.from_numpy(d[0, :0]).cuda(), torch.from_numpy(i[0, :0]).cuda(), 0)
    assert rc == -1                       # ... also with no queries; the header still travelled
    assert lib.pqh_shard_search_merge(ctx.ptr, ctypes.byref(comm), None, None, 1, 257, 0, 0, None,
                                      0, None, None, None) == -1                # at once
    n_calls = len(calls)
    assert lib.pqh_shard_search_merge(ctx.ptr, ctypes.byref(comm), None, None, 2 ** 31, 1, 0, 0,
                                      None, 0, None, None, None) == -4
    assert len(calls) == n_calls
