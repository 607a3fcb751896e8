"""pqh_ivf_regroup and pqh_decode_scatter on the GPU against the numpy reference
(tests/regroup_ref.py): every output compared with array_equal, the outputs pre-filled with the
poison patterns of tests/test_gpu_ivf.py and framed by guard rows."""
import ctypes

import numpy as np
import pytest

import datagen
import regroup_ref as rg

pytestmark = pytest.mark.gpu

POISON = (0xFFFFFFFF, 0xA5A5A5A5, 0x00000001)   # (the patterns of tests/test_gpu_ivf.py)
GUARD = 16                                      # guard elements on either side of an output
NS = (0, 1, 63, 1003)
NLISTS = (1, 13, 1030)


@pytest.fixture(scope="module")
def gpu():
    import torch
    from pq_huffman_amd import codec
    assert torch.cuda.is_available()
    return torch, codec, codec.Context(0)


def _status(fn):
    from pq_huffman_amd.capi import PqhError
    try:
        fn()
    except PqhError as err:
        return err.status
    return 0


class Framed:
    """an int64 output of `count` elements inside a poisoned buffer with GUARD elements around it"""

    def __init__(self, torch, count, value):
        self.count, self.value = count, value
        self.buf = torch.empty(count + 2 * GUARD, dtype=torch.int64, device="cuda")
        self.buf.view(torch.int32).fill_(value - (1 << 32) if value >= 1 << 31 else value)
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + 8 * GUARD)

    def get(self):
        """the output as numpy, after the check that the guards still hold the poison"""
        host = self.buf.cpu().numpy()
        word = np.array([self.value | (self.value << 32)], np.uint64).view(np.int64)[0]
        assert (host[:GUARD] == word).all() and (host[GUARD + self.count:] == word).all()
        return host[GUARD:GUARD + self.count]


def _regroup(gpu, offsets, n, keep, add_offsets, value):
    """pqh_ivf_regroup into framed, poisoned outputs -> numpy (new_offsets, dest, add_base)"""
    from pq_huffman_amd.capi import check, lib
    torch, codec, ctx = gpu
    nlist = len(offsets) - 1
    od = torch.from_numpy(np.ascontiguousarray(offsets, np.int64)).cuda()
    kd = None if keep is None else torch.from_numpy(rg.pack(keep).view(np.int32)).cuda()
    ad = None if add_offsets is None else torch.from_numpy(np.ascontiguousarray(add_offsets, np.int64)).cuda()
    outs = [Framed(torch, c, value) for c in (nlist + 1, n, nlist)]
    check(lib().pqh_ivf_regroup(ctx.ptr, codec._ptr(od), nlist, n, codec._ptr(kd), codec._ptr(ad),
                                outs[0].ptr, outs[1].ptr, outs[2].ptr), "pqh_ivf_regroup")
    ctx.sync()
    return [o.get() for o in outs]


def _offsets(rng, nlist, total):
    """nlist lists over `total` rows, about a third of them empty"""
    if nlist == 1:
        return np.array([0, total], np.int64)
    values = rng.integers(0, total + 1, size=max(1, 2 * (nlist - 1) // 3))
    cuts = np.sort(rng.choice(values, size=nlist - 1))          # (repeats: empty lists)
    return np.concatenate([[0], cuts, [total]]).astype(np.int64)


# ------------------------------------------------------------------------------ the plan
@pytest.mark.parametrize("n", NS)
def test_regroup_equals_reference(gpu, n):
    torch, codec, ctx = gpu
    rng = np.random.default_rng(300 + n)
    case = 0
    for nlist in NLISTS:
        offsets = _offsets(rng, nlist, n)
        add_offsets = _offsets(rng, nlist, 77)
        for kind in ("none", "zero", "random"):
            keep = {"none": None, "zero": np.zeros(n, bool), "random": rng.random(n) < 0.5}[kind]
            for add in (None, add_offsets):
                want = rg.regroup(offsets, keep, add)
                got = _regroup(gpu, offsets, n, keep, add, POISON[case % 3])
                case += 1
                for g, w, name in zip(got, want, ("new_offsets", "dest", "add_base")):
                    assert np.array_equal(g, w), (n, nlist, kind, add is not None, name)
    codec.ivf_status(ctx)


def test_regroup_six_lists_and_the_wrapper(gpu):
    """the hand-checked world (a list boundary inside a mask word, two empty lists) through
    codec.ivf_regroup, with n read from the offsets and given"""
    torch, codec, ctx = gpu
    od = torch.from_numpy(rg.SIX_OFFSETS).cuda()
    ad = torch.from_numpy(rg.SIX_ADD).cuda()
    for kind in ("none", "zero", "hand", "random"):
        keep = rg.six_keep(kind)
        kd = None if keep is None else torch.from_numpy(rg.pack(keep).view(np.int32)).cuda()
        for add, add_d in ((None, None), (rg.SIX_ADD, ad)):
            want = rg.regroup(rg.SIX_OFFSETS, keep, add)
            for n in (None, 40):
                got = codec.ivf_regroup(ctx, od, kd, add_d, n=n)
                for g, w in zip(got, want):
                    assert np.array_equal(g.cpu().numpy(), w), (kind, add is not None)
    codec.ivf_status(ctx)


def test_regroup_reports_offsets_that_do_not_cover_the_stream(gpu):
    torch, codec, ctx = gpu
    n = 1003
    rng = np.random.default_rng(7)
    good = _offsets(rng, 13, n)
    keep = rng.random(n) < 0.5
    add = _offsets(rng, 13, 50)
    bads = {"reversed": good[::-1].copy(), "starts above 0": np.concatenate([[2], good[1:]]),
            "ends short of n": np.concatenate([good[:-1], [n - 5]]),
            "beyond n": np.concatenate([good[:5], [n + 4000], good[6:]]),
            "negative": np.concatenate([good[:5], [-4000], good[6:]])}
    case = 0
    for name, bad in bads.items():
        for k in (None, keep):
            for a in (None, add):
                _regroup(gpu, bad, n, k, a, POISON[case % 3])      # (the guards are checked)
                case += 1
                assert _status(lambda: codec.ivf_status(ctx)) == -1, name
                codec.ivf_status(ctx)                              # read once, then clean
    for name, bad_add in (("add reversed", add[::-1].copy()), ("add above 0", add + 1)):
        _regroup(gpu, good, n, keep, bad_add, POISON[0])
        assert _status(lambda: codec.ivf_status(ctx)) == -1, name
    # and a good plan afterwards is clean
    got = _regroup(gpu, good, n, keep, add, POISON[1])
    codec.ivf_status(ctx)
    assert all(np.array_equal(g, w) for g, w in zip(got, rg.regroup(good, keep, add)))
    # the argument checks
    from pq_huffman_amd.capi import lib
    od = torch.from_numpy(good).cuda()
    out = torch.empty(n + 14, dtype=torch.int64, device="cuda")
    p = codec._ptr
    assert lib().pqh_ivf_regroup(ctx.ptr, p(od), 0, n, None, None, p(out), p(out), None) == -1
    assert lib().pqh_ivf_regroup(ctx.ptr, p(od), 13, -1, None, None, p(out), p(out), None) == -1
    assert lib().pqh_ivf_regroup(ctx.ptr, None, 13, n, None, None, p(out), p(out), None) == -1
    assert lib().pqh_ivf_regroup(ctx.ptr, p(od), 13, 1 << 31, None, None, p(out), p(out), None) == -4
    assert lib().pqh_ivf_regroup(ctx.ptr, p(od), (1 << 24) + 1, n, None, None, p(out), p(out), None) == -4


# ------------------------------------------------------------------------------ the scatter
SCATTER_NS = (1, 63, 1003)
CHUNKS = (1, 7, 64)
FILL = 0xA5


def _maps(rng, n):
    """(name, dest, n_out): the identity, a permutation, a random half dropped and the rest
    closed up, nothing kept, only the stream's last row kept"""
    ident = np.arange(n, dtype=np.int64)
    yield "identity", ident, n
    yield "permutation", rng.permutation(n).astype(np.int64), n
    half = rng.random(n) < 0.5
    dest = np.full(n, -1, np.int64)
    dest[half] = np.arange(half.sum()) + 2          # (rows 0 and 1 of the output stay a gap)
    yield "half", dest, int(half.sum()) + 3
    yield "nothing", np.full(n, -1, np.int64), 4
    last = np.full(n, -1, np.int64)
    last[-1] = 1
    yield "last row", last, 3


def _scatter(gpu, tabs, enc, dest, n_out, m):
    torch, codec, ctx = gpu
    out = torch.full((n_out, m), FILL, dtype=torch.uint8, device="cuda")
    got = codec.decode_scatter(ctx, tabs, enc, torch.from_numpy(dest).cuda(), out)
    assert got is out
    return out.cpu().numpy()


@pytest.mark.parametrize("context", [True, False])
@pytest.mark.parametrize("m", [5, 8, 16])
def test_scatter_equals_numpy(gpu, m, context):
    """m = 8 and 16: rows of whole u64 words (the packed walk), m = 5: the walk part by part;
    1,003 rows in chunks of 1: more than one workgroup, in chunks of 7: a cut last chunk"""
    torch, codec, ctx = gpu
    rng = np.random.default_rng(40 + m)
    for n in SCATTER_NS:
        codes = datagen.skewed_codes(n, m, 256, seed=50 + n)
        cd = torch.from_numpy(codes).cuda()
        tabs = codec.Tables(ctx, m, 256, context).build(codec.histogram(ctx, cd, 256, context))
        for chunk in CHUNKS:
            enc = codec.encode(ctx, tabs, cd, chunk_vectors=chunk)
            for name, dest, n_out in _maps(rng, n):
                want = rg.scatter(codes, dest, np.full((n_out, m), FILL, np.uint8))
                got = _scatter(gpu, tabs, enc, dest, n_out, m)
                assert np.array_equal(got, want), (n, chunk, name)
                if name == "identity":
                    assert np.array_equal(got, codec.decode(ctx, tabs, enc).cpu().numpy())
            codec.decode_status(ctx)
        tabs.close()


@pytest.fixture(scope="module")
def coded(gpu):
    """1,003 rows of 8 context-coded parts in chunks of 7, and the same without context"""
    torch, codec, ctx = gpu
    codes = datagen.skewed_codes(1003, 8, 256, seed=9)
    cd = torch.from_numpy(codes).cuda()
    made = {}
    for context in (True, False):
        tabs = codec.Tables(ctx, 8, 256, context).build(codec.histogram(ctx, cd, 256, context))
        made[context] = (tabs, codec.encode(ctx, tabs, cd, chunk_vectors=7))
    return codes, made


@pytest.mark.parametrize("context", [True, False])
def test_scatter_reports_destinations_outside_the_output(gpu, coded, context):
    torch, codec, ctx = gpu
    codes, made = coded
    tabs, enc = made[context]
    n = len(codes)
    for bad_value in (-2, n, -(1 << 40), 1 << 40):
        dest = np.arange(n, dtype=np.int64)[::-1].copy()
        dest[[0, 500, n - 1]] = bad_value
        want = rg.scatter(codes, dest, np.full((n, 8), FILL, np.uint8))
        got = _scatter(gpu, tabs, enc, dest, n, 8)
        assert np.array_equal(got, want), bad_value          # the other rows exact, these unwritten
        assert _status(lambda: codec.decode_status(ctx)) == -1, bad_value
        codec.decode_status(ctx)                             # read once, then clean


@pytest.mark.parametrize("context", [True, False])
def test_scatter_reports_a_damaged_chunk_only_when_it_is_wanted(gpu, coded, context):
    """a chunk whose offset lies past the stream, and a stream cut short inside chunk 100 (the
    56 symbols of that chunk need more than the 32 bits that are left of its first word, and every
    later chunk starts past the end): PQH_ERR_CORRUPT when a row of such a chunk has a
    destination, its rows left unwritten and every other chunk's exact; no error when none has"""
    torch, codec, ctx = gpu
    codes, made = coded
    tabs, enc = made[context]
    n = len(codes)
    off = enc.chunk_offsets.clone()
    off[70] = enc.stream.numel() * 8 + 64
    lost_offset = codec.Encoded(enc.stream, enc.bits, 7, off, enc.chunk_prev, n, 1)
    cut_bytes = (int(enc.chunk_offsets[100].item()) // 32 + 1) * 4
    cut = codec.Encoded(enc.stream[:cut_bytes].clone(), enc.bits, 7, enc.chunk_offsets,
                        enc.chunk_prev, n, 1)
    for bad, rows in ((lost_offset, np.arange(490, 497)), (cut, np.arange(700, n))):
        dest = np.arange(n, dtype=np.int64)
        want = rg.scatter(codes, dest, np.full((n, 8), FILL, np.uint8))
        want[rows] = FILL
        got = _scatter(gpu, tabs, bad, dest, n, 8)
        assert np.array_equal(got, want), rows[0]
        assert _status(lambda: codec.decode_status(ctx)) == -6   # PQH_ERR_CORRUPT
        # ... which a bad destination in the same call does not mask
        dest[0] = -2
        _scatter(gpu, tabs, bad, dest, n, 8)
        assert _status(lambda: codec.decode_status(ctx)) == -6
        codec.decode_status(ctx)
        # no row of the chunks wanted: they are not looked at
        dest = np.arange(n, dtype=np.int64)
        dest[rows] = -1
        want = rg.scatter(codes, dest, np.full((n, 8), FILL, np.uint8))
        assert np.array_equal(_scatter(gpu, tabs, bad, dest, n, 8), want), rows[0]
        codec.decode_status(ctx)


def test_scatter_argument_checks(gpu, coded):
    torch, codec, ctx = gpu
    codes, made = coded
    tabs, enc = made[True]
    from pq_huffman_amd.capi import PqhError, lib
    dest = torch.arange(len(codes), dtype=torch.int64, device="cuda")
    out = torch.empty((len(codes), 8), dtype=torch.uint8, device="cuda")
    for bad_dest, bad_out in ((dest[:-1], out), (dest.int(), out), (dest, out[:, :7]),
                              (dest, out.to(torch.int16))):
        with pytest.raises(PqhError) as err:
            codec.decode_scatter(ctx, tabs, enc, bad_dest, bad_out)
        assert err.value.status == -1
    args = codec._index_args(enc)
    p = codec._ptr
    assert lib().pqh_decode_scatter(ctx.ptr, tabs.ptr, *args, p(dest), p(out), -1) == -1
    assert lib().pqh_decode_scatter(ctx.ptr, tabs.ptr, *args, None, p(out), 5) == -1
    assert lib().pqh_decode_scatter(ctx.ptr, None, *args, p(dest), p(out), 5) == -1
    # no rows: nothing is launched, nothing is looked at
    assert lib().pqh_decode_scatter(ctx.ptr, tabs.ptr, None, 0, 0, 1, 7, None, None, None, None, 0) == 0
    codec.decode_status(ctx)
