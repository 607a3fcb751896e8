"""codec.IdMap on the GPU against the numpy statement (tests/idmap_ref.py): the blob byte for
byte, and every call exactly -- integers, so there is no tolerance.  The shapes are the smallest
at which each kernel can go wrong: word and block edges, a cut last block, no low part, empty
lists, a gap in the keys inside a block (and one of more than the 64 words a wave reads in a
step), low fields across two words, a compacted index.  None of the kernels uses LDS, so there
is no LDS poison case."""
import numpy as np
import pytest

import idmap_ref as ref
import regroup_ref as rg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    from pq_huffman_amd import codec
    assert torch.cuda.is_available()
    return torch, codec, codec.Context(0)


def _cases():
    c = {f"n{n}": ref.random_layout(n, n, 5, seed=n) + (True,)
         for n in (1, 63, 64, 255, 256, 257, 1000)}
    c["n0"] = (np.zeros(0, np.int64), np.zeros(6, np.int64), 0, True)
    c["n0_ids"] = (np.zeros(0, np.int64), np.zeros(6, np.int64), 77, True)
    c["identity"] = ref.identity(300) + (True,)                          # L = 0
    c["seven"] = ref.random_layout(1000, 1000, 7, seed=7, empty=(0, 3, 6)) + (True,)
    c["last_list"] = ref.last_list() + (True,)
    c["two_ends"] = ref.two_ends() + (True,)
    c["two_ends_wide"] = ref.two_ends(last=4000) + (True,)               # a span of > 64 words
    c["compacted"] = ref.random_layout(1000, 4000, 13, seed=8) + (True,)
    c["no_reverse"] = ref.random_layout(257, 300, 5, seed=3) + (False,)
    c["wide40"] = ref.random_layout(16, 2 ** 20, 2 ** 24, seed=9) + (True,)          # int32 reverse
    c["wide51"] = ref.random_layout(16, 2 ** 31 - 1, 2 ** 24, seed=10) + (False,)    # two-word fields
    return c


CASES = _cases()
_built = {}


def _map(gpu, name):
    """(IdMap, perm, offsets on the device) of a case, built once"""
    torch, codec, ctx = gpu
    if name not in _built:
        perm, offsets, n_ids, reverse = CASES[name]
        pd, od = torch.from_numpy(perm).cuda(), torch.from_numpy(offsets).cuda()
        _built[name] = (codec.IdMap(ctx, pd, od, n_ids, reverse=reverse), pd, od)
        codec.ivf_status(ctx)
    return _built[name]


def _raises_arg(codec, ctx):
    with pytest.raises(codec.PqhError) as err:
        codec.ivf_status(ctx)
    assert err.value.status == -1
    codec.ivf_status(ctx)                                  # read once, then clear


@pytest.mark.parametrize("name", sorted(CASES))
def test_blob_is_the_numpy_blob(gpu, name):
    torch, codec, ctx = gpu
    perm, offsets, n_ids, reverse = CASES[name]
    m, _, _ = _map(gpu, name)
    want = ref.build(perm, offsets, n_ids, reverse)
    assert (m.n, m.n_ids, m.nlist) == (len(perm), n_ids, len(offsets) - 1)
    assert m.nbytes == len(want) == codec.idmap_bytes(len(perm), n_ids, len(offsets) - 1, reverse)
    assert m.blob.dtype == torch.uint8 and np.array_equal(m.blob.cpu().numpy(), want)
    if name == "wide51":
        assert ref.View(want).L == 51
    if name == "two_ends_wide":
        assert ref.decode_span_words(want, 0) > 64


@pytest.mark.parametrize("name", sorted(CASES))
def test_decode(gpu, name):
    torch, codec, ctx = gpu
    perm = CASES[name][0]
    n = len(perm)
    m, pd, _ = _map(gpu, name)
    assert torch.equal(m.decode(), pd)
    for first, count in ((0, n), (1, n - 2), (255, 2), (256, 1), (n, 0), (n // 2, n - n // 2)):
        if count < 0 or first + count > n:
            continue
        out = torch.full((count,), -5, dtype=torch.int64, device="cuda")
        assert m.decode(first, count, out=out) is out
        assert torch.equal(out, pd[first:first + count]), (first, count)
    codec.ivf_status(ctx)
    with pytest.raises(codec.PqhError):
        m.decode(0, n + 1)


@pytest.mark.parametrize("name", sorted(CASES))
def test_ids(gpu, name):
    torch, codec, ctx = gpu
    perm = CASES[name][0]
    n = len(perm)
    m, pd, _ = _map(gpu, name)
    rng = np.random.default_rng(5)
    rows = np.concatenate([rng.integers(0, n, 700) if n else np.zeros(0, np.int64),
                           np.arange(n)[::-1], [-1, -1, -9]]).astype(np.int64)
    rows = np.concatenate([rows, np.full(-len(rows) % 3, -1, np.int64)])
    rows = rows[rng.permutation(len(rows))].reshape(3, -1)            # any shape, repeats
    want = np.where(rows >= 0, np.append(perm, 0)[np.maximum(rows, 0)], rows)
    assert np.array_equal(m.ids(torch.from_numpy(rows).cuda()).cpu().numpy(), want)
    assert m.ids(torch.zeros(0, dtype=torch.int64, device="cuda")).numel() == 0
    codec.ivf_status(ctx)
    # a row from n on: -1, the sticky error, and the status clear afterwards
    rows = torch.tensor([n, -1, n + 300] + ([n - 1] if n else []), dtype=torch.int64, device="cuda")
    got = m.ids(rows).cpu().numpy()
    assert got[:3].tolist() == [-1, -1, -1] and (n == 0 or got[3] == perm[-1])
    _raises_arg(codec, ctx)


@pytest.mark.parametrize("name", sorted(n for n in CASES if CASES[n][3]))
def test_rows(gpu, name):
    torch, codec, ctx = gpu
    perm, offsets, n_ids, _ = CASES[name]
    n = len(perm)
    m, pd, od = _map(gpu, name)
    every = torch.arange(n, dtype=torch.int64, device="cuda")
    assert torch.equal(m.rows(m.ids(every)), every)
    assert torch.equal(m.rows(pd, od), every)
    codec.ivf_status(ctx)
    if n_ids <= 5000:                     # every id: its row, or -1 for one the index dropped
        inv = np.full(n_ids, -1, np.int64)
        inv[perm] = np.arange(n)
        ids = torch.arange(n_ids, dtype=torch.int64, device="cuda")
        assert np.array_equal(m.rows(ids).cpu().numpy(), inv)
        assert name != "compacted" or (inv < 0).sum() == 3000
        codec.ivf_status(ctx)
    bad = torch.tensor([n_ids, -1, n_ids + 5], dtype=torch.int64, device="cuda")
    assert m.rows(bad).cpu().tolist() == [-1, -1, -1]
    _raises_arg(codec, ctx)


@pytest.mark.parametrize("name", ["no_reverse", "wide51"])
def test_rows_needs_the_reverse_part(gpu, name):
    torch, codec, ctx = gpu
    from pq_huffman_amd.capi import lib
    m, pd, od = _map(gpu, name)
    with pytest.raises(codec.PqhError) as err:
        m.rows(pd[:4])
    assert err.value.status == -1
    # the C call: asynchronous, so -1 for every id and the sticky error
    out = torch.full((4,), 7, dtype=torch.int64, device="cuda")
    assert lib().pqh_idmap_rows(ctx.ptr, m.blob.data_ptr(), od.data_ptr(), pd.data_ptr(), 4,
                                out.data_ptr()) == 0
    assert out.cpu().tolist() == [-1] * 4
    _raises_arg(codec, ctx)


def _pack_cases():
    c = {f"n{n}": ref.random_layout(n, n, 3, seed=100 + n) for n in (31, 32, 33, 257, 1000)}
    c["compacted"] = CASES["compacted"][:3]
    c["two_ends_wide"] = CASES["two_ends_wide"][:3]
    c["wide40"] = CASES["wide40"][:3]
    c["identity"] = CASES["identity"][:3]
    return c


@pytest.mark.parametrize("name", sorted(_pack_cases()))
def test_pack_mask(gpu, name):
    torch, codec, ctx = gpu
    perm, offsets, n_ids = _pack_cases()[name]
    n = len(perm)
    pd, od = torch.from_numpy(perm).cuda(), torch.from_numpy(offsets).cuda()
    m = codec.IdMap(ctx, pd, od, n_ids)
    rng = np.random.default_rng(6)
    last = np.uint32((1 << (n % 32)) - 1) if n % 32 else np.uint32(0xFFFFFFFF)
    for keep in (np.ones(n_ids, bool), np.zeros(n_ids, bool), rng.random(n_ids) < 0.5):
        kd = torch.from_numpy(keep).cuda()
        out = torch.full(((n + 31) // 32,), -1, dtype=torch.int32, device="cuda")
        assert m.pack_mask(kd, out=out) is out
        got = out.cpu().numpy().view(np.uint32)
        assert np.array_equal(got, rg.pack(keep[perm]))               # the bits from n on: zeros
        if n == n_ids:
            want = codec.pack_mask(ctx, kd, pd).cpu().numpy().view(np.uint32)
        else:   # pqh_mask_pack takes as many flags as rows: the gather first, as IVF._mask does
            want = codec.pack_mask(ctx, kd[pd]).cpu().numpy().view(np.uint32)
        assert np.array_equal(got[:-1], want[:-1]) and got[-1] == want[-1] & last
        assert torch.equal(m.pack_mask(kd.to(torch.uint8)), out)
    codec.ivf_status(ctx)


def test_pack_mask_with_another_n(gpu):
    """the C call sizes its grid by the n it is given: not the map's n writes zeros, in bounds"""
    torch, codec, ctx = gpu
    from pq_huffman_amd.capi import lib
    m, pd, od = _map(gpu, "n257")
    keep = torch.ones(257, dtype=torch.bool, device="cuda")
    out = torch.full((12,), -1, dtype=torch.int32, device="cuda")
    assert lib().pqh_mask_pack_idmap(ctx.ptr, keep.data_ptr(), m.blob.data_ptr(), 100,
                                     out.data_ptr()) == 0
    assert out.cpu().tolist() == [0, 0, 0, 0] + [-1] * 8
    _raises_arg(codec, ctx)


@pytest.mark.parametrize("what", ["equal", "descending", "n_ids", "negative", "offsets"])
def test_build_checks_what_it_codes(gpu, what):
    """bad data is reported and harmless: the map is unspecified, every later call in bounds"""
    torch, codec, ctx = gpu
    perm, offsets, n_ids = ref.random_layout(600, 600, 4, seed=17)
    perm, offsets = perm.copy(), offsets.copy()
    at = int(offsets[1]) + 3                                # inside list 1
    if what == "equal":
        perm[at + 1] = perm[at]
    elif what == "descending":
        perm[at], perm[at + 1] = perm[at + 1], perm[at]
    elif what == "n_ids":
        perm[at] = n_ids
    elif what == "negative":
        perm[at] = -4
    else:
        offsets[2] = offsets[1] - 1                         # a reversed pair
    pd, od = torch.from_numpy(perm).cuda(), torch.from_numpy(offsets).cuda()
    m = codec.IdMap(ctx, pd, od, n_ids)
    _raises_arg(codec, ctx)
    every = torch.arange(600, dtype=torch.int64, device="cuda")
    ids = m.ids(every)
    assert ((ids >= -1) & (ids < n_ids)).all()
    ids = m.decode()
    assert ((ids >= -1) & (ids < n_ids)).all()
    rows = m.rows(torch.arange(n_ids, dtype=torch.int64, device="cuda"))
    assert ((rows >= -1) & (rows < 600)).all()
    m.pack_mask(torch.ones(n_ids, dtype=torch.bool, device="cuda"))
    ctx.sync()
    try:
        codec.ivf_status(ctx)                               # may or may not be set: clear it
    except codec.PqhError as e:
        assert e.status == -1


def test_argument_checks(gpu):
    torch, codec, ctx = gpu
    m, pd, od = _map(gpu, "n257")
    with pytest.raises(codec.PqhError):
        codec.IdMap(ctx, pd.to(torch.int32), od, 257)
    with pytest.raises(codec.PqhError):
        codec.IdMap(ctx, pd, od, 100)                       # fewer ids than rows
    with pytest.raises(codec.PqhError):
        m.ids(pd.to(torch.int32))
    with pytest.raises(codec.PqhError):
        m.pack_mask(torch.ones(256, dtype=torch.bool, device="cuda"))
    with pytest.raises(codec.PqhError):
        m.rows(pd, od[:-1])
    codec.ivf_status(ctx)
