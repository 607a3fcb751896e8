"""Random access into a compressed stream through its chunk index (pqh_decode_select,
pqh_decode_range, pqh_fetch_vectors, pqh_decode_files_range, huffman_decoder --rows).
Expected values are the host codes that were encoded (codes[ids], codes[first:first + count])
or pqh_decode / pqh_pq_reconstruct of the same data -- never the calls under test."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden
import datagen

pytestmark = pytest.mark.gpu

N = 1003   # not a multiple of any chunk size below
CHUNKS = [1, 4, 7, 32, 64]
# name: (m, k, context)
MODES = {"ctx_m8": (8, 256, True), "noctx_m8": (8, 256, False), "ctx_m16": (16, 256, True),
         "noctx_k4096_m8": (8, 4096, False), "noctx_m3": (3, 256, False)}


@pytest.fixture(scope="module")
def gpu():
    import torch
    from pq_huffman_amd import codec
    assert torch.cuda.is_available()
    return torch, codec, codec.Context(0)


@pytest.fixture(scope="module")
def coded(gpu):
    """mode -> (host codes, device codes, tables), built once"""
    torch, codec, ctx = gpu
    made = {}

    def get(mode):
        if mode not in made:
            m, k, ctxm = MODES[mode]
            codes = datagen.skewed_codes(N, m, k=k, seed=100 + m + k)
            cd = torch.from_numpy(codes.view(np.int16) if k > 256 else codes).cuda()
            counts = codec.histogram(ctx, cd, k, ctxm)
            cbs = codec.Codebooks(codec.counts_to_host(counts), k, ctxm)
            made[mode] = (codes, cd, codec.Tables.from_codebooks(ctx, cbs))
        return made[mode]
    return get


def _host(t, like):
    a = t.cpu().numpy()
    return a.view(like.dtype) if a.dtype != like.dtype else a


def _ids(torch, ids):
    return torch.from_numpy(np.asarray(ids, np.int64)).cuda()


def _status(fn):
    """the pqh status a call raises, 0 if none (the exception is not kept: an excinfo bound
    in the test's frame would tie the frame, and every fixture in it, into a reference cycle)"""
    from pq_huffman_amd.capi import PqhError
    try:
        fn()
    except PqhError as err:
        return err.status
    return 0


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("mode", list(MODES))
def test_select_permutation_of_all_rows(gpu, coded, mode, chunk):
    torch, codec, ctx = gpu
    codes, cd, tabs = coded(mode)
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=chunk)
    perm = np.random.default_rng(chunk).permutation(N)
    got = codec.decode_rows(ctx, tabs, enc, _ids(torch, perm))
    codec.decode_status(ctx)
    assert np.array_equal(_host(got, codes), codes[perm])


@pytest.mark.parametrize("mode", ["ctx_m8", "noctx_m8"])
def test_select_edges(gpu, coded, mode):
    """C = 7: the raw row, the row in its context, the end of chunk 0, the first row that
    starts from chunk_prev, the short last chunk, a repeated id, descending order; counts
    around the 64-lane wave; no ids at all."""
    torch, codec, ctx = gpu
    codes, cd, tabs = coded(mode)
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=7)
    ids = np.array([0, 1, 6, 7, N - 1, 500, 500, 500] + list(range(40, 7, -1)) + [N - 2, 13, 14])
    got = codec.decode_rows(ctx, tabs, enc, _ids(torch, ids))
    codec.decode_status(ctx)
    assert np.array_equal(_host(got, codes), codes[ids])
    pool = np.random.default_rng(5).integers(0, N, 65)
    for count in (1, 64, 65):
        got = codec.decode_rows(ctx, tabs, enc, _ids(torch, pool[:count]))
        assert np.array_equal(_host(got, codes), codes[pool[:count]]), count
    out = torch.full((3, 8), 0xA5, dtype=torch.uint8, device="cuda")
    codec.decode_rows(ctx, tabs, enc, _ids(torch, []), out=out)   # count = 0: nothing runs
    assert bool((out == 0xA5).all())
    codec.decode_status(ctx)


@pytest.mark.parametrize("mode", ["ctx_m8", "noctx_m8"])
def test_select_single_row_stream(gpu, coded, mode):
    torch, codec, ctx = gpu
    codes, cd, tabs = coded(mode)
    enc = codec.encode(ctx, tabs, cd[:1], chunk_vectors=7)
    got = codec.decode_rows(ctx, tabs, enc, _ids(torch, [0, 0]))
    assert np.array_equal(_host(got, codes), codes[[0, 0]])
    got = codec.decode_range(ctx, tabs, enc, 0, 1)
    codec.decode_status(ctx)
    assert np.array_equal(_host(got, codes), codes[:1])


@pytest.mark.parametrize("chunk", [7, 64])
def test_select_from_a_shard(gpu, coded, chunk):
    """rows [500, N) encoded as a shard (raw_first = 0, the halo row as context) are addressed
    by the shard's own row numbers"""
    torch, codec, ctx = gpu
    codes, cd, tabs = coded("ctx_m8")
    enc = codec.encode(ctx, tabs, cd[500:], chunk_vectors=chunk, raw_first=0, prev_row=cd[499])
    ids = np.random.default_rng(3).permutation(N - 500)
    got = codec.decode_rows(ctx, tabs, enc, _ids(torch, ids))
    assert np.array_equal(_host(got, codes), codes[500 + ids])
    got = codec.decode_range(ctx, tabs, enc, 3, 200)
    codec.decode_status(ctx)
    assert np.array_equal(_host(got, codes), codes[503:703])


def test_select_long_codes(gpu):
    """Fibonacci counts (the fib32ctx code book fixture, 32 symbols in each of 32 contexts):
    codes of up to 31 bits, past the first level (9 bits) and the second (8 more), so the
    long-code list decodes them."""
    torch, codec, ctx = gpu
    g = golden("codebooks.npz")
    fix = g["fib32ctx__counts"].reshape(32, 32)
    m, k, n = 8, 256, 2000
    counts = np.zeros((m, k, k))
    counts[:, :32, :32] = fix
    cbs = codec.Codebooks(counts.reshape(m, k * k), k, True)
    tabs = codec.Tables.from_codebooks(ctx, cbs)
    # every row follows its predecessor through a coded pair; uniform draws reach the rare ones
    live = [p for p in range(32) if fix[p].sum() > 0]
    nxt = {p: [c for c in live if fix[p, c] > 0] for p in live}
    rng = np.random.default_rng(11)
    codes = np.zeros((n, m), np.uint8)
    codes[0] = rng.choice(live, m)
    for v in range(1, n):
        for i in range(m):
            codes[v, i] = rng.choice(nxt[int(codes[v - 1, i])])
    lens = cbs.lengths().reshape(m, k, k)
    used = lens[np.arange(m)[None, :], codes[:-1], codes[1:]]
    assert used.min() >= 1 and used.max() > 9 + 8, used.max()   # W1 + the second level
    cd = torch.from_numpy(codes).cuda()
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=7)
    perm = rng.permutation(n)
    got = codec.decode_rows(ctx, tabs, enc, _ids(torch, perm))
    codec.decode_status(ctx)
    assert np.array_equal(got.cpu().numpy(), codes[perm])
    assert np.array_equal(codec.decode_range(ctx, tabs, enc, 5, n - 9).cpu().numpy(), codes[5:n - 4])
    codec.decode_status(ctx)


RANGES = [(0, N), (0, 1), (3, 1), (3, 9), (5, 2), (N - 1, 1), (6, N - 6)]


@pytest.mark.parametrize("chunk", [7, 64])
@pytest.mark.parametrize("mode", list(MODES))
def test_range(gpu, coded, mode, chunk):
    torch, codec, ctx = gpu
    codes, cd, tabs = coded(mode)
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=chunk)
    for first, count in RANGES:
        out = torch.full((count + 8, codes.shape[1]), 0xA5, dtype=torch.uint8, device="cuda")
        if codes.dtype == np.uint16:
            out = torch.full((count + 8, codes.shape[1]), 0xA5A5 - 65536, dtype=torch.int16,
                             device="cuda")
        guard = out[count:].clone()
        codec.decode_range(ctx, tabs, enc, first, count, out=out)
        assert np.array_equal(_host(out[:count], codes), codes[first:first + count]), (first, count)
        assert torch.equal(out[count:], guard), (first, count)   # nothing past the range
    codec.decode_status(ctx)
    for first, count in ((-1, 2), (N - 1, 2), (0, N + 1)):
        assert _status(lambda: codec.decode_range(ctx, tabs, enc, first, count)) == -1


@pytest.mark.parametrize("m,dsub", [(8, 16), (16, 6)])
def test_fetch_reconstructs(gpu, coded, m, dsub):
    """SIFT shape (512-byte rows) and Deep shape (384-byte rows: 16-byte pieces that span two
    subspaces), with a row stride that keeps the 16-byte stores and one that does not"""
    torch, codec, ctx = gpu
    codes, cd, tabs = coded("ctx_m8" if m == 8 else "ctx_m16")
    cent = np.random.default_rng(m).normal(size=(m, 256, dsub)).astype(np.float32)
    pq = codec.PQ(ctx, cent)
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=7)
    ids = np.random.default_rng(9).integers(0, N, 203)
    ids[:4] = [0, N - 1, 7, 7]
    d = m * dsub
    want = pq.reconstruct(cd[_ids(torch, ids)])
    gathered = np.concatenate([cent[i, codes[ids, i]] for i in range(m)], axis=1)
    assert np.array_equal(want.cpu().numpy().view(np.uint32), gathered.view(np.uint32))
    for ld in (d, d + 4, d + 3):
        out = torch.full((len(ids), ld), 7.0, dtype=torch.float32, device="cuda")
        codec.fetch(ctx, tabs, pq, enc, _ids(torch, ids), out=out)
        assert torch.equal(out[:, :d].contiguous().view(torch.int32), want.view(torch.int32)), ld
        assert bool((out[:, d:] == 7.0).all()), ld   # the padding between rows is left alone
    codec.decode_status(ctx)


def test_bad_ids_are_reported(gpu, coded):
    torch, codec, ctx = gpu
    codes, cd, tabs = coded("ctx_m8")
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=7)
    ids = np.array([5, -1, 900, N, 0, 64])
    ok = (ids >= 0) & (ids < N)
    got = codec.decode_rows(ctx, tabs, enc, _ids(torch, ids)).cpu().numpy()
    assert np.array_equal(got[ok], codes[ids[ok]])
    assert not got[~ok].any()
    assert _status(lambda: codec.decode_status(ctx)) == -1   # PQH_ERR_ARG
    codec.decode_status(ctx)                                 # read once, then clean


def test_offset_past_the_stream_is_reported(gpu, coded):
    """a sidecar whose last chunk offset lies past the stream: PQH_ERR_CORRUPT (which a bad id
    in the same call does not mask), every other chunk's rows still right"""
    torch, codec, ctx = gpu
    codes, cd, tabs = coded("ctx_m8")
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=7)
    off = enc.chunk_offsets.clone()
    off[-1] = enc.stream.numel() * 8 + 64
    bad = codec.Encoded(enc.stream, enc.bits, 7, off, enc.chunk_prev, N, 1)
    ids = np.concatenate([np.arange(N), [-1]])
    got = codec.decode_rows(ctx, tabs, bad, _ids(torch, ids)).cpu().numpy()
    sound = (N - 1) // 7 * 7   # rows before the last chunk
    assert np.array_equal(got[:sound], codes[:sound])
    assert _status(lambda: codec.decode_status(ctx)) == -6   # PQH_ERR_CORRUPT
    codec.decode_status(ctx)


def _files_range(prefix, first, count):
    from pq_huffman_amd.capi import lib
    from pq_huffman_amd.codec import _libc
    buf, m = ctypes.c_void_p(), ctypes.c_int(0)
    rc = lib().pqh_decode_files_range(prefix.encode(), first, count, ctypes.byref(buf),
                                      ctypes.byref(m))
    if rc:
        return rc, None
    rows = np.ctypeslib.as_array(ctypes.cast(buf, ctypes.POINTER(ctypes.c_ubyte)),
                                 (count, m.value)).copy()
    _libc.free.argtypes = [ctypes.c_void_p]
    _libc.free(buf)
    return 0, rows


@pytest.mark.parametrize("sort", [0, 1])
def test_files_and_cli_row_range(tmp_path, sort):
    from pq_huffman_amd.capi import EncodeOptions, lib
    codes = np.ascontiguousarray(golden("huff_m8_n10000.npz")["input"])
    n, m = codes.shape
    prefix = str(tmp_path) + "/"
    opt = EncodeOptions(1, sort, 64, 0)
    assert lib().pqh_encode_files(codes.ctypes.data_as(ctypes.c_void_p), n, m, ctypes.byref(opt),
                                  prefix.encode()) == 0
    first, count = 4097, 130
    if sort:   # stream order is the encoder's sorted order: the full decode pins it
        buf, nn, mm = ctypes.c_void_p(), ctypes.c_longlong(0), ctypes.c_int(0)
        assert lib().pqh_decode_files(prefix.encode(), ctypes.byref(buf), ctypes.byref(nn),
                                      ctypes.byref(mm)) == 0
        stored = np.ctypeslib.as_array(ctypes.cast(buf, ctypes.POINTER(ctypes.c_ubyte)),
                                       (n, m)).copy()
        assert sorted(map(bytes, stored)) == sorted(map(bytes, codes))
    else:
        stored = codes
    want = stored[first:first + count]
    rc, rows = _files_range(prefix, first, count)
    assert rc == 0 and np.array_equal(rows, want)
    for f, c in ((0, 1), (n - 1, 1), (63, 2), (0, n)):
        rc, rows = _files_range(prefix, f, c)
        assert rc == 0 and np.array_equal(rows, stored[f:f + c]), (f, c)
    dec = tmp_path / "rows.bin"
    r = subprocess.run([os.path.join(ROOT, "pq_huffman_amd", "bin", "huffman_decoder"), prefix,
                        "--rows", f"{first}:{count}", "--output-file", str(dec)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(np.fromfile(dec, np.uint8).reshape(count, m), want)
    assert _files_range(prefix, n - 1, 2)[0] == -1          # past the file's rows
    os.unlink(prefix + "huffman_chunks.bin")
    assert _files_range(prefix, first, count)[0] == -1      # no index: PQH_ERR_ARG, no full decode
    r = subprocess.run([os.path.join(ROOT, "pq_huffman_amd", "bin", "huffman_decoder"), prefix,
                        "--rows", f"{first}:{count}"], capture_output=True, text=True)
    assert r.returncode == 1 and "huffman_chunks.bin" in r.stderr
