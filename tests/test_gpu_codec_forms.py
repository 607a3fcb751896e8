"""The codec kernels (pqh_huff.hip, pqh_decode.hip) in the forms the default-form tests never
launch.  Expected values come from numpy (tests/codec_forms_ref.py) and from the CPU oracle,
never from the calls under test; every comparison is array_equal or byte equality.  Each case
asserts, through the mirrored host dispatch, that its tensors reach the kernel it names.

What runs what (the numbers are the tests below, test_<number>_*):

  path                                         reached by                                 test
  -------------------------------------------  -----------------------------------------  ----
  hist_ctx_w<256,3,false>, <256,3,true>,       hist_block 256 x hist_split {0,1,2,4,8} x  1
  hist_ctx<u8,256,8>, every split other        row-major / part-major (pads 0, 5) x m in
  than 2 (the benchmark's 4x256 among them)    {8,16,12} (wave), 6 (thread); n = 130,001
  partials written with one split, reduced     partial on a hist_split = 4 context,       1
  on a context with another                    reduce on a hist_split = 1 context
  hist_flush_carry and the accumulator in      m = 16, n = 33 * 61,440 + 1 (34 chunks:    2
  the slim kernels (multi-round form)          7 groups of 5 rounds), 4x256, a constant
                                               run over one whole chunk
  hist_ctx, the `dw` branch                    PQH_HIST_IMPL=thread in a child process,   3
                                               m in {12,16}, aligned, blocks 0 and 256
  context histogram at k < 256: hist_split     k in {2,6,100,255,16} x m in {4,6} x n in  4
  fallbacks, odd k * k (half-used last word,   {1,5,70,001} x every split and block, 5%
  2 * w + 1 < items), the scalar store loop,   of the codes >= k, counts inside a
  the prev >= k || cur >= k skip               poisoned buffer
  hist_plain_rows16 at other even k, its       (8,1000), (8,258) aligned; n = 16384 * 64  5
  rows cap, its accumulate form                + 1 at (8,4096): 65 groups, the last of
                                               one row; accumulate twice
  hist_plain<u16> (odd k, m != 8, unaligned)   (8,1000) at a 2-byte offset, (8,257),      5
                                               (5,300), (20,1000)
  enc_onepass<u8,0>, <u16,16>, <u16,0>,        (24,256,ctx), (17,256); (12,1000);         6
  <u16,8>, generic <u8,8> and <u8,16> at       (20,300), (24,4096); (5,257); (8,256,ctx)
  m = 8 and 16, tiled and one-pass             and (16,256,ctx) with the codes or
                                               chunk_prev at byte 4; enc_impl 1 and 2
  bit_offset % 32 != 0, raw_first = 0 and a    two shards into one buffer at (6,256),     7
  halo row in the generic forms                (12,256), (24,256) ctx and (12,1000)
  the 0xFFFF -> u32 and ~0u -> u64 escapes     counts 2^20 / 1.5^j (codes to 21 bits)     8
  outside ROW8, CS = 1                         and 2^30 / 2^j (to ~31 bits) at (16,256),
                                               (12,256), (24,256) ctx, (8,4096),
                                               (12,4096)
  the LDS limit of the encoder                 m = 45 (161,296 bytes) encodes, m = 46 is  9
                                               refused and the error does not stick
  dec_chunks<8>, <16> (unaligned chunk_prev    m in {8,16}, ctx and plain: chunks of 33,  10
  or output, chunks > 32), dec_chunks<0,u16>,  64; of 8 with chunk_prev or the output at
  dec_rows<false,2,16>, the S halving,         byte 4; (8,1000), (8,4096) at 16 and 40;
  chunk_vectors >= n                           (12,1000); m = 16 at 1000, 4096, 8192

Test 6's chunk offsets are derived from the oracle codebooks' lengths by a numpy cumsum of the
per-row bits (ref.row_bits; test_codec_forms_cpu.py checks that against the oracle's prefix
streams).  Context streams exist only at K = 256, so test 4 checks the histogram alone."""
import dataclasses
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import ROOT
import codec_forms_ref as ref

pytestmark = pytest.mark.gpu

UNSUPPORTED = -4   # PQH_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def gpu():
    import torch
    from pq_huffman_amd import codec
    assert torch.cuda.is_available()
    return torch, codec


def _i16(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int16) if a.dtype == np.uint16 else a


def _dev(torch, codes, off=0):
    """the codes on the device, `off` bytes past a 16-byte aligned address"""
    a = _i16(codes)
    buf = torch.empty(a.nbytes + 32, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    flat = buf[off:off + a.nbytes]
    flat.copy_(torch.from_numpy(a.reshape(-1).view(np.uint8)))
    if a.dtype == np.int16:
        flat = flat.view(torch.int16)
    t = flat.view(a.shape)
    assert t.data_ptr() % 16 == off
    return t


def _parts(torch, cd, pad):
    """part-major copy [m][n + pad] of device rows [n][m], the pad filled with junk"""
    n, m = cd.shape
    parts = torch.full((m, n + pad), 0xAB, dtype=cd.dtype, device="cuda")
    parts[:, :n] = cd.t()
    return parts


def _want(torch, counts):
    assert counts.max() < 2 ** 31
    return torch.from_numpy(counts.astype(np.int32)).cuda()


def _junk(torch, like):
    return torch.full(tuple(like.shape), 12345, dtype=torch.int32, device="cuda")


def _case(item, **match):
    found = ref.cases(item, **match)
    assert found, match
    return found[0]


# ---------------------------------------------------------------- 1: every launch shape
@pytest.mark.parametrize("m", [8, 16, 12, 6])
def test_1_context_histogram_every_launch_shape(gpu, m):
    torch, codec = gpu
    n, k = ref.N_THREE_CHUNKS, 256
    # a constant run of 8,000 rows (> 4,095) across the edge of chunks 0 and 1
    codes = ref.codes_for(n, m, k, seed=300 + m, run=(58_000, 66_000, 9))
    cd = _dev(torch, codes)
    want = _want(torch, ref.hist(codes, k, True))
    halo = {s: _want(torch, ref.hist(codes[s:], k, True, prev_row=codes[s - 1])) for s in (1, 3, 64)}
    assert int(want[:, 9 * k + 9].min()) >= 7_999
    pbytes = ref.hist_plan(n, m, k)["total_bytes"]
    assert codec.histogram_partial_bytes(n, m, k) == pbytes
    partials = torch.empty(pbytes, dtype=torch.uint8, device="cuda")
    ctx, ctx_a, ctx_b = codec.Context(0), codec.Context(0), codec.Context(0)
    try:
        ctx_a.set_tuning(hist_split=4)
        ctx_b.set_tuning(hist_split=1)
        for pad in (-1, 0, 5):
            src = cd if pad < 0 else _parts(torch, cd, pad)

            def run(c, s, counts, accumulate):   # rows [s, n), row s - 1 the halo
                prev = cd[s - 1] if s else None
                if pad < 0:
                    return codec.histogram(c, cd[s:], k, True, prev_row=prev, counts=counts,
                                           accumulate=accumulate)
                return codec.histogram_parts(c, src[:, s:], n - s, k, True, prev_row=prev,
                                             counts=counts, accumulate=accumulate)

            def partial(c, s):
                prev = cd[s - 1] if s else None
                partials.fill_(0xFF)
                if pad < 0:
                    return codec.histogram_partial(c, cd[s:], k, partials, prev_row=prev)
                return codec.histogram_partial_parts(c, src[:, s:], n - s, k, partials, prev_row=prev)

            for blk in ref.HIST_BLOCKS:
                for sp in ref.HIST_SPLITS:
                    case = _case(1, m=m, pad=pad, hist_block=blk, hist_split=sp)
                    assert ref.case_form(case, codes_mod16=cd.data_ptr() % 16) == case.form
                    ctx.set_tuning(hist_block=blk, hist_split=sp)
                    tag = (pad, blk, sp)
                    got = run(ctx, 0, _junk(torch, want), False)            # set over junk
                    assert torch.equal(got, want), tag
                    for s, w in halo.items():
                        assert torch.equal(run(ctx, s, _junk(torch, want), False), w), (tag, s)
                    run(ctx, 3, got, True)                                  # accumulate
                    assert torch.equal(got, want + halo[3]), tag
                    partial(ctx, 0)                                         # partial + reduce
                    got = codec.histogram_reduce(ctx, partials, n, m, k, _junk(torch, want))
                    assert torch.equal(got, want), tag
                    partial(ctx, 1)
                    codec.histogram_reduce(ctx, partials, n - 1, m, k, got, accumulate=True)
                    assert torch.equal(got, want + halo[1]), tag
                # partials of a split-4 context reduced on a split-1 context, and back
                for blk_ctx in (ctx_a, ctx_b):
                    blk_ctx.set_tuning(hist_block=blk)
                partial(ctx_a, 0)
                got = codec.histogram_reduce(ctx_b, partials, n, m, k, _junk(torch, want))
                assert torch.equal(got, want), (pad, blk, "4 -> 1")
                partial(ctx_b, 64)
                codec.histogram_reduce(ctx_a, partials, n - 64, m, k, got, accumulate=True)
                assert torch.equal(got, want + halo[64]), (pad, blk, "1 -> 4")
    finally:
        for c in (ctx, ctx_a, ctx_b):
            c.set_tuning(hist_block=0, hist_split=0)
            c.close()


# ---------------------------------------------------------------- 2: rounds in the slim kernels
def test_2_slim_kernels_multi_round(gpu):
    torch, codec = gpu
    n, m, k = ref.N_ROUNDS, 16, 256
    plan = ref.hist_plan(n, m, k, 4)
    assert plan["rounds"] >= 2 and plan["split"] == 4
    c6 = 6 * ref.HIST_CHUNK   # chunk 6 is the second of its group: flushed before chunk 7
    codes = ref.codes_for(n, m, k, seed=77, stay=0.0, run=(c6 - 1, c6 + ref.HIST_CHUNK, 7))
    codes[20 * ref.HIST_CHUNK + 100:21 * ref.HIST_CHUNK - 100] = 8   # (an even bin: the low half)
    whole = ref.hist(codes, k, True)
    assert int(whole[:, 7 * k + 7].min()) >= ref.HIST_CHUNK   # a counter reaches 61,440
    want = _want(torch, whole)
    want1 = _want(torch, ref.hist(codes[1:], k, True, prev_row=codes[0]))
    cd = _dev(torch, codes)
    assert codec.histogram_partial_bytes(n, m, k) == plan["total_bytes"]
    partials = torch.empty(plan["total_bytes"], dtype=torch.uint8, device="cuda")
    ctx = codec.Context(0)
    try:
        ctx.set_tuning(hist_block=256, hist_split=4)
        for pad in (-1, 0):
            case = _case(2, pad=pad)
            assert ref.case_form(case, codes_mod16=cd.data_ptr() % 16) == case.form
            src = cd if pad < 0 else _parts(torch, cd, pad)
            for rep in range(2):   # the reduce leaves the accumulator cleared
                if pad < 0:
                    got = codec.histogram(ctx, cd, k, True, counts=_junk(torch, want), accumulate=False)
                else:
                    got = codec.histogram_parts(ctx, src, n, k, True, counts=_junk(torch, want),
                                                accumulate=False)
                assert torch.equal(got, want), (pad, rep)
            if pad < 0:
                codec.histogram(ctx, cd[1:], k, True, prev_row=cd[0], counts=got)
            else:
                codec.histogram_parts(ctx, src[:, 1:], n - 1, k, True, prev_row=cd[0], counts=got)
            assert torch.equal(got, want + want1), pad
            for rep in range(2):   # partial + reduce in the caller's buffer
                partials.fill_(0xFF)
                if pad < 0:
                    codec.histogram_partial(ctx, cd, k, partials)
                else:
                    codec.histogram_partial_parts(ctx, src, n, k, partials)
                got = codec.histogram_reduce(ctx, partials, n, m, k, _junk(torch, want))
                assert torch.equal(got, want), (pad, rep, "partial")
    finally:
        ctx.set_tuning(hist_block=0, hist_split=0)
        ctx.close()


# ---------------------------------------------------------------- 3: the thread form's dw branch
_THREAD_CHILD = """
import sys
import numpy as np, torch
sys.path.insert(0, %r)
from pq_huffman_amd import codec
ctx = codec.Context(0)
data = np.load(sys.argv[1])
out = {}
for m in (12, 16):
    cd = torch.from_numpy(data["m%%d" %% m]).cuda()
    assert cd.data_ptr() %% 4 == 0
    n = cd.shape[0]
    for blk in (0, 256):
        ctx.set_tuning(hist_block=blk)
        for rows in (n, 5000):
            c = codec.histogram(ctx, cd[:rows], 256, True)
            out["m%%d_b%%d_n%%d" %% (m, blk, rows)] = c.cpu().numpy()
        c = codec.histogram(ctx, cd[64:], 256, True, prev_row=cd[63])
        out["m%%d_b%%d_halo" %% (m, blk)] = c.cpu().numpy()
ctx.set_tuning(hist_block=0)
np.savez(sys.argv[2], **out)
"""


def test_3_thread_form_dword_branch(gpu):
    """PQH_HIST_IMPL is read once per process, so the thread form runs in a child: rows of 12
    and 16 bytes, 4-byte aligned, take hist_ctx's dword loads wherever a thread's whole run
    lies inside the rows (n = 130,001: two full chunks and a partial one; n = 5,000: a partial
    chunk, full and partial runs)."""
    torch, codec = gpu
    n = ref.N_THREE_CHUNKS
    codes = {m: ref.codes_for(n, m, 256, seed=500 + m, run=(58_000, 66_000, 9)) for m in (12, 16)}
    for m in codes:
        for blk in ref.HIST_BLOCKS:
            case = _case(3, m=m, hist_block=blk)
            assert ref.case_form(case) == case.form
        assert ref.hist_thread_branch(m, 0) == "dw"
    with tempfile.TemporaryDirectory() as td:
        fin, fout = os.path.join(td, "in.npz"), os.path.join(td, "out.npz")
        np.savez(fin, **{f"m{m}": c for m, c in codes.items()})
        r = subprocess.run([sys.executable, "-c", _THREAD_CHILD % ROOT, fin, fout],
                           capture_output=True, text=True,
                           env=dict(os.environ, PQH_HIST_IMPL="thread"), timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        got = dict(np.load(fout))
    for m, c in codes.items():
        for blk in ref.HIST_BLOCKS:
            for rows in (n, 5000):
                assert np.array_equal(got[f"m{m}_b{blk}_n{rows}"].view(np.uint32),
                                      ref.hist(c[:rows], 256, True)), (m, blk, rows)
            assert np.array_equal(got[f"m{m}_b{blk}_halo"].view(np.uint32),
                                  ref.hist(c[64:], 256, True, prev_row=c[63])), (m, blk)


# ---------------------------------------------------------------- 4: context histogram, k < 256
@pytest.mark.parametrize("k,splits", [(2, {1}), (6, {1}), (100, {1, 2}), (255, {1}),
                                      (16, {1, 2, 4, 8})])
def test_4_context_histogram_small_alphabets(gpu, k, splits):
    torch, codec = gpu
    poison, guard = 0x5A5A5A5A, 64
    ctx = codec.Context(0)
    reached = set()
    try:
        for m in (4, 6):
            for n in (1, 5, 70_001):
                codes = ref.codes_for(n, m, k, seed=7 * k + m + n % 11, bad=0.05)
                if n > 5:
                    assert (codes >= k).any()
                else:
                    codes[0, 0] = 255          # (k < 256: out of the alphabet)
                cd = _dev(torch, codes)
                want = _want(torch, ref.hist(codes, k, True))
                items = m * k * k
                for blk in ref.HIST_BLOCKS:
                    for sp in ref.HIST_SPLITS:
                        case = _case(4, m=m, k=k, hist_block=blk, hist_split=sp)
                        assert ref.case_form(case, codes_mod16=cd.data_ptr() % 16) == case.form
                        reached.add(ref.hist_plan(n, m, k, sp)["split"])
                        ctx.set_tuning(hist_block=blk, hist_split=sp)
                        frame = torch.full((items + 2 * guard,), poison, dtype=torch.int32, device="cuda")
                        counts = frame[guard:guard + items].view(m, k * k)
                        codec.histogram(ctx, cd, k, True, counts=counts, accumulate=False)
                        assert torch.equal(counts, want), (m, n, blk, sp)
                        assert bool((frame[:guard] == poison).all()), (m, n, blk, sp)
                        assert bool((frame[guard + items:] == poison).all()), (m, n, blk, sp)
                        codec.histogram(ctx, cd, k, True, counts=counts)   # accumulate
                        assert torch.equal(counts, 2 * want), (m, n, blk, sp)
        assert reached == splits
    finally:
        ctx.set_tuning(hist_block=0, hist_split=0)
        ctx.close()


# ---------------------------------------------------------------- 5: u16 (plain) histograms
_U16 = ref.cases(5)


@pytest.mark.parametrize("case", _U16, ids=[f"{c.id}_n{c.n[-1]}" for c in _U16])
def test_5_plain_histograms(gpu, case):
    torch, codec = gpu
    m, k = case.m, case.k
    ctx = codec.Context(0)
    try:
        for n in case.n:
            codes = ref.codes_for(n, m, k, seed=k + m + n % 13, bad=0.05, stay=0.3 if n < 5000 else 0.0)
            if n > 60:
                assert (codes >= k).any()
            cd = _dev(torch, codes, case.codes_off)
            esz = 1 if k <= 256 else 2
            assert ref.hist_form(m, k, False, esz, cd.data_ptr() % 16) == case.form
            if case.form == "hist_plain_rows16" and n == ref.N_ROWS16_CAP:
                plan = ref.rows16_plan(n)
                assert plan == dict(rows=16384, groups=65) and n - 64 * plan["rows"] == 1
            want = _want(torch, ref.hist(codes, k, False))
            frame = torch.full((m * k + 128,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            counts = frame[64:64 + m * k].view(m, k)
            codec.histogram(ctx, cd, k, False, counts=counts, accumulate=False)   # set over junk
            assert torch.equal(counts, want), n
            assert bool((frame[:64] == 0x5A5A5A5A).all()) and bool((frame[64 + m * k:] == 0x5A5A5A5A).all())
            counts.zero_()
            for rep in (1, 2):
                codec.histogram(ctx, cd, k, False, counts=counts)                 # accumulate
                assert torch.equal(counts, rep * want), (n, rep)
    finally:
        ctx.close()


# ---------------------------------------------------------------- encoder helpers
def _offset_rows(torch, rows, m, dtype, off, fill=0xCD):
    """an uninitialised [rows][m] tensor `off` bytes past an 8-byte aligned address"""
    esz = 2 if dtype == torch.int16 else 1
    buf = torch.full((rows * m * esz + 16,), fill, dtype=torch.uint8, device="cuda")
    flat = buf[off:off + rows * m * esz]
    if esz == 2:
        flat = flat.view(torch.int16)
    t = flat.view(rows, m)
    assert t.data_ptr() % 8 == off
    return t


def _encode(torch, codec, ctx, tabs, cd, cv, prev_off=0, parts=None, always_prev=False):
    """encode_size + encode_write into a zeroed buffer inside a poisoned frame; returns the
    Encoded and the frame check"""
    n, m = cd.shape
    bits = int(codec.encode_size(ctx, tabs, cd).item())
    nbytes = ((bits + 31) // 32 + 1) * 4
    frame = torch.full((nbytes + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    out = frame[32:32 + nbytes]
    out.zero_()
    chunks = (n + cv - 1) // cv
    coff = torch.full((chunks,), -1, dtype=torch.int64, device="cuda")
    cprev = _offset_rows(torch, chunks, m, cd.dtype, prev_off) if (tabs.context or always_prev) else None
    tot = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    if parts is None:
        codec.encode_write(ctx, tabs, cd, out, 0, 1, None, cv, coff, cprev if tabs.context else None, tot)
    else:
        codec.encode_write_parts(ctx, tabs, parts, n, out, 0, 1, None, cv, coff,
                                 cprev if tabs.context else None, tot)
    codec.encode_status(ctx)
    assert int(tot.item()) == bits
    assert bool((frame[:32] == 0xEE).all()) and bool((frame[32 + nbytes:] == 0xEE).all())
    return codec.Encoded(out, bits, cv, coff, cprev, n, 1)


def _tables(torch, codec, ctx, oracle, cd, codes, k, ctxm):
    tabs = codec.Tables(ctx, cd.shape[1], k, ctxm).build(codec.histogram(ctx, cd, k, ctxm))
    tabs.status()
    return tabs, oracle.build_codebooks(codes, k, ctxm)


def _check_stream(enc, want, bits):
    assert enc.bits == bits
    got = enc.stream.cpu().numpy().tobytes()
    assert got[:len(want)] == want
    assert not any(got[len(want):])          # nothing written past the stream's last byte


def _check_decode(torch, codec, ctx, oracle, tabs, ocb, enc, codes):
    n, m = codes.shape
    if m <= 16:
        dec = codec.decode(ctx, tabs, enc)
        codec.decode_status(ctx)
        assert np.array_equal(dec.cpu().numpy(), _i16(codes))
    else:   # pqh_decode refuses m > 16: the oracle decodes the GPU's bytes
        with pytest.raises(codec.PqhError) as e:
            codec.decode(ctx, tabs, enc)
        assert e.value.status == UNSUPPORTED
        got = enc.stream[:enc.nbytes].cpu().numpy().tobytes()
        assert np.array_equal(oracle.decode(got, n, m, ocb), codes)


def _twin(case, **kw):
    """the same case under the other enc_impl"""
    if "enc_impl" in kw:   # the case's form names the tiled or the one-pass kernel
        tile = 2 - kw["enc_impl"]
        kw["form"] = case.form.replace("tile=0", f"tile={tile}").replace("tile=1", f"tile={tile}")
    return dataclasses.replace(case, **kw)


# ---------------------------------------------------------------- 6: every encoder instantiation
_ENC6 = ref.cases(6, enc_impl=1)


@pytest.mark.parametrize("case", _ENC6, ids=[c.id + "_" + c.form.split("<")[1].split(",cs")[0].replace(",", "_")
                                             for c in _ENC6])
def test_6_encoder_instantiations(gpu, oracle, case):
    torch, codec = gpu
    m, k, ctxm = case.m, case.k, case.context
    nmax = max(case.n)
    codes = ref.codes_for(nmax, m, k, seed=600 + m + k % 97)
    cd = _dev(torch, codes, case.codes_off)
    parts = _parts(torch, cd, case.pad) if case.pad >= 0 else None
    for impl in (1, 2):
        ctx = codec.Context(0)   # a fresh context: its own scratch and look-back state
        try:
            ctx.set_tuning(enc_impl=impl)
            tabs, ocb = _tables(torch, codec, ctx, oracle, cd, codes, k, ctxm)
            twin = _twin(case, enc_impl=impl)
            assert twin in ref.CASES
            for n in case.n:
                want, bits = oracle.encode(codes[:n], ocb)
                rb = ref.row_bits(codes[:n], ocb.lens, k, ctxm)
                assert int(rb.sum()) == bits
                for cv in case.chunk_vectors:
                    enc = _encode(torch, codec, ctx, tabs, cd[:n], cv, case.prev_off, parts)
                    prev_mod = enc.chunk_prev.data_ptr() % 8 if ctxm else 0
                    assert ref.case_form(twin, codes_mod16=cd.data_ptr() % 16,
                                         prev_mod8=prev_mod) == twin.form
                    tag = (impl, n, cv)
                    _check_stream(enc, want, bits)
                    assert np.array_equal(enc.chunk_offsets.cpu().numpy(), ref.chunk_offsets(rb, cv)), tag
                    if ctxm and n > cv:
                        assert np.array_equal(enc.chunk_prev[1:].cpu().numpy(), codes[cv - 1:n - 1:cv]), tag
                    _check_decode(torch, codec, ctx, oracle, tabs, ocb, enc, codes[:n])
        finally:
            ctx.set_tuning(enc_impl=0)
            ctx.close()


# ---------------------------------------------------------------- 7: offset and halo
_ENC7 = ref.cases(7, enc_impl=1)


@pytest.mark.parametrize("case", _ENC7, ids=[c.id for c in _ENC7])
def test_7_generic_forms_offset_and_halo(gpu, oracle, case):
    """Two shards written into one buffer (encode_size, then encode_write at the first
    shard's length) == the oracle's one-shot stream: the second shard starts inside a word,
    raw_first = 0, its row 0 in the context of the halo row."""
    torch, codec = gpu
    m, k, ctxm = case.m, case.k, case.context
    n = case.n[0]
    codes = ref.codes_for(n, m, k, seed=700 + m)
    cd = _dev(torch, codes)
    for impl in (1, 2):
        ctx = codec.Context(0)
        try:
            ctx.set_tuning(enc_impl=impl)
            twin = _twin(case, enc_impl=impl)
            assert twin in ref.CASES
            assert ref.case_form(twin, codes_mod16=cd.data_ptr() % 16) == twin.form
            tabs, ocb = _tables(torch, codec, ctx, oracle, cd, codes, k, ctxm)
            want, bits = oracle.encode(codes, ocb)
            rb = ref.row_bits(codes, ocb.lens, k, ctxm)
            ends = np.cumsum(rb)
            cut = 1500 + int(np.flatnonzero(ends[1499:] % 32 != 0)[0])   # rows [0, cut), [cut, n)
            ta = int(ends[cut - 1])
            assert ta % 32 != 0
            a, b = cd[:cut], cd[cut:]
            halo = cd[cut - 1] if ctxm else None
            assert int(codec.encode_size(ctx, tabs, a, 1, None).item()) == ta
            assert int(codec.encode_size(ctx, tabs, b, 0, halo).item()) == bits - ta
            out = torch.zeros(((bits + 31) // 32 + 1) * 4, dtype=torch.uint8, device="cuda")
            cv = 64
            chunks = (n - cut + cv - 1) // cv
            coff = torch.full((chunks,), -1, dtype=torch.int64, device="cuda")
            cprev = _offset_rows(torch, chunks, m, cd.dtype, 0) if ctxm else None
            codec.encode_write(ctx, tabs, a, out, 0, 1, None, 0)
            codec.encode_write(ctx, tabs, b, out, ta, 0, halo, cv, coff, cprev)
            codec.encode_status(ctx)
            got = out.cpu().numpy().tobytes()
            assert got[:len(want)] == want and not any(got[len(want):]), impl
            assert np.array_equal(coff.cpu().numpy(), ref.chunk_offsets(rb[cut:], cv, ta)), impl
            if ctxm:
                assert np.array_equal(cprev.cpu().numpy(), codes[cut - 1:n - 1:cv]), impl
        finally:
            ctx.set_tuning(enc_impl=0)
            ctx.close()


# ---------------------------------------------------------------- 8: long codes
_ENC8 = ref.cases(8, enc_impl=1)


@pytest.mark.parametrize("deep", [False, True], ids=["to21bits", "past26bits"])
@pytest.mark.parametrize("case", _ENC8, ids=[c.id for c in _ENC8])
def test_8_long_codes_outside_the_row_encoder(gpu, oracle, case, deep):
    """The gather copies' escapes: a u16 entry 0xFFFF sends a code longer than 12 bits to the
    u32 copy (ROW8 only), a u32 entry ~0u one longer than 26 bits to the u64 table.  The counts
    2^20 / 1.5^j give codes of up to 21 bits, so the second escape needs the deeper family
    2^30 / 2^j (codes to ~31 bits); both are run."""
    torch, codec = gpu
    m, k, ctxm = case.m, case.k, case.context
    n, cv = case.n[0], case.chunk_vectors[0]
    counts = ref.long_code_counts(m, k, ctxm, deep)
    ocb = ref.oracle_codebooks(oracle, counts, k, ctxm)
    codes = ref.long_code_rows(n, m, k, seed=8 + m)
    part = np.arange(m)[None, :]
    c = codes.astype(np.int64)
    used = ocb.lens[part, c[:-1] * k + c[1:]] if ctxm else ocb.lens[part, c]
    assert used.min() >= 1 and used.max() > 12
    assert (used.max() > 26) == deep
    want, bits = oracle.encode(codes, ocb)
    rb = ref.row_bits(codes, ocb.lens, k, ctxm)
    cd = _dev(torch, codes)
    for impl in (1, 2):
        ctx = codec.Context(0)
        try:
            ctx.set_tuning(enc_impl=impl)
            twin = _twin(case, enc_impl=impl)
            assert twin in ref.CASES
            tabs = codec.Tables(ctx, m, k, ctxm).build(torch.from_numpy(counts.astype(np.int32)).cuda())
            tabs.status()
            enc = _encode(torch, codec, ctx, tabs, cd, cv)
            prev_mod = enc.chunk_prev.data_ptr() % 8 if ctxm else 0
            assert ref.case_form(twin, codes_mod16=cd.data_ptr() % 16, prev_mod8=prev_mod) == twin.form
            _check_stream(enc, want, bits)
            assert np.array_equal(enc.chunk_offsets.cpu().numpy(), ref.chunk_offsets(rb, cv)), impl
            _check_decode(torch, codec, ctx, oracle, tabs, ocb, enc, codes)
        finally:
            ctx.set_tuning(enc_impl=0)
            ctx.close()


# ---------------------------------------------------------------- 9: the LDS limit
@pytest.mark.parametrize("impl", [1, 2])
def test_9_encoder_lds_limit(gpu, oracle, impl):
    torch, codec = gpu
    n, k = 600, 256
    fits, over = _case(9, m=45, enc_impl=impl), _case(9, m=46, enc_impl=impl)
    assert ref.enc_lds_bytes(45, k, False) == 161_296
    assert ref.case_form(fits) == fits.form and ref.case_form(over) == over.form == ref.UNSUPPORTED
    codes = ref.codes_for(n, 46, k, seed=9)
    ctx = codec.Context(0)
    try:
        ctx.set_tuning(enc_impl=impl)
        c45 = np.ascontiguousarray(codes[:, :45])
        cd45, cd46 = _dev(torch, c45), _dev(torch, codes)
        tabs45, ocb = _tables(torch, codec, ctx, oracle, cd45, c45, k, False)
        tabs46, _ = _tables(torch, codec, ctx, oracle, cd46, codes, k, False)
        want, bits = oracle.encode(c45, ocb)
        for rep in range(2):
            enc = _encode(torch, codec, ctx, tabs45, cd45, 64)
            _check_stream(enc, want, bits)
            _check_decode(torch, codec, ctx, oracle, tabs45, ocb, enc, c45)
            if rep == 0:   # m = 46 is refused, and the next encode on this context succeeds
                with pytest.raises(codec.PqhError) as e:
                    _encode(torch, codec, ctx, tabs46, cd46, 64)
                assert e.value.status == UNSUPPORTED
                codec.encode_status(ctx)
    finally:
        ctx.set_tuning(enc_impl=0)
        ctx.close()


# ---------------------------------------------------------------- 10: decoder forms
def _dec_shapes():
    seen = []
    for c in ref.cases(10):
        if (c.m, c.k, c.context) not in seen:
            seen.append((c.m, c.k, c.context))
    return seen


@pytest.mark.parametrize("m,k,ctxm", _dec_shapes())
def test_10_decoder_forms(gpu, oracle, m, k, ctxm):
    torch, codec = gpu
    n = ref.DEC_N
    codes = ref.codes_for(n, m, k, seed=1000 + m + k % 89)
    cd = _dev(torch, codes)
    esz = 1 if k <= 256 else 2
    ctx = codec.Context(0)
    try:
        tabs, ocb = _tables(torch, codec, ctx, oracle, cd, codes, k, ctxm)
        want, bits = oracle.encode(codes, ocb)
        for case in ref.cases(10, m=m, k=k, context=ctxm):
            for cv in case.chunk_vectors:
                tag = (case.id, cv)
                # (a plain stream's chunk_prev is not read, but its address picks the form)
                enc = _encode(torch, codec, ctx, tabs, cd, cv, case.prev_off, always_prev=True)
                _check_stream(enc, want, bits)          # the encoder tests' stream
                frame = torch.full((n * m * esz + 64,), 0x77, dtype=torch.uint8, device="cuda")
                flat = frame[32 + case.out_off:32 + case.out_off + n * m * esz]
                out = (flat.view(torch.int16) if esz == 2 else flat).view(n, m)
                got = ref.dec_form(m, k, ctxm, cv, enc.chunk_prev.data_ptr() % 8, out.data_ptr() % 8)
                assert got == case.form, tag
                if case.form == ref.UNSUPPORTED:
                    with pytest.raises(codec.PqhError) as e:
                        codec.decode(ctx, tabs, enc, out=out)
                    assert e.value.status == UNSUPPORTED
                    continue
                if cv >= 1000:
                    assert ref.dec_stage_rows(m, k, cv) < cv          # staged in several batches
                codec.decode(ctx, tabs, enc, out=out)
                codec.decode_status(ctx)
                assert np.array_equal(out.cpu().numpy(), _i16(codes)), tag
                lo, hi = 32 + case.out_off, 32 + case.out_off + n * m * esz
                assert bool((frame[:lo] == 0x77).all()) and bool((frame[hi:] == 0x77).all()), tag
    finally:
        ctx.close()
