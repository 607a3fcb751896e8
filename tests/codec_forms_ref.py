"""References for the codec-forms tests (test infrastructure): a numpy histogram that is the
definition of the symbol counts, mirrors of the host dispatch of the histogram, the stream
encoder and the stream decoder (which kernel instantiation a call runs), and CASES, the list
of GPU cases with the form each one is meant to reach.

The mirrors restate pq_huffman_amd/csrc/hip/pqh_huff.hip (histogram_impl, hist_split,
hist_plan, encode_write_impl), pqh_decode.hip (pqh_decode), pqh_decode_dev.h
(packed_row_words) and pqh_tables.hip (pqh_tables_alloc); tests/test_codec_forms_cpu.py pins
them.  The expected forms in CASES are written out, not computed by the mirrors, so that a GPU
test's `form(actual pointers) == case.form` says the case reaches the kernel it was written
for."""
from __future__ import annotations

import dataclasses

import numpy as np

import datagen

HIST_CHUNK = 61440      # kHistChunk: vectors per context-histogram workgroup
HIST_WGS = 256          # PQH_HIST_WGS default: the multi-round grid's workgroups
ENC_BLOCK = 512         # kEncBlock
MAX_CODE_LEN = 56       # kMaxCodeLen (pqh_internal.h)
LDS_LIMIT = 160 * 1024
UNSUPPORTED = "unsupported"


# ------------------------------------------------------------------------- the definition
def hist(codes: np.ndarray, k: int, context: bool, prev_row=None) -> np.ndarray:
    """int64 [m][k * k or k]: counts[i][prev * k + cur] over consecutive rows (context; row 0's
    predecessor is prev_row, or nothing), or counts[i][cur] (plain).  A pair or a symbol with a
    value >= k is dropped (huffman_encoder.c:139-205 on in-alphabet codes)."""
    codes = np.asarray(codes)
    if codes.dtype == np.int16:
        codes = codes.view(np.uint16)
    n, m = codes.shape
    items = k * k if context else k
    out = np.zeros((m, items), np.int64)
    p0 = None
    if context and prev_row is not None:
        p0 = np.asarray(prev_row)
        p0 = (p0.view(np.uint16) if p0.dtype == np.int16 else p0).astype(np.int64).reshape(m)
    for i in range(m):   # (a part at a time: the temporaries of 2M x 16 rows stay small)
        cur = codes[:, i].astype(np.int64)
        if not context:
            idx = cur[cur < k]
        else:
            prev = cur[:-1] if p0 is None else np.concatenate([p0[i:i + 1], cur[:-1]])
            if p0 is None:
                cur = cur[1:]
            ok = (prev < k) & (cur < k)
            idx = prev[ok] * k + cur[ok]
        out[i] = np.bincount(idx, minlength=items)
    return out


# ------------------------------------------------------------------------- histogram dispatch
def hist_split(k: int, want: int = 0) -> int:
    """pqh_huff.hip hist_split (:1138-1146): the split asked for (0: the default, 2) if k is a
    multiple of twice it, else 2 if k % 4 == 0, else 1."""
    want = want if want > 0 else 2
    return want if k % (2 * want) == 0 else (2 if k % 4 == 0 else 1)


def hist_plan(n: int, m: int, k: int, split_want: int = 0) -> dict:
    """pqh_huff.hip hist_plan (:1148-1173): split, chunks, rounds, groups, the packed words of
    one partial image and the byte layout [partials][pad to 256][u32 carries if rounds > 1]."""
    chunks = (n + HIST_CHUNK - 1) // HIST_CHUNK
    gt = max(8, (HIST_WGS // (m * 2)) // 8 * 8)
    if chunks <= 4 * gt:
        rounds, groups = 1, chunks
    else:
        rounds = (chunks + gt - 1) // gt
        groups = (chunks + rounds - 1) // rounds
    words = (k * k + 1) // 2
    partial = m * groups * words * 4
    acc_offset = (partial + 255) & ~255
    total = acc_offset + m * k * k * 4 if rounds > 1 else partial
    return dict(split=hist_split(k, split_want), chunks=chunks, rounds=rounds, groups=groups,
                words=words, partial_bytes=partial, acc_offset=acc_offset, total_bytes=total)


def hist_form(m: int, k: int, context: bool, code_bytes: int, addr_mod16: int, ldc: int = 0,
              hist_block: int = 0, hist_split: int = 0, impl_env: str = "") -> str:
    """The kernel histogram_impl launches (pqh_huff.hip:1188-1304).  Context (:1198-1273):
    k > 256 is refused (:1188); wave_form = ldc or (not PQH_HIST_IMPL=thread and m % 4 == 0 and
    the codes aligned to 16 bytes at m = 8, else 4) (:1240); slim = hist_block == 256 (:1238).
    Plain: wide16 = k > 256, row-major, m == 8, even k <= 4096, 16-byte aligned (:1193-1194);
    else hist_plain of the code type (:1297-1303).  hist_split does not pick the kernel (it is
    an argument); it is here so a case names its whole launch shape."""
    del hist_split
    if context:
        if k > 256:
            return UNSUPPORTED
        assert code_bytes == 1
        thread_form = impl_env == "thread"
        wave = bool(ldc) or (not thread_form and m % 4 == 0 and
                             addr_mod16 % (16 if m == 8 else 4) == 0)
        slim = hist_block == 256
        if wave:
            pm = "true" if ldc else "false"
            return f"hist_ctx_w<256,3,{pm}>" if slim else f"hist_ctx_w<1024,5,{pm}>"
        return "hist_ctx<u8,256,8>" if slim else "hist_ctx<u8,1024,20>"
    wide16 = k > 256 and not ldc and m == 8 and k % 2 == 0 and k <= 4096 and addr_mod16 == 0
    if wide16:
        return "hist_plain_rows16"
    return "hist_plain<u8>" if k <= 256 else "hist_plain<u16>"


def hist_thread_branch(m: int, addr_mod4: int) -> str:
    """The load form of hist_ctx for a thread whose whole run lies inside the rows
    (pqh_huff.hip:115-120): "wide" at m == 8, "dw" for other m % 4 == 0 on 4-byte aligned
    codes, else "scalar" (partial runs are always scalar)."""
    if m == 8:
        return "wide"
    return "dw" if m % 4 == 0 and addr_mod4 == 0 else "scalar"


def rows16_plan(n: int) -> dict:
    """hist_plain_rows16's grid (pqh_huff.hip:1281-1282): rows per workgroup and groups."""
    rows = max(1, min(16384, (n + 63) // 64))
    return dict(rows=rows, groups=(n + rows - 1) // rows)


# ------------------------------------------------------------------------- encoder dispatch
def enc_lds_bytes(m: int, k: int, row8: bool) -> int:
    """the LDS image of one workgroup (pqh_huff.hip:1437-1439)"""
    blk = 256 if row8 or m <= 8 else ENC_BLOCK
    return (blk * (8 if row8 else m) * MAX_CODE_LEN // 32 + 4) * 4


def enc_form(m: int, k: int, codes_mod8: int = 0, chunk_prev_mod8: int = 0, ldc: int = 0,
             tree: bool = False, enc_impl: int = 0) -> str:
    """The kernel encode_write_impl launches (pqh_huff.hip:1416-1574).  Part-major codes need
    k <= 256, m in {8, 16}, no tree order and an 8-byte aligned chunk_prev (:1416-1418);
    row8 = k <= 256, m in {8, 16}, no tree order, codes (unless part-major) and chunk_prev
    8-byte aligned (:1432-1434); cs = m / 8 with row8 (:1435); the workgroup is 256 rows with
    row8 or m <= 8, else 512 (:1437, and B in PQH_ENC_T / PQH_ENC_PM); an image above 160 KB is
    refused (:1440); enc_impl 2 is the one-pass form, anything else the tiled one
    (:1451, :1462); the template arguments (:1504-1517, :1561-1574)."""
    if ldc and (k > 256 or m not in (8, 16) or tree or chunk_prev_mod8):
        return UNSUPPORTED
    row8 = (k <= 256 and m in (8, 16) and not tree and (bool(ldc) or codes_mod8 == 0) and
            chunk_prev_mod8 == 0)
    if enc_lds_bytes(m, k, row8) > LDS_LIMIT:
        return UNSUPPORTED
    tile = 0 if enc_impl == 2 else 1
    t = "u8" if k <= 256 else "u16"
    if row8:
        return f"enc_onepass<u8,8,256,row8,cs={m // 8},pm={int(bool(ldc))},tile={tile}>"
    maxm = 8 if m <= 8 else 16 if m <= 16 else 0
    blk = 256 if maxm == 8 else ENC_BLOCK
    return f"enc_onepass<{t},{maxm},{blk},generic,cs=1,pm=0,tile={tile}>"


# ------------------------------------------------------------------------- decoder dispatch
def dec_tables(m: int, k: int, context: bool) -> tuple[int, int]:
    """(tables, l1_bits) of a table set (pqh_tables.hip:1856-1863)"""
    return m * (k if context else 1), (9 if context else 13 if k > 256 else 11)


def dec_stage_rows(m: int, k: int, chunk_vectors: int) -> int:
    """S, the vectors a lane stages per batch: chunk_vectors halved (rounding up) until 64 lanes'
    batches fit 16 KB (pqh_decode.hip:500-501)"""
    esz = 1 if k <= 256 else 2
    s = chunk_vectors
    while s > 1 and 64 * s * m * esz > 16 * 1024:
        s = (s + 1) // 2
    return s


def packed_row_words(m: int, k: int, chunk_prev_mod8: int) -> int:
    """pqh_decode_dev.h packed_row_words (:360-366)"""
    esz = 1 if k <= 256 else 2
    rb = m * esz
    return rb // 8 if rb in (8, 16) and (esz == 1 or m == 8) and chunk_prev_mod8 == 0 else 0


def dec_form(m: int, k: int, context: bool, chunk_vectors: int, chunk_prev_mod8: int = 0,
             out_mod8: int = 0, tables: int = None, l1_bits: int = None) -> str:
    """The kernel pqh_decode launches (pqh_decode.hip:472-559): m > 16 is refused (:480);
    lds_l1 = the meta words and the first level fit 48 KB (:490-492); the staging S and the
    160 KB limit (:497-504); the whole-row decoder for packed rows, chunk_vectors <= 32 and an
    8-byte aligned output (:507-509; streams below 2^31 words, which every test stream is);
    else dec_chunks with the parts at compile time for u8 rows of 8 and 16 (:552-555)."""
    if m > 16 or (context and k != 256):   # (pqh_tables.hip:1846: context tables are K = 256)
        return UNSUPPORTED
    if tables is None:
        tables, l1_bits = dec_tables(m, k, context)
    esz = 1 if k <= 256 else 2
    l1_bytes = (tables << l1_bits) * 2
    meta_bytes = (tables * 4 + 15) & ~15
    lds_l1 = meta_bytes + l1_bytes <= 48 * 1024
    sym_bits = 12 if k <= 256 else 14
    span = (64 * chunk_vectors * m * sym_bits + 31) // 32 + 8
    win = min(4096, max(256, span))
    s = dec_stage_rows(m, k, chunk_vectors)
    lds = meta_bytes + (((l1_bytes + 15) & ~15) if lds_l1 else 0) + (win + 4) * 4 + 64 * s * m * esz + 16
    if lds > LDS_LIMIT:
        return UNSUPPORTED
    nw = packed_row_words(m, k, chunk_prev_mod8)
    if nw and chunk_vectors <= 32 and out_mod8 == 0:
        ctx = "true" if (context and k <= 256) else "false"
        return f"dec_rows<{ctx},{nw},{8 * esz}>"
    l1 = "true" if lds_l1 else "false"
    if esz == 2:
        return f"dec_chunks<0,u16,{l1}>"
    mt = m if m in (8, 16) else 0
    return f"dec_chunks<{mt},u8,{l1}>"


# ------------------------------------------------------------------------- code generators
def codes_for(n: int, m: int, k: int, seed: int, bad: float = 0.0, stay: float = 0.3,
              run: tuple = None) -> np.ndarray:
    """datagen.skewed_codes over an alphabet of k (uint8 / uint16), optionally with a share
    `bad` of symbols replaced by values in [k, 2^bits) and a constant run codes[a:b] = c."""
    if k < 256:
        codes = (datagen.skewed_codes(n, m, 256, seed=seed, stay=stay) % k).astype(np.uint8)
    else:
        codes = datagen.skewed_codes(n, m, k, seed=seed, stay=stay)
    top = 256 if codes.dtype == np.uint8 else 65536
    if bad > 0 and k < top:
        rng = np.random.default_rng(seed + 10_000)
        hit = rng.random(codes.shape) < bad
        codes[hit] = rng.integers(k, top, int(hit.sum())).astype(codes.dtype)
    if run is not None:
        a, b, c = run
        codes[a:b] = c
    return np.ascontiguousarray(codes)


def long_code_counts(m: int, k: int, context: bool, deep: bool = False) -> np.ndarray:
    """counts 2^20 / 1.5^j rolled per context and part (the counts of
    test_gpu_decode_tables_long_codes): every pair coded, codes of 2 to 21 bits, so past the
    12 bits of the u16 gather copy.  deep: 2^30 / 2^j instead, whose ~225 (or ~4,065) symbols of
    count 1 sit below a chain of 22 (18) levels: codes of 1 to ~31 bits, past the 26 bits of the
    u32 gather copy."""
    j = np.minimum(np.arange(k), 64).astype(np.float64)
    w = np.maximum(1, np.floor(2.0 ** 30 / 2.0 ** j if deep else 2.0 ** 20 / 1.5 ** j)).astype(np.int64)
    if not context:
        return np.stack([np.roll(w, (7 + i) % k) for i in range(m)])
    counts = np.zeros((m, k * k), np.int64)
    for i in range(m):
        for c in range(k):
            counts[i, c * k:(c + 1) * k] = np.roll(w, (7 * c + i) % k)
    return counts


def long_code_rows(n: int, m: int, k: int, seed: int = 3) -> np.ndarray:
    """uniform codes: with the long-code counts most symbols (and pairs) are the rare ones"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, k, (n, m)).astype(np.uint8 if k <= 256 else np.uint16)


def oracle_codebooks(oracle, counts: np.ndarray, k: int, context: bool, stride: int = 8):
    """the oracle's codebooks of given counts [m][items] (oracle.build_codebooks minus its
    histogram)"""
    both = [oracle.codebook(k, np.asarray(c, np.float64), context, stride) for c in counts]
    return oracle.Codebooks(k, context, np.stack([b[0] for b in both]),
                            np.stack([b[1] for b in both]), stride)


def row_bits(codes: np.ndarray, lens: np.ndarray, k: int, context: bool, prev_row=None) -> np.ndarray:
    """int64 [n]: the bits of every row from the codebooks' lengths lens [m][items] (context:
    row 0 is 8 raw bits a part unless prev_row gives its context)"""
    codes = np.asarray(codes)
    if codes.dtype == np.int16:
        codes = codes.view(np.uint16)
    c = codes.astype(np.int64)
    n, m = c.shape
    part = np.arange(m)[None, :]
    if not context:
        return lens[part, c].sum(1).astype(np.int64)
    out = np.empty(n, np.int64)
    out[1:] = lens[part, c[:-1] * k + c[1:]].sum(1)
    if prev_row is None:
        out[0] = 8 * m
    else:
        p = np.asarray(prev_row).astype(np.int64).reshape(1, m)
        out[0] = lens[part, p * k + c[:1]].sum()
    return out


def chunk_offsets(bits: np.ndarray, chunk_vectors: int, bit_offset: int = 0) -> np.ndarray:
    """the stream bit at which every chunk_vectors-th row starts"""
    start = np.concatenate([[0], np.cumsum(bits)[:-1]]) + bit_offset
    return start[::chunk_vectors].astype(np.int64)


# ------------------------------------------------------------------------- the GPU cases
@dataclasses.dataclass(frozen=True)
class Case:
    item: int                 # the test (numbered as in test_gpu_codec_forms.py's table)
    kind: str                 # "hist" | "enc" | "dec"
    m: int
    k: int
    context: bool
    form: str                 # the instantiation the case is meant to reach
    n: tuple = ()             # row counts
    codes_off: int = 0        # byte offset of the codes from a 16-byte aligned address
    prev_off: int = 0         # byte offset of chunk_prev from an 8-byte aligned address
    out_off: int = 0          # byte offset of the decoded rows from an 8-byte aligned address
    pad: int = -1             # part-major: ldc = n + pad (-1: row-major)
    hist_block: int = 0
    hist_split: int = 0
    impl_env: str = ""
    enc_impl: int = 1
    chunk_vectors: tuple = ()

    @property
    def id(self) -> str:
        s = f"m{self.m}k{self.k}{'c' if self.context else 'p'}"
        if self.codes_off:
            s += f"_codes{self.codes_off}"
        if self.prev_off:
            s += f"_prev{self.prev_off}"
        if self.out_off:
            s += f"_out{self.out_off}"
        if self.pad >= 0:
            s += f"_pm{self.pad}"
        return s


HIST_BLOCKS = (0, 256)
HIST_SPLITS = (0, 1, 2, 4, 8)
N_THREE_CHUNKS = 130_001                   # two full chunks of 61,440 and a partial one
N_ROUNDS = 33 * HIST_CHUNK + 1             # m = 16: gt = 8; 34 chunks > 32: 7 groups of 5 rounds
N_ROWS16_CAP = 16384 * 64 + 1              # hist_plain_rows16: the rows cap, 65 groups

_W = {0: "hist_ctx_w<1024,5,false>", 256: "hist_ctx_w<256,3,false>"}
_P = {0: "hist_ctx_w<1024,5,true>", 256: "hist_ctx_w<256,3,true>"}
_T = {0: "hist_ctx<u8,1024,20>", 256: "hist_ctx<u8,256,8>"}


def _hist_cases():
    out = []
    for blk in HIST_BLOCKS:
        for sp in HIST_SPLITS:
            for m in (8, 16, 12, 6):       # 1: every launch shape of the context histogram
                out.append(Case(1, "hist", m, 256, True, (_T if m == 6 else _W)[blk],
                                (N_THREE_CHUNKS,), hist_block=blk, hist_split=sp))
                for pad in (0, 5):
                    out.append(Case(1, "hist", m, 256, True, _P[blk], (N_THREE_CHUNKS,), pad=pad,
                                    hist_block=blk, hist_split=sp))
            for k in (2, 6, 100, 255, 16):  # 4: k < 256 (m = 4 the wave form, m = 6 the thread form)
                for m in (4, 6):
                    out.append(Case(4, "hist", m, k, True, (_T if m == 6 else _W)[blk],
                                    (1, 5, 70_001), hist_block=blk, hist_split=sp))
    for pad in (-1, 0):                     # 2: two rounds in the slim kernels
        out.append(Case(2, "hist", 16, 256, True, (_P if pad >= 0 else _W)[256], (N_ROUNDS,),
                        pad=pad, hist_block=256, hist_split=4))
    for m in (12, 16):                      # 3: PQH_HIST_IMPL=thread, the dw branch
        for blk in HIST_BLOCKS:
            out.append(Case(3, "hist", m, 256, True, _T[blk], (N_THREE_CHUNKS, 5000),
                            hist_block=blk, impl_env="thread"))
    ns = (1, 63, 64, 65, 4097)              # 5: u16 (and one u8) plain histograms
    out += [Case(5, "hist", 8, 1000, False, "hist_plain_rows16", ns),
            Case(5, "hist", 8, 258, False, "hist_plain_rows16", ns),
            Case(5, "hist", 8, 1000, False, "hist_plain<u16>", ns, codes_off=2),
            Case(5, "hist", 8, 257, False, "hist_plain<u16>", ns),
            Case(5, "hist", 5, 300, False, "hist_plain<u16>", ns),
            Case(5, "hist", 20, 1000, False, "hist_plain<u16>", ns),
            Case(5, "hist", 5, 200, False, "hist_plain<u8>", ns),
            Case(5, "hist", 8, 4096, False, "hist_plain_rows16", (N_ROWS16_CAP,))]
    return out


ENC_N = (255, 256, 257, 511, 512, 513, 3001)   # the tile edges of the 256- and the 512-row block
ENC_CHUNKS = (1, 7, 300, 4096)                 # 300 spans tiles; 4096 >= n


def _e(t, maxm, tile):
    return f"enc_onepass<{t},{maxm},{256 if maxm == 8 else 512},generic,cs=1,pm=0,tile={tile}>"


def _r(cs, pm, tile):
    return f"enc_onepass<u8,8,256,row8,cs={cs},pm={pm},tile={tile}>"


def _enc_cases():
    out = []
    for impl in (1, 2):
        tile = 2 - impl
        kw = dict(n=ENC_N, chunk_vectors=ENC_CHUNKS, enc_impl=impl)
        out += [   # 6: every instantiation, byte-exact
            Case(6, "enc", 24, 256, True, _e("u8", 0, tile), **kw),
            Case(6, "enc", 17, 256, False, _e("u8", 0, tile), **kw),
            Case(6, "enc", 12, 1000, False, _e("u16", 16, tile), **kw),
            Case(6, "enc", 20, 300, False, _e("u16", 0, tile), **kw),
            Case(6, "enc", 24, 4096, False, _e("u16", 0, tile), **kw),
            Case(6, "enc", 8, 256, True, _e("u8", 8, tile), codes_off=4, **kw),
            Case(6, "enc", 16, 256, True, _e("u8", 16, tile), codes_off=4, **kw),
            Case(6, "enc", 8, 256, True, _e("u8", 8, tile), prev_off=4, **kw),
            Case(6, "enc", 16, 256, True, _e("u8", 16, tile), prev_off=4, **kw),
            Case(6, "enc", 5, 257, False, _e("u16", 8, tile), **kw),
            # (the 8-byte-row forms, so that every form has a case here; the default-form tests
            # cover them in depth)
            Case(6, "enc", 8, 256, True, _r(1, 0, tile), **kw),
            Case(6, "enc", 16, 256, True, _r(2, 0, tile), **kw),
            Case(6, "enc", 8, 256, True, _r(1, 1, tile), pad=5, **kw),
            Case(6, "enc", 16, 256, True, _r(2, 1, tile), pad=5, **kw),
        ]
        for m, k, c, f in ((6, 256, True, _e("u8", 8, tile)), (12, 256, True, _e("u8", 16, tile)),
                           (24, 256, True, _e("u8", 0, tile)), (12, 1000, False, _e("u16", 16, tile))):
            out.append(Case(7, "enc", m, k, c, f, (3001,), enc_impl=impl))   # 7: offset and halo
        for m, k, c, f in ((16, 256, True, _r(2, 0, tile)), (12, 256, True, _e("u8", 16, tile)),
                           (24, 256, True, _e("u8", 0, tile)), (8, 4096, False, _e("u16", 8, tile)),
                           (12, 4096, False, _e("u16", 16, tile))):
            out.append(Case(8, "enc", m, k, c, f, (3000,), chunk_vectors=(33,), enc_impl=impl))
        out += [Case(9, "enc", 45, 256, False, _e("u8", 0, tile), (600,), enc_impl=impl),
                Case(9, "enc", 46, 256, False, UNSUPPORTED, (600,), enc_impl=impl)]
    return out


DEC_N = 4101


def _dec_cases():
    out = []
    for m in (8, 16):
        for c in (True, False):
            l1 = "true" if (not c and m == 8) else "false"   # 8 plain tables of 2^11 fit 48 KB
            chunks = f"dec_chunks<{m},u8,{l1}>"
            out += [Case(10, "dec", m, 256, c, chunks, (DEC_N,), chunk_vectors=(33, 64)),
                    Case(10, "dec", m, 256, c, chunks, (DEC_N,), out_off=4, chunk_vectors=(8,))]
            # (a plain stream's chunk_prev is never read, but its address still picks the form)
            out.append(Case(10, "dec", m, 256, c, chunks, (DEC_N,), prev_off=4, chunk_vectors=(8,)))
            # (the whole-row form beside them: the same streams, aligned)
            out.append(Case(10, "dec", m, 256, c,
                            f"dec_rows<{'true' if c else 'false'},{m // 8},8>", (DEC_N,),
                            chunk_vectors=(8,)))
    for k in (1000, 4096):
        out += [Case(10, "dec", 8, k, False, "dec_rows<false,2,16>", (DEC_N,), chunk_vectors=(16,)),
                Case(10, "dec", 8, k, False, "dec_chunks<0,u16,false>", (DEC_N,), chunk_vectors=(40,))]
    out += [Case(10, "dec", 12, 1000, False, "dec_chunks<0,u16,false>", (DEC_N,), chunk_vectors=(16, 40)),
            Case(10, "dec", 2, 1000, False, "dec_chunks<0,u16,true>", (DEC_N,), chunk_vectors=(16, 40)),
            Case(10, "dec", 5, 200, False, "dec_chunks<0,u8,true>", (DEC_N,), chunk_vectors=(16, 40)),
            Case(10, "dec", 12, 256, True, "dec_chunks<0,u8,false>", (DEC_N,), chunk_vectors=(16, 40)),
            # S halving (1000 -> 16 rows a batch); 8192 >= n: one chunk for all the rows
            Case(10, "dec", 16, 256, True, "dec_chunks<16,u8,false>", (DEC_N,),
                 chunk_vectors=(1000, 4096, 8192)),
            Case(10, "dec", 17, 256, False, UNSUPPORTED, (DEC_N,), chunk_vectors=(64,))]
    return out


CASES = _hist_cases() + _enc_cases() + _dec_cases()


def cases(item: int, **match) -> list:
    return [c for c in CASES if c.item == item and all(getattr(c, a) == v for a, v in match.items())]


def case_form(c: Case, **actual) -> str:
    """the mirrored dispatch for case c: `actual` overrides the case's alignment fields with
    what a test's tensors really have (data_ptr() % 16 and so on)"""
    codes_mod = actual.get("codes_mod16", c.codes_off)
    prev_mod = actual.get("prev_mod8", c.prev_off) % 8
    out_mod = actual.get("out_mod8", c.out_off) % 8
    ldc = 1 if c.pad >= 0 else 0
    if c.kind == "hist":
        return hist_form(c.m, c.k, c.context, 1 if c.k <= 256 else 2, codes_mod % 16, ldc,
                         c.hist_block, c.hist_split, c.impl_env)
    if c.kind == "enc":
        return enc_form(c.m, c.k, codes_mod % 8, prev_mod, ldc, False, c.enc_impl)
    cv = actual.get("chunk_vectors", c.chunk_vectors[0])
    return dec_form(c.m, c.k, c.context, cv, prev_mod, out_mod)
