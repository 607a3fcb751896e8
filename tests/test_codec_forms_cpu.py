"""CPU pins for tests/codec_forms_ref.py: the numpy histogram against the oracle and against a
plain loop, the oracle's encode/decode round trip on every encode shape the GPU tests use, the
mirrored dispatch at the values the issue's analysis states, the coverage of every returnable
form name by CASES, and the partial-layout claim the cross-context reduce relies on."""
import numpy as np
import pytest

import codec_forms_ref as ref


@pytest.mark.parametrize("m,k,ctxm", [(3, 256, True), (8, 256, True), (8, 256, False),
                                      (2, 300, True), (8, 1000, False), (5, 4096, False),
                                      (4, 6, True), (4, 255, True)])
def test_hist_equals_oracle_on_in_alphabet_codes(oracle, m, k, ctxm):
    n = 3001
    codes = ref.codes_for(n, m, k, seed=5 + m + k)
    assert codes.dtype == (np.uint8 if k <= 256 else np.uint16) and int(codes.max()) < k
    assert np.array_equal(ref.hist(codes, k, ctxm), oracle.histogram(codes, k, ctxm))
    if ctxm:   # rows [s, n) with the halo row s - 1: the whole run's pairs from row s - 1 on
        for s in (1, 3, 64):
            want = oracle.histogram(codes[s - 1:], k, True)
            want -= oracle.histogram(codes[s - 1:s], k, True)   # (a single row: no pair)
            assert np.array_equal(ref.hist(codes[s:], k, True, prev_row=codes[s - 1]), want), s
        whole = ref.hist(codes[:1000], k, True) + ref.hist(codes[1000:], k, True, codes[999])
        assert np.array_equal(whole, ref.hist(codes, k, True))
    if codes.dtype == np.uint16:   # the int16 view torch tensors carry
        assert np.array_equal(ref.hist(codes.view(np.int16), k, ctxm), ref.hist(codes, k, ctxm))


@pytest.mark.parametrize("k", [2, 6, 255, 300])
def test_hist_drops_out_of_alphabet_pairs(k):
    m, n = 3, 400
    codes = ref.codes_for(n, m, k, seed=k, bad=0.2)
    assert (codes >= k).any() and (codes < k).any()
    halo = codes[7]
    plain = np.zeros((m, k), np.int64)
    pairs = np.zeros((m, k * k), np.int64)
    for v in range(n):
        for i in range(m):
            prev, cur = int(codes[v - 1, i] if v else halo[i]), int(codes[v, i])
            if cur < k:
                plain[i, cur] += 1
                if prev < k:
                    pairs[i, prev * k + cur] += 1
    assert np.array_equal(ref.hist(codes, k, False), plain)
    assert np.array_equal(ref.hist(codes, k, True, prev_row=halo), pairs)
    first = np.zeros_like(pairs)   # without the halo row 0 has no pair
    for i in range(m):
        p, c = int(halo[i]), int(codes[0, i])
        if p < k and c < k:
            first[i, p * k + c] = 1
    assert np.array_equal(ref.hist(codes, k, True), pairs - first)


def _enc_shapes():
    shapes = {(c.m, c.k, c.context) for c in ref.CASES if c.kind == "enc" and c.form != ref.UNSUPPORTED}
    shapes |= {(m, k, False) for m in (5, 20, 24) for k in (257, 300, 1000)} | {(24, 256, True)}
    return sorted(shapes)


@pytest.mark.parametrize("m,k,ctxm", _enc_shapes())
def test_oracle_round_trips_every_encode_shape(oracle, m, k, ctxm):
    """The oracle's stream is the expected value of the encoder tests; where pqh_decode refuses
    the shape (m > 16) its decode is also the only check of the GPU's bytes."""
    n = 513
    codes = ref.codes_for(n, m, k, seed=m * 7 + k)
    ocb = oracle.build_codebooks(codes, k, ctxm)
    stream, bits = oracle.encode(codes, ocb)
    assert np.array_equal(oracle.decode(stream, n, m, ocb), codes)
    # the chunk offsets the GPU tests expect: the cumulative row bits of the codebooks' lengths
    rb = ref.row_bits(codes, ocb.lens, k, ctxm)
    assert int(rb.sum()) == bits
    for cut in (1, 7, 300):   # ... which are the lengths of the oracle's prefix streams
        assert oracle.encode(codes[:cut], ocb)[1] == int(rb[:cut].sum())
        assert ref.chunk_offsets(rb, cut)[1] == int(rb[:cut].sum())
    if ctxm:   # a shard's first row in the context of its halo row
        assert int(ref.row_bits(codes[100:], ocb.lens, k, True, codes[99]).sum()) == int(rb[100:].sum())


@pytest.mark.parametrize("deep", [False, True])
@pytest.mark.parametrize("m,k,ctxm", [(16, 256, True), (12, 256, True), (24, 256, True),
                                      (8, 4096, False), (12, 4096, False)])
def test_oracle_round_trips_long_codes(oracle, m, k, ctxm, deep):
    """The two count families of the long-code test: the first passes the 12 bits of the u16
    gather copy (its longest code has 21 bits), the deep one the 26 bits of the u32 copy."""
    counts = ref.long_code_counts(m, k, ctxm, deep)
    assert counts.max() < 2 ** 31 and counts.min() >= 1
    ocb = ref.oracle_codebooks(oracle, counts, k, ctxm)
    lens = ocb.lens
    assert lens.min() >= 1 and 12 < lens.max() <= ref.MAX_CODE_LEN
    assert (lens.max() > 26) == deep
    codes = ref.long_code_rows(300, m, k)
    stream, bits = oracle.encode(codes, ocb)
    assert bits == int(ref.row_bits(codes, lens, k, ctxm).sum())
    assert np.array_equal(oracle.decode(stream, 300, m, ocb), codes)


# every name the three mirrors can return; a form added to the dispatch (and to its mirror) fails
# test_every_form_has_a_case until CASES reaches it
HIST_FORMS = ["hist_ctx_w<1024,5,false>", "hist_ctx_w<1024,5,true>", "hist_ctx_w<256,3,false>",
              "hist_ctx_w<256,3,true>", "hist_ctx<u8,1024,20>", "hist_ctx<u8,256,8>",
              "hist_plain_rows16", "hist_plain<u8>", "hist_plain<u16>"]
ENC_FORMS = [f"enc_onepass<{body},tile={tile}>" for tile in (0, 1) for body in (
    "u8,8,256,row8,cs=1,pm=0", "u8,8,256,row8,cs=2,pm=0", "u8,8,256,row8,cs=1,pm=1",
    "u8,8,256,row8,cs=2,pm=1", "u8,8,256,generic,cs=1,pm=0", "u8,16,512,generic,cs=1,pm=0",
    "u8,0,512,generic,cs=1,pm=0", "u16,8,256,generic,cs=1,pm=0", "u16,16,512,generic,cs=1,pm=0",
    "u16,0,512,generic,cs=1,pm=0")] + [ref.UNSUPPORTED]
DEC_FORMS = ["dec_rows<true,1,8>", "dec_rows<true,2,8>", "dec_rows<false,1,8>",
             "dec_rows<false,2,8>", "dec_rows<false,2,16>", "dec_chunks<8,u8,true>",
             "dec_chunks<8,u8,false>", "dec_chunks<16,u8,false>", "dec_chunks<0,u8,true>",
             "dec_chunks<0,u8,false>", "dec_chunks<0,u16,true>", "dec_chunks<0,u16,false>",
             ref.UNSUPPORTED]


def _returnable():
    """the names the mirrors return over a sweep of their whole argument space"""
    h, e, d = set(), set(), set()
    ks = (2, 6, 16, 100, 255, 256, 257, 258, 300, 1000, 4095, 4096)
    for m in range(1, 49):
        for k in ks:
            for ctxm in (True, False):
                if ctxm and k > 256:
                    continue
                for a in (0, 2, 4, 8):
                    for ldc in (0, 1):
                        for blk in (0, 256, 1024):
                            for env in ("", "thread", "wave"):
                                h.add(ref.hist_form(m, k, ctxm, 1 if k <= 256 else 2, a, ldc, blk, 0, env))
                    for pm8 in (0, 4):
                        for cv in (1, 8, 32, 33, 1000, 4096):
                            d.add(ref.dec_form(m, k, ctxm, cv, pm8, a % 8))
            for a in (0, 4):
                for p in (0, 4):
                    for ldc in (0, 1):
                        for tree in (False, True):
                            for impl in (0, 1, 2):
                                e.add(ref.enc_form(m, k, a, p, ldc, tree, impl))
    return h, e, d


def test_every_form_has_a_case():
    h, e, d = _returnable()
    assert h == set(HIST_FORMS) and e == set(ENC_FORMS) and d == set(DEC_FORMS)
    for kind, names in (("hist", HIST_FORMS), ("enc", ENC_FORMS), ("dec", DEC_FORMS)):
        have = {c.form for c in ref.CASES if c.kind == kind}
        assert have == set(names), (kind, set(names) ^ have)


def test_cases_state_the_form_their_fields_give():
    """a case's written-out form is what the mirror gives for its own fields (the GPU tests ask
    the same of the tensors they really pass)"""
    for c in ref.CASES:
        for cv in c.chunk_vectors or (0,):
            assert ref.case_form(c, chunk_vectors=cv) == c.form, (c, cv)


def test_dispatch_values_stated_in_the_analysis():
    assert [ref.hist_split(k, 8) for k in (2, 6, 100, 255, 16, 256)] == [1, 1, 2, 1, 8, 8]
    assert [ref.hist_split(16, s) for s in ref.HIST_SPLITS] == [2, 1, 2, 4, 8]
    assert [ref.hist_split(100, s) for s in ref.HIST_SPLITS] == [2, 1, 2, 2, 2]
    assert [ref.hist_split(255, s) for s in ref.HIST_SPLITS] == [1] * 5   # odd k: always 1
    # two full chunks and a partial one; m = 16 starts its rounds above 32 chunks
    p = ref.hist_plan(ref.N_THREE_CHUNKS, 8, 256)
    assert (p["chunks"], p["rounds"], p["groups"]) == (3, 1, 3)
    assert ref.hist_plan(32 * ref.HIST_CHUNK, 16, 256)["rounds"] == 1
    p = ref.hist_plan(ref.N_ROUNDS, 16, 256, 4)
    assert (p["chunks"], p["rounds"], p["groups"], p["split"]) == (34, 5, 7, 4)
    assert p["total_bytes"] == p["acc_offset"] + 16 * 65536 * 4
    assert ref.hist_plan(64 * ref.HIST_CHUNK, 8, 256)["rounds"] == 1       # m = 8: gt = 16
    assert ref.hist_plan(5, 4, 255)["words"] == (255 * 255 + 1) // 2      # a half-used last word
    assert ref.rows16_plan(ref.N_ROWS16_CAP) == dict(rows=16384, groups=65)
    assert ref.rows16_plan(63) == dict(rows=1, groups=63) and ref.rows16_plan(65)["rows"] == 2
    # the encoder's LDS limit: m = 45 fits with 161,296 bytes, m = 46 does not
    assert ref.enc_lds_bytes(45, 256, False) == 161_296 <= ref.LDS_LIMIT
    assert ref.enc_lds_bytes(46, 256, False) > ref.LDS_LIMIT
    assert ref.enc_form(46, 256) == ref.UNSUPPORTED != ref.enc_form(45, 256)
    # the decoder's staging: 1000 rows of 16 bytes a chunk are staged 16 at a time
    assert ref.dec_stage_rows(16, 256, 1000) == 16 and ref.dec_stage_rows(16, 256, 4096) == 16
    assert ref.dec_stage_rows(8, 256, 32) == 32 and ref.dec_stage_rows(8, 4096, 40) == 10


@pytest.mark.parametrize("n,m,k", [(ref.N_THREE_CHUNKS, 8, 256), (ref.N_THREE_CHUNKS, 6, 256),
                                   (ref.N_ROUNDS, 16, 256), (70_001, 4, 16), (5, 6, 255)])
def test_partial_layout_does_not_depend_on_the_split(n, m, k):
    """hist_plan's claim: groups, words and the byte layout depend only on n, m and k, so
    partials written with one split may be reduced on a context with another -- and the
    library's histogram_partial_bytes (which takes no split) is that layout's size."""
    from pq_huffman_amd.capi import lib
    plans = [ref.hist_plan(n, m, k, s) for s in ref.HIST_SPLITS]
    for key in ("chunks", "rounds", "groups", "words", "partial_bytes", "acc_offset", "total_bytes"):
        assert len({p[key] for p in plans}) == 1, key
    if k % 16 == 0:
        assert len({p["split"] for p in plans}) == 4
    assert lib().pqh_histogram_partial_bytes(n, m, k) == plans[0]["total_bytes"]
