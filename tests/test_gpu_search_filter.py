"""Filtered search: the row mask of every ADC scan (the *_masked calls behind keep=),
codec.pack_mask, IVF.search(keep=...) and IVF.remove.  Expected values come from numpy
(tests/search_filter_ref.py: ivf_residual_ref.adc, np.lexsort((rows, dist)) over the kept rows,
np.packbits(..., bitorder="little")), never from the calls under test.  Every comparison is
array_equal on the ids and on the raw float bits."""
import numpy as np
import pytest

import search_filter_ref as fref
import search_lists_ref as lref
import search_shapes_ref as sref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    from pq_huffman_amd import codec
    assert torch.cuda.is_available()
    return torch, codec, codec.Context(0)


@pytest.fixture(scope="module")
def coded(gpu):
    """mode -> (host codes, device codes, tables, lut, its distances), built once"""
    torch, codec, ctx = gpu
    made = {}

    def get(mode):
        if mode not in made:
            m, k, ctxm = fref.MODES[mode]
            codes = fref.codes_of(mode)
            cd = torch.from_numpy(codes).cuda()
            counts = codec.histogram(ctx, cd, k, ctxm)
            cbs = codec.Codebooks(codec.counts_to_host(counts), k, ctxm)
            lut = fref.lut_of(fref.NQ, m, 7)
            made[mode] = (codes, cd, codec.Tables.from_codebooks(ctx, cbs), lut,
                          sref.dists(lut, codes))
        return made[mode]
    return get


def _bits(a):
    return a.view(np.uint32)


def _check(got, want, what=""):
    gd, gi = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert gd.dtype == np.float32 and gi.dtype == np.int64
    assert np.array_equal(gi, want[1]), what
    assert np.array_equal(_bits(gd), _bits(want[0])), what


def _same(a, b, what=""):
    assert np.array_equal(a[1].cpu().numpy(), b[1].cpu().numpy()), what
    assert np.array_equal(_bits(a[0].cpu().numpy()), _bits(b[0].cpu().numpy())), what


def _status(fn):
    from pq_huffman_amd.capi import PqhError
    try:
        fn()
    except PqhError as err:
        return err.status
    return 0


def _words(torch, keep, stale=False):
    return torch.from_numpy(fref.pack(keep, stale)).cuda()


@pytest.mark.parametrize("chunk", fref.CHUNKS)
@pytest.mark.parametrize("mode", list(fref.MODES))
def test_plain_search_with_a_mask(gpu, coded, mode, chunk):
    torch, codec, ctx = gpu
    codes, cd, tabs, lut, d = coded(mode)
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=chunk)
    ld = torch.from_numpy(lut).cuda()
    masks = fref.plain_masks(chunk, lut, codes, d)
    fref.check_plain_masks(chunk, lut, codes, masks, d)
    for name, keep in masks.items():
        kd = _words(torch, keep)
        for k in fref.TOP_KS:
            want = fref.want(lut, codes, k, keep, d=d)
            _check(codec.search(ctx, tabs, enc, ld, k, keep=kd), want, (name, k, "stream"))
            _check(codec.search_codes(ctx, cd, ld, k, keep=kd), want, (name, k, "codes"))
    # all ones: the unfiltered call's result, and keep=None's
    ones = _words(torch, masks["ones"])
    for k in fref.TOP_KS:
        free = sref.want(lut, codes, k)
        _check(codec.search(ctx, tabs, enc, ld, k), free, k)
        _check(codec.search(ctx, tabs, enc, ld, k, keep=None), free, k)
        _check(codec.search(ctx, tabs, enc, ld, k, keep=ones), free, k)
        _check(codec.search_codes(ctx, cd, ld, k, keep=None), free, k)
        _check(codec.search_codes(ctx, cd, ld, k, keep=ones), free, k)
    # id_base moves the kept ids and leaves the padding
    want = fref.want(lut, codes, 64, masks["sparse"], id_base=10 ** 12, d=d)
    assert (want[1] == -1).any()
    kd = _words(torch, masks["sparse"])
    _check(codec.search(ctx, tabs, enc, ld, 64, id_base=10 ** 12, keep=kd), want)
    _check(codec.search_codes(ctx, cd, ld, 64, id_base=10 ** 12, keep=kd), want)
    codec.decode_status(ctx)


@pytest.mark.parametrize("chunk", fref.CHUNKS)
def test_ties_among_the_kept_rows_are_decided_by_the_ids(gpu, coded, chunk):
    torch, codec, ctx = gpu
    codes, cd, tabs, _, _ = coded("ctx_m8")
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=chunk)
    lut = fref.ties_lut(fref.NQ, 8, 9)
    keep = fref.random_mask(fref.N, 0.5, 11)
    fref.check_ties(lut, codes, keep)
    ld, kd = torch.from_numpy(lut).cuda(), _words(torch, keep)
    for k in fref.TOP_KS:
        want = fref.want(lut, codes, k, keep)
        _check(codec.search(ctx, tabs, enc, ld, k, keep=kd), want, k)
        _check(codec.search_codes(ctx, cd, ld, k, keep=kd), want, k)
    codec.decode_status(ctx)


@pytest.mark.parametrize("chunk", [4, 64])
def test_stale_bits_past_n_are_ignored(gpu, coded, chunk):
    torch, codec, ctx = gpu
    codes, cd, tabs, lut, d = coded("ctx_m8")
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=chunk)
    ld = torch.from_numpy(lut).cuda()
    for keep in (fref.random_mask(fref.N, 0.5, 11), fref.single(fref.N, fref.N - 1),
                 np.zeros(fref.N, bool)):
        words = fref.pack(keep, stale=True)
        assert words.view(np.uint32)[-1] >> (fref.N & 31) == (1 << (32 - (fref.N & 31))) - 1
        kd = torch.from_numpy(words).cuda()
        want = fref.want(lut, codes, 64, keep, d=d)
        assert want[1].max() < fref.N
        _check(codec.search(ctx, tabs, enc, ld, 64, keep=kd), want)
        _check(codec.search_codes(ctx, cd, ld, 64, keep=kd), want)
    codec.decode_status(ctx)


def test_the_words_need_four_byte_alignment_only(gpu, coded):
    """a slice from an odd int32 index of a larger buffer, whatever lies around it"""
    torch, codec, ctx = gpu
    codes, cd, tabs, lut, d = coded("noctx_m8")
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=7)
    ld = torch.from_numpy(lut).cuda()
    keep = fref.random_mask(fref.N, 0.5, 11)
    want = fref.want(lut, codes, 64, keep, d=d)
    got = []
    for fill in (0xFFFFFFFF, 0):
        buf, at = fref.embedded(fref.pack(keep), fill)
        bd = torch.from_numpy(buf).cuda()
        kd = bd[at]
        assert kd.data_ptr() % 8 == 4 and kd.is_contiguous()
        got.append((codec.search(ctx, tabs, enc, ld, 64, keep=kd),
                    codec.search_codes(ctx, cd, ld, 64, keep=kd)))
        _check(got[-1][0], want, fill)
        _check(got[-1][1], want, fill)
        assert np.array_equal(bd.cpu().numpy(), buf)          # the words are only read
    _same(got[0][0], got[1][0])
    _same(got[0][1], got[1][1])
    codec.decode_status(ctx)


def test_a_bad_keep_tensor_is_refused(gpu, coded):
    torch, codec, ctx = gpu
    codes, cd, tabs, lut, d = coded("noctx_m8")
    ld = torch.from_numpy(lut).cuda()
    short = torch.zeros((fref.N + 31) // 32 - 1, dtype=torch.int32, device="cuda")
    assert _status(lambda: codec.search_codes(ctx, cd, ld, 4, keep=short)) == -1
    assert _status(lambda: codec.search_codes(ctx, cd, ld, 4, keep=short.to(torch.int64))) == -1


@pytest.mark.parametrize("m,K", fref.PROBE_SHAPES)
@pytest.mark.parametrize("chunk", fref.PROBE_CHUNKS)
@pytest.mark.parametrize("context", [True, False])
def test_probe_forms_with_a_mask(gpu, context, chunk, m, K):
    torch, codec, ctx = gpu
    case = sref.sweep_case(m, K, chunk, seed=40 + m + chunk)
    codes, offsets, probes, lut_q, lut_pair = case
    masks = fref.probe_masks(case)
    fref.check_probe_masks(chunk, case, masks)
    cd = torch.from_numpy(codes).cuda()
    counts = codec.histogram(ctx, cd, K, context)
    tabs = codec.Tables.from_codebooks(ctx, codec.Codebooks(codec.counts_to_host(counts), K, context))
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=chunk)
    ptr, ranges = lref.probe_ranges(offsets, probes)
    pd, rd = torch.from_numpy(ptr).cuda(), torch.from_numpy(ranges).cuda()
    od, bd = torch.from_numpy(offsets).cuda(), torch.from_numpy(probes).cuda()
    lq, lp = torch.from_numpy(lut_q).cuda(), torch.from_numpy(lut_pair).cuda()
    for name, keep in masks.items():
        kd = _words(torch, keep)
        for k in (10, 64):
            per_query, per_pair = fref.probe_want(case, keep, k)
            what = (name, k)
            # a table per query: the range form ("query") and the list form ("list")
            _check(codec.search_ranges(ctx, tabs, enc, lq, pd, rd, k, keep=kd), per_query, what)
            _check(codec.search_codes_ranges(ctx, cd, lq, pd, rd, k, keep=kd), per_query, what)
            _check(codec.search_lists(ctx, tabs, enc, lq, od, bd, k, keep=kd), per_query, what)
            _check(codec.search_codes_lists(ctx, cd, lq, od, bd, k, keep=kd), per_query, what)
            # a table per pair
            _check(codec.search_range_tables(ctx, tabs, enc, lp, pd, rd, k, keep=kd), per_pair, what)
            _check(codec.search_codes_range_tables(ctx, cd, lp, pd, rd, k, keep=kd), per_pair, what)
            _check(codec.search_lists(ctx, tabs, enc, lp, od, bd, k, keep=kd), per_pair, what)
            _check(codec.search_codes_lists(ctx, cd, lp, od, bd, k, keep=kd), per_pair, what)
    codec.decode_status(ctx)


def test_a_corrupt_chunk_is_reported_only_if_it_is_walked(gpu, coded):
    """error bit 1 is for the chunks that were walked: with the damaged chunk's rows masked
    out the search is clean and exact, with one of them kept it is PQH_ERR_CORRUPT"""
    torch, codec, ctx = gpu
    codes, cd, tabs, lut, d = coded("ctx_m8")
    enc = codec.encode(ctx, tabs, cd, chunk_vectors=4)
    ld = torch.from_numpy(lut).cuda()
    j = 100                                               # the chunk of rows 400 ... 403
    offs = enc.chunk_offsets.clone()
    offs[j] = enc.stream.numel() * 8 + 64                 # a start past the stream
    enc.chunk_offsets = offs
    keep = np.ones(fref.N, bool)
    keep[4 * j:4 * j + 4] = False
    _check(codec.search(ctx, tabs, enc, ld, 64, keep=_words(torch, keep)),
           fref.want(lut, codes, 64, keep, d=d))
    codec.decode_status(ctx)
    keep[4 * j + 1] = True
    codec.search(ctx, tabs, enc, ld, 64, keep=_words(torch, keep))
    assert _status(lambda: codec.decode_status(ctx)) == -6


@pytest.mark.parametrize("permuted", [False, True])
@pytest.mark.parametrize("n", fref.PACK_NS)
def test_pack_mask(gpu, n, permuted):
    torch, codec, ctx = gpu
    keep, perm, words = fref.pack_case(n, n + 1, permuted)
    kd = torch.from_numpy(keep).cuda()
    pd = torch.from_numpy(perm).cuda() if permuted else None
    got = codec.pack_mask(ctx, kd, pd)
    assert got.dtype == torch.int32 and got.shape == ((n + 31) // 32,)
    assert np.array_equal(got.cpu().numpy(), words)
    # bool flags, and an output of the caller's that is written up to its last word only
    out = torch.full((len(words) + 2,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    codec.pack_mask(ctx, kd != 0, pd, out=out[1:])
    oh = out.cpu().numpy()
    assert np.array_equal(oh[1:1 + len(words)], words)
    assert oh[0] == 0x5A5A5A5A and (oh[1 + len(words):] == 0x5A5A5A5A).all()
    codec.ivf_status(ctx)


def test_pack_mask_reports_a_bad_perm_entry(gpu):
    torch, codec, ctx = gpu
    keep, perm, words = fref.bad_perm_case()
    codec.ivf_status(ctx)
    got = codec.pack_mask(ctx, torch.from_numpy(keep).cuda(), torch.from_numpy(perm).cuda())
    assert _status(lambda: codec.ivf_status(ctx)) == -1
    assert np.array_equal(got.cpu().numpy(), words)
    codec.ivf_status(ctx)                                 # (read once, then clean)


@pytest.fixture(scope="module")
def world(gpu):
    torch, codec, ctx = gpu
    w = fref.ivf_world()
    fref.check_ivf_world(w)
    w.update(xd=torch.from_numpy(w["x"]).cuda(), qd=torch.from_numpy(w["q"]).cuda(),
             pq=codec.PQ(ctx, w["cent"]), coarse=codec.Coarse(ctx, w["cc"]))
    return w


@pytest.mark.parametrize("schedule", ["query", "list"])
@pytest.mark.parametrize("kind", ["plain", "residual"])
def test_ivf_keep_and_remove(gpu, world, kind, schedule):
    torch, codec, ctx = gpu
    w = world
    ivf = codec.IVF.build(ctx, w["pq"], w["coarse"], w["xd"], chunk_vectors=7,
                          residual=kind == "residual")
    codec.ivf_status(ctx)
    assert np.array_equal(ivf.perm.cpu().numpy(), w["perm"])
    assert np.array_equal(codec.decode(ctx, ivf.tables, ivf.enc).cpu().numpy(), w[kind]["codes"])
    nprobe, n = fref.IVF_NPROBE, fref.IVF_N
    keep = torch.from_numpy(w["keep"]).cuda()

    def search(k, keep=None):
        return ivf.search(w["qd"], nprobe, k, schedule=schedule, keep=keep)

    assert ivf.live_count() == n
    for k in (1, 10, 64):
        _check(search(k), fref.ivf_want(w, kind, k), k)
        _check(search(k, keep), fref.ivf_want(w, kind, k, w["keep"]), k)
    if kind == "residual":                                # every slab takes the mask
        ivf.table_budget = 2 * nprobe * fref.IVF_M * 256 * 4
        _check(search(10, keep), fref.ivf_want(w, kind, 10, w["keep"]), "slabs")
        del ivf.table_budget

    # remove the first query's whole unfiltered result
    first = fref.ivf_want(w, kind, 64)[1][0]
    first = first[first >= 0]
    assert len(first) == 64 and len(set(first)) == 64
    before = ivf.fetch(torch.from_numpy(first).cuda()).clone()
    ivf.remove(torch.from_numpy(first).cuda())
    for again in range(2):                                # the second time changes nothing
        assert ivf.live_count() == n - 64
        for k in (10, 64):
            got = search(k)
            assert not np.isin(got[1].cpu().numpy(), first).any()
            _check(got, fref.ivf_want(w, kind, k, removed=first), k)
            _check(search(k, keep), fref.ivf_want(w, kind, k, w["keep"], removed=first), k)
        ivf.remove(torch.from_numpy(first[:7]).cuda())
    assert torch.equal(ivf.fetch(torch.from_numpy(first).cuda()), before)   # the stream has them
    codec.decode_status(ctx)
    codec.ivf_status(ctx)
