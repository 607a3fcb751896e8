"""The exact-row kernels (pqh_flat.hip, pqh_flat_lists.hip, pqh_rows16.hip, pqh_sq.hip,
pqh_rerank.hip) in the instantiations, branches and layouts that test_gpu_flat.py,
test_gpu_flat_lists.py, test_gpu_rows16.py, test_gpu_sq.py and test_gpu_rerank.py never launch.
The cases and their numpy worlds are in tests/exact_forms_cases.py, the expected values come from
the definitions (flat_ref, flat_lists_ref, sq_ref, rerank_ref); ids are compared by array_equal
and dist by array_equal of its bits.  No tolerance, no case skipped or filtered.  NaN (255 for
codes) lies between the rows, behind d and in front of a shifted base, also behind d of strided
queries.  tests/test_exact_forms_cpu.py checks without a GPU that every case has the property it
is named for.

What launches what (test ids are test_flat[<case>-<rows>-<metric>], test_lists[<case>-<store>-
<metric>], test_rerank[<case>-<store>-<metric>]; <rows> is f32, f16, bf16 unless stated):

  gap  kernel form or branch                               cases
  ---  --------------------------------------------------  -----------------------------------------
  1    flat_screen<*, kWideKR, PAN, *>: wide list, two     test_flat[wide_panels_k129-*],
       panels (d = 136, the last one short), 33 queries    [wide_panels_k256-f32-*]; with a mask
       = one full and one almost dead query wave           [mask_wide_panel-*], [none_wide_panel-*]
  1    flat_valu<*, kWideKR, *>: wide list, d > 1024       test_flat[wide_valu_k65-*],
                                                           [wide_valu_k256-*]
  2    all_rows inside flat_screen with keep               test_flat[fb_reg_mask-*],
                                                           [fb_wide_panel_mask-*]
  2    all_rows and list_to_lds<kWideKR>                   test_flat[fb_wide_reg-*],
                                                           [fb_wide_panel_mask-*], [inf_row_wide-*]
  2    all_rows in the panel form                          test_flat[fb_panel-*],
                                                           [fb_wide_panel_mask-*], [inf_row_panel-*]
  2    every query through Cmax, the row masked out        test_flat[inf_row_wide-*],
                                                           [inf_row_panel-*]
  3    keep in the panel form (word read at pn == NP - 1)  test_flat[mask_panel-*],
                                                           [mask_wide_panel-*], [none_wide_panel-*]
  3    keep with the wide list, register form              test_flat[mask_wide_reg-*]
  3    keep in flat_valu, narrow and wide                  test_flat[mask_valu_k5-*],
                                                           [mask_valu_k65-*], [none_valu-*]
  4    load8 / load8_packed element loads at d % 16 == 0,  test_flat[elem_d32_stride1-*],
       no zero-filled tail, vec_chain == 0 (d = 144: the   [elem_d32_shift-*], [elem_d144_stride1-*],
       panel form)                                         [elem_d144_shift-*]
  4    vec_x != vec_q                                      test_flat[elem_d32_q_stride1-*],
                                                           [elem_d144_q_stride1-*],
                                                           [qstride_reg_pad3-*]
  5    workspace [slab][nq][k] with both grid dimensions   test_flat[groups_x_slabs_k5-*] (2 x 3),
       above 1                                             [groups_x_slabs_k70-*] (5 x 3)
  6    ld_q != d: qr, qp[u] of the drain                   test_flat[qstride_reg_pad3/4-*],
                                                           [qstride_panel_pad3/4-*]
  6    ld_q != d: flat_valu, all_rows                      test_flat[qstride_valu_pad3/4-*],
                                                           [qstride_fallback_pad3/4-*]
  6    ld_q != d: qrow[e] of flat_lists, rows16_lists,     test_lists[qstride_pad3-*],
       sq_lists, in a second unit too (17 pairs)           [qstride_pad4-*]
  6    ld_q != d: qrow of rerank_rows<*, *, WIDE>          test_rerank[qstride_narrow_pad3/4-*],
                                                           [qstride_wide_pad3/4-*]
  7    flat_lists vec fetch/stash at chunks c >= 1, with   test_lists[vec_d36-f32-*], [vec_d64-f32-*],
       a ragged last chunk (d % 32 != 0), d = 128          [vec_d100-f32-*], [vec_d128-f32-*],
                                                           [vec_d132-f32-*], [vec_d64_gap-f32-*],
                                                           [vec_d100_groups3-f32-*]
  7    flat_lists element loads at d % 4 == 0 (base off    test_lists[vec_d64_shift-f32-*]
       16 bytes, ld_x % 4 == 0)
  7    rows16_lists whole 16-byte pieces in chunk 1        test_lists[vec_d40-f16/bf16-*],
                                                           [vec_d64-f16/bf16-*], [vec_d72-f16/bf16-*]
  8    u_cnt = 1 .. 16: ng = 1, 2, 3, 4 of rows16_lists,   test_lists[pairs_sweep-*]
       every 4 * g4 >= u_cnt of flat_lists and sq_lists
  8    wide units of 1 .. 4 pairs, several units a list    test_lists[pairs_sweep_wide-*]
  9    k = 65, 128, 129, 256: Flat over three slabs and    test_flat[k_edges_k*-f32/bf16-*],
       the merge of wide partial lists; flat_valu          [wide_valu_k65-*], [wide_valu_k256-*],
                                                           [wide_panels_k256-f32-*]
  9    k = 65, 128, 129, 256 in the three list scans       test_lists[k_edges_k*-*]
  -    300 lists (empty ones among them), 512 pairs: the   test_lists[many_units-f32/sq8-*]
       grid bound above the real unit count
  -    groups that start and that end on a dead tile       test_lists[masked_groups-*]
  -    out= as column slices at ncand = 200, k = 129       test_rerank[out_stride_wide-*]

Flat.counts()[1] is asserted in every Flat case: 0 where the screen must hold, the stated number of
non-finite queries, and nq for flat_valu and for a non-finite row.  A non-finite query's own result
is not fixed by include/pqh.h beyond the range of its ids; only that range (and the mask) is
asserted for it.  NaN or -inf distances in the list scans are left out for the same reason: no
list-scan case here holds a non-finite value."""
import numpy as np
import pytest

import exact_forms_cases as cases
from exact_forms_cases import DTYPE, FLAT, LISTS, METRICS, RERANK

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    from pq_huffman_amd import codec
    assert torch.cuda.is_available()
    return torch, codec, codec.Context(0), codec.Context(0).set_search_max_k(256)


def _dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()


def _rows(torch, a, store, ld, shift=0):
    """a as a device tensor (n, ld) of the store's type, rows ld elements apart from element
    `shift` of its buffer on, NaN (255 for codes) everywhere else"""
    n, d = a.shape
    fill = 255 if store == "sq8" else float("nan")
    flat = torch.full((n * ld + shift,), fill, dtype=getattr(torch, DTYPE[store]), device="cuda")
    buf = flat[shift:].view(n, ld)
    buf[:, :d] = _dev(torch, a).to(buf.dtype)
    if store != "sq8":   # the conversion was exact
        assert np.array_equal(buf[:, :d].float().cpu().numpy().view(np.uint32), a.view(np.uint32))
    return buf


def _queries(torch, q, pad):
    """q as the first d columns of a (nq, d + pad) tensor, NaN behind them"""
    nq, d = q.shape
    wide = torch.full((nq, d + pad), float("nan"), device="cuda")
    wide[:, :d] = _dev(torch, q)
    return wide[:, :d]


def _equal(got, want):
    got = [t.cpu().numpy() if hasattr(t, "cpu") else t for t in got[:2]]
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("case,rows", cases.flat_ids())
def test_flat(gpu, case, rows, metric):
    torch, codec, ctx, wide = gpu
    c, w = FLAT[case], cases.flat_world(case, rows)
    n, d, nq, k = c["n"], c["d"], c["nq"], c["k"]
    layout = c.get("x_layout", "plain")
    buf = _rows(torch, w["x"], rows, d + 1 if layout == "stride1" else d, 1 if layout == "shift" else 0)
    keep, base = w["keep"], w["id_base"]
    flat = codec.Flat(wide if k > 64 else ctx, buf, d=d)
    try:
        dist, ids = flat.search(_queries(torch, w["q_sent"], c.get("q_pad", 0)), k, metric=metric,
                                keep=None if keep is None else _dev(torch, keep), id_base=base)
        counts = flat.counts()
    finally:
        flat.close()
    dist, ids = dist.cpu().numpy(), ids.cpu().numpy()
    print(case, rows, metric, "chains", counts[0], "fallback", counts[1])
    assert counts[1] == (nq if c["fallback"] == "nq" else c["fallback"])
    m = w["compared"]
    want = cases.flat_want(case, rows, metric)
    _equal((dist[m], ids[m]), (want[0][m], want[1][m]))
    rest = ids[~m]   # the non-finite queries: -1 or a row that takes part
    assert ((rest == -1) | ((rest >= base) & (rest < base + n))).all()
    if keep is not None:
        assert keep[rest[rest >= 0] - base].all()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("case,store", cases.list_ids())
def test_lists(gpu, case, store, metric):
    torch, codec, ctx, wide = gpu
    lengths, d, ld, nq, nprobe, k, opt = LISTS[case]
    w = cases.list_world(case, store)
    c = wide if k > 64 else ctx
    rows = _rows(torch, w["own"], store, ld, opt.get("shift", 0))
    q = _queries(torch, w["q"], opt.get("q_pad", 0))
    kw = dict(metric=metric, id_base=w["id_base"],
              keep=None if w["keep"] is None else _dev(torch, w["keep"]))
    offsets, probes = _dev(torch, w["offsets"]), _dev(torch, w["probes"])
    c.set_tuning(search_groups=opt.get("groups", 0))
    try:
        if store == "sq8":
            sq = codec.SQ(c, *(_dev(torch, v) for v in w["sq"]))
            got = codec.sq_search_lists(c, sq, rows, offsets, probes, q, k, **kw)
        else:
            got = codec.flat_search_lists(c, rows, offsets, probes, q, k, d=d, **kw)
        codec.ivf_status(c)
    finally:
        c.set_tuning(search_groups=0)
    _equal(got, cases.list_want(case, store, metric))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("store", cases.STORES)
@pytest.mark.parametrize("case", sorted(RERANK))
def test_rerank(gpu, case, store, metric):
    torch, codec, ctx, wide = gpu
    ncand, k, d, nq, opt = RERANK[case]
    w = cases.rerank_world(case, store)
    c = wide if ncand > 64 else ctx
    rows = _rows(torch, w["own"], store, (d + 3) // 4 * 4 + 4)
    st = rows if w["sq"] is None else (codec.SQ(c, *(_dev(torch, v) for v in w["sq"])), rows)
    out, bufs = None, None
    if "out_pad" in opt:
        bufs = (torch.full((nq, k + opt["out_pad"]), float("nan"), device="cuda"),
                torch.full((nq, k + opt["out_pad"]), -7, dtype=torch.int64, device="cuda"))
        out = tuple(t[:, :k] for t in bufs)
    got = codec.rerank(c, st, _queries(torch, w["q"], opt.get("q_pad", 0)), _dev(torch, w["cand"]), k,
                       metric=metric, d=d, out=out)
    codec.ivf_status(c)
    _equal(got, cases.rerank_want(case, store, metric))
    if bufs:   # what lies behind the k columns is left alone
        assert torch.isnan(bufs[0][:, k:]).all() and (bufs[1][:, k:] == -7).all()
