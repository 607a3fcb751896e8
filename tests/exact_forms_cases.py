"""The case tables of tests/test_gpu_exact_forms.py and their numpy worlds: the inputs, the layouts
they are to be laid out in, and the expected results by the definitions that already exist
(flat_ref, flat_lists_ref, sq_ref, rerank_ref).  Nothing here needs a GPU or calls the library;
tests/test_exact_forms_cpu.py runs every reference and checks that a case has the property it is
named for (the unit sizes of a probe table, a dead tile, the number of non-finite queries)."""
import functools

import numpy as np

import flat_lists_ref
import flat_ref
import rerank_ref
import sq_ref

METRICS = ["l2", "ip"]
ROWS = ["f32", "f16", "bf16"]           # the row types of Flat and flat_search_lists
STORES = ROWS + ["sq8"]                 # the stores of the list scans and of the re-rank
DTYPE = {"f32": "float32", "f16": "float16", "bf16": "bfloat16", "sq8": "uint8"}
ID_BASE = 2 ** 40 - 5
TILE, FLAT_TILE = 256, 32               # rows a list scan's tile, rows a tile of the flat screen
EDGE = [0, 1, 63, 64, 65, 257, 2300]


def exact(x, store):
    """x rounded so that every value is one of the store's row type (torch's .to() is then exact)"""
    if store == "f16":
        return x.astype(np.float16).astype(np.float32)
    if store == "bf16":
        return (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    return x


def _seed(*parts):
    return sum(ord(c) * (i + 1) for i, c in enumerate("/".join(map(str, parts))))


# ------------------------------------------------------------------------------------- Flat
# name: dict(n, d, nq, k) and
#   rows      the row types the case runs over (default: all three)
#   keep      "half": half the rows kept, tile 5 of 32 rows empty; "none": no row kept
#   id_base   default 0; every masked case uses ID_BASE
#   x_layout  "plain" (rows d apart), "stride1" (d + 1 elements apart), "shift" (d apart, the
#             base one element into its buffer)
#   q_pad     the columns of NaN behind d in the query tensor (the queries are wide[:, :d])
#   bad_q     the queries 3, 10 and 17 get a NaN, a +inf and a -inf
#   nan_q     query 3 gets a NaN
#   inf_row   row 40 gets a +inf (the mask keeps it out): Cmax sends every query to all_rows
#   fallback  what Flat.counts()[1] must be: a number, or "nq"
def _flat(n, d, nq, k, **kw):
    return dict(n=n, d=d, nq=nq, k=k, **kw)


FLAT = {
    # 1. wide list with panels, wide list without a screen
    "wide_panels_k129": _flat(700, 136, 33, 129, fallback=0),
    "wide_panels_k256": _flat(700, 136, 33, 256, fallback=0, rows=["f32"]),
    "wide_valu_k65": _flat(300, 1032, 3, 65, fallback="nq"),
    "wide_valu_k256": _flat(300, 1032, 3, 256, fallback="nq"),
    # 9. the wide k edges over three slabs
    **{f"k_edges_k{k}": _flat(2500, 32, 40, k, fallback=0, rows=["f32", "bf16"])
       for k in (65, 128, 129, 256)},
    # 5. query groups times slabs
    "groups_x_slabs_k5": _flat(2100, 20, 130, 5, fallback=0),
    "groups_x_slabs_k70": _flat(2100, 20, 130, 70, fallback=0),
    # 3. masks
    "mask_panel": _flat(700, 136, 33, 10, keep="half", id_base=ID_BASE, fallback=0),
    "mask_wide_reg": _flat(2500, 32, 40, 129, keep="half", id_base=ID_BASE, fallback=0),
    "mask_wide_panel": _flat(700, 136, 33, 129, keep="half", id_base=ID_BASE, fallback=0),
    "mask_valu_k5": _flat(300, 1032, 3, 5, keep="half", id_base=ID_BASE, fallback="nq"),
    "mask_valu_k65": _flat(300, 1032, 3, 65, keep="half", id_base=ID_BASE, fallback="nq"),
    "none_wide_panel": _flat(700, 136, 33, 129, keep="none", id_base=ID_BASE, fallback=0),
    "none_valu": _flat(300, 1032, 3, 65, keep="none", id_base=ID_BASE, fallback="nq"),
    # 2. the all-rows path in every form
    "fb_reg_mask": _flat(2500, 48, 70, 10, keep="half", id_base=ID_BASE, bad_q=True, fallback=3),
    "fb_wide_reg": _flat(2500, 32, 40, 129, id_base=5, bad_q=True, fallback=3),
    "fb_panel": _flat(700, 136, 33, 10, id_base=5, bad_q=True, fallback=3),
    "fb_wide_panel_mask": _flat(700, 136, 33, 129, keep="half", id_base=ID_BASE, bad_q=True,
                                fallback=3),
    "inf_row_wide": _flat(2500, 32, 40, 129, keep="half", id_base=ID_BASE, inf_row=True,
                          fallback="nq"),
    "inf_row_panel": _flat(700, 136, 33, 10, keep="half", id_base=ID_BASE, inf_row=True,
                           fallback="nq"),
    # 4. element loads at d % 16 == 0
    **{f"elem_d{d}_{lay}": _flat(300, d, 33, 10, fallback=0,
                                 **({"q_pad": 1} if lay == "q_stride1" else {"x_layout": lay}))
       for d in (32, 144) for lay in ("stride1", "shift", "q_stride1")},
    # 6. the query stride
    **{f"qstride_{form}_pad{pad}": _flat(*shape, q_pad=pad, **kw)
       for pad in (3, 4)
       for form, shape, kw in (("reg", (2500, 48, 70, 10), dict(fallback=0)),
                               ("panel", (700, 136, 33, 10), dict(fallback=0)),
                               ("valu", (300, 1032, 3, 5), dict(fallback="nq")),
                               ("fallback", (2500, 48, 70, 10), dict(nan_q=True, fallback=1)))},
}
BAD_QUERIES = (3, 10, 17)   # (7 i + 3 of test_gpu_flat.test_non_finite, below every nq here)


def flat_ids():
    return [(name, rows) for name, c in FLAT.items() for rows in c.get("rows", ROWS)]


@functools.lru_cache(maxsize=None)
def flat_world(name, rows):
    """dict(x, q, q_sent, keep, id_base, compared): x float32 (n, d), every value one of the row
    type; q the finite queries the expectation is computed from; q_sent what the search is
    given; compared: the queries whose result the definition fixes (the finite ones)"""
    c = FLAT[name]
    n, d, nq = c["n"], c["d"], c["nq"]
    rng = np.random.default_rng(_seed(name, rows))
    x = exact(rng.standard_normal((n, d)).astype(np.float32), rows)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    keep = None
    if c.get("keep") == "half":
        keep = (rng.random(n) < 0.5) & (np.arange(n) // FLAT_TILE != 5)
    elif c.get("keep") == "none":
        keep = np.zeros(n, bool)
    sent = q.copy()
    if c.get("bad_q"):
        for i, v in zip(BAD_QUERIES, (np.nan, np.inf, -np.inf)):
            sent[i, i % d] = v
    if c.get("nan_q"):
        sent[BAD_QUERIES[0], 1] = np.nan
    if c.get("inf_row"):
        x[40, 1] = np.inf
        keep[40] = False
    for a in (x, q, sent):
        a.setflags(write=False)
    return dict(x=x, q=q, q_sent=sent, keep=keep, id_base=c.get("id_base", 0),
                compared=np.isfinite(sent).all(axis=1))


@functools.lru_cache(maxsize=None)
def flat_want(name, rows, metric):
    w = flat_world(name, rows)   # (topk looks at kept rows only: a masked +inf row is never seen)
    return flat_ref.search(w["q"], w["x"], FLAT[name]["k"], metric, keep=w["keep"],
                           id_base=w["id_base"])


# ------------------------------------------------------------------------------- list scans
# name: (list lengths, d, ld, nq, nprobe, k, options).  ld: the elements between two rows of the
# store (floats, 16-bit elements or codes).  Options:
#   stores   the stores the case runs over (default: all four)
#   shift    the base that many elements into its buffer
#   groups   set_tuning(search_groups=)
#   probes   "longest" (default: every query on the longest list, then distinct others),
#            "sweep" (query i probes the lists i ..), "sample" (nprobe distinct lists a query)
#   keep     "dead_tiles": half the rows, tile 0 and the last tile of list 0 all clear
#   q_pad    the columns of NaN behind d in the query tensor
#   id_base
def _sweep_lengths():
    return [300 if l == 5 else 70 for l in range(16)]


LISTS = {
    # 7. 16-byte loads past one chunk, a ragged last chunk, the element loads at such a d
    **{f"vec_d{d}": ([65, 300, 1], d, d, 4, 2, 10, {"id_base": ID_BASE})
       for d in (36, 64, 100, 128, 132)},
    **{f"vec_d{d}": ([65, 300, 1], d, d, 4, 2, 10, {"stores": ["f16", "bf16"]}) for d in (40, 72)},
    "vec_d64_shift": ([65, 300, 1], 64, 64, 4, 2, 10, {"shift": 1, "stores": ["f32"]}),
    "vec_d64_gap": ([65, 300, 1], 64, 68, 4, 2, 10, {}),
    "vec_d100_groups3": (EDGE, 100, 100, 6, 3, 10, {"groups": 3}),
    # 8. every number of pairs a unit can hold
    "pairs_sweep": (_sweep_lengths(), 33, 36, 16, 16, 10, {"probes": "sweep"}),
    "pairs_sweep_wide": (_sweep_lengths(), 33, 36, 16, 16, 129, {"probes": "sweep"}),
    # 9. the wide k edges
    **{f"k_edges_k{k}": (EDGE, 8, 8, 9, 4, k, {"id_base": 7}) for k in (65, 128, 129, 256)},
    # 6. the query stride, 17 pairs on one list: two units
    "qstride_pad3": ([300, 40], 40, 40, 17, 2, 10, {"q_pad": 3}),
    "qstride_pad4": ([300, 40], 40, 40, 17, 2, 10, {"q_pad": 4}),
    # more units than any other case, empty lists, a grid bound above the unit count
    "many_units": ([l % 41 for l in range(300)], 12, 12, 64, 8, 10,
                   {"probes": "sample", "stores": ["f32", "sq8"]}),
    # groups that start and end on a dead tile
    "masked_groups": ([1200, 300], 40, 40, 7, 2, 64, {"groups": 3, "keep": "dead_tiles"}),
}


def list_ids():
    return [(name, s) for name, c in LISTS.items() for s in c[6].get("stores", STORES)]


def unit_sizes(probes, lengths, qb):
    """the pair counts of the work units the list-major plan makes (lists_plan of
    pqh_search.hip): per list with rows its valid pairs cut into units of qb, the last one short"""
    sizes = []
    for l, rows in enumerate(lengths):
        c = int((probes == l).sum()) if rows else 0
        sizes += [min(qb, c - b) for b in range(0, c, qb)]
    return sizes


@functools.lru_cache(maxsize=None)
def list_world(name, store):
    """dict(x, own, sq, q, offsets, probes, keep, id_base): x the rows as the definition sees
    them (the decoded rows of an sq8 store), own what the store holds (x, or the codes)"""
    lengths, d, ld, nq, nprobe, k, opt = LISTS[name]
    rng = np.random.default_rng(_seed(name, store))
    offsets = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    n, nlist = int(offsets[-1]), len(lengths)
    x = exact(rng.standard_normal((n, d)).astype(np.float32), store)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    sq, own = None, x
    if store == "sq8":
        sq = sq_ref.train(x)
        own = sq_ref.encode(x, *sq)
        x = sq_ref.decode(own, *sq)
    probes = np.full((nq, nprobe), -1, np.int64)
    kind = opt.get("probes", "longest")
    for i in range(nq):
        if kind == "sweep":      # the valid probes in front, -1 behind them
            row = list(range(i, nlist))
        elif kind == "sample":
            row = list(rng.choice(nlist, nprobe, replace=False))
        else:
            longest = int(np.argmax(lengths))
            row = [longest] + list(rng.permutation([l for l in range(nlist) if l != longest]))
        row = row[:nprobe]
        probes[i, :len(row)] = row
    keep = None
    if opt.get("keep") == "dead_tiles":
        keep = rng.random(n) < 0.5
        last = (lengths[0] - 1) // TILE
        keep[:TILE] = False
        keep[last * TILE:lengths[0]] = False
    for a in (x, own, q, probes):
        a.setflags(write=False)
    return dict(x=x, own=own, sq=sq, q=q, offsets=offsets, probes=probes, keep=keep,
                id_base=opt.get("id_base", 0))


@functools.lru_cache(maxsize=None)
def list_want(name, store, metric):
    w = list_world(name, store)
    return flat_lists_ref.search(w["q"], w["x"], w["offsets"], w["probes"], LISTS[name][5], metric,
                                 w["keep"], w["id_base"])


# ---------------------------------------------------------------------------------- re-rank
# name: (ncand, k, d, nq, options): q_pad as above; out_pad: out= given as the first k columns of
# tensors that many columns wider
RERANK_N = 300
RERANK = {
    "qstride_narrow_pad3": (64, 10, 130, 5, {"q_pad": 3}),
    "qstride_narrow_pad4": (64, 10, 130, 5, {"q_pad": 4}),
    "qstride_wide_pad3": (200, 100, 130, 5, {"q_pad": 3}),
    "qstride_wide_pad4": (200, 100, 130, 5, {"q_pad": 4}),
    "out_stride_wide": (200, 129, 130, 5, {"out_pad": 11}),
}


@functools.lru_cache(maxsize=None)
def rerank_world(name, store):
    """dict(own, sq, q, cand): duplicated rows, a query that is a copy of a row, distinct
    candidates per query with -1 in the middle and at the end, and a last query of -1 alone"""
    ncand, k, d, nq, opt = RERANK[name]
    n = RERANK_N
    rng = np.random.default_rng(_seed(name, store))
    x = exact(rng.standard_normal((n, d)).astype(np.float32), store)
    x[n // 2:] = x[:n // 2]
    q = rng.standard_normal((nq, d)).astype(np.float32)
    cand = np.stack([rng.permutation(n)[:ncand] for _ in range(nq)]).astype(np.int64)
    q[0] = x[cand[0, 0]]
    cand[:, ncand // 2] = -1
    cand[::2, -1] = -1
    cand[-1] = -1
    sq = sq_ref.train(x) if store == "sq8" else None
    own = sq_ref.encode(x, *sq) if sq else x
    for a in (own, q, cand):
        a.setflags(write=False)
    return dict(own=own, sq=sq, q=q, cand=cand)


@functools.lru_cache(maxsize=None)
def rerank_want(name, store, metric):
    w = rerank_world(name, store)
    wd, wi, bad = rerank_ref.rerank(w["q"], w["own"], w["cand"], RERANK[name][1], metric, w["sq"])
    assert not bad
    return wd, wi
