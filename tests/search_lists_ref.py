"""The numpy restatement of the list-major probe search (pqh_search_stream_lists,
pqh_search_codes_lists, codec.IVF.search(schedule="list")) and the inputs its tests share, for
tests/test_search_lists_cpu.py and tests/test_gpu_search_lists.py.  Nothing here calls the
library.

The schedule is restated, not the result: the probes are turned round into the pairs of every
list, a list's pairs are cut into batches of QB, every (list, batch) unit scores the list's rows
against the batch's tables and keeps k per pair, and a query's result is the merge of its
pairs' lists by (dist, row).  The arithmetic is ivf_residual_ref.adc's."""
import numpy as np

import datagen
import ivf_residual_ref as ref


def qb_of(m):
    """the pairs of a unit: eight tables of up to 8 parts, four of more"""
    return 8 if m <= 8 else 4


def probe_ranges(offsets, probes):
    """(ptr, ranges) as codec.probe_ranges gives them: range q * nprobe + p is list
    probes[q][p], (0, 0) for -1"""
    nq, nprobe = probes.shape
    flat = probes.reshape(-1)
    ranges = np.zeros((flat.size, 2), np.int64)
    some = flat >= 0
    ranges[some, 0] = offsets[flat[some]]
    ranges[some, 1] = offsets[flat[some] + 1] - offsets[flat[some]]
    return np.arange(nq + 1, dtype=np.int64) * nprobe, ranges


def invert(offsets, probes, n):
    """for every list the pairs q * nprobe + p that probe it, in pair order; a probe outside
    [0, nlist) and a list whose offsets are not 0 <= first <= next <= n or that has no rows
    have no pairs.  bad: some probe was neither -1 nor a list, or some probed list's offsets
    were bad."""
    nlist = len(offsets) - 1
    pairs = [[] for _ in range(nlist)]
    bad = False
    for pair, l in enumerate(probes.reshape(-1)):
        if not 0 <= l < nlist:
            bad |= l != -1
            continue
        first, nxt = int(offsets[l]), int(offsets[l + 1])
        if not 0 <= first <= nxt <= n:
            bad = True
        elif nxt > first:
            pairs[l].append(pair)
    return pairs, bad


def units(pairs, qb):
    """[(list, its pairs of this unit)]: ceil(pairs / qb) units a list"""
    return [(l, p[b:b + qb]) for l, p in enumerate(pairs) for b in range(0, len(p), qb)]


def search(lut, codes, k, offsets, probes, id_base=0, keep=None):
    """(dist float32 [nq][k], ids int64 [nq][k], units): lut [nq][m][K] (a table per query) or
    [nq * nprobe][m][K] (one per pair); keep: a row -> bool mask of the rows that take part"""
    n, m = codes.shape
    nq, nprobe = probes.shape
    per_pair = lut.shape[0] == nq * nprobe and nprobe > 1
    assert per_pair or lut.shape[0] == nq
    pairs, _ = invert(offsets, probes, n)
    work = units(pairs, qb_of(m))
    part = [[] for _ in range(nq * nprobe)]      # a pair's lists: one per unit that holds it
    for l, batch in work:
        rows = np.arange(offsets[l], offsets[l + 1], dtype=np.int64)
        if keep is not None:
            rows = rows[keep[rows]]
        decoded = codes[rows]                    # once for the whole batch
        for pair in batch:
            dist = ref.adc(lut[pair if per_pair else pair // nprobe], decoded)
            order = np.lexsort((rows, dist))[:k]
            part[pair].append((dist[order], rows[order]))
    wd = np.full((nq, k), np.inf, np.float32)
    wi = np.full((nq, k), -1, np.int64)
    for q in range(nq):
        mine = [e for pair in range(q * nprobe, (q + 1) * nprobe) for e in part[pair]]
        if not mine:
            continue
        dist = np.concatenate([d for d, _ in mine])
        rows = np.concatenate([r for _, r in mine])
        order = np.lexsort((rows, dist))[:k]
        wd[q, :len(order)] = dist[order]
        wi[q, :len(order)] = rows[order] + id_base
    return wd, wi, len(work)


# ------------------------------------------------------------------------------ the sweep's case
NLIST, NQ, NPROBE = 9, 21, 6
SHARED = (6, 7, 8)          # the queries that share one integer-valued table
PROBES = ([[3, 0, 2, 1, 4, 6],          # the long list, an empty and a single one
           [3, 6, 8, 7, 4, -1],         # list 8's only probe, the other empty list
           [2, -1, -1, -1, -1, -1],     # one row: fewer than k
           [1, 7, -1, -1, -1, -1],      # empty lists only: the padding
           [0, 3, -1, 3, 4, 0],         # lists 0 and 3 twice, -1 in the middle
           [-1] * 6] +                  # nothing at all
          [[6, 3, 0, -1, -1, -1]] * 3 +             # SHARED: ties across lists by stream row
          [[3, 6, 4, 2, -1, -1]] * 3 +
          [[3, 4, 0, 2, 1, -1]] * 7 +
          [[4, 0, 2, 7, -1, -1],
           [0, 4, -1, -1, -1, -1]])


def list_sizes(C):
    """list 1 and 7 empty, list 2 a single row, list 3 longer than 64 chunks and cut at both
    ends, the others of sizes that are no multiple of C (unless C = 1)"""
    return [3 * C + C // 2 + 1, 0, 1, 64 * C + C + 3, 37, 2 * C + 1, 150, 0, 5]


def sweep_case(m, chunk, seed):
    """(codes, offsets, probes, lut_q [NQ][m][256], lut_pair [NQ * NPROBE][m][256]): the codes
    in list order with the first 20 rows of list 0 again in lists 3 and 6; the tables of the
    SHARED queries (and of their pairs) one integer-valued table; the table of a pair without
    rows NaN"""
    offsets = np.concatenate([[0], np.cumsum(list_sizes(chunk))]).astype(np.int64)
    codes = datagen.skewed_codes(int(offsets[-1]), m, seed=seed)
    for l in (3, 6):
        codes[offsets[l]:offsets[l] + 20] = codes[:20]
    probes = np.array(PROBES, np.int64)
    assert probes.shape == (NQ, NPROBE)
    rng = np.random.default_rng(seed + 1)
    whole = rng.integers(0, 3, size=(m, 256)).astype(np.float32)
    lut_q = rng.normal(0.0, 100.0, size=(NQ, m, 256)).astype(np.float32)
    lut_pair = rng.normal(0.0, 100.0, size=(NQ * NPROBE, m, 256)).astype(np.float32)
    for q in SHARED:
        lut_q[q] = whole
        lut_pair[q * NPROBE:(q + 1) * NPROBE] = whole
    lut_pair[probe_ranges(offsets, probes)[1][:, 1] == 0] = np.nan
    return codes, offsets, probes, lut_q, lut_pair


def check_sweep_inputs(chunk, offsets, probes, m):
    """the properties the sweep relies on"""
    flat = probes.reshape(-1)
    times = np.bincount(flat[flat >= 0], minlength=NLIST)
    assert times[3] == 17 and times[6] == 8 and times[8] == 1 and times[5] == 0
    assert times[1] > 0 and times[7] > 0 and offsets[2] == offsets[1] and offsets[8] == offsets[7]
    assert offsets[3] - offsets[2] == 1
    f, c = offsets[3], offsets[4] - offsets[3]
    assert (f + c - 1) // chunk - f // chunk + 1 > 64
    assert chunk == 1 or (f % chunk and (f + c) % chunk)
    assert any(len(set(r[r >= 0])) < (r >= 0).sum() for r in probes)          # a list twice
    assert any((r[1:-1] == -1).any() and r[-1] >= 0 for r in probes)          # -1 in the middle
    assert any((r == -1).all() for r in probes)
    per_list = [len(p) for p in invert(offsets, probes, int(offsets[-1]))[0]]
    assert per_list[3] == 17 and per_list[1] == 0 and per_list[7] == 0
    n_units = len(units(invert(offsets, probes, int(offsets[-1]))[0], qb_of(m)))
    assert n_units == sum(-(-c // qb_of(m)) for c in per_list)
    return n_units
