"""The leaf heap of a Huffman build three ways (pure Python, no GPU):

push_heap    the reference's push loop (huffman_encode.c:33-46): every non-zero symbol, in
             symbol order, is appended and sifts up while strictly lighter than its parent;
level_heap   the same heap by level passes: a node only filters the entries that arrive at
             it, so every level is an exclusive prefix minimum per node under one composite
             order (weight, tie word);
lane_heap    level_heap in the schedule of the 16-lane group builder (huff_trees_grp,
             K <= 256): one u32 word per arrival, lane sub-groups with runs of 16 ranks and a
             segmented scan for levels 0-3, whole nodes per lane below, every run and every
             node's ranks 2^k .. 2^(k+1) - 1 one aligned vector of words.

Heaps are lists of (weight, symbol), position 1 first.
"""


def leaves(counts):
    return [(int(c), s) for s, c in enumerate(counts) if c]


def push_heap(counts):
    h = []
    for e in leaves(counts):
        i = len(h)
        h.append(e)
        while i > 0:
            p = (i - 1) >> 1
            if not e[0] < h[p][0]:
                break
            h[i] = h[p]
            i = p
        h[i] = e
    return h


def level_heap(counts, k=256):
    """Arrival t (1-based: the push's time and its final slot) carries an entry and a flag;
    its key is (weight, flag ? k - t : k - 1 + t): a displaced occupant takes the node from
    any equal weight, a later one from an earlier one; an entry still looking for its node
    takes it only from a strictly heavier one."""
    ev = leaves(counts)
    nz = len(ev)
    arr = {t: (ev[t - 1], 0) for t in range(1, nz + 1)}
    heap = {}
    level = 0
    while (1 << level) <= nz:
        for v in range(1 << level, min(2 << level, nz + 1)):
            occ = None   # (key, entry): the prefix minimum
            r = 0
            while True:
                kk = (r + 1).bit_length() - 1
                t = (v << kk) + r + 1 - (1 << kk)
                if t > nz:
                    break
                e, flag = arr[t]
                ky = (e[0], k - t if flag else k - 1 + t)
                if occ is None:
                    occ = (ky, e)
                elif ky < occ[0]:
                    arr[t] = (occ[1], 1)
                    occ = (ky, e)
                else:
                    assert not flag, "a displaced occupant always takes the node"
                r += 1
            heap[v] = occ[1]
        level += 1
    return [heap[v] for v in range(1, nz + 1)]


# ---- the group builder's schedule (K <= 256) -------------------------------------------------
# A word is the heap key weight << 10 | symbol with bit 9 set while the entry still looks for
# its node.  The tie word's other bits only say which of two arrivals came first, and the
# schedule knows that from where it stands: inside a run from the order of the ranks, between
# runs from the order of the lanes.  So "y (later) takes the node from x" is one compare.
# Arrival t lives in word t; words past the last leaf are all ones (they take no node and
# send themselves on), word 0 is nobody's.  The passes cover slots 1-255; the 256th symbol of
# a full alphabet is pushed after them.
_MAX = 0xFFFFFFFF


def _takes(y, xm):
    """arrival y against the occupant's compare form xm (its word & ~511, all ones = none)"""
    return y - (~y & 512) < xm


def _filter(x, occ, occm, send):
    """the arrivals x of one node in rank order; send: each is replaced by what it sends on"""
    for u in range(len(x)):
        if _takes(x[u], occm):
            out, occ, occm = occ & ~512, x[u], x[u] & ~511
        else:
            out = x[u]
        if send:
            x[u] = out
    return occ, occm


def lane_heap(counts):
    ev = leaves(counts)
    nz = len(ev)
    assert nz <= 256 and sum(c for c, _ in ev) < (1 << 22)
    n = min(nz, 255)
    w = [_MAX] * 256
    for j, (c, s) in enumerate(ev[:255]):
        w[j + 1] = (c << 10) | 512 | s
    h = {}
    level = 0
    while level < 4 and (1 << level) <= n:
        lanes = range(16)
        sl = [g & (15 >> level) for g in lanes]
        v = [(1 << level) + (g >> (4 - level)) for g in lanes]
        # a lane's words: b + j * mul, j = 0 .. 15
        idx = []
        for g in lanes:
            if sl[g]:
                b = ((v[g] - 1) << (3 + sl[g].bit_length())) + 16 * sl[g]
                idx.append([b + j for j in range(16)])
            else:
                idx.append([0, v[g]] + [2 * v[g] + j for j in range(2)]
                           + [4 * v[g] + j for j in range(4)] + [8 * v[g] + j for j in range(8)])
        m = [_filter([w[i] for i in idx[g]], _MAX, _MAX, False)[0] for g in lanes]
        for d in (1, 2, 4, 8):                 # row_shr d, kept inside the node's lanes
            y = [m[g - d] if g >= d else _MAX for g in lanes]
            m = [y[g] if sl[g] >= d and not _takes(m[g], y[g] & ~511) else m[g] for g in lanes]
        for g in lanes:
            if sl[g] == (15 >> level) and v[g] <= n:
                h[v[g]] = m[g] & ~512
        y = [m[g - 1] if g >= 1 else _MAX for g in lanes]
        new = {}
        for g in lanes:                        # (the lanes' words are disjoint, but for word 0)
            x = [w[i] for i in idx[g]]
            _filter(x, *((y[g], y[g] & ~511) if sl[g] else (_MAX, _MAX)), True)
            for i, xi in zip(idx[g], x):
                assert new.setdefault(i, xi) == xi
        for i, xi in new.items():
            w[i] = xi
        assert w[0] == _MAX
        level += 1
    while level < 8 and (1 << level) <= n:
        for v in range(1 << level, 2 << level):   # one lane each: v = 2^level + lane, + 16, ...
            segs = [[v]] + [[(v << k) + j for j in range(1 << k)] for k in range(1, 8 - level)]
            occ, occm = _MAX, _MAX
            for seg in segs:
                x = [w[i] for i in seg]
                occ, occm = _filter(x, occ, occm, True)
                if seg != [v]:                 # (rank 1 fills the node: not written)
                    for i, xi in zip(seg, x):
                        w[i] = xi
            if v <= n:
                h[v] = occ & ~512
        level += 1
    heap = [(h[v] >> 10, h[v] & 511) for v in range(1, n + 1)]
    if nz == 256:                              # the last symbol: one push
        e, i = ev[255], 255
        heap.append(e)
        while i > 0 and e[0] < heap[(i - 1) >> 1][0]:
            heap[i] = heap[(i - 1) >> 1]
            i = (i - 1) >> 1
        heap[i] = e
    return heap


# ---- count patterns ---------------------------------------------------------------------------
PATTERNS = ("equal", "two", "ascending", "descending", "few", "wide", "gaps")


def pattern_counts(name, nz, k, rng):
    """A count vector of k symbols with nz non-zero ones.  `rng` is a numpy Generator."""
    import numpy as np
    if name == "equal":
        w = np.full(nz, 7)
    elif name == "two":
        w = rng.choice([3, 11], nz)
    elif name == "ascending":
        w = np.arange(1, nz + 1)
    elif name == "descending":
        w = np.arange(nz, 0, -1)
    elif name == "few":
        w = rng.choice([1, 1, 1, 2, 5], nz)
    elif name in ("wide", "gaps"):
        w = rng.integers(1, 1 << 13, nz)
    else:
        raise ValueError(name)
    c = np.zeros(k, np.int64)
    if name == "gaps" and nz < k:
        # zeros interleaved with the non-zero symbols
        sym = np.sort(rng.choice(k, nz, replace=False))
    elif name == "gaps" or nz == k:
        sym = np.arange(nz)
    else:
        sym = np.arange(nz) + (k - nz) // 2   # one block, off the start
    c[sym] = w
    return c
