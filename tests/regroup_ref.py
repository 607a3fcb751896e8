"""numpy reference of the regroup plan (pqh_ivf_regroup) and of the decode through it
(pqh_decode_scatter), written from the definitions in include/pqh.h: a loop over the lists and
their rows, nothing of the prefix-count form the kernels use."""
import numpy as np


def pack(keep):
    """bool (n,) -> the mask words of pqh_mask_pack: bit i & 31 of word i >> 5"""
    keep = np.asarray(keep, bool)
    n = len(keep)
    words = np.zeros((n + 31) // 32, np.uint32)
    for i in np.flatnonzero(keep):
        words[i >> 5] |= np.uint32(1) << np.uint32(i & 31)
    return words


def regroup(offsets, keep=None, add_offsets=None):
    """(new_offsets, dest, add_base) for list offsets (nlist + 1,), keep bool (n,) or None = all,
    add_offsets (nlist + 1,) or None = none"""
    offsets = np.asarray(offsets, np.int64)
    nlist, n = len(offsets) - 1, int(offsets[-1])
    keep = np.ones(n, bool) if keep is None else np.asarray(keep, bool)
    add = np.zeros(nlist, np.int64) if add_offsets is None else np.diff(np.asarray(add_offsets, np.int64))
    new_offsets = np.zeros(nlist + 1, np.int64)
    dest = np.full(n, -1, np.int64)
    add_base = np.zeros(nlist, np.int64)
    for l in range(nlist):
        at = int(new_offsets[l])
        for r in range(int(offsets[l]), int(offsets[l + 1])):
            if keep[r]:
                dest[r] = at
                at += 1
        add_base[l] = at
        new_offsets[l + 1] = at + add[l]
    return new_offsets, dest, add_base


def scatter(codes, dest, out):
    """out[dest[r]] = codes[r] where 0 <= dest[r] < len(out), in place; returns out"""
    for r, d in enumerate(dest):
        if 0 <= d < len(out):
            out[d] = codes[r]
    return out


def add_slots(add_offsets, add_base):
    """the new row of every row of a batch in its own list order: add_base[list] + rank"""
    add_offsets = np.asarray(add_offsets, np.int64)
    return np.concatenate([add_base[l] + np.arange(add_offsets[l + 1] - add_offsets[l])
                           for l in range(len(add_base))] + [np.zeros(0, np.int64)]).astype(np.int64)


# the six-list world of the hand-checked cases: lists 1 and 4 empty, the boundaries 3 and 10 inside
# mask word 0 and 34 inside word 1
SIX_OFFSETS = np.array([0, 3, 3, 10, 34, 34, 40], np.int64)
SIX_ADD = np.array([0, 2, 2, 2, 5, 6, 6], np.int64)          # 2, 0, 0, 3, 1, 0 new rows
SIX_KEPT = (1, 3, 9, 10, 33, 34, 39)


def six_keep(kind, seed=5):
    n = int(SIX_OFFSETS[-1])
    if kind == "none":
        return None
    if kind == "zero":
        return np.zeros(n, bool)
    if kind == "hand":
        keep = np.zeros(n, bool)
        keep[list(SIX_KEPT)] = True
        return keep
    assert kind == "random"
    return np.random.default_rng(seed).random(n) < 0.5
