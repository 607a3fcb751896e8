"""The numpy float32 restatement of the 8-bit scalar quantizer of pqh.h (IVF-SQ8): every operation
one fp32 rounding, no fused multiply-add.  search is flat_lists_ref.search over the decoded rows.
Nothing calls the library."""
import numpy as np

import flat_lists_ref

F = np.float32


def train(x):
    """(vmin, step): per column the minimum of the finite values (-0 below +0) and a 255th of
    their range; (0, 0) for a column without one"""
    x = np.asarray(x, F)
    vmin, step = np.zeros(x.shape[1], F), np.zeros(x.shape[1], F)
    for j in range(x.shape[1]):
        col = x[:, j][np.isfinite(x[:, j])]
        if len(col):
            u = col.view(np.uint32)
            key = np.where(u >> 31, ~u, u | np.uint32(1 << 31))   # the order of the values
            lo, hi = col[np.argmin(key)], col[np.argmax(key)]
            vmin[j], step[j] = lo, F(hi - lo) / F(255)
    return vmin, step


def encode(x, vmin, step):
    with np.errstate(all="ignore"):
        t = (np.asarray(x, F) - vmin) / step
        return np.where(np.isnan(t), F(0), np.clip(np.rint(t), 0, 255)).astype(np.uint8)


def decode(codes, vmin, step):
    return vmin + codes.astype(F) * step


def search(q, codes, vmin, step, offsets, probes, k, metric="l2", keep=None, id_base=0):
    return flat_lists_ref.search(q, decode(codes, vmin, step), offsets, probes, k, metric, keep, id_base)
