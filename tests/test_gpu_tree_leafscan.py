"""The group tree builder's leaf heap by level passes (huff_trees_grp, PQH_TREE_LEAFSCAN):
alphabets of every size at which a heap level fills, a lane sub-group changes or a stretch
ends, under the count patterns of tests/leafscan_ref.py, with one heavy tree (64-bit keys,
the serial path) in a wavefront of scanned ones.  The group builder's codes must equal the
host builder's and the one-lane builder's byte for byte, in context and plain table sets,
through the split, the fused and the paired build."""
import numpy as np
import pytest

import leafscan_ref as L

pytestmark = pytest.mark.gpu

NZ = (0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256)


def _alphabets(seed):
    """(rows, 256) counts: every NZ x pattern, the heavy tree second in its wavefront"""
    rng = np.random.default_rng(seed)
    rows = [L.pattern_counts(p, nz, 256, rng) for nz in NZ for p in L.PATTERNS]
    heavy = L.pattern_counts("few", 200, 256, rng) * 30_000
    assert heavy.sum() >= 1 << 22 and all(r.sum() < 1 << 22 for r in rows)
    rows.insert(4 * 25 + 1, heavy)   # beside scanned trees of 128 symbols
    return np.stack(rows)


@pytest.fixture(scope="module")
def gpu():
    import torch
    from pq_huffman_amd import codec
    assert torch.cuda.is_available()
    return torch, codec, codec.Context(0)


@pytest.fixture(scope="module")
def sets():
    """context: 2 parts x 256 alphabets (the listed ones, then random sizes and patterns);
    plain: 127 parts of one alphabet each (the last wavefront has three trees)"""
    a = _alphabets(3)
    assert a.shape == (len(NZ) * len(L.PATTERNS) + 1, 256)
    rng = np.random.default_rng(5)
    more = [L.pattern_counts(L.PATTERNS[i % len(L.PATTERNS)], int(rng.integers(0, 257)), 256, rng)
            for i in range(512 - len(a))]
    ctx_counts = np.concatenate([a, np.stack(more)]).reshape(2, 256 * 256)
    return {True: ctx_counts, False: a}


@pytest.fixture(scope="module")
def host(sets):
    from pq_huffman_amd import codec
    return {c: codec.Codebooks(v.astype(np.float64), 256, c).file_bytes() for c, v in sets.items()}


def _dev(gpu, counts):
    return gpu[0].from_numpy(counts.astype(np.int32)).cuda()


@pytest.mark.parametrize("ctxm", [True, False])
def test_group_builder_equals_host_and_lane(gpu, sets, host, ctxm):
    torch, codec, ctx = gpu
    counts = _dev(gpu, sets[ctxm])
    m = sets[ctxm].shape[0]
    grp = codec.Tables(ctx, m, 256, ctxm).build(counts, trees="grp")
    grp.status()
    lane = codec.Tables(ctx, m, 256, ctxm).build(counts, trees="lane")
    lane.status()
    got = grp.codebooks().file_bytes()
    assert got == host[ctxm]
    assert got == lane.codebooks().file_bytes()


def test_fused_split_and_paired_builds(gpu, sets, host):
    """the same leaf phase through the other entry paths: the default (fused) build, the
    trees and the decode tables as two calls, and two table sets in one launch"""
    torch, codec, ctx = gpu
    counts = _dev(gpu, sets[True])
    fused = codec.Tables(ctx, 2, 256, True).build(counts)
    fused.status()
    assert fused.codebooks().file_bytes() == host[True]
    split = codec.Tables(ctx, 2, 256, True).build_trees(counts, trees="grp").build_luts()
    split.status()
    assert split.codebooks().file_bytes() == host[True]
    t1, t2 = codec.Tables(ctx, 2, 256, True), codec.Tables(ctx, 2, 256, True)
    swapped = np.ascontiguousarray(sets[True][::-1])
    t1.build_pair(counts, t2, _dev(gpu, swapped))
    t1.status()
    t2.status()
    assert t1.codebooks().file_bytes() == host[True]
    assert t2.codebooks().file_bytes() == codec.Codebooks(swapped.astype(np.float64), 256,
                                                          True).file_bytes()
