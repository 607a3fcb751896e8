"""The leaf heap by level passes (tests/leafscan_ref.py) against the reference's push loop:
every alphabet size from 0 to 256 and the sizes around the level edges of a 4,096-symbol
heap, each under all-equal, two-valued, ascending, descending, tie-heavy, wide-range and
zero-interleaved counts.  No GPU."""
import numpy as np
import pytest

import leafscan_ref as L

NZ_4096 = (1, 2, 63, 64, 65, 2047, 2048, 2049, 4095, 4096)


@pytest.mark.parametrize("pattern", L.PATTERNS)
def test_level_passes_equal_push_loop_k256(pattern):
    """the model of the level passes, and its schedule in the 16-lane builder, slot for slot"""
    rng = np.random.default_rng(L.PATTERNS.index(pattern))
    for nz in range(257):
        c = L.pattern_counts(pattern, nz, 256, rng)
        assert int((c != 0).sum()) == nz
        want = L.push_heap(c)
        assert L.level_heap(c) == want, (pattern, nz)
        assert L.lane_heap(c) == want, (pattern, nz)


@pytest.mark.parametrize("pattern", L.PATTERNS)
def test_level_passes_equal_push_loop_k4096(pattern):
    rng = np.random.default_rng(100 + L.PATTERNS.index(pattern))
    for nz in NZ_4096:
        c = L.pattern_counts(pattern, nz, 4096, rng)
        assert int((c != 0).sum()) == nz
        assert L.level_heap(c, 4096) == L.push_heap(c), (pattern, nz)


def test_lane_schedule_random_ties():
    """random alphabets with few distinct weights: displaced occupants meet equal weights at
    every level, in runs that cross lanes"""
    rng = np.random.default_rng(7)
    for _ in range(300):
        nz = int(rng.integers(0, 257))
        c = np.zeros(256, np.int64)
        c[rng.choice(256, nz, replace=False)] = rng.integers(1, 4, nz)
        want = L.push_heap(c)
        assert L.level_heap(c) == want
        assert L.lane_heap(c) == want


def test_lane_schedule_heaviest_light_tree():
    """one symbol of weight 2^22 - 1: the largest word a scanned tree can hold"""
    c = np.zeros(256, np.int64)
    c[255] = (1 << 22) - 1
    assert L.lane_heap(c) == L.push_heap(c) == [((1 << 22) - 1, 255)]
