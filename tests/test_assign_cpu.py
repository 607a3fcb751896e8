"""The inputs of the assignment and k-means edge tests, checked on the CPU: the near-tie rows
of assign_ref.near_tie cover the acceptance band of DESIGN.md section 4.1 (below, inside and
above tau), the oracle's codes survive the scales the GPU tests use (and not 2^-75), the
bf16-split screening score stays inside the split term of the documented bound on this data,
and the K = 4,096 k-means case leaves clusters empty.  Conditions on inputs and on the
oracle, not on the kernel."""
import numpy as np
import pytest

import assign_ref as ar


@pytest.fixture(scope="module")
def band():
    """{(dsub, offset): (x, cent)} of the near-tie cases the GPU tests run"""
    return {(dsub, off): ar.near_tie(ar.N_BAND, ar.parts_of(dsub), dsub, seed=100 + dsub,
                                     offset=off)
            for dsub in ar.DSUBS for off in (0.0, 64.0)}


def _pairs(x, cent):
    """per part: (x_part, cent_part)"""
    m, _, dsub = cent.shape
    return [(x[:, p * dsub:(p + 1) * dsub], cent[p]) for p in range(m)]


def _gap_over_tau(x, cent):
    """fp32 direct-form gap of the two best centroids over tau (any_lo), all (row, part) pairs"""
    out = []
    for xp, cp in _pairs(x, cent):
        _, g = ar.direct_gap(xp, cp)
        out.append(g / ar.tau_doc(xp, cp, True))
    return np.concatenate(out)


@pytest.mark.parametrize("dsub", ar.DSUBS)
def test_near_tie_rows_cover_the_band(band, oracle, dsub):
    """offset 0: rows far below tau, rows inside 0.1 tau .. 10 tau and rows far above it;
    offset 64 (cancellation): nearly every row far below tau.  numpy's direct form is the
    oracle's: the same codes."""
    x, cent = band[(dsub, 0.0)]
    want, _ = oracle.pq_assign(x, cent, threads=0)
    for p, (xp, cp) in enumerate(_pairs(x, cent)):
        assert np.array_equal(ar.direct_gap(xp, cp)[0], want[:, p])
    q = _gap_over_tau(x, cent)
    below, inside, above = (q < 0.1).mean(), ((q >= 0.1) & (q <= 10)).mean(), (q > 10).mean()
    print(f"dsub {dsub} offset 0: below {below:.3f} inside {inside:.3f} above {above:.3f}")
    assert below >= 0.20
    assert inside >= 0.15
    assert above >= 0.05
    q64 = _gap_over_tau(*band[(dsub, 64.0)])
    print(f"dsub {dsub} offset 64: below {(q64 < 0.1).mean():.4f}")
    assert (q64 < 0.1).mean() >= 0.90


def test_some_rows_need_the_direct_form(band, oracle):
    """Over the whole set some (row, part) pair's float64 argmin differs from the oracle's fp32
    argmin: there only the fp32 direct form gives the defined answer."""
    differ = 0
    for dsub in ar.DSUBS:
        x, cent = band[(dsub, 0.0)]
        want, _ = oracle.pq_assign(x, cent, threads=0)
        for p, (xp, cp) in enumerate(_pairs(x, cent)):
            differ += int((ar.argmin64(xp, cp) != want[:, p]).sum())
    print("pairs whose float64 argmin differs:", differ)
    assert differ >= 1


@pytest.mark.parametrize("dsub", ar.DSUBS)
def test_oracle_codes_survive_the_scales(band, oracle, dsub):
    """x and cent times 2^40, 2^-40, 2^62: the oracle's codes are those of scale 1 (a power of
    two scales every fp32 step exactly while nothing the minimum needs overflows); at 2^-75
    the squares underflow and the codes change, so a GPU test compares with the oracle at its
    own scale."""
    x, cent = band[(dsub, 0.0)]
    want, _ = oracle.pq_assign(x, cent, threads=0)
    for s in (40, -40, 62):
        got, _ = oracle.pq_assign(ar.scaled(x, s), ar.scaled(cent, s), threads=0)
        assert np.array_equal(got, want), (s, (got != want).sum())
    tiny, _ = oracle.pq_assign(ar.scaled(x, -75), ar.scaled(cent, -75), threads=0)
    changed = (tiny != want).any(axis=1).mean()
    print(f"dsub {dsub}: rows changed at 2^-75: {changed:.4f}")
    # (squares survive only as multiples of 2^-149, so near ties collapse onto the first
    # index: 41 % of the rows at dsub 32 to 99 % at dsub 4)
    assert not np.array_equal(tiny, want) and changed > 0.25


@pytest.mark.parametrize("offset", [0.0, 64.0])
@pytest.mark.parametrize("dsub", ar.DSUBS)
def test_split_score_within_the_split_term(band, dsub, offset):
    """The screening score from exact products of the bf16 halves lies within 2^-13 P of
    D_real - X, and the form without xl (x rounded to bf16 first) within 2 sqrt(X) R, at scales
    1 and 2^+-40.  This pins the dominant (split) term of E0 and build_afrag's r2_out
    definition on the test data; it says nothing about the MFMA's fp32 accumulation, which the
    other terms of E0 cover."""
    x0, c0 = band[(dsub, offset)]
    for s in (0, 40, -40):
        x, cent = ar.scaled(x0, s), ar.scaled(c0, s)
        for xp, cp in _pairs(x, cent):
            X = (xp.astype(np.float64) ** 2).sum(1)
            cmax = (cp.astype(np.float64) ** 2).sum(1).max()
            P = np.sqrt(X) * np.sqrt(cmax)
            err = np.abs(ar.screen_scores(xp, cp, True) - ar.real_scores(xp, cp)).max(1)
            assert (err <= 2.0 ** -13 * P).all(), (s, (err / P).max())
            # x = xh: the score misses exactly 2 x . r'_k (Cauchy-Schwarz; 1e-9: the float64
            # evaluation of both sides)
            xb = ar.bf16_rne(xp)
            Xb = (xb.astype(np.float64) ** 2).sum(1)
            err0 = np.abs(ar.screen_scores(xb, cp, False) - ar.real_scores(xb, cp)).max(1)
            bound = 2.0 * np.sqrt(Xb) * ar.split_remainder(cp)
            assert (err0 <= bound * (1 + 1e-9)).all(), (s, (err0 / bound).max())


def test_bf16_split_bits():
    """bf16_split on values whose rounding is known: ties go to even, the halves are bf16"""
    a = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.00390625 + 2.0 ** -20, -3.1415927,
                  2.0 ** -130], np.float32)
    hi, lo = ar.bf16_split(a)
    assert hi[0] == 1.0 and lo[0] == 0.0
    assert hi[1] == 1.0 and lo[1] == np.float32(2.0 ** -8)            # tie -> even (down)
    assert hi[2] == np.float32(1.0 + 2.0 ** -6) and lo[2] == np.float32(-(2.0 ** -8))   # tie -> even (up)
    assert not (hi.view(np.uint32) & 0xFFFF).any() and not (lo.view(np.uint32) & 0xFFFF).any()
    rem = a.astype(np.float64) - hi.astype(np.float64) - lo.astype(np.float64)
    assert (np.abs(rem) <= 2.0 ** -16 * np.abs(a.astype(np.float64))).all()


def test_kmeans_k4096_case_leaves_clusters_empty(oracle):
    """(n, d, m, k) = (3000, 32, 2, 4096): n < k, so clusters stay empty at every iteration.
    More than 1,000 of the 8,192 are empty in the last of two iterations; an empty cluster
    keeps its bits of the iteration before, and one empty in both keeps its initial bits."""
    x, init = ar.kmeans_case(3000, 32, 2, 4096)
    c1 = oracle.kmeans(x, init, 1, threads=0)
    c2 = oracle.kmeans(x, init, 2, threads=0)
    size1 = ar.cluster_sizes(oracle.pq_assign(x, init, threads=0)[0], 4096)
    size2 = ar.cluster_sizes(oracle.pq_assign(x, c1, threads=0)[0], 4096)
    empty2 = size2 == 0
    print("empty in the last iteration:", int(empty2.sum()), "of", empty2.size)
    assert empty2.sum() > 1000
    assert np.array_equal(c2[empty2].view(np.uint32), c1[empty2].view(np.uint32))
    both = empty2 & (size1 == 0)
    assert both.sum() > 1000
    assert np.array_equal(c2[both].view(np.uint32), init[both].view(np.uint32))
    assert np.isfinite(c2).all()


def test_kmeans_table_reaches_both_non_lds_forms():
    """the byte counts test_gpu_kmeans.py states: dsub 23 is the last LDS shape at K = 256"""
    assert ar.kmeans_lds_bytes(256, 23) == 48128 <= 48 * 1024
    assert ar.kmeans_lds_bytes(256, 24) == 50176 > 48 * 1024
    assert ar.kmeans_lds_bytes(256, 32) == 66560 > 48 * 1024
    assert ar.kmeans_lds_bytes(4096, 16) == 540672 > 48 * 1024
    assert ar.kmeans_lds_bytes(64, 128) == 65792 > 48 * 1024
    assert ar.kmeans_lds_bytes(16, 8) == 1088 <= 48 * 1024


def test_kmeans_scale_cases_stay_finite(oracle):
    """x 2^-120 (the shift clamps at 100: every fixed-point term rounds to 0, every square
    underflows) and x 2^100 (a negative shift; every squared distance overflows, all rows go
    to code 0): the oracle returns finite centroids for both."""
    x, init = ar.kmeans_case(3000, 32, 2, 256)
    for s in (-120, 100):
        xs, cs = ar.scaled(x, s), ar.scaled(init, s)
        assert np.isfinite(xs).all() and (xs != 0).any()
        shift = oracle.lib().orc_kmeans_shift(float(np.abs(xs).max()), xs.shape[0])
        assert (shift == 100) if s < 0 else (-126 < shift < 0)
        codes, _ = oracle.pq_assign(xs, cs, threads=0)
        # (2^100: a row that is its own initial centroid has distance 0, the only finite one)
        assert (codes == 0).all() if s < 0 else (codes == 0).mean() > 0.9
        got = oracle.kmeans(xs, cs, 2, threads=0)
        assert np.isfinite(got).all()
        if s < 0:   # cluster 0 takes every row and a sum of zeros; the rest keep their bits
            assert (got[:, 0] == 0).all()
            assert np.array_equal(got[:, 1:].view(np.uint32), cs[:, 1:].view(np.uint32))
