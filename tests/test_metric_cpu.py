"""Host-side parts of the inner-product metric: the calls are exported, declared and bound, a
process that sees no GPU gets PQH_ERR_NO_DEVICE from each of them, and the numpy reference the
GPU tests compare against (tests/metric_ref.py) is checked against integer arithmetic, against a
hand-made case that fixes what "nearest" means, and for the recall it was made for."""
import os
import subprocess
import sys

import numpy as np

import ivf_ref
import metric_ref as mr
import refine_ref
from conftest import ROOT
from pq_huffman_amd import capi, codec

NEW_CALLS = ["pqh_adc_tables_ip", "pqh_coarse_assign_ip", "pqh_coarse_probe_ip",
             "pqh_adc_tables_residual_ip", "pqh_refine_stream_ip", "pqh_refine_codes_ip"]
TWINS = {name: name[:-3] for name in NEW_CALLS}


def test_metric_calls_are_exported_declared_and_bound():
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    header = open(os.path.join(ROOT, "include", "pqh.h")).read()
    bound = {name: args for name, _, args in capi.SIGNATURES}
    for name in NEW_CALLS:
        assert name in exported and name in bound and f"int {name}(" in header, name
        assert bound[name] == bound[TWINS[name]], name          # the arguments of its L2 twin
        assert getattr(capi.lib(), name).argtypes
    import inspect
    for fn in (codec.adc_tables, codec.adc_tables_residual, codec.Coarse.assign,
               codec.Coarse.probe, codec.IVF.build):
        assert inspect.signature(fn).parameters["metric"].default == "l2", fn
    # the re-rank's parameter list is pinned by tests/test_refine_cpu.py: its ip form is a twin
    assert (list(inspect.signature(codec.refine_ip).parameters) ==
            list(inspect.signature(codec.refine).parameters))


def test_an_unknown_metric_is_an_argument_error():
    """before anything touches a device: every argument but the metric is None"""
    for fn in (lambda: codec.adc_tables(None, None, None, metric="cosine"),
               lambda: codec.adc_tables_residual(None, None, None, None, None, metric="L2"),
               lambda: codec.Coarse.assign(None, None, metric="dot"),
               lambda: codec.Coarse.probe(None, None, 1, None, metric=None),
               lambda: codec.IVF.build(None, None, None, None, metric="IP")):
        try:
            fn()
        except capi.PqhError as err:
            assert err.status == -1
        else:
            raise AssertionError("no PqhError")


PROBE = """
from pq_huffman_amd import capi
L = capi.lib()
print(L.pqh_adc_tables_ip(None, None, None, 1, 8, None),
      L.pqh_coarse_assign_ip(None, None, None, 10, 8, None, None),
      L.pqh_coarse_probe_ip(None, None, None, 1, 8, 2, None, None, None, None, None),
      L.pqh_adc_tables_residual_ip(None, None, None, None, 1, 8, None, 2, None),
      L.pqh_refine_stream_ip(None, None, None, None, 0, 1, 1, None, None, None, None, None, 0, 1, 1,
                             None, None, 10, None, None, None, 1, 8, None, 1, 1, None, None, 1),
      L.pqh_refine_codes_ip(None, None, None, None, None, 10, None, None, None, 1, 8, None, 1, 1,
                            None, None, 1),
      L.pqh_adc_tables(None, None, None, 1, 8, None),
      L.pqh_refine_codes(None, None, None, None, None, 10, None, None, None, 1, 8, None, 1, 1,
                         None, None, 1))
"""


def test_metric_calls_without_a_device():
    """the devices hidden: no context can exist, and every new call says so, as its twin does"""
    env = dict(os.environ)
    env["HIP_VISIBLE_DEVICES"] = ""
    env["ROCR_VISIBLE_DEVICES"] = ""
    r = subprocess.run([sys.executable, "-c", PROBE], capture_output=True, text=True, env=env,
                       cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["-2"] * 8, r.stdout + r.stderr


def test_the_chains_equal_int64_on_the_integer_grid():
    for n, d, nlist in ((63, 5, 70), (40, 130, 257), (7, 1, 3)):
        x, c = ivf_ref.integer_grid(n, d, nlist, seed=n + d)
        got = mr.nip(x, c)
        want = mr.nip_int64(x, c)
        assert got.dtype == np.float32 and np.abs(want).max() < 2 ** 24
        assert np.array_equal(got.astype(np.int64), want)
        lists, score = mr.assign(x, c, got)
        assert lists.dtype == np.int32 and np.array_equal(score.astype(np.int64), want.min(axis=1))
        first = np.array([np.flatnonzero(want[v] == want[v].min())[0] for v in range(n)])
        assert np.array_equal(lists, first)
        if d <= 5 and nlist >= 70:
            assert ((want == want.min(axis=1, keepdims=True)).sum(axis=1) > 1).any()
        # the probe order is (score, list), the padding as ivf_ref's
        offsets = np.arange(nlist + 1, dtype=np.int64) * 2
        ptr, ranges, probes, pd = mr.probe(x, c, 5, offsets, got)
        for v in range(n):
            key = sorted((want[v, l], l) for l in range(nlist))[:5]
            assert [l for _, l in key] == probes[v, :len(key)].tolist()
            assert (probes[v, len(key):] == -1).all() and np.isinf(pd[v, len(key):]).all()
        assert np.array_equal(pd[:, 0], score)
    # the sign of a zero: +0 - (+0 * y) is +0, and a chain that ends at zero ends at +0
    z = mr.nip(np.array([[0.0, 1.0, -1.0]], np.float32), np.array([[5.0, 2.0, 2.0]], np.float32))
    assert z.view(np.uint32)[0, 0] == 0
    z = mr.nip(np.array([[0.0]], np.float32), np.array([[-5.0]], np.float32))
    assert z.view(np.uint32)[0, 0] == 0


def test_the_tables_and_the_re_rank_equal_int64_on_the_integer_grid():
    rng = np.random.default_rng(8)
    m, k, dsub, nlist, nq, nprobe = 3, 17, 5, 6, 4, 3
    cent = rng.integers(-4, 5, size=(m, k, dsub)).astype(np.float32)
    q, c = ivf_ref.integer_grid(nq, m * dsub, nlist, seed=9)
    lut = mr.tables(q, cent)
    assert lut.shape == (nq, m, k) and lut.dtype == np.float32
    for i in range(m):
        assert np.array_equal(lut[:, i].astype(np.int64),
                              mr.nip_int64(q[:, i * dsub:(i + 1) * dsub], cent[i]))
    # a residual table summed over a code row is the score of c[l] + the reconstruction
    probes = np.array([[0, 5, -1], [2, 2, 1], [3, nlist, 4], [1, 0, -7]], np.int64)
    res = mr.tables_residual(q, c, probes, cent)
    codes = rng.integers(0, k, size=(50, m)).astype(np.uint8)
    rec = refine_ref.reconstruct(cent, codes)
    from ivf_residual_ref import adc
    for o, l in enumerate(probes.reshape(-1)):
        if not 0 <= l < nlist:
            assert np.isinf(res[o]).all() and (res[o] > 0).all()
            continue
        want = mr.nip_int64(q[o // nprobe][None], c[l][None] + rec)[0]
        assert np.array_equal(adc(res[o], codes).astype(np.int64), want)
    # the re-rank: two levels, with and without the centroid of the row's list
    w = refine_ref.ties_world()
    a, b = w["codes1"][:30], w["codes2"][:30]
    cl = ivf_ref.integer_grid(30, 16, 1, seed=3)[0]
    for cc in (None, cl):
        got = mr.refine_dists(w["q"][0], w["cent1"], a, w["cent2"], b, cc)
        assert np.array_equal(got.astype(np.int64),
                              mr.refine_int64(w["q"][0], w["cent1"], a, w["cent2"], b, cc))


def test_ranking_differs_from_l2():
    """q = (1, 0): the row (10, 0) is the nearest by inner product and the farthest by L2"""
    q = np.array([[1.0, 0.0]], np.float32)
    rows = np.array([[1.0, 0.0], [10.0, 0.0]], np.float32)
    ip, l2 = mr.nip(q, rows)[0], ivf_ref.dists(q, rows)[0]
    assert ip.tolist() == [-1.0, -10.0] and l2.tolist() == [0.0, 81.0]
    assert mr.assign(q, rows)[0].tolist() == [1] and ivf_ref.assign(q, rows)[0].tolist() == [0]
    offsets = np.array([0, 1, 2], np.int64)
    assert mr.probe(q, rows, 2, offsets)[2].tolist() == [[1, 0]]
    assert ivf_ref.probe(q, rows, 2, offsets)[2].tolist() == [[0, 1]]


def test_the_ip_mirror_finds_more_of_the_exact_answer_than_the_l2_mirror():
    """rows of spread norms (metric_ref.spread_world: 4,000 centred SIFT-like rows of 32
    dimensions scaled by a log-normal factor, 32 lists, 4 probes, an 8 x 64 PQ): recall@10 of the
    exact maximum-inner-product rows is 0.355 for the ip mirror and 0.0 for the L2 mirror, whose
    nearest rows are the short ones.  A statement about the mirrors, not a tolerance on the GPU."""
    x, q, cc, cent = mr.spread_world()
    truth = mr.exact_mips(x, q, 10)
    got = {}
    for metric in ("ip", "l2"):
        w = mr.build(x, cc, cent, False, metric)
        got[metric] = mr.recall(mr.search(w, q, 4, 10)[1], truth)
    print("recall@10 of the exact inner-product answer:", got)
    assert got["ip"] > got["l2"]
