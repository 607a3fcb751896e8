"""Host-side parts of the inverted-file front end (pqh_coarse_*, pqh_ivf_*): the calls are
exported, declared and bound, a process that sees no GPU gets PQH_ERR_NO_DEVICE from each call
that takes a context, and the numpy reference the GPU tests compare against (tests/ivf_ref.py)
is checked against integer arithmetic and against codec.ivf_layout on CPU tensors."""
import os
import subprocess
import sys

import numpy as np

import ivf_ref
from conftest import ROOT
from pq_huffman_amd import capi, codec

NEW_CALLS = ["pqh_coarse_create", "pqh_coarse_destroy", "pqh_coarse_assign", "pqh_ivf_layout",
             "pqh_coarse_probe", "pqh_ivf_status"]


def test_ivf_calls_are_exported_declared_and_bound():
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    header = open(os.path.join(ROOT, "include", "pqh.h")).read()
    bound = {name for name, _, _ in capi.SIGNATURES}
    for name in NEW_CALLS:
        assert name in exported and name in bound and f"int {name}(" in header, name
        assert getattr(capi.lib(), name).argtypes
    assert "#define PQH_IVF_MAX_NPROBE 64" in header
    for name in ("Coarse", "IVF", "ivf_status"):
        assert callable(getattr(codec, name))
    for name in ("assign", "layout", "probe", "close"):
        assert callable(getattr(codec.Coarse, name))
    for name in ("build", "search", "fetch"):
        assert callable(getattr(codec.IVF, name))


PROBE = """
import ctypes
from pq_huffman_amd import capi
L = capi.lib()
cq = ctypes.c_void_p()
print(L.pqh_coarse_create(None, None, 4, 8, ctypes.byref(cq)),
      L.pqh_coarse_assign(None, None, None, 10, 8, None, None),
      L.pqh_ivf_layout(None, None, 10, 4, None, None),
      L.pqh_coarse_probe(None, None, None, 1, 8, 2, None, None, None, None, None),
      L.pqh_ivf_status(None),
      L.pqh_coarse_destroy(None))
"""


def test_ivf_calls_without_a_device():
    """the devices hidden: no context can exist, and every call that takes one says why
    (pqh_coarse_destroy takes none: destroying nothing is no error)"""
    env = dict(os.environ)
    env["HIP_VISIBLE_DEVICES"] = ""
    env["ROCR_VISIBLE_DEVICES"] = ""
    r = subprocess.run([sys.executable, "-c", PROBE], capture_output=True, text=True, env=env,
                       cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["-2", "-2", "-2", "-2", "-2", "0"], r.stdout + r.stderr


def test_reference_distances_are_exact_on_the_integer_grid():
    for n, d, nlist in ((63, 5, 70), (40, 130, 257), (7, 1, 3)):
        x, c = ivf_ref.integer_grid(n, d, nlist, seed=n + d)
        got = ivf_ref.dists(x, c)
        want = ivf_ref.dists_int64(x, c)
        assert got.dtype == np.float32 and want.max() < 2 ** 24
        assert np.array_equal(got.astype(np.int64), want)
        assert np.array_equal(got, want.astype(np.float32))
        lists, dist = ivf_ref.assign(x, c, got)
        assert lists.dtype == np.int32 and np.array_equal(dist.astype(np.int64), want.min(axis=1))
        # the first of the equal minima, and there are rows with several
        ties = (want == want.min(axis=1, keepdims=True)).sum(axis=1)
        first = np.array([np.flatnonzero(want[v] == want[v].min())[0] for v in range(n)])
        assert np.array_equal(lists, first)
        if d <= 5 and nlist >= 70:
            assert (ties > 1).any()


def test_reference_probe_order_and_padding():
    x, c = ivf_ref.integer_grid(9, 5, 70, seed=3)
    c[7] = c[3]
    offsets = np.arange(71, dtype=np.int64) * 3
    offsets[11] = offsets[10] - 1      # a reversed pair: list 10
    ptr, ranges, probes, dist = ivf_ref.probe(x, c, 64, offsets)
    d = ivf_ref.dists_int64(x, c)
    assert np.array_equal(ptr, np.arange(10) * 64)
    for q in range(9):
        key = sorted((d[q, l], l) for l in range(70))[:64]
        assert [l for _, l in key] == probes[q].tolist()
        assert [v for v, _ in key] == dist[q].astype(np.int64).tolist()
        at3 = probes[q].tolist().index(3) if 3 in probes[q] else None
        if at3 is not None and at3 < 63:
            assert probes[q, at3 + 1] == 7
        for p, l in enumerate(probes[q]):
            want = [0, 0] if l == 10 else [offsets[l], offsets[l + 1] - offsets[l]]
            assert ranges[q * 64 + p].tolist() == want
    ptr, ranges, probes, dist = ivf_ref.probe(x, c[:3], 5, np.array([0, 2, 2, 9], np.int64))
    assert (probes[:, 3:] == -1).all() and np.isinf(dist[:, 3:]).all()
    assert (ranges.reshape(9, 5, 2)[:, 3:] == 0).all()
    assert sorted(probes[0, :3].tolist()) == [0, 1, 2]


def test_reference_layout_equals_ivf_layout():
    import torch
    rng = np.random.default_rng(11)
    for n, nlist in ((1003, 70), (1, 3), (0, 5), (5000, 1030)):
        ids = rng.integers(0, nlist, size=n)
        if n > 100:
            ids[ids == 4] = 5               # an empty list in the middle
            ids[ids == nlist - 1] = 0       # and an empty last one
        perm, offsets = ivf_ref.layout(ids, nlist)
        tp, to = codec.ivf_layout(torch.from_numpy(ids.astype(np.int64)), nlist)
        assert perm.dtype == np.int64 and offsets.dtype == np.int64
        assert np.array_equal(perm, tp.numpy()) and np.array_equal(offsets, to.numpy())
