"""Host-side parts of the probe search (pqh_search_stream_ranges, pqh_search_codes_ranges):
the calls are exported, declared and bound, a process that sees no GPU gets PQH_ERR_NO_DEVICE
from each of them, and the two torch helpers that lead from a list id per row to a probe list
(codec.ivf_layout, codec.probe_ranges) equal numpy on CPU tensors."""
import os
import subprocess
import sys

import numpy as np

from conftest import ROOT
from pq_huffman_amd import capi, codec

NEW_CALLS = ["pqh_search_stream_ranges", "pqh_search_codes_ranges"]


def test_range_calls_are_exported_declared_and_bound():
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    header = open(os.path.join(ROOT, "include", "pqh.h")).read()
    bound = {name for name, _, _ in capi.SIGNATURES}
    for name in NEW_CALLS:
        assert name in exported and name in bound and f"int {name}(" in header, name
        assert getattr(capi.lib(), name).argtypes
    for fn in ("search_ranges", "search_codes_ranges", "ivf_layout", "probe_ranges"):
        assert callable(getattr(codec, fn))


PROBE = """
from pq_huffman_amd import capi
L = capi.lib()
print(L.pqh_search_stream_ranges(None, None, None, 0, 10, 1, 4, None, None, None, 1, None, None,
                                 1, 10, 0, None, None),
      L.pqh_search_codes_ranges(None, None, 10, 8, 256, None, 1, None, None, 1, 10, 0, None, None))
"""


def test_range_calls_without_a_device():
    """the devices hidden: no context can exist, and every call says why"""
    env = dict(os.environ)
    env["HIP_VISIBLE_DEVICES"] = ""
    env["ROCR_VISIBLE_DEVICES"] = ""
    r = subprocess.run([sys.executable, "-c", PROBE], capture_output=True, text=True, env=env,
                       cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["-2", "-2"], r.stdout + r.stderr


def test_ivf_layout_is_a_stable_sort_by_list():
    import torch
    rng = np.random.default_rng(11)
    nlist = 13
    ids = rng.integers(0, nlist, size=500)
    ids[ids == 4] = 5          # an empty list in the middle
    ids[ids == nlist - 1] = 0  # and an empty last one
    perm, offsets = codec.ivf_layout(torch.from_numpy(ids), nlist)
    assert perm.dtype == torch.int64 and offsets.dtype == torch.int64
    assert np.array_equal(perm.numpy(), np.argsort(ids, kind="stable"))
    want = np.zeros(nlist + 1, np.int64)
    want[1:] = np.cumsum(np.bincount(ids, minlength=nlist))
    assert np.array_equal(offsets.numpy(), want)
    assert want[4] == want[5] and want[-1] == want[-2] == 500
    # stream row s holds original row perm[s]: the lists come out contiguous
    by_list = ids[perm.numpy()]
    for l in range(nlist):
        assert (by_list[want[l]:want[l + 1]] == l).all()
    # no rows at all
    perm, offsets = codec.ivf_layout(torch.zeros(0, dtype=torch.int64), 3)
    assert perm.numel() == 0 and offsets.tolist() == [0, 0, 0, 0]


def test_probe_ranges_with_a_probe_of_nothing():
    import torch
    offsets = np.array([0, 7, 7, 30, 41], np.int64)
    probes = np.array([[2, 0, -1], [3, 3, 1], [-1, -1, -1]], np.int64)
    range_ptr, ranges = codec.probe_ranges(torch.from_numpy(offsets), torch.from_numpy(probes))
    assert range_ptr.dtype == torch.int64 and ranges.dtype == torch.int64
    assert np.array_equal(range_ptr.numpy(), np.arange(4) * 3)
    want = np.zeros((9, 2), np.int64)
    for i, l in enumerate(probes.reshape(-1)):
        if l >= 0:
            want[i] = offsets[l], offsets[l + 1] - offsets[l]
    assert np.array_equal(ranges.numpy(), want)
    assert ranges.is_contiguous() and tuple(ranges.shape) == (9, 2)
    assert want[2].tolist() == [0, 0] and want[5].tolist() == [7, 0]
