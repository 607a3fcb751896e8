"""Host-side parts of PQ assignment mode 2 (pqh_assign_screen.hip): the two new calls are
exported, declared and bound, and a NULL context is answered as pqh_pq_assign answers it."""
import ctypes
import os
import subprocess

from conftest import ROOT
from pq_huffman_amd import capi, codec

CALLS = ["pqh_pq_last_screen_counts", "pqh_kmeans_train_mode"]


def test_screen_calls_are_exported_declared_and_bound():
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    header = open(os.path.join(ROOT, "include", "pqh.h")).read()
    bound = {name for name, _, _ in capi.SIGNATURES}
    for name in CALLS:
        assert name in exported and name in bound and f"int {name}(" in header, name
        assert getattr(capi.lib(), name).argtypes
    assert callable(codec.PQ.screen_counts)


def test_a_null_context_is_answered_as_the_assignment_answers_it():
    L = capi.lib()
    want = L.pqh_pq_assign(None, None, None, 10, 8, None, None, 2)
    assert want < 0
    a, b = ctypes.c_ulonglong(), ctypes.c_ulonglong()
    assert L.pqh_pq_last_screen_counts(None, ctypes.byref(a), ctypes.byref(b)) == want
    assert L.pqh_kmeans_train_mode(None, None, 10, 8, 1, 4, 8, 1, None, 2) == want
