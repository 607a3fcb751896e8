"""Host-side parts of the screened coarse assignment (pqh_coarse_assign_screen*): the calls are
exported, declared and bound, a NULL context is answered as pqh_coarse_assign answers it, and an
unknown method is refused before anything is launched."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT
from pq_huffman_amd import capi, codec

CALLS = ["pqh_coarse_assign_screen", "pqh_coarse_assign_screen_ip", "pqh_coarse_last_screen_counts"]


def test_screen_calls_are_exported_declared_and_bound():
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    header = open(os.path.join(ROOT, "include", "pqh.h")).read()
    bound = {name for name, _, _ in capi.SIGNATURES}
    for name in CALLS:
        assert name in exported and name in bound and f"int {name}(" in header, name
        assert getattr(capi.lib(), name).argtypes
    assert callable(codec.Coarse.screen_counts)


def test_a_null_context_is_answered_as_the_direct_call_answers_it():
    L = capi.lib()
    args = (None, None, None, 10, 8, None, None)
    assert L.pqh_coarse_assign_screen(*args) == L.pqh_coarse_assign(*args) < 0
    assert L.pqh_coarse_assign_screen_ip(*args) == L.pqh_coarse_assign_ip(*args) < 0
    a, b = ctypes.c_ulonglong(), ctypes.c_ulonglong()
    assert L.pqh_coarse_last_screen_counts(None, ctypes.byref(a), ctypes.byref(b)) == \
        L.pqh_coarse_assign(*args)


def test_an_unknown_method_is_a_value_error():
    coarse = object.__new__(codec.Coarse)   # no context: the method is checked first
    with pytest.raises(ValueError):
        coarse.assign(None, method="nonsense")
    with pytest.raises(ValueError):
        codec.IVF.build(None, None, coarse, None, assign="nonsense")
