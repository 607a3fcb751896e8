"""Host-side parts of the random-access decode: huffman_decoder --rows is checked before any
device call, and the new entry points are exported, declared and bound."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from pq_huffman_amd import capi, codec

DECODER = os.path.join(ROOT, "pq_huffman_amd", "bin", "huffman_decoder")
NEW_CALLS = ["pqh_decode_select", "pqh_decode_range", "pqh_fetch_vectors",
             "pqh_decode_files_range"]


def _no_gpu_env():
    env = dict(os.environ)
    env["HIP_VISIBLE_DEVICES"] = ""
    env["ROCR_VISIBLE_DEVICES"] = ""
    return env


@pytest.mark.parametrize("value", ["abc", "5", "-1:3", "0:0", "3:", ":4", "1:2x", "1:-2"])
def test_rows_flag_malformed_is_a_usage_error(tmp_path, value):
    r = subprocess.run([DECODER, str(tmp_path) + "/", "--rows", value], capture_output=True,
                       text=True, env=_no_gpu_env())
    assert r.returncode == 1
    assert "Usage:" in r.stderr and "--rows" in r.stderr


@pytest.mark.parametrize("value", ["10:1", "8:3", "0:11"])
def test_rows_flag_outside_the_file_is_a_usage_error(tmp_path, value):
    """the range is compared with the row count in the stream's header: no GPU, no other file"""
    (tmp_path / "huffman_indices.bin").write_bytes(np.uint64(10).tobytes() + b"\0" * 16)
    r = subprocess.run([DECODER, str(tmp_path) + "/", "--rows", value], capture_output=True,
                       text=True, env=_no_gpu_env())
    assert r.returncode == 1
    assert "Usage:" in r.stderr


def test_rows_flag_does_not_combine_with_tree_or_check(tmp_path):
    for extra in (["--tree"], ["--check-file", "x"]):
        r = subprocess.run([DECODER, str(tmp_path) + "/", "--rows", "0:1"] + extra,
                           capture_output=True, text=True, env=_no_gpu_env())
        assert r.returncode == 1 and "Usage:" in r.stderr


class _FakeLib:
    """records the destroy calls codec makes, in order"""

    def __init__(self):
        self.calls = []

    def pqh_ctx_destroy(self, p):
        self.calls.append("ctx")

    def pqh_tables_destroy(self, p):
        self.calls.append("tables")

    def pqh_pq_destroy(self, p):
        self.calls.append("pq")


@pytest.mark.parametrize("order", ["ctx_first", "ctx_last", "ctx_between"])
def test_context_is_destroyed_after_its_tables_and_pq(monkeypatch, order):
    """pqh_tables_destroy and pqh_pq_destroy synchronise the stream of the context the object
    was made with, so whatever order the Python objects are closed or finalised in (a garbage
    cycle's finalisers run in any order), the context goes last, once."""
    import ctypes
    fake = _FakeLib()
    monkeypatch.setattr(codec, "lib", lambda: fake)
    ctx = object.__new__(codec.Context)
    ctx._deps, ctx._closing, ctx.ptr = 0, False, ctypes.c_void_p(1)
    tabs = object.__new__(codec.Tables)
    tabs.ctx, tabs.ptr = ctx, ctypes.c_void_p(2)
    ctx._retain()
    pq = object.__new__(codec.PQ)
    pq.ctx, pq.ptr = ctx, ctypes.c_void_p(3)
    ctx._retain()
    seq = {"ctx_first": [ctx, tabs, pq], "ctx_last": [pq, tabs, ctx],
           "ctx_between": [tabs, ctx, pq]}[order]
    for obj in seq:
        obj.__del__()
    for obj in seq:     # a second close of anything does nothing
        obj.close()
    assert sorted(fake.calls[:2]) == ["pq", "tables"] and fake.calls[2:] == ["ctx"]
    assert not ctx.ptr and not tabs.ptr and not pq.ptr


def test_new_calls_are_exported_declared_and_bound():
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    header = open(os.path.join(ROOT, "include", "pqh.h")).read()
    bound = {name for name, _, _ in capi.SIGNATURES}
    for name in NEW_CALLS:
        assert name in exported and name in bound and f"int {name}(" in header, name
        assert getattr(capi.lib(), name).argtypes
    for fn in ("decode_rows", "decode_range", "fetch"):
        assert callable(getattr(codec, fn))
