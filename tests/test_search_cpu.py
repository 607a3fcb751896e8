"""Host-side parts of the ADC search (pqh_adc_tables, pqh_search_stream, pqh_search_codes):
the calls are exported, declared and bound, and a process that sees no GPU gets
PQH_ERR_NO_DEVICE from each of them (pqh.h: that check comes before every argument check)."""
import os
import subprocess
import sys

from conftest import ROOT
from pq_huffman_amd import capi, codec

NEW_CALLS = ["pqh_adc_tables", "pqh_search_stream", "pqh_search_codes"]


def test_search_calls_are_exported_declared_and_bound():
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    header = open(os.path.join(ROOT, "include", "pqh.h")).read()
    bound = {name for name, _, _ in capi.SIGNATURES}
    for name in NEW_CALLS:
        assert name in exported and name in bound and f"int {name}(" in header, name
        assert getattr(capi.lib(), name).argtypes
    assert "#define PQH_SEARCH_MAX_K 64" in header
    assert "PQH_TUNE_SEARCH_GROUPS = 5" in header
    for fn in ("adc_tables", "search", "search_codes"):
        assert callable(getattr(codec, fn))
    assert codec.Context.TUNE["search_groups"] == 5


PROBE = """
from pq_huffman_amd import capi
L = capi.lib()
print(L.pqh_adc_tables(None, None, None, 3, 128, None),
      L.pqh_search_stream(None, None, None, 0, 10, 1, 4, None, None, None, 1, 10, 0, None, None),
      L.pqh_search_codes(None, None, 10, 8, 256, None, 1, 10, 0, None, None))
"""


def test_search_calls_without_a_device():
    """the devices hidden: no context can exist, and every call says why"""
    env = dict(os.environ)
    env["HIP_VISIBLE_DEVICES"] = ""
    env["ROCR_VISIBLE_DEVICES"] = ""
    r = subprocess.run([sys.executable, "-c", PROBE], capture_output=True, text=True, env=env,
                       cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["-2", "-2", "-2"], r.stdout + r.stderr
