"""The flat range search without a GPU: its five calls are declared in pqh.h, exported by the
library and bound, and codec.Flat.range_search has the documented signature."""
import inspect

from pq_huffman_amd import capi, codec
from test_clib_cpu import _declared_functions

NAMES = {"pqh_flat_range_plan_bytes", "pqh_flat_range_count", "pqh_flat_range_count_ip",
         "pqh_flat_range_fill", "pqh_flat_range_fill_ip"}


def test_declared_exported_and_bound():
    assert NAMES <= _declared_functions()
    assert NAMES <= {n for n, _, _ in capi.SIGNATURES}
    for name in NAMES:
        assert getattr(capi.lib(), name).argtypes   # (a missing export raises here)


def test_python_signature():
    p = inspect.signature(codec.Flat.range_search).parameters
    assert list(p) == ["self", "queries", "radius", "metric", "keep", "id_base", "capacity"]
    assert (p["metric"].default, p["keep"].default, p["id_base"].default,
            p["capacity"].default) == ("l2", None, 0, None)
