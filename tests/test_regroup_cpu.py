"""The regroup plan and the scatter without a GPU: the numpy reference (tests/regroup_ref.py)
against values worked out by hand on a six-list world, the properties every plan has, and the
interface -- the C entry points declared, exported and bound, their NULL-context rule, the new
methods of codec.IVF."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import regroup_ref as rg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------ by hand
def test_six_lists_without_a_mask():
    new_offsets, dest, add_base = rg.regroup(rg.SIX_OFFSETS)
    assert np.array_equal(new_offsets, rg.SIX_OFFSETS)
    assert np.array_equal(dest, np.arange(40))
    assert np.array_equal(add_base, rg.SIX_OFFSETS[1:])
    # 2, 0, 0, 3, 1, 0 new rows: every list moves up by the rows added before it
    new_offsets, dest, add_base = rg.regroup(rg.SIX_OFFSETS, None, rg.SIX_ADD)
    assert new_offsets.tolist() == [0, 5, 5, 12, 39, 40, 46]
    assert add_base.tolist() == [3, 5, 12, 36, 39, 46]
    assert dest[:3].tolist() == [0, 1, 2]
    assert dest[3:10].tolist() == list(range(5, 12))
    assert dest[10:34].tolist() == list(range(12, 36))
    assert dest[34:].tolist() == list(range(40, 46))
    assert rg.add_slots(rg.SIX_ADD, add_base).tolist() == [3, 4, 36, 37, 38, 39]


def test_six_lists_with_nothing_kept():
    new_offsets, dest, add_base = rg.regroup(rg.SIX_OFFSETS, rg.six_keep("zero"))
    assert not new_offsets.any() and not add_base.any() and (dest == -1).all()
    new_offsets, dest, add_base = rg.regroup(rg.SIX_OFFSETS, rg.six_keep("zero"), rg.SIX_ADD)
    assert np.array_equal(new_offsets, rg.SIX_ADD) and (dest == -1).all()
    assert np.array_equal(add_base, rg.SIX_ADD[:-1])


def test_six_lists_with_seven_rows_kept():
    """rows 1 | - | 3, 9 | 10, 33 | - | 34, 39 kept: a kept row on either side of the boundaries
    3 | 10 (word 0) and 34 (word 1)"""
    keep = rg.six_keep("hand")
    new_offsets, dest, add_base = rg.regroup(rg.SIX_OFFSETS, keep)
    assert new_offsets.tolist() == [0, 1, 1, 3, 5, 5, 7]
    assert add_base.tolist() == [1, 1, 3, 5, 5, 7]
    assert dest[list(rg.SIX_KEPT)].tolist() == [0, 1, 2, 3, 4, 5, 6]
    assert (np.delete(dest, rg.SIX_KEPT) == -1).all()
    new_offsets, dest, add_base = rg.regroup(rg.SIX_OFFSETS, keep, rg.SIX_ADD)
    assert new_offsets.tolist() == [0, 3, 3, 5, 10, 11, 13]
    assert add_base.tolist() == [1, 3, 5, 7, 10, 13]
    assert dest[list(rg.SIX_KEPT)].tolist() == [0, 3, 4, 5, 6, 11, 12]
    assert rg.add_slots(rg.SIX_ADD, add_base).tolist() == [1, 2, 7, 8, 9, 10]


def test_pack_is_the_mask_format():
    keep = rg.six_keep("hand")
    words = rg.pack(keep)
    assert words.dtype == np.uint32 and words.tolist() == [
        (1 << 1) | (1 << 3) | (1 << 9) | (1 << 10), (1 << 1) | (1 << 2) | (1 << 7)]
    assert rg.pack(np.zeros(0, bool)).shape == (0,) and rg.pack(np.ones(33, bool)).tolist() == [0xFFFFFFFF, 1]


# ------------------------------------------------------------------------------ properties
def _worlds():
    yield rg.SIX_OFFSETS, rg.SIX_ADD
    rng = np.random.default_rng(11)
    for nlist, n, n_add in ((1, 0, 4), (1, 63, 0), (13, 1003, 300), (1030, 1003, 77), (7, 0, 0)):
        cuts = np.sort(rng.integers(0, n + 1, size=nlist - 1))
        acuts = np.sort(rng.integers(0, n_add + 1, size=nlist - 1))
        yield (np.concatenate([[0], cuts, [n]]).astype(np.int64),
               np.concatenate([[0], acuts, [n_add]]).astype(np.int64))


@pytest.mark.parametrize("kind", ["none", "zero", "random"])
@pytest.mark.parametrize("with_add", [False, True])
def test_plan_is_an_order_preserving_bijection(kind, with_add):
    """dest on the kept rows, followed by the add slots, maps one to one onto
    [0, new_offsets[nlist]); a list's kept rows keep their order and come before its new ones"""
    for wi, (offsets, add_offsets) in enumerate(_worlds()):
        n, nlist = int(offsets[-1]), len(offsets) - 1
        keep = {"none": None, "zero": np.zeros(n, bool),
                "random": np.random.default_rng(100 + wi).random(n) < 0.6}[kind]
        add = add_offsets if with_add else None
        new_offsets, dest, add_base = rg.regroup(offsets, keep, add)
        kept = np.ones(n, bool) if keep is None else keep
        assert ((dest >= 0) == kept).all()
        slots = rg.add_slots(add_offsets, add_base) if with_add else np.zeros(0, np.int64)
        both = np.concatenate([dest[kept], slots])
        assert np.array_equal(np.sort(both), np.arange(new_offsets[-1])), wi
        assert new_offsets[0] == 0 and (np.diff(new_offsets) >= 0).all()
        for l in range(nlist):
            mine = dest[offsets[l]:offsets[l + 1]]
            mine = mine[mine >= 0]
            assert np.array_equal(mine, np.arange(new_offsets[l], add_base[l])), (wi, l)
            gap = add_offsets[l + 1] - add_offsets[l] if with_add else 0
            assert new_offsets[l + 1] - add_base[l] == gap, (wi, l)


def test_scatter_reference():
    codes = np.arange(40 * 3, dtype=np.uint8).reshape(40, 3)
    _, dest, _ = rg.regroup(rg.SIX_OFFSETS, rg.six_keep("hand"), rg.SIX_ADD)
    out = rg.scatter(codes, dest, np.full((13, 3), 0xEE, np.uint8))
    assert np.array_equal(out[[0, 3, 4, 5, 6, 11, 12]], codes[list(rg.SIX_KEPT)])
    assert (out[[1, 2, 7, 8, 9, 10]] == 0xEE).all()                   # the gaps are not written
    # destinations outside the output are passed over
    out = rg.scatter(codes[:3], np.array([-2, 5, 1]), np.full((5, 3), 0xEE, np.uint8))
    assert np.array_equal(out[1], codes[2]) and (np.delete(out, 1, axis=0) == 0xEE).all()


# ------------------------------------------------------------------------------ the interface
def test_entry_points_are_declared_exported_and_bound():
    from pq_huffman_amd import capi
    header = open(os.path.join(ROOT, "include", "pqh.h")).read()
    bound = {name: args for name, _, args in capi.SIGNATURES}
    for name in ("pqh_ivf_regroup", "pqh_decode_scatter"):
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert decl, name
        args = re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S)
        assert len(bound[name]) == args.count(",") + 1, name
        assert hasattr(capi.lib(), name)
    # the stream and index arguments of pqh_decode_select, then the map, the output, its rows
    assert len(bound["pqh_decode_scatter"]) == len(bound["pqh_decode_select"])
    assert bound["pqh_decode_scatter"][:9] == bound["pqh_decode_select"][:9]
    makefile = open(os.path.join(ROOT, "pq_huffman_amd", "csrc", "Makefile")).read()
    assert re.search(r"^HIP_SRC\s*:=.*\bpqh_regroup\.hip\b", makefile, flags=re.M)


def test_null_context_is_refused_first():
    from pq_huffman_amd import capi
    lib = capi.lib()
    n = ctypes.c_int(0)
    lib.pqh_device_count(ctypes.byref(n))
    want = -1 if n.value > 0 else -2
    assert lib.pqh_ivf_regroup(None, None, -3, -5, None, None, None, None, None) == want
    assert lib.pqh_decode_scatter(None, None, None, 0, -5, 0, 0, None, None, None, None, -1) == want


def test_codec_has_the_new_calls():
    from pq_huffman_amd import codec
    assert list(inspect.signature(codec.IVF.add).parameters) == ["self", "x"]
    assert list(inspect.signature(codec.IVF.compact).parameters) == ["self"]
    assert inspect.signature(codec.IVF.add).return_annotation in (int, "int")
    assert inspect.signature(codec.IVF.compact).return_annotation in (int, "int")
    p = inspect.signature(codec.ivf_regroup).parameters
    assert list(p)[:4] == ["ctx", "offsets", "keep", "add_offsets"]
    assert p["keep"].default is None and p["add_offsets"].default is None
    assert list(inspect.signature(codec.decode_scatter).parameters) == [
        "ctx", "tables", "enc", "dest", "out"]
    for text in (codec.IVF.add.__doc__, codec.IVF.compact.__doc__):
        assert "O(n" in text
