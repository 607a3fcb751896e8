"""The Elias-Fano id map without a GPU: the numpy statement (tests/idmap_ref.py) against perm
itself, the size formula of the library (host arithmetic) against it and against the bound that
follows from the coding, the invariant the coding rests on -- the ids of a list ascend, after
every build, add and compact -- on the numpy mirrors of those steps, and the interface."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import idmap_ref as ref
import ivf_ref
import regroup_ref as rg
from conftest import ROOT

# (n, n_ids, nlist) of the size checks: the documented sizes, the edges, and the widest fields
SIZES = [(1_000_000, 1_000_000, 1024), (65_536, 65_536, 256), (10_000_000, 11_000_000, 4096),
         (300, 300, 1), (257, 257, 4), (1000, 4000, 7), (1, 1, 1), (0, 0, 1), (0, 500, 9),
         (1000, 2 ** 31 - 1, 65_535), (16, 2 ** 20, 2 ** 24), (16, 2 ** 31 - 1, 2 ** 24),
         (1, 2 ** 31 - 1, 2 ** 24), (63, 63, 3), (64, 64, 3), (255, 255, 3), (256, 256, 3)]


def layouts():
    out = {f"n{n}": ref.random_layout(n, n, 5, seed=n) for n in (1, 63, 64, 255, 256, 257, 1000)}
    out["empty"] = (np.zeros(0, np.int64), np.zeros(4, np.int64), 0)
    out["identity"] = ref.identity(300)
    out["seven"] = ref.random_layout(1000, 1000, 7, seed=7, empty=(0, 3, 6))
    out["last_list"] = ref.last_list()
    out["two_ends"] = ref.two_ends()
    out["two_ends_wide"] = ref.two_ends(last=4000)
    out["compacted"] = ref.random_layout(1000, 4000, 13, seed=8)
    out["wide40"] = ref.random_layout(16, 2 ** 20, 2 ** 24, seed=9)
    return out


LAYOUTS = layouts()


# ------------------------------------------------------------------------------ the numpy form
@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_round_trip(name):
    perm, offsets, n_ids = LAYOUTS[name]
    n = len(perm)
    blob = ref.build(perm, offsets, n_ids)
    assert len(blob) == ref.idmap_bytes(n, n_ids, len(offsets) - 1)
    assert np.array_equal(ref.decode(blob), perm)
    rng = np.random.default_rng(1)
    rows = np.concatenate([rng.integers(0, max(n, 1), 50) if n else np.zeros(0, np.int64),
                           np.array([-1, -7, n, n + 5])]).astype(np.int64)
    want = np.where(rows < 0, rows, np.where(rows < n, np.append(perm, 0)[np.clip(rows, 0, n)], -1))
    assert np.array_equal(ref.ids(blob, rows), want)
    # the reverse search: every row back, and ids the map does not hold
    assert np.array_equal(ref.rows(blob, offsets, perm), np.arange(n))
    absent = np.setdiff1d(np.arange(min(n_ids, 5000)), perm)[:20]
    probe = np.concatenate([absent, [-1, n_ids, n_ids + 9]]).astype(np.int64)
    assert (ref.rows(blob, offsets, probe) == -1).all()
    if n_ids <= 5000:
        keep = rng.random(n_ids) < 0.5
        assert np.array_equal(ref.pack_mask(blob, keep), rg.pack(keep[perm]))


def test_shapes_take_the_paths_they_are_for():
    s = lambda name: ref.shape(len(LAYOUTS[name][0]), LAYOUTS[name][2], len(LAYOUTS[name][1]) - 1)
    assert s("identity")["L"] == 0 and s("identity")["low_words"] == 0
    assert s("wide40")["L"] == 40 and s("wide40")["rev_size"] == 4
    assert ref.shape(16, 2 ** 31 - 1, 2 ** 24, reverse=False)["L"] == 51
    assert ref.shape(1, 2 ** 31 - 1, 2 ** 24, reverse=False)["L"] == 55
    assert ref.shape(1000, 2 ** 31 - 1, 65_535, reverse=False)["L"] == 37
    # the gap between the first and the last list lies inside block 0, and the block's span of
    # high-bit words is longer than the 64 a wave reads in one step
    # (with 150 rows in each the whole high part is 15 words; 150 and 4,000 rows give the span)
    assert ref.decode_span_words(ref.build(*ref.two_ends()), 0) > 8
    assert ref.decode_span_words(ref.build(*ref.two_ends(last=4000)), 0) > 64
    assert ref.decode_span_words(ref.build(*LAYOUTS["n1000"]), 0) <= 64


def test_without_the_reverse_part():
    perm, offsets, n_ids = LAYOUTS["n257"]
    full, bare = ref.build(perm, offsets, n_ids), ref.build(perm, offsets, n_ids, reverse=False)
    assert len(bare) < len(full) and np.array_equal(ref.decode(bare), perm)
    assert ref.View(bare).rev is None
    perm, offsets, n_ids = ref.random_layout(16, 2 ** 31 - 1, 2 ** 24, seed=10)
    blob = ref.build(perm, offsets, n_ids, reverse=False)
    assert ref.View(blob).L == 51 and np.array_equal(ref.decode(blob), perm)


def test_build_refuses_what_it_cannot_code():
    perm, offsets, n_ids = ref.identity(10)
    for bad in ([0, 1, 2, 3, 3, 5, 6, 7, 8, 9], [0, 1, 2, 4, 3, 5, 6, 7, 8, 9]):
        with pytest.raises(AssertionError):
            ref.build(np.array(bad, np.int64), offsets, n_ids)


# ------------------------------------------------------------------------------ the size
@pytest.mark.parametrize("n,n_ids,nlist", SIZES)
def test_size_formula_and_bound(n, n_ids, nlist):
    from pq_huffman_amd import codec
    for reverse in (True, False):
        assert codec.idmap_bytes(n, n_ids, nlist, reverse) == ref.idmap_bytes(n, n_ids, nlist, reverse)
    s = ref.shape(n, n_ids, nlist, reverse=False)
    assert s["high_bits"] < 3 * n + 1
    assert s["L"] <= 55
    # Elias-Fano: L low bits and fewer than 3 high bits a row, 8 bytes of sample per 256 rows
    assert s["words"] * 8 <= n * (s["L"] + 3) / 8 + n / 32 + 4096


def test_derived_sizes_of_the_documents():
    from pq_huffman_amd import codec
    n = 1_000_000
    assert ref.shape(n, n, 1024)["L"] == 10
    assert abs(codec.idmap_bytes(n, n, 1024, reverse=False) / n - 1.53) < 0.01
    assert abs(codec.idmap_bytes(n, n, 1024) / n - 3.53) < 0.01
    # 10M rows of 11M ids in 4,096 lists: B = 24, L = 12, 2^24 + 10M high bits, 2 B an id of
    # reverse part -- 3.70 B an id (an estimate of 3.99 was made before the format was fixed)
    s = ref.shape(10_000_000, 11_000_000, 4096)
    assert (s["B"], s["L"], s["high_bits"]) == (24, 12, 2 ** 24 + 10_000_000 - 1)
    per_id = codec.idmap_bytes(10_000_000, 11_000_000, 4096) / 11_000_000
    assert abs(per_id - 3.70) < 0.01 and per_id < 3.99


def test_size_arguments():
    from pq_huffman_amd import capi
    out = ctypes.c_ulonglong(0)
    f = capi.lib().pqh_idmap_bytes
    assert f(5, 4, 1, 1, ctypes.byref(out)) == -1          # more rows than ids
    assert f(-1, 4, 1, 1, ctypes.byref(out)) == -1
    assert f(1, 4, 0, 1, ctypes.byref(out)) == -1
    assert f(1, 4, 1, 1, None) == -1
    assert f(1, 2 ** 31, 1, 1, ctypes.byref(out)) == -4
    assert f(1, 4, 2 ** 24 + 1, 1, ctypes.byref(out)) == -4
    assert f(0, 0, 1, 1, ctypes.byref(out)) == 0 and out.value == 128    # the header alone


# ------------------------------------------------------------------------------ the invariant
def _ascending_in_every_list(perm, offsets):
    return all((np.diff(perm[offsets[l]:offsets[l + 1]]) > 0).all() for l in range(len(offsets) - 1))


def test_ids_ascend_in_every_list_through_the_life_of_an_index():
    """build, add, remove + compact, add -- each step as the numpy mirrors state it (ivf_ref.layout,
    regroup_ref.regroup / add_slots, and IVF.add's ids n_ids ... for the new rows)"""
    rng = np.random.default_rng(11)
    nlist = 9
    lists = rng.integers(0, nlist, 500)
    lists[lists == 4] = 5                                   # an empty list
    perm, offsets = ivf_ref.layout(lists, nlist)
    n_ids = 500
    assert _ascending_in_every_list(perm, offsets)

    def add(perm, offsets, n_ids, count, seed):
        b_lists = np.random.default_rng(seed).integers(0, nlist, count)
        b_perm, b_offsets = ivf_ref.layout(b_lists, nlist)
        new_offsets, dest, add_base = rg.regroup(offsets, None, b_offsets)
        out = np.full(len(perm) + count, -1, np.int64)
        out[dest] = perm
        out[rg.add_slots(b_offsets, add_base)] = b_perm + n_ids
        assert (out >= 0).all()
        return out, new_offsets, n_ids + count

    def compact(perm, offsets, gone):
        live = ~np.isin(perm, gone)
        new_offsets, dest, _ = rg.regroup(offsets, live, None)
        out = np.empty(int(live.sum()), np.int64)
        out[dest[live]] = perm[live]
        return out, new_offsets

    perm, offsets, n_ids = add(perm, offsets, n_ids, 300, 12)
    assert _ascending_in_every_list(perm, offsets)
    perm, offsets = compact(perm, offsets, rng.choice(n_ids, 250, replace=False))
    assert _ascending_in_every_list(perm, offsets) and len(perm) == 550
    perm, offsets, n_ids = add(perm, offsets, n_ids, 120, 13)
    assert _ascending_in_every_list(perm, offsets) and n_ids == 920
    # ... and so the map codes it
    assert np.array_equal(ref.decode(ref.build(perm, offsets, n_ids)), perm)


# ------------------------------------------------------------------------------ the interface
CALLS = ("pqh_idmap_bytes", "pqh_idmap_build", "pqh_idmap_ids", "pqh_idmap_decode",
         "pqh_idmap_rows", "pqh_mask_pack_idmap")


def test_entry_points_are_declared_exported_and_bound():
    from pq_huffman_amd import capi
    header = open(os.path.join(ROOT, "include", "pqh.h")).read()
    bound = {name: args for name, _, args in capi.SIGNATURES}
    for name in CALLS:
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert decl, name
        args = re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S)
        assert len(bound[name]) == args.count(",") + 1, name
        assert hasattr(capi.lib(), name)
    makefile = open(os.path.join(ROOT, "pq_huffman_amd", "csrc", "Makefile")).read()
    assert re.search(r"^HIP_SRC\s*:=.*\bpqh_idmap\.hip\b", makefile, flags=re.M)


def test_null_context_is_refused_first():
    from pq_huffman_amd import capi
    lib = capi.lib()
    n = ctypes.c_int(0)
    lib.pqh_device_count(ctypes.byref(n))
    want = -1 if n.value > 0 else -2
    assert lib.pqh_idmap_build(None, None, None, -1, 0, -1, 1, None, 0) == want
    assert lib.pqh_idmap_ids(None, None, None, -1, None) == want
    assert lib.pqh_idmap_decode(None, None, -1, -1, None) == want
    assert lib.pqh_idmap_rows(None, None, None, None, -1, None) == want
    assert lib.pqh_mask_pack_idmap(None, None, None, -1, None) == want


def test_codec_has_the_new_names():
    from pq_huffman_amd import codec
    assert list(inspect.signature(codec.IdMap.__init__).parameters) == [
        "self", "ctx", "perm", "offsets", "n_ids", "reverse"]
    assert inspect.signature(codec.IdMap.__init__).parameters["reverse"].default is True
    for name in ("ids", "rows", "decode", "pack_mask"):
        assert callable(getattr(codec.IdMap, name))
    assert list(inspect.signature(codec.idmap_bytes).parameters) == ["n", "n_ids", "nlist", "reverse"]
    assert inspect.signature(codec.IVF.build).parameters["compress_ids"].default is False
    assert callable(codec.IVF.compress_ids) and callable(codec.IVF.id_bytes)
