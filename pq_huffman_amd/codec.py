"""Python mirror of the reference's encode/decode flow over the pqh C ABI.

The reference pipeline is pq_encoder -> huffman_encoder ->
huffman_decoder, gluing CLI programs through files.  Here the same stages run as C-ABI
calls on device-resident data:

    PQ.assign            pq_encoder.c:270-272 (yael kmeans assignment) + :192-205
    kmeans_train         pq_encoder.c:265-274 (training, deterministic Lloyd on the GPU)
    sort_rows            huffman_encoder.c:301-317 (default sort mode)
    histogram            huffman_encoder.c:139-205
    build_codebooks      huffman_encoder.c:377-388 (huffman_codebook_[context_]encode_init)
    encode               huffman_encoder.c:413-428 (+ sidecar chunk index)
    decode               huffman_decoder.c:206-255
    search               ADC top-k over the stream, fused into the decoder (no reference analogue)
    search_ranges        the same over per-query row ranges: the probe search of an inverted file
    Coarse, IVF          the front end of that search: rows to lists, the list layout, each
                         query's probe list, and the whole path from vectors to neighbour ids
    search_range_tables  the probe search with one table per (query, list): the residual form
                         of the inverted file (Coarse.residuals, adc_tables_residual,
                         IVF.build(residual=True))
    search_lists         the probe search in list-major order: a list decoded once per batch of
                         the queries that probe it (IVF.search(schedule="list"))
    pack_mask, keep=     filtered search: a bit per stream row, rows and chunks that are not kept
                         are not decoded (IVF.search(keep=...), IVF.remove)
    refine, pq_residuals a second, finer code of what the first quantizer left over, as a stream
                         of its own, and the fused re-rank of a search's candidates with both
                         (IVF.build(refine_pq=...), IVF.search(refine=64), IVF.fetch(refined=True))
    ivf_regroup, decode_scatter  a list-ordered stream taken to a new list order, rows dropped
                         and gaps left for new rows: an index that grows and shrinks
                         (IVF.add, IVF.compact)
    IdMap, idmap_bytes   an index's ids in Elias-Fano form in place of the int64 perm and inv:
                         rows to ids, ids to rows, a row range, and pack_mask through the map
                         (IVF.build(compress_ids=True), IVF.compress_ids)
    Rotation, opq_train  a learned rotation in front of the quantizers (OPQ): the map itself,
                         the exact sums X^T Y its training needs (cross_moments), the Procrustes
                         step and the PCA start on the host (IVF.build(rotation=...))

torch is used only for device memory and the stream (data_ptr / cuda_stream); every
computation is a libpqh kernel, but for the index bookkeeping of ivf_layout and probe_ranges
(a sort and gathers of int64 in plain torch; Coarse.layout and Coarse.probe are their libpqh
forms), IVF's gathers through its permutation and the indexed stores of IVF.add / IVF.compact
(the new rows' codes into their gaps, perm, inv and the live flags), the centroid a residual IVF's fetch adds
back and the subtract of pq_residuals (one torch add or sub_ each, not a hot path).  Device buffers are torch tensors owned by
the caller.
"""
from __future__ import annotations

import ctypes
import os
import tempfile
from dataclasses import dataclass

import numpy as np

from .capi import (EncodeOptions, HuffmanCodebook, PqhError, check, lib)

_libc = ctypes.CDLL(None)
_libc.fopen.restype = ctypes.c_void_p
_libc.fopen.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
_libc.fclose.argtypes = [ctypes.c_void_p]
_libc.fwrite.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]
_libc.fseek.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_int]


def _ptr(t):
    """device/host pointer of a torch tensor or numpy array (None -> NULL)."""
    if t is None:
        return None
    if isinstance(t, np.ndarray):
        return t.ctypes.data_as(ctypes.c_void_p)
    return ctypes.c_void_p(t.data_ptr())


def _torch():
    import torch
    return torch


def device_count() -> int:
    n = ctypes.c_int(0)
    lib().pqh_device_count(ctypes.byref(n))
    return n.value


class Context:
    """pqh_ctx_t bound to a torch device and a stream (pqh.h).

    Default: torch's current stream, so torch's fills and copies are ordered with the pqh
    kernels.  cus > 0: the context keeps its own stream limited to that many compute units
    (pqh_ctx_create_cu_split), or with complement=True to all the OTHER compute units;
    `stream` is then a torch.cuda.ExternalStream over it."""

    def __init__(self, device: int = 0, stream=None, cus: int = 0, complement: bool = False):
        torch = _torch()
        # Tables and PQ objects free their device memory through the context they were made
        # with (pqh_tables_destroy / pqh_pq_destroy synchronise its stream), so the context
        # is destroyed only after the last of them: close() waits for _deps to reach 0.
        # Finalisers of a garbage cycle run in any order; this keeps that order harmless.
        self._deps = 0
        self._closing = False
        self.device = device
        torch.cuda.set_device(device)
        self.ptr = ctypes.c_void_p()
        if cus != 0:   # (< 0: all CUs on a CU-masked stream, a hardware queue of its own)
            check(lib().pqh_ctx_create_cu_split(ctypes.byref(self.ptr), device, cus,
                                                int(complement)), "pqh_ctx_create_cu_split")
            self.stream = torch.cuda.ExternalStream(lib().pqh_ctx_stream(self.ptr), device=device)
            return
        self.stream = stream or torch.cuda.current_stream(device)
        check(lib().pqh_ctx_create(ctypes.byref(self.ptr), device), "pqh_ctx_create")
        # bind to torch's stream (often the NULL/default stream) so torch's allocations,
        # fills and copies are ordered with the pqh kernels
        check(lib().pqh_ctx_set_stream(self.ptr, ctypes.c_void_p(self.stream.cuda_stream)),
              "pqh_ctx_set_stream")

    def set_stream(self, stream) -> None:
        self.stream = stream
        check(lib().pqh_ctx_set_stream(self.ptr, ctypes.c_void_p(stream.cuda_stream)))

    TUNE = {"assign_wgs_per_cu": 1, "hist_split": 2, "hist_block": 3, "enc_impl": 4,
            "search_groups": 5}

    def set_tuning(self, **kw) -> "Context":
        """launch shapes of this context's kernels (pqh_ctx_set_tuning; results never
        change): assign_wgs_per_cu, hist_split, hist_block, enc_impl (1 tiled, 2 one-pass),
        search_groups (workgroups per query batch of the ADC scan) -- 0 restores the default"""
        for key, value in kw.items():
            check(lib().pqh_ctx_set_tuning(self.ptr, self.TUNE[key], float(value)),
                  f"pqh_ctx_set_tuning({key})")
        return self

    def set_search_max_k(self, max_k: int) -> "Context":
        """the largest k of the searches and candidate count of refine() this context accepts
        (pqh_ctx_set_search_max_k): 64 for a new context, up to 256.  Calls with k <= 64 run
        the same kernels whatever the limit; above 64 the scans keep a list of 256 a wave."""
        check(lib().pqh_ctx_set_search_max_k(self.ptr, int(max_k)), "pqh_ctx_set_search_max_k")
        return self

    @property
    def search_max_k(self) -> int:
        limit = lib().pqh_ctx_search_max_k(self.ptr)
        if limit < 0:
            raise PqhError(limit, "pqh_ctx_search_max_k")
        return limit

    def sync(self) -> None:
        check(lib().pqh_ctx_sync(self.ptr), "pqh_ctx_sync")

    def release_scratch(self) -> None:
        """free the context's grow-only device scratch (pqh_ctx_release_scratch)"""
        check(lib().pqh_ctx_release_scratch(self.ptr), "pqh_ctx_release_scratch")

    def last_error(self) -> str:
        return (lib().pqh_ctx_last_error(self.ptr) or b"").decode()

    def _retain(self) -> None:
        self._deps += 1

    def _release(self) -> None:
        self._deps -= 1
        if self._closing and self._deps <= 0:
            self.close()

    def close(self) -> None:
        if self._deps > 0:      # destroyed when the last Tables / PQ made with it closes
            self._closing = True
            return
        if self.ptr:
            lib().pqh_ctx_destroy(self.ptr)
            self.ptr = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PQ:
    """Prepared sub-codebooks on the device (pq.h centroids_codebook_t + MFMA fragments)."""

    def __init__(self, ctx: Context, centroids: np.ndarray):
        c = np.ascontiguousarray(centroids, np.float32)
        self.m, self.k, self.dsub = c.shape
        self.ctx = ctx
        self.ptr = ctypes.c_void_p()
        check(lib().pqh_pq_create(ctx.ptr, _ptr(c), self.m, self.k, self.dsub,
                                  ctypes.byref(self.ptr)), "pqh_pq_create")
        ctx._retain()

    @property
    def code_dtype(self):
        torch = _torch()
        return torch.uint8 if self.k <= 256 else torch.int16

    def assign(self, x, codes=None, counts=None, mode: int = 0, ctx: Context = None):
        """codes (n, m) of x; on `ctx`'s stream (any context of the same device, default the
        one the codebook was prepared with)."""
        torch = _torch()
        n = x.shape[0]
        if codes is None:
            codes = torch.empty((n, self.m), dtype=self.code_dtype, device=x.device)
        c = ctx or self.ctx
        check(lib().pqh_pq_assign(c.ptr, self.ptr, _ptr(x), n, x.stride(0), _ptr(codes),
                                  _ptr(counts), mode), "pqh_pq_assign")
        return codes

    def assign_parts(self, x, parts=None, counts=None, mode: int = 0, ctx: Context = None):
        """codes of x PART-MAJOR: parts (m, >= n), part i's codes contiguous in parts[i]
        (pqh_pq_assign_parts: the kernel stores whole lines)."""
        torch = _torch()
        n = x.shape[0]
        if parts is None:   # (rows padded to 128 codes: whole-line stores, see the kernel)
            parts = torch.empty((self.m, (n + 127) // 128 * 128), dtype=self.code_dtype,
                                device=x.device)[:, :n]
        c = ctx or self.ctx
        check(lib().pqh_pq_assign_parts(c.ptr, self.ptr, _ptr(x), n, x.stride(0), _ptr(parts),
                                        parts.stride(0), _ptr(counts), mode),
              "pqh_pq_assign_parts")
        return parts

    def rerank_count(self, ctx: Context = None) -> int:
        v = ctypes.c_ulonglong(0)
        check(lib().pqh_pq_last_rerank_count((ctx or self.ctx).ptr, ctypes.byref(v)))
        return v.value

    def error(self, x, codes) -> float:
        v = ctypes.c_double(0)
        check(lib().pqh_pq_error(self.ctx.ptr, self.ptr, _ptr(x), x.shape[0], x.stride(0),
                                 _ptr(codes), ctypes.byref(v)), "pqh_pq_error")
        return v.value

    def reconstruct(self, codes):
        torch = _torch()
        out = torch.empty((codes.shape[0], self.m * self.dsub), dtype=torch.float32,
                          device=codes.device)
        check(lib().pqh_pq_reconstruct(self.ctx.ptr, self.ptr, _ptr(codes), codes.shape[0],
                                       _ptr(out), out.stride(0)), "pqh_pq_reconstruct")
        return out

    def close(self):
        if self.ptr:
            lib().pqh_pq_destroy(self.ptr)
            self.ptr = ctypes.c_void_p()
            self.ctx._release()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def kmeans_train(ctx: Context, x, init: np.ndarray, iters: int) -> np.ndarray:
    """Lloyd k-means of every subspace on the GPU (pqh_kmeans_train): exact assignment and
    fixed-point centroid means, deterministic; init [m][k][dsub] -> trained centroids."""
    cent = np.ascontiguousarray(init, np.float32).copy()
    m, k, ds = cent.shape
    check(lib().pqh_kmeans_train(ctx.ptr, _ptr(x), x.shape[0], x.stride(0), m, k, ds, iters,
                                 _ptr(cent)), "pqh_kmeans_train")
    return cent


class Codebooks:
    """m host codebooks (huffman.h huffman_codebook_t) built by the library."""

    def __init__(self, counts: np.ndarray, k: int, context: bool, threads: int = 0):
        counts = np.ascontiguousarray(counts, np.float64)
        self.m = counts.shape[0]
        self.k, self.context = k, bool(context)
        self.arr = (HuffmanCodebook * self.m)()
        check(lib().pqh_codebooks_build(_ptr(counts), self.m, k, int(context),
                                        ctypes.cast(self.arr, ctypes.c_void_p),
                                        threads or min(self.m, os.cpu_count() or 1)),
              "pqh_codebooks_build")
        self.counts = counts

    @classmethod
    def _empty(cls, m):
        obj = cls.__new__(cls)
        obj.m = m
        obj.arr = (HuffmanCodebook * m)()
        return obj

    @property
    def items(self):
        return self.k * self.k if self.context else self.k

    def lengths(self) -> np.ndarray:
        out = np.zeros((self.m, self.items), np.int32)
        for i in range(self.m):
            cb = self.arr[i]
            for j in range(cb.num_items):
                out[i, j] = cb.items[j].bit_length
        return out

    def estimate(self) -> np.ndarray:
        return np.array([lib().huffman_estimate_size(ctypes.byref(self.arr[i]),
                                                     _ptr(np.ascontiguousarray(self.counts[i])))
                         for i in range(self.m)])

    def file_bytes(self) -> bytes:
        """huffman_codebooks.bin content (huffman_encoder.c:398-409)."""
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "cb.bin").encode()
            f = _libc.fopen(path, b"wb")
            _libc.fwrite(ctypes.byref(ctypes.c_uint32(self.m)), 4, 1, ctypes.c_void_p(f))
            for i in range(self.m):
                lib().huffman_codebook_save(ctypes.byref(self.arr[i]), ctypes.c_void_p(f))
            _libc.fclose(ctypes.c_void_p(f))
            with open(path, "rb") as fh:
                return fh.read()

    @classmethod
    def load_file(cls, path: str) -> "Codebooks":
        with open(path, "rb") as fh:
            m = int(np.frombuffer(fh.read(4), np.uint32)[0])
        obj = cls._empty(m)
        f = _libc.fopen(path.encode(), b"rb")
        _libc.fseek(ctypes.c_void_p(f), ctypes.c_long(4), 0)
        for i in range(m):
            lib().huffman_codebook_load(ctypes.byref(obj.arr[i]), ctypes.c_void_p(f))
        _libc.fclose(ctypes.c_void_p(f))
        obj.k = obj.arr[0].alphabet_size
        obj.context = bool(obj.arr[0].is_context)
        obj.counts = None
        return obj

    def close(self):
        if getattr(self, "arr", None) is not None:
            for i in range(self.m):
                if self.arr[i].items:
                    lib().huffman_codebook_destroy(ctypes.byref(self.arr[i]))
            self.arr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Tables:
    """Device code tables (pqh_tables_t): encode entries + decode lookup tables."""

    def __init__(self, ctx: Context, m: int, k: int, context: bool):
        self.ctx, self.m, self.k, self.context = ctx, m, k, bool(context)
        self.ptr = ctypes.c_void_p()
        st = lib().pqh_tables_alloc(ctx.ptr, m, k, int(context), ctypes.byref(self.ptr))
        if st:
            raise PqhError(st, "pqh_tables_alloc: " + ctx.last_error())
        ctx._retain()

    @classmethod
    def from_codebooks(cls, ctx: Context, cbs: "Codebooks") -> "Tables":
        t = cls(ctx, cbs.m, cbs.k, cbs.context)
        st = lib().pqh_tables_upload(ctx.ptr, t.ptr, ctypes.cast(cbs.arr, ctypes.c_void_p))
        if st:
            raise PqhError(st, "pqh_tables_upload: " + ctx.last_error())
        return t

    TREES = {None: 0, "lane": 1, "wave": 2, "grp": 3}

    def build(self, counts, ctx: Context = None, trees: str = None) -> "Tables":
        """GPU codebook construction from device counts (async, on `ctx`'s stream: any
        context of the same device, default the one the tables were allocated with).
        trees: the tree builder (pqh_tables_build_impl) -- None = the library default,
        "lane" (one lane per tree) or "wave" (one wavefront per tree); all build the same
        tables."""
        c = ctx or self.ctx
        check(lib().pqh_tables_build_impl(c.ptr, self.ptr, _ptr(counts), self.TREES[trees]),
              "pqh_tables_build")
        return self

    def build_trees(self, counts, ctx: Context = None, trees: str = None) -> "Tables":
        """The first half of build(): the Huffman trees only (on `ctx`'s stream)."""
        c = ctx or self.ctx
        check(lib().pqh_tables_build_trees(c.ptr, self.ptr, _ptr(counts), self.TREES[trees]),
              "pqh_tables_build_trees")
        return self

    def build_pair(self, counts, other: "Tables", counts2, ctx: Context = None) -> "Tables":
        """This table set from `counts` and `other` from `counts2` in one tree launch
        (pqh_tables_build_pair: the same tables as two build() calls)."""
        c = ctx or self.ctx
        check(lib().pqh_tables_build_pair(c.ptr, self.ptr, _ptr(counts), other.ptr, _ptr(counts2)),
              "pqh_tables_build_pair")
        return self

    def build_luts(self, ctx: Context = None) -> "Tables":
        """The second half of build(): decode tables + the encoder's gather copy, on
        `ctx`'s stream, which the caller has ordered behind build_trees (an event)."""
        c = ctx or self.ctx
        check(lib().pqh_tables_build_luts(c.ptr, self.ptr), "pqh_tables_build_luts")
        return self

    def encode_ready(self) -> bool:
        """whether the last build_trees completed the encoder's tables (the group builder
        writes the gather copy itself), so an encode need not wait for build_luts"""
        return bool(lib().pqh_tables_encode_ready(self.ptr))

    def status(self) -> None:
        st = lib().pqh_tables_status(self.ctx.ptr, self.ptr)
        if st:
            raise PqhError(st, "pqh_tables: " + self.ctx.last_error())

    def codebooks(self, counts_host=None) -> "Codebooks":
        cbs = Codebooks._empty(self.m)
        st = lib().pqh_tables_codebooks(self.ctx.ptr, self.ptr, ctypes.cast(cbs.arr, ctypes.c_void_p))
        if st:
            raise PqhError(st, "pqh_tables_codebooks: " + self.ctx.last_error())
        cbs.k, cbs.context, cbs.counts = self.k, self.context, counts_host
        return cbs

    def close(self):
        if self.ptr:
            lib().pqh_tables_destroy(self.ptr)
            self.ptr = ctypes.c_void_p()
            self.ctx._release()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def histogram(ctx: Context, codes, k: int, context: bool, prev_row=None, counts=None,
              accumulate: bool = True):
    """counts (+)= the symbol histogram of codes (huffman_encoder.c:139-205);
    accumulate=False overwrites `counts` (pqh_histogram_set: no zeroing pass)."""
    torch = _torch()
    n, m = codes.shape
    items = k * k if context else k
    if counts is None:
        counts = torch.empty((m, items), dtype=torch.int32, device=codes.device)
        accumulate = False
    fn = lib().pqh_histogram if accumulate else lib().pqh_histogram_set
    check(fn(ctx.ptr, _ptr(codes), n, m, k, int(context), _ptr(prev_row), _ptr(counts)),
          "pqh_histogram")
    return counts


def histogram_partial_bytes(n: int, m: int, k: int) -> int:
    return int(lib().pqh_histogram_partial_bytes(n, m, k))


def histogram_partial(ctx: Context, codes, k: int, partials, prev_row=None):
    """First half of the context histogram: per-chunk partial pair counts into `partials`
    (a device byte buffer of histogram_partial_bytes(n, m, k)); pqh_histogram_partial."""
    n, m = codes.shape
    check(lib().pqh_histogram_partial(ctx.ptr, _ptr(codes), n, m, k, _ptr(prev_row),
                                      _ptr(partials)), "pqh_histogram_partial")
    return partials


def histogram_parts(ctx: Context, parts, n: int, k: int, context: bool, prev_row=None,
                    counts=None, accumulate: bool = True):
    """histogram() of part-major codes parts (m, >= n) (pqh_histogram_parts)."""
    torch = _torch()
    m = parts.shape[0]
    items = k * k if context else k
    if counts is None:
        counts = torch.empty((m, items), dtype=torch.int32, device=parts.device)
        accumulate = False
    check(lib().pqh_histogram_parts(ctx.ptr, _ptr(parts), parts.stride(0), n, m, k, int(context),
                                    _ptr(prev_row), _ptr(counts), 0 if accumulate else 1),
          "pqh_histogram_parts")
    return counts


def histogram_partial_parts(ctx: Context, parts, n: int, k: int, partials, prev_row=None):
    """histogram_partial() of part-major codes (pqh_histogram_partial_parts)."""
    m = parts.shape[0]
    check(lib().pqh_histogram_partial_parts(ctx.ptr, _ptr(parts), parts.stride(0), n, m, k,
                                            _ptr(prev_row), _ptr(partials)),
          "pqh_histogram_partial_parts")
    return partials


def transpose_codes(ctx: Context, parts, n: int, rows=None):
    """part-major codes (m, >= n) -> rows (n, m) (pqh_transpose_codes)."""
    torch = _torch()
    m = parts.shape[0]
    if rows is None:
        rows = torch.empty((n, m), dtype=parts.dtype, device=parts.device)
    check(lib().pqh_transpose_codes(ctx.ptr, _ptr(parts), parts.stride(0), n, m,
                                    parts.element_size(), _ptr(rows)), "pqh_transpose_codes")
    return rows


def histogram_reduce(ctx: Context, partials, n: int, m: int, k: int, counts,
                     accumulate: bool = False):
    """Second half: counts (+)= the sum of the partials (pqh_histogram_reduce)."""
    check(lib().pqh_histogram_reduce(ctx.ptr, _ptr(partials), n, m, k, _ptr(counts),
                                     0 if accumulate else 1), "pqh_histogram_reduce")
    return counts


def sort_rows(ctx: Context, codes, tmp=None):
    """In-place stable sort of uint8 code rows in strncmp order -- the reference encoder's
    default mode (huffman_encoder.c:301-317).  `tmp`: optional n*m byte device scratch."""
    n, m = codes.shape
    check(lib().pqh_sort_rows(ctx.ptr, _ptr(codes), n, m, _ptr(tmp)), "pqh_sort_rows")
    return codes


def counts_to_host(counts) -> np.ndarray:
    """uint32 device counts -> float64 host counts (the reference keeps counts in double)."""
    return counts.cpu().numpy().view(np.uint32).astype(np.float64)


@dataclass
class Encoded:
    stream: object            # device uint8, length padded to a multiple of 4
    bits: int
    chunk_vectors: int
    chunk_offsets: object     # device int64 [chunks]
    chunk_prev: object        # device codes [chunks, m] (context) or None
    n: int
    raw_first: int

    @property
    def nbytes(self) -> int:
        return (self.bits + 7) // 8


def encode_size(ctx: Context, tables: Tables, codes, raw_first: int = 1, prev_row=None):
    """device int64[1] total bits (async)."""
    torch = _torch()
    total = torch.zeros(1, dtype=torch.int64, device=codes.device)
    check(lib().pqh_encode_size(ctx.ptr, tables.ptr, _ptr(codes), codes.shape[0], raw_first,
                                _ptr(prev_row), _ptr(total)), "pqh_encode_size")
    return total


def encode_write(ctx: Context, tables: Tables, codes, out, bit_offset: int = 0, raw_first: int = 1,
                 prev_row=None, chunk_vectors: int = 64, chunk_offsets=None, chunk_prev=None,
                 total=None):
    """One-pass encode into `out` at `bit_offset` (no zeroing needed; bits of the first word
    before bit_offset are kept).  total: optional device int64[1] receiving the bit count."""
    check(lib().pqh_encode_write(ctx.ptr, tables.ptr, _ptr(codes), codes.shape[0], raw_first,
                                 _ptr(prev_row), bit_offset, _ptr(out), out.numel(),
                                 chunk_vectors, _ptr(chunk_offsets), _ptr(chunk_prev),
                                 _ptr(total)),
          "pqh_encode_write: " + ctx.last_error())
    return total


def encode_write_parts(ctx: Context, tables: Tables, parts, n: int, out, bit_offset: int = 0,
                       raw_first: int = 1, prev_row=None, chunk_vectors: int = 64,
                       chunk_offsets=None, chunk_prev=None, total=None):
    """encode_write() of part-major codes parts (m, >= n) (pqh_encode_write_parts)."""
    check(lib().pqh_encode_write_parts(ctx.ptr, tables.ptr, _ptr(parts), parts.stride(0), n,
                                       raw_first, _ptr(prev_row), bit_offset, _ptr(out),
                                       out.numel(), chunk_vectors, _ptr(chunk_offsets),
                                       _ptr(chunk_prev), _ptr(total)),
          "pqh_encode_write_parts: " + ctx.last_error())
    return total


def encode_write_at(ctx: Context, tables: Tables, codes, out, global_bit_offset, raw_first: int = 1,
                    prev_row=None, chunk_vectors: int = 64, chunk_offsets=None, chunk_prev=None,
                    total=None):
    """encode_write for one shard of a multi-GPU stream: the shard's global bit offset is a
    device int64[1] (shard.bit_offsets_device), so no host round trip; the shard lands at
    bit (offset % 32) of `out`."""
    check(lib().pqh_encode_write_at(ctx.ptr, tables.ptr, _ptr(codes), codes.shape[0], raw_first,
                                    _ptr(prev_row), _ptr(global_bit_offset), _ptr(out),
                                    out.numel(), chunk_vectors, _ptr(chunk_offsets),
                                    _ptr(chunk_prev), _ptr(total)),
          "pqh_encode_write_at: " + ctx.last_error())
    return total


def encode(ctx: Context, tables: Tables, codes, chunk_vectors: int = 64, raw_first: int = 1,
           prev_row=None) -> Encoded:
    torch = _torch()
    n, m = codes.shape
    total = encode_size(ctx, tables, codes, raw_first, prev_row)
    bits = int(total.item())
    words = (bits + 31) // 32 + 1
    out = torch.zeros(words * 4, dtype=torch.uint8, device=codes.device)
    chunks = (n + chunk_vectors - 1) // chunk_vectors
    coff = torch.empty(max(chunks, 1), dtype=torch.int64, device=codes.device)
    cprev = torch.empty((max(chunks, 1), m), dtype=codes.dtype, device=codes.device) \
        if tables.context else None
    encode_write(ctx, tables, codes, out, 0, raw_first, prev_row, chunk_vectors, coff, cprev)
    encode_status(ctx)
    return Encoded(out, bits, chunk_vectors, coff, cprev, n, raw_first)


def decode(ctx: Context, tables: Tables, enc: Encoded, out=None):
    torch = _torch()
    dt = torch.uint8 if tables.k <= 256 else torch.int16
    if out is None:
        out = torch.empty((enc.n, tables.m), dtype=dt, device=enc.stream.device)
    check(lib().pqh_decode(ctx.ptr, tables.ptr, _ptr(enc.stream), enc.stream.numel(), enc.n,
                           enc.raw_first, enc.chunk_vectors, _ptr(enc.chunk_offsets),
                           _ptr(enc.chunk_prev), _ptr(out)), "pqh_decode")
    return out


def _index_args(enc: Encoded):
    """the stream and chunk-index arguments every decode call takes, in pqh.h order"""
    return (_ptr(enc.stream), enc.stream.numel(), enc.n, enc.raw_first, enc.chunk_vectors,
            _ptr(enc.chunk_offsets), _ptr(enc.chunk_prev))


def decode_rows(ctx: Context, tables: Tables, enc: Encoded, ids, out=None):
    """rows `ids` (device int64, any order, repeats allowed) of the stream, out[q] = row
    ids[q], without decoding the rest (pqh_decode_select).  Async; an id outside [0, n) gives
    a zero row and decode_status raises PQH_ERR_ARG."""
    torch = _torch()
    dt = torch.uint8 if tables.k <= 256 else torch.int16
    if out is None:
        out = torch.empty((ids.numel(), tables.m), dtype=dt, device=enc.stream.device)
    check(lib().pqh_decode_select(ctx.ptr, tables.ptr, *_index_args(enc), _ptr(ids), ids.numel(),
                                  _ptr(out)), "pqh_decode_select")
    return out


def decode_range(ctx: Context, tables: Tables, enc: Encoded, first: int, count: int, out=None):
    """rows [first, first + count) of the stream (pqh_decode_range); async."""
    torch = _torch()
    dt = torch.uint8 if tables.k <= 256 else torch.int16
    if out is None:
        out = torch.empty((count, tables.m), dtype=dt, device=enc.stream.device)
    check(lib().pqh_decode_range(ctx.ptr, tables.ptr, *_index_args(enc), first, count, _ptr(out)),
          "pqh_decode_range")
    return out


def decode_scatter(ctx: Context, tables: Tables, enc: Encoded, dest, out):
    """decode() through a row map: row r of the stream is stored at out[dest[r]] where
    dest[r] >= 0 (pqh_decode_scatter).  dest: device int64 (enc.n,), as ivf_regroup makes it;
    out: contiguous codes (n_out, m), only the rows that are a destination written.  A chunk is
    walked up to its last row with a destination, one without such a row is not read.  Async;
    decode_status reports a destination outside [-1, n_out) (PQH_ERR_ARG, nothing written for
    it) and a corrupt chunk (PQH_ERR_CORRUPT, its rows left unwritten)."""
    torch = _torch()
    dt = torch.uint8 if tables.k <= 256 else torch.int16
    if out.dtype != dt or not out.is_contiguous() or out.dim() != 2 or out.shape[1] != tables.m:
        raise PqhError(-1, "decode_scatter: out is a contiguous tensor of codes of shape (n_out, m)")
    if dest.dtype != torch.int64 or not dest.is_contiguous() or dest.numel() != enc.n:
        raise PqhError(-1, "decode_scatter: dest is a contiguous int64 tensor of shape (n,)")
    check(lib().pqh_decode_scatter(ctx.ptr, tables.ptr, *_index_args(enc), _ptr(dest), _ptr(out),
                                   out.shape[0]), "pqh_decode_scatter")
    return out


def fetch(ctx: Context, tables: Tables, pq: PQ, enc: Encoded, ids, out=None):
    """reconstructed float vectors of rows `ids`: out[q] = pq.reconstruct of row ids[q], the
    codes never written to memory (pqh_fetch_vectors).  out: (count, >= m * dsub) float32,
    rows out.stride(0) apart."""
    torch = _torch()
    if out is None:
        out = torch.empty((ids.numel(), pq.m * pq.dsub), dtype=torch.float32,
                          device=enc.stream.device)
    check(lib().pqh_fetch_vectors(ctx.ptr, tables.ptr, pq.ptr, *_index_args(enc), _ptr(ids),
                                  ids.numel(), _ptr(out), out.stride(0)), "pqh_fetch_vectors")
    return out


def pq_residuals(ctx: Context, pq: PQ, x, codes=None):
    """what `pq` leaves over: x - pq.reconstruct(pq.assign(x)), float32 (n, m * dsub), one fp32
    subtract per element (codes: the assignment, where the caller has it already).  The rows a
    refinement codebook is trained on (IVF.build(refine_pq=...))."""
    if codes is None:
        codes = pq.assign(x, ctx=ctx)
    return x[:, :pq.m * pq.dsub].clone().sub_(pq.reconstruct(codes))


def _metric_suffix(metric, what: str) -> str:
    """"" for metric "l2", "_ip" for "ip" (the name of the C call), PqhError(-1) otherwise"""
    if metric == "l2":
        return ""
    if metric == "ip":
        return "_ip"
    raise PqhError(-1, f"{what}: metric {metric!r} (\"l2\" or \"ip\")")


def _refine_level(level):
    """(is a stream, n, the level's arguments in pqh.h order) of (tables, pq, enc) or (pq, codes)"""
    if len(level) == 3:
        tables, pq, enc = level
        return True, enc.n, (tables.ptr, pq.ptr, _ptr(enc.stream), enc.stream.numel(),
                             enc.raw_first, enc.chunk_vectors, _ptr(enc.chunk_offsets),
                             _ptr(enc.chunk_prev))
    pq, codes = level
    if codes.dtype != _torch().uint8 or not codes.is_contiguous() or codes.shape[1] != pq.m:
        raise PqhError(-1, "refine: codes is a contiguous uint8 tensor of shape (n, m)")
    return False, codes.shape[0], (pq.ptr, _ptr(codes))


def refine(ctx: Context, level1, level2, queries, rows, k: int, coarse: "Coarse" = None,
           offsets=None, out=None):
    """(dist, rows), each (nq, k): the candidates rows[q] (device int64 (nq, ncand), stream rows,
    -1 = padding, ncand <= ctx.search_max_k) of every query re-ranked by the distance to the sum of both
    levels' reconstructions, ||q - (c1[a] + c2[b])||^2 in fp32 over all d dimensions in order;
    the k <= ncand smallest by (dist, row), padded with (+inf, -1).  A level is (tables, pq, enc)
    -- its row is decoded from the stream inside the kernel (pqh_refine_stream) -- or
    (pq, codes) with plain uint8 codes (pqh_refine_codes); both levels in the same form.
    coarse, offsets: the quantizer and the list offsets of a residual index (the query then
    loses the centroid of the row's list first).  out: a (dist, rows) pair to fill, rows
    out[0].stride(0) apart in both.  Async; decode_status reports a row outside [0, n)
    (dropped) and a corrupt stream."""
    return _refine(ctx, level1, level2, queries, rows, k, coarse, offsets, out, "l2")


def refine_ip(ctx: Context, level1, level2, queries, rows, k: int, coarse: "Coarse" = None,
              offsets=None, out=None):
    """refine() by inner product: dist is the negated inner product of the query and the sum of
    both levels' reconstructions (residual index: the centroid of the row's list added to that
    sum), acc = acc - q[j] * y[j] over all d dimensions in order (pqh_refine_stream_ip,
    pqh_refine_codes_ip).  Arguments, order, padding and errors are refine()'s."""
    return _refine(ctx, level1, level2, queries, rows, k, coarse, offsets, out, "ip")


def _refine(ctx, level1, level2, queries, rows, k, coarse, offsets, out, metric):
    torch = _torch()
    sfx = _metric_suffix(metric, "refine")
    s1, n1, a1 = _refine_level(level1)
    s2, n2, a2 = _refine_level(level2)
    if s1 != s2 or n1 != n2:
        raise PqhError(-1, "refine: both levels as streams or both as codes, of the same rows")
    if rows.dtype != torch.int64 or rows.dim() != 2 or not rows.is_contiguous() or \
            rows.shape[0] != queries.shape[0]:
        raise PqhError(-1, "refine: rows is a contiguous int64 tensor of shape (nq, ncand)")
    if (coarse is None) != (offsets is None):
        raise PqhError(-1, "refine: coarse and offsets go together")
    nq, ncand = rows.shape
    if out is None:
        out = (torch.empty((nq, k), dtype=torch.float32, device=queries.device),
               torch.empty((nq, k), dtype=torch.int64, device=queries.device))
    dist, ids = out
    ld = dist.stride(0) if nq > 1 else max(k, 1)
    if nq > 1 and ids.stride(0) != ld or (k > 1 and (dist.stride(1) != 1 or ids.stride(1) != 1)):
        raise PqhError(-1, "refine: out is a pair of tensors with rows the same distance apart")
    tail = (n1, coarse.ptr if coarse is not None else None, _ptr(offsets), _ptr(queries), nq,
            queries.stride(0), _ptr(rows), ncand, k, _ptr(dist), _ptr(ids), ld)
    name = ("pqh_refine_stream" if s1 else "pqh_refine_codes") + sfx
    check(getattr(lib(), name)(ctx.ptr, *a1, *a2, *tail), name)
    return dist, ids


def adc_tables(ctx: Context, pq: PQ, queries, out=None, metric: str = "l2"):
    """the ADC tables of `queries` (device float32 (nq, >= m * dsub)): float32 (nq, m, K),
    lut[q][i][c] = ||q_i - cent[i][c]||^2 in the assignment's arithmetic (pqh_adc_tables).
    metric="ip": lut[q][i][c] = the negated inner product of q_i and cent[i][c],
    acc = acc - q[j] * c[j] in order (pqh_adc_tables_ip); every scan takes either kind."""
    torch = _torch()
    name = "pqh_adc_tables" + _metric_suffix(metric, "adc_tables")
    nq = queries.shape[0]
    if out is None:
        out = torch.empty((nq, pq.m, pq.k), dtype=torch.float32, device=queries.device)
    check(getattr(lib(), name)(ctx.ptr, pq.ptr, _ptr(queries), nq, queries.stride(0), _ptr(out)),
          name)
    return out


def _search_out(lut, k, out):
    torch = _torch()
    if out is not None:
        return out
    nq = lut.shape[0]
    return (torch.empty((nq, k), dtype=torch.float32, device=lut.device),
            torch.empty((nq, k), dtype=torch.int64, device=lut.device))


def pack_mask(ctx: Context, keep, perm=None, out=None):
    """the row mask of the searches' keep= from a flag per row: int32 (ceil(n / 32),), bit
    i & 31 of word i >> 5 = keep[perm[i]] (perm None: keep[i]) (pqh_mask_pack).  keep: device
    bool or uint8 (n,), nonzero = the row may be returned; perm: device int64 (n,), e.g. an
    IVF's (stream row -> caller row).  Async; ivf_status reports a perm entry outside [0, n)
    (its bit is zero)."""
    torch = _torch()
    n = keep.numel()
    if keep.dtype not in (torch.bool, torch.uint8) or keep.dim() != 1:
        raise PqhError(-1, "pack_mask: keep is a bool or uint8 tensor of shape (n,)")
    if perm is not None and perm.numel() != n:
        raise PqhError(-1, f"pack_mask: {perm.numel()} perm entries for {n} rows")
    keep = keep.contiguous()
    if perm is not None and not perm.is_contiguous():
        perm = perm.contiguous()
    if out is None:
        out = torch.empty((n + 31) // 32, dtype=torch.int32, device=keep.device)
    check(lib().pqh_mask_pack(ctx.ptr, _ptr(keep), _ptr(perm), n, _ptr(out)), "pqh_mask_pack")
    return out


def _entry(name: str, keep, n: int):
    """(entry point, its trailing arguments): today's call without a mask, the _masked one
    with the words behind d_ids.  keep: device int32, at least ceil(n / 32) words."""
    if keep is None:
        return getattr(lib(), name), ()
    if keep.dtype != _torch().int32 or not keep.is_contiguous() or keep.numel() < (n + 31) // 32:
        raise PqhError(-1, f"{name}: keep is a contiguous int32 tensor of ceil(n / 32) words")
    return getattr(lib(), name + "_masked"), (_ptr(keep),)


def search(ctx: Context, tables: Tables, enc: Encoded, lut, k: int, id_base: int = 0, out=None,
           keep=None):
    """(dist, ids), each (nq, k): per query table lut[q] (float32 (m, K)) the k rows of the
    stream with the smallest summed entries, ascending by (dist, id), ids = stream rows +
    id_base, padded with (+inf, -1); the stream is decoded and scored in one kernel, the
    codes never written (pqh_search_stream).  Async; decode_status reports a corrupt stream.
    out: a (dist, ids) pair to fill.
    keep: the row mask, device int32 words as pack_mask makes them (bit r & 31 of word r >> 5 =
    stream row r may be returned; the bits from n on are ignored).  The result is then the top k
    among the kept rows, and what is not kept is not decoded (pqh_search_stream_masked); this
    holds for every search_* function below."""
    dist, ids = _search_out(lut, k, out)
    fn, mask = _entry("pqh_search_stream", keep, enc.n)
    check(fn(ctx.ptr, tables.ptr, *_index_args(enc), _ptr(lut), lut.shape[0], k, id_base,
             _ptr(dist), _ptr(ids), *mask), "pqh_search_stream")
    return dist, ids


def search_codes(ctx: Context, codes, lut, k: int, id_base: int = 0, out=None, keep=None):
    """search() over plain uint8 codes (n, m) (pqh_search_codes)."""
    dist, ids = _search_out(lut, k, out)
    fn, mask = _entry("pqh_search_codes", keep, codes.shape[0])
    check(fn(ctx.ptr, _ptr(codes), codes.shape[0], codes.shape[1], lut.shape[2], _ptr(lut),
             lut.shape[0], k, id_base, _ptr(dist), _ptr(ids), *mask), "pqh_search_codes")
    return dist, ids


def merge_topk(ctx: Context, dist, ids, k: int = None, id_base=None, out=None):
    """(dist, ids), each (nq, k): several top-k results into one (pqh_topk_merge).  dist: device
    float32 (parts, nq, k_in), ids: int64 of the same shape -- e.g. the searches of the row
    blocks of an index, stacked, or what an all-gather of every rank's result leaves.  Per query
    the k (default k_in) smallest of all parts' entries with id >= 0, each id moved by its part's
    id_base (None: zeros, a sequence of ints, or a device int64 tensor (parts,)), ascending by
    (dist, moved id), padded with (+inf, -1).  Nothing is assumed about the order inside a part,
    and padding may sit anywhere.  k <= ctx.search_max_k.  Async.

    Over the searches of the row blocks of one data set (no refine=) the distances are those of
    one index over all rows, bit for bit, and so are the ids wherever a query's distances are
    distinct; equal distances come in id order here, in (list, id) order from one IVF."""
    torch = _torch()
    if dist.dim() != 3 or ids.shape != dist.shape or dist.dtype != torch.float32 or \
            ids.dtype != torch.int64:
        raise PqhError(-1, "merge_topk: dist float32 and ids int64, both (parts, nq, k_in)")
    parts, nq, k_in = dist.shape
    k = k_in if k is None else int(k)
    dist, ids = dist.contiguous(), ids.contiguous()
    if id_base is not None and not torch.is_tensor(id_base):
        id_base = torch.tensor([int(v) for v in id_base], dtype=torch.int64, device=dist.device)
    if id_base is not None:
        if id_base.dtype != torch.int64 or id_base.numel() != parts:
            raise PqhError(-1, "merge_topk: id_base is int64 with one entry per part")
        id_base = id_base.to(dist.device).contiguous()
    if out is None:
        out = (torch.empty((nq, k), dtype=torch.float32, device=dist.device),
               torch.empty((nq, k), dtype=torch.int64, device=dist.device))
    check(lib().pqh_topk_merge(ctx.ptr, _ptr(dist), _ptr(ids), parts, nq, k_in, _ptr(id_base), k,
                               _ptr(out[0]), _ptr(out[1])), "pqh_topk_merge")
    return out


def search_ranges(ctx: Context, tables: Tables, enc: Encoded, lut, range_ptr, ranges, k: int,
                  id_base: int = 0, out=None, keep=None):
    """search() of per-query row ranges, the way an inverted file is probed: query q scores
    only the rows [ranges[r, 0], ranges[r, 0] + ranges[r, 1]) for r in
    [range_ptr[q], range_ptr[q + 1]), and only the chunks under them are decoded
    (pqh_search_stream_ranges).  range_ptr: device int64 (nq + 1,); ranges: device int64
    (nr, 2).  Ranges may cut chunks and may overlap (a row is then offered once per range).
    Async; decode_status reports a corrupt chunk that was walked (PQH_ERR_CORRUPT) or a bad
    range or range_ptr value (PQH_ERR_ARG, the range or query skipped)."""
    dist, ids = _search_out(lut, k, out)
    fn, mask = _entry("pqh_search_stream_ranges", keep, enc.n)
    check(fn(ctx.ptr, tables.ptr, *_index_args(enc), _ptr(lut), lut.shape[0], _ptr(range_ptr),
             _ptr(ranges), ranges.shape[0], k, id_base, _ptr(dist), _ptr(ids), *mask),
          "pqh_search_stream_ranges")
    return dist, ids


def search_codes_ranges(ctx: Context, codes, lut, range_ptr, ranges, k: int, id_base: int = 0,
                        out=None, keep=None):
    """search_ranges() over plain uint8 codes (n, m) (pqh_search_codes_ranges)."""
    dist, ids = _search_out(lut, k, out)
    fn, mask = _entry("pqh_search_codes_ranges", keep, codes.shape[0])
    check(fn(ctx.ptr, _ptr(codes), codes.shape[0], codes.shape[1], lut.shape[2], _ptr(lut),
             lut.shape[0], _ptr(range_ptr), _ptr(ranges), ranges.shape[0], k, id_base, _ptr(dist),
             _ptr(ids), *mask), "pqh_search_codes_ranges")
    return dist, ids


def adc_tables_residual(ctx: Context, pq: PQ, coarse: "Coarse", queries, probes, out=None,
                        metric: str = "l2"):
    """one ADC table per (query, probed list): float32 (nq * nprobe, m, K), table q * nprobe + p
    that of queries[q] - centroid[probes[q, p]] in adc_tables' arithmetic
    (pqh_adc_tables_residual).  probes: device int64 (nq, nprobe) as Coarse.probe returns them;
    an entry of -1 gives a table of +inf.  Async; ivf_status reports any other entry outside
    [0, nlist).
    metric="ip": table q * nprobe + p is adc_tables(metric="ip") of queries[q] with the negated
    inner product of queries[q] and centroid[probes[q, p]] (Coarse.probe's probe_dist, bit for
    bit) added to every entry of part 0 (pqh_adc_tables_residual_ip)."""
    torch = _torch()
    name = "pqh_adc_tables_residual" + _metric_suffix(metric, "adc_tables_residual")
    nq, nprobe = probes.shape
    if not probes.is_contiguous():
        probes = probes.contiguous()
    if out is None:
        out = torch.empty((nq * nprobe, pq.m, pq.k), dtype=torch.float32, device=queries.device)
    check(getattr(lib(), name)(ctx.ptr, pq.ptr, coarse.ptr, _ptr(queries), nq, queries.stride(0),
                               _ptr(probes), nprobe, _ptr(out)), name)
    return out


def _range_search_out(range_ptr, k, out):
    torch = _torch()
    if out is not None:
        return out
    nq = range_ptr.numel() - 1
    return (torch.empty((nq, k), dtype=torch.float32, device=range_ptr.device),
            torch.empty((nq, k), dtype=torch.int64, device=range_ptr.device))


def search_range_tables(ctx: Context, tables: Tables, enc: Encoded, lut, range_ptr, ranges,
                        k: int, id_base: int = 0, out=None, keep=None):
    """search_ranges() with one table per range: lut float32 (nr, m, K), range r scored with
    lut[r] (pqh_search_stream_range_tables) -- the probe search of a residual inverted file,
    lut from adc_tables_residual.  The number of queries is range_ptr.numel() - 1."""
    dist, ids = _range_search_out(range_ptr, k, out)
    fn, mask = _entry("pqh_search_stream_range_tables", keep, enc.n)
    check(fn(ctx.ptr, tables.ptr, *_index_args(enc), _ptr(lut), range_ptr.numel() - 1,
             _ptr(range_ptr), _ptr(ranges), ranges.shape[0], k, id_base, _ptr(dist), _ptr(ids),
             *mask), "pqh_search_stream_range_tables")
    return dist, ids


def search_codes_range_tables(ctx: Context, codes, lut, range_ptr, ranges, k: int,
                              id_base: int = 0, out=None, keep=None):
    """search_range_tables() over plain uint8 codes (n, m) (pqh_search_codes_range_tables)."""
    dist, ids = _range_search_out(range_ptr, k, out)
    fn, mask = _entry("pqh_search_codes_range_tables", keep, codes.shape[0])
    check(fn(ctx.ptr, _ptr(codes), codes.shape[0], codes.shape[1], lut.shape[2], _ptr(lut),
             range_ptr.numel() - 1, _ptr(range_ptr), _ptr(ranges), ranges.shape[0], k, id_base,
             _ptr(dist), _ptr(ids), *mask), "pqh_search_codes_range_tables")
    return dist, ids


def _lists_args(lut, offsets, probes, k, out):
    """(nlist, probes, nq, nprobe, tables_per_probe, dist, ids) of the list-major calls: the
    table form from lut.shape[0], nq for a table per query, nq * nprobe for one per pair"""
    torch = _torch()
    nq, nprobe = probes.shape
    if lut.shape[0] == nq * nprobe and nprobe > 1:
        per_probe = 1
    elif lut.shape[0] == nq:
        per_probe = 0
    else:
        raise PqhError(-1, f"search_lists: {lut.shape[0]} tables for {nq} queries of {nprobe} probes")
    if not probes.is_contiguous():
        probes = probes.contiguous()
    if out is None:
        out = (torch.empty((nq, k), dtype=torch.float32, device=probes.device),
               torch.empty((nq, k), dtype=torch.int64, device=probes.device))
    return offsets.numel() - 1, probes, nq, nprobe, per_probe, out[0], out[1]


def search_lists(ctx: Context, tables: Tables, enc: Encoded, lut, offsets, probes, k: int,
                 id_base: int = 0, out=None, keep=None):
    """the probe search in list-major order (pqh_search_stream_lists): the result of
    search_ranges (lut float32 (nq, m, K)) or search_range_tables (lut (nq * nprobe, m, K)) on
    probe_ranges(offsets, probes), bit for bit, but a list probed by several queries is decoded
    once per batch of eight of them (four when m > 8) -- the schedule for many queries.
    offsets: device int64 (nlist + 1,) as ivf_layout gives them; probes: device int64
    (nq, nprobe), -1 = none.  Async; decode_status reports a corrupt chunk that was walked
    (PQH_ERR_CORRUPT) or a probe outside [-1, nlist) or a bad offsets pair of a probed list
    (PQH_ERR_ARG, the probe skipped)."""
    nlist, probes, nq, nprobe, per_probe, dist, ids = _lists_args(lut, offsets, probes, k, out)
    fn, mask = _entry("pqh_search_stream_lists", keep, enc.n)
    check(fn(ctx.ptr, tables.ptr, *_index_args(enc), _ptr(offsets), nlist, _ptr(probes), nq,
             nprobe, _ptr(lut), per_probe, k, id_base, _ptr(dist), _ptr(ids), *mask),
          "pqh_search_stream_lists")
    return dist, ids


def search_codes_lists(ctx: Context, codes, lut, offsets, probes, k: int, id_base: int = 0,
                       out=None, keep=None):
    """search_lists() over plain uint8 codes (n, m) (pqh_search_codes_lists)."""
    nlist, probes, nq, nprobe, per_probe, dist, ids = _lists_args(lut, offsets, probes, k, out)
    fn, mask = _entry("pqh_search_codes_lists", keep, codes.shape[0])
    check(fn(ctx.ptr, _ptr(codes), codes.shape[0], codes.shape[1], lut.shape[2], _ptr(offsets),
             nlist, _ptr(probes), nq, nprobe, _ptr(lut), per_probe, k, id_base, _ptr(dist),
             _ptr(ids), *mask), "pqh_search_codes_lists")
    return dist, ids


def _range_search(ctx: Context, name: str, src, n: int, m: int, k: int, chunk_vectors: int, lut,
                  nq: int, probe, radius, keep, id_base: int, capacity):
    """count, (read the total,) fill: pqh_range_count_<name> and pqh_range_fill_<name> over a
    plan allocated here.  src: the calls' leading arguments; probe: None (the whole stream) or
    (range_ptr, ranges, tables_per_range)."""
    torch = _torch()
    dev = lut.device
    if torch.is_tensor(radius):
        if radius.dtype != torch.float32 or radius.shape != (nq,):
            raise PqhError(-1, f"range_search: radius is a float or a float32 tensor of shape ({nq},)")
        radius = radius.contiguous()
    else:
        radius = torch.full((nq,), float(radius), dtype=torch.float32, device=dev)
    if keep is not None and (keep.dtype != torch.int32 or not keep.is_contiguous() or
                             keep.numel() < (n + 31) // 32):
        raise PqhError(-1, "range_search: keep is a contiguous int32 tensor of ceil(n / 32) words")
    if probe is None:
        list_args = (None, None, -1, 0)
    else:
        range_ptr, ranges, per_range = probe
        list_args = (_ptr(range_ptr), _ptr(ranges), ranges.shape[0], int(bool(per_range)))
    nbytes = ctypes.c_ulonglong(0)
    check(lib().pqh_range_plan_bytes(ctx.ptr, n, m, k, chunk_vectors, nq, list_args[2],
                                     list_args[3], ctypes.byref(nbytes)), "pqh_range_plan_bytes")
    plan = torch.empty((nbytes.value + 7) // 8, dtype=torch.int64, device=dev)
    lims = torch.empty(nq + 1, dtype=torch.int64, device=dev)
    args = (ctx.ptr, *src, _ptr(lut), nq, *list_args, _ptr(radius), _ptr(keep), _ptr(plan),
            plan.numel() * 8, _ptr(lims))
    check(getattr(lib(), f"pqh_range_count_{name}")(*args), f"pqh_range_count_{name}")
    if capacity is None:
        capacity = int(lims[-1].item())     # the one synchronisation
        dist = torch.empty(capacity, dtype=torch.float32, device=dev)
        ids = torch.empty(capacity, dtype=torch.int64, device=dev)
    else:
        dist = torch.full((capacity,), float("inf"), dtype=torch.float32, device=dev)
        ids = torch.full((capacity,), -1, dtype=torch.int64, device=dev)
    check(getattr(lib(), f"pqh_range_fill_{name}")(*args, capacity, id_base, _ptr(dist), _ptr(ids)),
          f"pqh_range_fill_{name}")
    return lims, dist, ids


def range_search(ctx: Context, tables: Tables, enc: Encoded, lut, radius, keep=None,
                 id_base: int = 0, capacity=None):
    """(lims, dist, ids): every row of the stream with dist < radius[q] (strict; search()'s
    fp32 sum), as many as there are, in CSR form: query q's hits are dist / ids
    [lims[q], lims[q + 1]) in ascending stream row, ids = stream rows + id_base; lims int64
    (nq + 1,), dist float32 and ids int64 (lims[nq],).  Two scans of the stream
    (pqh_range_count_stream, pqh_range_fill_stream): the first counts, the second writes, and
    where the first counted nothing the second decodes nothing.  A NaN radius or distance is no
    hit; bits and order do not depend on the grid.
    radius: a float, or a device float32 tensor (nq,).  keep: the row mask of search().
    capacity=None: the outputs are allocated exactly, which waits once for the device to read
    lims[-1] between the two scans (as encode() does for the stream's length).  capacity=int:
    no wait; dist and ids have that length, hold the first `capacity` entries of the result and
    (+inf, -1) behind lims[-1]; lims always holds the full counts, so lims[-1] > capacity says
    that the result was cut.  Async otherwise; decode_status reports a corrupt stream."""
    return _range_search(ctx, "stream", (tables.ptr, *_index_args(enc)), enc.n, tables.m, tables.k,
                         enc.chunk_vectors, lut, lut.shape[0], None, radius, keep, id_base, capacity)


def range_search_codes(ctx: Context, codes, lut, radius, keep=None, id_base: int = 0,
                       capacity=None):
    """range_search() over plain uint8 codes (n, m) (pqh_range_count_codes, pqh_range_fill_codes)."""
    n, m = codes.shape
    return _range_search(ctx, "codes", (_ptr(codes), n, m, lut.shape[2]), n, m, lut.shape[2], 0,
                         lut, lut.shape[0], None, radius, keep, id_base, capacity)


def range_search_ranges(ctx: Context, tables: Tables, enc: Encoded, lut, range_ptr, ranges, radius,
                        tables_per_range: bool = False, keep=None, id_base: int = 0,
                        capacity=None):
    """range_search() of per-query row ranges (search_ranges' probe list; tables_per_range:
    lut (nr, m, K), range r scored with lut[r], as search_range_tables).  Query q's hits come
    range by range in the order of its list, ascending row inside a range; a row under two
    overlapping or repeated ranges appears once per range.  decode_status also reports a bad
    range or range_ptr value (PQH_ERR_ARG, the range or query skipped)."""
    nq = range_ptr.numel() - 1
    return _range_search(ctx, "stream", (tables.ptr, *_index_args(enc)), enc.n, tables.m, tables.k,
                         enc.chunk_vectors, lut, nq, (range_ptr, ranges, tables_per_range), radius,
                         keep, id_base, capacity)


def range_search_codes_ranges(ctx: Context, codes, lut, range_ptr, ranges, radius,
                              tables_per_range: bool = False, keep=None, id_base: int = 0,
                              capacity=None):
    """range_search_ranges() over plain uint8 codes (n, m)."""
    n, m = codes.shape
    nq = range_ptr.numel() - 1
    return _range_search(ctx, "codes", (_ptr(codes), n, m, lut.shape[2]), n, m, lut.shape[2], 0,
                         lut, nq, (range_ptr, ranges, tables_per_range), radius, keep, id_base,
                         capacity)


def ivf_layout(list_ids, nlist: int):
    """(perm, offsets) for storing rows list by list: perm is the stable order of the rows by
    list id (stream row s holds original row perm[s]), offsets int64 (nlist + 1,) with list l
    at stream rows [offsets[l], offsets[l + 1]).  list_ids: int64 (n,) in [0, nlist).  Plain
    torch on the tensor's device, no sync."""
    torch = _torch()
    by_list, perm = torch.sort(list_ids, stable=True)
    offsets = torch.searchsorted(by_list, torch.arange(nlist + 1, dtype=list_ids.dtype,
                                                       device=list_ids.device))
    return perm, offsets.to(torch.int64)


def probe_ranges(offsets, probes):
    """(range_ptr, ranges) for search_ranges from ivf_layout's offsets and the lists each query
    probes: probes int64 (nq, nprobe), an entry of -1 probing nothing (an empty range, so
    range_ptr is arange(nq + 1) * nprobe and nothing is compacted).  No sync."""
    torch = _torch()
    nq, nprobe = probes.shape
    lists = probes.reshape(-1)
    none = lists < 0
    lists = lists.clamp(min=0)
    first = offsets[lists]
    count = offsets[lists + 1] - first
    zero = torch.zeros_like(first)
    ranges = torch.stack((torch.where(none, zero, first), torch.where(none, zero, count)), dim=1)
    range_ptr = torch.arange(nq + 1, dtype=torch.int64, device=probes.device) * nprobe
    return range_ptr, ranges.contiguous()


class Coarse:
    """The coarse quantizer of an inverted file (pqh_coarse_t): nlist centroids of full
    d-dimensional vectors on the device.  centroids: host float32 (nlist, d) -- or
    (1, nlist, d), as kmeans_train(m = 1, k = nlist, dsub = d) returns them.  Distances are the
    direct form in fp32 (the arithmetic of PQ.assign and adc_tables), ties go to the smaller
    list id."""

    def __init__(self, ctx: Context, centroids: np.ndarray):
        c = np.ascontiguousarray(centroids, np.float32)
        if c.ndim == 3 and c.shape[0] == 1:
            c = c[0]
        self.nlist, self.d = c.shape
        self.ctx = ctx
        self.ptr = ctypes.c_void_p()
        check(lib().pqh_coarse_create(ctx.ptr, _ptr(c), self.nlist, self.d,
                                      ctypes.byref(self.ptr)), "pqh_coarse_create")
        ctx._retain()
        # a device copy for torch (the fetch of a residual index adds a row's centroid back)
        self.centroids = _torch().tensor(c, device=f"cuda:{ctx.device}")

    def assign(self, x, out=None, dist=None, metric: str = "l2"):
        """list ids int32 (n,) of the rows of x (device float32 (n, >= d)), the nearest
        centroid each (pqh_coarse_assign); dist: an optional float32 (n,) tensor that takes the
        winning distances.  metric="ip": the centroid of the largest inner product, dist its
        negation (pqh_coarse_assign_ip).  Async."""
        torch = _torch()
        name = "pqh_coarse_assign" + _metric_suffix(metric, "Coarse.assign")
        n = x.shape[0]
        if out is None:
            out = torch.empty(n, dtype=torch.int32, device=x.device)
        check(getattr(lib(), name)(self.ctx.ptr, self.ptr, _ptr(x), n, x.stride(0), _ptr(out),
                                   _ptr(dist)), name)
        return out

    def layout(self, list_ids):
        """(perm, offsets) as ivf_layout gives them, by pqh_ivf_layout: list_ids device int32
        (n,).  Async; ivf_status reports an id outside [0, nlist)."""
        torch = _torch()
        if list_ids.dtype != torch.int32 or not list_ids.is_contiguous():
            list_ids = list_ids.to(torch.int32).contiguous()
        n = list_ids.numel()
        perm = torch.empty(n, dtype=torch.int64, device=list_ids.device)
        offsets = torch.empty(self.nlist + 1, dtype=torch.int64, device=list_ids.device)
        check(lib().pqh_ivf_layout(self.ctx.ptr, _ptr(list_ids), n, self.nlist, _ptr(perm),
                                   _ptr(offsets)), "pqh_ivf_layout")
        return perm, offsets

    def residuals(self, x, list_ids, perm=None, out=None):
        """out[s] = x[p] - centroid[list_ids[p]], p = perm[s] (perm None: p = s): the rows in
        list order and their residuals in one pass (pqh_ivf_residuals).  list_ids: device int32
        (n,) by caller row, as assign() returns them; perm: device int64 (n,) as layout()
        returns it; out: float32 (n, >= d), only its first d columns written.  Async;
        ivf_status reports a perm entry or a list id out of range (the row is then zeros)."""
        torch = _torch()
        n = x.shape[0]
        if list_ids.dtype != torch.int32 or not list_ids.is_contiguous():
            list_ids = list_ids.to(torch.int32).contiguous()
        if perm is not None and not perm.is_contiguous():
            perm = perm.contiguous()
        if out is None:
            out = torch.empty((n, self.d), dtype=torch.float32, device=x.device)
        check(lib().pqh_ivf_residuals(self.ctx.ptr, self.ptr, _ptr(x), n, x.stride(0),
                                      _ptr(list_ids), _ptr(perm), _ptr(out), out.stride(0)),
              "pqh_ivf_residuals")
        return out

    def probe(self, queries, nprobe: int, offsets, lists: bool = True, metric: str = "l2"):
        """(range_ptr, ranges, probes, probe_dist): for every query (device float32
        (nq, >= d)) its nprobe nearest lists by (dist, list id) and their row ranges in the CSR
        form search_ranges takes (pqh_coarse_probe).  probes int64 (nq, nprobe) and probe_dist
        float32 (nq, nprobe), padded with (-1, +inf) and the range (0, 0) when nprobe > nlist;
        lists=False leaves the two out (None).  metric="ip": the lists of the largest inner
        products, probe_dist their negations (pqh_coarse_probe_ip).  Async, no sync."""
        torch = _torch()
        name = "pqh_coarse_probe" + _metric_suffix(metric, "Coarse.probe")
        nq = queries.shape[0]
        dev = queries.device
        range_ptr = torch.empty(nq + 1, dtype=torch.int64, device=dev)
        ranges = torch.empty((nq * nprobe, 2), dtype=torch.int64, device=dev)
        probes = torch.empty((nq, nprobe), dtype=torch.int64, device=dev) if lists else None
        pdist = torch.empty((nq, nprobe), dtype=torch.float32, device=dev) if lists else None
        check(getattr(lib(), name)(self.ctx.ptr, self.ptr, _ptr(queries), nq, queries.stride(0),
                                   nprobe, _ptr(offsets), _ptr(range_ptr), _ptr(ranges),
                                   _ptr(probes), _ptr(pdist)), name)
        return range_ptr, ranges, probes, pdist

    def close(self):
        if self.ptr:
            lib().pqh_coarse_destroy(self.ptr)
            self.ptr = ctypes.c_void_p()
            self.ctx._release()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _ld(t, d: int) -> int:
    """the floats between two rows of t; a tensor of fewer than two rows has no such distance
    (torch reports 0 for an empty one), and any value >= d serves"""
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), d)


class Rotation:
    """A d x d matrix on the device (pqh_rotation_t), applied to rows before the quantizers see
    them: the learned rotation of OPQ.  R: host float32 (d, d), 1 <= d <= 1024.  Any matrix is
    accepted, apply() is a linear map; defect() says how far R is from orthonormal, and
    IVF.build(rotation=) checks it."""

    def __init__(self, ctx: Context, R: np.ndarray):
        r = np.ascontiguousarray(R, np.float32)
        if r.ndim != 2 or r.shape[0] != r.shape[1]:
            raise PqhError(-1, "Rotation: R is a square matrix")
        self.d = r.shape[0]
        self.R = r                  # the float32 host copy
        self.ctx = ctx
        self.ptr = ctypes.c_void_p()
        check(lib().pqh_rotation_create(ctx.ptr, _ptr(r), self.d, ctypes.byref(self.ptr)),
              "pqh_rotation_create")
        ctx._retain()

    def apply(self, x, out=None, transpose: bool = False):
        """out[v] = x[v] @ R (transpose: x[v] @ R.T, the way back when R is orthonormal), one
        fp32 chain per output with t ascending (pqh_rotate): x device float32 (n, >= d), out
        float32 (n, >= d), only its first d columns written, and not x itself.  Async."""
        torch = _torch()
        n = x.shape[0]
        if out is None:
            out = torch.empty((n, self.d), dtype=torch.float32, device=x.device)
        check(lib().pqh_rotate(self.ctx.ptr, self.ptr, _ptr(x), n, _ld(x, self.d), _ptr(out),
                               _ld(out, self.d), int(bool(transpose))), "pqh_rotate")
        return out

    def defect(self) -> float:
        """max |R^T R - I| in float64 on the host: 0 for an orthonormal matrix, about
        d * 2^-24 for one rounded to float32"""
        r = self.R.astype(np.float64)
        return float(np.abs(r.T @ r - np.eye(self.d)).max())

    def close(self):
        if self.ptr:
            lib().pqh_rotation_destroy(self.ptr)
            self.ptr = ctypes.c_void_p()
            self.ctx._release()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def cross_moments(ctx: Context, x, y) -> np.ndarray:
    """float64 (dx, dy): M[a][b] = sum_v x[v][a] * y[v][b] over device float32 rows x (n, dx)
    and y (n, dy), every product one fp32 multiply and the sum exact in 64-bit fixed point
    (pqh_cross_moments), so the result is the same on every run.  dx, dy <= 1024.  Waits for
    the device."""
    n, dx = x.shape
    if y.shape[0] != n:
        raise PqhError(-1, "cross_moments: x and y disagree in rows")
    dy = y.shape[1]
    out = np.empty((dx, dy), np.float64)
    check(lib().pqh_cross_moments(ctx.ptr, _ptr(x), n, _ld(x, dx), dx, _ptr(y), _ld(y, dy), dy,
                                  _ptr(out)), "pqh_cross_moments")
    return out


def procrustes(M: np.ndarray) -> np.ndarray:
    """float32 (d, d): the orthonormal R that maximises trace(R^T M), U @ Vt of M's singular
    value decomposition -- with M = X^T Y the rotation that takes the rows of X nearest to those
    of Y.  Host numpy on a d x d matrix."""
    u, _, vt = np.linalg.svd(np.asarray(M, np.float64))
    return (u @ vt).astype(np.float32)


def pca_rotation(ctx: Context, x, m: int) -> np.ndarray:
    """float32 (d, d): the PCA start of OPQ with eigenvalue allocation.  The covariance of x
    (device float32 (n, d), d a multiple of m) is cross_moments(x, x) / n - mu mu^T with mu from
    the column sums cross_moments(x, ones); its eigenvectors, eigenvalues descending (a stable
    order), go one by one to the subspace with room (fewer than d / m columns) whose sum of
    log max(eigenvalue, tiny) is smallest so far, ties to the lower subspace.  The columns of R
    are subspace by subspace in the order they were taken, so x @ R has subspaces of balanced
    variance products."""
    torch = _torch()
    n, d = x.shape
    if m < 1 or d % m or n < 1:
        raise PqhError(-1, "pca_rotation: d is a multiple of m and x has rows")
    ones = torch.ones((n, 1), dtype=torch.float32, device=x.device)
    mu = cross_moments(ctx, x, ones)[:, 0] / n
    cov = cross_moments(ctx, x, x) / n - np.outer(mu, mu)
    lam, vec = np.linalg.eigh(cov)
    order = np.argsort(-lam, kind="stable")
    dsub = d // m
    taken = [[] for _ in range(m)]
    logs = np.zeros(m, np.float64)
    tiny = np.finfo(np.float64).tiny
    for e in order:
        best = -1
        for i in range(m):
            if len(taken[i]) < dsub and (best < 0 or logs[i] < logs[best]):
                best = i
        taken[best].append(e)
        logs[best] += np.log(max(lam[e], tiny))
    cols = [e for t in taken for e in t]
    return np.ascontiguousarray(vec[:, cols]).astype(np.float32)


def opq_train(ctx: Context, x, m: int, k: int, cent_init: np.ndarray, outer: int = 8,
              inner: int = 2, init="identity", trace: list = None):
    """(R, centroids, errors): a rotation and the product quantizer of the rotated rows, trained
    together (OPQ, the non-parametric form).  x: device float32 (n, d), d a multiple of m.

        R = init;  cent = cent_init
        for it in 0 .. outer:
            xr   = Rotation(R).apply(x)
            cent = kmeans_train(xr, cent, inner)            # warm start
            codes = PQ(cent).assign(xr);  errors[it] = PQ.error(xr, codes)
            if it == outer: break
            R = procrustes(cross_moments(x, PQ.reconstruct(codes)))      # X^T Y

    It ends on a k-means at the final R, so the returned codebook belongs to the returned
    rotation: outer + 1 rounds of `inner` Lloyd iterations and `outer` Procrustes steps.
    cent_init [m][k][dsub] are centroids in the ROTATED space: rows of init-rotated sample
    vectors, say.  The k-means starts from the last round's centroids and the Procrustes step is
    the best rotation for the codes at hand, so no step can raise the error and the result is
    never worse than the PQ of init.

    init: "identity" (the default, the safe start: on a 4,000 x 32 world of a decaying spectrum
    behind a random orthonormal mix, m = 8, K = 64, a numpy prototype with a float64 Lloyd took
    the error from 2,554 to 1,017 and recall@10 from 0.64 to 0.74; about +4 % on SIFT-like and
    +5 % on deep-like rows), "pca" (pca_rotation: for data with a spectrum -- 320 and 0.85 on
    that world, but 12 % behind the plain PQ on SIFT-like rows), or a (d, d) matrix.
    trace: a list that takes dict(R, cent, err, M) of every round (M: the moments the next R
    came from, None for the last).  Synchronous."""
    torch = _torch()
    n, d = x.shape
    cent = np.ascontiguousarray(cent_init, np.float32)
    if m < 1 or d % m or cent.shape != (m, k, d // m) or outer < 0 or inner < 0:
        raise PqhError(-1, "opq_train: cent_init is [m][k][d / m] and d a multiple of m")
    if isinstance(init, str):
        if init == "identity":
            R = np.eye(d, dtype=np.float32)
        elif init == "pca":
            R = pca_rotation(ctx, x, m)
        else:
            raise PqhError(-1, f"opq_train: init {init!r}")
    else:
        R = np.ascontiguousarray(init, np.float32)
        if R.shape != (d, d):
            raise PqhError(-1, "opq_train: init is a (d, d) matrix")
    xr = torch.empty((n, d), dtype=torch.float32, device=x.device)
    errors = []
    for it in range(outer + 1):
        rot = Rotation(ctx, R)
        rot.apply(x, out=xr)
        rot.close()
        cent = kmeans_train(ctx, xr, cent, inner)
        pq = PQ(ctx, cent)
        try:
            codes = pq.assign(xr)
            errors.append(pq.error(xr, codes))
            if trace is not None:
                trace.append(dict(R=R, cent=cent, err=errors[-1], M=None))
            if it == outer:
                break
            M = cross_moments(ctx, x, pq.reconstruct(codes))
        finally:
            pq.close()
        if trace is not None:
            trace[-1]["M"] = M
        R = procrustes(M)
    return R, cent, errors


def ivf_regroup(ctx: Context, offsets, keep=None, add_offsets=None, n: int = None):
    """(new_offsets, dest, add_base): the plan that takes a list-ordered stream to a new list
    order (pqh_ivf_regroup).  offsets: device int64 (nlist + 1,) of the stream's n rows; keep:
    the rows that stay, int32 words as pack_mask makes them (None: all); add_offsets: the
    layout offsets of a batch of new rows (None: none).  In the new order a list holds its kept
    rows in their old order, then the gap for its added rows: dest int64 (n,) is the new row of
    every old one (-1: dropped), new_offsets (nlist + 1,) the new lists, add_base (nlist,) the
    first row of every gap.  n: the stream's rows, where the caller knows them; None reads
    offsets[-1] (synchronises).  Async otherwise; ivf_status reports offsets that do not cover
    [0, n) in ascending order."""
    torch = _torch()
    if n is None:
        n = int(offsets[-1].item())
    nlist = offsets.numel() - 1
    for name, t in (("offsets", offsets), ("add_offsets", add_offsets)):
        if t is not None and (t.dtype != torch.int64 or not t.is_contiguous() or
                              t.numel() != nlist + 1):
            raise PqhError(-1, f"ivf_regroup: {name} is a contiguous int64 tensor of nlist + 1 entries")
    if keep is not None and (keep.dtype != torch.int32 or not keep.is_contiguous() or
                             keep.numel() < (n + 31) // 32):
        raise PqhError(-1, "ivf_regroup: keep is a contiguous int32 tensor of ceil(n / 32) words")
    dev = offsets.device
    new_offsets = torch.empty(nlist + 1, dtype=torch.int64, device=dev)
    dest = torch.empty(n, dtype=torch.int64, device=dev)
    add_base = torch.empty(nlist, dtype=torch.int64, device=dev)
    check(lib().pqh_ivf_regroup(ctx.ptr, _ptr(offsets), nlist, n, _ptr(keep), _ptr(add_offsets),
                                _ptr(new_offsets), _ptr(dest), _ptr(add_base)), "pqh_ivf_regroup")
    return new_offsets, dest, add_base


def ivf_status(ctx: Context) -> None:
    """raises PQH_ERR_ARG if a Coarse.layout / Coarse.probe / Coarse.residuals /
    adc_tables_residual / pack_mask / ivf_regroup / IdMap call since the last call met a bad
    value (a list id outside [0, nlist), a reversed offsets pair, a perm entry outside [0, n), a
    row or id an IdMap does not hold); synchronises
    (pqh_ivf_status)"""
    st = lib().pqh_ivf_status(ctx.ptr)
    if st:
        raise PqhError(st, "pqh_ivf")


def idmap_bytes(n: int, n_ids: int, nlist: int, reverse: bool = True) -> int:
    """the bytes of the id map of n rows in nlist lists with ids below n_ids (pqh_idmap_bytes;
    host arithmetic, runs without a GPU)"""
    out = ctypes.c_ulonglong(0)
    check(lib().pqh_idmap_bytes(n, n_ids, nlist, int(bool(reverse)), ctypes.byref(out)),
          "pqh_idmap_bytes")
    return out.value


class IdMap:
    """The ids of a list-ordered stream in Elias-Fano form (include/pqh.h, "compressed ids"):
    what an IVF's perm (stream row -> id) and inv (id -> stream row) hold, in about
    2 + log2(nlist) bits a row plus, with reverse=True, a list number per id.  perm: device
    int64 (n,), ascending inside every list; offsets: device int64 (nlist + 1,); both as
    Coarse.layout gives them.  Neither is kept, but for offsets as the default of rows().
    Async; ivf_status reports a perm the map cannot code (an id outside [0, n_ids), a list
    whose ids do not ascend).

    blob: the device uint8 tensor of the map; nbytes, n, n_ids, nlist, reverse."""

    def __init__(self, ctx: Context, perm, offsets, n_ids: int, reverse: bool = True):
        torch = _torch()
        for name, t in (("perm", perm), ("offsets", offsets)):
            if t.dtype != torch.int64 or t.dim() != 1 or not t.is_contiguous():
                raise PqhError(-1, f"IdMap: {name} is a contiguous int64 vector")
        self.ctx, self.offsets = ctx, offsets
        self.n, self.n_ids, self.nlist = perm.numel(), int(n_ids), offsets.numel() - 1
        self.reverse = bool(reverse)
        self.nbytes = idmap_bytes(self.n, self.n_ids, self.nlist, self.reverse)
        self.blob = torch.empty(self.nbytes, dtype=torch.uint8, device=offsets.device)
        check(lib().pqh_idmap_build(ctx.ptr, _ptr(perm), _ptr(offsets), self.n, self.nlist,
                                    self.n_ids, int(self.reverse), _ptr(self.blob), self.nbytes),
              "pqh_idmap_build")

    def _out(self, shape, out):
        torch = _torch()
        if out is None:
            return torch.empty(shape, dtype=torch.int64, device=self.blob.device)
        if out.dtype != torch.int64 or out.shape != shape or not out.is_contiguous():
            raise PqhError(-1, f"IdMap: out is a contiguous int64 tensor of shape {tuple(shape)}")
        return out

    def ids(self, rows, out=None):
        """the ids of the stream rows `rows` (device int64, any shape, any order, repeats
        allowed); a negative row is copied through, as the -1 padding of a search result is.
        Async; ivf_status reports a row >= n (its id is -1)."""
        torch = _torch()
        if rows.dtype != torch.int64:
            raise PqhError(-1, "IdMap.ids: rows is an int64 tensor")
        rows = rows.contiguous()
        out = self._out(rows.shape, out)
        check(lib().pqh_idmap_ids(self.ctx.ptr, _ptr(self.blob), _ptr(rows), rows.numel(),
                                  _ptr(out)), "pqh_idmap_ids")
        return out

    def rows(self, ids, offsets=None, out=None):
        """the stream rows of `ids` (device int64, any shape), -1 for an id without a row (one a
        compact() dropped); offsets: the lists' (default: those the map was built from).  Needs
        the reverse part.  Async; ivf_status reports an id outside [0, n_ids) (its row is -1)."""
        torch = _torch()
        if not self.reverse:
            raise PqhError(-1, "IdMap.rows: the map was built with reverse=False")
        offsets = self.offsets if offsets is None else offsets
        if (offsets.dtype != torch.int64 or not offsets.is_contiguous() or
                offsets.numel() != self.nlist + 1):
            raise PqhError(-1, "IdMap.rows: offsets is a contiguous int64 tensor of nlist + 1 entries")
        if ids.dtype != torch.int64:
            raise PqhError(-1, "IdMap.rows: ids is an int64 tensor")
        ids = ids.contiguous()
        out = self._out(ids.shape, out)
        check(lib().pqh_idmap_rows(self.ctx.ptr, _ptr(self.blob), _ptr(offsets), _ptr(ids),
                                   ids.numel(), _ptr(out)), "pqh_idmap_rows")
        return out

    def decode(self, first: int = 0, count: int = None, out=None):
        """the ids of the rows first ... first + count - 1 (count None: up to the last): perm, or
        a slice of it.  Async."""
        count = self.n - first if count is None else count
        if first < 0 or count < 0 or first + count > self.n:
            raise PqhError(-1, f"IdMap.decode: rows [{first}, {first + count}) of {self.n}")
        out = self._out((count,), out)
        check(lib().pqh_idmap_decode(self.ctx.ptr, _ptr(self.blob), first, count, _ptr(out)),
              "pqh_idmap_decode")
        return out

    def pack_mask(self, keep, out=None):
        """pack_mask(ctx, keep, perm) without perm: int32 (ceil(n / 32),), bit s & 31 of word
        s >> 5 = keep[id of row s].  keep: device bool or uint8 (n_ids,).  Async."""
        torch = _torch()
        if keep.dtype not in (torch.bool, torch.uint8) or keep.shape != (self.n_ids,):
            raise PqhError(-1, "IdMap.pack_mask: keep is a bool or uint8 tensor of shape (n_ids,)")
        keep = keep.contiguous()
        if out is None:
            out = torch.empty((self.n + 31) // 32, dtype=torch.int32, device=self.blob.device)
        elif (out.dtype != torch.int32 or not out.is_contiguous() or
              out.numel() != (self.n + 31) // 32):
            raise PqhError(-1, "IdMap.pack_mask: out is a contiguous int32 tensor of ceil(n / 32) words")
        check(lib().pqh_mask_pack_idmap(self.ctx.ptr, _ptr(keep), _ptr(self.blob), self.n,
                                        _ptr(out)), "pqh_mask_pack_idmap")
        return out


class IVF:
    """An inverted-file index over a compressed stream: the rows of x assigned to the lists
    of a coarse quantizer, stored list by list as one Huffman-coded PQ stream, and searched by
    probing each query's nearest lists.  ids are rows of the caller's x.

    The order of a result is (dist, stream row), that is (dist, list, caller row): rows of
    equal distance come list by list, NOT in caller-row order.

    residual=True (IVFADC): the stream holds the PQ codes of x - centroid[list], every
    (query, probed list) pair is scored with the table of query - centroid[list], and fetch()
    adds the centroid back.  `pq` must then be trained on residuals, e.g.
    kmeans_train(ctx, coarse.residuals(x, coarse.assign(x)), init, iters); a codebook trained
    on x itself works but throws the gain away.  The tables of a search are
    nq * nprobe * m * K * 4 bytes, so search() walks the queries in slabs whose tables stay
    under `table_budget` bytes.

    search(keep=...) searches a subset of the rows, and remove(ids) takes rows out of every
    later search (tombstones: the stream keeps them, the searches pass over them).  Both are a
    bit per stream row that the scan reads before it decodes: a chunk without a kept row is not
    decoded, a list without one costs the read of its mask words.

    refine_pq (IVFPQR): a second codebook over what `pq` leaves over of a row (train it on
    pq_residuals of the rows the first one codes) gives every row a second code, kept as a
    stream of its own (refine_tables, refine_enc).  search(refine=c) then takes the c <= 64 best
    (c <= 256 after ctx.set_search_max_k(256)) rows of the scan and returns the k best of them by the distance to the sum of both
    reconstructions (codec.refine); fetch(refined=True) returns that sum.

    add(x) appends rows and compact() drops the removed ones for good; both rebuild the streams
    from the streams themselves (ivf_regroup, decode_scatter, then histogram, tables and encode
    again), so the index is at any time what build() of its rows would be.  ids are stable:
    n_ids counts the ids ever given out, an id is never reused, and after a compact() the
    dropped ones are unknown to the index (inv holds -1 for them).

    range_search(queries, nprobe, radius) returns every row of the probed lists closer than
    radius, as many as there are (CSR: lims, dist, ids), where search() returns the k nearest.

    build(compress_ids=True) or compress_ids() keeps the ids as an IdMap (idmap; perm and inv
    are then None): 16 bytes a row become a few bits a row and a list number per id, and every
    method returns the same bits.  id_bytes() is what the ids cost either way.

    build(metric="ip") makes a maximum-inner-product index: rows go to the list of the largest
    inner product, every stage of search() and range_search() scores with the negated inner
    product (scores = -dist: smaller is still nearer, the order, the padding and the strict
    `dist < radius` are unchanged), and add() assigns its rows the same way.  The stream of a
    residual index still holds the codes of x - centroid[list]; its per-(query, list) tables
    are the query's plain table with the list's score folded into part 0.  The scans, the
    filters, remove(), compact(), compress_ids() and fetch() are the same code for both metrics.

    build(rotation=Rotation(ctx, R)) makes a rotated index (OPQ, opq_train): the index lives in
    the space of x @ R.  build() rotates x once at the top, add() its batch, search() and
    range_search() the queries (one small launch more), and fetch() rotates what it
    reconstructed back with R's transpose, refined=True included.  coarse, pq and refine_pq hold
    centroids of the rotated space: train them on rotation.apply(x), or take existing centroids
    there with rotation.apply.  Everything behind the rotation -- both metrics (R orthonormal
    keeps distances and inner products), residual, keep=, remove, compact, compress_ids, every
    schedule, refine= -- is the code of an unrotated index on rotated rows.  rotation=None, the
    default, launches what it launched before.

    Every stage is a call on the context's stream.  search() never waits for the device;
    range_search() waits once per slab of queries (once on a plain index), for the number of
    hits it has to allocate; build(), add() and compact() wait where encode() does, once per
    stream, for the stream's length."""

    table_budget = 256 << 20   # bytes of per-(query, list) tables a residual search holds at once
    # schedule="auto": list-major from nq * nprobe >= list_major_ratio * nlist on.  Measured at
    # 125M rows in 1,024 lists: in chunks of 4 rows the list form is
    # ahead from a ratio of 1 on (1.35x, 3.2x at 4, 5x at 8), in chunks of 64 from 4 on (0.68x at
    # 1, 1.6x at 4); 4.0 is the first point ahead on both.  With lists of under a thousand rows
    # the query-major form stays ahead up to a ratio of 32.
    list_major_ratio = 4.0

    def __init__(self, ctx, pq, coarse, tables, enc, perm, inv, offsets, residual=False,
                 metric="l2"):
        self.ctx, self.pq, self.coarse, self.tables, self.enc = ctx, pq, coarse, tables, enc
        self.perm, self.inv, self.offsets = perm, inv, offsets
        self.idmap = None           # compress_ids(): an IdMap in place of perm and inv
        self.n_ids = perm.numel()   # ids ever given out: inv's length; perm's until a compact()
        self.residual = residual
        self.metric = metric        # "l2" or "ip": how rows go to lists and how a search scores
        self.refine_pq = self.refine_tables = self.refine_enc = None   # build(refine_pq=...)
        self.rotation = None     # build(rotation=...): the index lives in the rotated space
        self.live = None         # remove(): device bool per stream row, allocated on first use
        self._live_words = None  # its packed form, made again after a remove()

    @classmethod
    def build(cls, ctx: Context, pq: PQ, coarse: Coarse, x, chunk_vectors: int = 64,
              context: bool = True, residual: bool = False, refine_pq: PQ = None,
              refine_chunk_vectors: int = None, compress_ids: bool = False,
              metric: str = "l2", rotation: "Rotation" = None) -> "IVF":
        """x: device float32 (n, d), d = coarse.d = pq.m * pq.dsub.  The stages: rows to
        lists, layout, gather x[perm] (residual: coarse.residuals(x, lists, perm) in its
        place), pq.assign, histogram, Tables.build, encode.  refine_pq: what pq leaves over
        (rows - pq.reconstruct(codes), in place) goes through the same four stages with
        refine_pq, in chunks of refine_chunk_vectors (default: chunk_vectors).  compress_ids:
        the index keeps its ids as an IdMap (compress_ids()).  metric: "l2" or "ip" (see the
        class).  rotation: the index lives in the rotated space (see the class) -- x is rotated
        once at the top, into one extra n x d buffer that lives until build() returns, and
        coarse, pq and refine_pq must hold centroids of rotated rows; PqhError if rotation.d is
        not d or rotation.defect() > 1e-3 (rounding an orthonormal matrix to float32 leaves
        about d * 2^-24 <= 6e-5)."""
        torch = _torch()
        _metric_suffix(metric, "IVF.build")
        if rotation is not None:
            if rotation.d != x.shape[1]:
                raise PqhError(-1, "IVF.build: the rotation and x disagree in d")
            if not rotation.defect() <= 1e-3:
                raise PqhError(-1, "IVF.build: the rotation is not orthonormal (defect > 1e-3)")
        if pq.k > 256 or pq.m > 16:
            raise PqhError(-4, "IVF.build: the search takes K <= 256 and m <= 16")
        if coarse.d != pq.m * pq.dsub or x.shape[1] != coarse.d:
            raise PqhError(-1, "IVF.build: x, the coarse centroids and the PQ disagree in d")
        if refine_pq is not None:
            if refine_pq.k > 256 or refine_pq.m > 16:
                raise PqhError(-4, "IVF.build: the re-rank takes K <= 256 and m <= 16")
            if refine_pq.m * refine_pq.dsub != coarse.d:
                raise PqhError(-1, "IVF.build: refine_pq and the PQ disagree in d")
        if rotation is not None:
            x = rotation.apply(x)
        lists = coarse.assign(x, metric=metric)
        perm, offsets = coarse.layout(lists)
        rows = coarse.residuals(x, lists, perm) if residual else x[perm]
        codes = pq.assign(rows, ctx=ctx)
        refined = None
        if refine_pq is not None:
            rows.sub_(pq.reconstruct(codes))
            codes2 = refine_pq.assign(rows, ctx=ctx)
            tables2 = Tables(ctx, refine_pq.m, refine_pq.k, context).build(
                histogram(ctx, codes2, refine_pq.k, context))
            refined = (tables2, encode(ctx, tables2, codes2,
                                       chunk_vectors=refine_chunk_vectors or chunk_vectors))
        del rows
        counts = histogram(ctx, codes, pq.k, context)
        tables = Tables(ctx, pq.m, pq.k, context).build(counts)
        enc = encode(ctx, tables, codes, chunk_vectors=chunk_vectors)
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(perm.numel(), dtype=torch.int64, device=perm.device)
        ivf = cls(ctx, pq, coarse, tables, enc, perm, inv, offsets, residual, metric)
        ivf.rotation = rotation
        if refined is not None:
            ivf.refine_pq, (ivf.refine_tables, ivf.refine_enc) = refine_pq, refined
        if compress_ids:
            ivf.compress_ids()
        return ivf

    def compress_ids(self) -> int:
        """keep the ids as an IdMap (Elias-Fano, with the reverse part) in place of perm and inv,
        which become None; returns the bytes freed.  Every method gives the same bits as before;
        the lookups at the end of a search are one launch, keep= is packed through the map, and
        add() and compact() decode perm for the length of the call and build a new map.  On an
        index that is compressed already nothing is touched.  Async; ivf_status would report
        ids that do not ascend inside a list, which no index of build(), add() and compact()
        has."""
        if self.idmap is not None:
            return 0
        before = self.id_bytes()
        self.idmap = IdMap(self.ctx, self.perm, self.offsets, self.n_ids)
        self.perm = self.inv = None
        return before - self.id_bytes()

    def id_bytes(self) -> int:
        """the bytes of the id structures the index holds: perm and inv, or the IdMap"""
        if self.idmap is not None:
            return self.idmap.nbytes
        return (self.perm.numel() * self.perm.element_size() +
                self.inv.numel() * self.inv.element_size())

    def _ids_of(self, rows, padded: bool = True):
        """stream rows to ids; padded: rows may hold the -1 of a search result"""
        torch = _torch()
        if self.idmap is not None:
            return self.idmap.ids(rows)
        if not padded:
            return self.perm[rows]
        return torch.where(rows >= 0, self.perm[rows.clamp(min=0)], rows)

    def _rows_of(self, ids):
        """ids to stream rows (-1: an id a compact() dropped)"""
        if self.idmap is not None:
            return self.idmap.rows(ids, self.offsets)
        return self.inv[ids]

    def _perm(self):
        """perm, decoded for the length of a call where the index holds an IdMap"""
        return self.perm if self.idmap is None else self.idmap.decode()

    def remove(self, ids) -> None:
        """take the caller rows `ids` (device int64, each in [0, n)) out of every later search,
        with or without keep=.  Tombstones: a live flag per stream row is cleared, the stream
        is not rebuilt, so fetch() still returns a removed row and the index does not shrink
        (compact() does that).  Removing a row twice is harmless, and so is an id that a
        compact() has dropped.  Async, but for the pass over such ids on a compacted index."""
        torch = _torch()
        if self.live is None:
            self.live = torch.ones(self.enc.n, dtype=torch.bool, device=self.offsets.device)
        rows = self._rows_of(ids.reshape(-1))
        if self.enc.n != self.n_ids:   # compacted: a dropped id has no row
            rows = rows[rows >= 0]
        self.live[rows] = False
        self._live_words = pack_mask(self.ctx, self.live)

    def _stage_batch(self, x):
        """(perm, offsets, list of every sorted row, codes, level-2 codes or None) of a batch of
        new rows, the codes in the batch's own list order: the stages of build()"""
        if self.rotation is not None:
            x = self.rotation.apply(x)
        lists = self.coarse.assign(x, metric=self.metric)
        perm, offsets = self.coarse.layout(lists)
        rows = self.coarse.residuals(x, lists, perm) if self.residual else x[perm]
        codes = self.pq.assign(rows, ctx=self.ctx)
        codes2 = None
        if self.refine_pq is not None:
            rows.sub_(self.pq.reconstruct(codes))
            codes2 = self.refine_pq.assign(rows, ctx=self.ctx)
        return perm, offsets, lists[perm].long(), codes, codes2

    def _recode(self, tables, enc, dest, n_new: int, slots=None, codes=None):
        """(tables, enc) of the stream `enc` taken through the plan `dest` into n_new rows, with
        `codes` stored at rows `slots`: decode_scatter, histogram, Tables.build, encode"""
        torch = _torch()
        merged = torch.empty((n_new, tables.m), dtype=torch.uint8, device=self.offsets.device)
        decode_scatter(self.ctx, tables, enc, dest, merged)
        if slots is not None:
            merged[slots] = codes
        new_tables = Tables(self.ctx, tables.m, tables.k, tables.context).build(
            histogram(self.ctx, merged, tables.k, tables.context))
        new_enc = encode(self.ctx, new_tables, merged, chunk_vectors=enc.chunk_vectors)
        decode_status(self.ctx)
        return new_tables, new_enc

    def _rebuild(self, keep, batch, n_new: int):
        """both streams through one plan (ivf_regroup with the mask `keep` and the batch's
        offsets); returns what replaces the index's state, which is touched by the caller only"""
        torch = _torch()
        n = self.enc.n
        new_offsets, dest, add_base = ivf_regroup(
            self.ctx, self.offsets, keep, None if batch is None else batch[1], n=n)
        slots = codes = codes2 = None
        if batch is not None:
            b_perm, b_offsets, b_lists, codes, codes2 = batch
            rank = torch.arange(b_perm.numel(), dtype=torch.int64, device=b_perm.device)
            slots = add_base[b_lists] + (rank - b_offsets[b_lists])
        level1 = self._recode(self.tables, self.enc, dest, n_new, slots, codes)
        level2 = None
        if self.refine_pq is not None:
            level2 = self._recode(self.refine_tables, self.refine_enc, dest, n_new, slots, codes2)
        ivf_status(self.ctx)
        return new_offsets, dest, slots, level1, level2

    def _commit(self, n_ids: int, new_offsets, perm, live, level1, level2):
        torch = _torch()
        if self.idmap is not None:   # a new map of the new perm: never patched, B and L may change
            idmap, perm, inv = IdMap(self.ctx, perm, new_offsets, n_ids), None, None
        else:
            idmap = None
            inv = torch.full((n_ids,), -1, dtype=torch.int64, device=perm.device)
            inv[perm] = torch.arange(perm.numel(), dtype=torch.int64, device=perm.device)
        self.n_ids, self.idmap = n_ids, idmap
        self.tables, self.enc = level1
        if level2 is not None:
            self.refine_tables, self.refine_enc = level2
        self.perm, self.inv, self.offsets = perm, inv, new_offsets
        self.live = live
        self._live_words = None if live is None else pack_mask(self.ctx, live)

    def add(self, x) -> int:
        """append the rows of x (device float32 (n_add, d)); returns the id of the first, the
        rows get the ids n_ids ... n_ids + n_add - 1.  The index is afterwards what build() of
        all its rows gives, stream for stream: the new rows go through build()'s stages (rows to
        lists, layout, residuals, pq.assign, the level-2 codes), the old stream is decoded
        straight into the merged list order (ivf_regroup, decode_scatter), and histogram, tables
        and encode run again with the index's own chunk_vectors and context.  So the cost is
        O(n + n_add) per call, everything is re-coded: add in large batches.  Rows taken out by
        remove() stay stored and stay out; add() drops nothing.  Waits where encode() does, once
        per stream.  A PqhError leaves the index as it was.  n_add == 0 does nothing."""
        torch = _torch()
        n_add = x.shape[0]
        first = self.n_ids
        if n_add == 0:
            return first
        if x.dim() != 2 or x.shape[1] != self.coarse.d:
            raise PqhError(-1, "IVF.add: x, the coarse centroids and the PQ disagree in d")
        n = self.enc.n
        batch = self._stage_batch(x)
        new_offsets, dest, slots, level1, level2 = self._rebuild(None, batch, n + n_add)
        perm = torch.empty(n + n_add, dtype=torch.int64, device=self.offsets.device)
        perm[dest] = self._perm()
        perm[slots] = batch[0] + first
        live = None
        if self.live is not None:
            live = torch.ones(n + n_add, dtype=torch.bool, device=self.offsets.device)
            live[dest] = self.live
        self._commit(first + n_add, new_offsets, perm, live, level1, level2)
        return first

    def compact(self) -> int:
        """drop the rows remove() took out for good; returns how many.  The streams, perm and
        offsets shrink to the live rows -- the same pass as add(), with the live words as the
        mask and no new rows, so the cost is O(n) -- and the live flags are reset.  ids stay
        what they were: perm holds the caller's ids, inv keeps n_ids entries with -1 for the
        dropped ones, which remove() then ignores, fetch() reports (see there) and keep= still
        has an entry for.  Without a removed row nothing is touched.  Waits where encode() does,
        once per stream, and once for the count.  A PqhError leaves the index as it was."""
        if self.live is None:
            return 0
        n = self.enc.n
        n_live = int(self.live.sum().item())
        if n_live == n:
            return 0
        new_offsets, _, _, level1, level2 = self._rebuild(self._live_words, None, n_live)
        self._commit(self.n_ids, new_offsets, self._perm()[self.live], None, level1, level2)
        return n - n_live

    def live_count(self) -> int:
        """the rows remove() has left (synchronises once a row was removed)"""
        return self.enc.n if self.live is None else int(self.live.sum().item())

    def _mask(self, keep):
        """the words of keep (bool over the ids, packed through perm into stream order) ANDed
        with those of the live rows; None: no filter"""
        torch = _torch()
        if keep is None:
            return self._live_words
        if keep.dtype != torch.bool or keep.shape != (self.n_ids,):
            raise PqhError(-1, "IVF.search: keep is a bool tensor of shape (n_ids,)")
        if self.idmap is not None:
            words = self.idmap.pack_mask(keep)
        elif self.perm.numel() == self.n_ids:
            words = pack_mask(self.ctx, keep, self.perm)
        else:   # compacted: fewer rows than ids, so the gather comes first
            words = pack_mask(self.ctx, keep[self.perm])
        return words if self._live_words is None else words & self._live_words

    def search(self, queries, nprobe: int, k: int, schedule: str = "query", keep=None,
               refine: int = 0):
        """(dist, ids), each (nq, k): the k nearest rows by ADC distance among the rows of each
        query's nprobe nearest lists; ids are rows of the caller's x, padded with (+inf, -1).
        schedule: "query" decodes a list once for every query that probes it (search_ranges),
        "list" once per batch of the queries that probe it (search_lists), "auto" takes "list"
        from nq * nprobe >= list_major_ratio * nlist on; the result is the same bits.
        keep: device bool (n_ids,) over the ids (the caller's rows of x): only rows with keep[id] set are
        returned -- the k nearest among them, not the kept ones of the k nearest.  Rows taken
        out by remove() are never returned.
        refine: 0, or the number c of candidates, k <= c <= ctx.search_max_k, on an index built
        with
        refine_pq: the scan returns its c best rows and the k best of those by the refined
        distance (both levels' reconstructions added, codec.refine) are the result, their
        distances the refined ones."""
        torch = _torch()
        if schedule not in ("query", "list", "auto"):
            raise PqhError(-1, f"IVF.search: schedule {schedule!r}")
        if refine:
            if self.refine_pq is None:
                raise PqhError(-1, "IVF.search: refine > 0 on an index built without refine_pq")
            limit = self.ctx.search_max_k
            if not k <= refine <= limit:
                raise PqhError(-1, f"IVF.search: refine = {refine} outside [k, {limit}]")
            top_k, k = k, refine
        by_list = schedule == "list" or (
            schedule == "auto" and
            queries.shape[0] * nprobe >= self.list_major_ratio * self.coarse.nlist)
        mask = self._mask(keep)
        if self.rotation is not None:
            queries = self.rotation.apply(queries)
        if self.residual:
            dist, rows = self._search_residual(queries, nprobe, k, by_list, mask,
                                               top_k if refine else 0)
            return dist, self._ids_of(rows)
        lut = adc_tables(self.ctx, self.pq, queries, metric=self.metric)
        range_ptr, ranges, probes, _ = self.coarse.probe(queries, nprobe, self.offsets,
                                                         lists=by_list, metric=self.metric)
        if by_list:
            dist, rows = search_lists(self.ctx, self.tables, self.enc, lut, self.offsets, probes, k,
                                      keep=mask)
        else:
            dist, rows = search_ranges(self.ctx, self.tables, self.enc, lut, range_ptr, ranges, k,
                                       keep=mask)
        if refine:
            dist, rows = self._refine(queries, rows, top_k)
        return dist, self._ids_of(rows)

    def _refine(self, queries, rows, k: int, out=None):
        """(dist, stream rows): the k best of the scan's candidate rows by both levels' codes"""
        return _refine(self.ctx, (self.tables, self.pq, self.enc),
                       (self.refine_tables, self.refine_pq, self.refine_enc), queries, rows, k,
                       self.coarse if self.residual else None,
                       self.offsets if self.residual else None, out, self.metric)

    def _search_residual(self, queries, nprobe: int, k: int, by_list: bool = False, mask=None,
                         refine_k: int = 0):
        """(dist, stream rows): probe, one table per (query, list), the probe search with a
        table per range (by_list: per pair, list-major) -- slab by slab, the table buffer reused;
        mask: the words of the rows that may be returned, the same for every slab; refine_k > 0:
        every slab's k candidates re-ranked to refine_k results"""
        torch = _torch()
        nq = queries.shape[0]
        per_query = nprobe * self.pq.m * self.pq.k * 4
        slab = max(1, min(max(nq, 1), int(self.table_budget) // per_query))
        dist = torch.empty((nq, k), dtype=torch.float32, device=queries.device)
        rows = torch.empty((nq, k), dtype=torch.int64, device=queries.device)
        if refine_k:
            fine = (torch.empty((nq, refine_k), dtype=torch.float32, device=queries.device),
                    torch.empty((nq, refine_k), dtype=torch.int64, device=queries.device))
        lut = torch.empty((slab * nprobe, self.pq.m, self.pq.k), dtype=torch.float32,
                          device=queries.device)
        for s in range(0, nq, slab):
            q = queries[s:s + slab]
            range_ptr, ranges, probes, _ = self.coarse.probe(q, nprobe, self.offsets, lists=True,
                                                             metric=self.metric)
            adc_tables_residual(self.ctx, self.pq, self.coarse, q, probes,
                                out=lut[:q.shape[0] * nprobe], metric=self.metric)
            out = (dist[s:s + slab], rows[s:s + slab])
            if by_list:
                search_lists(self.ctx, self.tables, self.enc, lut[:q.shape[0] * nprobe],
                             self.offsets, probes, k, out=out, keep=mask)
            else:
                search_range_tables(self.ctx, self.tables, self.enc, lut, range_ptr, ranges, k,
                                    out=out, keep=mask)
            if refine_k:
                self._refine(q, out[1], refine_k, out=(fine[0][s:s + slab], fine[1][s:s + slab]))
        return fine if refine_k else (dist, rows)

    def range_search(self, queries, nprobe: int, radius, keep=None):
        """(lims, dist, ids): every row of each query's nprobe nearest lists with an ADC distance
        below radius (codec.range_search_ranges: strict, CSR, as many hits as there are); ids are
        rows of the caller's x, a query's hits list by list in the order of its probes, in
        stream order inside a list.  radius: a float, or a device float32 tensor (nq,).  keep
        and remove() act as in search().  A residual index scores every (query, list) pair with
        its own table, slab by slab under table_budget, and the slabs' results are concatenated.
        Unlike search(), it waits for the device: once per slab (once for a plain index), for
        the number of hits."""
        torch = _torch()
        nq = queries.shape[0]
        mask = self._mask(keep)
        if self.rotation is not None:
            queries = self.rotation.apply(queries)
        if torch.is_tensor(radius):
            if radius.dtype != torch.float32 or radius.shape != (nq,):
                raise PqhError(-1, "IVF.range_search: radius is a float or a float32 tensor (nq,)")
        else:
            radius = torch.full((nq,), float(radius), dtype=torch.float32, device=queries.device)
        if not self.residual:
            lut = adc_tables(self.ctx, self.pq, queries, metric=self.metric)
            range_ptr, ranges, _, _ = self.coarse.probe(queries, nprobe, self.offsets, lists=False,
                                                        metric=self.metric)
            lims, dist, rows = range_search_ranges(self.ctx, self.tables, self.enc, lut, range_ptr,
                                                   ranges, radius, keep=mask)
            return lims, dist, self._ids_of(rows, padded=False)
        per_query = nprobe * self.pq.m * self.pq.k * 4
        slab = max(1, min(max(nq, 1), int(self.table_budget) // per_query))
        lut = torch.empty((slab * nprobe, self.pq.m, self.pq.k), dtype=torch.float32,
                          device=queries.device)
        lims = torch.zeros(nq + 1, dtype=torch.int64, device=queries.device)
        parts = []
        for s in range(0, nq, slab):
            q = queries[s:s + slab]
            range_ptr, ranges, probes, _ = self.coarse.probe(q, nprobe, self.offsets, lists=True,
                                                             metric=self.metric)
            adc_tables_residual(self.ctx, self.pq, self.coarse, q, probes,
                                out=lut[:q.shape[0] * nprobe], metric=self.metric)
            l, d, r = range_search_ranges(self.ctx, self.tables, self.enc, lut, range_ptr, ranges,
                                          radius[s:s + slab], tables_per_range=True, keep=mask)
            lims[s + 1:s + 1 + q.shape[0]] = l[1:] + lims[s]
            parts.append((d, r))
        if not parts:
            return (lims, torch.empty(0, dtype=torch.float32, device=queries.device),
                    torch.empty(0, dtype=torch.int64, device=queries.device))
        dist = torch.cat([p[0] for p in parts])
        return lims, dist, self._ids_of(torch.cat([p[1] for p in parts]), padded=False)

    def fetch(self, ids, out=None, refined: bool = False):
        """the reconstructed vectors of caller rows `ids` (device int64, each in [0, n)): what
        the index knows of them (fetch through the inverse permutation; residual: the decoded
        residual plus the centroid of the stream row's list, one fp32 add).  refined=True, on an
        index built with refine_pq: the level-2 reconstruction is fetched too and added first,
        (c1 + c2) and then + centroid -- the vectors search(refine=...) measures against.
        remove() does not affect it: the stream still holds a removed row.  After a compact()
        it does not: the row of a dropped id comes back as zeros (residual: the first list's
        centroid) and decode_status reports PQH_ERR_ARG, as for any id the index does not know."""
        torch = _torch()
        if refined and self.refine_pq is None:
            raise PqhError(-1, "IVF.fetch: refined=True on an index built without refine_pq")
        rows = self._rows_of(ids.reshape(-1))
        back, out = out, (out if self.rotation is None else None)
        out = fetch(self.ctx, self.tables, self.pq, self.enc, rows, out)
        if refined:
            out[:, :self.coarse.d] += fetch(self.ctx, self.refine_tables, self.refine_pq,
                                            self.refine_enc, rows)
        if self.residual:
            # (right=True passes over the empty lists that end where the row's list begins)
            lists = torch.searchsorted(self.offsets[1:].contiguous(), rows, right=True)
            out[:, :self.coarse.d] += self.coarse.centroids[lists]
        if self.rotation is not None:   # what was reconstructed, taken back to the caller's axes
            out = self.rotation.apply(out, out=back, transpose=True)
        return out


def encode_status(ctx: Context) -> None:
    st = lib().pqh_encode_status(ctx.ptr)
    if st:
        raise PqhError(st, "pqh_encode_write")


def decode_status(ctx: Context) -> None:
    st = lib().pqh_decode_status(ctx.ptr)
    if st:
        raise PqhError(st, "pqh_decode")


def indices_file_bytes(enc: Encoded) -> bytes:
    """huffman_indices.bin content: u64 N + stream bytes."""
    body = enc.stream[:enc.nbytes].cpu().numpy().tobytes()
    return np.uint64(enc.n).tobytes() + body


# ---- tree-ordered context coding (huffman_encoder.c --tree; mst.c:253-490) ---------------
def load_tree(path: str):
    """mst.tree (tree_save_file, mst.c:253-265): i64 N, i64 E, u32 targets[E], i32 counts[N].
    Returns (n, targets, counts)."""
    with open(path, "rb") as fh:
        raw = fh.read()
    n, e = (int(v) for v in np.frombuffer(raw[:16], np.int64))
    if len(raw) < 16 + 4 * e + 4 * n:
        raise ValueError(f"{path}: truncated tree file")
    targets = np.frombuffer(raw[16:16 + 4 * e], np.uint32).copy()
    counts = np.frombuffer(raw[16 + 4 * e:16 + 4 * e + 4 * n], np.int32).copy()
    return n, targets, counts


def tree_order(targets, counts):
    """DFS order of the forest (tree_collect_vertices_dfs, mst.c:290-364) and each stream
    row's coding context (tree_traverser, mst.c:366-405), by the library's host walk.
    Returns (vertices u32[n], num_children i32[n], parents i64[n] (-1: root), num_roots)."""
    targets = np.ascontiguousarray(targets, np.uint32)
    counts = np.ascontiguousarray(counts, np.int32)
    n = len(counts)
    vert = np.zeros(max(n, 1), np.uint32)
    nch = np.zeros(max(n, 1), np.int32)
    par = np.zeros(max(n, 1), np.int64)
    roots = lib().pqh_tree_order(n, len(targets), _ptr(targets), _ptr(counts), _ptr(vert),
                                 _ptr(nch), _ptr(par))
    if roots < 0:
        raise PqhError(roots, "pqh_tree_order: malformed forest")
    return vert[:n], nch[:n], par[:n], roots


def tree_order_device(ctx: Context, targets, counts):
    """tree_order on the device (pqh_tree_order_device): targets / counts as host arrays or
    device tensors.  Returns (vertices i32, num_children i32, parents i64) device tensors and
    num_roots, or None when the graph is not a forest (tree_order walks any graph)."""
    torch = _torch()
    dev = torch.device("cuda", ctx.device)
    t = torch.as_tensor(np.asarray(targets, np.uint32).view(np.int32)
                        if not torch.is_tensor(targets) else targets).to(dev, torch.int32)
    c = torch.as_tensor(np.asarray(counts, np.int32) if not torch.is_tensor(counts)
                        else counts).to(dev, torch.int32)
    n = c.numel()
    vert = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    nch = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    par = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    roots = ctypes.c_int(0)
    rc = lib().pqh_tree_order_device(ctx.ptr, n, t.numel(), _ptr(t), _ptr(c), _ptr(vert),
                                     _ptr(nch), _ptr(par), ctypes.byref(roots))
    if rc == -4:   # PQH_ERR_UNSUPPORTED
        return None
    check(rc, "pqh_tree_order_device: " + ctx.last_error())
    return vert[:n], nch[:n], par[:n], roots.value


@dataclass
class TreeEncoded:
    stream: object             # device uint8 (huffman_indices.bin payload), padded to 4 B
    bits: int
    n: int
    num_roots: int
    tables: object             # Tables (context, m parts)
    vertices: np.ndarray       # stream row p is input row vertices[p]
    num_children: np.ndarray
    children_codebook: object  # Codebooks (one non-context book, alphabet max + 1)
    children: object           # Encoded: the children stream (huffman_children.bin)
    chunk_vectors: int = 0     # decode sidecar: chunk bit offsets (device int64 [chunks])
    chunk_offsets: object = None
    ext_rows: object = None    # device uint8 [ext, m]: contexts that precede their chunk

    @property
    def nbytes(self) -> int:
        return (self.bits + 7) // 8


def tree_ext_index(num_children, chunk_vectors: int):
    """(parent_pos i64[n], ext_offsets i64[chunks + 1], ext_positions i64[ext]) -- the
    decode-side index of a tree stream (pqh_tree_ext_index)."""
    nch = np.ascontiguousarray(num_children, np.int32)
    n = len(nch)
    chunks = (n + chunk_vectors - 1) // chunk_vectors
    pp = np.zeros(max(n, 1), np.int64)
    eo = np.zeros(chunks + 1, np.int64)
    cnt = lib().pqh_tree_ext_index(n, _ptr(nch), chunk_vectors, _ptr(pp), _ptr(eo), None)
    if cnt < 0:
        raise PqhError(int(cnt), "pqh_tree_ext_index")
    ep = np.zeros(max(cnt, 1), np.int64)
    lib().pqh_tree_ext_index(n, _ptr(nch), chunk_vectors, _ptr(pp), _ptr(eo), _ptr(ep))
    return pp[:n], eo, ep[:cnt]


def tree_encode(ctx: Context, codes, targets, counts, chunk_vectors: int = 16) -> TreeEncoded:
    """Tree mode of huffman_encoder (huffman_encoder.c:321-375, encode_tree_data :240-286)
    on device uint8 codes [n, m]: DFS order (device Euler tour; the host walk for a graph
    that is not a forest) -> device gather of the rows in stream order
    beside their parents' codes -> parent/child pair histogram -> GPU code tables -> one-pass
    encode with explicit contexts; plus the children-count stream (non-context code book of
    tree_collect_num_children_stats, mst.c:407-440, coded by the GPU encoder).
    chunk_vectors: rows per decode lane (16: ~4x the lanes of 64 at ~10 % more sidecar)."""
    torch = _torch()
    n, m = codes.shape
    if len(counts) != n:
        raise ValueError(f"tree has {len(counts)} vertices for {n} rows")
    dev = codes.device
    order = tree_order_device(ctx, targets, counts)
    if order is not None:
        d_vert, d_nch, d_par, roots = order
        vert, nch = d_vert.cpu().numpy().view(np.uint32), d_nch.cpu().numpy()
    else:   # not a forest: the host walk reproduces the reference's DFS on any graph
        vert, nch, par, roots = tree_order(targets, counts)
        d_vert = torch.from_numpy(vert.astype(np.int32)).to(dev)
        d_par = torch.from_numpy(par).to(dev)
        d_nch = torch.from_numpy(np.ascontiguousarray(nch, np.int32)).to(dev)
    rows = torch.empty((n, m), dtype=torch.uint8, device=dev)
    prev = torch.empty((n, m), dtype=torch.int16, device=dev)
    check(lib().pqh_tree_gather(ctx.ptr, _ptr(codes), n, m, 256, _ptr(d_vert), _ptr(d_par),
                                _ptr(rows), _ptr(prev)), "pqh_tree_gather")
    check(lib().pqh_tree_status(ctx.ptr), "pqh_tree_gather: " + ctx.last_error())
    cnt = torch.zeros((m, 256 * 256), dtype=torch.int32, device=dev)
    check(lib().pqh_histogram_tree(ctx.ptr, _ptr(rows), _ptr(prev), n, m, 256, _ptr(cnt)),
          "pqh_histogram_tree")
    tables = Tables(ctx, m, 256, True).build(cnt)
    tables.status()
    words = (n * m * 56 + 31) // 32 + 2          # 56-bit codes at most
    out = torch.zeros(words * 4, dtype=torch.uint8, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    chunks = (n + chunk_vectors - 1) // chunk_vectors
    coff = torch.empty(max(chunks, 1), dtype=torch.int64, device=dev)
    check(lib().pqh_encode_tree_write(ctx.ptr, tables.ptr, _ptr(rows), _ptr(prev), n, 0,
                                      _ptr(out), out.numel(), chunk_vectors, _ptr(coff),
                                      _ptr(total)),
          "pqh_encode_tree_write: " + ctx.last_error())
    # decode sidecar: the contexts each chunk needs from before it (the encoder has them)
    _, _, _, ext_pos = tree_ext_index_device(ctx, d_nch, chunk_vectors, positions=True)
    ext_rows = rows.index_select(0, ext_pos)
    encode_status(ctx)
    bits = int(total.item())
    # children stream: one non-context part over the child counts
    alphabet = int(nch.max(initial=0)) + 1
    if alphabet > 4096:
        raise PqhError(-4, f"tree_encode: {alphabet - 1} children at one vertex (max 4095)")
    ccounts = np.bincount(nch, minlength=alphabet).astype(np.float64)[None]
    cbook = Codebooks(ccounts, alphabet, False)
    ctab = Tables.from_codebooks(ctx, cbook)
    ccodes = d_nch.to(torch.uint8 if alphabet <= 256 else torch.int16).reshape(n, 1)
    children = encode(ctx, ctab, ccodes, chunk_vectors=64, raw_first=1)
    return TreeEncoded(out, bits, n, roots, tables, vert, nch, cbook, children, chunk_vectors,
                       coff, ext_rows)


def tree_ext_index_device(ctx: Context, num_children, chunk_vectors: int,
                          positions: bool = False):
    """tree_ext_index on the device (pqh_tree_ext_index_device) from a device tensor of child
    counts (uint8, int16-as-u16 or int32): (parent_pos i64[n], ext_offsets i64[chunks + 1])
    device tensors and the ext count -- plus ext_positions i64[ext] with positions=True."""
    torch = _torch()
    nch = num_children.contiguous()
    n = nch.numel()
    nbytes = {torch.uint8: 1, torch.int16: 2, torch.int32: 4}[nch.dtype]
    chunks = (n + chunk_vectors - 1) // chunk_vectors
    pp = torch.empty(max(n, 1), dtype=torch.int64, device=nch.device)
    eo = torch.empty(chunks + 1, dtype=torch.int64, device=nch.device)
    ep = torch.empty(max(n, 1), dtype=torch.int64, device=nch.device) if positions else None
    ext = lib().pqh_tree_ext_index_device(ctx.ptr, n, _ptr(nch), nbytes, chunk_vectors,
                                          _ptr(pp), _ptr(eo), _ptr(ep) if positions else None)
    if ext < 0:
        raise PqhError(int(ext), "pqh_tree_ext_index_device: " + ctx.last_error())
    if positions:
        return pp[:n], eo, int(ext), ep[:ext]
    return pp[:n], eo, int(ext)


def tree_decode(ctx: Context, enc: TreeEncoded, tables: Tables = None, out=None,
                stream_bytes: int = None):
    """huffman_decoder --tree on the GPU (huffman_decoder.c:214-247): the children stream
    first (GPU decode of its non-context book), then the traverser's index over the decoded
    child counts (on the device), then one lane per chunk with the encoder's sidecar.  Rows come back in
    stream (DFS) order, as the reference decoder writes them.  stream_bytes (default: the
    encoded length) bounds the bits the decoder may consume: a stream shorter than its
    sidecar says raises PqhError (PQH_ERR_CORRUPT)."""
    torch = _torch()
    t = tables or enc.tables
    ctab = Tables.from_codebooks(ctx, enc.children_codebook)
    nch = decode(ctx, ctab, enc.children)
    decode_status(ctx)
    # the traverser's index on the device, from the decoded child counts in place
    d_pp, d_eo, _ = tree_ext_index_device(ctx, nch.reshape(-1), enc.chunk_vectors)
    dev = enc.stream.device
    if out is None:
        out = torch.empty((enc.n, t.m), dtype=torch.uint8, device=dev)
    nb = enc.nbytes if stream_bytes is None else stream_bytes
    check(lib().pqh_decode_tree(ctx.ptr, t.ptr, _ptr(enc.stream), nb, enc.n,
                                enc.chunk_vectors, _ptr(enc.chunk_offsets), _ptr(d_pp),
                                _ptr(d_eo), _ptr(enc.ext_rows), _ptr(out)), "pqh_decode_tree")
    decode_status(ctx)
    return out


def tree_files(enc: TreeEncoded) -> dict:
    """The reference's tree-mode output files (huffman_encoder.c:343-375, :398-428)."""
    cb = enc.tables.codebooks()
    stream = enc.stream[:enc.nbytes].cpu().numpy().tobytes()
    cstream = enc.children.stream[:enc.children.nbytes].cpu().numpy().tobytes()
    return {"huffman_codebooks.bin": cb.file_bytes(),
            "huffman_indices.bin": np.uint64(enc.n).tobytes() + stream,
            "huffman_children_codebooks.bin": enc.children_codebook.file_bytes()[4:],
            "huffman_children.bin": cstream}
