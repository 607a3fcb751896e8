// pqh_regroup.hip -- a list-ordered stream taken to a new list order, with rows dropped and gaps
// left for new rows, without the old codes being materialised in their old order: the plan
// (pqh_ivf_regroup) and the decode through it (pqh_decode_scatter).  IVF.add and IVF.compact
// (codec.py) are these two calls, a histogram, a table build and an encode.
//
//  keep_popc     the kept bits of every mask word; rocPRIM's exclusive scan of them gives
//                W[w] = the kept rows before word w, so that
//                    P(r) = W[r >> 5] + popc(keep[r >> 5] & ((1 << (r & 31)) - 1))
//                is the number of kept rows before row r (no mask: P(r) = r).
//  regroup_plan  the lists of a stream are contiguous, so the kept rows before list l are
//                P(offsets[l]) and the added rows before it add_offsets[l]:
//                    new_offsets[l] = P(offsets[l]) + add_offsets[l]
//                    add_base[l]    = P(offsets[l + 1]) + add_offsets[l]
//                    dest[r]        = P(r) + add_offsets[list of r]     (kept; else -1)
//                One thread per row and per list, no pass over a list by one thread or wave: a
//                list of any length costs what its rows cost.  The list of a row (the last l
//                with offsets[l] <= r, a binary search) is needed only with add_offsets.
//  scat_rows     the decoder's row walk (pqh_decode_dev.h) with a scattered write-back: one lane
//                per chunk, the chunk walked up to its last row with a destination, the
//                workgroup's rows staged in LDS and stored row by row at dest[r], the lanes of
//                a row on consecutive words, so neighbouring rows with consecutive destinations
//                are one contiguous store.
#include <rocprim/device/device_scan.hpp>

#include <algorithm>

#include "pqh_internal.h"
#include "pqh_decode_dev.h"

namespace {

// ------------------------------------------------------------------- the plan
// cnt[w] = popc(keep[w]) for w < nw, cnt[nw] = 0 (so the scan's last entry is the total).  The
// bits from n on in the last word are never counted into a P(r) that is used: P(r) looks below
// bit r & 31 only, and W[nw] is read only for r = n a multiple of 32.
__global__ void __launch_bounds__(256)
keep_popc(const uint32_t* __restrict__ keep, long long nw, uint32_t* __restrict__ cnt) {
    const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
    if (w <= nw) cnt[w] = w < nw ? (uint32_t)__popc(keep[w]) : 0u;
}

// kept rows before row r, 0 <= r <= n
__device__ __forceinline__ long long kept_before(const uint32_t* __restrict__ keep,
                                                 const uint32_t* __restrict__ W, long long r) {
    if (!keep) return r;
    const int b = (int)(r & 31);
    return (long long)W[r >> 5] + (b ? __popc(keep[r >> 5] & ((1u << b) - 1u)) : 0);
}

// Thread i < n: dest[i].  Thread i <= nlist: new_offsets[i], add_base[i] (i < nlist) and the
// check of offsets[i] and add_offsets[i].  Offsets are held to [0, n] before anything is
// indexed with them, and the binary search ends in [0, nlist) whatever they hold.
__global__ void __launch_bounds__(256)
regroup_plan(const long long* __restrict__ offsets, long long nlist, long long n,
             const uint32_t* __restrict__ keep, const uint32_t* __restrict__ W,
             const long long* __restrict__ add_off, long long* __restrict__ new_off,
             long long* __restrict__ dest, long long* __restrict__ add_base,
             unsigned long long* __restrict__ err) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (i < n) {
        long long d = -1;
        if (!keep || ((keep[i >> 5] >> (i & 31)) & 1u)) {
            d = kept_before(keep, W, i);
            if (add_off) {
                long long lo = 0, hi = nlist;   // the last l with offsets[l] <= i
                while (hi - lo > 1) {
                    const long long mid = lo + (hi - lo) / 2;
                    if (offsets[mid] <= i)
                        lo = mid;
                    else
                        hi = mid;
                }
                d += add_off[lo];
            }
        }
        dest[i] = d;
    }
    if (i <= nlist) {
        const long long o = offsets[i];
        const long long a = add_off ? add_off[i] : 0;
        bad = o < 0 || o > n || (i == 0 && (o != 0 || a != 0)) || (i == nlist && o != n);
        if (i < nlist) bad = bad || o > offsets[i + 1] || (add_off && a > add_off[i + 1]);
        new_off[i] = kept_before(keep, W, min(max(o, 0ll), n)) + a;
        if (i < nlist && add_base)
            add_base[i] = kept_before(keep, W, min(max(offsets[i + 1], 0ll), n)) + a;
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(err, 1ull);
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// ------------------------------------------------------------------- the decode through it
// One lane per chunk of C rows, L <= 64 chunks a workgroup (L * C rows fit the stage).
//  1. The workgroup reads the destinations of its rows (coalesced): rows_of[c] = 1 + the last
//     row of chunk c with a destination in [0, n_out), so a chunk without one is neither read
//     nor walked, and a workgroup without one ends here.  A destination below -1 or from n_out
//     on counts as none and sets error bit 2.
//  2. The stream window of the chunks between the first and the last one to walk, staged as
//     the filtered scan stages it (byte-swapped, for PosRd); an index that does not ascend or
//     leaves the stream gets no window, and every lane's own offset is then checked by SelRd.
//  3. The walk: walk_packed for rows of NW u64 words, walk_parts for any m <= 16, the running
//     row of the latter being the stage slot that is decoded.  The whole chunk is staged before
//     anything is stored, so a chunk that fails (error bit 1) leaves its rows unwritten.
//     (These are the lines of stage_step in pqh_scan_dev.h, here for u16 codes too.  As one
//     function that both call they cost adc_scan's filtered whole-stream form 2 to 7 %, so the
//     two copies stay: a change to one is a change to the other.)
//  4. The write-back: unit U of 8, 4, 2 or 1 bytes, lane q the unit q % per of staged row
//     q / per (per = units a row), stored at out[dest[row]].
template <typename CodeT, int NW, bool CTX>
__global__ void __launch_bounds__(64)
scat_rows(const uint32_t* __restrict__ words, long long nwords, long long n, int m, int raw_first,
          int C, const unsigned long long* __restrict__ chunk_off,
          const void* __restrict__ chunk_prev, DecTabs T, const long long* __restrict__ dest,
          unsigned char* __restrict__ out, long long n_out, unsigned long long* __restrict__ err,
          int win_words, int L, int stage_bytes) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ int rows_of[64];
    unsigned char* stage = lds;                                          // [L][C][m] codes
    uint32_t* win = reinterpret_cast<uint32_t*>(lds + stage_bytes);      // [win_words + 4]
    const int lane = threadIdx.x;
    const int rb = m * (int)sizeof(CodeT);
    const long long chunks = (n + C - 1) / C;
    const long long j0 = (long long)blockIdx.x * L;
    const int jn = (int)min(chunks - j0, (long long)L);
    const long long row0 = j0 * C;
    const int nrows = (int)(min(n, (j0 + jn) * C) - row0);
    const unsigned long long nbits = (unsigned long long)nwords * 32;

    rows_of[lane] = 0;
    lds_barrier();
    bool bad = false;
#pragma unroll 1
    for (int q = lane; q < nrows; q += 64) {
        const long long d = dest[row0 + q];
        if (d >= 0 && d < n_out)
            atomicMax(&rows_of[q / C], q % C + 1);
        else if (d != -1)
            bad = true;
    }
    if (__ballot(bad) && lane == 0) atomicOr(err, 2ull);
    lds_barrier();
    const int cnt = lane < jn ? rows_of[lane] : 0;
    const unsigned long long todo = __ballot(cnt > 0);
    if (!todo) return;
    const int c_lo = __ffsll((long long)todo) - 1, c_hi = 63 - __clzll((long long)todo);

    bool use_win = false;
    StreamWin sw{0, 0, false};
    {
        const long long ja = j0 + c_lo, jb = j0 + c_hi + 1;
        const unsigned long long b_lo = chunk_off[ja];
        const unsigned long long b_hi = jb < chunks ? chunk_off[jb] : nbits;
        if (b_lo <= nbits && b_hi >= b_lo && b_hi <= nbits) {
            sw = stage_window<4, true>(words, nwords, chunk_off, ja, chunks, win, win_words,
                                       (int)(jb - ja));
            use_win = sw.in_lds;
        }
    }
    lds_barrier();

    bool ok = true;
    if (cnt > 0) {
        const long long j = j0 + lane;
        const unsigned long long off = chunk_off[j];
        const bool raw = CTX && j == 0 && raw_first;
        auto walk = [&](auto& br) -> bool {
            if constexpr (NW > 0) {
                unsigned long long* st =
                    reinterpret_cast<unsigned long long*>(stage) + (long long)lane * C * NW;
                unsigned long long prev[NW];
#pragma unroll
                for (int w = 0; w < NW; ++w) prev[w] = 0;
                if (CTX && !raw) {
#pragma unroll
                    for (int w = 0; w < NW; ++w)
                        prev[w] = static_cast<const unsigned long long*>(chunk_prev)[j * NW + w];
                }
                return walk_packed<CTX, NW, 8 * (int)sizeof(CodeT)>(
                    br, T, raw, cnt, prev,
                    [&](int s, int w, unsigned long long row) { st[s * NW + w] = row; });
            } else {
                // the running row is the stage slot being decoded: it starts as a copy of the
                // row before it
                CodeT* st = reinterpret_cast<CodeT*>(stage) + (long long)lane * C * m;
                for (int i = 0; i < m; ++i)
                    st[i] = (CTX && !raw) ? static_cast<const CodeT*>(chunk_prev)[j * m + i]
                                          : (CodeT)0;
                int cur = 0;
                return walk_parts<0>(
                    br, T, m, CTX, raw, cnt, [&](int i) -> CodeT& { return st[cur * m + i]; },
                    [&](int s) {
                        if (s + 1 < cnt)
                            for (int i = 0; i < m; ++i) st[(s + 1) * m + i] = st[s * m + i];
                        cur = s + 1;
                    });
            }
        };
        ok = off <= nbits;   // a start past the stream is refused before anything is read
        if (ok && use_win) {
            const unsigned long long w_bits = (unsigned long long)sw.w_lo * 32;
            ok = off >= w_bits && off <= w_bits + (unsigned long long)sw.nw * 32;
            if (ok) {
                PosRd br;
                br.init(win, (uint32_t)(sw.nw + 3), off - w_bits);
                ok = walk(br) && w_bits + br.bit() <= nbits;
            }
        } else if (ok) {
            SelRd rd;
            ok = rd.init(words, nwords, off);
            if (ok) ok = walk(rd.br) && rd.pos() <= nbits;
        }
    }
    const unsigned long long dead = __ballot(!ok);
    if (dead && lane == 0) atomicOr(err, 1ull);
    lds_barrier();

    auto flush = [&](auto unit) {
        using U = decltype(unit);
        const int per = rb / (int)sizeof(U);
#pragma unroll 1
        for (int q = lane; q < nrows * per; q += 64) {
            const int r = q / per, u = q - r * per;
            const int c = r / C;
            if (r - c * C >= rows_of[c] || ((dead >> c) & 1ull)) continue;   // not decoded
            const long long d = dest[row0 + r];
            if (d < 0 || d >= n_out) continue;
            reinterpret_cast<U*>(out + d * rb)[u] =
                reinterpret_cast<const U*>(stage + (long long)r * rb)[u];
        }
    };
    const uintptr_t o = reinterpret_cast<uintptr_t>(out);
    if (!(rb & 7) && !(o & 7))
        flush((unsigned long long)0);
    else if (!(rb & 3) && !(o & 3))
        flush((uint32_t)0);
    else if (!(rb & 1) && !(o & 1))
        flush((uint16_t)0);
    else
        flush((unsigned char)0);
}

}  // namespace

extern "C" {

int pqh_ivf_regroup(pqh_ctx_t* ctx, const long long* d_offsets, long long nlist, long long n,
                    const unsigned int* d_keep, const long long* d_add_offsets,
                    long long* d_new_offsets, long long* d_dest, long long* d_add_base) {
    if (!ctx) return pqh_no_ctx_status();
    if (n < 0 || nlist < 1 || !d_offsets || !d_new_offsets || (n > 0 && !d_dest) ||
        (reinterpret_cast<uintptr_t>(d_keep) & 3u))
        return PQH_ERR_ARG;
    if (n > 0x7FFFFFFFll || nlist > PQH_IVF_MAX_NLIST) return PQH_ERR_UNSUPPORTED;
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    if (n == 0) d_keep = nullptr;   // (no row, no word)
    const uint32_t* W = nullptr;
    if (d_keep) {
        const long long nw = (n + 31) >> 5;
        const size_t items = (size_t)nw + 1;
        size_t temp = 0;
        if (rocprim::exclusive_scan(nullptr, temp, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u,
                                    items, rocprim::plus<uint32_t>(), ctx->stream) != hipSuccess)
            return pqh_set_error(ctx, PQH_ERR_HIP, "ivf regroup: temp storage query failed");
        const size_t wb = align256(items * 4);
        rc = pqh_ensure_ws(ctx, 2 * wb + align256(temp));
        if (rc) return rc;
        uint32_t* cnt = static_cast<uint32_t*>(ctx->ws);
        uint32_t* pre = reinterpret_cast<uint32_t*>(static_cast<char*>(ctx->ws) + wb);
        hipLaunchKernelGGL(keep_popc, dim3((unsigned)((items + 255) / 256)), dim3(256), 0,
                           ctx->stream, d_keep, nw, cnt);
        PQH_HIP(ctx, rocprim::exclusive_scan(static_cast<char*>(ctx->ws) + 2 * wb, temp, cnt, pre,
                                             0u, items, rocprim::plus<uint32_t>(), ctx->stream));
        W = pre;
    }
    const long long threads = std::max<long long>(n, nlist + 1);
    hipLaunchKernelGGL(regroup_plan, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0,
                       ctx->stream, d_offsets, nlist, n, d_keep, W, d_add_offsets, d_new_offsets,
                       d_dest, d_add_base, ctx->d_diag + kDiagIvf);
    PQH_LAUNCH_CHECK(ctx);
    return PQH_OK;
}

int pqh_decode_scatter(pqh_ctx_t* ctx, const pqh_tables_t* t, const unsigned char* d_stream,
                       unsigned long long stream_bytes, long long n, int raw_first,
                       int chunk_vectors, const unsigned long long* d_chunk_offsets,
                       const void* d_chunk_prev, const long long* d_dest, void* d_out,
                       long long n_out) {
    if (!ctx) return pqh_no_ctx_status();
    if (!t || n < 0 || n_out < 0 || chunk_vectors <= 0) return PQH_ERR_ARG;
    if (n > 0 && (!d_stream || !d_chunk_offsets || !d_dest || stream_bytes < 4 ||
                  (n_out > 0 && !d_out)))
        return PQH_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(d_stream) & 3u) return PQH_ERR_ARG;
    if (t->context && !d_chunk_prev && (!raw_first || n > chunk_vectors)) return PQH_ERR_ARG;
    if (t->m > 16 || (t->context && t->k > 256)) return PQH_ERR_UNSUPPORTED;
    const int esz = t->k <= 256 ? 1 : 2;
    if (reinterpret_cast<uintptr_t>(d_out) & (uintptr_t)(esz - 1)) return PQH_ERR_ARG;
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    if (n == 0) return PQH_OK;
    // the stage: the whole chunks of L lanes, at most 32 KB (one chunk: at most 96 KB)
    const long long chunk_bytes = (long long)chunk_vectors * t->m * esz;
    int L = 64;
    while (L > 1 && L * chunk_bytes > 32 * 1024) L /= 2;
    if (L * chunk_bytes > 96 * 1024) return PQH_ERR_UNSUPPORTED;
    const int stage_bytes = (int)((L * chunk_bytes + 15) & ~15ll);
    // the window: pqh_decode's (12 or 14 bits a symbol at the most, 16 KB at the most)
    const long long sym_bits = t->k <= 256 ? 12 : 14;
    const long long span_words = ((long long)L * chunk_vectors * t->m * sym_bits + 31) / 32 + 8;
    const int win_words = (int)std::min<long long>(4096, std::max<long long>(256, span_words));
    const size_t lds = (size_t)stage_bytes + ((size_t)win_words + 4) * 4;
    const long long chunks = (n + chunk_vectors - 1) / chunk_vectors;
    const long long blocks = (chunks + L - 1) / L;
    if (blocks > 0x7FFFFFFFll) return PQH_ERR_UNSUPPORTED;
    const DecTabs T = dec_tabs(t, 0);
    rc = with_shape(t, packed_row_words(t, d_chunk_prev), [&](auto code, auto nw, auto cx) -> int {
        auto* kern = scat_rows<decltype(code), decltype(nw)::value, decltype(cx)::value>;
        if (lds > 64 * 1024)
            PQH_HIP(ctx, hipFuncSetAttribute((const void*)kern,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(64), lds, ctx->stream,
                           reinterpret_cast<const uint32_t*>(d_stream),
                           (long long)(stream_bytes / 4), n, t->m, raw_first, chunk_vectors,
                           d_chunk_offsets, d_chunk_prev, T, d_dest,
                           static_cast<unsigned char*>(d_out), n_out, ctx->d_diag + 1, win_words, L,
                           stage_bytes);
        return PQH_OK;
    });
    if (rc) return rc;
    PQH_LAUNCH_CHECK(ctx);
    return PQH_OK;
}

}  // extern "C"
