// pqh_decode.hip -- the chunked stream decoder over the two-level code tables of
// pqh_tables.hip (layout: pqh_internal.h).  The bit readers, dec_sym, the two walks and the
// stream window are in pqh_decode_dev.h, shared with pqh_search.hip.
//
//  dec_sym      one symbol: first level, second level, long list (huffman_decode.c:137-191
//               as table lookups) -- the only statement of it, over any of the bit readers.
//  walk_packed  the rows of one chunk, one lane per chunk: rows of whole u64 words in
//  walk_parts   registers, or part by part for any m <= 16.  Every kernel but dec_tree walks
//               its chunks through one of the two.
//  dec_rows     huffman_decoder.c:211-255 for rows of 8/16 u8 or 8 u16 codes and chunks of
//               C <= 32 vectors: <= 34 VGPRs, the stream window and the rows staged in LDS.
//  dec_chunks   the same for every other shape (any m <= 16, any C).
//  sel_rows     the same decode for selected rows only: one lane per requested id, walking
//  dec_range    its chunk from the chunk index; the cut chunks of a row range; optionally
//               fused with the PQ reconstruction (pqh_decode_select / _range / pqh_fetch_vectors).
//  dec_tree     huffman_decoder --tree: every row in the context of its parent row.
#include <algorithm>
#include <type_traits>
#include <vector>

#include "pqh_internal.h"
#include "pqh_decode_dev.h"

namespace {

// ------------------------------------------------------------------- whole streams
// Per-lane decode of chunk j in batches of S vectors staged in LDS; every lane of the
// workgroup runs the batch loop (barriers).  `br` reads the LDS window or the global stream.
template <int MT, typename CodeT>
__device__ __forceinline__ void decode_batches(BitRd& br, bool live, long long j, long long j0,
                                               long long jn, long long n, int m, int context,
                                               int raw_first, int chunk_vectors, int S,
                                               const CodeT* __restrict__ chunk_prev,
                                               const DecTabs& T, CodeT* stage,
                                               CodeT* __restrict__ out, bool& ok) {
    const int lane = threadIdx.x;
    const long long v0 = j * chunk_vectors;
    const long long v1 = min(n, v0 + chunk_vectors);
    unsigned prev[MT ? MT : 16];
    bool warm = context && j == 0 && raw_first && live;   // global row 0 of a context stream
#pragma unroll
    for (int i = 0; i < (MT ? MT : 16); ++i)
        prev[i] = (live && i < m && context && !warm) ? (unsigned)chunk_prev[j * m + i] : 0u;
    const long long run = (long long)S * m;   // staged codes per lane per batch

    for (int s0 = 0; s0 < chunk_vectors; s0 += S) {
        const int rows = live ? (int)(min(v1, v0 + s0 + S) - (v0 + s0)) : 0;
        CodeT* base = stage + lane * run;
        const bool good = walk_parts<MT ? MT : 16>(
            br, T, m, context != 0, warm, ok ? rows : 0, [&](int i) -> unsigned& { return prev[i]; },
            [&](int s) {
                CodeT* o = base + (long long)s * m;
                if constexpr (sizeof(CodeT) == 1 && MT % 4 == 0 && MT > 0) {
#pragma unroll
                    for (int q = 0; q < MT / 4; ++q)
                        reinterpret_cast<uint32_t*>(o)[q] = prev[4 * q] | (prev[4 * q + 1] << 8) |
                                                            (prev[4 * q + 2] << 16) | (prev[4 * q + 3] << 24);
                } else {
#pragma unroll
                    for (int i = 0; i < (MT ? MT : 16); ++i)
                        if (MT || i < m) o[i] = (CodeT)prev[i];
                }
            });
        if (!good) ok = false;
        warm = false;
        __syncthreads();
        // write back: lane-run r holds rows (j0 + r) * C + s0 ... of at most S rows
        if (S == chunk_vectors && (run * (long long)sizeof(CodeT)) % 4 == 0) {
            // runs are contiguous: one linear copy of the workgroup's rows
            const long long rows_wg = min(n, (j0 + 64) * chunk_vectors) - j0 * chunk_vectors;
            const long long nbytes = rows_wg * m * (long long)sizeof(CodeT);
            char* dst = reinterpret_cast<char*>(out + j0 * chunk_vectors * m);
            const long long n4 = nbytes / 4;
            for (long long q = lane; q < n4; q += 64)
                __builtin_nontemporal_store(reinterpret_cast<const uint32_t*>(stage)[q],
                                            reinterpret_cast<uint32_t*>(dst) + q);
            for (long long q = n4 * 4 + lane; q < nbytes; q += 64)
                dst[q] = reinterpret_cast<const char*>(stage)[q];
        } else {
            for (long long q = lane; q < 64 * run; q += 64) {
                const long long r = q / run, w = q % run;
                const long long row = (j0 + r) * chunk_vectors + s0 + w / m;
                if (r < jn && s0 + w / m < chunk_vectors && row < n) out[row * m + w % m] = stage[q];
            }
        }
        __syncthreads();
    }
}

// One lane per chunk of C vectors (huffman_decoder.c:211-255), any m <= 16 and any C: the
// workgroup's stream window in LDS (global fallback when it does not fit); decoded codes are
// staged in LDS and written back coalesced, S vectors per lane at a time.  The only global
// loads in the symbol loop are then the table lookups (the meta words, and with L1_IN_LDS the
// first level, are LDS copies), and no store sits in front of them in the vmcnt queue.
// MT = parts at compile time (0 = runtime m <= 16).
template <int MT, typename CodeT, bool L1_IN_LDS>
__global__ void __launch_bounds__(64)
dec_chunks(const uint32_t* __restrict__ words, long long nwords, long long n, int m_rt,
           int context, int raw_first, int chunk_vectors,
           const unsigned long long* __restrict__ chunk_off, const CodeT* __restrict__ chunk_prev,
           DecTabs T, long long tables, CodeT* __restrict__ out,
           unsigned long long* __restrict__ err, int win_words, int S) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int m = MT ? MT : m_rt;
    const long long meta_b = (tables * 4 + 15) & ~15ll;
    const long long l1_b = L1_IN_LDS ? (((tables << T.w1) * 2 + 15) & ~15ll) : 0;
    uint32_t* meta = reinterpret_cast<uint32_t*>(lds);
    uint16_t* l1s = reinterpret_cast<uint16_t*>(lds + meta_b);
    uint32_t* win = reinterpret_cast<uint32_t*>(lds + meta_b + l1_b);
    CodeT* stage = reinterpret_cast<CodeT*>(lds + meta_b + l1_b + ((long long)win_words + 4) * 4);
    const int lane = threadIdx.x;
    for (long long t = lane; t < tables; t += 64) meta[t] = T.meta[t];
    T.meta = meta;
    if constexpr (L1_IN_LDS) {
        const long long n16 = ((tables << T.w1) * 2 + 15) / 16;
        const uint4* src = reinterpret_cast<const uint4*>(T.lut1);
        uint4* dst = reinterpret_cast<uint4*>(l1s);
        for (long long i = lane; i < n16; i += 64) dst[i] = src[i];
        T.lut1 = l1s;
    }
    const long long chunks = (n + chunk_vectors - 1) / chunk_vectors;
    const long long j0 = (long long)blockIdx.x * 64;
    const long long jn = min(chunks - j0, 64ll);
    const StreamWin sw = stage_window<8, false>(words, nwords, chunk_off, j0, chunks, win, win_words);
    __syncthreads();

    const long long j = j0 + lane;
    const bool live = lane < jn;
    bool ok = true;
    const unsigned long long start = live ? chunk_off[j] - (unsigned long long)sw.w_lo * 32 : 0;
    BitRd br;
    if (sw.in_lds) {
        br.init(win, (uint32_t)(sw.nw + 3), start);
        decode_batches<MT, CodeT>(br, live, j, j0, jn, n, m, context, raw_first, chunk_vectors, S,
                                  chunk_prev, T, stage, out, ok);
    } else {
        // (any stream length: the last word index clamped as SelRd's)
        br.init(words + sw.w_lo, (uint32_t)min(nwords - 1 - sw.w_lo, 0xFFFFFFF0ll), start);
        decode_batches<MT, CodeT>(br, live, j, j0, jn, n, m, context, raw_first, chunk_vectors, S,
                                  chunk_prev, T, stage, out, ok);
    }
    if (!ok) atomicOr(err, 1ull);
}

// The slim decoder for rows of whole u64 words (the bench shape): <= 34 VGPRs, so, like the
// table builds, it runs beside the assignment grid.  One lane per chunk of C <= 32 vectors, 64
// chunks per workgroup; the chunks' stream window byte-swapped in LDS (or, if it does not fit,
// the global stream at 32-bit offsets from the window's first word); a row is decoded into NW
// registers, staged in LDS and written back as whole rows; the context row is those registers.
template <bool CTX, int NW, int SB>
__global__ void __launch_bounds__(64)
dec_rows(const uint32_t* __restrict__ words, long long nwords, long long n, int raw_first,
         int chunk_vectors, const unsigned long long* __restrict__ chunk_off,
         const unsigned long long* __restrict__ chunk_prev, DecTabs T,
         unsigned long long* __restrict__ out, unsigned long long* __restrict__ err, int win_words) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    unsigned long long* stage = reinterpret_cast<unsigned long long*>(lds);   // [64][C][NW]
    uint32_t* win = reinterpret_cast<uint32_t*>(lds + 64 * 8 * NW * chunk_vectors);
    const int lane = threadIdx.x;
    pqh_set_prio(T.prio);   // latency-bound: issue ahead of the assignment's waves
    const long long chunks = (n + chunk_vectors - 1) / chunk_vectors;
    const long long j0 = (long long)blockIdx.x * 64;
    const long long jn = min(chunks - j0, 64ll);
    const StreamWin sw = stage_window<4, true>(words, nwords, chunk_off, j0, chunks, win, win_words);
    __syncthreads();
    const long long j = j0 + lane;
    bool ok = true;
    if (lane < jn) {
        const unsigned long long start = chunk_off[j] - (unsigned long long)sw.w_lo * 32;
        unsigned long long* st = stage + (long long)lane * chunk_vectors * NW;
        // (one copy of the lane's set-up per reader: shared, it costs the context kernels registers)
        auto walk = [&](auto br, const uint32_t* src, uint32_t lim) {
            br.init(src, lim, start);
            const int cnt = (int)min((long long)chunk_vectors, n - j * chunk_vectors);
            const bool raw = CTX && j == 0 && raw_first;
            unsigned long long prev[NW];
#pragma unroll
            for (int w = 0; w < NW; ++w) prev[w] = 0;
            if (CTX && !raw) {   // (a branch, not a select: one load of the whole row)
#pragma unroll
                for (int w = 0; w < NW; ++w) prev[w] = chunk_prev[j * NW + w];
            }
            return walk_packed<CTX, NW, SB>(br, T, raw, cnt, prev, [&](int s, int w, unsigned long long row) {
                st[s * NW + w] = row;
            });
        };
        ok = sw.in_lds ? walk(PosRd(), win, (uint32_t)(sw.nw + 3))
                       : walk(BitRd(), words + sw.w_lo, (uint32_t)(nwords - 1 - sw.w_lo));
    }
    __syncthreads();
    // the workgroup's rows are contiguous: whole-row stores
    const long long r0 = j0 * chunk_vectors * NW;
    const long long words_out = (min(n, (j0 + 64) * chunk_vectors) - j0 * chunk_vectors) * NW;
#pragma unroll 1
    for (long long q = lane; q < words_out; q += 64) __builtin_nontemporal_store(stage[q], out + r0 + q);
    if (!ok) atomicOr(err, 1ull);
}

// ---- random access: selected rows, fused reconstruction, row ranges -------------------
// (pqh_decode_select / pqh_fetch_vectors / pqh_decode_range).  The chunk index is the only
// structure these need: a row is reached by walking its chunk from the chunk's bit offset,
// in the chunk's stored context.  The ids of a wave are scattered over the stream, so there
// is no window to stage: every lane reads the global stream through SelRd.

// One lane per requested id v (huffman_decoder.c:211-255 for the rows asked for): chunk
// j = v / C from chunk_off[j] in the context chunk_prev[j] (raw row 0 for j = 0 when
// raw_first), rows j*C ... v, row v into output slot q.  NW > 0: rows of NW u64 words (8 or
// 16 u8 codes, 8 u16 codes) in registers; NW = 0: any m <= 16, per part.  The wave's 64
// result rows are staged in LDS and stored whole (FETCH = false), or reconstructed from
// there (FETCH: x_hat[q] = concat_i cent[i][code_i], every float row written by the whole
// wave as consecutive 16-byte stores; the codes never reach memory).  An id outside [0, n)
// gives a zero row and error bit 2; an invalid code, a chunk offset or a symbol past the
// stream a zero row and error bit 1.
template <typename CodeT, int NW, bool CTX, bool FETCH>
__global__ void __launch_bounds__(64)
sel_rows(const uint32_t* __restrict__ words, long long nwords, long long n, int m, int raw_first,
         int chunk_vectors, const unsigned long long* __restrict__ chunk_off,
         const void* __restrict__ chunk_prev, DecTabs T, const long long* __restrict__ ids,
         long long count, void* __restrict__ out, long long ld_out, const float* __restrict__ cent,
         int dsub, unsigned long long* __restrict__ err) {
    __shared__ __attribute__((aligned(16))) unsigned char stage_b[64 * 16 * sizeof(CodeT)];
    __shared__ unsigned char dead[64];
    CodeT* stage = reinterpret_cast<CodeT*>(stage_b);
    const int lane = threadIdx.x;
    const long long q0 = (long long)blockIdx.x * 64;
    const int rows = (int)min(64ll, count - q0);
    CodeT* row = stage + lane * m;
    unsigned flag = 0;
    bool good = false;
    if (lane < rows) {
        const long long v = ids[q0 + lane];
        if (v < 0 || v >= n) {
            flag = 2;
        } else {
            const long long j = v / chunk_vectors;
            const int steps = (int)(v - j * chunk_vectors) + 1;
            const bool raw = CTX && j == 0 && raw_first;
            SelRd rd;
            good = rd.init(words, nwords, chunk_off[j]);
            if (good) {
                if constexpr (NW > 0) {
                    unsigned long long prev[NW];
#pragma unroll
                    for (int w = 0; w < NW; ++w)
                        prev[w] = (CTX && !raw)
                                      ? static_cast<const unsigned long long*>(chunk_prev)[j * NW + w]
                                      : 0ull;
                    good = walk_packed<CTX, NW, 8 * (int)sizeof(CodeT)>(
                        rd.br, T, raw, steps, prev, [](int, int, unsigned long long) {});
#pragma unroll
                    for (int w = 0; w < NW; ++w) reinterpret_cast<unsigned long long*>(row)[w] = prev[w];
                } else {
                    for (int i = 0; i < m; ++i)
                        row[i] = (CTX && !raw) ? static_cast<const CodeT*>(chunk_prev)[j * m + i]
                                               : (CodeT)0;
                    good = walk_parts<0>(rd.br, T, m, CTX, raw, steps,
                                         [&](int i) -> CodeT& { return row[i]; }, [](int) {});
                }
                good = good && rd.pos() <= (unsigned long long)nwords * 32;
            }
            if (!good) flag = 1;
        }
    }
    if (!good)
        for (int i = 0; i < m; ++i) row[i] = (CodeT)0;
    dead[lane] = good ? 0 : 1;
    if (flag) atomicOr(err, (unsigned long long)flag);
    lds_barrier();
    if constexpr (!FETCH) {
        // the workgroup's rows are contiguous in the output: whole-row stores
        const long long nbytes = (long long)rows * m * (long long)sizeof(CodeT);
        unsigned char* dst = static_cast<unsigned char*>(out) + q0 * m * (long long)sizeof(CodeT);
        long long done = 0;
        if (!(reinterpret_cast<uintptr_t>(dst) & 3u)) {
            done = nbytes & ~3ll;
            for (long long q = lane; q < done / 4; q += 64)
                reinterpret_cast<uint32_t*>(dst)[q] = reinterpret_cast<const uint32_t*>(stage_b)[q];
        }
        for (long long q = done + lane; q < nbytes; q += 64) dst[q] = stage_b[q];
    } else {
        float* o = static_cast<float*>(out) + q0 * ld_out;
        const int d = m * dsub;
        const long long k = T.k;
        if (!(d & 3) && !(ld_out & 3) && !(reinterpret_cast<uintptr_t>(out) & 15u)) {
            const int per = d >> 2;   // 16-byte pieces of a row; a piece may span two parts
            for (int it = lane; it < rows * per; it += 64) {
                const int r = it / per, c = (it - r * per) * 4;
                const CodeT* cr = stage + r * m;
                float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
                if (!dead[r]) {
                    if (!(dsub & 3)) {
                        const int i = c / dsub;
                        val = *reinterpret_cast<const float4*>(cent + (i * k + cr[i]) * dsub + (c - i * dsub));
                    } else {
                        float e[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const int i = (c + u) / dsub;
                            e[u] = cent[(i * k + cr[i]) * dsub + (c + u - i * dsub)];
                        }
                        val = make_float4(e[0], e[1], e[2], e[3]);
                    }
                }
                *reinterpret_cast<float4*>(o + (long long)r * ld_out + c) = val;
            }
        } else {
            for (int it = lane; it < rows * d; it += 64) {
                const int r = it / d, c = it - r * d;
                const int i = c / dsub;
                o[(long long)r * ld_out + c] =
                    dead[r] ? 0.f : cent[(i * k + stage[r * m + i]) * dsub + (c - i * dsub)];
            }
        }
    }
}

// Rows [first, first + count) where they are not whole chunks: one lane per chunk, as
// dec_rows, walking its chunk from the start and storing only the rows inside the range
// (the first and the last chunk of a range may be cut; the whole chunks between them go
// through pqh_decode's kernels, skipped here as [skip_at, skip_at + skip_len)).  The running
// row is the lane's LDS slot; a failed chunk's rows of the range are zeroed.
template <typename CodeT, bool CTX>
__global__ void __launch_bounds__(64)
dec_range(const uint32_t* __restrict__ words, long long nwords, long long n, int m, int raw_first,
          int chunk_vectors, const unsigned long long* __restrict__ chunk_off,
          const CodeT* __restrict__ chunk_prev, DecTabs T, long long first, long long count,
          long long jbeg, long long skip_at, long long skip_len, long long lanes,
          CodeT* __restrict__ out, unsigned long long* __restrict__ err) {
    __shared__ CodeT stage[64 * 16];
    const long long idx = (long long)blockIdx.x * 64 + threadIdx.x;
    if (idx >= lanes) return;   // (no barriers below: lanes are independent)
    long long j = jbeg + idx;
    if (j >= skip_at) j += skip_len;
    const long long v0 = j * chunk_vectors;
    const long long lo = max(v0, first);
    const long long hi = min(min(n, v0 + chunk_vectors), first + count);
    if (lo >= hi) return;
    CodeT* row = stage + threadIdx.x * m;
    const bool raw = CTX && j == 0 && raw_first;
    for (int i = 0; i < m; ++i) row[i] = (CTX && !raw) ? chunk_prev[j * m + i] : (CodeT)0;
    SelRd rd;
    bool ok = rd.init(words, nwords, chunk_off[j]);
    ok = ok && walk_parts<0>(rd.br, T, m, CTX, raw, (int)(hi - v0),
                             [&](int i) -> CodeT& { return row[i]; },
                             [&](int s) {
                                 const long long v = v0 + s;
                                 if (v >= lo)
                                     for (int i = 0; i < m; ++i) out[(v - first) * m + i] = row[i];
                             });
    if (ok && rd.pos() > (unsigned long long)nwords * 32) ok = false;
    if (!ok) {
        for (long long q = (lo - first) * m; q < (hi - first) * m; ++q) out[q] = (CodeT)0;
        atomicOr(err, 1ull);
    }
}

// the chunk offsets handed to pqh_decode's kernels by pqh_decode_range: within the stream
// and not decreasing, else the decode error (those kernels clamp their reads but report only
// invalid codes)
__global__ void __launch_bounds__(256)
chk_offsets(const unsigned long long* __restrict__ off, long long cnt, int last_has_next,
            unsigned long long total_bits, unsigned long long* __restrict__ err) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= cnt) return;
    const unsigned long long a = off[j];
    const bool next = j + 1 < cnt || last_has_next;
    if (a > total_bits || (next && a > off[j + 1])) atomicOr(err, 1ull);
}

// ---- tree mode ------------------------------------------------------------------------
// huffman_decoder --tree (huffman_decoder.c:214-247): row p is decoded in the context of the
// row at stream position parent_pos[p] (the traverser replayed over the children stream),
// a root starting every part with the raw warm-up bits.  One lane per chunk of C rows from
// the encoder's chunk index; the chunk's rows are staged in LDS, so a parent inside the
// chunk is read back from there, and the parents that lie before the chunk come from the
// ext sidecar (ext_rows[ext_off[j] ...], in row order) -- every chunk decodes independently.
// (Its context row changes with every row, so it keeps its own loop over dec_sym.)
__global__ void __launch_bounds__(64)
dec_tree(const uint32_t* __restrict__ words, long long nwords, long long n, int m,
         int chunk_vectors, const unsigned long long* __restrict__ chunk_off,
         const long long* __restrict__ parent_pos, const long long* __restrict__ ext_off,
         const uint8_t* __restrict__ ext_rows, DecTabs T, uint8_t* __restrict__ out,
         unsigned long long* __restrict__ err, unsigned long long total_bits) {
    extern __shared__ uint8_t tstage[];   // [64 lanes][C rows][m]
    const long long chunks = (n + chunk_vectors - 1) / chunk_vectors;
    const long long j = (long long)blockIdx.x * 64 + threadIdx.x;
    if (j >= chunks) return;               // no barriers below: lanes are independent
    const long long v0 = j * chunk_vectors;
    const long long v1 = min(n, v0 + chunk_vectors);
    uint8_t* st = tstage + (long long)threadIdx.x * chunk_vectors * m;
    long long e = ext_off[j];
    const long long e_end = ext_off[j + 1];
    const int wb = warm_bits_of(T.k);
    // a chunk that starts past the stream's end (a truncated file or a stale sidecar) reads
    // nothing; one whose symbols run past it is reported below -- never decoded silently
    SelRd rd;
    bool ok = chunk_off[j] <= total_bits && rd.init(words, nwords, chunk_off[j]);
    for (long long p = v0; p < v1 && ok; ++p) {
        const long long pp = parent_pos[p];
        const uint8_t* prow = nullptr;
        if (pp >= v0 && pp < p) {
            prow = st + (pp - v0) * m;
        } else if (pp >= 0) {
            if (pp >= p || e >= e_end) { ok = false; break; }   // inconsistent sidecar
            prow = ext_rows + e * m;
            ++e;
        }
        uint8_t* o = st + (p - v0) * m;
        for (int i = 0; i < m; ++i) {
            int sym;
            if (!prow) {
                sym = (int)rd.br.peek(wb);
                rd.br.skip(wb);
            } else {
                sym = dec_sym(rd.br, T, (unsigned)i * (unsigned)T.k + prow[i]);
            }
            if (sym < 0) {
                ok = false;
                break;
            }
            o[i] = (uint8_t)sym;
        }
    }
    if (ok && rd.pos() > total_bits) ok = false;
    const long long nb = (v1 - v0) * m;
    uint8_t* dst = out + v0 * m;
    for (long long q = 0; q < nb; ++q) dst[q] = ok ? st[q] : 0;
    if (!ok) atomicOr(err, 1ull);
}

// ------------------------------------------------------------------- host side
// argument checks shared by the random-access calls
int sel_check(pqh_ctx_t* ctx, const pqh_tables_t* t, const unsigned char* d_stream,
              unsigned long long stream_bytes, long long n, int raw_first, int chunk_vectors,
              const unsigned long long* d_chunk_offsets, const void* d_chunk_prev, long long count,
              const void* d_out) {
    if (!ctx || !t || n < 0 || chunk_vectors <= 0 || count < 0) return PQH_ERR_ARG;
    if (count > 0 && (!d_out || (n > 0 && (!d_stream || !d_chunk_offsets || stream_bytes < 4))))
        return PQH_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(d_stream) & 3u) return PQH_ERR_ARG;
    if (t->context && !d_chunk_prev && (!raw_first || n > chunk_vectors)) return PQH_ERR_ARG;
    if (t->m > 16 || (t->context && t->k > 256)) return PQH_ERR_UNSUPPORTED;
    return pqh_use_device(ctx);
}

// sel_rows over `count` ids: codes [count][m] (FETCH = false) or float rows ld_out apart
template <bool FETCH>
int sel_launch(pqh_ctx_t* ctx, const pqh_tables_t* t, const unsigned char* d_stream,
               unsigned long long stream_bytes, long long n, int raw_first, int chunk_vectors,
               const unsigned long long* d_chunk_offsets, const void* d_chunk_prev,
               const long long* d_ids, long long count, void* d_out, long long ld_out,
               const float* d_cent, int dsub) {
    const DecTabs T = dec_tabs(t, 0);
    const uint32_t* wp = reinterpret_cast<const uint32_t*>(d_stream);
    const long long nwords = (long long)(stream_bytes / 4);
    const unsigned blocks = (unsigned)((count + 63) / 64);
    with_shape(t, packed_row_words(t, d_chunk_prev), [&](auto code, auto nw, auto cx) {
        hipLaunchKernelGGL((sel_rows<decltype(code), decltype(nw)::value, decltype(cx)::value, FETCH>),
                           dim3(blocks), dim3(64), 0, ctx->stream, wp, nwords, n, t->m, raw_first,
                           chunk_vectors, d_chunk_offsets, d_chunk_prev, T, d_ids, count, d_out,
                           ld_out, d_cent, dsub, ctx->d_diag + 1);
        return 0;
    });
    PQH_LAUNCH_CHECK(ctx);
    return PQH_OK;
}

}  // namespace

extern "C" {

int pqh_decode(pqh_ctx_t* ctx, const pqh_tables_t* t, const unsigned char* d_stream,
               unsigned long long stream_bytes, long long n, int raw_first, int chunk_vectors,
               const unsigned long long* d_chunk_offsets, const void* d_chunk_prev, void* d_codes) {
    if (!ctx || !t || n < 0 || chunk_vectors <= 0 ||
        (n > 0 && (!d_stream || !d_chunk_offsets || !d_codes)))
        return PQH_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(d_stream) & 3u) return PQH_ERR_ARG;
    if (t->context && !raw_first && !d_chunk_prev) return PQH_ERR_ARG;
    if (t->m > 16) return PQH_ERR_UNSUPPORTED;
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    if (n == 0) return PQH_OK;
    // (no memset: d_diag[1] is sticky until pqh_decode_status reads it)
    const long long chunks = (n + chunk_vectors - 1) / chunk_vectors;
    const long long nwords = (long long)(stream_bytes / 4);
    const unsigned blocks = (unsigned)((chunks + 63) / 64);
    const uint32_t* wp = reinterpret_cast<const uint32_t*>(d_stream);
    if (reinterpret_cast<uintptr_t>(d_codes) & 3u) return PQH_ERR_ARG;
    const size_t l1_bytes = (size_t)(t->tables << t->l1_bits) * 2;
    const size_t meta_bytes = ((size_t)t->tables * 4 + 15) & ~(size_t)15;
    const bool lds_l1 = meta_bytes + l1_bytes <= 48 * 1024;
    const size_t esz = t->k <= 256 ? 1 : 2;
    // stream window: the workgroup's 64 chunks at up to 12 (K <= 256; Huffman averages
    // at most ~8.x bits) or 14 bits per symbol, at most 16 KB -- a larger span reads the
    // global stream instead; staging: S vectors per lane, at most 16 KB
    const long long sym_bits = t->k <= 256 ? 12 : 14;
    const long long span_words = (64ll * chunk_vectors * t->m * sym_bits + 31) / 32 + 8;
    const int win_words = (int)std::min<long long>(4096, std::max<long long>(256, span_words));
    int S = chunk_vectors;
    while (S > 1 && (size_t)64 * S * t->m * esz > 16 * 1024) S = (S + 1) / 2;
    const size_t lds = meta_bytes + (lds_l1 ? ((l1_bytes + 15) & ~(size_t)15) : 0) +
                       ((size_t)win_words + 4) * 4 + (size_t)64 * S * t->m * esz + 16;
    if (lds > 160 * 1024) return PQH_ERR_UNSUPPORTED;
    // whole-row decoders (<= 34 VGPRs: they run beside the assignment grid): packed rows,
    // chunks of C <= 32 vectors, 8-byte aligned output rows
    const int nw_row = packed_row_words(t, d_chunk_prev);
    if (nw_row && chunk_vectors <= 32 && nwords < (1ll << 31) &&
        !(reinterpret_cast<uintptr_t>(d_codes) & 7)) {
        const int ww = (int)std::min<long long>(4096 - 1024 * (nw_row - 1),
                                                std::max<long long>(256, span_words));
        const size_t lds_r = (size_t)64 * 8 * nw_row * chunk_vectors + ((size_t)ww + 4) * 4;
        const DecTabs T = dec_tabs(t, pqh_prio("DECODE", 3));
        rc = with_shape(t, nw_row, [&](auto code, auto nw, auto cx) -> int {
            constexpr int NW = decltype(nw)::value, SB = 8 * (int)sizeof(code);
            constexpr bool CTX = decltype(cx)::value;
            if constexpr (NW > 0) {
                if (lds_r > 64 * 1024)
                    PQH_HIP(ctx, hipFuncSetAttribute((const void*)(dec_rows<CTX, NW, SB>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     (int)lds_r));
                hipLaunchKernelGGL((dec_rows<CTX, NW, SB>), dim3(blocks), dim3(64), lds_r,
                                   ctx->stream, wp, nwords, n, raw_first, chunk_vectors,
                                   d_chunk_offsets,
                                   static_cast<const unsigned long long*>(d_chunk_prev), T,
                                   static_cast<unsigned long long*>(d_codes), ctx->d_diag + 1, ww);
            }
            return PQH_OK;
        });
        if (rc) return rc;
        PQH_LAUNCH_CHECK(ctx);
        return PQH_OK;
    }
    const DecTabs T = dec_tabs(t, 0);
    auto launch = [&](auto mt, auto code, auto l1) -> int {
        using CodeT = decltype(code);
        constexpr int MT = decltype(mt)::value;
        constexpr bool L1 = decltype(l1)::value;
        if (lds > 64 * 1024)
            PQH_HIP(ctx, hipFuncSetAttribute((const void*)(dec_chunks<MT, CodeT, L1>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((dec_chunks<MT, CodeT, L1>), dim3(blocks), dim3(64), lds, ctx->stream,
                           wp, nwords, n, t->m, t->context, raw_first, chunk_vectors,
                           d_chunk_offsets, static_cast<const CodeT*>(d_chunk_prev), T, t->tables,
                           static_cast<CodeT*>(d_codes), ctx->d_diag + 1, win_words, S);
        return PQH_OK;
    };
    auto with_l1 = [&](auto mt, auto code) -> int {
        return lds_l1 ? launch(mt, code, std::true_type()) : launch(mt, code, std::false_type());
    };
    // parts at compile time for the common u8 shapes
    rc = esz == 2      ? with_l1(Int<0>(), uint16_t())
         : t->m == 8   ? with_l1(Int<8>(), uint8_t())
         : t->m == 16  ? with_l1(Int<16>(), uint8_t())
                       : with_l1(Int<0>(), uint8_t());
    if (rc) return rc;
    PQH_LAUNCH_CHECK(ctx);
    return PQH_OK;
}

int pqh_decode_status(pqh_ctx_t* ctx) {
    unsigned long long e = 0;
    PQH_HIP(ctx, hipMemcpyAsync(&e, ctx->d_diag + 1, 8, hipMemcpyDeviceToHost, ctx->stream));
    PQH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (e) PQH_HIP(ctx, hipMemsetAsync(ctx->d_diag + 1, 0, 8, ctx->stream));   // (sticky until read)
    // bit 0: an invalid code (every decoder); bit 1: an id outside the rows (pqh_decode_select,
    // pqh_fetch_vectors) -- reported only when no code was invalid
    if (e & 1ull) return pqh_set_error(ctx, PQH_ERR_CORRUPT, "invalid code in stream");
    return e ? pqh_set_error(ctx, PQH_ERR_ARG, "row id outside the stream's rows") : PQH_OK;
}

int pqh_decode_select(pqh_ctx_t* ctx, const pqh_tables_t* t, const unsigned char* d_stream,
                      unsigned long long stream_bytes, long long n, int raw_first,
                      int chunk_vectors, const unsigned long long* d_chunk_offsets,
                      const void* d_chunk_prev, const long long* d_ids, long long count,
                      void* d_codes) {
    int rc = sel_check(ctx, t, d_stream, stream_bytes, n, raw_first, chunk_vectors,
                       d_chunk_offsets, d_chunk_prev, count, d_codes);
    if (rc) return rc;
    if (count == 0) return PQH_OK;
    if (!d_ids) return PQH_ERR_ARG;
    return sel_launch<false>(ctx, t, d_stream, stream_bytes, n, raw_first, chunk_vectors,
                             d_chunk_offsets, d_chunk_prev, d_ids, count, d_codes, 0, nullptr, 0);
}

int pqh_fetch_vectors(pqh_ctx_t* ctx, const pqh_tables_t* t, const pqh_pq_t* pq,
                      const unsigned char* d_stream, unsigned long long stream_bytes, long long n,
                      int raw_first, int chunk_vectors, const unsigned long long* d_chunk_offsets,
                      const void* d_chunk_prev, const long long* d_ids, long long count,
                      float* d_out, long long ld_out) {
    int m = 0, k = 0, dsub = 0;
    const float* d_cent = nullptr;
    if (!t || pqh_pq_view(pq, &m, &k, &dsub, &d_cent) || m != t->m || k != t->k ||
        ld_out < (long long)m * dsub)
        return PQH_ERR_ARG;
    int rc = sel_check(ctx, t, d_stream, stream_bytes, n, raw_first, chunk_vectors,
                       d_chunk_offsets, d_chunk_prev, count, d_out);
    if (rc) return rc;
    if (count == 0) return PQH_OK;
    if (!d_ids || (reinterpret_cast<uintptr_t>(d_out) & 3u)) return PQH_ERR_ARG;
    return sel_launch<true>(ctx, t, d_stream, stream_bytes, n, raw_first, chunk_vectors,
                            d_chunk_offsets, d_chunk_prev, d_ids, count, d_out, ld_out, d_cent,
                            dsub);
}

int pqh_decode_range(pqh_ctx_t* ctx, const pqh_tables_t* t, const unsigned char* d_stream,
                     unsigned long long stream_bytes, long long n, int raw_first, int chunk_vectors,
                     const unsigned long long* d_chunk_offsets, const void* d_chunk_prev,
                     long long first, long long count, void* d_codes) {
    int rc = sel_check(ctx, t, d_stream, stream_bytes, n, raw_first, chunk_vectors,
                       d_chunk_offsets, d_chunk_prev, count, d_codes);
    if (rc) return rc;
    if (first < 0 || first > n - count) return PQH_ERR_ARG;
    if (count == 0) return PQH_OK;
    const long long C = chunk_vectors;
    const int esz = t->k <= 256 ? 1 : 2;
    if (reinterpret_cast<uintptr_t>(d_codes) & (uintptr_t)(esz - 1)) return PQH_ERR_ARG;
    const long long chunks = (n + C - 1) / C;
    const long long end = first + count;
    const long long j_lo = first / C, j_hi = (end - 1) / C;
    // the whole chunks [ja, jb) of the range go through pqh_decode (its windowed kernels, with
    // the index pointers moved to chunk ja); the cut chunks at either end -- and every chunk
    // when that output would not be 4-byte aligned -- through dec_range
    long long ja = j_lo + (first % C ? 1 : 0);
    long long jb = j_hi + 1 - ((end % C && end != n) ? 1 : 0);
    unsigned char* o_in = static_cast<unsigned char*>(d_codes) + (ja * C - first) * t->m * esz;
    if (jb <= ja || (reinterpret_cast<uintptr_t>(o_in) & 3u)) jb = ja = j_hi + 1;
    if (jb > ja) {
        const unsigned char* cp = static_cast<const unsigned char*>(d_chunk_prev);
        rc = pqh_decode(ctx, t, d_stream, stream_bytes, std::min(n, jb * C) - ja * C,
                        ja == 0 ? raw_first : 0, chunk_vectors, d_chunk_offsets + ja,
                        cp ? cp + ja * t->m * esz : nullptr, o_in);
        if (rc == PQH_ERR_UNSUPPORTED) {   // (a chunk too long for its staging)
            jb = ja = j_hi + 1;
        } else if (rc) {
            return rc;
        } else {
            const long long cnt = jb - ja;
            hipLaunchKernelGGL(chk_offsets, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0,
                               ctx->stream, d_chunk_offsets + ja, cnt, jb < chunks ? 1 : 0,
                               (stream_bytes / 4) * 32ull, ctx->d_diag + 1);
        }
    }
    const long long lanes = (j_hi - j_lo + 1) - (jb - ja);
    if (lanes > 0) {
        const DecTabs T = dec_tabs(t, 0);
        const unsigned blocks = (unsigned)((lanes + 63) / 64);
        with_shape(t, 0, [&](auto code, auto, auto cx) {
            using CodeT = decltype(code);
            hipLaunchKernelGGL((dec_range<CodeT, decltype(cx)::value>), dim3(blocks), dim3(64), 0,
                               ctx->stream, reinterpret_cast<const uint32_t*>(d_stream),
                               (long long)(stream_bytes / 4), n, t->m, raw_first, chunk_vectors,
                               d_chunk_offsets, static_cast<const CodeT*>(d_chunk_prev), T, first,
                               count, j_lo, ja, jb - ja, lanes, static_cast<CodeT*>(d_codes),
                               ctx->d_diag + 1);
            return 0;
        });
    }
    PQH_LAUNCH_CHECK(ctx);
    return PQH_OK;
}

// Chunk index of a stream that came without a sidecar: a sequential walk over a HOST copy
// of the code table (index building only; the symbols are decoded by pqh_decode).
int pqh_chunk_index_host(const pqh_tables_t* t, const unsigned char* stream,
                         unsigned long long stream_bytes, long long n, int raw_first,
                         int chunk_vectors, unsigned long long* chunk_offsets, void* chunk_prev) {
    if (!t || n < 0 || chunk_vectors <= 0 || (n > 0 && (!stream || !chunk_offsets))) return PQH_ERR_ARG;
    if (t->context && !chunk_prev) return PQH_ERR_ARG;
    pqh_ctx* ctx = t->ctx;
    std::vector<unsigned long long> enc((size_t)t->m * t->items);
    PQH_HIP(ctx, hipMemcpyAsync(enc.data(), t->d_enc, enc.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    PQH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // per-table canonical lookup: (len, code) -> symbol, via sorted vectors per length
    const int W = 16;
    std::vector<int32_t> lut((size_t)t->tables << W, -1);
    std::vector<std::vector<std::pair<unsigned long long, int>>> longs(t->tables);
    for (long long tab = 0; tab < t->tables; ++tab)
        for (int s = 0; s < t->k; ++s) {
            const unsigned long long v = enc[(size_t)tab * t->k + s];
            const int L = (int)(v >> 56);
            if (!L) continue;
            const unsigned long long code = v & kCodeMask;
            if (L <= W) {
                for (unsigned long long e = code << (W - L); e < (code + 1) << (W - L); ++e)
                    lut[((size_t)tab << W) + e] = (L << 16) | s;
            } else {
                longs[tab].push_back({(code << 8) | (unsigned long long)L, s});
            }
        }
    const unsigned long long total = stream_bytes * 8;
    auto peek = [&](unsigned long long p, int nb) -> unsigned long long {
        unsigned long long r = 0;
        for (int b = 0; b < nb; ++b) {
            const unsigned long long q = p + b;
            r = (r << 1) | (q < total ? (unsigned long long)((stream[q >> 3] >> (7 - (q & 7))) & 1u) : 0ull);
        }
        return r;
    };
    std::vector<unsigned> prev(t->m, 0);
    bool warm = t->context && raw_first;
    int warm_bits = 1;
    while ((1 << warm_bits) < t->k) ++warm_bits;
    unsigned long long pos = 0;
    for (long long v = 0; v < n; ++v) {
        if (v % chunk_vectors == 0) {
            const long long j = v / chunk_vectors;
            chunk_offsets[j] = pos;
            if (t->context)
                for (int i = 0; i < t->m; ++i) {
                    if (t->k <= 256) static_cast<uint8_t*>(chunk_prev)[j * t->m + i] = (uint8_t)prev[i];
                    else static_cast<uint16_t*>(chunk_prev)[j * t->m + i] = (uint16_t)prev[i];
                }
        }
        for (int i = 0; i < t->m; ++i) {
            unsigned sym;
            if (warm) {
                sym = (unsigned)peek(pos, warm_bits);
                pos += warm_bits;
            } else {
                const long long tab = (long long)i * t->roots + (t->context ? prev[i] : 0);
                const int32_t e = lut[((size_t)tab << W) + peek(pos, W)];
                if (e >= 0) {
                    pos += (unsigned)e >> 16;
                    sym = (unsigned)e & 0xFFFFu;
                } else {
                    bool found = false;
                    sym = 0;
                    for (auto& lc : longs[tab]) {
                        const int L = (int)(lc.first & 0xFF);
                        if (peek(pos, L) == (lc.first >> 8)) {
                            pos += L;
                            sym = (unsigned)lc.second;
                            found = true;
                            break;
                        }
                    }
                    if (!found) return PQH_ERR_CORRUPT;
                }
                if (pos > total) return PQH_ERR_CORRUPT;
            }
            prev[i] = sym;
        }
        warm = false;
    }
    return PQH_OK;
}

int pqh_decode_tree(pqh_ctx_t* ctx, const pqh_tables_t* t, const unsigned char* d_stream,
                    unsigned long long stream_bytes, long long n, int chunk_vectors,
                    const unsigned long long* d_chunk_offsets, const long long* d_parent_pos,
                    const long long* d_ext_offsets, const unsigned char* d_ext_rows,
                    void* d_rows) {
    if (!ctx || !t || !t->context || t->k > 256 || n < 0 || chunk_vectors <= 0 ||
        (n > 0 && (!d_stream || !d_chunk_offsets || !d_parent_pos || !d_ext_offsets || !d_rows)))
        return PQH_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(d_stream) & 3u) return PQH_ERR_ARG;
    const size_t lds = (size_t)64 * chunk_vectors * t->m;
    if (lds > 160 * 1024) return PQH_ERR_UNSUPPORTED;
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    if (n == 0) return PQH_OK;
    const long long chunks = (n + chunk_vectors - 1) / chunk_vectors;
    if (lds > 64 * 1024)
        PQH_HIP(ctx, hipFuncSetAttribute((const void*)dec_tree,
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(dec_tree, dim3((unsigned)((chunks + 63) / 64)), dim3(64), lds, ctx->stream,
                       reinterpret_cast<const uint32_t*>(d_stream), (long long)((stream_bytes + 3) / 4),
                       n, t->m, chunk_vectors, d_chunk_offsets, d_parent_pos, d_ext_offsets,
                       d_ext_rows, dec_tabs(t, 0), static_cast<uint8_t*>(d_rows), ctx->d_diag + 1,
                       stream_bytes * 8ull);
    PQH_LAUNCH_CHECK(ctx);
    return PQH_OK;
}

}  // extern "C"
