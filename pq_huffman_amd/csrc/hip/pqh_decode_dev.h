// pqh_decode_dev.h -- the stream decoder's device code shared by pqh_decode.hip, pqh_search.hip
// and pqh_regroup.hip (not installed): the bit readers, the symbol lookup, the two row walks,
// the stream window and the host's choice of a row shape.  One statement of each; every kernel
// that reads a stream includes this.
#pragma once

#include <type_traits>

#include "pqh_internal.h"

namespace {

// ------------------------------------------------------------------- bit readers
// All readers are MSB-first over 32-bit stream words with 32-bit word indices, clamped to
// [0, lim]; a stream of any length is served by basing the reader at the word its chunks
// start in.  peek(nb) shows the next nb <= 32 bits, skip(nb) consumes nb <= 32, word(i) is
// the i-th word as an MSB-first integer and bit() the position.

// a 64-bit buffer refilled one word at a time, branch-free (the next word is always read)
struct BitRd {
    const uint32_t* w;
    uint32_t lim;
    uint32_t next;
    unsigned long long buf;
    int have;
    __device__ __forceinline__ uint32_t word(uint32_t i) const { return __builtin_bswap32(w[min(i, lim)]); }
    __device__ __forceinline__ void init(const uint32_t* words, uint32_t last, unsigned long long p) {
        w = words;
        lim = last;
        const uint32_t wi = (uint32_t)(p >> 5);
        const int o = (int)(p & 31);
        buf = (((unsigned long long)word(wi) << 32) | word(wi + 1)) << o;
        have = 64 - o;
        next = wi + 2;
    }
    __device__ __forceinline__ unsigned long long bit() const {
        return (unsigned long long)next * 32 - (unsigned long long)have;
    }
    __device__ __forceinline__ uint32_t peek(int nb) const { return (uint32_t)(buf >> (64 - nb)); }
    __device__ __forceinline__ void skip(int nb) {
        const uint32_t x = word(next);
        buf <<= nb;
        have -= nb;
        const bool need = have <= 32;
        buf |= need ? ((unsigned long long)x << (32 - have)) : 0ull;
        next += need ? 1u : 0u;
        have += need ? 32 : 0;
    }
};

// BitRd whose skip loads the next word only when the buffer needs it: a load with 64
// distinct lane addresses is what a step of the random-access walks pays for, and only the
// lanes that refill take part in it (over an LDS window the branch-free refill is cheaper)
struct LazyRd : BitRd {
    __device__ __forceinline__ void skip(int nb) {
        buf <<= nb;
        have -= nb;
        if (have <= 32) {
            buf |= (unsigned long long)word(next) << (32 - have);
            next += 1u;
            have += 32;
        }
    }
};

// The reader of a byte-swapped LDS window (the words MSB-first as integers, swapped once when
// they are staged): it keeps only the bit position, so a peek is one two-word LDS read and a
// funnel shift and a skip one add (BitRd's buffer costs ~17 VALU per skip: the refill's
// shifts and selects).  Words past `lim` read as the last one (the window's zero pad).
struct PosRd {
    const uint32_t* w;
    uint32_t lim;
    uint32_t pos;
    __device__ __forceinline__ uint32_t word(uint32_t i) const { return w[min(i, lim)]; }
    __device__ __forceinline__ void init(const uint32_t* words, uint32_t last, unsigned long long p) {
        w = words;
        lim = last;
        pos = (uint32_t)p;
    }
    __device__ __forceinline__ unsigned long long bit() const { return pos; }
    __device__ __forceinline__ uint32_t peek(int nb) const {   // 1 <= nb <= 32
        // words i and i + 1 in one ds_read2 (i clamped so both are in [0, lim]: past the
        // window's data both are its zero pad), then one 64-bit shift
        const uint32_t i = min(pos >> 5, lim - 1);
        const unsigned long long ab = ((unsigned long long)w[i] << 32) | w[i + 1];
        return (uint32_t)((ab << (pos & 31u)) >> 32) >> (32 - nb);
    }
    __device__ __forceinline__ void skip(int nb) { pos += (uint32_t)nb; }
};

// A lane's own reader of the global stream at bit `off`: LazyRd based at the word the chunk
// starts in and clamped to the stream's last word.  A start past the stream is refused before
// anything is read; the caller compares pos() with the stream's length after its walk.
struct SelRd {
    LazyRd br;
    unsigned long long base_bits;
    __device__ __forceinline__ bool init(const uint32_t* words, long long nwords,
                                         unsigned long long off) {
        if (off > (unsigned long long)nwords * 32) return false;
        const long long bw = min((long long)(off >> 5), nwords - 1);
        base_bits = (unsigned long long)bw * 32;
        // (off - base_bits is at most bit 32 of the base word: the stream's end)
        br.init(words + bw, (uint32_t)min(nwords - 1 - bw, 0xFFFFFFF0ll), off - base_bits);
        return true;
    }
    __device__ __forceinline__ unsigned long long pos() const { return base_bits + br.bit(); }
};

template <typename Rd>
__device__ __forceinline__ unsigned long long peek56(const Rd& br) {   // the next 56 bits
    const unsigned long long p = br.bit();
    const uint32_t i = (uint32_t)(p >> 5);
    const int o = (int)(p & 31);
    const unsigned long long hi = ((unsigned long long)br.word(i) << 32) | br.word(i + 1);
    const unsigned long long lo = br.word(i + 2);
    return (o ? ((hi << o) | (lo >> (32 - o))) : hi) >> 8;
}

template <typename Rd>
__device__ __forceinline__ void skip_bits(Rd& br, int nb) {   // nb may exceed 32
    for (; nb > 0; nb -= 32) br.skip(nb < 32 ? nb : 32);
}

// ------------------------------------------------------------------- one symbol
// The decode tables as a kernel sees them (global memory, or a workgroup's LDS copies).
struct DecTabs {
    const uint16_t* lut1;
    const uint16_t* lut2;
    const uint32_t* meta;
    const pqh_long_code* longs;
    const uint32_t* long_cnt;
    long long lut2_cap;
    int w1, k;
    int prio;   // wave issue priority (pqh_prio; 0: the kernel keeps the default)
};

DecTabs dec_tabs(const pqh_tables_t* t, int prio) {
    return DecTabs{t->d_lut1, t->d_lut2, t->d_meta, t->d_long, t->d_long_cnt, t->lut2_cap,
                   t->l1_bits, t->k, prio};
}

// codes beyond both table levels: linear search of the alphabet's long list against the
// next 56 stream bits; returns len << 16 | sym, or 0 if none matches (inlined: a call would
// cost the kernel its register budget)
__device__ __forceinline__ uint32_t dec_long(const pqh_long_code* __restrict__ longs, uint32_t cnt,
                                          unsigned long long bits56) {
    for (uint32_t q = 0; q < cnt; ++q) {
        const pqh_long_code lc = longs[q];
        if (lc.len >= 1 && lc.len <= (uint32_t)kMaxCodeLen &&
            (bits56 >> (kMaxCodeLen - lc.len)) == lc.code)
            return (lc.len << 16) | lc.sym;
    }
    return 0;
}

// One symbol of alphabet `tab`, or -1 (invalid).
// A wave decodes 64 chains in lock step, so a branch taken by any lane costs every lane: with
// W1 = 9 about 3 % of a SIFT batch's symbols are longer than the first level, so 87 % of the
// wave's symbol steps run the second level.  This form keeps that path short: the alphabet's
// meta word is loaded with the first-level entry (8 KB per table set: cache-resident), so the
// second level is one dependent load, and every path but the long list ends in the same
// single skip.
// It peeks 32 bits at once, so the reader holds at least 33 valid bits (every reader above
// does) and W1 + w2 <= 25: W1 <= 13 (kL1Max) and w2 <= l2_bits <= 12 for every table set the
// build makes, K = 4096 included.
template <typename Rd>
__device__ __forceinline__ int dec_sym(Rd& br, const DecTabs& T, unsigned tab) {
    const int w1 = T.w1;
    const uint32_t mt = T.meta[tab];
    const uint32_t p32 = br.peek(32);
    const uint16_t e = T.lut1[(tab << w1) + (p32 >> (32 - w1))];
    // (both loads complete here: without this the compiler sinks the meta load into the
    // second-level branch, behind the first-level load's result)
    asm volatile("" ::"v"(mt), "v"(e));
    const int len = e >> 12;
    unsigned sym = e & 0xFFFu;
    int adv = -1;   // bits to skip; 0: the long list; -1: invalid
    if (len >= 1 && len <= w1) {
        adv = len;
    } else if (len == 15) {
        adv = 0;
        if (sym != 0xFFFu) {   // second level
            const int w2 = (int)((mt >> 4) & 15u);
            const long long li = (long long)(mt >> 9) + ((long long)sym << w2) +
                                 ((p32 >> (32 - w1 - w2)) & ((1u << w2) - 1u));
            adv = -1;
            if (w2 >= 1 && !(mt & 0x100u) && li < T.lut2_cap) {
                const uint16_t e2 = T.lut2[li];
                const int len2 = e2 >> 12;
                if (len2 >= 1 && len2 <= w2) {
                    adv = w1 + len2;
                    sym = e2 & 0xFFFu;
                } else if (len2 == 15) {
                    adv = 0;
                }
            }
        }
    }
    if (adv == 0) {   // codes beyond both levels: the alphabet's long list
        const uint32_t f = dec_long(T.longs + (long long)tab * T.k, T.long_cnt[tab], peek56(br));
        if (!f) return -1;
        skip_bits(br, (int)(f >> 16));
        sym = f & 0xFFFFu;
        return sym < (unsigned)T.k ? (int)sym : -1;
    }
    if (adv < 0) return -1;
    br.skip(adv);
    return sym < (unsigned)T.k ? (int)sym : -1;
}

// ------------------------------------------------------------------- the rows of a chunk
// ceil(log2 K): the raw bits per part of global row 0 (huffman_decode.c:73-76; the encoder
// writes 8)
__device__ __forceinline__ int warm_bits_of(int k) {
    int wb = 1;
    while ((1 << wb) < k) ++wb;
    return wb;
}

// Rows [0, steps) of one chunk as NW u64 words of SB-bit symbols packed little-end first
// (SB = 8: u8 codes, 8 NW parts; SB = 16: u16 codes, 4 NW parts), so the running row is NW
// registers: prev = the chunk's context row on entry (raw: row 0 is raw bits instead), the
// last decoded row on return.  put(s, w, word) sees every finished word of every row.
template <bool CTX, int NW, int SB, typename Rd, typename Put>
__device__ __forceinline__ bool walk_packed(Rd& br, const DecTabs& T, bool raw, int steps,
                                            unsigned long long (&prev)[NW], Put&& put) {
    constexpr int PW = 64 / SB;   // parts per word
    constexpr unsigned SMASK = (1u << SB) - 1u;
    const unsigned roots = CTX ? (unsigned)T.k : 1u;
    int s = 0;
    if (CTX && raw) {
        const int wb = warm_bits_of(T.k);
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            prev[w] = 0;
#pragma unroll 1
            for (int i = 0; i < PW; ++i) {
                prev[w] |= (unsigned long long)br.peek(wb) << (SB * i);
                br.skip(wb);
            }
            put(0, w, prev[w]);
        }
        s = 1;
    }
    for (; s < steps; ++s) {
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            unsigned long long row = 0;
#pragma unroll 1
            for (int i = 0; i < PW; ++i) {   // (rolled: one copy of the lookup code, fewer registers)
                const unsigned part = (unsigned)(w * PW + i);
                const unsigned tab =
                    part * roots + (CTX ? (unsigned)(prev[w] >> (SB * i)) & SMASK : 0u);
                const int sym = dec_sym(br, T, tab);
                if (sym < 0) return false;
                row |= (unsigned long long)sym << (SB * i);
            }
            prev[w] = row;
            put(s, w, row);
        }
    }
    return true;
}

// f(i) for the parts i < m until it returns false.  UN = 0: a rolled loop (one copy of the
// body); UN > 0: unrolled UN >= m times, so that f may index registers.
template <int UN, typename F>
__device__ __forceinline__ bool for_parts(int m, F&& f) {
    if constexpr (UN == 0) {
#pragma unroll 1
        for (int i = 0; i < m; ++i)
            if (!f(i)) return false;
    } else {
#pragma unroll
        for (int i = 0; i < UN; ++i) {
            if (i >= m) break;
            if (!f(i)) return false;
        }
    }
    return true;
}

// The same walk part by part, for any m <= 16: row(i) is a reference to part i of the running
// row (the chunk's context row on entry; an LDS slot, or with UN > 0 registers), done(s) sees
// every finished row.
template <int UN, typename Rd, typename Row, typename Done>
__device__ __forceinline__ bool walk_parts(Rd& br, const DecTabs& T, int m, bool ctx, bool raw,
                                           int steps, Row&& row, Done&& done) {
    using Sym = typename std::remove_reference<decltype(row(0))>::type;
    const unsigned roots = ctx ? (unsigned)T.k : 1u;
    int s = 0;
    if (ctx && raw) {
        const int wb = warm_bits_of(T.k);
        for_parts<UN>(m, [&](int i) {
            row(i) = (Sym)br.peek(wb);
            br.skip(wb);
            return true;
        });
        done(0);
        s = 1;
    }
    for (; s < steps; ++s) {
        const bool ok = for_parts<UN>(m, [&](int i) {
            const int sym = dec_sym(br, T, (unsigned)i * roots + (ctx ? (unsigned)row(i) : 0u));
            if (sym >= 0) row(i) = (Sym)sym;
            return sym >= 0;
        });
        if (!ok) return false;
        done(s);
    }
    return true;
}

// ------------------------------------------------------------------- the stream window
// The `span` (64 unless the caller has fewer) chunks [j0, j0 + span) of a workgroup are
// contiguous in the stream, so their words [w_lo, w_lo + nw) are copied into an LDS window
// with coalesced non-temporal loads (streamed once, so the code tables keep the L2), FLIGHT
// loads in flight per lane, byte-swapped on the way in for PosRd (SWAP), followed by a 4-word
// zero pad that reads past the data land in.
// A span longer than the window is left in global memory (in_lds = false).  No barrier here.
struct StreamWin {
    long long w_lo, nw;
    bool in_lds;
};
template <int FLIGHT, bool SWAP>
__device__ __forceinline__ StreamWin stage_window(const uint32_t* __restrict__ words, long long nwords,
                                                  const unsigned long long* __restrict__ chunk_off,
                                                  long long j0, long long chunks, uint32_t* win,
                                                  int win_words, int span = 64) {
    const int lane = threadIdx.x;
    const unsigned long long b_lo = chunk_off[j0];
    const unsigned long long b_hi = j0 + span < chunks ? chunk_off[j0 + span] : (unsigned long long)nwords * 32;
    const long long w_lo = (long long)(b_lo >> 5);
    const long long w_hi = min(nwords, (long long)((b_hi + 31) >> 5) + 2);
    const long long nw = w_hi - w_lo;
    const bool in_lds = nw <= win_words;
    if (in_lds) {
#pragma unroll 1
        for (long long w0 = 0; w0 < nw; w0 += FLIGHT * 64) {
            uint32_t r[FLIGHT];
#pragma unroll
            for (int u = 0; u < FLIGHT; ++u) {
                const long long w = w0 + u * 64 + lane;
                r[u] = w < nw ? __builtin_nontemporal_load(words + w_lo + w) : 0u;
            }
#pragma unroll
            for (int u = 0; u < FLIGHT; ++u) {
                const long long w = w0 + u * 64 + lane;
                if (w < nw) win[w] = SWAP ? __builtin_bswap32(r[u]) : r[u];
            }
        }
        if (lane < 4) win[nw + lane] = 0;
    }
    return StreamWin{w_lo, nw, in_lds};
}

// ------------------------------------------------------------------- host side: the row shapes
// A packed row: 8 or 16 bytes of u8 codes, or 8 u16 codes, with the chunk contexts readable
// as u64 words.  Returns its u64 words (1 or 2), or 0 for the per-part kernels.
inline int packed_row_words(const pqh_tables_t* t, const void* d_chunk_prev) {
    const int esz = t->k <= 256 ? 1 : 2;
    const int row_bytes = t->m * esz;
    const bool packed = (row_bytes == 8 || row_bytes == 16) && (esz == 1 || t->m == 8) &&
                        !(reinterpret_cast<uintptr_t>(d_chunk_prev) & 7);
    return packed ? row_bytes / 8 : 0;
}

// f(CodeT(), NW, CTX) with the table set's code type, the row's u64 words nw (0: per part)
// and the context flag as compile-time values (u16 codes are never context coded)
template <int N>
using Int = std::integral_constant<int, N>;
template <typename F>
int with_shape(const pqh_tables_t* t, int nw, F&& f) {
    if (t->k > 256)
        return nw ? f(uint16_t(), Int<2>(), std::false_type())
                  : f(uint16_t(), Int<0>(), std::false_type());
    auto with_nw = [&](auto ctx) -> int {
        return nw == 1   ? f(uint8_t(), Int<1>(), ctx)
               : nw == 2 ? f(uint8_t(), Int<2>(), ctx)
                         : f(uint8_t(), Int<0>(), ctx);
    };
    return t->context ? with_nw(std::true_type()) : with_nw(std::false_type());
}

}  // namespace
