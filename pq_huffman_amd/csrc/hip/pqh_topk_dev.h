// pqh_topk_dev.h -- the wave-wide top-k list of the search kernels (pqh_search.hip) and of the
// coarse quantizer's probe selection (pqh_ivf.hip): 64 entries, one per lane, kept ascending by
// (value, id); and beside it the wide list of the searches and the re-rank with top_k in
// (64, 256], four entries a lane (TopKW, at the end).  Device code only; every function is
// called by a whole wave whose lane number is threadIdx.x.
#pragma once

#include <cmath>

#include "pqh_internal.h"

namespace {

// ------------------------------------------------------------------- the top-k list
// A wave's list: 64 entries, one per lane, ascending by (d, id); unused entries are
// (+inf, -1), which every finite candidate precedes.  Only the first top_k lanes are the
// result; the threshold a candidate has to beat is the entry of lane top_k - 1.
struct TopK {
    float d;
    long long id;
};

__device__ __forceinline__ bool lex_lt(float a, long long ia, float b, long long ib) {
    return (a < b) | ((a == b) & (ia < ib));   // (no short circuit: selects, not branches)
}
__device__ __forceinline__ float lane_f(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ __forceinline__ long long lane_ll(long long v, int l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((unsigned long long)v >> 32), l);
    return (long long)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ int wave_shr1(int v) {   // lane i takes lane i - 1 (lane 0 keeps v)
    return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xF, 0xF, false);
}

// the wave-uniform candidate (cd, cid) into its place: its position is the number of entries
// before it; the entries from there on move one lane up (the last one falls off)
__device__ __forceinline__ void list_insert(TopK& e, float cd, long long cid) {
    const int lane = threadIdx.x;
    const int pos = __popcll(__ballot(lex_lt(e.d, e.id, cd, cid)));
    const float pd = __int_as_float(wave_shr1(__float_as_int(e.d)));
    const uint32_t plo = (uint32_t)wave_shr1((int)(uint32_t)e.id);
    const uint32_t phi = (uint32_t)wave_shr1((int)(uint32_t)((unsigned long long)e.id >> 32));
    const long long pid = (long long)(((unsigned long long)phi << 32) | plo);
    e.d = lane > pos ? pd : lane == pos ? cd : e.d;
    e.id = lane > pos ? pid : lane == pos ? cid : e.id;
}

// ---- many candidates at once: a bitonic network over the wave, one key per lane
// the lane keeps the smaller (take_min) or the larger of its key and lane ^ j's
__device__ __forceinline__ void key_exchange(TopK& x, int j, bool take_min) {
    const TopK p{__shfl_xor(x.d, j), __shfl_xor(x.id, j)};
    const bool take = take_min == lex_lt(p.d, p.id, x.d, x.id);
    x.d = take ? p.d : x.d;
    x.id = take ? p.id : x.id;
}

// The 64 smallest of the list and the 64 keys c, sorted, into the list.  c is sorted ascending
// first unless it already is (SORTED); reversed, its lane-wise minimum with the list holds the
// 64 smallest of both as a bitonic sequence, which six exchange steps sort.  Lanes without a
// candidate carry (+inf, max id), which no list entry follows.
template <bool SORTED>
__device__ __forceinline__ void list_merge(TopK& e, TopK c) {
    const int lane = threadIdx.x;
    if constexpr (!SORTED) {
#pragma unroll
        for (int k = 2; k <= 64; k <<= 1)
#pragma unroll
            for (int j = k >> 1; j > 0; j >>= 1)
                key_exchange(c, j, ((lane & j) == 0) == ((lane & k) == 0));
    }
    const TopK r{__shfl(c.d, 63 - lane), __shfl(c.id, 63 - lane)};
    const bool take = lex_lt(r.d, r.id, e.d, e.id);
    e.d = take ? r.d : e.d;
    e.id = take ? r.id : e.id;
#pragma unroll
    for (int j = 32; j > 0; j >>= 1) key_exchange(e, j, (lane & j) == 0);
}

// Every lane offers one candidate (d, id) (valid: it takes part).  The ones before the
// threshold are inserted one by one, lowest lane first, the threshold moving with every insert
// so that the rest are filtered again; more than kSerialMax of them go through list_merge
// instead (an insert is a chain of ~50 dependent instructions, the network ~28 exchange steps
// whatever the count).  SORTED: the candidates ascend with the lane.  Called by the whole wave.
constexpr int kSerialMax = 6;
template <bool SORTED>
__device__ __forceinline__ void list_offer(TopK& e, float d, long long id, bool valid, int kth) {
    float td = lane_f(e.d, kth);
    long long tid = lane_ll(e.id, kth);
    const bool pass = valid && lex_lt(d, id, td, tid);
    unsigned long long mask = __ballot(pass);
    if (!mask) return;
    if (__popcll(mask) > kSerialMax) {
        list_merge<SORTED>(e, pass ? TopK{d, id} : TopK{INFINITY, 0x7FFFFFFFFFFFFFFFll});
        return;
    }
    while (mask) {
        const int l = __builtin_ctzll(mask);
        list_insert(e, lane_f(d, l), lane_ll(id, l));
        td = lane_f(e.d, kth);
        tid = lane_ll(e.id, kth);
        mask &= mask - 1;
        mask &= __ballot(valid && lex_lt(d, id, td, tid));
    }
}

// ------------------------------------------------------------------- the wide list
// 64 * kWideKR entries a wave, kWideKR a lane, for top_k in (64, 256]: entry j is register
// j >> 6 of lane j & 63, so a block of 64 entries is one TopK across the wave and the code
// above serves it block by block.  The same order, padding and threshold (entry top_k - 1) as
// the list above; only the blocks up to the threshold's are ever touched, the ones behind it
// stay padding.  The threshold is kept beside the entries (wave-uniform) so that the offer
// nobody passes -- nearly every one once the list is warm -- reads no lane.
constexpr int kWideKR = 4;
struct TopKW {
    float d[kWideKR];
    long long id[kWideKR];
    float td;        // entry kth, refreshed by whatever changes the list
    long long tid;
};

__device__ __forceinline__ void list_clear(TopKW& e) {
#pragma unroll
    for (int b = 0; b < kWideKR; ++b) e.d[b] = INFINITY, e.id[b] = -1ll;
    e.td = INFINITY;
    e.tid = -1ll;
}

__device__ __forceinline__ void list_threshold(TopKW& e, int kth) {
    const int kb = kth >> 6, kl = kth & 63;
#pragma unroll
    for (int b = 0; b < kWideKR; ++b)
        if (b == kb) e.td = lane_f(e.d[b], kl), e.tid = lane_ll(e.id[b], kl);
}

// list_insert across the blocks: the candidate's position is the number of entries before it
// (it beats the threshold, so pos <= kth); from there on every entry moves one up, lane 63 of a
// block into lane 0 of the next.  Highest block first: a block takes its predecessor's last
// entry as it was.
__device__ __forceinline__ void list_insert(TopKW& e, float cd, long long cid, int kth) {
    const int lane = threadIdx.x;
    const int kb = kth >> 6;
    int pos = 0;
#pragma unroll
    for (int b = 0; b < kWideKR; ++b)
        if (b <= kb) pos += __popcll(__ballot(lex_lt(e.d[b], e.id[b], cd, cid)));
    const int pb = pos >> 6;
#pragma unroll
    for (int b = kWideKR - 1; b >= 0; --b) {
        if (b > kb || b < pb) continue;   // (wave-uniform)
        float pd = __int_as_float(wave_shr1(__float_as_int(e.d[b])));
        const uint32_t plo = (uint32_t)wave_shr1((int)(uint32_t)e.id[b]);
        const uint32_t phi = (uint32_t)wave_shr1((int)(uint32_t)((unsigned long long)e.id[b] >> 32));
        long long pid = (long long)(((unsigned long long)phi << 32) | plo);
        if (b > 0) {
            const float ud = lane_f(e.d[b - 1], 63);
            const long long uid = lane_ll(e.id[b - 1], 63);
            pd = lane == 0 ? ud : pd;
            pid = lane == 0 ? uid : pid;
        }
        const int g = b * 64 + lane;
        e.d[b] = g > pos ? pd : g == pos ? cd : e.d[b];
        e.id[b] = g > pos ? pid : g == pos ? cid : e.id[b];
    }
}

// list_merge across the blocks.  The sorted 64 keys c against block b: reversed, the lane-wise
// minimum is the block's new content and the lane-wise maximum what is left over, each a
// bitonic sequence that six exchange steps sort; the maximum is carried into block b + 1.  A
// block none of whose entries follows a key of c stays as it is and c is carried whole, which
// also ends the work once the carry is all padding.  The carry out of the threshold's block
// is dropped.
template <bool SORTED>
__device__ __forceinline__ void list_merge(TopKW& e, TopK c, int kth) {
    const int lane = threadIdx.x;
    const int kb = kth >> 6;
    if constexpr (!SORTED) {
#pragma unroll
        for (int k = 2; k <= 64; k <<= 1)
#pragma unroll
            for (int j = k >> 1; j > 0; j >>= 1)
                key_exchange(c, j, ((lane & j) == 0) == ((lane & k) == 0));
    }
#pragma unroll
    for (int b = 0; b < kWideKR; ++b) {
        if (b > kb) continue;   // (wave-uniform, as the next)
        if (!lex_lt(lane_f(c.d, 0), lane_ll(c.id, 0), lane_f(e.d[b], 63), lane_ll(e.id[b], 63)))
            continue;
        const TopK r{__shfl(c.d, 63 - lane), __shfl(c.id, 63 - lane)};
        const bool take = lex_lt(r.d, r.id, e.d[b], e.id[b]);
        TopK lo{take ? r.d : e.d[b], take ? r.id : e.id[b]};
        c = TopK{take ? e.d[b] : r.d, take ? e.id[b] : r.id};
#pragma unroll
        for (int j = 32; j > 0; j >>= 1) key_exchange(lo, j, (lane & j) == 0);
        e.d[b] = lo.d;
        e.id[b] = lo.id;
        if (b < kb) {
#pragma unroll
            for (int j = 32; j > 0; j >>= 1) key_exchange(c, j, (lane & j) == 0);
        }
    }
}

// list_offer for the wide list: the same early exit, the same split between serial inserts
// and the network.
template <bool SORTED>
__device__ __forceinline__ void list_offer(TopKW& e, float d, long long id, bool valid, int kth) {
    const bool pass = valid && lex_lt(d, id, e.td, e.tid);
    unsigned long long mask = __ballot(pass);
    if (!mask) return;
    if (__popcll(mask) > kSerialMax) {
        list_merge<SORTED>(e, pass ? TopK{d, id} : TopK{INFINITY, 0x7FFFFFFFFFFFFFFFll}, kth);
        list_threshold(e, kth);
        return;
    }
    while (mask) {
        const int l = __builtin_ctzll(mask);
        list_insert(e, lane_f(d, l), lane_ll(id, l), kth);
        list_threshold(e, kth);
        mask &= mask - 1;
        mask &= __ballot(valid && lex_lt(d, id, e.td, e.tid));
    }
}

}  // namespace
