// pqh_flat_range.hip -- the exact range search: every kept row of a pqh_flat with
// dist(q, v) < radius[q], dist the definition's chain of pqh_flat_search bit for bit, as many as
// there are, in ascending row.
//
//  flat_range<IP, FILL, PAN, XT>  d <= 1024.  The work split and the tile staging are
//                 flat_screen's (pqh_flat.hip): grid (query groups of 128) x (row slabs), a wave
//                 owns 32 queries as the qh | ql B operand, the slab streams past in tiles of 32
//                 rows staged once per workgroup as bf16-split fragments, passes xh.qh, xl.qh,
//                 xh.ql with the same skips, panels of 128 dimensions above d = 128.  What is
//                 its own: the threshold is fixed, T = (r - ||q||^2) + tau (IP: r + tau), known
//                 before the first tile, so there is no list, no warm-up and no refresh; a drain
//                 chains the pending pairs, compares the exact value with r and sets bit
//                 (row & 31) of the query's word of the row's tile.  A wave walks its slab in
//                 epochs of kEpoch tiles and keeps hit[32 queries][kEpoch] words in LDS; an
//                 epoch is closed by a drain, so every row before a hit of the epoch has been
//                 chained when the hit ranks itself: the popcount of its query's words before
//                 its tile plus that of its own word below its bit.
//                 FILL = 0  adds each epoch's popcounts to a count per query, stored once per
//                           (query, slab) in the plan; pqh_range_offsets_launch turns the counts,
//                           ordered (query, slab), into offsets and lims.
//                 FILL = 1  writes (dist, id) at offset[q][slab] + hits of earlier epochs + rank.
//                           A workgroup whose queries counted nothing in its slab leaves before
//                           it stages anything; a query that counted nothing, or has written all
//                           it counted, has no candidates.
//                 One template for both, so no comparison can differ between them.
//  flat_range_valu<IP, FILL, XT>  d > 1024: one wave per (query, slab), lane = row, the chain
//                 for every kept row; as a device function it is the all-rows path of a query
//                 whose tau is not below 2^110.
#include <atomic>
#include <cmath>
#include <type_traits>

#include "pqh_flat_dev.h"
#include "pqh_flat_screen_dev.h"
#include "pqh_internal.h"
#include "pqh_screen_dev.h"

namespace {

constexpr int kEpoch = 64;                 // tiles of an epoch
constexpr int kEpochStride = kEpoch + 1;   // a query's words, a bank apart from the next query's
constexpr int kHeaderWords = 8;            // the plan's header, in long longs
constexpr long long kPlanMagic = 0x50514846524e4745ll;   // "PQHFRNGE"

// The plan, in the caller's memory: the header the count pass writes (the geometry it ran with),
// then nq * slabs + 1 entries, entry q * slabs + s the count of query q in slab s, turned into
// exclusive prefixes over all of them: an entry is where the hits of its (query, slab) begin, the
// next one where they end, and entry q * slabs is lims[q].  Behind the entries one word: the
// queries that took the all-rows path, which the count pass adds up and the fill reports again
// (a workgroup that the fill skips never learns which of its queries those are).
struct RangeGeo {
    long long magic, nq, n, slabs, groups, slab_rows, epoch, d;
};
static_assert(sizeof(RangeGeo) == kHeaderWords * 8, "the header is eight words");

struct RangeArgs {
    const void* x;       // the rows, elements of the kernel's row type
    long long n, ld_x;
    int d, P;
    const float* norms;
    const unsigned* cmax;
    const float* q;
    long long nq, ld_q;
    const float* radius;
    const unsigned* keep;
    long long slab_rows;
    float kq;
    int vec_x, vec_q, vec_chain;
    long long* plan;
    RangeGeo geo;        // what this launch runs with
    long long capacity, id_base;   // FILL
    float* dist;
    long long* ids;
    unsigned long long* counts;
    unsigned long long* err;
};

__global__ void range_clear(unsigned long long* counts, long long* fallback) {
    counts[kDiagChains] = 0, counts[kDiagFallback] = 0;
    if (fallback) *fallback = 0;
}

// the all-rows queries of the call: counted by the count pass, into the plan too; the fill's first
// thread reports the plan's word
template <bool FILL>
__device__ __forceinline__ void report_fallback(const RangeArgs& a, long long slabs, long long nfb) {
    long long* const word = a.plan + kHeaderWords + a.nq * slabs + 1;
    if constexpr (FILL) {
        a.counts[kDiagFallback] = (unsigned long long)*word;
    } else if (nfb) {
        atomicAdd(a.counts + kDiagFallback, (unsigned long long)nfb);
        atomicAdd(reinterpret_cast<unsigned long long*>(word), (unsigned long long)nfb);
    }
}

// LDS written by some lanes of the wave (stores and atomics) and read by others
__device__ __forceinline__ void wave_sync() {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// FILL: a plan counted with another geometry (the tuning changed in between, another object):
// nothing is written, and pqh_decode_status reports PQH_ERR_ARG.  (uniform over the grid)
__device__ __forceinline__ bool same_geometry(const RangeArgs& a) {
    const RangeGeo* h = reinterpret_cast<const RangeGeo*>(a.plan);
    const RangeGeo& g = a.geo;
    return h->magic == g.magic && h->nq == g.nq && h->n == g.n && h->slabs == g.slabs &&
           h->groups == g.groups && h->slab_rows == g.slab_rows && h->epoch == g.epoch && h->d == g.d;
}

// the all-rows path of one query over one slab: lane = row, the chain for every kept row, a hit
// where the chain's value is below r; FILL: hit number i of the slab goes to entry out0 + i.
// Returns the hits, adds the chains run to ran (both wave-uniform).
template <bool IP, bool FILL, typename T>
__device__ __forceinline__ int all_rows(const float* __restrict__ qrow, float r, const RangeArgs& a,
                                        long long row0, long long rows, long long out0,
                                        unsigned long long& ran) {
    const int lane = threadIdx.x;
    int hits = 0;
#pragma unroll 1
    for (long long base = 0; base < rows; base += 64) {
        const long long v = row0 + base + lane;
        bool valid = base + lane < rows;
        if (valid && a.keep) valid = ((a.keep[v >> 5] >> (v & 31)) & 1u) != 0u;
        const unsigned long long m = __ballot(valid);
        if (!m) continue;   // (wave-uniform)
        const float* const qp[1] = {qrow};
        const T* const xp[1] = {static_cast<const T*>(a.x) + (valid ? v : row0 + base) * a.ld_x};
        float dist[1];
        chains<IP, 1, T>(qp, xp, a.d, a.vec_chain != 0, dist);
        const bool hit = valid && dist[0] < r;
        const unsigned long long hb = __ballot(hit);
        if constexpr (FILL) {
            const long long p = out0 + hits + __popcll(hb & ((1ull << lane) - 1ull));
            if (hit && p < a.capacity) a.dist[p] = dist[0], a.ids[p] = a.id_base + v;
        }
        hits += __popcll(hb);
        ran += (unsigned long long)__popcll(m);
    }
    return hits;
}

template <bool IP, bool FILL, typename T>
__global__ void __launch_bounds__(64)
flat_range_valu(const RangeArgs a) {
    const int lane = threadIdx.x;
    const long long q = blockIdx.x, slab = blockIdx.y, slabs = gridDim.y;
    long long* const ent = a.plan + kHeaderWords + q * slabs + slab;
    long long out0 = 0;
    if constexpr (FILL) {
        if (!same_geometry(a)) {
            if (q == 0 && slab == 0 && lane == 0) atomicOr(a.err, 2ull);
            return;
        }
        if (q == 0 && slab == 0 && lane == 0) report_fallback<true>(a, slabs, 0);
        out0 = ent[0];
        if (ent[1] == out0) return;
    } else if (q == 0 && slab == 0 && lane == 0) {
        *reinterpret_cast<RangeGeo*>(a.plan) = a.geo;
    }
    const long long row0 = slab * a.slab_rows;
    unsigned long long ran = 0;
    const int hits = all_rows<IP, FILL, T>(a.q + q * a.ld_q, a.radius[q], a, row0,
                                           min(a.slab_rows, a.n - row0), out0, ran);
    if (lane == 0) {
        if constexpr (!FILL) ent[0] = hits;
        if (ran) atomicAdd(a.counts + kDiagChains, ran);
        if (!FILL && slab == 0) report_fallback<false>(a, slabs, 1);
    }
}

// ------------------------------------------------------------------- the screen
// LDS of flat_range, in 4-byte words behind the two tile buffers, per wave: the candidates
// [kFlatCand][64], the drain's prefix [64], the epoch's hit words [32][kEpochStride], and in the
// fill the chains' values [kFlatCand][64] beside the candidates
constexpr int range_wave_words(bool fill) {
    return kFlatCand * 64 * (fill ? 2 : 1) + 64 + 32 * kEpochStride;
}
size_t range_lds_bytes(int P, bool fill) {
    return (size_t)2 * flat_tile_u4(P) * 16 + (size_t)4 * range_wave_words(fill) * 4;
}

template <bool IP, bool FILL, bool PAN, typename XT>
__global__ void __launch_bounds__(256, 1)
flat_range(const RangeArgs a) {
    // bf16 rows are their own high half: no low half is staged and the xl.qh pass is compiled out
    constexpr bool kNoLow = std::is_same_v<XT, __bf16>;
    const XT* const ax = static_cast<const XT*>(a.x);
    constexpr int W = 4, NTHR = 64 * W, PIECES = 64 * kRegPasses / NTHR;
    extern __shared__ u32x4 smem[];
    const int lane = threadIdx.x, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.y);
    const int tid = wave * 64 + lane, h = lane >> 5;
    const int P = a.P;
    const long long slab = blockIdx.y, slabs = gridDim.y;
    long long* const ent = a.plan + kHeaderWords;

    if constexpr (FILL) {
        if (!same_geometry(a)) {
            if (blockIdx.x == 0 && slab == 0 && tid == 0) atomicOr(a.err, 2ull);
            return;
        }
        if (blockIdx.x == 0 && slab == 0 && tid == 0) report_fallback<true>(a, slabs, 0);
        // a workgroup none of whose queries counted a hit in its slab stages nothing
        const long long qg = (long long)blockIdx.x * (32 * W) + tid;
        bool any = false;
        if (tid < 32 * W && qg < a.nq) any = ent[qg * slabs + slab + 1] != ent[qg * slabs + slab];
        if (!__syncthreads_or(any)) return;
    } else if (blockIdx.x == 0 && slab == 0 && tid == 0) {
        *reinterpret_cast<RangeGeo*>(a.plan) = a.geo;
    }

    // a staged unit is one panel of one tile: PU passes, NP panels a tile
    const int PU = min(P, kRegPasses), NP = (P + kRegPasses - 1) / kRegPasses;
    const int st = 2 * PU * 64, tile_u4 = flat_tile_u4(PU);
    u32x4* const tiles = smem;
    int* const words = reinterpret_cast<int*>(smem + 2 * tile_u4);
    int* const cand = words + wave * range_wave_words(FILL);
    int* const pre = cand + kFlatCand * 64;
    unsigned* const hitw = reinterpret_cast<unsigned*>(pre + 64);
    float* const cdist = reinterpret_cast<float*>(hitw + 32 * kEpochStride);   // (FILL)

    const long long row0 = slab * a.slab_rows;
    const long long rows = min(a.slab_rows, a.n - row0);
    const int nt = (int)((rows + 31) >> 5);

    // ---- the wave's queries: the B operand, ||q||^2, whether the ql pass is needed
    const long long qw0 = ((long long)blockIdx.x * W + wave) * 32;
    const bool wave_live = qw0 < a.nq;   // (wave-uniform)
    const long long qi = qw0 + (lane & 31);
    const bool live = qi < a.nq;
    const float* __restrict__ qr = a.q + (live ? qi : a.nq - 1) * a.ld_q;
    bf16x8 Bh[kRegPasses], Bl[kRegPasses];
    float X = 0.f;
    unsigned qlow = 0u;
    // the fragments of panel pn (passes 8 pn ...) into the registers; REG: once, with the sums
    auto make_B = [&](int pn, bool sums) {
#pragma unroll
        for (int p = 0; p < kRegPasses; ++p) {
            if (kRegPasses * pn + p < P) {
                float v[8];
                load8(qr, 16 * (kRegPasses * pn + p) + 8 * h, a.d, a.vec_q != 0, v);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    if (sums) X = X + v[e] * v[e];
                    const float s = IP ? v[e] : 2.f * v[e];
                    const __bf16 hb = (__bf16)s;
                    Bh[p][e] = hb;
                    Bl[p][e] = (__bf16)(s - (float)hb);
                    if (sums) qlow |= __float_as_uint(s) & 0xFFFFu;
                }
            }
        }
    };
    if constexpr (PAN) {   // the fragments are made again per panel; here only the sums
#pragma unroll 1
        for (int p = 0; p < P; ++p) {
            float v[8];
            load8(qr, 16 * p + 8 * h, a.d, a.vec_q != 0, v);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                X = X + v[e] * v[e];
                qlow |= __float_as_uint(IP ? v[e] : 2.f * v[e]) & 0xFFFFu;
            }
        }
    } else {
        make_B(0, true);
    }
    X = X + __shfl_xor(X, 32);
    const bool any_qlo = __ballot(qlow != 0u) != 0ull;
    // tau: DESIGN.md 4.5.17.  Not below 2^110 (NaN included): the all-rows path
    const float Q = X + __uint_as_float(*a.cmax);
    const float tau = a.kq * Q + 0x1p-100f;
    const bool fb = !(tau < 0x1p110f);
    const bool active = live && !fb;

    // ---- the threshold, fixed: a score is a candidate iff it is <= T.
    // NaN: no hit.  Above 4 Q every kept row is a candidate (the margin's premise, and nearly
    // all of them are hits); L2 at or below 0, IP below -4 Q: no distance is below r
    const float r = live ? a.radius[qi] : NAN;
    float T = -INFINITY;
    if (active && r > 4.f * Q) {
        T = INFINITY;
    } else if (active && (IP ? r >= -4.f * Q : r > 0.f)) {
        T = (IP ? r : r - X) + tau;
    }
    long long off = 0;   // FILL: where the query's hits of this slab begin, and how many
    int todo = 0;
    if constexpr (FILL) {
        if (live) {
            off = ent[qi * slabs + slab];
            todo = (int)(ent[qi * slabs + slab + 1] - off);
        }
        if (todo == 0) T = -INFINITY;
    }

    for (int i = lane; i < 32 * kEpochStride; i += 64) hitw[i] = 0u;
    int cnt = 0;        // the lane's pending candidates
    int found = 0;      // the query's hits in the epochs closed so far
    int et0 = 0;        // the epoch's first tile
    bool dirty = false;   // the epoch has a hit (wave-uniform)
    unsigned long long ran = 0;
    wave_sync();

    // pending pair pc of the wave: its lane (the largest whose first pair is at or before pc;
    // pre[0] = 0, so that lane has pairs, pc among them) and its slot in the lane's buffer
    auto locate = [&](int pc, int& lo) {
        int hi = 63;
        lo = 0;
#pragma unroll
        for (int it = 0; it < 6; ++it) {
            const int mid = (lo + hi + 1) >> 1;
            const bool le = pre[mid] <= pc;
            lo = le ? mid : lo;
            hi = le ? hi : mid - 1;
        }
        return (pc - pre[lo]) * 64 + lo;
    };

    // the pending pairs of the wave, lane = pair: the chain, the compare, the hit's bit; then
    // (FILL), every bit of the drain set, the hits' ranks and their entries
    auto drain = [&]() {
        int incl = cnt;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const int v = __shfl_up(incl, s);
            if (lane >= s) incl += v;
        }
        const int total = __shfl(incl, 63);
        pre[lane] = incl - cnt;
        wave_sync();
#pragma unroll 1
        for (int p0 = 0; p0 < total; p0 += 64 * kChainU) {
            int ql[kChainU], rw[kChainU], slot[kChainU];
            const float* qp[kChainU];
            const XT* xp[kChainU];
            float dist[kChainU];
#pragma unroll
            for (int u = 0; u < kChainU; ++u) {
                const int p = p0 + 64 * u + lane;
                int lo;
                slot[u] = locate(p < total ? p : 0, lo);
                // (a lane past the last pair reads pair 0's slot, which the fill may have marked)
                rw[u] = max(cand[slot[u]], 0);
                ql[u] = lo & 31;
                qp[u] = a.q + (qw0 + ql[u]) * a.ld_q;
                xp[u] = ax + (row0 + rw[u]) * a.ld_x;
            }
            chains<IP, kChainU, XT>(qp, xp, a.d, a.vec_chain != 0, dist);
#pragma unroll
            for (int u = 0; u < kChainU; ++u) {
                const bool ok = p0 + 64 * u + lane < total;
                const float ru = __shfl(r, ql[u]);
                const bool hit = ok && dist[u] < ru;
                if (hit) atomicOr(hitw + ql[u] * kEpochStride + ((rw[u] >> 5) - et0), 1u << (rw[u] & 31));
                dirty = dirty || __ballot(hit) != 0ull;
                if constexpr (FILL) {
                    if (ok) cand[slot[u]] = hit ? rw[u] : -1, cdist[slot[u]] = dist[u];
                }
            }
        }
        ran += (unsigned long long)total;
        cnt = 0;
        if constexpr (FILL) {
            wave_sync();
#pragma unroll 1
            for (int p0 = 0; p0 < total; p0 += 64) {
                const int p = p0 + lane;
                int lo;
                const int sl = locate(p < total ? p : 0, lo);
                const int row = p < total ? cand[sl] : -1;
                const long long at = __shfl(off + found, lo & 31);
                if (row >= 0) {
                    const unsigned* hw = hitw + (lo & 31) * kEpochStride;
                    const int e = (row >> 5) - et0;
                    int rank = __popc(hw[e] & ((1u << (row & 31)) - 1u));
                    for (int i = 0; i < e; ++i) rank += __popc(hw[i]);
                    if (at + rank < a.capacity) {
                        a.dist[at + rank] = cdist[sl];
                        a.ids[at + rank] = a.id_base + row0 + row;
                    }
                }
            }
            wave_sync();   // (the buffers are appended to again)
        }
    };

    // the end of an epoch: what is pending is drained, the epoch's hits join the queries' counts
    // and the words are cleared; half-wave h sums one half of its query's words
    auto close_epoch = [&]() {
        if (__ballot(cnt > 0)) drain();
        if (!dirty) return;
        int s = 0;
#pragma unroll 4
        for (int i = 0; i < kEpoch / 2; ++i) {
            unsigned* w = hitw + (lane & 31) * kEpochStride + h * (kEpoch / 2) + i;
            s += __popc(*w);
            *w = 0u;
        }
        found += s + __shfl_xor(s, 32);
        dirty = false;
        if constexpr (FILL) {
            if (found == todo) T = -INFINITY;   // everything counted is written
        }
        wave_sync();
    };

    // ---- the units.  Thread tid converts the pieces k * NTHR + tid of a unit: piece = (pass of
    // the panel, fragment lane), eight values of one row
    // (16-bit rows wait as the four packed dwords they are in memory)
    std::conditional_t<kRows16<XT>, u32x4, float[8]> pre_v[PIECES];
    float pre_n = 0.f;
    unsigned pre_m = 0u;
    auto fetch = [&](int t, int pn) {
        const long long trow = row0 + 32ll * t;
#pragma unroll
        for (int kk = 0; kk < PIECES; ++kk) {
            const int pc = min(kk * NTHR + tid, 64 * PU - 1);   // (no branch around a load)
            const int li = pc & 63, pg = kRegPasses * pn + (pc >> 6);
            const long long row = trow + (li & 31);
            const bool in = row < a.n && pg < P;   // (the last panel may have fewer passes)
            if constexpr (kRows16<XT>) {
                pre_v[kk] = load8_packed<XT>(ax + min(row, a.n - 1) * a.ld_x,
                                            16 * min(pg, P - 1) + 8 * (li >> 5), a.d, a.vec_x != 0);
#pragma unroll
                for (int e = 0; e < 4; ++e) pre_v[kk][e] = in ? pre_v[kk][e] : 0u;
            } else {
                load8(ax + min(row, a.n - 1) * a.ld_x, 16 * min(pg, P - 1) + 8 * (li >> 5), a.d,
                      a.vec_x != 0, pre_v[kk]);
#pragma unroll
                for (int e = 0; e < 8; ++e) pre_v[kk][e] = in ? pre_v[kk][e] : 0.f;
            }
        }
        // the norms start the accumulator at a tile's first panel, the word is read after its
        // last: the panels between carry neither (pn is workgroup-uniform)
        if (pn == 0) {
            const long long rown = trow + (tid & 31);
            const float nv = IP ? 0.f : a.norms[min(rown, a.n - 1)];
            pre_n = rown < a.n ? nv : INFINITY;
        }
        // the tile's rows that take part: kept, and below n (trow < n: the word exists)
        unsigned word = 0u;
        if (pn == NP - 1) {
            word = a.keep ? a.keep[trow >> 5] : ~0u;
            const long long left = a.n - trow;
            if (left < 32) word &= (1u << (int)left) - 1u;
        }
        pre_m = word;
    };
    auto stash = [&](u32x4* dst) {
        unsigned low = 0u;
#pragma unroll
        for (int kk = 0; kk < PIECES; ++kk) {
            const int piece = kk * NTHR + tid;
            if constexpr (kNoLow) {
                // h = -x: a sign flip of the packed words; there is no low half
                if (piece < 64 * PU) dst[piece] = pre_v[kk] ^ 0x80008000u;
            } else if (piece < 64 * PU) {
                bf16x8 hi, lo;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float c;
                    if constexpr (kRows16<XT>) {
                        c = -(e & 1 ? half_hi<XT>(pre_v[kk][e >> 1]) : half_lo<XT>(pre_v[kk][e >> 1]));
                    } else {
                        c = -pre_v[kk][e];
                    }
                    const __bf16 hb = (__bf16)c;
                    hi[e] = hb;
                    lo[e] = (__bf16)(c - (float)hb);
                    low |= __float_as_uint(c) & 0xFFFFu;
                }
                dst[piece] = __builtin_bit_cast(u32x4, hi);           // [p][fragment lane]
                dst[64 * PU + piece] = __builtin_bit_cast(u32x4, lo);
            }
        }
        if (tid < 32) reinterpret_cast<float*>(dst + st)[tid] = pre_n;
        const bool any = __ballot(low != 0u) != 0ull;
        if (lane == 0) {
            reinterpret_cast<unsigned*>(dst + st + 9)[wave] = any ? 1u : 0u;
            if (wave == 0) reinterpret_cast<unsigned*>(dst + st + 8)[0] = pre_m;
        }
    };

    // Unit order: tile by tile, inside a tile panel by panel; the accumulator lives across a
    // tile's panels, the B fragments of a panel are made again before each unit (PAN)
    f32x16 acc;
    int u = 0;
    fetch(0, 0);
    stash(tiles);
    lds_barrier();
#pragma unroll 1
    for (int t = 0; t < nt; ++t) {
#pragma unroll 1
        for (int pn = 0; pn < NP; ++pn) {
            if constexpr (PAN) {
                if (wave_live) make_B(pn, false);
            }
            const u32x4* cur = tiles + (u & 1) * tile_u4;
            const bool down = pn + 1 < NP, more = down || t + 1 < nt;   // the unit after this one
            if (more) fetch(down ? t : t + 1, down ? pn + 1 : 0);
            if (wave_live) {
                const u32x4 flags = cur[st + 9];
                const bool any_xlo = __builtin_amdgcn_readfirstlane(
                                             (int)(flags[0] | flags[1] | flags[2] | flags[3])) != 0;
                if (pn == 0) {
                    const float* cnp = reinterpret_cast<const float*>(cur + st);
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const f32x4 c4 = *reinterpret_cast<const f32x4*>(cnp + 8 * c + 4 * h);
                        acc[4 * c] = c4[0], acc[4 * c + 1] = c4[1], acc[4 * c + 2] = c4[2],
                                acc[4 * c + 3] = c4[3];
                    }
                }
#pragma unroll
                for (int p = 0; p < kRegPasses; ++p) {
                    if (kRegPasses * pn + p < P) {
                        const bf16x8 ah = __builtin_bit_cast(bf16x8, cur[p * 64 + lane]);
                        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, Bh[p], acc, 0, 0, 0);
                        if (!kNoLow && any_xlo) {
                            const bf16x8 al = __builtin_bit_cast(bf16x8, cur[(PU + p) * 64 + lane]);
                            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, Bh[p], acc, 0, 0, 0);
                        }
                        if (any_qlo)
                            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, Bl[p], acc, 0, 0, 0);
                    }
                }
                if (!down) {   // the tile's scores are complete
                    const unsigned word = (unsigned)__builtin_amdgcn_readfirstlane(
                            (int)reinterpret_cast<const unsigned*>(cur + st + 8)[0]);
                    // register i of half-wave h is row (i & 3) + 8 (i >> 2) + 4 h of the tile
                    float m = fmin2(acc[0], acc[1]);
#pragma unroll
                    for (int i = 2; i < 16; i += 2) m = fmin2(m, fmin2(acc[i], acc[i + 1]));
                    const bool go = m <= T;
                    if (word && __ballot(go)) {   // (wave-uniform)
                        if (__ballot(cnt > kFlatCand - 16)) drain();
#pragma unroll
                        for (int i = 0; i < 16; ++i) {
                            const int rr = (i & 3) + 8 * (i >> 2) + 4 * h;
                            if (go && acc[i] <= T && ((word >> rr) & 1u)) {
                                cand[cnt * 64 + lane] = 32 * t + rr;
                                ++cnt;
                            }
                        }
                    }
                    if (t + 1 == nt || (t + 1) % kEpoch == 0) {
                        close_epoch();
                        et0 = t + 1;
                    }
                }
            }
            // the other buffer was last read before the barrier that ended the unit before
            if (more) stash(tiles + ((u + 1) & 1) * tile_u4);
            lds_barrier();
            ++u;
        }
    }

    if (!wave_live) return;   // (no barrier follows)

    // ---- the queries that cannot trust a score: all rows of the slab
    unsigned long long fa = __ballot(fb && live && h == 0);
    const int nfb = __popcll(fa);
    while (fa) {
        const int f = __builtin_ctzll(fa);
        fa &= fa - 1;
        const int hits = all_rows<IP, FILL, XT>(a.q + (qw0 + f) * a.ld_q, __shfl(r, f), a, row0, rows,
                                                __shfl(off, f), ran);
        if ((lane & 31) == f) found = hits;
    }

    if constexpr (!FILL) {
        if (lane < 32 && live) ent[qi * slabs + slab] = found;
    }
    if (lane == 0) {
        if (ran) atomicAdd(a.counts + kDiagChains, ran);
        if (!FILL && slab == 0) report_fallback<false>(a, slabs, nfb);
    }
}

// ------------------------------------------------------------------- the host side
// The slabs of a call: pqh_flat_search's rule (about one workgroup per compute unit, eight waves
// for the VALU kernel, multiples of 32 rows, kMinSlab at least); the context's search_groups
// tuning sets the slabs a query group's rows are cut into outright.
struct Geometry {
    bool screen, pan;
    long long groups, slab_rows;
    int slabs;
};

Geometry geometry(const pqh_ctx* ctx, const pqh_flat* flat, long long nq) {
    Geometry g;
    g.screen = flat->d <= 16 * kMaxPasses;
    g.pan = flat->d > 16 * kRegPasses;
    g.groups = g.screen ? (nq + 127) / 128 : nq;
    const long long cap = (long long)ctx->num_cus * (g.screen ? 1 : 8);
    long long target = cap / g.groups > 1 ? cap / g.groups : 1;
    if (ctx->tune_search_groups > 0) target = ctx->tune_search_groups;
    g.slab_rows = ((flat->n + target - 1) / target + 31) / 32 * 32;
    if (g.slab_rows < kMinSlab) g.slab_rows = kMinSlab;
    g.slabs = (int)((flat->n + g.slab_rows - 1) / g.slab_rows);
    return g;
}

unsigned long long plan_bytes_of(const Geometry& g, long long nq) {
    return ((unsigned long long)kHeaderWords + (unsigned long long)nq * g.slabs + 2) * 8;
}

template <bool IP, bool FILL, bool PAN, typename T>
int screen_launch(pqh_ctx* ctx, const RangeArgs& a, const Geometry& g) {
    const size_t lds = range_lds_bytes(a.P < kRegPasses ? a.P : kRegPasses, FILL);
    const auto fn = flat_range<IP, FILL, PAN, T>;
    // more than 64 KB of dynamic LDS is granted once per instantiation and device (the bitmap
    // holds devices 0 to 63; a device beyond them is granted again on every call)
    static std::atomic<unsigned long long> granted{0};
    const unsigned long long bit = ctx->device < 64 ? 1ull << ctx->device : 0ull;
    if (lds > 64 * 1024 && !(granted.load() & bit)) {
        PQH_HIP(ctx, hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)range_lds_bytes(kRegPasses, FILL)));
        granted.fetch_or(bit);
    }
    hipLaunchKernelGGL(fn, dim3((unsigned)g.groups, (unsigned)g.slabs), dim3(64, 4), lds,
                       ctx->stream, a);
    PQH_LAUNCH_CHECK(ctx);
    return PQH_OK;
}

template <bool IP, bool FILL, typename T>
int range_launch(pqh_ctx* ctx, const RangeArgs& a, const Geometry& g) {
    if (!g.screen) {
        hipLaunchKernelGGL((flat_range_valu<IP, FILL, T>), dim3((unsigned)a.nq, (unsigned)g.slabs),
                           dim3(64), 0, ctx->stream, a);
        PQH_LAUNCH_CHECK(ctx);
        return PQH_OK;
    }
    return g.pan ? screen_launch<IP, FILL, true, T>(ctx, a, g) : screen_launch<IP, FILL, false, T>(ctx, a, g);
}

template <bool IP, bool FILL>
int flat_range_call(pqh_ctx_t* ctx, const pqh_flat_t* flat, const float* d_queries, long long nq,
                    long long ld_q, const float* d_radius, const unsigned int* d_keep_bits,
                    void* d_plan, unsigned long long plan_bytes, long long* d_lims,
                    long long capacity, long long id_base, float* d_dist, long long* d_ids) {
    if (!ctx) return pqh_no_ctx_status();
    if (!flat || flat->ctx != ctx || nq < 0 || ld_q < flat->d || !d_lims) return PQH_ERR_ARG;
    if (nq > 0 && (!d_queries || !d_radius || !d_plan)) return PQH_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(d_plan) | reinterpret_cast<uintptr_t>(d_lims)) & 7u)
        return PQH_ERR_ARG;
    if (d_keep_bits && (reinterpret_cast<uintptr_t>(d_keep_bits) & 3u)) return PQH_ERR_ARG;
    if (FILL && (capacity < 0 || (capacity > 0 && (!d_dist || !d_ids)) || id_base < 0 ||
                 id_base > 0x7FFFFFFFFFFFFFFFll - flat->n))
        return PQH_ERR_ARG;
    if (nq > 0x7FFFFFFFll) return PQH_ERR_UNSUPPORTED;
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    if (nq == 0) return PQH_OK;
    // (without rows the fill has nothing to write: lims is the count's)
    if (flat->n == 0) return FILL ? PQH_OK : pqh_range_no_rows_launch(ctx, nq, d_lims);

    const Geometry g = geometry(ctx, flat, nq);
    if (plan_bytes < plan_bytes_of(g, nq)) return PQH_ERR_ARG;
    const int d = flat->d;
    RangeArgs a{};
    a.x = flat->d_x, a.n = flat->n, a.ld_x = flat->ld_x, a.d = d, a.P = (d + 15) / 16;
    a.norms = flat->d_norms, a.cmax = flat->d_cmax;
    a.q = d_queries, a.nq = nq, a.ld_q = ld_q, a.radius = d_radius, a.keep = d_keep_bits;
    a.slab_rows = g.slab_rows;
    a.kq = screen_kq(16 * a.P);
    // float4 loads where every piece lies inside a row and on 16 bytes
    // (16 bytes are eight elements of a 16-bit row)
    const int per16 = flat->rows == PQH_ROWS_F32 ? 4 : 8;
    const bool x16 = flat->ld_x % per16 == 0 && aligned16(flat->d_x);
    const bool q16 = ld_q % 4 == 0 && aligned16(d_queries);
    a.vec_x = d % 16 == 0 && x16;
    a.vec_q = d % 16 == 0 && q16;
    a.vec_chain = d % per16 == 0 && x16 && q16;
    a.plan = static_cast<long long*>(d_plan);
    a.geo = RangeGeo{kPlanMagic, nq, flat->n, g.slabs, g.groups, g.slab_rows, kEpoch, d};
    a.capacity = capacity, a.id_base = id_base, a.dist = d_dist, a.ids = d_ids;
    a.counts = ctx->d_diag, a.err = ctx->d_diag + 1;

    hipLaunchKernelGGL(range_clear, dim3(1), dim3(1), 0, ctx->stream, ctx->d_diag,
                       FILL ? nullptr : a.plan + kHeaderWords + nq * g.slabs + 1);
    PQH_LAUNCH_CHECK(ctx);
    rc = flat->rows == PQH_ROWS_F16    ? range_launch<IP, FILL, _Float16>(ctx, a, g)
         : flat->rows == PQH_ROWS_BF16 ? range_launch<IP, FILL, __bf16>(ctx, a, g)
                                       : range_launch<IP, FILL, float>(ctx, a, g);
    if (rc || FILL) return rc;
    return pqh_range_offsets_launch(ctx, a.plan + kHeaderWords, g.slabs, nq, d_lims);
}

}  // namespace

extern "C" {

int pqh_flat_range_plan_bytes(pqh_ctx_t* ctx, const pqh_flat_t* flat, long long nq,
                              unsigned long long* bytes) {
    if (!ctx) return pqh_no_ctx_status();
    if (!flat || flat->ctx != ctx || !bytes || nq < 0) return PQH_ERR_ARG;
    if (nq > 0x7FFFFFFFll) return PQH_ERR_UNSUPPORTED;
    *bytes = (kHeaderWords + 2) * 8;
    if (nq > 0 && flat->n > 0) *bytes = plan_bytes_of(geometry(ctx, flat, nq), nq);
    return PQH_OK;
}

int pqh_flat_range_count(pqh_ctx_t* ctx, const pqh_flat_t* flat, const float* d_queries,
                         long long nq, long long ld_q, const float* d_radius,
                         const unsigned int* d_keep_bits, void* d_plan,
                         unsigned long long plan_bytes, long long* d_lims) {
    return flat_range_call<false, false>(ctx, flat, d_queries, nq, ld_q, d_radius, d_keep_bits,
                                         d_plan, plan_bytes, d_lims, 0, 0, nullptr, nullptr);
}

int pqh_flat_range_count_ip(pqh_ctx_t* ctx, const pqh_flat_t* flat, const float* d_queries,
                            long long nq, long long ld_q, const float* d_radius,
                            const unsigned int* d_keep_bits, void* d_plan,
                            unsigned long long plan_bytes, long long* d_lims) {
    return flat_range_call<true, false>(ctx, flat, d_queries, nq, ld_q, d_radius, d_keep_bits,
                                        d_plan, plan_bytes, d_lims, 0, 0, nullptr, nullptr);
}

int pqh_flat_range_fill(pqh_ctx_t* ctx, const pqh_flat_t* flat, const float* d_queries,
                        long long nq, long long ld_q, const float* d_radius,
                        const unsigned int* d_keep_bits, const void* d_plan,
                        unsigned long long plan_bytes, const long long* d_lims,
                        long long capacity, long long id_base, float* d_dist, long long* d_ids) {
    return flat_range_call<false, true>(ctx, flat, d_queries, nq, ld_q, d_radius, d_keep_bits,
                                        const_cast<void*>(d_plan), plan_bytes,
                                        const_cast<long long*>(d_lims), capacity, id_base, d_dist,
                                        d_ids);
}

int pqh_flat_range_fill_ip(pqh_ctx_t* ctx, const pqh_flat_t* flat, const float* d_queries,
                           long long nq, long long ld_q, const float* d_radius,
                           const unsigned int* d_keep_bits, const void* d_plan,
                           unsigned long long plan_bytes, const long long* d_lims,
                           long long capacity, long long id_base, float* d_dist,
                           long long* d_ids) {
    return flat_range_call<true, true>(ctx, flat, d_queries, nq, ld_q, d_radius, d_keep_bits,
                                       const_cast<void*>(d_plan), plan_bytes,
                                       const_cast<long long*>(d_lims), capacity, id_base, d_dist,
                                       d_ids);
}

}  // extern "C"
