// pqh_flat.hip -- the exact search: the k nearest of a set of raw fp32 rows for a batch of
// queries, by the definition's own chain (pqh_coarse_assign's direct form) run only for the
// (query, row) pairs a bf16-split MFMA screen cannot rule out.
//
//  flat_norms     once per data set: ||x_v||^2 summed in double and rounded once to fp32, and
//                 Cmax, their maximum by atomicMax on the bits (screen_norms' rule: a non-finite
//                 row leaves a Cmax that fails every query's tau test).
//  flat_screen<IP, KR, PAN>  d <= 1024.  Grid (query groups) x (row slabs).  A wave owns 32 queries,
//                 the MFMA's B operand, 2q (L2) or q (IP) as qh | ql in registers; a workgroup
//                 of four waves (one with the wide list) streams the slab's rows past them in
//                 tiles of 32: a tile is read from global memory once per workgroup, negated
//                 and split into xh | xl on the way into a double buffer in LDS, in the A
//                 operand's fragment order, its 32 row norms (the accumulator start, 0 for IP)
//                 and its mask word beside it; the loads of tile t + 1 are issued before the
//                 MFMAs of tile t, one barrier per tile.  Passes xh.qh, xl.qh (skipped when
//                 the tile is bf16-exact), xh.ql (skipped when the wave's queries are).
//                 Score S = ||x||^2 - 2 q.x (= D - ||q||^2), or -q.x.  A query's running list
//                 in LDS holds EXACT (dist, row) pairs; a score is a candidate iff
//                 S <= (Dkth - ||q||^2) + tau (IP: Dkth + tau), Dkth the list's k-th distance
//                 (+inf until it is full).  A lane reduces its 16 scores to a minimum and walks
//                 them only when the minimum passes; candidates go to the lane's buffer in LDS
//                 ([e][lane]), which the wave drains at a wave-uniform point (some lane's
//                 buffer past half, and the slab's end): lane = pending pair, four pairs a
//                 lane in flight, the definition's chain from the fp32 rows, the results
//                 offered to the query's list with list_offer.  A query whose tau is not below
//                 2^110 takes the all-rows path for the slab.
//                 PAN (d > 128): d walked in panels of 128 through the same double buffer, the
//                 accumulator kept across a tile's panels, the B fragments of a panel made
//                 again from the fp32 queries before each unit.
//  flat_valu<IP, KR>  d > 1024, and the all-rows path: one wave per (query, slab), lane = row,
//                 the chain per lane, the same lists.
//  Every (slab, query) writes its exact top k with global ids to the workspace
//  [slabs][nq][k]; pqh_topk_merge reduces them (one slab: straight into the result).
#include <atomic>
#include <cmath>
#include <new>
#include <type_traits>

#include "pqh_flat_dev.h"
#include "pqh_flat_screen_dev.h"
#include "pqh_internal.h"
#include "pqh_screen_dev.h"
#include "pqh_topk_dev.h"

namespace {

// panel form: the tiles a panel's B fragments serve before the next panel's are made.  Two
// halve the conversions, but the selection is then compiled twice and spills to scratch
constexpr int kPanelTiles = 1;

struct FlatArgs {
    const void* x;       // the rows, elements of the kernel's row type T
    long long n, ld_x;
    int d, P;
    const float* norms;
    const unsigned* cmax;
    const float* q;
    long long nq, ld_q;
    int k;
    const unsigned* keep;
    long long id_base, slab_rows;
    float kq;
    int vec_x, vec_q, vec_chain;
    float* out_d;
    long long* out_id;
    unsigned long long* counts;
};

__global__ void flat_clear(unsigned long long* counts, unsigned* cmax) {
    if (counts) counts[kDiagChains] = 0, counts[kDiagFallback] = 0;
    if (cmax) *cmax = 0u;
}

template <typename T>
__global__ void __launch_bounds__(256)
flat_norms(const T* __restrict__ x, long long n, long long ld_x, int d,
           float* __restrict__ norms, unsigned* __restrict__ cmax) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    unsigned bits = 0u;
    if (v < n) {
        double s = 0.0;
        for (int j = 0; j < d; ++j) {
            const double c = (float)x[v * ld_x + j];
            s += c * c;
        }
        const float f = (float)s;
        norms[v] = f;
        bits = __float_as_uint(f);
    }
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) bits = max(bits, (unsigned)__shfl_xor((int)bits, s));
    if ((threadIdx.x & 63) == 0 && bits) atomicMax(cmax, bits);
}

// the all-rows path of one query over one slab: lane = row, the chain for every kept row.
// Returns the number of chains run (wave-uniform).
template <bool IP, int KR, typename T>
__device__ __forceinline__ unsigned long long all_rows(ListT<KR>& e, const float* __restrict__ qrow,
                                                       const FlatArgs& a, long long row0,
                                                       long long rows, int kth) {
    const int lane = threadIdx.x;
    unsigned long long ran = 0;
#pragma unroll 1
    for (long long base = 0; base < rows; base += 64) {
        const long long r = base + lane;
        bool valid = r < rows;
        if (valid && a.keep) {
            const long long v = row0 + r;
            valid = ((a.keep[v >> 5] >> (v & 31)) & 1u) != 0u;
        }
        const unsigned long long m = __ballot(valid);
        if (!m) continue;   // (wave-uniform)
        const float* const qp[1] = {qrow};
        const T* const xp[1] = {static_cast<const T*>(a.x) + (row0 + (valid ? r : base)) * a.ld_x};
        float dist[1];
        chains<IP, 1, T>(qp, xp, a.d, a.vec_chain != 0, dist);
        list_offer<false>(e, dist[0], r, valid, kth);
        ran += (unsigned long long)__popcll(m);
    }
    return ran;
}

template <bool IP, int KR, typename T>
__global__ void __launch_bounds__(64)
flat_valu(const FlatArgs a) {
    const int lane = threadIdx.x;
    const long long q = blockIdx.x, slab = blockIdx.y;
    const long long row0 = slab * a.slab_rows;
    const long long rows = min(a.slab_rows, a.n - row0);
    const int k = a.k;
    ListT<KR> e;
    list_reset<KR>(e);
    const unsigned long long ran = all_rows<IP, KR, T>(e, a.q + q * a.ld_q, a, row0, rows, k - 1);
    const long long at = (slab * a.nq + q) * k;
    if constexpr (KR == 1) {
        if (lane < k) {
            a.out_d[at + lane] = e.d;
            a.out_id[at + lane] = e.id < 0 ? -1ll : a.id_base + row0 + e.id;
        }
    } else {
#pragma unroll
        for (int b = 0; b < kWideKR; ++b) {
            if (b * 64 + lane < k) {
                a.out_d[at + b * 64 + lane] = e.d[b];
                a.out_id[at + b * 64 + lane] = e.id[b] < 0 ? -1ll : a.id_base + row0 + e.id[b];
            }
        }
    }
    if (lane == 0 && a.counts) {
        if (ran) atomicAdd(a.counts + kDiagChains, ran);
        if (slab == 0) atomicAdd(a.counts + kDiagFallback, 1ull);
    }
}

// ------------------------------------------------------------------- the screen
// LDS of flat_screen, in 4-byte words behind the two tile buffers: per wave the candidates
// [kFlatCand][64], the drain's prefix [64] and the k-th distances [32], then the lists
// [W][32][k] floats and [W][32][k] rows
__host__ __device__ constexpr int flat_wave_words() { return kFlatCand * 64 + 64 + 32; }
size_t flat_lds_bytes(int P, int W, int k) {
    return (size_t)2 * flat_tile_u4(P) * 16 + (size_t)W * flat_wave_words() * 4 +
           (size_t)W * 32 * k * 8;
}

template <bool IP, int KR, bool PAN, typename XT>
__global__ void __launch_bounds__(KR == 1 ? 256 : 64, 1)
flat_screen(const FlatArgs a) {
    // bf16 rows are their own high half: no low half is staged and the xl.qh pass is compiled out
    constexpr bool kNoLow = std::is_same_v<XT, __bf16>;
    const XT* const ax = static_cast<const XT*>(a.x);
    constexpr int W = KR == 1 ? 4 : 1, NTHR = 64 * W, PIECES = 64 * kRegPasses / NTHR;
    constexpr int TG = PAN ? kPanelTiles : 1;   // tiles whose accumulators a wave keeps
    extern __shared__ u32x4 smem[];
    const int lane = threadIdx.x, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.y);
    const int tid = wave * 64 + lane, h = lane >> 5;
    const int P = a.P, k = a.k, kth = k - 1;
    // a staged unit is one panel of one tile: PU passes, NP panels a tile
    const int PU = min(P, kRegPasses), NP = (P + kRegPasses - 1) / kRegPasses;
    const int st = 2 * PU * 64, tile_u4 = flat_tile_u4(PU);
    u32x4* const tiles = smem;
    int* const words = reinterpret_cast<int*>(smem + 2 * tile_u4);
    int* const cand = words + wave * flat_wave_words();
    int* const pre = cand + kFlatCand * 64;
    float* const thr = reinterpret_cast<float*>(pre + 64);
    float* const lds_d = reinterpret_cast<float*>(words + W * flat_wave_words()) + (size_t)wave * 32 * k;
    int* const lds_i = words + W * flat_wave_words() + (size_t)W * 32 * k + (size_t)wave * 32 * k;

    const long long row0 = (long long)blockIdx.y * a.slab_rows;
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
    const float tau = a.kq * (X + __uint_as_float(*a.cmax)) + 0x1p-100f;
    const bool fb = !(tau < 0x1p110f);
    const bool active = live && !fb;

    // ---- the lists of the wave's queries, empty
    for (int i = lane; i < 32 * k; i += 64) lds_d[i] = INFINITY, lds_i[i] = -1;
    if (lane < 32) thr[lane] = INFINITY;
    float T = active ? INFINITY : -INFINITY;   // a score is a candidate iff it is <= T
    int cnt = 0;
    unsigned long long ran = 0;

    // the pending pairs of the wave, lane = pair: the chain, then the offers query by query
    auto drain = [&]() {
        int incl = cnt;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const int v = __shfl_up(incl, s);
            if (lane >= s) incl += v;
        }
        const int total = __shfl(incl, 63);
        pre[lane] = incl - cnt;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll 1
        for (int p0 = 0; p0 < total; p0 += 64 * kChainU) {
            int ql[kChainU], rw[kChainU];
            const float* qp[kChainU];
            const XT* xp[kChainU];
            float dist[kChainU];
#pragma unroll
            for (int u = 0; u < kChainU; ++u) {
                const int p = p0 + 64 * u + lane;
                const int pc = p < total ? p : 0;
                // the largest lane whose first pair is at or before pc (pre[0] = 0): that lane
                // has pairs, pc among them
                int lo = 0, hi = 63;
#pragma unroll
                for (int it = 0; it < 6; ++it) {
                    const int mid = (lo + hi + 1) >> 1;
                    const bool le = pre[mid] <= pc;
                    lo = le ? mid : lo;
                    hi = le ? hi : mid - 1;
                }
                rw[u] = cand[(pc - pre[lo]) * 64 + lo];
                ql[u] = lo & 31;
                qp[u] = a.q + (qw0 + ql[u]) * a.ld_q;
                xp[u] = ax + (row0 + rw[u]) * a.ld_x;
            }
            chains<IP, kChainU, XT>(qp, xp, a.d, a.vec_chain != 0, dist);
#pragma unroll
            for (int u = 0; u < kChainU; ++u) {
                if (p0 + 64 * u >= total) continue;   // (wave-uniform)
                const bool ok = p0 + 64 * u + lane < total;
                unsigned long long rem = __ballot(ok);
                while (rem) {
                    const int qs = __builtin_amdgcn_readfirstlane(__shfl(ql[u], __builtin_ctzll(rem)));
                    const bool mine = ok && ql[u] == qs;
                    ListT<KR> e;
                    list_from_lds<KR>(e, lds_d + qs * k, lds_i + qs * k, k);
                    list_offer<false>(e, dist[u], (long long)rw[u], mine, kth);
                    list_to_lds<KR>(e, lds_d + qs * k, lds_i + qs * k, k);
                    const float dk = list_kth<KR>(e, kth);
                    if (lane == 0) thr[qs] = dk;
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    rem &= ~__ballot(mine);
                }
            }
        }
        ran += (unsigned long long)total;
        cnt = 0;
        const float dk = thr[lane & 31];
        T = active ? (IP ? dk : dk - X) + tau : -INFINITY;
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
        // the tile's rows that take part: kept, and below n; none of a tile past the slab's
        // last (the panel form rounds the tiles up to whole groups)
        unsigned word = 0u;
        if (t < nt && pn == NP - 1) {   // (trow < n: the word exists)
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

    // Unit order: groups of TG tiles; inside a group panel by panel, inside a panel tile by
    // tile, so that the B fragments of a panel are made once per group (REG: one tile, one
    // panel, B made above).  The accumulators of the group's tiles live across its panels.
    const int ng = (nt + TG - 1) / TG;
    f32x16 acc[TG];
    int u = 0;
    fetch(0, 0);
    stash(tiles);
    lds_barrier();
#pragma unroll 1
    for (int g = 0; g < ng; ++g) {
#pragma unroll 1
        for (int pn = 0; pn < NP; ++pn) {
            if constexpr (PAN) {
                if (wave_live) make_B(pn, false);
            }
#pragma unroll
            for (int tt = 0; tt < TG; ++tt) {
                const int t = g * TG + tt;
                const u32x4* cur = tiles + (u & 1) * tile_u4;
                // the unit after this one
                const bool same = tt + 1 < TG, down = pn + 1 < NP;
                const int t1 = same ? t + 1 : down ? g * TG : (g + 1) * TG;
                const int pn1 = same ? pn : down ? pn + 1 : 0;
                const bool more = same || down || g + 1 < ng;
                if (more) fetch(t1, pn1);
                if (wave_live) {
                    const u32x4 flags = cur[st + 9];
                    unsigned xl = flags[0];
                    if constexpr (W > 1) xl |= flags[1] | flags[2] | flags[3];
                    const bool any_xlo = __builtin_amdgcn_readfirstlane((int)xl) != 0;
                    if (pn == 0) {
                        const float* cnp = reinterpret_cast<const float*>(cur + st);
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            const f32x4 c4 = *reinterpret_cast<const f32x4*>(cnp + 8 * c + 4 * h);
                            acc[tt][4 * c] = c4[0], acc[tt][4 * c + 1] = c4[1],
                                    acc[tt][4 * c + 2] = c4[2], acc[tt][4 * c + 3] = c4[3];
                        }
                    }
#pragma unroll
                    for (int p = 0; p < kRegPasses; ++p) {
                        if (kRegPasses * pn + p < P) {
                            const bf16x8 ah = __builtin_bit_cast(bf16x8, cur[p * 64 + lane]);
                            acc[tt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, Bh[p], acc[tt], 0, 0, 0);
                            if (!kNoLow && any_xlo) {
                                const bf16x8 al = __builtin_bit_cast(bf16x8, cur[(PU + p) * 64 + lane]);
                                acc[tt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, Bh[p], acc[tt], 0, 0, 0);
                            }
                            if (any_qlo)
                                acc[tt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, Bl[p], acc[tt], 0, 0, 0);
                        }
                    }
                    if (pn == NP - 1) {   // the tile's scores are complete
                        const unsigned word = (unsigned)__builtin_amdgcn_readfirstlane(
                                (int)reinterpret_cast<const unsigned*>(cur + st + 8)[0]);
                        // register i of half-wave h is row (i & 3) + 8 (i >> 2) + 4 h of the tile
                        float m = fmin2(acc[tt][0], acc[tt][1]);
#pragma unroll
                        for (int i = 2; i < 16; i += 2) m = fmin2(m, fmin2(acc[tt][i], acc[tt][i + 1]));
                        const bool go = active && m <= T;
                        if (word && __ballot(go)) {   // (wave-uniform)
                            if (__ballot(cnt > kFlatCand - 16)) drain();
                            const bool go2 = active && m <= T;   // (a drain only lowers T)
#pragma unroll
                            for (int i = 0; i < 16; ++i) {
                                const int r = (i & 3) + 8 * (i >> 2) + 4 * h;
                                if (go2 && acc[tt][i] <= T && ((word >> r) & 1u)) {
                                    cand[cnt * 64 + lane] = 32 * t + r;
                                    ++cnt;
                                }
                            }
                        }
                    }
                }
                // the other buffer was last read before the barrier that ended the unit before
                if (more) stash(tiles + ((u + 1) & 1) * tile_u4);
                lds_barrier();
                ++u;
            }
        }
    }

    if (!wave_live) return;   // (no barrier follows)
    if (__ballot(cnt > 0)) drain();

    // ---- the queries that cannot trust a score: all rows of the slab
    unsigned long long fa = __ballot(fb && live && h == 0);
    const int nfb = __popcll(fa);
    while (fa) {
        const int r = __builtin_ctzll(fa);
        fa &= fa - 1;
        ListT<KR> e;
        list_reset<KR>(e);
        ran += all_rows<IP, KR, XT>(e, a.q + (qw0 + r) * a.ld_q, a, row0, rows, kth);
        list_to_lds<KR>(e, lds_d + r * k, lds_i + r * k, k);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

    // ---- this slab's part of the result
    const int nqw = (int)min(32ll, a.nq - qw0);
#pragma unroll 1
    for (int r = 0; r < nqw; ++r) {
        const long long at = ((long long)blockIdx.y * a.nq + qw0 + r) * k;
        for (int i = lane; i < k; i += 64) {
            const int id = lds_i[r * k + i];
            a.out_d[at + i] = lds_d[r * k + i];
            a.out_id[at + i] = id < 0 ? -1ll : a.id_base + row0 + id;
        }
    }
    if (lane == 0) {
        if (ran) atomicAdd(a.counts + kDiagChains, ran);
        if (blockIdx.y == 0 && nfb) atomicAdd(a.counts + kDiagFallback, (unsigned long long)nfb);
    }
}

// ------------------------------------------------------------------- the host side
template <bool IP, int KR, bool PAN, typename T>
int screen_launch(pqh_ctx* ctx, const FlatArgs& a, long long groups, int slabs) {
    constexpr int W = KR == 1 ? 4 : 1;
    const size_t lds = flat_lds_bytes(a.P < kRegPasses ? a.P : kRegPasses, W, a.k);
    const auto fn = flat_screen<IP, KR, PAN, T>;
    // more than 64 KB of dynamic LDS is granted once per instantiation and device: the most
    // any call can ask for (a panel of eight passes, the list's largest k).  The bitmap holds
    // devices 0 to 63; a device beyond them has no bit and is granted again on every call
    static std::atomic<unsigned long long> granted{0};
    const unsigned long long bit = ctx->device < 64 ? 1ull << ctx->device : 0ull;
    if (lds > 64 * 1024 && !(granted.load() & bit)) {
        const size_t most = flat_lds_bytes(kRegPasses, W, KR == 1 ? PQH_SEARCH_MAX_K : PQH_SEARCH_MAX_K_WIDE);
        PQH_HIP(ctx, hipFuncSetAttribute((const void*)fn,
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)most));
        granted.fetch_or(bit);
    }
    hipLaunchKernelGGL(fn, dim3((unsigned)groups, (unsigned)slabs), dim3(64, W), lds, ctx->stream,
                       a);
    PQH_LAUNCH_CHECK(ctx);
    return PQH_OK;
}

template <bool IP, int KR, typename T>
int valu_launch(pqh_ctx* ctx, const FlatArgs& a, int slabs) {
    hipLaunchKernelGGL((flat_valu<IP, KR, T>), dim3((unsigned)a.nq, (unsigned)slabs), dim3(64), 0,
                       ctx->stream, a);
    PQH_LAUNCH_CHECK(ctx);
    return PQH_OK;
}

// the kernel of a search over rows of type T
template <typename T>
int flat_launch(bool ip, bool wide, bool screen, bool pan, pqh_ctx* ctx, const FlatArgs& a,
                long long groups, int slabs) {
    if (screen && pan)
        return ip ? (wide ? screen_launch<true, kWideKR, true, T>(ctx, a, groups, slabs)
                        : screen_launch<true, 1, true, T>(ctx, a, groups, slabs))
                : (wide ? screen_launch<false, kWideKR, true, T>(ctx, a, groups, slabs)
                        : screen_launch<false, 1, true, T>(ctx, a, groups, slabs));
    if (screen)
        return ip ? (wide ? screen_launch<true, kWideKR, false, T>(ctx, a, groups, slabs)
                        : screen_launch<true, 1, false, T>(ctx, a, groups, slabs))
                : (wide ? screen_launch<false, kWideKR, false, T>(ctx, a, groups, slabs)
                        : screen_launch<false, 1, false, T>(ctx, a, groups, slabs));
    return ip ? (wide ? valu_launch<true, kWideKR, T>(ctx, a, slabs) : valu_launch<true, 1, T>(ctx, a, slabs))
                : (wide ? valu_launch<false, kWideKR, T>(ctx, a, slabs)
                        : valu_launch<false, 1, T>(ctx, a, slabs));
}

int flat_search(bool ip, pqh_ctx_t* ctx, const pqh_flat_t* flat, const float* d_queries,
                long long nq, long long ld_q, int k, const unsigned int* d_keep_bits,
                long long id_base, float* d_dist, long long* d_ids) {
    if (!ctx) return pqh_no_ctx_status();
    if (!flat || flat->ctx != ctx || nq < 0 || ld_q < flat->d || k < 1 || k > ctx->search_max_k || id_base < 0 ||
        id_base > 0x7FFFFFFFFFFFFFFFll - flat->n)
        return PQH_ERR_ARG;
    if (nq > 0 && (!d_queries || !d_dist || !d_ids)) return PQH_ERR_ARG;
    if (d_keep_bits && (reinterpret_cast<uintptr_t>(d_keep_bits) & 3u)) return PQH_ERR_ARG;
    if (nq > 0x7FFFFFFFll) return PQH_ERR_UNSUPPORTED;
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    if (nq == 0) return PQH_OK;

    const int d = flat->d;
    const bool wide = k > PQH_SEARCH_MAX_K;
    const bool screen = d <= 16 * kMaxPasses && flat->n > 0, pan = d > 16 * kRegPasses;
    FlatArgs a{};
    a.x = flat->d_x, a.n = flat->n, a.ld_x = flat->ld_x, a.d = d, a.P = (d + 15) / 16;
    a.norms = flat->d_norms, a.cmax = flat->d_cmax;
    a.q = d_queries, a.nq = nq, a.ld_q = ld_q, a.k = k, a.keep = d_keep_bits, a.id_base = id_base;
    a.kq = screen_kq(16 * a.P);
    // float4 loads where every piece lies inside a row and on 16 bytes
    // (16 bytes are eight elements of a 16-bit row)
    const int per16 = flat->rows == PQH_ROWS_F32 ? 4 : 8;
    const bool x16 = flat->ld_x % per16 == 0 && aligned16(flat->d_x);
    const bool q16 = ld_q % 4 == 0 && aligned16(d_queries);
    a.vec_x = d % 16 == 0 && x16;
    a.vec_q = d % 16 == 0 && q16;
    a.vec_chain = d % per16 == 0 && x16 && q16;

    // the slabs: about one workgroup per compute unit (the screen's LDS admits one), a wave's
    // worth of them for the VALU kernel; multiples of 32 rows, kMinSlab at least, so that the
    // warm-up of a list stays a small share of the pairs
    const long long groups = screen ? (nq + (wide ? 32 : 128) - 1) / (wide ? 32 : 128) : nq;
    const long long cap = (long long)ctx->num_cus * (screen ? 1 : 8);
    const long long target = cap / groups > 1 ? cap / groups : 1;
    long long slab_rows = ((flat->n + target - 1) / target + 31) / 32 * 32;
    if (slab_rows < kMinSlab) slab_rows = kMinSlab;
    const int slabs = flat->n > 0 ? (int)((flat->n + slab_rows - 1) / slab_rows) : 1;
    a.slab_rows = slab_rows;

    a.out_d = d_dist, a.out_id = d_ids;
    if (slabs > 1) {
        const size_t cnt = (size_t)slabs * nq * k, db = (cnt * 4 + 7) / 8 * 8;
        rc = pqh_ensure_ws(ctx, db + cnt * 8);
        if (rc) return rc;
        a.out_d = static_cast<float*>(ctx->ws);
        a.out_id = reinterpret_cast<long long*>(static_cast<char*>(ctx->ws) + db);
    }
    if (flat->n > 0) {
        hipLaunchKernelGGL(flat_clear, dim3(1), dim3(1), 0, ctx->stream, ctx->d_diag,
                           (unsigned*)nullptr);
        PQH_LAUNCH_CHECK(ctx);
        a.counts = ctx->d_diag;
    }
    rc = flat->rows == PQH_ROWS_F16    ? flat_launch<_Float16>(ip, wide, screen, pan, ctx, a, groups, slabs)
         : flat->rows == PQH_ROWS_BF16 ? flat_launch<__bf16>(ip, wide, screen, pan, ctx, a, groups, slabs)
                                       : flat_launch<float>(ip, wide, screen, pan, ctx, a, groups, slabs);
    if (rc || slabs == 1) return rc;
    return pqh_topk_merge(ctx, a.out_d, a.out_id, slabs, nq, k, nullptr, k, d_dist, d_ids);
}

}  // namespace

extern "C" {

int pqh_flat_create_rows(pqh_ctx_t* ctx, const void* d_x, int rows, long long n, long long ld_x,
                         int d, pqh_flat_t** flat) {
    if (!pqh_rows_ok(rows, d_x)) return PQH_ERR_ARG;
    if (!ctx) return pqh_no_ctx_status();
    if (!flat || n < 0 || d < 1 || ld_x < d || (n > 0 && !d_x)) return PQH_ERR_ARG;
    if (n > 0x7FFFFFFFll) return PQH_ERR_UNSUPPORTED;
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    pqh_flat* f = new (std::nothrow) pqh_flat;
    if (!f) return PQH_ERR_NOMEM;
    f->ctx = ctx, f->d_x = d_x, f->rows = rows, f->n = n, f->ld_x = ld_x, f->d = d;
    const size_t bytes = ((size_t)n + 1) * 4;
    if (hipMalloc(&f->d_norms, bytes) != hipSuccess) {
        (void)hipGetLastError();
        delete f;
        return pqh_set_error(ctx, PQH_ERR_NOMEM, "flat: cannot allocate %zu bytes", bytes);
    }
    f->d_cmax = reinterpret_cast<unsigned*>(f->d_norms + n);
    hipLaunchKernelGGL(flat_clear, dim3(1), dim3(1), 0, ctx->stream,
                       (unsigned long long*)nullptr, f->d_cmax);
    const dim3 nb((unsigned)((n + 255) / 256));
    if (n > 0 && rows == PQH_ROWS_F32)
        hipLaunchKernelGGL(flat_norms<float>, nb, dim3(256), 0, ctx->stream,
                           static_cast<const float*>(d_x), n, ld_x, d, f->d_norms, f->d_cmax);
    else if (n > 0 && rows == PQH_ROWS_F16)
        hipLaunchKernelGGL(flat_norms<_Float16>, nb, dim3(256), 0, ctx->stream,
                           static_cast<const _Float16*>(d_x), n, ld_x, d, f->d_norms, f->d_cmax);
    else if (n > 0)
        hipLaunchKernelGGL(flat_norms<__bf16>, nb, dim3(256), 0, ctx->stream,
                           static_cast<const __bf16*>(d_x), n, ld_x, d, f->d_norms, f->d_cmax);
    if (hipGetLastError() != hipSuccess) {
        (void)hipFree(f->d_norms);
        delete f;
        return pqh_set_error(ctx, PQH_ERR_HIP, "flat: the norm pass failed to launch");
    }
    *flat = f;
    return PQH_OK;
}

int pqh_flat_create(pqh_ctx_t* ctx, const float* d_x, long long n, long long ld_x, int d,
                    pqh_flat_t** flat) {
    return pqh_flat_create_rows(ctx, d_x, PQH_ROWS_F32, n, ld_x, d, flat);
}

int pqh_flat_destroy(pqh_flat_t* flat) {
    if (!flat) return PQH_OK;
    int rc = pqh_use_device(flat->ctx);
    if (!rc && hipStreamSynchronize(flat->ctx->stream) != hipSuccess) rc = PQH_ERR_HIP;
    if (flat->d_norms) (void)hipFree(flat->d_norms);
    delete flat;
    return rc;
}

int pqh_flat_search(pqh_ctx_t* ctx, const pqh_flat_t* flat, const float* d_queries, long long nq,
                    long long ld_q, int k, const unsigned int* d_keep_bits, long long id_base,
                    float* d_dist, long long* d_ids) {
    return flat_search(false, ctx, flat, d_queries, nq, ld_q, k, d_keep_bits, id_base, d_dist, d_ids);
}

int pqh_flat_search_ip(pqh_ctx_t* ctx, const pqh_flat_t* flat, const float* d_queries,
                       long long nq, long long ld_q, int k, const unsigned int* d_keep_bits,
                       long long id_base, float* d_dist, long long* d_ids) {
    return flat_search(true, ctx, flat, d_queries, nq, ld_q, k, d_keep_bits, id_base, d_dist, d_ids);
}

int pqh_flat_last_counts(pqh_ctx_t* ctx, unsigned long long* chains, unsigned long long* fallback) {
    if (!ctx) return pqh_no_ctx_status();
    if (!chains || !fallback) return PQH_ERR_ARG;
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    unsigned long long v[2] = {0, 0};
    PQH_HIP(ctx, hipMemcpyAsync(v, ctx->d_diag + kDiagChains, sizeof(v), hipMemcpyDeviceToHost,
                                ctx->stream));
    PQH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *chains = v[0];
    *fallback = v[1];
    return PQH_OK;
}

}  // extern "C"
