// pqh_radius.hip -- range search: every scanned row with dist(q, v) < radius[q], straight from
// the compressed stream, as many results as there are.
//
//  radius_scan     adc_scan's staging and scoring (pqh_search.hip: one lane per chunk, 64 chunks
//                  per wave and step, the rows staged in the wave's LDS and scored 64 at a time
//                  against QB tables held in LDS with the query innermost) with a compare where
//                  the list offer was.  The output's size depends on the data, so the scan runs
//                  twice over a plan in the caller's memory:
//                  FILL = 0  counts: per query a wave-uniform running count (the popcount of the
//                            hit ballot), stored once per (query, group, wave);
//                  FILL = 1  writes: the wave starts at its offset of the plan and a hit lane
//                            stores (dist, id) at offset + popcount(ballot & lanes below).
//                  One template for both, so no comparison can differ between them.  Every wave
//                  takes a contiguous share of its workgroup's span of steps (the form the
//                  per-range-table scan already has), so ascending (group, wave) is ascending
//                  scan order and the result does not depend on the grid.
//                  The forms are adc_scan's but the list-major one: the whole stream with a
//                  batch of QB tables, RG (per-query CSR ranges, one query per workgroup), RT
//                  (one table per range, kept per wave), each with FL (the row mask).
//  radius_plan     adc_plan's step prefix of the ranges (a copy: pqh_search.hip stays as it is).
//  radius_offsets  the plan's counts into exclusive int64 prefixes, and lims.
//
// What the fill pass skips: a workgroup whose span counted nothing (before its tables), a wave
// whose share counted nothing, the rest of a share once all it counted is written, and -- by a
// 64-bit word per share that the count pass leaves in the plan -- every step of a sub-share
// without a hit.  -DPQH_RADIUS_NO_SKIP compiles the rule out (tools/bench_range_search.py).
//
// dist is the scan's: ((lut[0][c_0] + lut[1][c_1]) + ...) in fp32, no contraction.  The step
// staging block is adc_scan's, duplicated here (DESIGN.md section 4.5.11 lists the follow-up).
#include <algorithm>
#include <cmath>
#include <type_traits>

#include "pqh_internal.h"
#include "pqh_decode_dev.h"

namespace {

constexpr int kScanWavesMax = 16;          // waves per workgroup (threadIdx.y; threadIdx.x = lane)
constexpr int kLdsBytes = 160 * 1024;
constexpr int kCodesRowsPerLane = 4;       // SRC = 1: a wave stages 64 * 4 rows per step
constexpr int kRangeWaves = 4;             // the probe forms: waves per workgroup, and how many
constexpr int kRangeFill = 4;              // times over their workgroups fill the compute units
constexpr int kRangeTableWaves = 2;        // the same with a table per range (and per wave)
constexpr int kPlanWaves = 16;
constexpr int kHeaderWords = 8;            // the plan's header, in long longs
constexpr long long kPlanMagic = 0x5051485241444953ll;   // "PQHRADIS"

__device__ __forceinline__ void wave_lds_sync() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// The plan, in the caller's memory: the header the count pass writes (the geometry it ran
// with), then nq * shares + 1 entries, shares = groups * waves, entry q * shares + g * waves + w
// the count of query q in the share of wave w of group g; radius_offsets turns them into
// exclusive prefixes over all of them, so an entry is where its share begins to write, the next
// one where it ends, and entry q * shares is lims[q].  Behind the entries one word per
// (batch, group, wave): the share cut into up to 64 sub-shares of ceil(steps / 64) steps, bit j
// set when sub-share j held a hit of any query of the batch.  The fill pass passes over the
// steps of a sub-share whose bit is clear before anything is staged.
struct PlanHeader {
    long long magic, nq, groups, waves, batches, L, n, nr;
};
static_assert(sizeof(PlanHeader) == kHeaderWords * 8, "the header is eight words");

struct RadiusArgs {
    const uint32_t* words;      // SRC = 0: the stream
    long long nwords;
    const unsigned long long* chunk_off;
    const void* chunk_prev;
    DecTabs T;
    int raw_first;
    const unsigned char* codes; // SRC = 1: rows [n][m]
    long long n;
    int m, k;
    int C;                      // rows per lane and step (SRC = 0: the chunk size)
    int L;                      // lanes (chunks) per wave and step
    long long steps;            // ceil(chunks / L)
    int stage_bytes, win_words; // per wave
    const float* lut;           // [nq][m][k]; RT: [nr][m][k]
    const float* radius;        // [nq]
    long long nq;
    const long long* range_ptr; // RG: [nq + 1]
    const long long* ranges;    // [nr][2]: first row, count
    long long nr;
    const long long* steps_of;  // [nr + 1]: radius_plan's prefix
    const uint32_t* keep;       // FL
    long long* plan;            // header, then the entries
    PlanHeader geo;             // what this launch runs with
    long long capacity, id_base;   // FILL
    float* dist;
    long long* ids;
    unsigned long long* err;
};

// FL: the rows a lane has to decode of its chunk, of which [r_lo, r_hi) are inside the step's
// rows: up to the last kept one of them, 0 without one (adc_scan's rule, bit for bit).
__device__ __forceinline__ int kept_rows(const uint32_t* __restrict__ keep, long long chunk_row0,
                                         long long r_lo, long long r_hi) {
    if (r_hi <= r_lo) return 0;
    const long long w_lo = r_lo >> 5, w_hi = (r_hi - 1) >> 5;
    for (long long w = w_hi; w >= w_lo; --w) {
        uint32_t v = keep[w];
        if (w == w_hi) v &= 0xFFFFFFFFu >> (31 - (int)((r_hi - 1) & 31));
        if (w == w_lo) v &= 0xFFFFFFFFu << (int)(r_lo & 31);
        if (v) return (int)(w * 32 + (31 - __clz((int)v)) - chunk_row0) + 1;
    }
    return 0;
}

__device__ __forceinline__ bool range_ok(long long first, long long count, long long n) {
    return first >= 0 && count >= 0 && first <= n && count <= n - first;
}

// adc_plan: steps_of[r] = the steps of the ranges before r, steps_of[nr] = all of them; a range
// of count > 0 rows takes ceil(its chunks / L) steps, an empty or a bad one none, and a bad one
// sets error bit 2.
__global__ void __launch_bounds__(64 * kPlanWaves)
radius_plan(const long long* __restrict__ ranges, long long nr, long long n, int C, int L,
            long long* __restrict__ plan, unsigned long long* __restrict__ err) {
    __shared__ long long wsum[kPlanWaves];
    const int lane = threadIdx.x;
    const int wave = threadIdx.y;
    long long carry = 0;
    bool bad = false;
    for (long long base = 0; base < nr; base += 64 * kPlanWaves) {
        const long long r = base + wave * 64 + lane;
        long long s = 0;
        if (r < nr) {
            const long long first = ranges[2 * r], count = ranges[2 * r + 1];
            if (!range_ok(first, count, n))
                bad = true;
            else if (count > 0)
                s = ((first + count - 1) / C - first / C + L) / L;   // ceil(chunks / L)
        }
        long long inc = s;   // the wave's inclusive prefix
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long long t = __shfl_up(inc, d);
            inc += lane >= d ? t : 0;
        }
        if (lane == 63) wsum[wave] = inc;
        lds_barrier();
        long long before = 0, all = 0;
        for (int w = 0; w < kPlanWaves; ++w) {
            before += w < wave ? wsum[w] : 0;
            all += wsum[w];
        }
        if (r < nr) plan[r] = carry + before + inc - s;
        carry += all;
        lds_barrier();   // (wsum is written again in the next round)
    }
    if (wave == 0 && lane == 0) plan[nr] = carry;
    if (bad) atomicOr(err, 2ull);
}

// The counts of the plan into exclusive prefixes, in place, entry `total` the sum of all; and
// lims[q] = entry q * shares.  One workgroup, 1,024 entries a round: the int64 prefix of
// radius_plan.  (The lims of a round's entries are written in that round: entry q * shares is
// final once its round is.)
__global__ void __launch_bounds__(64 * kPlanWaves)
radius_offsets(long long* __restrict__ ent, long long total, long long shares, long long nq,
               long long* __restrict__ lims) {
    __shared__ long long wsum[kPlanWaves];
    const int lane = threadIdx.x;
    const int wave = threadIdx.y;
    long long carry = 0;
    for (long long base = 0; base < total; base += 64 * kPlanWaves) {
        const long long i = base + wave * 64 + lane;
        const long long s = i < total ? ent[i] : 0;
        long long inc = s;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long long t = __shfl_up(inc, d);
            inc += lane >= d ? t : 0;
        }
        if (lane == 63) wsum[wave] = inc;
        lds_barrier();
        long long before = 0, all = 0;
        for (int w = 0; w < kPlanWaves; ++w) {
            before += w < wave ? wsum[w] : 0;
            all += wsum[w];
        }
        if (i < total) {
            const long long ex = carry + before + inc - s;
            ent[i] = ex;
            if (i % shares == 0) lims[i / shares] = ex;
        }
        carry += all;
        lds_barrier();
    }
    if (wave == 0 && lane == 0) {
        ent[total] = carry;
        lims[nq] = carry;
    }
}

// nothing to scan (n == 0 or nr == 0): lims all zero
__global__ void __launch_bounds__(256) radius_no_rows(long long nq, long long* __restrict__ lims) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i <= nq) lims[i] = 0;
}

__device__ __forceinline__ bool same_geometry(const long long* __restrict__ plan, const PlanHeader& g) {
    const PlanHeader* h = reinterpret_cast<const PlanHeader*>(plan);
    return h->magic == g.magic && h->nq == g.nq && h->groups == g.groups && h->waves == g.waves &&
           h->batches == g.batches && h->L == g.L && h->n == g.n && h->nr == g.nr;
}

template <int SRC, int NW, bool CTX, int QB, bool RG, bool RT, bool FL, bool FILL>
__global__ void __launch_bounds__(64 * kScanWavesMax) radius_scan(const RadiusArgs a) {
    static_assert(RG == (QB == 1), "one query per workgroup is the probe search's form");
    static_assert(!RT || RG, "a table per range is a form of the probe search");
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int lane = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.y);
    const int waves = (int)blockDim.y;
    const int m = NW ? 8 * NW : a.m;
    const int k = a.k;
    const int C = a.C;
    const int mk = m * k;
    const long long q0 = (long long)blockIdx.x * QB;
    const long long shares = (long long)gridDim.y * waves;
    long long* ent = a.plan + kHeaderWords;
    unsigned long long* hit_words =
        reinterpret_cast<unsigned long long*>(ent + a.nq * shares + 1) + (long long)blockIdx.x * shares;

    if constexpr (FILL) {
        // a plan counted with another geometry (the tuning changed in between, say): nothing
        // is written, and the call is reported as PQH_ERR_ARG by pqh_decode_status
        if (!same_geometry(a.plan, a.geo)) {
            if (blockIdx.x == 0 && blockIdx.y == 0 && wave == 0 && lane == 0) atomicOr(a.err, 2ull);
            return;
        }
#ifndef PQH_RADIUS_NO_SKIP
        // a workgroup none of whose queries counted a hit in its span leaves before its tables
        // are loaded: its waves' entries are neighbours, so one difference per query says so
        bool any = false;
#pragma unroll
        for (int qq = 0; qq < QB; ++qq) {
            if (q0 + qq < a.nq) {
                const long long e = (q0 + qq) * shares + (long long)blockIdx.y * waves;
                any = any || ent[e + waves] != ent[e];
            }
        }
        if (!any) return;
#endif
    } else {
        if (blockIdx.x == 0 && blockIdx.y == 0 && wave == 0 && lane == 0)
            *reinterpret_cast<PlanHeader*>(a.plan) = a.geo;
    }

    // [m][k][QB]; RT: the wave's own [m][k], the waves' tables side by side before the stages
    const int table_bytes = (mk * 4 + 15) & ~15;
    float* lut_lds = reinterpret_cast<float*>(lds + (RT ? (size_t)wave * table_bytes : 0));
    const int per_wave = a.stage_bytes + (a.win_words ? (a.win_words + 4) * 4 : 0);
    unsigned char* stage = reinterpret_cast<unsigned char*>(lds) +
                           (RT ? (size_t)waves * table_bytes : (size_t)mk * QB * 4) +
                           (size_t)wave * per_wave;
    uint32_t* win = reinterpret_cast<uint32_t*>(stage + a.stage_bytes);

    for (int e = wave * 64 + lane; !RT && e < mk; e += waves * 64) {
        float v[QB];
#pragma unroll
        for (int qq = 0; qq < QB; ++qq) v[qq] = q0 + qq < a.nq ? a.lut[(q0 + qq) * mk + e] : 0.f;
#pragma unroll
        for (int u = 0; u < QB / 4; ++u)
            reinterpret_cast<float4*>(lut_lds + (size_t)e * QB)[u] =
                make_float4(v[4 * u], v[4 * u + 1], v[4 * u + 2], v[4 * u + 3]);
        if constexpr (QB == 1) lut_lds[e] = v[0];
    }
    lds_barrier();   // (the only barrier of the workgroup: from here on every wave is on its own)

    // a query past nq has a NaN radius: no row is below it
    float rad[QB];
#pragma unroll
    for (int qq = 0; qq < QB; ++qq) rad[qq] = q0 + qq < a.nq ? a.radius[q0 + qq] : NAN;

    // RG: the query's ranges [r_lo, r_hi) and its steps [t0, t0 + steps) of the step prefix;
    // range_ptr entries that are reversed or leave [0, nr] leave the query without steps
    long long steps = a.steps;
    long long r_lo = 0, r_hi = 0, t0 = 0;
    if constexpr (RG) {
        const long long p0 = a.range_ptr[q0], p1 = a.range_ptr[q0 + 1];
        steps = 0;
        if (p0 >= 0 && p0 <= p1 && p1 <= a.nr) {
            r_lo = p0;
            r_hi = p1;
            t0 = a.steps_of[p0];
            steps = a.steps_of[p1] - t0;
        } else if (blockIdx.y == 0 && wave == 0 && lane == 0) {
            atomicOr(a.err, 2ull);
        }
    }

    // the wave's share: a contiguous piece of the workgroup's span of steps
    const long long g_lo = (long long)blockIdx.y * steps / gridDim.y;
    const long long g_hi = ((long long)blockIdx.y + 1) * steps / gridDim.y;
    const long long g_first = g_lo + (long long)wave * (g_hi - g_lo) / waves;
    const long long g_end = g_lo + ((long long)wave + 1) * (g_hi - g_lo) / waves;
    const long long share = (long long)blockIdx.y * waves + wave;

    // FILL = 0: cnt counts the hits; FILL = 1: cnt is where the next hit goes, and stop where
    // the share's hits end.  Both are the same for every lane.
    long long cnt[QB], stop[QB];
    bool todo = !FILL;
#pragma unroll
    for (int qq = 0; qq < QB; ++qq) {
        cnt[qq] = stop[qq] = 0;
        if constexpr (FILL) {
            if (q0 + qq < a.nq) {
                cnt[qq] = ent[(q0 + qq) * shares + share];
                stop[qq] = ent[(q0 + qq) * shares + share + 1];
                todo = todo || cnt[qq] != stop[qq];
            }
        }
    }
    // the share's sub-shares with a hit (FILL = 0: found here; FILL = 1: the count's)
    const long long sub = max(1ll, (g_end - g_first + 63) / 64);
    unsigned long long hit_mask = FILL ? hit_words[share] : 0ull;
#ifdef PQH_RADIUS_NO_SKIP
    todo = true;
    if constexpr (FILL) hit_mask = ~0ull;
#endif

    const long long chunks = (a.n + C - 1) / C;
    const unsigned long long nbits = (unsigned long long)a.nwords * 32;
    long long r_loaded = -1;   // RT: the range whose table the wave holds
    long long r_cur = r_lo;    // RG: the range of the wave's last step (its steps ascend)
#pragma unroll 1
    for (long long g = g_first; g < g_end && todo; ++g) {
        long long j0 = g * a.L;
        long long jn = min(chunks - j0, (long long)a.L);
        long long lo = 0, hi = 0;   // RG: the step's rows inside its range are [lo, hi)
        int fl_cnt = 0;
        if constexpr (FILL)   // (a sub-share without a hit: nothing to write, no count moves)
            if (!((hit_mask >> ((g - g_first) / sub)) & 1ull)) continue;
        bool step_hit = false;
        if constexpr (RG) {
            const long long t = t0 + g;
            long long e = r_hi;
            while (e - r_cur > 1) {
                const long long mid = r_cur + (e - r_cur) / 2;
                if (a.steps_of[mid] <= t)
                    r_cur = mid;
                else
                    e = mid;
            }
            const long long first = a.ranges[2 * r_cur], count = a.ranges[2 * r_cur + 1];
            j0 = first / C + (t - a.steps_of[r_cur]) * a.L;
            jn = min((first + count - 1) / C + 1 - j0, (long long)a.L);
            lo = max(first, j0 * C);
            hi = min(first + count, (j0 + jn) * C);
            if constexpr (FL) {
                if (lane < jn) fl_cnt = kept_rows(a.keep, (j0 + lane) * C, max(lo, (j0 + lane) * C),
                                                  min(hi, (j0 + lane + 1) * C));
                if (!__ballot(fl_cnt > 0)) continue;   // (before the table: a step without a kept row)
            }
            if constexpr (RT) {
                if (r_cur != r_loaded) {
                    const float* src = a.lut + r_cur * mk;
                    if (!(mk & 3) && !(reinterpret_cast<uintptr_t>(a.lut) & 15u)) {
                        for (int e = lane; e < mk / 4; e += 64)
                            reinterpret_cast<float4*>(lut_lds)[e] =
                                reinterpret_cast<const float4*>(src)[e];
                    } else {
                        for (int e = lane; e < mk; e += 64) lut_lds[e] = src[e];
                    }
                    r_loaded = r_cur;
                }
            }
        }
        const long long row0 = j0 * C;
        const int nrows = (int)(min(a.n, (j0 + (RG ? jn : (long long)a.L)) * C) - row0);
        if constexpr (FL && !RG) {
            if (lane < jn) fl_cnt = kept_rows(a.keep, (j0 + lane) * C, max(row0, (j0 + lane) * C),
                                              min(row0 + nrows, (j0 + lane + 1) * C));
            if (!__ballot(fl_cnt > 0)) continue;
        }
        const int span = RG ? (int)jn : 64;   // the chunks the stream window is staged for
        unsigned long long dead = 0;   // lanes whose chunk failed
        if constexpr (SRC == 0) {
            bool use_win = false;
            StreamWin sw{0, 0, false};
            if (a.win_words > 0) {   // (then L = 64: the window is that of 64 chunks)
                const unsigned long long b_lo = a.chunk_off[j0];
                const unsigned long long b_hi = j0 + span < chunks ? a.chunk_off[j0 + span] : nbits;
                if (b_lo <= nbits && b_hi >= b_lo) {
                    sw = stage_window<4, true>(a.words, a.nwords, a.chunk_off, j0, chunks, win,
                                               a.win_words, span);
                    use_win = sw.in_lds;
                }
            }
            wave_lds_sync();
            bool ok = true;
            if (lane < jn && (!FL || fl_cnt > 0)) {
                const long long j = j0 + lane;
                const unsigned long long off = a.chunk_off[j];
                const int cnt_rows = FL ? fl_cnt : (int)min((long long)C, (RG ? hi : a.n) - j * C);
                const bool raw = CTX && j == 0 && a.raw_first;
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
                                prev[w] = static_cast<const unsigned long long*>(a.chunk_prev)[j * NW + w];
                        }
                        return walk_packed<CTX, NW, 8>(br, a.T, raw, cnt_rows, prev,
                                                       [&](int s, int w, unsigned long long row) {
                                                           st[s * NW + w] = row;
                                                       });
                    } else {
                        unsigned char* st = stage + (long long)lane * C * m;
                        for (int i = 0; i < m; ++i)
                            st[i] = (CTX && !raw)
                                        ? static_cast<const unsigned char*>(a.chunk_prev)[j * m + i]
                                        : (unsigned char)0;
                        int cur = 0;
                        return walk_parts<0>(
                            br, a.T, m, CTX, raw, cnt_rows,
                            [&](int i) -> unsigned char& { return st[cur * m + i]; },
                            [&](int s) {
                                if (s + 1 < cnt_rows)
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
                    ok = rd.init(a.words, a.nwords, off);
                    if (ok) ok = walk(rd.br) && rd.pos() <= nbits;
                }
            }
            dead = __ballot(lane < jn && !ok);
            if (dead && lane == 0) atomicOr(a.err, 1ull);
        } else {
            const long long nbytes = (long long)nrows * m;
            const unsigned char* src = a.codes + row0 * m;
            long long done = 0;
            if (!(reinterpret_cast<uintptr_t>(src) & 3u)) {
                done = nbytes & ~3ll;
                for (long long q = lane; q < done / 4; q += 64)
                    reinterpret_cast<uint32_t*>(stage)[q] =
                        __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(src) + q);
            }
            for (long long q = done + lane; q < nbytes; q += 64) stage[q] = src[q];
        }
        wave_lds_sync();

        // the stage holds the wave's rows row0 ... row0 + nrows - 1 in order: lane scores
        // rows lane, lane + 64, ..., so a ballot's bits are in row order
#pragma unroll 1
        for (int base = 0; base < nrows; base += 64) {
            const int r = base + lane;
            bool valid = r < nrows;
            if (dead && valid) valid = !((dead >> (r / C)) & 1ull);
            if constexpr (RG) valid = valid && row0 + r >= lo && row0 + r < hi;
            if constexpr (FL)
                if (r < nrows) valid = valid && ((a.keep[(row0 + r) >> 5] >> ((row0 + r) & 31)) & 1u);
            if constexpr (FL)
                if (!__ballot(valid)) continue;
            const unsigned char* row = stage + (long long)(r < nrows ? r : 0) * m;
            float sum[QB];
            auto add = [&](int i, unsigned c) {
                // (a failed chunk's slots hold anything: keep the read inside the table)
                if constexpr (QB == 1) {
                    const float v = lut_lds[i * k + (int)min(c, (unsigned)(k - 1))];
                    if (i == 0)
                        sum[0] = v;
                    else
                        sum[0] = sum[0] + v;
                }
                const float4* e = reinterpret_cast<const float4*>(
                    lut_lds + (size_t)(i * k + (int)min(c, (unsigned)(k - 1))) * QB);
#pragma unroll
                for (int u = 0; u < QB / 4; ++u) {
                    const float4 v = e[u];
                    if (i == 0) {
                        sum[4 * u] = v.x, sum[4 * u + 1] = v.y, sum[4 * u + 2] = v.z, sum[4 * u + 3] = v.w;
                    } else {
                        sum[4 * u] = sum[4 * u] + v.x;
                        sum[4 * u + 1] = sum[4 * u + 1] + v.y;
                        sum[4 * u + 2] = sum[4 * u + 2] + v.z;
                        sum[4 * u + 3] = sum[4 * u + 3] + v.w;
                    }
                }
            };
            if constexpr (NW > 0) {
#pragma unroll
                for (int w = 0; w < NW; ++w) {
                    const unsigned long long word = reinterpret_cast<const unsigned long long*>(row)[w];
#pragma unroll
                    for (int i = 0; i < 8; ++i) add(w * 8 + i, (unsigned)(word >> (8 * i)) & 255u);
                }
            } else {
                add(0, row[0]);
#pragma unroll 1
                for (int i = 1; i < m; ++i) add(i, row[i]);
            }
            const long long id = row0 + r;
#pragma unroll
            for (int qq = 0; qq < QB; ++qq) {
                // (NaN on either side: no hit)
                const unsigned long long hits = __ballot(valid && sum[qq] < rad[qq]);
                if constexpr (FILL) {
                    if ((hits >> lane) & 1ull) {
                        const long long p = cnt[qq] + __popcll(hits & ((1ull << lane) - 1ull));
                        if (p < a.capacity) {
                            a.dist[p] = sum[qq];
                            a.ids[p] = id + a.id_base;
                        }
                    }
                }
                cnt[qq] += __popcll(hits);
                step_hit = step_hit || hits != 0;
            }
        }
        if constexpr (!FILL)
            if (step_hit) hit_mask |= 1ull << ((g - g_first) / sub);
        if constexpr (FILL) {
#ifndef PQH_RADIUS_NO_SKIP
            // everything the share counted is written: the rest of it holds no hit
            todo = false;
#pragma unroll
            for (int qq = 0; qq < QB; ++qq) todo = todo || cnt[qq] != stop[qq];
#endif
        }
        wave_lds_sync();   // the next step's staging overwrites what was just read
    }

    if constexpr (!FILL) {
        if (lane == 0) {
#pragma unroll
            for (int qq = 0; qq < QB; ++qq)
                if (q0 + qq < a.nq) ent[(q0 + qq) * shares + share] = cnt[qq];
            hit_words[share] = hit_mask;
        }
    }
}

// ------------------------------------------------------------------- host side
template <int N>
using Int = std::integral_constant<int, N>;

int floor_pow2(long long v) {
    int p = 1;
    while (2ll * p <= v) p *= 2;
    return p;
}

// The launch of both passes, from the shapes alone (pqh_search.hip's scan_launch, with a
// contiguous share per wave in every form and no lists to exchange at the end).
struct Geometry {
    int qb, L, stage_bytes, win_words, waves;
    long long steps, batches, groups;
    size_t lds;
};

int geometry(const pqh_ctx_t* ctx, int src, int nw, long long n, int m, int k, int C, long long nq,
             bool rg, bool rt, Geometry* g) {
    g->qb = rg ? 1 : (m <= 8 && (long long)m * k <= 2048) ? 8 : 4;
    const long long lut_bytes = (long long)m * k * g->qb * 4;
    const long long budget = kLdsBytes - lut_bytes;
    const long long chunks = (n + C - 1) / C;
    const long long row_bytes = (long long)C * m;
    g->L = 64;
    if (((64 * row_bytes + 15) & ~15ll) > budget) g->L = (int)((budget - 16) / row_bytes);
    if (g->L < 1) return PQH_ERR_UNSUPPORTED;
    g->stage_bytes = (int)((g->L * row_bytes + 15) & ~15ll);
    g->win_words = 0;
    if (src == 0 && g->L == 64) {
        const long long span_words = (64ll * C * m * 12 + 31) / 32 + 8;
        const long long ww = std::min<long long>(4096 - 1024 * (nw == 2 ? 1 : 0),
                                                 std::max<long long>(256, span_words));
        g->win_words = (int)((ww + 3) & ~3ll);
        if (g->stage_bytes + (g->win_words + 4) * 4 > budget) g->win_words = 0;
    }
    const long long per_wave = g->stage_bytes + (g->win_words ? (g->win_words + 4) * 4 : 0);
    const long long wave_table = rt ? ((m * k * 4 + 15) & ~15) : 0;
    if (per_wave + wave_table > kLdsBytes) return PQH_ERR_UNSUPPORTED;
    int fit = floor_pow2(std::min<long long>(
        kScanWavesMax, rt ? kLdsBytes / (per_wave + wave_table) : budget / per_wave));
    g->steps = (chunks + g->L - 1) / g->L;
    g->batches = (nq + g->qb - 1) / g->qb;
    long long groups = ctx->tune_search_groups > 0
                           ? ctx->tune_search_groups
                           : std::max<long long>(1, ctx->num_cus / g->batches);
    if (rg) {
        fit = std::min(fit, rt ? kRangeTableWaves : kRangeWaves);
        long long wgs = (kRangeFill * (long long)ctx->num_cus + nq - 1) / nq;
        if (rt) wgs = kLdsBytes / (fit * (per_wave + wave_table)) * (long long)ctx->num_cus / nq;
        if (ctx->tune_search_groups <= 0)
            groups = std::min<long long>(wgs, (g->steps + fit - 1) / fit);
        groups = std::min<long long>(std::max<long long>(groups, 1), 65535);
    } else {
        groups = std::min<long long>(std::min<long long>(groups, g->steps), 65535);
    }
    g->groups = groups;
    g->waves = rg ? fit : std::min(fit, floor_pow2((g->steps + 2 * groups - 1) / (2 * groups)));
    g->lds = rt ? (size_t)g->waves * (size_t)(wave_table + per_wave)
                : (size_t)lut_bytes + (size_t)g->waves * (size_t)per_wave;
    return PQH_OK;
}

unsigned long long plan_bytes_of(const Geometry& g, long long nq) {
    // the header, an entry per (query, group, wave) and the total, a word per (batch, group, wave)
    const unsigned long long shares = (unsigned long long)g.groups * g.waves;
    return ((unsigned long long)kHeaderWords + (unsigned long long)nq * shares + 1 +
            (unsigned long long)g.batches * shares) * 8;
}

// what the calls share: the source, the probe list and both passes' buffers
struct Call {
    const float* lut;
    long long nq;
    const long long* range_ptr;
    const long long* ranges;
    long long nr;
    int tables_per_range;
    const float* radius;
    const unsigned int* keep;
    void* plan;
    unsigned long long plan_bytes;
    long long* lims;
    bool fill;
    long long capacity, id_base;
    float* dist;
    long long* ids;
};

// the argument checks of both sources; *run = false: nothing (more) to launch
int call_check(pqh_ctx_t* ctx, bool have_src, long long n, const Call& c, bool* run) {
    *run = false;
    if (n < 0 || c.nq < 0 || c.nr < -1) return PQH_ERR_ARG;
    // the whole stream: no probe list at all; else range_ptr, and ranges where there are any
    if (c.nr == -1 ? (c.range_ptr || c.ranges || c.tables_per_range)
                   : (c.nq > 0 && (!c.range_ptr || (c.nr > 0 && !c.ranges))))
        return PQH_ERR_ARG;
    if (!c.lims) return PQH_ERR_ARG;
    if (c.nq > 0 && (!c.lut || !c.radius || !c.plan || (n > 0 && !have_src))) return PQH_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(c.plan) | reinterpret_cast<uintptr_t>(c.lims)) & 7u)
        return PQH_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(c.keep) & 3u) return PQH_ERR_ARG;
    if (c.fill && (c.capacity < 0 || (c.capacity > 0 && (!c.dist || !c.ids)))) return PQH_ERR_ARG;
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    if (c.nq > 0x7FFFFFFFll) return PQH_ERR_UNSUPPORTED;
    if (c.nq == 0 || n == 0 || c.nr == 0) {
        // (the fill has nothing to write: lims is the count's)
        if (!c.fill) {
            hipLaunchKernelGGL(radius_no_rows, dim3((unsigned)(c.nq / 256 + 1)), dim3(256), 0,
                               ctx->stream, c.nq, c.lims);
            PQH_LAUNCH_CHECK(ctx);
        }
        return PQH_OK;
    }
    *run = true;
    return PQH_OK;
}

int scan_launch(pqh_ctx_t* ctx, int src, int nw, bool cx, RadiusArgs a, const Call& c) {
    const bool rg = c.nr >= 0, rt = rg && c.tables_per_range;
    Geometry g;
    int rc = geometry(ctx, src, nw, a.n, a.m, a.k, a.C, c.nq, rg, rt, &g);
    if (rc) return rc;
    if (c.plan_bytes < plan_bytes_of(g, c.nq)) return PQH_ERR_ARG;
    a.L = g.L;
    a.stage_bytes = g.stage_bytes;
    a.win_words = g.win_words;
    a.steps = g.steps;
    a.lut = c.lut;
    a.radius = c.radius;
    a.nq = c.nq;
    a.keep = c.keep;
    a.plan = static_cast<long long*>(c.plan);
    a.geo = PlanHeader{kPlanMagic, c.nq, g.groups, g.waves, g.batches, g.L, a.n, c.nr};
    a.capacity = c.capacity;
    a.id_base = c.id_base;
    a.dist = c.dist;
    a.ids = c.ids;
    a.err = ctx->d_diag + 1;
    if (rg) {
        // the ranges' step prefix, made again by either pass: nothing of the context has to
        // survive from the count to the fill
        rc = pqh_ensure_ws(ctx, ((size_t)c.nr + 1) * 8);
        if (rc) return rc;
        long long* steps_of = static_cast<long long*>(ctx->ws);
        hipLaunchKernelGGL(radius_plan, dim3(1), dim3(64, kPlanWaves), 0, ctx->stream, c.ranges,
                           c.nr, a.n, a.C, a.L, steps_of, a.err);
        PQH_LAUNCH_CHECK(ctx);
        a.range_ptr = c.range_ptr;
        a.ranges = c.ranges;
        a.nr = c.nr;
        a.steps_of = steps_of;
    }
    auto launch_pass = [&](auto s, auto w, auto cxt, auto q, auto tb, auto fl, auto fi) -> int {
        auto* fn = radius_scan<decltype(s)::value, decltype(w)::value, decltype(cxt)::value,
                               decltype(q)::value, decltype(q)::value == 1, decltype(tb)::value,
                               decltype(fl)::value, decltype(fi)::value>;
        if (g.lds > 64 * 1024)
            PQH_HIP(ctx, hipFuncSetAttribute((const void*)fn,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds));
        hipLaunchKernelGGL(fn, dim3((unsigned)g.batches, (unsigned)g.groups), dim3(64, g.waves),
                           g.lds, ctx->stream, a);
        return PQH_OK;
    };
    auto launch_fl = [&](auto s, auto w, auto cxt, auto q, auto tb, auto fl) -> int {
        return c.fill ? launch_pass(s, w, cxt, q, tb, fl, std::true_type())
                      : launch_pass(s, w, cxt, q, tb, fl, std::false_type());
    };
    auto launch = [&](auto s, auto w, auto cxt, auto q, auto tb) -> int {
        return a.keep ? launch_fl(s, w, cxt, q, tb, std::true_type())
                      : launch_fl(s, w, cxt, q, tb, std::false_type());
    };
    auto with_qb = [&](auto s, auto w, auto cxt) -> int {
        const std::false_type no;
        if (rt) return launch(s, w, cxt, Int<1>(), std::true_type());
        if (rg) return launch(s, w, cxt, Int<1>(), no);
        if constexpr (decltype(w)::value != 2)
            if (g.qb == 8) return launch(s, w, cxt, Int<8>(), no);
        return launch(s, w, cxt, Int<4>(), no);
    };
    auto with_nw = [&](auto s, auto cxt) -> int {
        return nw == 1 ? with_qb(s, Int<1>(), cxt) : nw == 2 ? with_qb(s, Int<2>(), cxt)
                                                             : with_qb(s, Int<0>(), cxt);
    };
    if (src == 1)
        rc = with_nw(Int<1>(), std::false_type());
    else
        rc = cx ? with_nw(Int<0>(), std::true_type()) : with_nw(Int<0>(), std::false_type());
    if (rc) return rc;
    PQH_LAUNCH_CHECK(ctx);
    if (!c.fill) {
        const long long shares = g.groups * g.waves;
        hipLaunchKernelGGL(radius_offsets, dim3(1), dim3(64, kPlanWaves), 0, ctx->stream,
                           a.plan + kHeaderWords, c.nq * shares, shares, c.nq, c.lims);
        PQH_LAUNCH_CHECK(ctx);
    }
    return PQH_OK;
}

int range_stream(pqh_ctx_t* ctx, const pqh_tables_t* t, const unsigned char* d_stream,
                 unsigned long long stream_bytes, long long n, int raw_first, int chunk_vectors,
                 const unsigned long long* d_chunk_offsets, const void* d_chunk_prev,
                 const Call& c) {
    if (!ctx) return pqh_no_ctx_status();
    if (!t || chunk_vectors < 1) return PQH_ERR_ARG;
    if (n > 0 && c.nq > 0 && (stream_bytes < 4 || !d_chunk_offsets)) return PQH_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(d_stream) & 3u) return PQH_ERR_ARG;
    if (t->context && !d_chunk_prev && (!raw_first || n > chunk_vectors)) return PQH_ERR_ARG;
    if (t->k > 256 || t->m > 16) return PQH_ERR_UNSUPPORTED;
    bool run = false;
    int rc = call_check(ctx, d_stream != nullptr, n, c, &run);
    if (rc || !run) return rc;
    if (stream_bytes / 4 >= (1ull << 58)) return PQH_ERR_UNSUPPORTED;
    RadiusArgs a{};
    a.words = reinterpret_cast<const uint32_t*>(d_stream);
    a.nwords = (long long)(stream_bytes / 4);
    a.chunk_off = d_chunk_offsets;
    a.chunk_prev = d_chunk_prev;
    a.T = dec_tabs(t, 0);
    a.raw_first = raw_first;
    a.n = n;
    a.m = t->m;
    a.k = t->k;
    a.C = chunk_vectors;
    const bool packed = (t->m == 8 || t->m == 16) && !(reinterpret_cast<uintptr_t>(d_chunk_prev) & 7);
    return scan_launch(ctx, 0, packed ? t->m / 8 : 0, t->context != 0, a, c);
}

int range_codes(pqh_ctx_t* ctx, const void* d_codes, long long n, int m, int k, const Call& c) {
    if (!ctx) return pqh_no_ctx_status();
    if (m < 1 || k < 1) return PQH_ERR_ARG;
    if (k > 256 || m > 16) return PQH_ERR_UNSUPPORTED;
    bool run = false;
    int rc = call_check(ctx, d_codes != nullptr, n, c, &run);
    if (rc || !run) return rc;
    RadiusArgs a{};
    a.codes = static_cast<const unsigned char*>(d_codes);
    a.n = n;
    a.m = m;
    a.k = k;
    a.C = kCodesRowsPerLane;
    return scan_launch(ctx, 1, (m == 8 || m == 16) ? m / 8 : 0, false, a, c);
}

}  // namespace

extern "C" {

int pqh_range_plan_bytes(pqh_ctx_t* ctx, long long n, int m, int k, int chunk_vectors,
                         long long nq, long long nr, int tables_per_range,
                         unsigned long long* bytes) {
    if (!ctx) return pqh_no_ctx_status();
    if (!bytes || n < 0 || m < 1 || k < 1 || chunk_vectors < 0 || nq < 0 || nr < -1 ||
        (nr == -1 && tables_per_range))
        return PQH_ERR_ARG;
    if (k > 256 || m > 16 || nq > 0x7FFFFFFFll) return PQH_ERR_UNSUPPORTED;
    *bytes = (kHeaderWords + 1) * 8;
    if (nq == 0 || n == 0 || nr == 0) return PQH_OK;
    const int src = chunk_vectors == 0 ? 1 : 0;
    // the stream window, and with it the waves that fit, depends on the walk, which the call
    // takes from the alignment of d_chunk_prev: the larger of the two
    for (int nw : {0, (m == 8 || m == 16) ? m / 8 : 0}) {
        Geometry g;
        int rc = geometry(ctx, src, nw, n, m, k, src ? kCodesRowsPerLane : chunk_vectors, nq,
                          nr >= 0, nr >= 0 && tables_per_range, &g);
        if (rc) return rc;
        *bytes = std::max(*bytes, plan_bytes_of(g, nq));
    }
    return PQH_OK;
}

int pqh_range_count_stream(pqh_ctx_t* ctx, const pqh_tables_t* t, const unsigned char* d_stream,
                           unsigned long long stream_bytes, long long n, int raw_first,
                           int chunk_vectors, const unsigned long long* d_chunk_offsets,
                           const void* d_chunk_prev, const float* d_lut, long long nq,
                           const long long* d_range_ptr, const long long* d_ranges, long long nr,
                           int tables_per_range, const float* d_radius, const unsigned int* d_keep,
                           void* d_plan, unsigned long long plan_bytes, long long* d_lims) {
    const Call c{d_lut, nq, d_range_ptr, d_ranges, nr, tables_per_range, d_radius, d_keep, d_plan,
                 plan_bytes, d_lims, false, 0, 0, nullptr, nullptr};
    return range_stream(ctx, t, d_stream, stream_bytes, n, raw_first, chunk_vectors,
                        d_chunk_offsets, d_chunk_prev, c);
}

int pqh_range_fill_stream(pqh_ctx_t* ctx, const pqh_tables_t* t, const unsigned char* d_stream,
                          unsigned long long stream_bytes, long long n, int raw_first,
                          int chunk_vectors, const unsigned long long* d_chunk_offsets,
                          const void* d_chunk_prev, const float* d_lut, long long nq,
                          const long long* d_range_ptr, const long long* d_ranges, long long nr,
                          int tables_per_range, const float* d_radius, const unsigned int* d_keep,
                          const void* d_plan, unsigned long long plan_bytes,
                          const long long* d_lims, long long capacity, long long id_base,
                          float* d_dist, long long* d_ids) {
    const Call c{d_lut, nq, d_range_ptr, d_ranges, nr, tables_per_range, d_radius, d_keep,
                 const_cast<void*>(d_plan), plan_bytes, const_cast<long long*>(d_lims), true,
                 capacity, id_base, d_dist, d_ids};
    return range_stream(ctx, t, d_stream, stream_bytes, n, raw_first, chunk_vectors,
                        d_chunk_offsets, d_chunk_prev, c);
}

int pqh_range_count_codes(pqh_ctx_t* ctx, const void* d_codes, long long n, int m, int k,
                          const float* d_lut, long long nq, const long long* d_range_ptr,
                          const long long* d_ranges, long long nr, int tables_per_range,
                          const float* d_radius, const unsigned int* d_keep, void* d_plan,
                          unsigned long long plan_bytes, long long* d_lims) {
    const Call c{d_lut, nq, d_range_ptr, d_ranges, nr, tables_per_range, d_radius, d_keep, d_plan,
                 plan_bytes, d_lims, false, 0, 0, nullptr, nullptr};
    return range_codes(ctx, d_codes, n, m, k, c);
}

int pqh_range_fill_codes(pqh_ctx_t* ctx, const void* d_codes, long long n, int m, int k,
                         const float* d_lut, long long nq, const long long* d_range_ptr,
                         const long long* d_ranges, long long nr, int tables_per_range,
                         const float* d_radius, const unsigned int* d_keep, const void* d_plan,
                         unsigned long long plan_bytes, const long long* d_lims,
                         long long capacity, long long id_base, float* d_dist, long long* d_ids) {
    const Call c{d_lut, nq, d_range_ptr, d_ranges, nr, tables_per_range, d_radius, d_keep,
                 const_cast<void*>(d_plan), plan_bytes, const_cast<long long*>(d_lims), true,
                 capacity, id_base, d_dist, d_ids};
    return range_codes(ctx, d_codes, n, m, k, c);
}

}  // extern "C"
