// pqh_scan_dev.h -- what the ADC top-k scan (adc_scan, pqh_search.hip) and the range scan
// (radius_scan, pqh_radius.hip) have in common (not installed): one lane per chunk, 64 chunks
// per wave and step, the rows staged in the wave's LDS and scored 64 at a time against tables
// held in LDS with the query innermost.  One statement of each piece: the launch constants, the
// mask rule, the step prefix of the probe ranges (scan_plan), the table loads, the step's
// location in its range, the staging of a step (stage_step, over the readers and the walks of
// pqh_decode_dev.h) and the scoring of a staged row (score_row); on the host the launch geometry,
// the way from run-time flags to template arguments, and the set-up of the two sources.  What a
// kernel does with a row's sums -- offer them to a list, or compare them with a radius -- and
// the order its waves take the steps in is its own.  (One exception: radius_scan holds a copy of
// score_row's body, see there.)
#pragma once

#include <algorithm>
#include <type_traits>

#include "pqh_internal.h"
#include "pqh_decode_dev.h"

namespace {

constexpr int kScanWavesMax = 16;          // waves per workgroup (threadIdx.y; threadIdx.x = lane)
constexpr int kWideWavesMax = 8;           // the same with the wide list (top_k > 64)
constexpr int kLdsBytes = 160 * 1024;
constexpr int kCodesRowsPerLane = 4;       // SRC = 1: a wave stages 64 * 4 rows per step
constexpr int kRangeWaves = 4;             // the probe forms: waves per workgroup, and how many
constexpr int kRangeFill = 4;              // times over their workgroups fill the compute units
constexpr int kRangeTableWaves = 2;        // the same with a table per range (and per wave)
constexpr int kPlanWaves = 16;

// LDS written by some lanes of this wave and read by others: all of it done before any lane
// goes on (the stage and the window are the wave's own, so no workgroup barrier)
__device__ __forceinline__ void wave_lds_sync() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// FL: the rows a lane has to decode of its chunk, of which [r_lo, r_hi) are inside the step's
// rows: up to the last kept one of them, 0 without one.  Bits outside [r_lo, r_hi) are masked
// off, so nothing past row n of the last word counts (r_hi <= n) and no word beyond it is read.
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

// The chunks of a good range: [first / C, (first + count - 1) / C + 1); a range is good when
// 0 <= first <= n and 0 <= count <= n - first (no sum that could overflow).
__device__ __forceinline__ bool range_ok(long long first, long long count, long long n) {
    return first >= 0 && count >= 0 && first <= n && count <= n - first;
}

// the bytes of one wave's table in the RT form (the stages after the tables stay 16-byte aligned)
__host__ __device__ __forceinline__ int range_table_bytes(int mk) { return (mk * 4 + 15) & ~15; }

// The exclusive prefix of `s` over the 64 * kPlanWaves threads of a workgroup (dim3(64,
// kPlanWaves)) in the order wave * 64 + lane, and *all = their sum: the wave's sums by
// shuffles, the waves' through LDS.  Two barriers, the second because wsum is written again by
// the next call; every thread of the workgroup has to make the call.
__device__ __forceinline__ long long block_prefix(long long s, long long* all) {
    __shared__ long long wsum[kPlanWaves];
    const int lane = threadIdx.x;
    const int wave = threadIdx.y;
    long long inc = s;   // the wave's inclusive prefix
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long t = __shfl_up(inc, d);
        inc += lane >= d ? t : 0;
    }
    if (lane == 63) wsum[wave] = inc;
    lds_barrier();
    long long before = 0, sum = 0;
    for (int w = 0; w < kPlanWaves; ++w) {
        before += w < wave ? wsum[w] : 0;
        sum += wsum[w];
    }
    lds_barrier();
    *all = sum;
    return before + inc - s;
}

// plan[r] = the steps of the ranges before r, plan[nr] = all of them: a range of count > 0
// rows takes ceil(its chunks / L) steps, an empty or a bad one none (so no step ever leads to
// it), and a bad one sets error bit 2.  The prefix is over all ranges, not per query: the
// queries' spans of it may overlap or repeat, and query q's steps are
// [plan[range_ptr[q]], plan[range_ptr[q + 1]]) whatever the others are.  One workgroup:
// 1,024 ranges a round.
__global__ void __launch_bounds__(64 * kPlanWaves)
scan_plan(const long long* __restrict__ ranges, long long nr, long long n, int C, int L,
          long long* __restrict__ plan, unsigned long long* __restrict__ err) {
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
        long long all;
        const long long ex = block_prefix(s, &all);
        if (r < nr) plan[r] = carry + ex;
        carry += all;
    }
    if (wave == 0 && lane == 0) plan[nr] = carry;
    if (bad) atomicOr(err, 2ull);
}

// The tables of the batch's queries q0 ... q0 + QB - 1 into LDS as [m][k][QB], the query
// innermost: one 16-byte read is four queries' entries.  A query past nq zeros.  The whole
// workgroup loads; the caller's barrier follows.
template <int QB>
__device__ __forceinline__ void load_batch_tables(float* lut_lds, const float* lut,
                                                  long long q0, long long nq, int mk, int wave,
                                                  int lane, int waves) {
    for (int e = wave * 64 + lane; e < mk; e += waves * 64) {
        float v[QB];
#pragma unroll
        for (int qq = 0; qq < QB; ++qq) v[qq] = q0 + qq < nq ? lut[(q0 + qq) * mk + e] : 0.f;
#pragma unroll
        for (int u = 0; u < QB / 4; ++u)
            reinterpret_cast<float4*>(lut_lds + (size_t)e * QB)[u] =
                make_float4(v[4 * u], v[4 * u + 1], v[4 * u + 2], v[4 * u + 3]);
        if constexpr (QB == 1) lut_lds[e] = v[0];
    }
}

// RG: step t of the step prefix.  Its range r is the last one of [r_cur, r_hi) whose steps begin
// at or before it (ranges without steps share their successor's entry and are passed over);
// the caller goes on from r, a wave's steps ascend.  The step is the chunks [j0, j0 + jn) of
// that range, up to L of them, and its rows inside the range are [lo, hi).  (By value: with
// reference parameters two radius_scan instantiations lose a wave of occupancy.)
struct RangeStep {
    long long r, j0, jn, lo, hi;
};
__device__ __forceinline__ RangeStep range_step(long long r_cur, long long r_hi, long long t,
                                            const long long* steps_of, const long long* ranges,
                                            int C, int L) {
    long long e = r_hi;
    while (e - r_cur > 1) {
        const long long mid = r_cur + (e - r_cur) / 2;
        if (steps_of[mid] <= t)
            r_cur = mid;
        else
            e = mid;
    }
    const long long first = ranges[2 * r_cur], count = ranges[2 * r_cur + 1];
    RangeStep s;
    s.r = r_cur;
    s.j0 = first / C + (t - steps_of[r_cur]) * L;
    s.jn = min((first + count - 1) / C + 1 - s.j0, (long long)L);
    s.lo = max(first, s.j0 * C);
    s.hi = min(first + count, (s.j0 + s.jn) * C);
    return s;
}

// RT: the table of range r, lut[r][m][k], into the wave's own LDS.  (The reads of the table
// before are done: the wave_lds_sync that ends a step; the new one is complete at the
// wave_lds_sync before the scoring.)
__device__ __forceinline__ void load_range_table(float* lut_lds, const float* lut,
                                                 long long r, int mk, int lane) {
    const float* src = lut + r * mk;
    if (!(mk & 3) && !(reinterpret_cast<uintptr_t>(lut) & 15u)) {
        for (int e = lane; e < mk / 4; e += 64)
            reinterpret_cast<float4*>(lut_lds)[e] = reinterpret_cast<const float4*>(src)[e];
    } else {
        for (int e = lane; e < mk; e += 64) lut_lds[e] = src[e];
    }
}

// One step into the wave's stage: the chunks [j0, j0 + jn), lane by lane, whose rows begin at
// row0 = j0 * C and are nrows.  Args is the kernel's argument struct (words, nwords, chunk_off,
// chunk_prev, T, raw_first, codes, n, win_words and err are read).
//  SRC = 0  the chunks' stream window into `win`, then every lane decodes its chunk into its
//           stage slot: PosRd over the window where there is one, the lane's own SelRd of the
//           global stream otherwise; walk_packed for rows of NW u64 words, walk_parts for any
//           m <= 16.  BOUNDED: the step belongs to a range or a list that
//           ends at row `hi`, so the window is that of jn chunks, not of 64, and a chunk cut by
//           that end is decoded up to it only.  FL: a lane decodes fl_cnt rows, up to its last
//           kept one, and a chunk without a kept row is not looked at.
//  SRC = 1  the plain rows copied into the stage.
// Returns the lanes whose chunk failed (error bit 1 is set then); on return the stage is
// complete for every lane of the wave.
// (scat_rows of pqh_regroup.hip has the lane's walk a second time, for u16 codes too: with the
// walk as a function of its own that both call, adc_scan's filtered whole-stream form measured
// 2 to 7 % slower, whichever way its arguments were passed.)
template <int SRC, int NW, bool CTX, bool FL, bool BOUNDED, class Args>
__device__ __forceinline__ unsigned long long stage_step(const Args& a, unsigned char* stage,
                                                         uint32_t* win, int lane, int m, int C,
                                                         long long j0, long long jn, long long hi,
                                                         long long row0, int nrows, int fl_cnt,
                                                         long long chunks) {
    unsigned long long dead = 0;   // lanes whose chunk failed
    if constexpr (SRC == 0) {
        const unsigned long long nbits = (unsigned long long)a.nwords * 32;
        const int span = BOUNDED ? (int)jn : 64;   // the chunks the stream window is staged for
        bool use_win = false;
        StreamWin sw{0, 0, false};
        if (a.win_words > 0) {   // (then L = 64: the window is that of 64 chunks)
            const unsigned long long b_lo = a.chunk_off[j0];
            const unsigned long long b_hi = j0 + span < chunks ? a.chunk_off[j0 + span] : nbits;
            // (an index that does not ascend or leaves the stream: no window, every
            // lane's own offset is then checked by SelRd)
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
            // (BOUNDED: a chunk cut by the range's end is decoded up to that end only; FL: up
            // to its last kept row, and one without a kept row is not looked at)
            const int cnt = FL ? fl_cnt : (int)min((long long)C, (BOUNDED ? hi : a.n) - j * C);
            const unsigned long long off = a.chunk_off[j];
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
                    return walk_packed<CTX, NW, 8>(br, a.T, raw, cnt, prev,
                                                   [&](int s, int w, unsigned long long row) {
                                                       st[s * NW + w] = row;
                                                   });
                } else {
                    // the running row is the stage slot being decoded: it starts as a
                    // copy of the row before it
                    unsigned char* st = stage + (long long)lane * C * m;
                    for (int i = 0; i < m; ++i)
                        st[i] = (CTX && !raw)
                                    ? static_cast<const unsigned char*>(a.chunk_prev)[j * m + i]
                                    : (unsigned char)0;
                    int cur = 0;
                    return walk_parts<0>(
                        br, a.T, m, CTX, raw, cnt,
                        [&](int i) -> unsigned char& { return st[cur * m + i]; },
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
    return dead;
}

// A staged row against the tables in LDS ([m][k][QB]): sum[q] = ((lut[0][c_0] + lut[1][c_1]) +
// ...) in fp32, part by part.  (A failed chunk's slots hold anything: min(c, k - 1) keeps the
// read inside the table.)  adc_scan calls this; radius_scan has the same lines in its loop,
// because as a call of any shape tried its count instantiations with a batch of tables take
// twice the registers.  A change here is a change there.
template <int NW, int QB>
__device__ __forceinline__ void score_row(const unsigned char* row, const float* lut_lds, int m,
                                          int k, float (&sum)[QB]) {
    auto add = [&](int i, unsigned c) {
        if constexpr (QB == 1) {   // one ds_read_b32 a part
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
}

// ------------------------------------------------------------------- host side
inline int floor_pow2(long long v) {
    int p = 1;
    while (2ll * p <= v) p *= 2;
    return p;
}

// The launch of a scan from the shapes alone (plain integers: nothing of a context or a device).
//  src 0: the stream in chunks of C rows; 1: plain codes, C = kCodesRowsPerLane.  nw: the row's
//  u64 words (0: per part).  rg: per-query ranges, one query per workgroup; rt (with rg): one
//  table per range, kept per wave.  wide: top_k > 64, the wide list.
struct ScanGeometry {
    int qb;                     // queries (tables) per workgroup
    int L;                      // lanes (chunks) per wave and step
    int stage_bytes, win_words; // per wave
    long long lut_bytes;        // the batch's tables
    long long per_wave;         // stage and window
    long long wave_table;       // rt: the wave's table
    int fit;                    // the waves the LDS and the form allow
    int waves;
    long long steps, batches, groups;
    size_t lds;                 // tables, stages and windows of `waves` waves
    size_t lds_of(int w) const {
        return wave_table ? (size_t)w * (size_t)(wave_table + per_wave)
                          : (size_t)lut_bytes + (size_t)w * (size_t)per_wave;
    }
};

inline int scan_geometry(int num_cus, int tune_search_groups, int src, int nw, long long n, int m,
                         int k, int C, long long nq, bool rg, bool rt, bool wide, ScanGeometry* g) {
    // the batch's tables: at most 64 KB; 16-part rows keep to four queries (eight running
    // sums beside sixteen unrolled parts spill registers)
    // wide: four queries at the most (the list's entries are registers) and kWideWavesMax
    // waves (the lists' exchange at the end has to fit the LDS)
    g->qb = rg ? 1 : (!wide && m <= 8 && (long long)m * k <= 2048) ? 8 : 4;
    g->lut_bytes = (long long)m * k * g->qb * 4;
    const long long budget = kLdsBytes - g->lut_bytes;
    const long long chunks = (n + C - 1) / C;
    // a wave's stage: the rows of 64 chunks, or of as many as fit
    const long long row_bytes = (long long)C * m;
    g->L = 64;
    if (((64 * row_bytes + 15) & ~15ll) > budget) g->L = (int)((budget - 16) / row_bytes);
    if (g->L < 1) return PQH_ERR_UNSUPPORTED;   // (a chunk of more than ~96 KB of codes)
    g->stage_bytes = (int)((g->L * row_bytes + 15) & ~15ll);
    // the stream window as pqh_decode's row kernels size it (a longer span is read from
    // global memory)
    g->win_words = 0;
    if (src == 0 && g->L == 64) {
        const long long span_words = (64ll * C * m * 12 + 31) / 32 + 8;
        const long long ww = std::min<long long>(4096 - 1024 * (nw == 2 ? 1 : 0),
                                                 std::max<long long>(256, span_words));
        g->win_words = (int)((ww + 3) & ~3ll);
        if (g->stage_bytes + (g->win_words + 4) * 4 > budget) g->win_words = 0;
    }
    g->per_wave = g->stage_bytes + (g->win_words ? (g->win_words + 4) * 4 : 0);
    // rt: every wave has a table of its own beside its stage (one of them is in the budget,
    // so one wave always fits)
    g->wave_table = rt ? range_table_bytes(m * k) : 0;
    if (g->per_wave + g->wave_table > kLdsBytes) return PQH_ERR_UNSUPPORTED;   // (rounding, at most)
    g->fit = floor_pow2(std::min<long long>(
        wide ? kWideWavesMax : kScanWavesMax,
        rt ? kLdsBytes / (g->per_wave + g->wave_table) : budget / g->per_wave));
    g->steps = (chunks + g->L - 1) / g->L;
    g->batches = (nq + g->qb - 1) / g->qb;
    // one workgroup per compute unit over all query batches (a workgroup's tables take most
    // of a compute unit's LDS), each wave with at least two steps where there are that many
    long long groups = tune_search_groups > 0 ? tune_search_groups
                                              : std::max<long long>(1, num_cus / g->batches);
    if (rg) {
        // A query's steps are known on the device only: the grid is fixed here.  One table
        // leaves room for several workgroups of kRangeWaves waves on a compute unit, and
        // nq * groups workgroups fill the compute units kRangeFill times over; a query has at
        // most the stream's steps unless its ranges overlap.
        g->fit = std::min(g->fit, rt ? kRangeTableWaves : kRangeWaves);
        // rt: the waves' tables are most of the LDS, which holds twelve waves a compute unit at
        // m = 8 where the one-table form holds twenty.  The grid is what is resident at once
        // and no more (rounded down: a workgroup more would wait for a whole round of the
        // others), in workgroups of two waves so that the rounding costs little
        long long wgs = (kRangeFill * (long long)num_cus + nq - 1) / nq;
        if (rt)
            wgs = kLdsBytes / (g->fit * (g->per_wave + g->wave_table)) * (long long)num_cus / nq;
        if (tune_search_groups <= 0)
            groups = std::min<long long>(wgs, (g->steps + g->fit - 1) / g->fit);
        groups = std::min<long long>(std::max<long long>(groups, 1), 65535);
    } else {
        groups = std::min<long long>(std::min<long long>(groups, g->steps), 65535);
    }
    g->groups = groups;
    g->waves = rg ? g->fit
                  : std::min(g->fit, floor_pow2((g->steps + 2 * groups - 1) / (2 * groups)));
    g->lds = g->lds_of(g->waves);
    return PQH_OK;
}

// f(SRC, NW, CTX, QB, RT) with the run-time values as integral constants: rt and rg are one
// query per workgroup, the others a batch of qb = 8 or 4 (16-part rows: four).  The kernel's
// own last flags are f's to add.
template <typename F>
int scan_dispatch(int src, int nw, bool cx, int qb, bool rg, bool rt, F&& f) {
    auto with_qb = [&](auto s, auto w, auto c) -> int {
        if (rt) return f(s, w, c, Int<1>(), std::true_type());
        if (rg) return f(s, w, c, Int<1>(), std::false_type());
        if constexpr (decltype(w)::value != 2)
            if (qb == 8) return f(s, w, c, Int<8>(), std::false_type());
        return f(s, w, c, Int<4>(), std::false_type());
    };
    auto with_nw = [&](auto s, auto c) -> int {
        return nw == 1 ? with_qb(s, Int<1>(), c) : nw == 2 ? with_qb(s, Int<2>(), c)
                                                           : with_qb(s, Int<0>(), c);
    };
    if (src == 1) return with_nw(Int<1>(), std::false_type());
    return cx ? with_nw(Int<0>(), std::true_type()) : with_nw(Int<0>(), std::false_type());
}

// The stream as a scan's source: the argument checks that need no device, and the source
// fields of either argument struct.  *nw = the row's u64 words for the packed walk (rows of
// whole u64 words with the chunk contexts readable as such), 0 for the walk part by part.
// (A stream of 2^60 bytes or more is refused by the caller, once its other arguments are good.)
template <class Args>
int stream_source(Args& a, const pqh_tables_t* t, const unsigned char* d_stream,
                  unsigned long long stream_bytes, long long n, long long nq, int raw_first,
                  int chunk_vectors, const unsigned long long* d_chunk_offsets,
                  const void* d_chunk_prev, int* nw) {
    if (!t || chunk_vectors < 1) return PQH_ERR_ARG;
    if (n > 0 && nq > 0 && (stream_bytes < 4 || !d_chunk_offsets)) return PQH_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(d_stream) & 3u) return PQH_ERR_ARG;
    if (t->context && !d_chunk_prev && (!raw_first || n > chunk_vectors)) return PQH_ERR_ARG;
    if (t->k > 256 || t->m > 16) return PQH_ERR_UNSUPPORTED;
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
    *nw = packed ? t->m / 8 : 0;
    return PQH_OK;
}

// The same for plain u8 codes [n][m].
template <class Args>
int codes_source(Args& a, const void* d_codes, long long n, int m, int k, int* nw) {
    if (m < 1 || k < 1) return PQH_ERR_ARG;
    if (k > 256 || m > 16) return PQH_ERR_UNSUPPORTED;
    a.codes = static_cast<const unsigned char*>(d_codes);
    a.n = n;
    a.m = m;
    a.k = k;
    a.C = kCodesRowsPerLane;
    *nw = (m == 8 || m == 16) ? m / 8 : 0;
    return PQH_OK;
}

}  // namespace
