// pqh_search.hip -- asymmetric distance (ADC) search of a compressed stream: the decoder of
// pqh_decode.hip with a scoring phase where its store was.
//
//  adc_lut<IP> lut[q][i][c] = ||q_i - cent[i][c]||^2, one thread per entry (the oracle
//              arithmetic of pqh_pq_assign: fp32, j order, no contraction).  IP = 1
//              (pqh_adc_tables_ip): the negated inner product nip(q_i, cent[i][c]) of
//              pqh_ivf.hip's header in the entry's place; the scan is the same for both.
//  adc_scan    one lane per chunk, 64 chunks per wave and step: the chunks' stream window and
//              their decoded rows staged in the wave's LDS (stage_step; the walks are
//              pqh_decode_dev.h's), then every row scored against a batch of QB query tables
//              held in LDS with the query innermost (score_row), and offered to QB per-wave
//              top-k lists (one entry per lane, ascending by (dist, id)), merged per workgroup
//              at the end.  The codes never reach memory.  The mask rule, the step prefix of
//              the ranges (scan_plan), the table loads, a step's location in its range, the
//              staging and the scoring are pqh_scan_dev.h's, one statement shared with
//              radius_scan (pqh_radius.hip); here is what differs: the list-major form, the
//              wave-interleaved step order, the lists, and the exchange and merge at the end.
//              SRC = 1 loads plain u8 rows into the same stage instead of decoding them.
//              RG = 1 (the probe search): every query has its own row ranges, so a workgroup
//              holds one query's table (QB = 1) and its steps are those of scan_plan: a step
//              is up to L chunks of one range, and only the rows inside the range are offered.
//              RT = 1 (beside RG): one table per range, not per query.  Every wave keeps the
//              table of its current range in LDS of its own, reloads it when its step's range
//              changes, and takes a contiguous share of the workgroup's steps.
//              LM = 1 (the list-major probe search, QB = 8 or 4): a workgroup holds a list
//              and the tables of up to QB of the (query, probe) pairs that probe it, so a step
//              of the list is decoded once for all of them; its lists go to the pairs' slots.
//              FL = 1 (the *_masked calls, every form above): a bit per stream row says whether
//              the row may be returned.  A lane decodes its chunk as far as its last kept row
//              (not at all without one), and a step without a kept row is passed over before
//              its window, its rows or (RT) its table are loaded.
//              KR = 4 (top_k > 64, a context whose limit pqh_ctx_set_search_max_k raised; every
//              form above): the lists are pqh_topk_dev.h's wide ones, 256 entries a wave, four a
//              lane.  At most four queries a workgroup (QB <= 4, LM's units with it) and eight
//              waves: twelve more registers a query, and the waves' lists exchanged through LDS
//              at the end are waves * QB * 256 * 12 bytes.  KR = 1 is the code it was.
//  lists_*     the probe list turned round for LM: the pairs of every list in CSR form
//              (count, scan, fill), cut into work units of up to QB pairs.
//  adc_merge   one workgroup per query: every scan workgroup's list through the same list code
//              (pqh_topk_dev.h, shared with the probe selection of pqh_ivf.hip); adc_merge_wide
//              for top_k > 64.
//
// dist(v) = ((lut[0][c_0] + lut[1][c_1]) + ...) + lut[m-1][c_{m-1}] in fp32, the order total
// (dist, then row id), so the result does not depend on the grid.
#include <algorithm>
#include <cmath>
#include <type_traits>

#include "pqh_internal.h"
#include "pqh_scan_dev.h"
#include "pqh_topk_dev.h"

namespace {

template <bool IP>
__global__ void __launch_bounds__(256)
adc_lut(const float* __restrict__ queries, long long nq, long long ld_q,
        const float* __restrict__ cent, int m, int k, int dsub, float* __restrict__ lut) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long per = (long long)m * k;
    if (idx >= nq * per) return;
    const long long q = idx / per;
    const int e = (int)(idx - q * per);   // i * k + c
    const float* x = queries + q * ld_q + (long long)(e / k) * dsub;
    const float* c = cent + (long long)e * dsub;
    float acc = 0.f;
    for (int j = 0; j < dsub; ++j) {
        if constexpr (IP) {
            acc = acc - x[j] * c[j];
        } else {
            const float t = x[j] - c[j];
            acc = acc + t * t;
        }
    }
    lut[idx] = acc;
}

// ------------------------------------------------------------------- the scan
struct ScanArgs {
    const uint32_t* words;      // SRC = 0: the stream
    long long nwords;
    const unsigned long long* chunk_off;
    const void* chunk_prev;
    DecTabs T;
    int raw_first;
    int nprobe;                 // LM (in what was padding, as pair_tables: the struct keeps its
                                // layout, and the other forms' code with it)
    const unsigned char* codes; // SRC = 1: rows [n][m]
    long long n;
    int m, k;
    int C;                      // rows per lane and step (SRC = 0: the chunk size)
    int L;                      // lanes (chunks) per wave and step, 64 unless a chunk's rows
                                // are too many for the stage
    long long steps;            // ceil(chunks / L)
    int stage_bytes, win_words; // per wave
    const float* lut;           // [nq][m][k]; RT: [nr][m][k]; LM: either, by pair_tables
    long long nq;
    int top_k;
    int pair_tables;            // LM: lut holds one table per pair, not one per query
    float* part_d;              // [nq][groups][top_k]: one list per workgroup and query
    long long* part_id;         // (LM: [nq * nprobe][groups][top_k], per pair and workgroup)
    unsigned long long* err;
    union {
        // RG: the probe list in CSR form (device data, checked on the device) and scan_plan's
        // prefix
        struct {
            const long long* range_ptr; // [nq + 1]
            const long long* ranges;    // [nr][2]: first row, count
            long long nr;
            const long long* plan;      // [nr + 1]
        };
        // LM: the lists' rows, and lists_plan's work units with the pairs behind them
        struct {
            const long long* offsets;   // [nlist + 1]
            const long long* units;     // [unit bound][3]: list, first entry of pairs, entries
            const long long* nunits;    // how many of them there are
            const int* pairs;           // the pairs q * nprobe + p of every list, list by list
        };
    };
    const uint32_t* keep;       // FL: bit r & 31 of word r >> 5 = row r may be returned (at the
                                // end: the fields the other forms read stay where they were)
};
static_assert(sizeof(ScanArgs) == sizeof(DecTabs) + 176, "FL's field must not move the others");

// ------------------------------------------------------------------- the list-major plan
// The probe list [nq][nprobe] turned round: for every list the pairs q * nprobe + p that probe
// it, and the work units of the scan, a list and up to qb of its pairs each.  A pair takes
// part when its list id is in [0, nlist) and the list's offsets are a good range with rows;
// every other pair has no unit, so its partial lists are filled with the padding here (no
// memset of the buffer), and a list id that is neither -1 nor in [0, nlist) or a bad offsets
// pair sets error bit 2.  Four small launches: the counts zeroed, counted, scanned into units,
// and the pairs filled in (in any order: a pair's result does not depend on its batch).
struct ListArgs {
    const long long* offsets;   // [nlist + 1]
    long long nlist;
    const long long* probes;    // [pairs], -1 = none
    long long npairs;
    long long n;
    int qb;
    long long pad;              // groups * top_k: a pair's entries of the partial lists
    int* cnt;                   // [nlist]: the list's pairs, then the fill's cursor
    long long* units;
    long long* nunits;
    int* pairs;
    float* part_d;
    long long* part_id;
    unsigned long long* err;
};

// the list of pair i if it takes part, else -1 (*bad: a value that is reported)
__device__ __forceinline__ long long list_of_pair(const ListArgs& a, long long i, bool* bad) {
    const long long l = a.probes[i];
    *bad = false;
    if (l < 0 || l >= a.nlist) {
        *bad = l != -1;
        return -1;
    }
    const long long first = a.offsets[l], next = a.offsets[l + 1];
    if (first < 0 || next < first || !range_ok(first, next - first, a.n)) {
        *bad = true;
        return -1;
    }
    return next > first ? l : -1;
}

__global__ void __launch_bounds__(256) lists_zero(const ListArgs a) {
    const long long l = (long long)blockIdx.x * 256 + threadIdx.x;
    if (l < a.nlist) a.cnt[l] = 0;
}

__global__ void __launch_bounds__(256) lists_count(const ListArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.npairs) return;
    bool bad;
    const long long l = list_of_pair(a, i, &bad);
    if (l >= 0) {
        atomicAdd(a.cnt + l, 1);
    } else {
        for (long long e = i * a.pad; e < (i + 1) * a.pad; ++e) {
            a.part_d[e] = INFINITY;
            a.part_id[e] = -1ll;
        }
    }
    if (bad) atomicOr(a.err, 2ull);
}

// One workgroup, 1,024 lists a round as scan_plan: the exclusive prefixes of the lists' pairs
// and of their units, cnt[l] left as the first entry of the list's pairs, and every list's
// units written by its thread.
__global__ void __launch_bounds__(64 * kPlanWaves) lists_plan(const ListArgs a) {
    __shared__ int wsum[2][kPlanWaves];
    const int lane = threadIdx.x;
    const int wave = threadIdx.y;
    int carry_p = 0, carry_u = 0;   // (fewer than 2^31 pairs, so as many units at the most)
    for (long long base = 0; base < a.nlist; base += 64 * kPlanWaves) {
        const long long l = base + wave * 64 + lane;
        const int c = l < a.nlist ? a.cnt[l] : 0;
        const int s = (c + a.qb - 1) / a.qb;
        int inc_p = c, inc_u = s;   // the wave's inclusive prefixes
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int tp = __shfl_up(inc_p, d), tu = __shfl_up(inc_u, d);
            inc_p += lane >= d ? tp : 0;
            inc_u += lane >= d ? tu : 0;
        }
        if (lane == 63) wsum[0][wave] = inc_p, wsum[1][wave] = inc_u;
        lds_barrier();
        int p0 = carry_p + inc_p - c, u0 = carry_u + inc_u - s;
#pragma unroll 1
        for (int w = 0; w < kPlanWaves; ++w) {
            p0 += w < wave ? wsum[0][w] : 0;
            u0 += w < wave ? wsum[1][w] : 0;
            carry_p += wsum[0][w];
            carry_u += wsum[1][w];
        }
        if (l < a.nlist) {
            a.cnt[l] = p0;
#pragma unroll 1
            for (int b = 0; b < s; ++b) {
                long long* u = a.units + 3 * ((long long)u0 + b);
                u[0] = l;
                u[1] = p0 + b * a.qb;
                u[2] = min(a.qb, c - b * a.qb);
            }
        }
        lds_barrier();   // (wsum is written again in the next round)
    }
    if (wave == 0 && lane == 0) a.nunits[0] = carry_u;
}

__global__ void __launch_bounds__(256) lists_fill(const ListArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.npairs) return;
    bool bad;
    const long long l = list_of_pair(a, i, &bad);
    if (l >= 0) a.pairs[atomicAdd(a.cnt + l, 1)] = (int)i;
}

template <int SRC, int NW, bool CTX, int QB, bool RG = false, bool RT = false, bool LM = false,
          bool FL = false, int KR = 1>
__global__ void __launch_bounds__(64 * (KR == 1 ? kScanWavesMax : kWideWavesMax))
adc_scan(const ScanArgs a) {
    static_assert(KR == 1 || (KR == kWideKR && QB <= 4), "the wide list: four queries at the most");
    static_assert(RG == (QB == 1), "one query per workgroup is the probe search's form");
    static_assert(!RT || RG, "a table per range is a form of the probe search");
    static_assert(!LM || !RG, "the list-major form scores a batch of pairs");
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int lane = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.y);
    const int waves = (int)blockDim.y;
    const int m = NW ? 8 * NW : a.m;
    const int k = a.k;
    const int C = a.C;
    const int mk = m * k;
    // [m][k][QB]; RT: the wave's own [m][k], the waves' tables side by side before the stages
    float* lut_lds = reinterpret_cast<float*>(lds + (RT ? (size_t)wave * range_table_bytes(mk) : 0));
    const int per_wave = a.stage_bytes + (a.win_words ? (a.win_words + 4) * 4 : 0);
    unsigned char* stage = reinterpret_cast<unsigned char*>(lds) +
                           (RT ? (size_t)waves * range_table_bytes(mk) : (size_t)mk * QB * 4) +
                           (size_t)wave * per_wave;
    uint32_t* win = reinterpret_cast<uint32_t*>(stage + a.stage_bytes);

    // the batch's tables, the query innermost: one 16-byte read is four queries' entries
    // (RT: nothing yet, a wave loads the table of a range when it comes to it)
    const long long q0 = (long long)blockIdx.x * QB;
    // LM: the workgroup's unit, a list and up to QB of the pairs that probe it.  The grid is
    // the host's bound of the units: a workgroup beyond those there are leaves as a whole,
    // before any barrier
    long long u_list = 0, u_first = 0;
    int u_cnt = 0;
    if constexpr (LM) {
        if ((long long)blockIdx.x >= a.nunits[0]) return;
        u_list = a.units[3 * (long long)blockIdx.x];
        u_first = a.units[3 * (long long)blockIdx.x + 1];
        u_cnt = (int)a.units[3 * (long long)blockIdx.x + 2];
        // slot qq holds the table of its pair (or of the pair's query); a missing slot zeros
        const float* tab[QB];
#pragma unroll
        for (int qq = 0; qq < QB; ++qq) {
            const long long pair = qq < u_cnt ? a.pairs[u_first + qq] : 0;
            tab[qq] = a.lut + (a.pair_tables ? pair : pair / a.nprobe) * mk;
        }
        for (int e = wave * 64 + lane; e < mk; e += waves * 64) {
            float v[QB];
#pragma unroll
            for (int qq = 0; qq < QB; ++qq) v[qq] = qq < u_cnt ? tab[qq][e] : 0.f;
#pragma unroll
            for (int u = 0; u < QB / 4; ++u)
                reinterpret_cast<float4*>(lut_lds + (size_t)e * QB)[u] =
                    make_float4(v[4 * u], v[4 * u + 1], v[4 * u + 2], v[4 * u + 3]);
        }
    }
    if constexpr (!RT && !LM) load_batch_tables<QB>(lut_lds, a.lut, q0, a.nq, mk, wave, lane, waves);
    lds_barrier();

    // RG: the query's ranges [r_lo, r_hi) and its steps [t0, t0 + steps) of the plan; range_ptr
    // entries that are reversed or leave [0, nr] leave the query without steps (error bit 2)
    long long steps = a.steps;
    long long r_lo = 0, r_hi = 0, t0 = 0;
    if constexpr (RG) {
        const long long p0 = a.range_ptr[q0], p1 = a.range_ptr[q0 + 1];
        steps = 0;
        if (p0 >= 0 && p0 <= p1 && p1 <= a.nr) {
            r_lo = p0;
            r_hi = p1;
            t0 = a.plan[p0];
            steps = a.plan[p1] - t0;
        } else if (blockIdx.y == 0 && wave == 0 && lane == 0) {
            atomicOr(a.err, 2ull);
        }
    }

    // LM: the list's rows [l_first, l_first + l_count) -- a good pair with rows, or lists_plan
    // had made no unit of it -- and the steps of its chunks
    long long l_first = 0, l_count = 0;
    if constexpr (LM) {
        l_first = a.offsets[u_list];
        l_count = a.offsets[u_list + 1] - l_first;
        steps = ((l_first + l_count - 1) / C - l_first / C + a.L) / a.L;
    }

    std::conditional_t<KR == 1, TopK, TopKW> list[QB];
#pragma unroll
    for (int qq = 0; qq < QB; ++qq) {
        if constexpr (KR == 1)
            list[qq] = TopK{INFINITY, -1ll};
        else
            list_clear(list[qq]);
    }
    const int kth = a.top_k - 1;

    const long long chunks = (a.n + C - 1) / C;
    // this workgroup's span of steps; its waves take them in turn
    const long long g_lo = (long long)blockIdx.y * steps / gridDim.y;
    const long long g_hi = ((long long)blockIdx.y + 1) * steps / gridDim.y;
    // RT: a contiguous share for every wave instead.  A range's steps are neighbours, so its
    // table is loaded by the waves that share it, not by every wave of the workgroup (the
    // result is the same: the order is total).  In either form the trip counts differ from
    // wave to wave, so nothing in the loop may wait for another wave: the table is the wave's
    // own.  (g_inc an int: as a long long it changes the code of the other forms)
    const long long g_first = RT ? g_lo + (long long)wave * (g_hi - g_lo) / waves : g_lo + wave;
    const long long g_end = RT ? g_lo + ((long long)wave + 1) * (g_hi - g_lo) / waves : g_hi;
    const int g_inc = RT ? 1 : waves;
    long long r_loaded = -1;   // RT: the range whose table the wave holds
    long long r_cur = r_lo;   // RG: the range of the wave's last step (its steps ascend)
#pragma unroll 1
    for (long long g = g_first; g < g_end; g += g_inc) {
        long long j0 = g * a.L;
        long long jn = min(chunks - j0, (long long)a.L);
        long long lo = 0, hi = 0;   // RG: the step's rows inside its range are [lo, hi)
        // FL: the rows the lane decodes of its chunk.  A step none of whose chunks has a kept
        // row is left here: nothing of it is staged, and the wave_lds_sync that ended the step
        // before stands for it too (the loop has no barrier of the workgroup, and the waves'
        // trip counts differ anyway)
        int fl_cnt = 0;
        if constexpr (RG) {
            const RangeStep rs = range_step(r_cur, r_hi, t0 + g, a.plan, a.ranges, C, a.L);
            r_cur = rs.r, j0 = rs.j0, jn = rs.jn, lo = rs.lo, hi = rs.hi;
            if constexpr (FL) {
                if (lane < jn) fl_cnt = kept_rows(a.keep, (j0 + lane) * C, max(lo, (j0 + lane) * C),
                                                  min(hi, (j0 + lane + 1) * C));
                if (!__ballot(fl_cnt > 0)) continue;   // (before the table: a step without a kept row)
            }
            if constexpr (RT) {
                if (r_cur != r_loaded) {
                    load_range_table(lut_lds, a.lut, r_cur, mk, lane);
                    r_loaded = r_cur;
                }
            }
        }
        if constexpr (LM) {   // the step's chunks of the list, and its rows inside the list
            j0 = l_first / C + g * a.L;
            jn = min((l_first + l_count - 1) / C + 1 - j0, (long long)a.L);
            lo = max(l_first, j0 * C);
            hi = min(l_first + l_count, (j0 + jn) * C);
        }
        const long long row0 = j0 * C;
        const int nrows = (int)(min(a.n, (j0 + (RG || LM ? jn : (long long)a.L)) * C) - row0);
        if constexpr (FL && !RG) {
            const long long s_lo = LM ? lo : row0, s_hi = LM ? hi : row0 + nrows;
            if (lane < jn) fl_cnt = kept_rows(a.keep, (j0 + lane) * C, max(s_lo, (j0 + lane) * C),
                                              min(s_hi, (j0 + lane + 1) * C));
            if (!__ballot(fl_cnt > 0)) continue;
        }
        // lanes whose chunk failed
        const unsigned long long dead = stage_step<SRC, NW, CTX, FL, RG || LM>(
            a, stage, win, lane, m, C, j0, jn, hi, row0, nrows, fl_cnt, chunks);

        // the stage holds the wave's rows row0 ... row0 + nrows - 1 in order: lane scores
        // rows lane, lane + 64, ...
#pragma unroll 1
        for (int base = 0; base < nrows; base += 64) {
            const int r = base + lane;
            bool valid = r < nrows;
            if (dead && valid) valid = !((dead >> (r / C)) & 1ull);
            if constexpr (RG || LM) valid = valid && row0 + r >= lo && row0 + r < hi;
            if constexpr (FL)   // (the word of a row < n; the stage slots of rows no lane
                                // decoded hold anything and are not valid)
                if (r < nrows) valid = valid && ((a.keep[(row0 + r) >> 5] >> ((row0 + r) & 31)) & 1u);
            if constexpr (FL)   // (64 rows none of which takes part: no sums, nothing to offer)
                if (!__ballot(valid)) continue;
            const unsigned char* row = stage + (long long)(r < nrows ? r : 0) * m;
            float sum[QB];
            score_row<NW>(row, lut_lds, m, k, sum);
            const long long id = row0 + r;
#pragma unroll
            for (int qq = 0; qq < QB; ++qq)
                if (LM ? qq < u_cnt : q0 + qq < a.nq)
                    list_offer<false>(list[qq], sum[qq], id, valid, kth);
        }
        wave_lds_sync();   // the next step's staging overwrites what was just read
    }

    // The workgroup's lists into one per query: the tables and the stages are done with, so
    // every wave leaves its lists in LDS and wave w merges those of queries w, w + waves, ...
    lds_barrier();
    if constexpr (KR > 1) {
        // the wide list: a wave's blocks side by side, each offered as the sorted 64 it is
        float* wx_d = reinterpret_cast<float*>(lds);   // [waves][QB][KR][64]
        long long* wx_id = reinterpret_cast<long long*>(lds + (size_t)waves * QB * KR * 64 * 4);
#pragma unroll
        for (int qq = 0; qq < QB; ++qq) {
#pragma unroll
            for (int b = 0; b < KR; ++b) {
                wx_d[((wave * QB + qq) * KR + b) * 64 + lane] = list[qq].d[b];
                wx_id[((wave * QB + qq) * KR + b) * 64 + lane] = list[qq].id[b];
            }
        }
        lds_barrier();
#pragma unroll 1
        for (int qq = wave; qq < QB && (LM ? qq < u_cnt : q0 + qq < a.nq); qq += waves) {
            TopKW e;
            list_clear(e);
#pragma unroll 1
            for (int s = 0; s < waves; ++s) {
#pragma unroll 1
                for (int b = 0; b <= (kth >> 6); ++b) {
                    const float d = wx_d[((s * QB + qq) * KR + b) * 64 + lane];
                    const long long id = wx_id[((s * QB + qq) * KR + b) * 64 + lane];
                    list_offer<true>(e, d, id, id >= 0, kth);
                }
            }
            const long long slot = LM ? (long long)a.pairs[u_first + qq] : q0 + qq;
            const long long o = (slot * gridDim.y + blockIdx.y) * a.top_k;
#pragma unroll
            for (int b = 0; b < KR; ++b) {
                if (b * 64 + lane < a.top_k) {
                    a.part_d[o + b * 64 + lane] = e.d[b];
                    a.part_id[o + b * 64 + lane] = e.id[b];
                }
            }
        }
    } else {
        float* ex_d = reinterpret_cast<float*>(lds);   // [waves][QB][64]
        long long* ex_id = reinterpret_cast<long long*>(lds + (size_t)waves * QB * 64 * 4);
#pragma unroll
        for (int qq = 0; qq < QB; ++qq) {
            ex_d[(wave * QB + qq) * 64 + lane] = list[qq].d;
            ex_id[(wave * QB + qq) * 64 + lane] = list[qq].id;
        }
        lds_barrier();
#pragma unroll 1
        for (int qq = wave; qq < QB && (LM ? qq < u_cnt : q0 + qq < a.nq); qq += waves) {
            TopK e{INFINITY, -1ll};
#pragma unroll 1
            for (int s = 0; s < waves; ++s) {
                const float d = ex_d[(s * QB + qq) * 64 + lane];
                const long long id = ex_id[(s * QB + qq) * 64 + lane];
                list_offer<true>(e, d, id, id >= 0, kth);
            }
            if (lane < a.top_k) {
                // (LM: the pair's lists, one per group -- a group without steps leaves the padding)
                const long long slot = LM ? (long long)a.pairs[u_first + qq] : q0 + qq;
                const long long o = (slot * gridDim.y + blockIdx.y) * a.top_k + lane;
                a.part_d[o] = e.d;
                a.part_id[o] = e.id;
            }
        }
    }
}

// One workgroup of kMergeWaves waves per query: each wave takes its share of the scan's lists
// through the same list code (kMergeAhead loads in flight per lane), wave 0 then the other waves'; the
// result padded with (+inf, -1) and the ids moved by id_base.  lists = 0: the padding alone.
constexpr int kMergeWaves = 16;
constexpr int kMergeAhead = 4;
__global__ void __launch_bounds__(64 * kMergeWaves)
adc_merge(const float* __restrict__ part_d, const long long* __restrict__ part_id, long long lists,
          int top_k, long long id_base, float* __restrict__ dist, long long* __restrict__ ids) {
    __shared__ float xd[(kMergeWaves - 1) * 64];
    __shared__ long long xid[(kMergeWaves - 1) * 64];
    const int lane = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.y);
    const long long q = blockIdx.x;
    const long long total = lists * top_k;
    const int kth = top_k - 1;
    TopK e{INFINITY, -1ll};
#pragma unroll 1
    for (long long base = (long long)wave * 64 * kMergeAhead; base < total;
         base += 64 * kMergeAhead * kMergeWaves) {
        float d[kMergeAhead];
        long long id[kMergeAhead];
#pragma unroll
        for (int u = 0; u < kMergeAhead; ++u) {
            const long long idx = base + u * 64 + lane;
            d[u] = idx < total ? part_d[q * total + idx] : INFINITY;
            id[u] = idx < total ? part_id[q * total + idx] : -1ll;
        }
#pragma unroll
        for (int u = 0; u < kMergeAhead; ++u) {   // (64 entries are one sorted list when top_k = 64)
            if (top_k == 64)
                list_offer<true>(e, d[u], id[u], id[u] >= 0, kth);
            else
                list_offer<false>(e, d[u], id[u], id[u] >= 0, kth);
        }
    }
    if (wave > 0) {
        xd[(wave - 1) * 64 + lane] = e.d;
        xid[(wave - 1) * 64 + lane] = e.id;
    }
    lds_barrier();
    if (wave == 0) {
#pragma unroll 1
        for (int s = 0; s < kMergeWaves - 1; ++s) {
            const long long id = xid[s * 64 + lane];
            list_offer<true>(e, xd[s * 64 + lane], id, id >= 0, kth);
        }
        if (lane < top_k) {
            dist[q * top_k + lane] = e.d;
            ids[q * top_k + lane] = e.id < 0 ? -1ll : e.id + id_base;
        }
    }
}

// adc_merge for top_k > 64: the same shares and the same two rounds with the wide list.  A
// 64-entry piece of the partial lists is one sorted run only when no list ends inside it, that
// is when top_k is a multiple of 64.
__global__ void __launch_bounds__(64 * kMergeWaves)
adc_merge_wide(const float* __restrict__ part_d, const long long* __restrict__ part_id,
               long long lists, int top_k, long long id_base, float* __restrict__ dist,
               long long* __restrict__ ids) {
    __shared__ float xd[(kMergeWaves - 1) * kWideKR * 64];
    __shared__ long long xid[(kMergeWaves - 1) * kWideKR * 64];
    const int lane = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.y);
    const long long q = blockIdx.x;
    const long long total = lists * top_k;
    const int kth = top_k - 1;
    const bool runs = (top_k & 63) == 0;
    TopKW e;
    list_clear(e);
#pragma unroll 1
    for (long long base = (long long)wave * 64 * kMergeAhead; base < total;
         base += 64 * kMergeAhead * kMergeWaves) {
        float d[kMergeAhead];
        long long id[kMergeAhead];
#pragma unroll
        for (int u = 0; u < kMergeAhead; ++u) {
            const long long idx = base + u * 64 + lane;
            d[u] = idx < total ? part_d[q * total + idx] : INFINITY;
            id[u] = idx < total ? part_id[q * total + idx] : -1ll;
        }
#pragma unroll
        for (int u = 0; u < kMergeAhead; ++u) {
            if (runs)
                list_offer<true>(e, d[u], id[u], id[u] >= 0, kth);
            else
                list_offer<false>(e, d[u], id[u], id[u] >= 0, kth);
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int b = 0; b < kWideKR; ++b) {
            xd[((wave - 1) * kWideKR + b) * 64 + lane] = e.d[b];
            xid[((wave - 1) * kWideKR + b) * 64 + lane] = e.id[b];
        }
    }
    lds_barrier();
    if (wave == 0) {
#pragma unroll 1
        for (int s = 0; s < kMergeWaves - 1; ++s) {
#pragma unroll 1
            for (int b = 0; b <= (kth >> 6); ++b) {
                const long long id = xid[(s * kWideKR + b) * 64 + lane];
                list_offer<true>(e, xd[(s * kWideKR + b) * 64 + lane], id, id >= 0, kth);
            }
        }
#pragma unroll
        for (int b = 0; b < kWideKR; ++b) {
            if (b * 64 + lane < top_k) {
                dist[q * top_k + b * 64 + lane] = e.d[b];
                ids[q * top_k + b * 64 + lane] = e.id[b] < 0 ? -1ll : e.id[b] + id_base;
            }
        }
    }
}
// ------------------------------------------------------------------- host side
int merge_launch(pqh_ctx_t* ctx, const float* pd, const long long* pid, long long lists,
                 long long nq, int top_k, long long id_base, float* d_dist, long long* d_ids) {
    hipLaunchKernelGGL(top_k > PQH_SEARCH_MAX_K ? adc_merge_wide : adc_merge, dim3((unsigned)nq),
                       dim3(64, kMergeWaves), 0, ctx->stream, pd, pid, lists, top_k, id_base,
                       d_dist, d_ids);
    PQH_LAUNCH_CHECK(ctx);
    return PQH_OK;
}

// the scan and the merge; a.C, a.n, a.m, a.k and the source are set by the caller, nw = the
// row's u64 words (0: per part).  rg: the probe search (a.range_ptr, a.ranges and a.nr set):
// the plan first, then one query per workgroup.  rt (with rg): a.lut holds one table per
// range; the stage, the window and so the plan are those of rg, only the waves may be fewer.
// ls: the list-major probe search (a.offsets, a.nprobe and a.pair_tables set too): the lists_*
// kernels first, then one workgroup row per unit of the host's bound, and nprobe * groups lists
// per query for the merge.
struct ListProbe {
    const long long* offsets;
    long long nlist;
    const long long* probes;
    int nprobe;
    bool tables;   // d_lut is [nq * nprobe][m][K]
};
constexpr int kListWaves = 16;   // the list-major form: waves per workgroup at the most

int scan_launch(pqh_ctx_t* ctx, int src, int nw, bool cx, ScanArgs a, long long id_base,
                float* d_dist, long long* d_ids, bool rg = false, bool rt = false,
                const ListProbe* ls = nullptr) {
    if (a.nq > 0x7FFFFFFFll) return PQH_ERR_UNSUPPORTED;
    // the stage, the window, the batch and the grid of the whole-stream and the probe forms
    // (scan_geometry); top_k > 64 is the wide list
    const bool wide = a.top_k > PQH_SEARCH_MAX_K;
    ScanGeometry g;
    int rc = scan_geometry(ctx->num_cus, ctx->tune_search_groups, src, nw, a.n, a.m, a.k, a.C, a.nq,
                           rg, rt, wide, &g);
    if (rc) return rc;
    const int qb = g.qb;
    a.L = g.L;
    a.stage_bytes = g.stage_bytes;
    a.win_words = g.win_words;
    a.steps = g.steps;
    long long batches = g.batches, groups = g.groups;
    int waves = g.waves;
    // ls: the units are device data, at most one per pair and at most one part-filled per list
    const long long npairs = ls ? a.nq * ls->nprobe : 0;
    if (ls) {
        batches = std::min<long long>(npairs, ls->nlist + npairs / qb);
        // the default fills the compute units with the bound's units (a workgroup's tables
        // take most of a compute unit's LDS) and no list has more steps than the stream; a
        // group without steps writes the padding
        groups = ctx->tune_search_groups > 0 ? ctx->tune_search_groups
                                             : std::max<long long>(1, ctx->num_cus / batches);
        if (ctx->tune_search_groups <= 0) groups = std::min<long long>(groups, a.steps);
        groups = std::min<long long>(groups, 65535);
        // a list's steps are known on the device only; twice the mean list's share of steps
        // per group, kListWaves at the most
        const long long mean2 = 2 * ((a.steps + ls->nlist - 1) / ls->nlist);
        waves = std::min(std::min(g.fit, kListWaves), floor_pow2((mean2 + groups - 1) / groups));
    }
    // (a workgroup merges its waves' lists; ls: a list per pair and group)
    const long long lists = ls ? ls->nprobe * groups : groups;
    const size_t entries = (size_t)a.nq * lists * a.top_k;
    // beside the partial lists -- rg: the plan; ls: the units [batches][3] and their count,
    // the lists' counts and the pairs
    const size_t cnt_bytes = ls ? (((size_t)ls->nlist * 4 + 7) & ~(size_t)7) : 0;
    const size_t plan_bytes = rg   ? ((size_t)a.nr + 1) * 8
                              : ls ? ((size_t)batches * 3 + 1) * 8 + cnt_bytes + (size_t)npairs * 4
                                   : 0;
    rc = pqh_ensure_ws(ctx, entries * 12 + 16 + plan_bytes);
    if (rc) return rc;
    a.part_id = static_cast<long long*>(ctx->ws);
    a.part_d = reinterpret_cast<float*>(a.part_id + entries);
    a.err = ctx->d_diag + 1;
    if (rg) {
        long long* plan = static_cast<long long*>(ctx->ws) + ((entries * 12 + 15) / 8);
        hipLaunchKernelGGL(scan_plan, dim3(1), dim3(64, kPlanWaves), 0, ctx->stream, a.ranges, a.nr,
                           a.n, a.C, a.L, plan, a.err);
        PQH_LAUNCH_CHECK(ctx);
        a.plan = plan;
    }
    if (ls) {
        long long* units = static_cast<long long*>(ctx->ws) + ((entries * 12 + 15) / 8);
        ListArgs la{};
        la.offsets = ls->offsets;
        la.nlist = ls->nlist;
        la.probes = ls->probes;
        la.npairs = npairs;
        la.n = a.n;
        la.qb = qb;
        la.pad = groups * a.top_k;
        la.units = units;
        la.nunits = units + batches * 3;
        la.cnt = reinterpret_cast<int*>(la.nunits + 1);
        la.pairs = reinterpret_cast<int*>(reinterpret_cast<char*>(la.cnt) + cnt_bytes);
        la.part_d = a.part_d;
        la.part_id = a.part_id;
        la.err = a.err;
        const dim3 by_list((unsigned)((ls->nlist + 255) / 256)), by_pair((unsigned)((npairs + 255) / 256));
        hipLaunchKernelGGL(lists_zero, by_list, dim3(256), 0, ctx->stream, la);
        hipLaunchKernelGGL(lists_count, by_pair, dim3(256), 0, ctx->stream, la);
        hipLaunchKernelGGL(lists_plan, dim3(1), dim3(64, kPlanWaves), 0, ctx->stream, la);
        hipLaunchKernelGGL(lists_fill, by_pair, dim3(256), 0, ctx->stream, la);
        PQH_LAUNCH_CHECK(ctx);
        a.units = la.units;
        a.nunits = la.nunits;
        a.pairs = la.pairs;
    }
    // (the end of the kernel exchanges the waves' lists, 12 bytes an entry, through the same LDS)
    const size_t lds =
        std::max<size_t>(g.lds_of(waves), (size_t)waves * qb * (wide ? kWideKR : 1) * 64 * 12);
    auto launch_fl = [&](auto s, auto w, auto c, auto q, auto tb, auto lm, auto fl) -> int {
        auto go = [&](auto* fn) -> int {
            if (lds > 64 * 1024)
                PQH_HIP(ctx, hipFuncSetAttribute((const void*)fn,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(fn, dim3((unsigned)batches, (unsigned)groups), dim3(64, waves), lds,
                               ctx->stream, a);
            return PQH_OK;
        };
        if constexpr (decltype(q)::value <= 4)
            if (wide)
                return go(adc_scan<decltype(s)::value, decltype(w)::value, decltype(c)::value,
                                   decltype(q)::value, decltype(q)::value == 1, decltype(tb)::value,
                                   decltype(lm)::value, decltype(fl)::value, kWideKR>);
        return go(adc_scan<decltype(s)::value, decltype(w)::value, decltype(c)::value,
                           decltype(q)::value, decltype(q)::value == 1, decltype(tb)::value,
                           decltype(lm)::value, decltype(fl)::value>);
    };
    auto launch = [&](auto s, auto w, auto c, auto q, auto tb, auto lm) -> int {
        return a.keep ? launch_fl(s, w, c, q, tb, lm, std::true_type())
                      : launch_fl(s, w, c, q, tb, lm, std::false_type());
    };
    // search's own flags: LM for the batch forms of a *_lists call, a.keep set (the *_masked
    // calls) the filtered form of the same kernel, and the wide list
    rc = scan_dispatch(src, nw, cx, qb, rg, rt, [&](auto s, auto w, auto c, auto q, auto tb) -> int {
        if constexpr (decltype(q)::value > 1)
            if (ls) return launch(s, w, c, q, tb, std::true_type());
        return launch(s, w, c, q, tb, std::false_type());
    });
    if (rc) return rc;
    PQH_LAUNCH_CHECK(ctx);
    return merge_launch(ctx, a.part_d, a.part_id, lists, a.nq, a.top_k, id_base, d_dist, d_ids);
}

// the checks the two scans share; *run = false: nothing (more) to launch
int search_check(pqh_ctx_t* ctx, bool have_src, long long n, const float* d_lut, long long nq,
                 int top_k, long long id_base, float* d_dist, long long* d_ids, bool* run) {
    *run = false;
    if (n < 0 || nq < 0 || top_k < 1 || top_k > ctx->search_max_k) return PQH_ERR_ARG;
    if (nq > 0 && (!d_lut || !d_dist || !d_ids || (n > 0 && !have_src))) return PQH_ERR_ARG;
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    if (nq == 0) return PQH_OK;
    if (nq > 0x7FFFFFFFll) return PQH_ERR_UNSUPPORTED;
    if (n == 0) return merge_launch(ctx, nullptr, nullptr, 0, nq, top_k, id_base, d_dist, d_ids);
    *run = true;
    return PQH_OK;
}

// the probe list's host-side checks (its values are device data: scan_plan and adc_scan)
bool ranges_args_ok(long long nq, const long long* d_range_ptr, const long long* d_ranges,
                    long long nr) {
    return nr >= 0 && !(nq > 0 && (!d_range_ptr || (nr > 0 && !d_ranges)));
}

// the same for the *_lists calls (the values are device data: lists_count), and what the
// list-major form does not take: 2^31 pairs or lists
bool lists_args_ok(long long nq, const ListProbe* ls) {
    return ls->nlist >= 1 && ls->nprobe >= 1 && !(nq > 0 && (!ls->offsets || !ls->probes));
}
bool lists_too_many(long long nq, const ListProbe* ls) {
    return ls->nlist > 0x7FFFFFFFll || nq > 0x7FFFFFFFll / ls->nprobe;
}

// the probe list of the *_ranges calls
struct Probe {
    const long long* range_ptr;
    const long long* ranges;
    long long nr;
    bool tables = false;   // the *_range_tables calls: d_lut is [nr][m][K]
};

// pqh_search_stream (pr = null), pqh_search_stream_ranges and pqh_search_stream_range_tables;
// pqh_search_stream_lists (ls)
int search_stream(pqh_ctx_t* ctx, const pqh_tables_t* t, const unsigned char* d_stream,
                  unsigned long long stream_bytes, long long n, int raw_first, int chunk_vectors,
                  const unsigned long long* d_chunk_offsets, const void* d_chunk_prev,
                  const float* d_lut, long long nq, const Probe* pr, int top_k, long long id_base,
                  float* d_dist, long long* d_ids, const ListProbe* ls = nullptr,
                  const unsigned int* d_keep = nullptr) {
    if (!ctx) return pqh_no_ctx_status();
    if (reinterpret_cast<uintptr_t>(d_keep) & 3u) return PQH_ERR_ARG;
    if (pr && !ranges_args_ok(nq, pr->range_ptr, pr->ranges, pr->nr)) return PQH_ERR_ARG;
    if (ls && !lists_args_ok(nq, ls)) return PQH_ERR_ARG;
    ScanArgs a{};
    int nw = 0;
    int rc = stream_source(a, t, d_stream, stream_bytes, n, nq, raw_first, chunk_vectors,
                           d_chunk_offsets, d_chunk_prev, &nw);
    if (rc) return rc;
    if (ls && lists_too_many(nq, ls)) return PQH_ERR_UNSUPPORTED;
    bool run = false;
    rc = search_check(ctx, d_stream != nullptr, n, d_lut, nq, top_k, id_base, d_dist, d_ids, &run);
    if (rc || !run) return rc;
    if (pr && pr->nr == 0)
        return merge_launch(ctx, nullptr, nullptr, 0, nq, top_k, id_base, d_dist, d_ids);
    if (stream_bytes / 4 >= (1ull << 58)) return PQH_ERR_UNSUPPORTED;
    a.lut = d_lut;
    a.nq = nq;
    a.top_k = top_k;
    a.keep = d_keep;
    if (pr) a.range_ptr = pr->range_ptr, a.ranges = pr->ranges, a.nr = pr->nr;
    if (ls) a.offsets = ls->offsets, a.nprobe = ls->nprobe, a.pair_tables = ls->tables;
    return scan_launch(ctx, 0, nw, t->context != 0, a, id_base, d_dist, d_ids,
                       pr != nullptr, pr && pr->tables, ls);
}

// pqh_search_codes (pr = null), pqh_search_codes_ranges and pqh_search_codes_range_tables;
// pqh_search_codes_lists (ls)
int search_codes(pqh_ctx_t* ctx, const void* d_codes, long long n, int m, int k,
                 const float* d_lut, long long nq, const Probe* pr, int top_k, long long id_base,
                 float* d_dist, long long* d_ids, const ListProbe* ls = nullptr,
                 const unsigned int* d_keep = nullptr) {
    if (!ctx) return pqh_no_ctx_status();
    if (reinterpret_cast<uintptr_t>(d_keep) & 3u) return PQH_ERR_ARG;
    if (pr && !ranges_args_ok(nq, pr->range_ptr, pr->ranges, pr->nr)) return PQH_ERR_ARG;
    if (ls && !lists_args_ok(nq, ls)) return PQH_ERR_ARG;
    ScanArgs a{};
    int nw = 0;
    int rc = codes_source(a, d_codes, n, m, k, &nw);
    if (rc) return rc;
    if (ls && lists_too_many(nq, ls)) return PQH_ERR_UNSUPPORTED;
    bool run = false;
    rc = search_check(ctx, d_codes != nullptr, n, d_lut, nq, top_k, id_base, d_dist, d_ids, &run);
    if (rc || !run) return rc;
    if (pr && pr->nr == 0)
        return merge_launch(ctx, nullptr, nullptr, 0, nq, top_k, id_base, d_dist, d_ids);
    a.lut = d_lut;
    a.nq = nq;
    a.top_k = top_k;
    a.keep = d_keep;
    if (pr) a.range_ptr = pr->range_ptr, a.ranges = pr->ranges, a.nr = pr->nr;
    if (ls) a.offsets = ls->offsets, a.nprobe = ls->nprobe, a.pair_tables = ls->tables;
    return scan_launch(ctx, 1, nw, false, a, id_base, d_dist, d_ids,
                       pr != nullptr, pr && pr->tables, ls);
}

int adc_tables_call(bool ip, pqh_ctx_t* ctx, const pqh_pq_t* pq, const float* d_queries,
                    long long nq, long long ld_q, float* d_lut) {
    if (!ctx) return pqh_no_ctx_status();
    int m = 0, k = 0, dsub = 0;
    const float* d_cent = nullptr;
    if (pqh_pq_view(pq, &m, &k, &dsub, &d_cent) || nq < 0 || ld_q < (long long)m * dsub ||
        (nq > 0 && (!d_queries || !d_lut)))
        return PQH_ERR_ARG;
    if (k > 256) return PQH_ERR_UNSUPPORTED;
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    if (nq == 0) return PQH_OK;
    const long long blocks = (nq * m * k + 255) / 256;
    if (blocks > 0x7FFFFFFFll) return PQH_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(ip ? adc_lut<true> : adc_lut<false>, dim3((unsigned)blocks), dim3(256), 0,
                       ctx->stream, d_queries, nq, ld_q, d_cent, m, k, dsub, d_lut);
    PQH_LAUNCH_CHECK(ctx);
    return PQH_OK;
}

}  // namespace

extern "C" {

int pqh_adc_tables(pqh_ctx_t* ctx, const pqh_pq_t* pq, const float* d_queries, long long nq,
                   long long ld_q, float* d_lut) {
    return adc_tables_call(false, ctx, pq, d_queries, nq, ld_q, d_lut);
}

int pqh_adc_tables_ip(pqh_ctx_t* ctx, const pqh_pq_t* pq, const float* d_queries, long long nq,
                      long long ld_q, float* d_lut) {
    return adc_tables_call(true, ctx, pq, d_queries, nq, ld_q, d_lut);
}

int pqh_search_stream(pqh_ctx_t* ctx, const pqh_tables_t* t, const unsigned char* d_stream,
                      unsigned long long stream_bytes, long long n, int raw_first,
                      int chunk_vectors, const unsigned long long* d_chunk_offsets,
                      const void* d_chunk_prev, const float* d_lut, long long nq, int top_k,
                      long long id_base, float* d_dist, long long* d_ids) {
    return search_stream(ctx, t, d_stream, stream_bytes, n, raw_first, chunk_vectors,
                         d_chunk_offsets, d_chunk_prev, d_lut, nq, nullptr, top_k, id_base, d_dist,
                         d_ids);
}

int pqh_search_codes(pqh_ctx_t* ctx, const void* d_codes, long long n, int m, int k,
                     const float* d_lut, long long nq, int top_k, long long id_base,
                     float* d_dist, long long* d_ids) {
    return search_codes(ctx, d_codes, n, m, k, d_lut, nq, nullptr, top_k, id_base, d_dist, d_ids);
}

int pqh_search_stream_ranges(pqh_ctx_t* ctx, const pqh_tables_t* t, const unsigned char* d_stream,
                             unsigned long long stream_bytes, long long n, int raw_first,
                             int chunk_vectors, const unsigned long long* d_chunk_offsets,
                             const void* d_chunk_prev, const float* d_lut, long long nq,
                             const long long* d_range_ptr, const long long* d_ranges, long long nr,
                             int top_k, long long id_base, float* d_dist, long long* d_ids) {
    const Probe pr{d_range_ptr, d_ranges, nr};
    return search_stream(ctx, t, d_stream, stream_bytes, n, raw_first, chunk_vectors,
                         d_chunk_offsets, d_chunk_prev, d_lut, nq, &pr, top_k, id_base, d_dist,
                         d_ids);
}

int pqh_search_codes_ranges(pqh_ctx_t* ctx, const void* d_codes, long long n, int m, int k,
                            const float* d_lut, long long nq, const long long* d_range_ptr,
                            const long long* d_ranges, long long nr, int top_k, long long id_base,
                            float* d_dist, long long* d_ids) {
    const Probe pr{d_range_ptr, d_ranges, nr};
    return search_codes(ctx, d_codes, n, m, k, d_lut, nq, &pr, top_k, id_base, d_dist, d_ids);
}

int pqh_search_stream_range_tables(pqh_ctx_t* ctx, const pqh_tables_t* t,
                                   const unsigned char* d_stream, unsigned long long stream_bytes,
                                   long long n, int raw_first, int chunk_vectors,
                                   const unsigned long long* d_chunk_offsets,
                                   const void* d_chunk_prev, const float* d_lut, long long nq,
                                   const long long* d_range_ptr, const long long* d_ranges,
                                   long long nr, int top_k, long long id_base, float* d_dist,
                                   long long* d_ids) {
    const Probe pr{d_range_ptr, d_ranges, nr, true};
    return search_stream(ctx, t, d_stream, stream_bytes, n, raw_first, chunk_vectors,
                         d_chunk_offsets, d_chunk_prev, d_lut, nq, &pr, top_k, id_base, d_dist,
                         d_ids);
}

int pqh_search_codes_range_tables(pqh_ctx_t* ctx, const void* d_codes, long long n, int m, int k,
                                  const float* d_lut, long long nq, const long long* d_range_ptr,
                                  const long long* d_ranges, long long nr, int top_k,
                                  long long id_base, float* d_dist, long long* d_ids) {
    const Probe pr{d_range_ptr, d_ranges, nr, true};
    return search_codes(ctx, d_codes, n, m, k, d_lut, nq, &pr, top_k, id_base, d_dist, d_ids);
}

int pqh_search_stream_lists(pqh_ctx_t* ctx, const pqh_tables_t* t, const unsigned char* d_stream,
                            unsigned long long stream_bytes, long long n, int raw_first,
                            int chunk_vectors, const unsigned long long* d_chunk_offsets,
                            const void* d_chunk_prev, const long long* d_offsets, long long nlist,
                            const long long* d_probes, long long nq, int nprobe,
                            const float* d_lut, int tables_per_probe, int top_k,
                            long long id_base, float* d_dist, long long* d_ids) {
    const ListProbe ls{d_offsets, nlist, d_probes, nprobe, tables_per_probe != 0};
    return search_stream(ctx, t, d_stream, stream_bytes, n, raw_first, chunk_vectors,
                         d_chunk_offsets, d_chunk_prev, d_lut, nq, nullptr, top_k, id_base, d_dist,
                         d_ids, &ls);
}

int pqh_search_codes_lists(pqh_ctx_t* ctx, const void* d_codes, long long n, int m, int k,
                           const long long* d_offsets, long long nlist, const long long* d_probes,
                           long long nq, int nprobe, const float* d_lut, int tables_per_probe,
                           int top_k, long long id_base, float* d_dist, long long* d_ids) {
    const ListProbe ls{d_offsets, nlist, d_probes, nprobe, tables_per_probe != 0};
    return search_codes(ctx, d_codes, n, m, k, d_lut, nq, nullptr, top_k, id_base, d_dist, d_ids,
                        &ls);
}

// The *_masked calls: the same entry with d_keep behind d_ids (NULL: the call above, kernel
// for kernel).
int pqh_search_stream_masked(pqh_ctx_t* ctx, const pqh_tables_t* t, const unsigned char* d_stream,
                             unsigned long long stream_bytes, long long n, int raw_first,
                             int chunk_vectors, const unsigned long long* d_chunk_offsets,
                             const void* d_chunk_prev, const float* d_lut, long long nq, int top_k,
                             long long id_base, float* d_dist, long long* d_ids,
                             const unsigned int* d_keep) {
    return search_stream(ctx, t, d_stream, stream_bytes, n, raw_first, chunk_vectors,
                         d_chunk_offsets, d_chunk_prev, d_lut, nq, nullptr, top_k, id_base, d_dist,
                         d_ids, nullptr, d_keep);
}

int pqh_search_codes_masked(pqh_ctx_t* ctx, const void* d_codes, long long n, int m, int k,
                            const float* d_lut, long long nq, int top_k, long long id_base,
                            float* d_dist, long long* d_ids, const unsigned int* d_keep) {
    return search_codes(ctx, d_codes, n, m, k, d_lut, nq, nullptr, top_k, id_base, d_dist, d_ids,
                        nullptr, d_keep);
}

int pqh_search_stream_ranges_masked(pqh_ctx_t* ctx, const pqh_tables_t* t,
                                    const unsigned char* d_stream, unsigned long long stream_bytes,
                                    long long n, int raw_first, int chunk_vectors,
                                    const unsigned long long* d_chunk_offsets,
                                    const void* d_chunk_prev, const float* d_lut, long long nq,
                                    const long long* d_range_ptr, const long long* d_ranges,
                                    long long nr, int top_k, long long id_base, float* d_dist,
                                    long long* d_ids, const unsigned int* d_keep) {
    const Probe pr{d_range_ptr, d_ranges, nr};
    return search_stream(ctx, t, d_stream, stream_bytes, n, raw_first, chunk_vectors,
                         d_chunk_offsets, d_chunk_prev, d_lut, nq, &pr, top_k, id_base, d_dist,
                         d_ids, nullptr, d_keep);
}

int pqh_search_codes_ranges_masked(pqh_ctx_t* ctx, const void* d_codes, long long n, int m, int k,
                                   const float* d_lut, long long nq, const long long* d_range_ptr,
                                   const long long* d_ranges, long long nr, int top_k,
                                   long long id_base, float* d_dist, long long* d_ids,
                                   const unsigned int* d_keep) {
    const Probe pr{d_range_ptr, d_ranges, nr};
    return search_codes(ctx, d_codes, n, m, k, d_lut, nq, &pr, top_k, id_base, d_dist, d_ids,
                        nullptr, d_keep);
}

int pqh_search_stream_range_tables_masked(pqh_ctx_t* ctx, const pqh_tables_t* t,
                                          const unsigned char* d_stream,
                                          unsigned long long stream_bytes, long long n,
                                          int raw_first, int chunk_vectors,
                                          const unsigned long long* d_chunk_offsets,
                                          const void* d_chunk_prev, const float* d_lut,
                                          long long nq, const long long* d_range_ptr,
                                          const long long* d_ranges, long long nr, int top_k,
                                          long long id_base, float* d_dist, long long* d_ids,
                                          const unsigned int* d_keep) {
    const Probe pr{d_range_ptr, d_ranges, nr, true};
    return search_stream(ctx, t, d_stream, stream_bytes, n, raw_first, chunk_vectors,
                         d_chunk_offsets, d_chunk_prev, d_lut, nq, &pr, top_k, id_base, d_dist,
                         d_ids, nullptr, d_keep);
}

int pqh_search_codes_range_tables_masked(pqh_ctx_t* ctx, const void* d_codes, long long n, int m,
                                         int k, const float* d_lut, long long nq,
                                         const long long* d_range_ptr, const long long* d_ranges,
                                         long long nr, int top_k, long long id_base, float* d_dist,
                                         long long* d_ids, const unsigned int* d_keep) {
    const Probe pr{d_range_ptr, d_ranges, nr, true};
    return search_codes(ctx, d_codes, n, m, k, d_lut, nq, &pr, top_k, id_base, d_dist, d_ids,
                        nullptr, d_keep);
}

int pqh_search_stream_lists_masked(pqh_ctx_t* ctx, const pqh_tables_t* t,
                                   const unsigned char* d_stream, unsigned long long stream_bytes,
                                   long long n, int raw_first, int chunk_vectors,
                                   const unsigned long long* d_chunk_offsets,
                                   const void* d_chunk_prev, const long long* d_offsets,
                                   long long nlist, const long long* d_probes, long long nq,
                                   int nprobe, const float* d_lut, int tables_per_probe, int top_k,
                                   long long id_base, float* d_dist, long long* d_ids,
                                   const unsigned int* d_keep) {
    const ListProbe ls{d_offsets, nlist, d_probes, nprobe, tables_per_probe != 0};
    return search_stream(ctx, t, d_stream, stream_bytes, n, raw_first, chunk_vectors,
                         d_chunk_offsets, d_chunk_prev, d_lut, nq, nullptr, top_k, id_base, d_dist,
                         d_ids, &ls, d_keep);
}

int pqh_search_codes_lists_masked(pqh_ctx_t* ctx, const void* d_codes, long long n, int m, int k,
                                  const long long* d_offsets, long long nlist,
                                  const long long* d_probes, long long nq, int nprobe,
                                  const float* d_lut, int tables_per_probe, int top_k,
                                  long long id_base, float* d_dist, long long* d_ids,
                                  const unsigned int* d_keep) {
    const ListProbe ls{d_offsets, nlist, d_probes, nprobe, tables_per_probe != 0};
    return search_codes(ctx, d_codes, n, m, k, d_lut, nq, nullptr, top_k, id_base, d_dist, d_ids,
                        &ls, d_keep);
}

}  // extern "C"
