// pqh_radius.hip -- range search: every scanned row with dist(q, v) < radius[q], straight from
// the compressed stream, as many results as there are.
//
//  radius_scan     the staging and scoring that adc_scan (pqh_search.hip) has, from the same
//                  source (pqh_scan_dev.h: one lane per chunk, 64 chunks per wave and step, the
//                  rows staged in the wave's LDS and scored 64 at a time against QB tables held
//                  in LDS with the query innermost), with a compare where adc_scan offers to its
//                  lists.  The output's size depends on the data, so the scan runs
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
//  scan_plan       (pqh_scan_dev.h) the step prefix of the ranges, as the probe search makes it.
//  radius_offsets  the plan's counts into exclusive int64 prefixes, and lims.
//
// What the fill pass skips: a workgroup whose span counted nothing (before its tables), a wave
// whose share counted nothing, the rest of a share once all it counted is written, and -- by a
// 64-bit word per share that the count pass leaves in the plan -- every step of a sub-share
// without a hit.  -DPQH_RADIUS_NO_SKIP compiles the rule out (tools/bench_range_search.py).
//
// dist is the scan's: ((lut[0][c_0] + lut[1][c_1]) + ...) in fp32, no contraction.  What is
// here is what differs from adc_scan: the contiguous shares, the plan and its header, the
// counts, the hit words, the skip rule and the fill; the mask rule, the step's location, the
// staging and the scoring are pqh_scan_dev.h's, and so are the launch geometry (scan_geometry)
// and the way to the template arguments (scan_dispatch).
#include <algorithm>
#include <cmath>
#include <type_traits>

#include "pqh_internal.h"
#include "pqh_scan_dev.h"

namespace {

constexpr int kHeaderWords = 8;            // the plan's header, in long longs
constexpr long long kPlanMagic = 0x5051485241444953ll;   // "PQHRADIS"

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
    const long long* steps_of;  // [nr + 1]: scan_plan's prefix
    const uint32_t* keep;       // FL
    long long* plan;            // header, then the entries
    PlanHeader geo;             // what this launch runs with
    long long capacity, id_base;   // FILL
    float* dist;
    long long* ids;
    unsigned long long* err;
};

// The counts of the plan into exclusive prefixes, in place, entry `total` the sum of all; and
// lims[q] = entry q * shares.  One workgroup, 1,024 entries a round: the int64 prefix of
// scan_plan (block_prefix).  (The lims of a round's entries are written in that round: entry
// q * shares is final once its round is.)
__global__ void __launch_bounds__(64 * kPlanWaves)
radius_offsets(long long* __restrict__ ent, long long total, long long shares, long long nq,
               long long* __restrict__ lims) {
    const int lane = threadIdx.x;
    const int wave = threadIdx.y;
    long long carry = 0;
    for (long long base = 0; base < total; base += 64 * kPlanWaves) {
        const long long i = base + wave * 64 + lane;
        long long all;
        const long long ex = carry + block_prefix(i < total ? ent[i] : 0, &all);
        if (i < total) {
            ent[i] = ex;
            if (i % shares == 0) lims[i / shares] = ex;
        }
        carry += all;
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
    float* lut_lds = reinterpret_cast<float*>(lds + (RT ? (size_t)wave * range_table_bytes(mk) : 0));
    const int per_wave = a.stage_bytes + (a.win_words ? (a.win_words + 4) * 4 : 0);
    unsigned char* stage = reinterpret_cast<unsigned char*>(lds) +
                           (RT ? (size_t)waves * range_table_bytes(mk) : (size_t)mk * QB * 4) +
                           (size_t)wave * per_wave;
    uint32_t* win = reinterpret_cast<uint32_t*>(stage + a.stage_bytes);

    if constexpr (!RT) load_batch_tables<QB>(lut_lds, a.lut, q0, a.nq, mk, wave, lane, waves);
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
            const RangeStep rs = range_step(r_cur, r_hi, t0 + g, a.steps_of, a.ranges, C, a.L);
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
        const long long row0 = j0 * C;
        const int nrows = (int)(min(a.n, (j0 + (RG ? jn : (long long)a.L)) * C) - row0);
        if constexpr (FL && !RG) {
            if (lane < jn) fl_cnt = kept_rows(a.keep, (j0 + lane) * C, max(row0, (j0 + lane) * C),
                                              min(row0 + nrows, (j0 + lane + 1) * C));
            if (!__ballot(fl_cnt > 0)) continue;
        }
        // lanes whose chunk failed
        const unsigned long long dead = stage_step<SRC, NW, CTX, FL, RG>(
            a, stage, win, lane, m, C, j0, jn, hi, row0, nrows, fl_cnt, chunks);

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
            // score_row's code, kept here: as a call (five cuts of it were tried) twelve count
            // instantiations go from 43-73 to 84-99 VGPRs and lose two or three waves a SIMD
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
// The launch of both passes is scan_geometry's, from the shapes alone: a contiguous share per
// wave in every form and no lists to exchange at the end, so its LDS is the stage part alone.
int geometry(const pqh_ctx_t* ctx, int src, int nw, long long n, int m, int k, int C, long long nq,
             bool rg, bool rt, ScanGeometry* g) {
    return scan_geometry(ctx->num_cus, ctx->tune_search_groups, src, nw, n, m, k, C, nq, rg, rt,
                         false, g);
}

unsigned long long plan_bytes_of(const ScanGeometry& g, long long nq) {
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
    ScanGeometry g;
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
        hipLaunchKernelGGL(scan_plan, dim3(1), dim3(64, kPlanWaves), 0, ctx->stream, c.ranges,
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
    // the range scan's own flags: a.keep set the filtered form, c.fill the pass
    rc = scan_dispatch(src, nw, cx, g.qb, rg, rt, [&](auto s, auto w, auto cxt, auto q, auto tb) -> int {
        return a.keep ? launch_fl(s, w, cxt, q, tb, std::true_type())
                      : launch_fl(s, w, cxt, q, tb, std::false_type());
    });
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
    RadiusArgs a{};
    int nw = 0;
    int rc = stream_source(a, t, d_stream, stream_bytes, n, c.nq, raw_first, chunk_vectors,
                           d_chunk_offsets, d_chunk_prev, &nw);
    if (rc) return rc;
    bool run = false;
    rc = call_check(ctx, d_stream != nullptr, n, c, &run);
    if (rc || !run) return rc;
    if (stream_bytes / 4 >= (1ull << 58)) return PQH_ERR_UNSUPPORTED;
    return scan_launch(ctx, 0, nw, t->context != 0, a, c);
}

int range_codes(pqh_ctx_t* ctx, const void* d_codes, long long n, int m, int k, const Call& c) {
    if (!ctx) return pqh_no_ctx_status();
    RadiusArgs a{};
    int nw = 0;
    int rc = codes_source(a, d_codes, n, m, k, &nw);
    if (rc) return rc;
    bool run = false;
    rc = call_check(ctx, d_codes != nullptr, n, c, &run);
    if (rc || !run) return rc;
    return scan_launch(ctx, 1, nw, false, a, c);
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
        ScanGeometry g;
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
