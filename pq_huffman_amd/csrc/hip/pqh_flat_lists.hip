// pqh_flat_lists.hip -- IVF-Flat: the exact k nearest among the raw fp32 rows of the lists every
// query probes.  Every distance is the definition's chain (chain_step, the
// arithmetic of pqh_flat_search), so there is no screen, no norm and no limit on d.
//
//  flat_lists<IP, KR>  grid (work units) x (G groups), four waves.  A unit is a list and up to
//                 QB of the (query, probe) pairs that probe it (the list-major plan of
//                 pqh_search.hip; QB = 16 with the 64-entry list, 4 with the wide one).  The
//                 list's rows are walked in tiles of 256, lane = row, a wave 64 of them; group g
//                 of a unit takes the tiles [g nt / G, (g + 1) nt / G).  A tile passes through LDS
//                 in chunks of kJC dimensions, [row][kJC + 1] floats: read from global memory
//                 with consecutive lanes on consecutive floats of a row (float4 where d % 4 == 0
//                 and the rows lie on 16 bytes), double-buffered, the loads of chunk c + 1 issued
//                 before the arithmetic of chunk c, one barrier a chunk.  The unit's query
//                 values of the chunk lie beside it as [j][QB], read by every lane at one
//                 address (an LDS broadcast, four pairs a 16-byte read).  A lane keeps QB
//                 accumulators across the chunks of a tile: the chain order is the definition's.
//                 After a tile's last chunk the wave leaves its distances in its own rows of the
//                 buffer it has just read, and pair by pair offers them to the pair's running
//                 list, which lives in LDS per (wave, pair) and enters the lanes only when some
//                 lane beats its k-th entry.  Rows past the list's end or with a clear keep bit
//                 are not offered; a tile without a kept row is passed over before it is loaded.
//                 At the end wave w merges the four lists of pairs w, w + 4, ... and writes them
//                 to the pair's partial slot [pair][G][k] with stream rows as ids.
//  The partial lists of a query, nprobe * G of them, are merged by adc_merge (pqh_search.hip).
//  The order (dist, stream row) is total and every list an exact top k of its rows, so the
//  result depends on neither the grid nor G nor the order of the units.
#include <algorithm>
#include <atomic>

#include "pqh_flat_dev.h"
#include "pqh_internal.h"
#include "pqh_topk_dev.h"

namespace {

constexpr int kTile = 256;          // rows a workgroup scores at once, lane = row
constexpr int kJC = 32;             // dimensions a staged chunk
// Rows kPitch floats apart in LDS.  The lanes of a wave read one column of 64 consecutive rows:
// word addresses lane * kPitch + j, which fall into distinct banks iff kPitch is odd (coprime
// to the number of banks, a power of two).  kJC + 1 is the smallest such pitch.
constexpr int kPitch = kJC + 1;
constexpr int kWaves = 4;
constexpr int kPre = kTile * kJC / (64 * kWaves);   // floats of a chunk a thread moves: 32

struct ListsArgs {
    const float* x;
    long long ld_x;
    int d, nprobe;
    const long long* offsets;
    const long long* units;
    const long long* nunits;
    const int* pairs;
    const float* q;
    long long ld_q;
    int k, vec_x;
    const unsigned* keep;
    float* part_d;       // [pairs][G][k]
    long long* part_id;
};

__host__ __device__ constexpr int lists_qb(int KR) { return KR == 1 ? 16 : 4; }
size_t lists_lds_bytes(int qb, int k) {
    return (size_t)2 * (kTile * kPitch + kJC * qb) * 4 + (size_t)kWaves * qb * k * 8;
}

template <bool IP, int KR>
__global__ void __launch_bounds__(64 * kWaves)
flat_lists(const ListsArgs a) {
    constexpr int QB = lists_qb(KR);
    constexpr int QE = (kJC * QB + 64 * kWaves - 1) / (64 * kWaves);   // query values a thread stages
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.y);
    const int tid = wave * 64 + lane;
    // the grid is the host's bound of the units: a workgroup beyond those there are leaves as a
    // whole, before any barrier
    if ((long long)blockIdx.x >= a.nunits[0]) return;
    const long long u_list = a.units[3 * (long long)blockIdx.x];
    const long long u_first = a.units[3 * (long long)blockIdx.x + 1];
    const int u_cnt = (int)a.units[3 * (long long)blockIdx.x + 2];
    // (a good pair of offsets with rows, or lists_plan had made no unit of the list)
    const long long l_first = a.offsets[u_list];
    const int l_count = (int)(a.offsets[u_list + 1] - l_first);
    const int k = a.k, kth = k - 1, d = a.d;
    const bool vec = a.vec_x != 0;

    float* const xbuf = smem;                             // [2][kTile][kPitch]
    float* const qbuf = smem + 2 * kTile * kPitch;        // [2][kJC][QB]
    float* const ls_d = qbuf + 2 * kJC * QB;              // [kWaves][QB][k]
    int* const ls_i = reinterpret_cast<int*>(ls_d + kWaves * QB * k);
    for (int i = lane; i < QB * k; i += 64) ls_d[wave * QB * k + i] = INFINITY, ls_i[wave * QB * k + i] = -1;

    // the query values this thread stages per chunk: entry idx = e * 256 + tid of [QB][kJC]
    const float* qrow[QE];
    int qat[QE], qj[QE];
#pragma unroll
    for (int e = 0; e < QE; ++e) {
        const int idx = e * 64 * kWaves + tid, qq = idx / kJC;
        qj[e] = idx % kJC;
        qat[e] = idx < kJC * QB ? qj[e] * QB + qq : -1;
        qrow[e] = qq < u_cnt ? a.q + (long long)(a.pairs[u_first + qq] / a.nprobe) * a.ld_q : nullptr;
    }

    // this group's tiles
    const int nt = (l_count + kTile - 1) / kTile;
    const int t_lo = (int)((long long)blockIdx.y * nt / gridDim.y);
    const int t_hi = (int)(((long long)blockIdx.y + 1) * nt / gridDim.y);
    // whether this thread's row of tile t takes part (the keep word of a row below n exists)
    auto row_live = [&](int t) -> bool {
        const int r = kTile * t + tid;
        if (r >= l_count) return false;
        if (!a.keep) return true;
        const long long v = l_first + r;
        return ((a.keep[v >> 5] >> (v & 31)) & 1u) != 0u;
    };
    // the first tile from t on with a kept row (workgroup-uniform; a barrier per tile looked at)
    auto next_live = [&](int t) -> int {
        if (a.keep)
            while (t < t_hi && !__syncthreads_or(row_live(t))) ++t;
        return t;
    };

    float pre[kPre], preq[QE];
    auto fetch = [&](int t, int c) {
        const long long r0 = l_first + (long long)kTile * t, last = l_first + l_count - 1;
        if (vec) {   // eight lanes a row's 32 floats
#pragma unroll
            for (int i = 0; i < kPre / 4; ++i) {
                const int p = i * 64 * kWaves + tid, j = c * kJC + 4 * (p & 7);
                const float* src = a.x + min(r0 + (p >> 3), last) * a.ld_x + j;
                const float4 v = j < d ? *reinterpret_cast<const float4*>(src) : make_float4(0.f, 0.f, 0.f, 0.f);
                pre[4 * i] = v.x, pre[4 * i + 1] = v.y, pre[4 * i + 2] = v.z, pre[4 * i + 3] = v.w;
            }
        } else {   // 32 lanes a row's 32 floats
#pragma unroll
            for (int i = 0; i < kPre; ++i) {
                const int p = i * 64 * kWaves + tid, j = c * kJC + (p & 31);
                pre[i] = j < d ? a.x[min(r0 + (p >> 5), last) * a.ld_x + j] : 0.f;
            }
        }
#pragma unroll
        for (int e = 0; e < QE; ++e) {
            const int j = c * kJC + qj[e];
            preq[e] = qrow[e] && j < d ? qrow[e][j] : 0.f;
        }
    };
    auto stash = [&](int b) {
        float* xd = xbuf + b * kTile * kPitch;
        if (vec) {
#pragma unroll
            for (int i = 0; i < kPre / 4; ++i) {
                const int p = i * 64 * kWaves + tid;
                float* dst = xd + (p >> 3) * kPitch + 4 * (p & 7);
                dst[0] = pre[4 * i], dst[1] = pre[4 * i + 1], dst[2] = pre[4 * i + 2], dst[3] = pre[4 * i + 3];
            }
        } else {
#pragma unroll
            for (int i = 0; i < kPre; ++i) {
                const int p = i * 64 * kWaves + tid;
                xd[(p >> 5) * kPitch + (p & 31)] = pre[i];
            }
        }
#pragma unroll
        for (int e = 0; e < QE; ++e)
            if (qat[e] >= 0) qbuf[b * kJC * QB + qat[e]] = preq[e];
    };

    const int nc = (d + kJC - 1) / kJC;
    float acc[QB];
    int t = next_live(t_lo), u = 0;
    if (t < t_hi) {
        fetch(t, 0);
        stash(0);
    }
    lds_barrier();
#pragma unroll 1
    while (t < t_hi) {
        int t1 = t;
#pragma unroll 1
        for (int c = 0; c < nc; ++c) {
            const bool end = c == nc - 1;
            if (end) t1 = next_live(t + 1);
            const bool more = !end || t1 < t_hi;
            if (more) fetch(end ? t1 : t, end ? 0 : c + 1);
            float* const xs = xbuf + (u & 1) * kTile * kPitch + tid * kPitch;
            const float* const qs = qbuf + (u & 1) * kJC * QB;
            const int jn = min(kJC, d - c * kJC);
            if (c == 0) {
#pragma unroll
                for (int qq = 0; qq < QB; ++qq) acc[qq] = 0.f;
            }
            // four pairs at a time, as far as the unit has pairs (wave-uniform)
#pragma unroll
            for (int g4 = 0; g4 < QB / 4; ++g4) {
                if (4 * g4 >= u_cnt) continue;
#pragma unroll 8
                for (int j = 0; j < jn; ++j) {
                    const float xv = xs[j];
                    const float4 qv = *reinterpret_cast<const float4*>(qs + j * QB + 4 * g4);
                    chain_step<IP>(acc[4 * g4], qv.x, xv);
                    chain_step<IP>(acc[4 * g4 + 1], qv.y, xv);
                    chain_step<IP>(acc[4 * g4 + 2], qv.z, xv);
                    chain_step<IP>(acc[4 * g4 + 3], qv.w, xv);
                }
            }
            if (end) {
                // The tile's distances.  The wave's 64 rows of this buffer are read by no other
                // wave and written again only after the next barrier: they take the distances,
                // [pair][lane], so that the pairs can be walked by a loop
                const bool valid = row_live(t);
                const int rel = kTile * t + tid;   // the row inside the list
                float* const ds = xbuf + (u & 1) * kTile * kPitch + wave * 64 * kPitch;
#pragma unroll
                for (int qq = 0; qq < QB; ++qq) ds[qq * 64 + lane] = acc[qq];
#pragma unroll 1
                for (int qq = 0; qq < u_cnt; ++qq) {
                    float* const ld = ls_d + (wave * QB + qq) * k;
                    int* const li = ls_i + (wave * QB + qq) * k;
                    const float dist = ds[qq * 64 + lane];
                    if (!__ballot(valid && lex_lt(dist, (long long)rel, ld[kth], (long long)li[kth])))
                        continue;   // (wave-uniform: nobody beats the k-th entry)
                    ListT<KR> e;
                    list_from_lds<KR>(e, ld, li, k);
                    list_offer<false>(e, dist, (long long)rel, valid, kth);
                    list_to_lds<KR>(e, ld, li, k);
                }
            }
            // the other buffer was last read before the barrier that ended the chunk before
            if (more) stash((u + 1) & 1);
            lds_barrier();
            ++u;
        }
        t = t1;
    }

    // ---- the four waves' lists of a pair into one, to the pair's slot of this group
#pragma unroll 1
    for (int qq = wave; qq < u_cnt; qq += kWaves) {
        ListT<KR> e;
        list_from_lds<KR>(e, ls_d + qq * k, ls_i + qq * k, k);
#pragma unroll 1
        for (int s = 1; s < kWaves; ++s) {
            const float* ld = ls_d + (s * QB + qq) * k;
            const int* li = ls_i + (s * QB + qq) * k;
#pragma unroll 1
            for (int b = 0; b <= (kth >> 6); ++b) {   // (a list ascends: 64 entries are sorted)
                const bool in = b * 64 + lane < k;
                const int id = in ? li[b * 64 + lane] : -1;
                list_offer<true>(e, in ? ld[b * 64 + lane] : INFINITY, (long long)id, id >= 0, kth);
            }
        }
        const long long at = ((long long)a.pairs[u_first + qq] * gridDim.y + blockIdx.y) * k;
        if constexpr (KR == 1) {
            if (lane < k) {
                a.part_d[at + lane] = e.d;
                a.part_id[at + lane] = e.id < 0 ? -1ll : l_first + e.id;
            }
        } else {
#pragma unroll
            for (int b = 0; b < kWideKR; ++b) {
                if (b * 64 + lane < k) {
                    a.part_d[at + b * 64 + lane] = e.d[b];
                    a.part_id[at + b * 64 + lane] = e.id[b] < 0 ? -1ll : l_first + e.id[b];
                }
            }
        }
    }
}

// ------------------------------------------------------------------- the host side
template <bool IP, int KR>
int lists_launch(pqh_ctx* ctx, const ListsArgs& a, long long units, int groups) {
    const size_t lds = lists_lds_bytes(lists_qb(KR), a.k);
    const auto fn = flat_lists<IP, KR>;
    // more than 64 KB of dynamic LDS is granted once per instantiation and device (the bitmap
    // holds devices 0 to 63; a device beyond them is granted again on every call)
    static std::atomic<unsigned long long> granted{0};
    const unsigned long long bit = ctx->device < 64 ? 1ull << ctx->device : 0ull;
    if (!(granted.load() & bit)) {
        const size_t most = lists_lds_bytes(lists_qb(KR), KR == 1 ? PQH_SEARCH_MAX_K : PQH_SEARCH_MAX_K_WIDE);
        PQH_HIP(ctx, hipFuncSetAttribute((const void*)fn,
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)most));
        granted.fetch_or(bit);
    }
    hipLaunchKernelGGL(fn, dim3((unsigned)units, (unsigned)groups), dim3(64, kWaves), lds,
                       ctx->stream, a);
    PQH_LAUNCH_CHECK(ctx);
    return PQH_OK;
}

int search_lists(bool ip, pqh_ctx_t* ctx, const float* d_x, long long n, long long ld_x, int d,
                 const long long* d_offsets, long long nlist, const long long* d_probes,
                 const float* d_queries, long long nq, long long ld_q, int nprobe, int top_k,
                 const unsigned int* d_keep_bits, long long id_base, float* d_dist,
                 long long* d_ids) {
    // what is wrong whatever the context
    if (n < 0 || d < 1 || ld_x < d || nlist < 1 || nq < 0 || ld_q < d || nprobe < 1 ||
        nprobe > PQH_IVF_MAX_NPROBE || top_k < 1 || top_k > PQH_SEARCH_MAX_K_WIDE || id_base < 0 ||
        id_base > 0x7FFFFFFFFFFFFFFFll - n)
        return PQH_ERR_ARG;
    if (nq > 0 && (!d_offsets || !d_probes || !d_queries || !d_dist || !d_ids || (n > 0 && !d_x)))
        return PQH_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(d_keep_bits) & 3u) return PQH_ERR_ARG;
    if (!ctx) return pqh_no_ctx_status();
    if (top_k > ctx->search_max_k) return PQH_ERR_ARG;
    if (n > 0x7FFFFFFFll || nlist > 0x7FFFFFFFll || nq > 0x7FFFFFFFll / nprobe)
        return PQH_ERR_UNSUPPORTED;
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    if (nq == 0) return PQH_OK;
    if (n == 0) return pqh_lists_merge_launch(ctx, nullptr, nullptr, 0, nq, top_k, id_base, d_dist, d_ids);

    const bool wide = top_k > PQH_SEARCH_MAX_K;
    const int qb = lists_qb(wide ? kWideKR : 1);
    const long long npairs = nq * nprobe;
    const long long bound = std::min<long long>(npairs, nlist + npairs / qb);
    const long long groups = lists_groups(ctx, n, nlist, bound, kTile);   // (pqh_flat_dev.h)

    const size_t entries = (size_t)npairs * groups * top_k;
    rc = pqh_ensure_ws(ctx, entries * 12 + 16 + pqh_list_plan_bytes(nlist, npairs, bound));
    if (rc) return rc;
    long long* part_id = static_cast<long long*>(ctx->ws);
    float* part_d = reinterpret_cast<float*>(part_id + entries);
    pqh_list_plan lp{};
    lp.offsets = d_offsets, lp.nlist = nlist, lp.probes = d_probes, lp.npairs = npairs, lp.n = n;
    lp.qb = qb, lp.pad = groups * top_k, lp.units_bound = bound;
    lp.mem = static_cast<long long*>(ctx->ws) + ((entries * 12 + 15) / 8);
    lp.part_d = part_d, lp.part_id = part_id, lp.err = ctx->d_diag + kDiagIvf;
    rc = pqh_list_plan_launch(ctx, &lp);
    if (rc) return rc;

    ListsArgs a{};
    a.x = d_x, a.ld_x = ld_x, a.d = d, a.nprobe = nprobe, a.offsets = d_offsets;
    a.units = lp.units, a.nunits = lp.nunits, a.pairs = lp.pairs;
    a.q = d_queries, a.ld_q = ld_q, a.k = top_k, a.keep = d_keep_bits;
    a.vec_x = d % 4 == 0 && ld_x % 4 == 0 && (reinterpret_cast<uintptr_t>(d_x) & 15u) == 0;
    a.part_d = part_d, a.part_id = part_id;
    rc = ip ? (wide ? lists_launch<true, kWideKR>(ctx, a, bound, (int)groups)
                    : lists_launch<true, 1>(ctx, a, bound, (int)groups))
            : (wide ? lists_launch<false, kWideKR>(ctx, a, bound, (int)groups)
                    : lists_launch<false, 1>(ctx, a, bound, (int)groups));
    if (rc) return rc;
    return pqh_lists_merge_launch(ctx, part_d, part_id, nprobe * groups, nq, top_k, id_base, d_dist, d_ids);
}

}  // namespace

extern "C" {

int pqh_flat_search_lists(pqh_ctx_t* ctx, const float* d_x, long long n, long long ld_x, int d,
                          const long long* d_offsets, long long nlist, const long long* d_probes,
                          const float* d_queries, long long nq, long long ld_q, int nprobe,
                          int top_k, const unsigned int* d_keep_bits, long long id_base,
                          float* d_dist, long long* d_ids) {
    return search_lists(false, ctx, d_x, n, ld_x, d, d_offsets, nlist, d_probes, d_queries, nq, ld_q,
                        nprobe, top_k, d_keep_bits, id_base, d_dist, d_ids);
}

int pqh_flat_search_lists_ip(pqh_ctx_t* ctx, const float* d_x, long long n, long long ld_x, int d,
                             const long long* d_offsets, long long nlist, const long long* d_probes,
                             const float* d_queries, long long nq, long long ld_q, int nprobe,
                             int top_k, const unsigned int* d_keep_bits, long long id_base,
                             float* d_dist, long long* d_ids) {
    return search_lists(true, ctx, d_x, n, ld_x, d, d_offsets, nlist, d_probes, d_queries, nq, ld_q,
                        nprobe, top_k, d_keep_bits, id_base, d_dist, d_ids);
}

}  // extern "C"
