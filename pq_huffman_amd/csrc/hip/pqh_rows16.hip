// pqh_rows16.hip -- IVF-Flat over rows stored as fp16 or bf16, and the calls
// that take a row type (pqh_flat_search_lists_rows / _ip; pqh_flat_create_rows is pqh_flat.hip's).
// Every 16-bit value is an fp32 value, so the search is pqh_flat_search_lists over the rows
// converted to fp32: the definition's chain (chain_step) from the converted values, ids and the
// bits of dist.
//
//  rows16_lists<T, IP, KR>  flat_lists' outer shape (the list-major plan, a unit = a list and up
//                 to QB of its pairs, four waves, tiles of 256 rows with lane = row, G groups of
//                 tiles, partial lists [pair][G][k] merged by adc_merge, the row mask and the
//                 tile skip) and sq_lists' way of moving a tile.  A tile lies in LDS as 16-bit
//                 values in chunks of kJC = 32 dimensions, 64 bytes of a row, [256 rows][17
//                 dwords]: the lanes of a wave read one dword column of 64 consecutive rows, and
//                 the odd pitch keeps them in distinct banks.  A chunk comes from global memory
//                 16 bytes a lane, four lanes a row's 64 bytes, four such loads a thread (16
//                 registers); the loads of chunk c + 1 are issued before the arithmetic of chunk
//                 c, one barrier a chunk.  Beside a chunk lie the unit's query values [j][QB] as
//                 fp32, read at one address by every lane (LDS broadcasts).  A lane reads a dword
//                 of its row, converts its two halves once, and runs the chain steps of the
//                 unit's pairs four at a time; the number of groups of four is a template value
//                 of the chunk's loop.  No element from d on reaches an accumulator: it is not
//                 loaded, its half of the staged dword is zero, and so is its query value, so
//                 the chain step adds (0 - 0)^2 or subtracts 0 * 0, which changes no bit.
//                 2 (4,352 + 32 QB) dwords and the lists, 4 QB k 8 bytes: 71,680 B at k = 64,
//                 two workgroups a CU.
#include <algorithm>
#include <atomic>
#include <type_traits>

#include "pqh_flat_dev.h"
#include "pqh_internal.h"
#include "pqh_topk_dev.h"

namespace {

constexpr int kTile = 256;          // rows a workgroup scores at once, lane = row
// Dimensions a staged chunk.  32 (64 bytes of a row, pitch 17, two workgroups a CU) against 64
// (-DPQH_ROWS16_JC=64: pitch 33, one workgroup a CU, half the barriers): DESIGN.md 4.5.20.
#ifndef PQH_ROWS16_JC
#define PQH_ROWS16_JC 32
#endif
constexpr int kJC = PQH_ROWS16_JC;
static_assert(kJC == 32 || kJC == 64, "a chunk is 16 bytes a lane, 4 or 8 lanes a row");
// Rows kPitch dwords apart in LDS: word addresses lane * kPitch + w lie in distinct banks iff
// kPitch is odd; kJC / 2 + 1 is the smallest odd pitch that holds a chunk.
constexpr int kPitch = kJC / 2 + 1;
constexpr int kWaves = 4;
constexpr int kChunkWords = kTile * kPitch;   // 4,352 dwords = 17,408 B
constexpr int kLR = kJC / 8;                  // lanes a row's chunk, 16 bytes (eight elements) each
constexpr int kPre = kTile * kLR / (64 * kWaves);   // such pieces a thread moves: 4

struct __attribute__((aligned(4))) Quad {   // 16 bytes of a row that lie on 4 bytes
    unsigned w[4];
};

struct Rows16Args {
    const unsigned short* x;   // the rows as 16-bit words
    long long ld_x;
    int d, nprobe;
    const long long* offsets;
    const long long* units;
    const long long* nunits;
    const int* pairs;
    const float* q;
    long long ld_q;
    int k, words;        // words: ld_x even and the base on 4 bytes, a chunk is read by dwords
    const unsigned* keep;
    float* part_d;       // [pairs][G][k]
    long long* part_id;
};

__host__ __device__ constexpr int rows16_qb(int KR) { return KR == 1 ? 16 : 4; }
size_t rows16_lds_bytes(int qb, int k) {
    return (size_t)2 * (kChunkWords + kJC * qb) * 4 + (size_t)kWaves * qb * k * 8;
}

template <typename T, bool IP, int KR>
__global__ void __launch_bounds__(64 * kWaves)
rows16_lists(const Rows16Args a) {
    constexpr int QB = rows16_qb(KR);
    constexpr int QE = (kJC * QB + 64 * kWaves - 1) / (64 * kWaves);   // query values a thread stages
    static_assert(QB * 64 <= 64 * kPitch, "a tile's distances fit the wave's rows of a chunk");
    extern __shared__ __attribute__((aligned(16))) unsigned smem[];
    const int lane = threadIdx.x, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.y);
    const int tid = wave * 64 + lane;
    // the grid is the host's bound of the units: a workgroup beyond those there are leaves as a
    // whole, before any barrier
    if ((long long)blockIdx.x >= a.nunits[0]) return;
    const long long u_list = a.units[3 * (long long)blockIdx.x];
    const long long u_first = a.units[3 * (long long)blockIdx.x + 1];
    const int u_cnt = (int)a.units[3 * (long long)blockIdx.x + 2];
    // (a good pair of offsets with rows, or the plan had made no unit of the list)
    const long long l_first = a.offsets[u_list];
    const int l_count = (int)(a.offsets[u_list + 1] - l_first);
    const int k = a.k, kth = k - 1, d = a.d;

    unsigned* const xbuf = smem;                                              // [2][kTile][kPitch]
    float* const qbuf = reinterpret_cast<float*>(smem + 2 * kChunkWords);     // [2][kJC][QB]
    float* const ls_d = qbuf + 2 * kJC * QB;                                  // [kWaves][QB][k]
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

    // The prefetch: kPre times 16 bytes of a row (kLR lanes a row's chunk, 256 / kLR rows a step)
    // and the query values.  A row past the list's end reads the list's last row; an element from
    // d on is not read, its half of the dword is zero.
    unsigned pre[kPre][4];
    float preq[QE];
    auto fetch = [&](int t, int c) {
        const long long r0 = l_first + (long long)kTile * t, last = l_first + l_count - 1;
        const int j0 = c * kJC + 8 * (tid % kLR);
#pragma unroll
        for (int i = 0; i < kPre; ++i) {
            const unsigned short* src = a.x + min(r0 + kTile / kPre * i + tid / kLR, last) * a.ld_x + j0;
            if (a.words) {   // (every row on 4 bytes, j0 even: a dword of the row lies on 4 bytes)
                if (j0 + 8 <= d) {
                    const Quad v = *reinterpret_cast<const Quad*>(src);
                    pre[i][0] = v.w[0], pre[i][1] = v.w[1], pre[i][2] = v.w[2], pre[i][3] = v.w[3];
                } else {
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        const int e = j0 + 2 * w;
                        pre[i][w] = e + 2 <= d ? *reinterpret_cast<const unsigned*>(src + 2 * w)
                                    : e < d    ? (unsigned)src[2 * w]
                                               : 0u;
                    }
                }
            } else {
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const int e = j0 + 2 * w;
                    const unsigned lo = e < d ? (unsigned)src[2 * w] : 0u;
                    const unsigned hi = e + 1 < d ? (unsigned)src[2 * w + 1] : 0u;
                    pre[i][w] = lo | hi << 16;
                }
            }
        }
#pragma unroll
        for (int e = 0; e < QE; ++e) {
            const int j = c * kJC + qj[e];
            preq[e] = qrow[e] && j < d ? qrow[e][j] : 0.f;
        }
    };
    auto stash = [&](int b) {
#pragma unroll
        for (int i = 0; i < kPre; ++i) {
            unsigned* dst = xbuf + b * kChunkWords + (kTile / kPre * i + tid / kLR) * kPitch + 4 * (tid % kLR);
            dst[0] = pre[i][0], dst[1] = pre[i][1], dst[2] = pre[i][2], dst[3] = pre[i][3];
        }
#pragma unroll
        for (int e = 0; e < QE; ++e)
            if (qat[e] >= 0) qbuf[b * kJC * QB + qat[e]] = preq[e];
    };

    const int nc = (d + kJC - 1) / kJC;
    const int ng = (min(u_cnt, QB) + 3) >> 2;   // the unit's groups of four pairs (wave-uniform)
    float acc[QB];
    // a chunk's arithmetic for NG groups of four pairs: per dword of the row two conversions,
    // then the chain steps of every pair, j ascending
    auto chunk = [&](auto ngc, const unsigned* xs, const float* qs, int nw) {
        constexpr int NG = decltype(ngc)::value;
#pragma unroll 4
        for (int w = 0; w < nw; ++w) {
            const unsigned cw = xs[w];
            const float xv[2] = {half_lo<T>(cw), half_hi<T>(cw)};
#pragma unroll
            for (int g4 = 0; g4 < NG; ++g4) {
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const float4 qv = *reinterpret_cast<const float4*>(qs + (2 * w + b) * QB + 4 * g4);
                    chain_step<IP>(acc[4 * g4], qv.x, xv[b]);
                    chain_step<IP>(acc[4 * g4 + 1], qv.y, xv[b]);
                    chain_step<IP>(acc[4 * g4 + 2], qv.z, xv[b]);
                    chain_step<IP>(acc[4 * g4 + 3], qv.w, xv[b]);
                }
            }
        }
    };

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
            unsigned* const xc = xbuf + (u & 1) * kChunkWords;
            const unsigned* const xs = xc + tid * kPitch;
            const float* const qs = qbuf + (u & 1) * kJC * QB;
            const int nw = (min(kJC, d - c * kJC) + 1) >> 1;
            if (c == 0) {
#pragma unroll
                for (int qq = 0; qq < QB; ++qq) acc[qq] = 0.f;
            }
            if constexpr (QB == 4) {
                chunk(std::integral_constant<int, 1>{}, xs, qs, nw);
            } else {
                switch (ng) {
                    case 1: chunk(std::integral_constant<int, 1>{}, xs, qs, nw); break;
                    case 2: chunk(std::integral_constant<int, 2>{}, xs, qs, nw); break;
                    case 3: chunk(std::integral_constant<int, 3>{}, xs, qs, nw); break;
                    default: chunk(std::integral_constant<int, 4>{}, xs, qs, nw); break;
                }
            }
            if (end) {
                // The tile's distances.  The wave's 64 rows of this buffer are read by no other
                // wave and written again only after the next barrier: they take the distances,
                // [pair][lane] (QB * 64 of the 64 * kPitch dwords), so that the pairs can be
                // walked by a loop
                const bool valid = row_live(t);
                const int rel = kTile * t + tid;   // the row inside the list
                float* const ds = reinterpret_cast<float*>(xc + wave * 64 * kPitch);
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
template <typename T, bool IP, int KR>
int rows16_launch(pqh_ctx* ctx, const Rows16Args& a, long long units, int groups) {
    const size_t lds = rows16_lds_bytes(rows16_qb(KR), a.k);
    const auto fn = rows16_lists<T, IP, KR>;
    // more than 64 KB of dynamic LDS is granted once per instantiation and device (the bitmap
    // holds devices 0 to 63; a device beyond them is granted again on every call)
    static std::atomic<unsigned long long> granted{0};
    const unsigned long long bit = ctx->device < 64 ? 1ull << ctx->device : 0ull;
    if (!(granted.load() & bit)) {
        const size_t most = rows16_lds_bytes(rows16_qb(KR), KR == 1 ? PQH_SEARCH_MAX_K : PQH_SEARCH_MAX_K_WIDE);
        PQH_HIP(ctx, hipFuncSetAttribute((const void*)fn,
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)most));
        granted.fetch_or(bit);
    }
    hipLaunchKernelGGL(fn, dim3((unsigned)units, (unsigned)groups), dim3(64, kWaves), lds,
                       ctx->stream, a);
    PQH_LAUNCH_CHECK(ctx);
    return PQH_OK;
}

template <typename T>
int rows16_dispatch(bool ip, bool wide, pqh_ctx* ctx, const Rows16Args& a, long long units, int groups) {
    return ip ? (wide ? rows16_launch<T, true, kWideKR>(ctx, a, units, groups)
                      : rows16_launch<T, true, 1>(ctx, a, units, groups))
              : (wide ? rows16_launch<T, false, kWideKR>(ctx, a, units, groups)
                      : rows16_launch<T, false, 1>(ctx, a, units, groups));
}

// pqh_flat_search_lists' checks in its order, then the plan, the scan and the merge
int rows16_search(bool ip, pqh_ctx_t* ctx, const void* d_x, int rows, long long n, long long ld_x,
                  int d, const long long* d_offsets, long long nlist, const long long* d_probes,
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
    const int qb = rows16_qb(wide ? kWideKR : 1);
    const long long npairs = nq * nprobe;
    const long long bound = std::min<long long>(npairs, nlist + npairs / qb);
    const long long groups = lists_groups(ctx, n, nlist, bound, kTile);

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

    Rows16Args a{};
    a.x = static_cast<const unsigned short*>(d_x), a.ld_x = ld_x, a.d = d, a.nprobe = nprobe;
    a.offsets = d_offsets, a.units = lp.units, a.nunits = lp.nunits, a.pairs = lp.pairs;
    a.q = d_queries, a.ld_q = ld_q, a.k = top_k, a.keep = d_keep_bits;
    a.words = ld_x % 2 == 0 && (reinterpret_cast<uintptr_t>(d_x) & 3u) == 0;
    a.part_d = part_d, a.part_id = part_id;
    rc = rows == PQH_ROWS_F16 ? rows16_dispatch<_Float16>(ip, wide, ctx, a, bound, (int)groups)
                              : rows16_dispatch<__bf16>(ip, wide, ctx, a, bound, (int)groups);
    if (rc) return rc;
    return pqh_lists_merge_launch(ctx, part_d, part_id, nprobe * groups, nq, top_k, id_base, d_dist, d_ids);
}

}  // namespace

extern "C" {

int pqh_flat_search_lists_rows(pqh_ctx_t* ctx, const void* d_x, int rows, long long n,
                               long long ld_x, int d, const long long* d_offsets, long long nlist,
                               const long long* d_probes, const float* d_queries, long long nq,
                               long long ld_q, int nprobe, int top_k,
                               const unsigned int* d_keep_bits, long long id_base, float* d_dist,
                               long long* d_ids) {
    if (!pqh_rows_ok(rows, d_x)) return PQH_ERR_ARG;
    if (rows == PQH_ROWS_F32)
        return pqh_flat_search_lists(ctx, static_cast<const float*>(d_x), n, ld_x, d, d_offsets, nlist,
                                     d_probes, d_queries, nq, ld_q, nprobe, top_k, d_keep_bits,
                                     id_base, d_dist, d_ids);
    return rows16_search(false, ctx, d_x, rows, n, ld_x, d, d_offsets, nlist, d_probes, d_queries, nq,
                         ld_q, nprobe, top_k, d_keep_bits, id_base, d_dist, d_ids);
}

int pqh_flat_search_lists_rows_ip(pqh_ctx_t* ctx, const void* d_x, int rows, long long n,
                                  long long ld_x, int d, const long long* d_offsets,
                                  long long nlist, const long long* d_probes,
                                  const float* d_queries, long long nq, long long ld_q, int nprobe,
                                  int top_k, const unsigned int* d_keep_bits, long long id_base,
                                  float* d_dist, long long* d_ids) {
    if (!pqh_rows_ok(rows, d_x)) return PQH_ERR_ARG;
    if (rows == PQH_ROWS_F32)
        return pqh_flat_search_lists_ip(ctx, static_cast<const float*>(d_x), n, ld_x, d, d_offsets,
                                        nlist, d_probes, d_queries, nq, ld_q, nprobe, top_k,
                                        d_keep_bits, id_base, d_dist, d_ids);
    return rows16_search(true, ctx, d_x, rows, n, ld_x, d, d_offsets, nlist, d_probes, d_queries, nq,
                         ld_q, nprobe, top_k, d_keep_bits, id_base, d_dist, d_ids);
}

}  // extern "C"
