// pqh_rerank.hip -- the exact re-rank of a search's candidates against stored rows (DESIGN.md
// 4.5.21): pqh_rerank_rows / _ip over fp32, fp16 or bf16 rows, pqh_rerank_sq / _ip over SQ8
// codes.  The distance of a (query, candidate) pair is the definition's chain (chain_step of
// pqh_flat_dev.h) over the stored row -- an fp32 value itself, a 16-bit value converted exactly,
// an SQ8 code decoded as vmin[j] + code * step[j] -- j ascending in one accumulator: the bits
// pqh_flat_search and pqh_flat_search_lists return for that pair.
//
//  rerank_rows<Row, IP, WIDE>  one workgroup per query, ceil(ncand / 64) waves (one, or up to
//                four in the wide form), wave w the candidates [64 w, 64 w + 64).
//                Gather: a row is taken in segments of 128 bytes (32 floats, 64 16-bit values,
//                128 codes).  Eight consecutive lanes take one row's segment as eight 16-byte
//                loads, so a load instruction of the wave covers 8 rows in whole 128-byte runs,
//                and eight such loads a lane (32 registers) hold the wave's 64 rows of the
//                segment.  The 16-byte form needs rows and base on 4 bytes; a lane whose 16 bytes
//                cross d reads the dwords that begin below d; rows off 4 bytes are read element
//                by element, those below d only.  Lanes of padded, invalid or absent candidates
//                load nothing.  The loads of segment s + 1 are issued before the arithmetic of
//                segment s.
//                LDS: the wave stores the segment as raw bytes into a tile of its own,
//                [64 rows][33 dwords] (8,448 B; the odd pitch puts a dword column of 64 rows in
//                64 distinct banks).  A wave reads only what it stored: the segment loop has no
//                workgroup barrier, only the wave's own wait for its stores.
//                Chain: lane = candidate; per dword of its tile row one LDS read, the conversion
//                and one, two or four chain steps.  The loop stops at d: what a last dword holds
//                past d is never converted.  The query values (and vmin, step) are read from
//                global memory at wave-uniform addresses, which the compiler turns into scalar
//                loads (s_load_dwordx4 / x8 in the object).
//                Select: ncand <= 64 sorts the wave's keys by list_merge on an empty list; the
//                wide form leaves the keys in the waves' tiles and wave 0 sorts them through the
//                wide list after one barrier (refine_rows_wide's end, restated).
#include <type_traits>

#include "pqh_flat_dev.h"
#include "pqh_internal.h"
#include "pqh_topk_dev.h"

namespace {

constexpr int kSegBytes = 128;              // bytes of a row a segment
constexpr int kPitch = kSegBytes / 4 + 1;   // dwords between two rows of a tile: odd
constexpr int kLoads = 8;                   // 16-byte loads a lane and segment: 8 rows each
constexpr int kMaxWaves = PQH_SEARCH_MAX_K_WIDE / 64;
static_assert(kMaxWaves == kWideKR, "the wide list holds the candidates of every wave");
static_assert(64 * 4 + 64 * 8 <= 64 * kPitch * 4, "a wave's keys fit its tile");

struct __attribute__((aligned(4))) Quad16 {   // 16 bytes of a row that lie on 4 bytes
    unsigned w[4];
};

struct Sq8 {};   // the row type of SQ8 codes: a byte an element, decoded by vmin and step

template <typename Row>
struct RowBits {
    using type = std::conditional_t<std::is_same_v<Row, float>, unsigned,
                                    std::conditional_t<std::is_same_v<Row, Sq8>, unsigned char, unsigned short>>;
};

// pqh_sq.hip's decode, restated: one multiply, one add, each rounded
__device__ __forceinline__ float rr_dec(unsigned w, int b, float vmin, float step) {
    const float code = (float)((w >> (8 * b)) & 0xFFu);   // v_cvt_f32_ubyte0..3
    return vmin + code * step;
}

// the chain steps of the first `cnt` elements of dword w, the elements j, j + 1, ... of the row
template <typename Row, bool IP, int CNT>
__device__ __forceinline__ void dword_steps(float& acc, unsigned w, int j, const float* __restrict__ q,
                                            const float* __restrict__ vmin,
                                            const float* __restrict__ step) {
    if constexpr (std::is_same_v<Row, float>) {
        chain_step<IP>(acc, q[j], __uint_as_float(w));
    } else if constexpr (std::is_same_v<Row, Sq8>) {
#pragma unroll
        for (int b = 0; b < CNT; ++b) chain_step<IP>(acc, q[j + b], rr_dec(w, b, vmin[j + b], step[j + b]));
    } else {
        chain_step<IP>(acc, q[j], half_lo<Row>(w));
        if constexpr (CNT > 1) chain_step<IP>(acc, q[j + 1], half_hi<Row>(w));
    }
}

template <typename Row, bool IP, bool WIDE>
__global__ void __launch_bounds__(WIDE ? 64 * kMaxWaves : 64)
rerank_rows(const typename RowBits<Row>::type* __restrict__ x, long long n, long long ld_x, int d,
            int vec, const float* __restrict__ vmin, const float* __restrict__ step,
            const float* __restrict__ queries, long long ld_q, const long long* __restrict__ cand,
            int ncand, int top_k, float* __restrict__ dist, long long* __restrict__ ids,
            long long ld_out, unsigned long long* __restrict__ err) {
    using Bits = typename RowBits<Row>::type;
    constexpr int kSize = (int)sizeof(Bits);
    constexpr int kPer = 4 / kSize;            // elements a dword
    constexpr int kPer16 = 16 / kSize;         // elements a 16-byte load
    constexpr int kSegE = kSegBytes / kSize;   // elements a segment
    constexpr int kUnroll = std::is_same_v<Row, Sq8> ? 4 : 8;   // dwords whose scalars are in flight
    __shared__ unsigned tiles[WIDE ? kMaxWaves : 1][64 * kPitch];
    const int lane = threadIdx.x & 63;
    const int w = WIDE ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : 0;
    unsigned* const tile = tiles[w];
    const long long q = blockIdx.x;
    const float* __restrict__ qrow = queries + q * ld_q;

    const int c = w * 64 + lane;
    const long long v = c < ncand ? cand[q * ncand + c] : -1ll;
    const bool valid = v >= 0 && v < n;
    if (v < -1 || v >= n) atomicOr(err, 1ull);

    // the rows this lane loads from: row 8 i + lane / 8 of the wave, its first element (-1: none)
    const long long mine = valid ? v * ld_x : -1ll;
    long long roff[kLoads];
#pragma unroll
    for (int i = 0; i < kLoads; ++i) roff[i] = __shfl(mine, 8 * i + (lane >> 3));
    const int piece = lane & 7, trow = lane >> 3;

    // A segment that lies below d as a whole is read 16 bytes a lane (WHOLE); the last one of a
    // ragged d by the dwords that begin below d.  Two texts, chosen per segment by the wave: as
    // two sides of one branch the compiler hoists dword 0 out of the 16-byte load.
    unsigned pre[kLoads][4];
    auto fetch_as = [&](auto whole, int s) __attribute__((always_inline)) {
        constexpr bool WHOLE = decltype(whole)::value;
        const int e0 = s * kSegE + kPer16 * piece;   // the first element of this lane's 16 bytes
#pragma unroll
        for (int i = 0; i < kLoads; ++i) {
            pre[i][0] = pre[i][1] = pre[i][2] = pre[i][3] = 0u;
            if (roff[i] < 0 || (!WHOLE && e0 >= d)) continue;
            const Bits* src = x + roff[i] + e0;
            if (kSize == 4 || vec) {
                if constexpr (WHOLE) {
                    const Quad16 t = *reinterpret_cast<const Quad16*>(src);
                    pre[i][0] = t.w[0], pre[i][1] = t.w[1], pre[i][2] = t.w[2], pre[i][3] = t.w[3];
                } else {   // (a dword that begins below d ends inside the row)
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (e0 + kPer * k < d) pre[i][k] = *reinterpret_cast<const unsigned*>(src + kPer * k);
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int b = 0; b < kPer; ++b)
                        if (WHOLE || e0 + kPer * k + b < d)
                            pre[i][k] |= (unsigned)src[kPer * k + b] << (8 * kSize * b);
            }
        }
    };
    auto fetch = [&](int s) __attribute__((always_inline)) {
        if ((s + 1) * kSegE <= d) fetch_as(std::true_type{}, s);
        else fetch_as(std::false_type{}, s);
    };
    auto stash = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < kLoads; ++i) {
            unsigned* dst = tile + (8 * i + trow) * kPitch + 4 * piece;
            dst[0] = pre[i][0], dst[1] = pre[i][1], dst[2] = pre[i][2], dst[3] = pre[i][3];
        }
    };

    const int ns = (d + kSegE - 1) / kSegE;
    const unsigned* const mrow = tile + lane * kPitch;
    float acc = 0.f;
    fetch(0);
    stash();
#pragma unroll 1
    for (int s = 0; s < ns; ++s) {
        if (s + 1 < ns) fetch(s + 1);
        // the wave's own stores before its reads of other lanes' dwords: lds_barrier's wait
        // without the s_barrier, since no other wave touches this tile
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const int j0 = s * kSegE;
        const int ne = min(kSegE, d - j0);
        if (ne == kSegE) {
#pragma unroll kUnroll
            for (int k = 0; k < kSegBytes / 4; ++k)
                dword_steps<Row, IP, kPer>(acc, mrow[k], j0 + kPer * k, qrow, vmin, step);
        } else {   // the last segment: whole dwords, then the elements of one more below d
            const int nfull = ne / kPer;
#pragma unroll 4
            for (int k = 0; k < nfull; ++k)
                dword_steps<Row, IP, kPer>(acc, mrow[k], j0 + kPer * k, qrow, vmin, step);
            if constexpr (kPer > 1) {
                const int rest = ne - nfull * kPer, j = j0 + kPer * nfull;
                const unsigned last = mrow[nfull];
                if (rest == 1) dword_steps<Row, IP, 1>(acc, last, j, qrow, vmin, step);
                if constexpr (kPer == 4) {
                    if (rest == 2) dword_steps<Row, IP, 2>(acc, last, j, qrow, vmin, step);
                    if (rest == 3) dword_steps<Row, IP, 3>(acc, last, j, qrow, vmin, step);
                }
            }
        }
        if (s + 1 < ns) stash();   // (after this wave's reads of segment s, in program order)
    }

    const TopK key = valid ? TopK{acc, v} : TopK{INFINITY, 0x7FFFFFFFFFFFFFFFll};
    if constexpr (!WIDE) {
        // ---- select: the wave's 64 keys sorted by (dist, id)
        TopK e{INFINITY, -1};
        list_merge<false>(e, key);
        if (lane < top_k) {
            dist[q * ld_out + lane] = e.d;
            ids[q * ld_out + lane] = e.id;
        }
    } else {
        // ---- select: the waves' keys from their tiles, 64 at a time, into the wide list
        reinterpret_cast<float*>(tile)[lane] = key.d;
        reinterpret_cast<long long*>(tile + 64)[lane] = key.id;
        lds_barrier();
        if (w) return;
        const int kth = ncand - 1;
        TopKW e;
        list_clear(e);
#pragma unroll 1
        for (int b = 0; b <= (kth >> 6); ++b)
            list_merge<false>(e, TopK{reinterpret_cast<const float*>(tiles[b])[lane],
                                      reinterpret_cast<const long long*>(tiles[b] + 64)[lane]}, kth);
#pragma unroll
        for (int b = 0; b < kWideKR; ++b) {
            if (b * 64 + lane < top_k) {
                dist[q * ld_out + b * 64 + lane] = e.d[b];
                ids[q * ld_out + b * 64 + lane] = e.id[b];
            }
        }
    }
}

struct RerankArgs {
    const void* x;
    long long n, ld_x;
    int d;
    const float* vmin;
    const float* step;
    const float* queries;
    long long nq, ld_q;
    const long long* cand;
    int ncand, top_k;
    float* dist;
    long long* ids;
    long long ld_out;
};

template <typename Row, bool IP>
int rerank_launch(pqh_ctx* ctx, const RerankArgs& a) {
    using Bits = typename RowBits<Row>::type;
    const bool wide = a.ncand > PQH_SEARCH_MAX_K;
    // the 16-byte loads: rows and base on 4 bytes (fp32 rows always are)
    const int vec = (a.ld_x * (long long)sizeof(Bits)) % 4 == 0 && (reinterpret_cast<uintptr_t>(a.x) & 3u) == 0;
    const dim3 block(64 * ((a.ncand + 63) / 64));
    // (a name with a comma in it is two arguments to the launch macro: the parentheses)
    hipLaunchKernelGGL((wide ? rerank_rows<Row, IP, true> : rerank_rows<Row, IP, false>),
                       dim3((unsigned)a.nq), block, 0, ctx->stream, static_cast<const Bits*>(a.x),
                       a.n, a.ld_x, a.d, vec, a.vmin, a.step, a.queries, a.ld_q, a.cand, a.ncand,
                       a.top_k, a.dist, a.ids, a.ld_out, ctx->d_diag + kDiagIvf);
    PQH_LAUNCH_CHECK(ctx);
    return PQH_OK;
}

// rows: PQH_ROWS_*, or -1 for SQ8 codes
int rerank(bool ip, pqh_ctx_t* ctx, int rows, const RerankArgs& a) {
    // what is wrong whatever the context
    if (a.n < 0 || a.d < 1 || a.ld_x < a.d || a.nq < 0 || a.ld_q < a.d || a.ncand < 1 ||
        a.ncand > PQH_SEARCH_MAX_K_WIDE || a.top_k < 1 || a.top_k > a.ncand || a.ld_out < a.top_k)
        return PQH_ERR_ARG;
    if (a.nq > 0 && (!a.queries || !a.cand || !a.dist || !a.ids ||
                     (a.n > 0 && (!a.x || (rows < 0 && (!a.vmin || !a.step))))))
        return PQH_ERR_ARG;
    if (!ctx) return pqh_no_ctx_status();
    if (a.ncand > ctx->search_max_k) return PQH_ERR_ARG;
    if (a.nq > 0x7FFFFFFFll || a.n > 0x7FFFFFFFFFFFFFFFll / a.ld_x) return PQH_ERR_UNSUPPORTED;
    const int rc = pqh_use_device(ctx);
    if (rc) return rc;
    if (a.nq == 0) return PQH_OK;
    // (n == 0 launches too: every candidate but -1 is reported, every result is padding)
    switch (rows) {
        case PQH_ROWS_F32: return ip ? rerank_launch<float, true>(ctx, a) : rerank_launch<float, false>(ctx, a);
        case PQH_ROWS_F16: return ip ? rerank_launch<_Float16, true>(ctx, a) : rerank_launch<_Float16, false>(ctx, a);
        case PQH_ROWS_BF16: return ip ? rerank_launch<__bf16, true>(ctx, a) : rerank_launch<__bf16, false>(ctx, a);
        default: return ip ? rerank_launch<Sq8, true>(ctx, a) : rerank_launch<Sq8, false>(ctx, a);
    }
}

}  // namespace

extern "C" {

int pqh_rerank_rows(pqh_ctx_t* ctx, const void* d_x, int rows, long long n, long long ld_x, int d,
                    const float* d_queries, long long nq, long long ld_q, const long long* d_cand,
                    int ncand, int top_k, float* d_dist, long long* d_ids, long long ld_out) {
    if (!pqh_rows_ok(rows, d_x)) return PQH_ERR_ARG;
    return rerank(false, ctx, rows, RerankArgs{d_x, n, ld_x, d, nullptr, nullptr, d_queries, nq, ld_q,
                                               d_cand, ncand, top_k, d_dist, d_ids, ld_out});
}

int pqh_rerank_rows_ip(pqh_ctx_t* ctx, const void* d_x, int rows, long long n, long long ld_x,
                       int d, const float* d_queries, long long nq, long long ld_q,
                       const long long* d_cand, int ncand, int top_k, float* d_dist,
                       long long* d_ids, long long ld_out) {
    if (!pqh_rows_ok(rows, d_x)) return PQH_ERR_ARG;
    return rerank(true, ctx, rows, RerankArgs{d_x, n, ld_x, d, nullptr, nullptr, d_queries, nq, ld_q,
                                              d_cand, ncand, top_k, d_dist, d_ids, ld_out});
}

int pqh_rerank_sq(pqh_ctx_t* ctx, const unsigned char* d_codes, long long n, long long ld_c, int d,
                  const float* d_vmin, const float* d_step, const float* d_queries, long long nq,
                  long long ld_q, const long long* d_cand, int ncand, int top_k, float* d_dist,
                  long long* d_ids, long long ld_out) {
    return rerank(false, ctx, -1, RerankArgs{d_codes, n, ld_c, d, d_vmin, d_step, d_queries, nq, ld_q,
                                             d_cand, ncand, top_k, d_dist, d_ids, ld_out});
}

int pqh_rerank_sq_ip(pqh_ctx_t* ctx, const unsigned char* d_codes, long long n, long long ld_c,
                     int d, const float* d_vmin, const float* d_step, const float* d_queries,
                     long long nq, long long ld_q, const long long* d_cand, int ncand, int top_k,
                     float* d_dist, long long* d_ids, long long ld_out) {
    return rerank(true, ctx, -1, RerankArgs{d_codes, n, ld_c, d, d_vmin, d_step, d_queries, nq, ld_q,
                                            d_cand, ncand, top_k, d_dist, d_ids, ld_out});
}

}  // extern "C"
