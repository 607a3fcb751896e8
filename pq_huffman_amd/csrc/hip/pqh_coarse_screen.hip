// pqh_coarse_screen.hip -- the coarse assignment through a bf16-split MFMA screen and an exact
// finish: what coarse_assign<IP> (pqh_ivf.hip) computes, list and distance bit for bit, at a
// fraction of its 3 * n * nlist * d lane operations.
//
//  screen_frags / screen_norms  the prepared centroids, once per quantizer: -c split into two
//                 bf16 halves (c = ch + cl + r) in the A-operand order of
//                 v_mfma_f32_32x32x16_bf16, [tile of 32 lists][half][pass of 16 dims][lane],
//                 d padded with zero slots and nlist with zero rows; ||c||^2 in fp32 (from a
//                 double sum) for L2, 0 for the inner product, +inf in the padded slots, so a
//                 padded slot never wins; and Cmax = max ||c||^2.
//  coarse_screen<IP, BLDS>  a wave owns 32 rows, the MFMA's B operand: 2x (L2) or x (IP) as
//                 xh | xl, the two bf16 halves.  REG form (d <= 128): a workgroup of four waves
//                 owns 128 rows, every wave holds its B fragments in registers (32 VGPRs per
//                 half at d = 128), and the tiles of 32 centroids stream through a double
//                 buffer in LDS, loaded once per workgroup, the global read of a tile
//                 overlapping the MFMAs of the one before: one barrier per tile.  BLDS form
//                 (d <= 1024): the B fragments live in LDS (2 KB per wave and pass), the
//                 workgroup has two waves (one above d = 512) and the waves read the A
//                 fragments from L2 themselves, no barrier in the loop.
//                 Score of a list: S = ||c||^2 - 2 x.c (the accumulator starts at ||c||^2), or
//                 S = -x.c; passes xh.ch, xh.cl and, when some x of the wave is not bf16-exact,
//                 xl.ch.
//                 Selection: a lane reduces its 16 scores of a tile to one minimum and walks
//                 them only where that minimum is at or below its running best + tau; the walk
//                 appends (score, list) pairs at or below best + tau to the lane's own
//                 candidate list in LDS (16 entries; full: the entries above the bound, which
//                 has fallen since, are dropped; still full: the row overflows).  The running
//                 best only falls, so the candidates at or below the final best + tau hold
//                 every list that can be the fp32 argmin or tie with it (tau: DESIGN.md).
//                 Finish, same kernel: one candidate and no d_dist -- the list is stored; else
//                 the definition's chain for every candidate, the smallest by (dist, list).
//                 A row that overflowed, or whose tau is not below 2^110 (a non-finite x or
//                 centroid, or scores that may have overflowed), takes the chain over all
//                 lists, lane = list, with coarse_assign's own rule for what `<` rejects.
#include <cmath>
#include <cstring>

#include "pqh_internal.h"
#include "pqh_screen_dev.h"

namespace {

constexpr int kRegPasses = 8;      // REG: d <= 128, the B fragments in 64 VGPRs
constexpr int kLdsPasses = 64;     // BLDS: d <= 1024, 128 KB of B fragments for one wave
constexpr int kLdsPasses2 = 32;    // BLDS with two waves: d <= 512
constexpr int kDiagRerank = 9, kDiagFallback = 10;   // pqh_ctx::d_diag slots of the counts

// the image of a quantizer: [nt][2][P][64] u32x4 fragments, [2][nlistP] floats (the accumulator
// start per metric), Cmax
struct Image {
    const u32x4* frag;
    float* cn;
    unsigned* cmax;
    int P, nt;
};
size_t image_frag_bytes(int nt, int P) { return (size_t)nt * 2 * P * 64 * 16; }
Image image_of(void* base, int nlist, int d) {
    Image im;
    im.P = (d + 15) / 16;
    im.nt = (nlist + 31) / 32;
    char* b = static_cast<char*>(base);
    im.frag = reinterpret_cast<const u32x4*>(b);
    im.cn = reinterpret_cast<float*>(b + image_frag_bytes(im.nt, im.P));
    im.cmax = reinterpret_cast<unsigned*>(im.cn + (size_t)2 * im.nt * 32);
    return im;
}

__global__ void __launch_bounds__(64)
screen_frags(const float* __restrict__ cent, int nlist, int d, int P, u32x4* __restrict__ frag,
             unsigned* __restrict__ cmax) {
    const int t = blockIdx.x, p = blockIdx.y, lane = threadIdx.x;
    const int row = 32 * t + (lane & 31), j0 = 16 * p + 8 * (lane >> 5);
    bf16x8 hi, lo;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float c = 0.f;
        if (row < nlist && j0 + j < d) c = -cent[(long long)row * d + j0 + j];
        const __bf16 h = (__bf16)c;
        hi[j] = h;
        lo[j] = (__bf16)(c - (float)h);
    }
    frag[((size_t)(t * 2 + 0) * P + p) * 64 + lane] = __builtin_bit_cast(u32x4, hi);
    frag[((size_t)(t * 2 + 1) * P + p) * 64 + lane] = __builtin_bit_cast(u32x4, lo);
    if (t == 0 && p == 0 && lane == 0) *cmax = 0u;   // screen_norms, the next launch, raises it
}

// non-negative floats order as their bits, and a NaN's bits lie above +inf's: a non-finite
// centroid leaves a Cmax that fails every row's tau test
__global__ void __launch_bounds__(256)
screen_norms(const float* __restrict__ cent, int nlist, int nlistP, int d, float* __restrict__ cn,
             unsigned* __restrict__ cmax) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= nlistP) return;
    float l2 = INFINITY, ip = INFINITY;
    if (l < nlist) {
        double s = 0.0;
        for (int j = 0; j < d; ++j) {
            const double c = cent[(long long)l * d + j];
            s += c * c;
        }
        l2 = (float)s;
        ip = 0.f;
        atomicMax(cmax, __float_as_uint(l2));
    }
    cn[l] = l2;
    cn[nlistP + l] = ip;
}

__global__ void screen_clear(unsigned long long* counts) {
    counts[kDiagRerank] = 0;
    counts[kDiagFallback] = 0;
}

// the definition's chain, c's elements cs floats apart
template <bool IP>
__device__ __forceinline__ float exact_chain(const float* __restrict__ x,
                                             const float* __restrict__ c, long long cs, int d) {
    float acc = 0.f;
#pragma unroll 4
    for (int j = 0; j < d; ++j) {
        if constexpr (IP) {
            acc = acc - x[j] * c[j * cs];
        } else {
            const float t = x[j] - c[j * cs];
            acc = acc + t * t;
        }
    }
    return acc;
}

// eight x values of a row from dimension j0 on (zeros from d on)
__device__ __forceinline__ void load8(const float* __restrict__ xr, int j0, int d, bool vec,
                                      float* v) {
    if (vec) {   // d % 16 == 0 and every row on 16 bytes: j0 + 8 <= d
        const float4 a = *reinterpret_cast<const float4*>(xr + j0);
        const float4 b = *reinterpret_cast<const float4*>(xr + j0 + 4);
        v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
        v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = j0 + e < d ? xr[j0 + e] : 0.f;
    }
}

template <bool IP, bool BLDS>
__global__ void __launch_bounds__(256, BLDS ? 1 : 2)
coarse_screen(const float* __restrict__ x, long long n, long long ld_x,
              const float* __restrict__ cent, const float* __restrict__ cent_t, int nlist, int d,
              int P, int nt, const u32x4* __restrict__ frag, const float* __restrict__ cn,
              const unsigned* __restrict__ cmax_p, float kq, int vec, int32_t* __restrict__ list,
              float* __restrict__ dist, unsigned long long* __restrict__ counts) {
    extern __shared__ u32x4 smem[];
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5;
    const long long row = (long long)blockIdx.x * (nthr >> 1) + wave * 32 + (lane & 31);
    const bool valid = row < n;
    const float* __restrict__ xr = x + (valid ? row : n - 1) * ld_x;

    Cands cd;
    cd.s = reinterpret_cast<float*>(smem);
    cd.l = reinterpret_cast<int*>(cd.s + kCand * nthr);
    cd.nthr = nthr, cd.tid = tid, cd.cnt = 0, cd.ovf = false;
    u32x4* const rest = smem + (kCand * nthr * 8) / 16;
    // REG: two tile buffers of 2 P fragments-of-a-wave and 32 accumulator starts each
    const int tile_u4 = 2 * P * 64 + 8;
    // BLDS: this wave's B fragments [2][P][64]
    u32x4* const bst = rest + (size_t)wave * 2 * P * 64;

    // ---- the wave's B operand, ||x||^2 and whether the lo pass is needed
    bf16x8 Bh[BLDS ? 1 : kRegPasses], Bl[BLDS ? 1 : kRegPasses];
    float X = 0.f;
    unsigned low = 0u;
    auto make_pass = [&](int p, bf16x8& bh, bf16x8& bl) {
        float v[8];
        load8(xr, 16 * p + 8 * h, d, vec != 0, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            X = X + v[e] * v[e];
            const float s = IP ? v[e] : 2.f * v[e];
            const __bf16 hb = (__bf16)s;
            bh[e] = hb;
            bl[e] = (__bf16)(s - (float)hb);
            low |= __float_as_uint(s) & 0xFFFFu;
        }
    };
    if constexpr (BLDS) {
#pragma unroll 1
        for (int p = 0; p < P; ++p) {
            bf16x8 bh, bl;
            make_pass(p, bh, bl);
            bst[p * 64 + lane] = __builtin_bit_cast(u32x4, bh);
            bst[(P + p) * 64 + lane] = __builtin_bit_cast(u32x4, bl);
        }
    } else {
#pragma unroll
        for (int p = 0; p < kRegPasses; ++p)
            if (p < P) make_pass(p, Bh[p], Bl[p]);
    }
    X = X + __shfl_xor(X, 32);
    const bool any_lo = __ballot(low != 0u) != 0ull;
    // tau: DESIGN.md 4.5.16.  Not below 2^110 (NaN included): the all-lists path
    const float tau = kq * (X + __uint_as_float(*cmax_p)) + 0x1p-100f;
    bool fb = !(tau < 0x1p110f);
    float best = INFINITY;

    // ---- the tiles
    const int st = 2 * P * 64;   // u32x4s of a tile's fragments
    auto scores = [&](const u32x4* a, const float* cnp) {
        f32x16 acc;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 c4 = *reinterpret_cast<const f32x4*>(cnp + 8 * q + 4 * h);
            acc[4 * q] = c4[0], acc[4 * q + 1] = c4[1], acc[4 * q + 2] = c4[2],
                    acc[4 * q + 3] = c4[3];
        }
        auto pass = [&](int p, const bf16x8& bh, const bf16x8& bl) {
            const bf16x8 ah = __builtin_bit_cast(bf16x8, a[p * 64 + lane]);
            const bf16x8 al = __builtin_bit_cast(bf16x8, a[(P + p) * 64 + lane]);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
            if (any_lo) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
        };
        if constexpr (BLDS) {
#pragma unroll 1
            for (int p = 0; p < P; ++p)
                pass(p, __builtin_bit_cast(bf16x8, bst[p * 64 + lane]),
                     __builtin_bit_cast(bf16x8, bst[(P + p) * 64 + lane]));
        } else {
#pragma unroll
            for (int p = 0; p < kRegPasses; ++p)
                if (p < P) pass(p, Bh[p], Bl[p]);
        }
        return acc;
    };
    auto select = [&](const f32x16& acc, int t) {
        float m = fmin2(acc[0], acc[1]);
#pragma unroll
        for (int i = 2; i < 16; i += 2) m = fmin2(m, fmin2(acc[i], acc[i + 1]));
        if (!fb && m <= best + tau) {
            best = fmin2(best, m);
            const float thr = best + tau;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int l = 32 * t + (i & 3) + 8 * (i >> 2) + 4 * h;
                if (acc[i] <= thr && l < nlist) cd.append(acc[i], l, thr);
            }
        }
    };

    if constexpr (BLDS) {
#pragma unroll 1
        for (int t = 0; t < nt; ++t)
            select(scores(frag + (size_t)t * st, cn + 32 * t), t);
    } else {
        // thread tid moves u32x4 tid + 256 k of a tile (k < P / 2, rounded up), thread k < 32
        // its accumulator start
        u32x4 pre[kRegPasses / 2];
        float pre_cn = 0.f;
        auto fetch = [&](int t) {
            const u32x4* src = frag + (size_t)t * st;
#pragma unroll
            for (int k = 0; k < kRegPasses / 2; ++k)
                pre[k] = src[min(k * 256 + tid, st - 1)];   // (no branch around a load)
            pre_cn = cn[32 * t + (tid & 31)];
        };
        auto stash = [&](u32x4* dst) {
#pragma unroll
            for (int k = 0; k < kRegPasses / 2; ++k)
                if (k * 256 + tid < st) dst[k * 256 + tid] = pre[k];
            if (tid < 32) reinterpret_cast<float*>(dst + st)[tid] = pre_cn;
        };
        fetch(0);
        stash(rest);
        lds_barrier();
#pragma unroll 1
        for (int t = 0; t < nt; ++t) {
            const u32x4* cur = rest + (t & 1) * tile_u4;
            if (t + 1 < nt) fetch(t + 1);
            select(scores(cur, reinterpret_cast<const float*>(cur + st)), t);
            // the other buffer was last read before the barrier that ended tile t - 1
            if (t + 1 < nt) stash(rest + ((t + 1) & 1) * tile_u4);
            lds_barrier();
        }
    }

    // ---- the finish.  The two lanes of a row (lane, lane ^ 32) hold its two candidate lists
    best = fmin2(best, __shfl_xor(best, 32));
    const float thr = best + tau;
    cd.prune(thr);
    const int total = cd.cnt + __shfl_xor(cd.cnt, 32);
    fb = fb || cd.ovf || __shfl_xor((int)cd.ovf, 32) != 0;
    if (valid && !fb && total == 1 && cd.cnt == 1) {
        const int L = cd.l[tid];
        list[row] = L;
        if (dist) dist[row] = exact_chain<IP>(xr, cent + (long long)L * d, 1, d);
    }
    const long long wrow0 = row - (lane & 31);
    unsigned long long rr = __ballot(valid && !fb && total > 1 && h == 0);
    unsigned long long fa = __ballot(valid && fb && h == 0);
    if (lane == 0) {
        if (rr) atomicAdd(counts + kDiagRerank, (unsigned long long)__popcll(rr));
        if (fa) atomicAdd(counts + kDiagFallback, (unsigned long long)__popcll(fa));
    }
    // a row with several candidates: lane = candidate (at most 2 kCand <= 64)
    while (rr) {
        const int r = __builtin_ctzll(rr);
        rr &= rr - 1;
        const int c0 = __shfl(cd.cnt, r), c1 = __shfl(cd.cnt, r + 32);
        const float* __restrict__ xw = x + (wrow0 + r) * ld_x;
        float bd = INFINITY;
        int bi = 0x7FFFFFFF;
        if (lane < c0 + c1) {
            const int src = (tid - lane) + (lane < c0 ? r : r + 32);
            bi = cd.l[(lane < c0 ? lane : lane - c0) * nthr + src];
            bd = exact_chain<IP>(xw, cent + (long long)bi * d, 1, d);
        }
        wave_first_min(bd, bi);
        if (lane == 0) {
            list[wrow0 + r] = bi;
            if (dist) dist[wrow0 + r] = bd;
        }
    }
    // the all-lists path: lane = list, coarse_assign's strict `<` from (+inf, 0)
    while (fa) {
        const int r = __builtin_ctzll(fa);
        fa &= fa - 1;
        const float* __restrict__ xw = x + (wrow0 + r) * ld_x;
        float bd = INFINITY;
        int bi = 0;
#pragma unroll 1
        for (int l = lane; l < nlist; l += 64) {
            const float a = exact_chain<IP>(xw, cent_t + l, nlist, d);
            if (a < bd) bd = a, bi = l;
        }
        wave_first_min(bd, bi);
        if (lane == 0) {
            list[wrow0 + r] = bi;
            if (dist) dist[wrow0 + r] = bd;
        }
    }
}

int screen_prepare(pqh_ctx* ctx, pqh_coarse* cq) {
    if (cq->d_screen) return PQH_OK;
    const int P = (cq->d + 15) / 16, nt = (cq->nlist + 31) / 32;
    const size_t bytes = image_frag_bytes(nt, P) + (size_t)2 * nt * 32 * 4 + 256;
    void* base = nullptr;
    if (hipMalloc(&base, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return pqh_set_error(ctx, PQH_ERR_NOMEM, "coarse screen: cannot allocate %zu bytes", bytes);
    }
    const Image im = image_of(base, cq->nlist, cq->d);
    hipLaunchKernelGGL(screen_frags, dim3((unsigned)nt, (unsigned)P), dim3(64), 0, ctx->stream,
                       cq->d_cent, cq->nlist, cq->d, P, const_cast<u32x4*>(im.frag), im.cmax);
    hipLaunchKernelGGL(screen_norms, dim3((unsigned)((nt * 32 + 255) / 256)), dim3(256), 0,
                       ctx->stream, cq->d_cent, cq->nlist, nt * 32, cq->d, im.cn, im.cmax);
    if (hipGetLastError() != hipSuccess) {
        (void)hipFree(base);
        return pqh_set_error(ctx, PQH_ERR_HIP, "coarse screen: the centroid image launch failed");
    }
    cq->d_screen = base;
    return PQH_OK;
}

template <bool IP, bool BLDS>
int screen_launch(pqh_ctx* ctx, const pqh_coarse* cq, const float* d_x, long long n, long long ld_x,
                  int32_t* d_list, float* d_dist) {
    const Image im = image_of(cq->d_screen, cq->nlist, cq->d);
    const int waves = !BLDS ? 4 : im.P <= kLdsPasses2 ? 2 : 1;
    const long long blocks = (n + 32 * waves - 1) / (32 * waves);
    if (blocks > 0x7FFFFFFFll) return PQH_ERR_UNSUPPORTED;
    const size_t lds = (size_t)kCand * 64 * waves * 8 +
                       (BLDS ? (size_t)waves * 2 * im.P * 1024
                             : (size_t)2 * (2 * im.P * 1024 + 128));
    const auto fn = coarse_screen<IP, BLDS>;
    if (lds > 64 * 1024)
        PQH_HIP(ctx, hipFuncSetAttribute((const void*)fn,
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    // float4 loads of x where every piece of eight lies inside a row and on 16 bytes
    const int vec = cq->d % 16 == 0 && ld_x % 4 == 0 && !(reinterpret_cast<uintptr_t>(d_x) & 15u);
    hipLaunchKernelGGL(fn, dim3((unsigned)blocks), dim3(64 * waves), lds, ctx->stream, d_x, n, ld_x,
                       cq->d_cent, cq->d_cent_t, cq->nlist, cq->d, im.P, im.nt, im.frag,
                       im.cn + (IP ? (size_t)im.nt * 32 : 0), im.cmax, screen_kq(16 * im.P), vec,
                       d_list, d_dist, ctx->d_diag);
    PQH_LAUNCH_CHECK(ctx);
    return PQH_OK;
}

int coarse_screen_call(bool ip, pqh_ctx_t* ctx, const pqh_coarse_t* cq, const float* d_x,
                       long long n, long long ld_x, int32_t* d_list, float* d_dist) {
    if (!ctx) return pqh_no_ctx_status();
    if (!cq || n < 0 || ld_x < cq->d || (n > 0 && (!d_x || !d_list))) return PQH_ERR_ARG;
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    if (n == 0) return PQH_OK;
    hipLaunchKernelGGL(screen_clear, dim3(1), dim3(1), 0, ctx->stream, ctx->d_diag);
    PQH_LAUNCH_CHECK(ctx);
    const int P = (cq->d + 15) / 16;
    if (P > kLdsPasses)   // more than the LDS staging holds: the direct kernel, counts (0, 0)
        return ip ? pqh_coarse_assign_ip(ctx, cq, d_x, n, ld_x, d_list, d_dist)
                  : pqh_coarse_assign(ctx, cq, d_x, n, ld_x, d_list, d_dist);
    rc = screen_prepare(ctx, const_cast<pqh_coarse*>(cq));
    if (rc) return rc;
    if (P <= kRegPasses)
        return ip ? screen_launch<true, false>(ctx, cq, d_x, n, ld_x, d_list, d_dist)
                  : screen_launch<false, false>(ctx, cq, d_x, n, ld_x, d_list, d_dist);
    return ip ? screen_launch<true, true>(ctx, cq, d_x, n, ld_x, d_list, d_dist)
              : screen_launch<false, true>(ctx, cq, d_x, n, ld_x, d_list, d_dist);
}

}  // namespace

extern "C" {

int pqh_coarse_assign_screen(pqh_ctx_t* ctx, const pqh_coarse_t* cq, const float* d_x, long long n,
                             long long ld_x, int32_t* d_list, float* d_dist) {
    return coarse_screen_call(false, ctx, cq, d_x, n, ld_x, d_list, d_dist);
}

int pqh_coarse_assign_screen_ip(pqh_ctx_t* ctx, const pqh_coarse_t* cq, const float* d_x,
                                long long n, long long ld_x, int32_t* d_list, float* d_dist) {
    return coarse_screen_call(true, ctx, cq, d_x, n, ld_x, d_list, d_dist);
}

int pqh_coarse_last_screen_counts(pqh_ctx_t* ctx, unsigned long long* reranked,
                                  unsigned long long* fallback) {
    if (!ctx) return pqh_no_ctx_status();
    if (!reranked || !fallback) return PQH_ERR_ARG;
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    unsigned long long v[2] = {0, 0};
    PQH_HIP(ctx, hipMemcpyAsync(v, ctx->d_diag + kDiagRerank, sizeof(v), hipMemcpyDeviceToHost,
                                ctx->stream));
    PQH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *reranked = v[0];
    *fallback = v[1];
    return PQH_OK;
}

}  // extern "C"
