// pqh_assign_screen.hip -- PQ assignment for any codebook shape (mode 2 of pqh_pq_assign and
// pqh_pq_assign_parts): a bf16-split MFMA screen over a sub-codebook held in LDS and an exact
// finish, the codes of pq_assign_exact bit for bit (score, bound, selection and
// finish are those of 4.5.16, per subspace).
//
//  pq_image_frags / pq_image_norms  the prepared codebook, once per pqh_pq: per subspace -c split
//                 into two bf16 halves (-c = ch + cl + r) in the A-operand order of
//                 v_mfma_f32_32x32x16_bf16, [subspace][tile of 32 codes][half][pass of 16 dims]
//                 [lane], dsub padded with zero slots and K with zero rows; ||c||^2 in fp32 (from
//                 a double sum), +inf for the padded codes, so a padded code never wins; Cmax =
//                 max ||c||^2 per subspace.
//  pq_screen<RES, PM>  one subspace per workgroup (grid y), persistent over blocks of 32 rows.  A
//                 wave owns 32 rows x dsub, the MFMA's B operand: 2x as xh | xl, the two bf16
//                 halves, in registers (P = ceil(dsub / 16) <= PM passes; 8 PM VGPRs).
//                 RES: the workgroup copies the subspace's image into LDS once; its waves then
//                 take blocks of rows on their own: no barrier and no global A traffic in the
//                 loop.  Streamed (an image that does not fit): the workgroup's four waves take
//                 four blocks together, and the tiles of 32 codes pass through a double buffer in
//                 LDS, tile t + 1's global loads issued before tile t's MFMAs, one barrier per
//                 tile.
//                 Score of a code: S = ||c||^2 - 2 x.c (the accumulator starts at ||c||^2);
//                 passes xh.ch, xh.cl and, when some x of the wave is not bf16-exact, xl.ch.
//                 Selection: a lane reduces its 16 scores of a tile to one minimum and walks them
//                 only where that minimum is at or below its running best + tau; the walk appends
//                 (score, code) pairs to the lane's own 16-entry list in LDS.
//                 Finish, same kernel: one candidate -- that code; else the definition's chain for
//                 every candidate, the smallest by (dist, code).  A (row, subspace) whose list
//                 overflowed, or whose tau is not below 2^110 (a non-finite x or centroid, or
//                 scores that may have overflowed), takes the chain over all K codes, lane = code,
//                 strict `<` from (+inf, 0): pq_assign_exact's rule.
//                 The codes of a block are gathered in the lanes of its rows and stored once, with
//                 the fused histogram's atomic beside the store.
#include <algorithm>
#include <cstring>

#include "pqh_internal.h"
#include "pqh_screen_dev.h"

namespace {

constexpr int kMaxPasses = 8;                 // dsub <= 128: the B fragments in 64 VGPRs
constexpr int kStreamWaves = 4;               // waves that share the streamed form's tiles
constexpr int kMaxWaves = 8;                  // of a resident workgroup
constexpr size_t kLdsBytes = 160 * 1024;      // of a compute unit
constexpr size_t kCandBytes = (size_t)kCand * 64 * 8;   // a wave's candidate lists
constexpr int kDiagRerank = 11, kDiagFallback = 12;     // pqh_ctx::d_diag slots of the counts

// the image of a codebook: [m][nt][2][P][64] u32x4 fragments, [m][nt * 32] floats, [m] Cmax bits
struct Image {
    u32x4* frag;
    float* cn;
    unsigned* cmax;
    int P, nt;
    size_t bytes;
};
Image image_of(void* base, int m, int k, int dsub) {
    Image im;
    im.P = (dsub + 15) / 16;
    im.nt = (k + 31) / 32;
    const size_t fb = (size_t)m * im.nt * 2 * im.P * 64 * 16;
    char* b = static_cast<char*>(base);
    im.frag = reinterpret_cast<u32x4*>(b);
    im.cn = reinterpret_cast<float*>(b + fb);
    im.cmax = reinterpret_cast<unsigned*>(im.cn + (size_t)m * im.nt * 32);
    im.bytes = fb + (size_t)m * im.nt * 32 * 4 + (size_t)m * 4;
    return im;
}
// LDS bytes of one subspace's image: a tile's fragments and its 32 accumulator starts
size_t tile_bytes(int P) { return (size_t)2 * P * 1024 + 128; }

__global__ void __launch_bounds__(64)
pq_image_frags(const float* __restrict__ cent, int k, int dsub, int P, u32x4* __restrict__ frag,
               unsigned* __restrict__ cmax) {
    const int t = blockIdx.x, p = blockIdx.y, sub = blockIdx.z, lane = threadIdx.x;
    const int nt = gridDim.x;
    const int row = 32 * t + (lane & 31), j0 = 16 * p + 8 * (lane >> 5);
    const float* __restrict__ cs = cent + (size_t)sub * k * dsub;
    bf16x8 hi, lo;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float c = 0.f;
        if (row < k && j0 + j < dsub) c = -cs[(size_t)row * dsub + j0 + j];
        const __bf16 h = (__bf16)c;
        hi[j] = h;
        lo[j] = (__bf16)(c - (float)h);
    }
    u32x4* __restrict__ ft = frag + ((size_t)sub * nt + t) * 2 * P * 64;
    ft[(size_t)p * 64 + lane] = __builtin_bit_cast(u32x4, hi);
    ft[(size_t)(P + p) * 64 + lane] = __builtin_bit_cast(u32x4, lo);
    if (t == 0 && p == 0 && lane == 0) cmax[sub] = 0u;   // pq_image_norms, the next launch, raises it
}

// non-negative floats order as their bits, and a NaN's bits lie above +inf's: a non-finite
// centroid leaves a Cmax that fails every row's tau test
__global__ void __launch_bounds__(256)
pq_image_norms(const float* __restrict__ cent, int k, int kP, int dsub, float* __restrict__ cn,
               unsigned* __restrict__ cmax) {
    const int c = blockIdx.x * 256 + threadIdx.x, sub = blockIdx.y;
    if (c >= kP) return;
    float v = INFINITY;
    if (c < k) {
        const float* __restrict__ cr = cent + ((size_t)sub * k + c) * dsub;
        double s = 0.0;
        for (int j = 0; j < dsub; ++j) s += (double)cr[j] * (double)cr[j];
        v = (float)s;
        atomicMax(cmax + sub, __float_as_uint(v));
    }
    cn[(size_t)sub * kP + c] = v;
}

__global__ void pq_screen_clear(unsigned long long* counts) {
    counts[kDiagRerank] = 0;
    counts[kDiagFallback] = 0;
}

// the definition's chain: t = x_j - c_j; acc = acc + t * t, j ascending (no contraction: the
// file is compiled with -ffp-contract=off)
__device__ __forceinline__ float exact_chain(const float* __restrict__ x,
                                             const float* __restrict__ c, int dsub) {
    float acc = 0.f;
#pragma unroll 4
    for (int j = 0; j < dsub; ++j) {
        const float t = __fsub_rn(x[j], c[j]);
        acc = __fadd_rn(acc, __fmul_rn(t, t));
    }
    return acc;
}

// eight x values of a row's slice from dimension j0 on (zeros from dsub on)
__device__ __forceinline__ void load8(const float* __restrict__ xs, int j0, int dsub, bool vec,
                                      float* v) {
    if (vec) {   // dsub % 8 == 0 and every slice on 16 bytes: a piece lies inside or outside
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        if (j0 < dsub) {
            a = *reinterpret_cast<const float4*>(xs + j0);
            b = *reinterpret_cast<const float4*>(xs + j0 + 4);
        }
        v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
        v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = j0 + e < dsub ? xs[j0 + e] : 0.f;
    }
}

struct ScreenArgs {
    const float* x;           // the first row
    long long n, ld_x;
    int m, k, dsub, P, nt;
    const float* cent;        // [m][k][dsub]
    const u32x4* frag;
    const float* cn;
    const unsigned* cmax;
    float kq;
    int vec, wide;            // float4 loads of x; u16 codes
    void* codes;
    long long ldc;            // 0: codes [n][m]; else part i's codes at i * ldc
    uint32_t* hist;           // [m][k] or null
    unsigned long long* diag;
};

template <bool RES, int PM>
__global__ void __launch_bounds__(64 * (RES ? kMaxWaves : kStreamWaves))
pq_screen(const ScreenArgs a) {
    extern __shared__ u32x4 smem[];
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nwaves = nthr >> 6;
    const int h = lane >> 5;
    const int sub = blockIdx.y, P = PM == 1 ? 1 : a.P, nt = a.nt, k = a.k, dsub = a.dsub;
    const float* __restrict__ cent = a.cent + (size_t)sub * k * dsub;
    const u32x4* __restrict__ frag = a.frag + (size_t)sub * nt * 2 * P * 64;
    const float* __restrict__ cn = a.cn + (size_t)sub * nt * 32;
    const float cmax = __uint_as_float(a.cmax[sub]);
    const int st = 2 * P * 64;   // u32x4s of a tile's fragments

    Cands cd;
    cd.s = reinterpret_cast<float*>(smem);
    cd.l = reinterpret_cast<int*>(cd.s + kCand * nthr);
    cd.nthr = nthr, cd.tid = tid;
    u32x4* const rest = smem + (kCand * nthr * 8) / 16;
    // RES: [nt][st] fragments, then [nt * 32] accumulator starts.  Streamed: two tile buffers of
    // st fragments and 32 accumulator starts each
    const float* const cn_lds = reinterpret_cast<const float*>(rest + (size_t)nt * st);
    const int tile_u4 = st + 8;

    if constexpr (RES) {
        const int nf = nt * st;
        for (int i = tid; i < nf; i += nthr) rest[i] = frag[i];
        float* cw = reinterpret_cast<float*>(rest + (size_t)nt * st);
        for (int i = tid; i < nt * 32; i += nthr) cw[i] = cn[i];
        lds_barrier();
    }

    const long long nblk = (a.n + 31) / 32;
    // RES: a wave's blocks, a stride of all waves apart.  Streamed: the workgroup's four blocks
    // (a wave past the last block runs the tiles beside the others and stores nothing)
    const long long first = RES ? (long long)blockIdx.x * nwaves + wave
                                : (long long)blockIdx.x * kStreamWaves;
    const long long stride = (long long)gridDim.x * (RES ? nwaves : kStreamWaves);
#pragma unroll 1
    for (long long b0 = first; b0 < nblk; b0 += stride) {
        const long long blk = RES ? b0 : b0 + wave;
        const long long wrow0 = blk * 32;
        const long long row = wrow0 + (lane & 31);
        const bool valid = row < a.n;
        const float* __restrict__ xr = a.x + (valid ? row : a.n - 1) * a.ld_x + (long long)sub * dsub;

        // ---- the wave's B operand, ||x||^2 and whether the lo pass is needed
        bf16x8 Bh[PM], Bl[PM];
        float X = 0.f;
        unsigned low = 0u;
#pragma unroll
        for (int p = 0; p < PM; ++p) {
            if (p < P) {
                float v[8];
                load8(xr, 16 * p + 8 * h, dsub, a.vec != 0, v);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    X = X + v[e] * v[e];
                    const float s = 2.f * v[e];
                    const __bf16 hb = (__bf16)s;
                    Bh[p][e] = hb;
                    Bl[p][e] = (__bf16)(s - (float)hb);
                    low |= __float_as_uint(s) & 0xFFFFu;
                }
            }
        }
        X = X + __shfl_xor(X, 32);
        const bool any_lo = __ballot(low != 0u) != 0ull;
        // tau: DESIGN.md 4.5.16.  Not below 2^110 (NaN included): the all-codes path
        const float tau = a.kq * (X + cmax) + 0x1p-100f;
        bool fb = !(tau < 0x1p110f);
        float best = INFINITY;
        cd.cnt = 0, cd.ovf = false;

        // ---- the tiles
        auto scores = [&](const u32x4* af, const float* cnp) {
            f32x16 acc;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 c4 = *reinterpret_cast<const f32x4*>(cnp + 8 * q + 4 * h);
                acc[4 * q] = c4[0], acc[4 * q + 1] = c4[1], acc[4 * q + 2] = c4[2],
                        acc[4 * q + 3] = c4[3];
            }
#pragma unroll
            for (int p = 0; p < PM; ++p) {
                if (p < P) {
                    const bf16x8 ah = __builtin_bit_cast(bf16x8, af[p * 64 + lane]);
                    const bf16x8 al = __builtin_bit_cast(bf16x8, af[(P + p) * 64 + lane]);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, Bh[p], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, Bh[p], acc, 0, 0, 0);
                    if (any_lo)
                        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, Bl[p], acc, 0, 0, 0);
                }
            }
            return acc;
        };
        auto select = [&](const f32x16& acc, int t) {
            float mn = fmin2(acc[0], acc[1]);
#pragma unroll
            for (int i = 2; i < 16; i += 2) mn = fmin2(mn, fmin2(acc[i], acc[i + 1]));
            if (!fb && mn <= best + tau) {
                best = fmin2(best, mn);
                const float thr = best + tau;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int c = 32 * t + (i & 3) + 8 * (i >> 2) + 4 * h;
                    if (acc[i] <= thr && c < k) cd.append(acc[i], c, thr);
                }
            }
        };

        if constexpr (RES) {
#pragma unroll 1
            for (int t = 0; t < nt; ++t) select(scores(rest + (size_t)t * st, cn_lds + 32 * t), t);
        } else {
            // thread tid moves u32x4 tid + 256 j of a tile (j < P / 2, rounded up), thread j < 32
            // its accumulator start
            constexpr int kPre = (PM + 1) / 2;
            u32x4 pre[kPre];
            float pre_cn = 0.f;
            auto fetch = [&](int t) {
                const u32x4* src = frag + (size_t)t * st;
#pragma unroll
                for (int j = 0; j < kPre; ++j)
                    pre[j] = src[min(j * 256 + tid, st - 1)];   // (no branch around a load)
                pre_cn = cn[32 * t + (tid & 31)];
            };
            auto stash = [&](u32x4* dst) {
#pragma unroll
                for (int j = 0; j < kPre; ++j)
                    if (j * 256 + tid < st) dst[j * 256 + tid] = pre[j];
                if (tid < 32) reinterpret_cast<float*>(dst + st)[tid] = pre_cn;
            };
            // (the barrier that ended the block before this one freed both buffers)
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

        // ---- the finish.  The two lanes of a row (lane, lane ^ 32) hold its two candidate lists;
        // the row's code ends in its lane of the first half
        best = fmin2(best, __shfl_xor(best, 32));
        const float thr = best + tau;
        cd.prune(thr);
        const int other = __shfl_xor(cd.cnt, 32);
        const int total = cd.cnt + other;
        fb = fb || total == 0 || cd.ovf || __shfl_xor((int)cd.ovf, 32) != 0;
        int code = cd.cnt > 0 ? cd.l[tid] : 0;
        const int ocode = __shfl_xor(code, 32);
        if (cd.cnt == 0) code = ocode;   // (one candidate: in this lane's list or its twin's)
        unsigned long long rr = __ballot(valid && !fb && total > 1 && h == 0);
        unsigned long long fa = __ballot(valid && fb && h == 0);
        if (lane == 0) {
            if (rr) atomicAdd(a.diag + kDiagRerank, (unsigned long long)__popcll(rr));
            if (fa) atomicAdd(a.diag + kDiagFallback, (unsigned long long)__popcll(fa));
        }
        // a row with several candidates: lane = candidate (at most 2 kCand <= 64)
        while (rr) {
            const int r = __builtin_ctzll(rr);
            rr &= rr - 1;
            const int c0 = __shfl(cd.cnt, r), c1 = __shfl(cd.cnt, r + 32);
            const float* __restrict__ xw = a.x + (wrow0 + r) * a.ld_x + (long long)sub * dsub;
            float bd = INFINITY;
            int bi = 0x7FFFFFFF;
            if (lane < c0 + c1) {
                const int src = (tid - lane) + (lane < c0 ? r : r + 32);
                bi = cd.l[(lane < c0 ? lane : lane - c0) * nthr + src];
                bd = exact_chain(xw, cent + (size_t)bi * dsub, dsub);
            }
            wave_first_min(bd, bi);
            if (lane == r) code = bi;
        }
        // the all-codes path: lane = code, pq_assign_exact's strict `<` from (+inf, 0)
        while (fa) {
            const int r = __builtin_ctzll(fa);
            fa &= fa - 1;
            const float* __restrict__ xw = a.x + (wrow0 + r) * a.ld_x + (long long)sub * dsub;
            float bd = INFINITY;
            int bi = 0;
#pragma unroll 1
            for (int c = lane; c < k; c += 64) {
                const float d = exact_chain(xw, cent + (size_t)c * dsub, dsub);
                if (d < bd) bd = d, bi = c;
            }
            wave_first_min(bd, bi);
            if (lane == r) code = bi;
        }
        if (valid && h == 0) {
            const long long at = a.ldc ? (long long)sub * a.ldc + row : row * a.m + sub;
            if (a.wide)
                static_cast<uint16_t*>(a.codes)[at] = (uint16_t)code;
            else
                static_cast<uint8_t*>(a.codes)[at] = (uint8_t)code;
            if (a.hist) atomicAdd(a.hist + (size_t)sub * k + code, 1u);
        }
    }
}

// The LDS budget rule.  A resident workgroup needs the subspace's image and
// 8 KB of candidate lists per wave; g workgroups share a compute unit's 160 KB.  Among the g
// that leave a workgroup at least two waves (at most kMaxWaves), take the one with the most waves
// on a compute unit, 16 at the most (four a SIMD), and of equals the smaller g: fewer copies of
// the image to load.  None: the streamed form.
struct Form {
    int waves, per_cu;   // waves == 0: streamed
    size_t lds;
};
Form choose_form(int nt, int P) {
    const size_t image = (size_t)nt * tile_bytes(P);
    Form f{0, 0, 0};
    for (int g = 1; g <= 8; ++g) {
        const size_t share = kLdsBytes / g;
        if (share < image + 2 * kCandBytes) break;
        int w = (int)std::min<size_t>((share - image) / kCandBytes, kMaxWaves);
        w = std::min(w, 16 / g);
        if (w >= 2 && w * g > f.waves * f.per_cu) f = Form{w, g, image + w * kCandBytes};
    }
    if (!f.waves) {
        f.lds = kStreamWaves * kCandBytes + 2 * tile_bytes(P);
        f.per_cu = (int)std::min<size_t>(kLdsBytes / f.lds, 4);
    }
    return f;
}

int image_prepare(pqh_ctx* ctx, int m, int k, int dsub, const float* d_cent, void** image) {
    if (*image) return PQH_OK;
    const size_t bytes = image_of(nullptr, m, k, dsub).bytes;
    void* base = nullptr;
    if (hipMalloc(&base, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return pqh_set_error(ctx, PQH_ERR_NOMEM, "assign screen: cannot allocate %zu bytes", bytes);
    }
    const Image im = image_of(base, m, k, dsub);
    hipLaunchKernelGGL(pq_image_frags, dim3((unsigned)im.nt, (unsigned)im.P, (unsigned)m), dim3(64),
                       0, ctx->stream, d_cent, k, dsub, im.P, im.frag, im.cmax);
    hipLaunchKernelGGL(pq_image_norms, dim3((unsigned)((im.nt * 32 + 255) / 256), (unsigned)m),
                       dim3(256), 0, ctx->stream, d_cent, k, im.nt * 32, dsub, im.cn, im.cmax);
    if (hipGetLastError() != hipSuccess) {
        (void)hipFree(base);
        return pqh_set_error(ctx, PQH_ERR_HIP, "assign screen: the codebook image launch failed");
    }
    *image = base;
    return PQH_OK;
}

template <bool RES, int PM>
int screen_launch(pqh_ctx* ctx, const ScreenArgs& a, const Form& f) {
    const auto fn = pq_screen<RES, PM>;
    if (f.lds > 64 * 1024)
        PQH_HIP(ctx, hipFuncSetAttribute((const void*)fn,
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)f.lds));
    const int waves = RES ? f.waves : kStreamWaves;
    // the workgroups that are resident at once, shared among the subspaces; no more than the work
    const long long nblk = (a.n + 31) / 32;
    long long gx = std::max(1ll, (long long)ctx->num_cus * f.per_cu / a.m);
    gx = std::min(gx, (nblk + waves - 1) / waves);
    hipLaunchKernelGGL(fn, dim3((unsigned)gx, (unsigned)a.m), dim3(64 * waves), f.lds, ctx->stream,
                       a);
    PQH_LAUNCH_CHECK(ctx);
    return PQH_OK;
}

template <bool RES>
int screen_launch_p(pqh_ctx* ctx, const ScreenArgs& a, const Form& f) {
    if (a.P == 1) return screen_launch<RES, 1>(ctx, a, f);
    if (a.P == 2) return screen_launch<RES, 2>(ctx, a, f);
    if (a.P <= 4) return screen_launch<RES, 4>(ctx, a, f);
    return screen_launch<RES, 8>(ctx, a, f);
}

}  // namespace

bool pqh_assign_screen_serves(int dsub) { return dsub <= 16 * kMaxPasses; }

int pqh_assign_screen_clear(pqh_ctx* ctx) {
    hipLaunchKernelGGL(pq_screen_clear, dim3(1), dim3(1), 0, ctx->stream, ctx->d_diag);
    PQH_LAUNCH_CHECK(ctx);
    ctx->rerank_slot = kDiagRerank;
    return PQH_OK;
}

int pqh_assign_screen_launch(pqh_ctx* ctx, int m, int k, int dsub, const float* d_cent, void** image,
                             const float* d_x, long long n, long long ld_x, void* d_codes,
                             long long ldc, uint32_t* d_counts) {
    if (m > 65535) return PQH_ERR_UNSUPPORTED;   // grid y
    int rc = image_prepare(ctx, m, k, dsub, d_cent, image);
    if (rc) return rc;
    const Image im = image_of(*image, m, k, dsub);
    ScreenArgs a;
    a.x = d_x, a.n = n, a.ld_x = ld_x;
    a.m = m, a.k = k, a.dsub = dsub, a.P = im.P, a.nt = im.nt;
    a.cent = d_cent, a.frag = im.frag, a.cn = im.cn, a.cmax = im.cmax;
    a.kq = screen_kq(16 * im.P);
    // float4 loads of x where every piece of eight lies inside or outside a slice, on 16 bytes
    a.vec = dsub % 8 == 0 && ld_x % 4 == 0 && !(reinterpret_cast<uintptr_t>(d_x) & 15u);
    a.wide = k > 256;
    a.codes = d_codes, a.ldc = ldc, a.hist = d_counts, a.diag = ctx->d_diag;
    const Form f = choose_form(im.nt, im.P);
    return f.waves ? screen_launch_p<true>(ctx, a, f) : screen_launch_p<false>(ctx, a, f);
}

void pqh_assign_screen_free(void* image) { (void)hipFree(image); }

extern "C" {

int pqh_pq_last_screen_counts(pqh_ctx_t* ctx, unsigned long long* reranked,
                              unsigned long long* fallback) {
    if (!ctx || !reranked || !fallback) return PQH_ERR_ARG;
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
