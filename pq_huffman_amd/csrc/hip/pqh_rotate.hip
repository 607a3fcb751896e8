// pqh_rotate.hip -- a full-dimension linear map in front of the product quantizer (OPQ) and the
// sums its training needs.
//
//  rotate         out[v][j] = sum_t x[v][t] * R[t][j], one fp32 chain from +0.0 with t ascending,
//                 one multiply and one add per element, no contraction: coarse_assign's shape
//                 (pqh_ivf.hip) with a store where the argmin was.  A workgroup of 256 threads
//                 owns kTR = 128 rows and streams the columns of R past them in tiles of
//                 kTC = 128, both staged kTT = 32 steps of t at a time into LDS with t outermost
//                 (R[t][j..] is contiguous, so its tile needs no transposed staging); thread
//                 (ty, tx) keeps an 8 x 8 block of sums (rows 8 ty .. 8 ty + 7, columns
//                 4 tx .. 4 tx + 3 and 64 + 4 tx .. + 3 of the tile) and reads 16 floats (four
//                 ds_read_b128) for 128 operations per step.  transpose = 1 is the same kernel
//                 over the transposed copy the object keeps.  The result does not depend on the
//                 grid: a row's sums and their order are the same wherever the row falls.
//  cross_moments  M[a][b] = sum_v x[v][a] * y[v][b]: every product one fp32 multiply, scaled by
//                 2^s, rounded to an int64 and added as an integer (the sums of pqh_kmeans.hip),
//                 so neither the order nor the grid can matter.  A workgroup owns a 64 x 64 tile
//                 of M and a range of rows, staged kMR = 32 rows at a time; thread (ty, tx) keeps
//                 a 4 x 4 block of int64 sums in registers over the whole range.  An entry of the
//                 tile has one owner in a workgroup, so the flush is one global 64-bit atomic per
//                 (workgroup, entry) -- the LDS stage of kmeans_accum, where many threads share
//                 a cell, has nothing to combine here.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "pqh_internal.h"

struct pqh_rotation {
    pqh_ctx* ctx = nullptr;
    int d = 0;
    float* d_r = nullptr;     // [d][d]: R[t][j]
    float* d_rt = nullptr;    // [d][d]: R[j][t]
};

namespace {

constexpr int kTR = 128;            // rows of a workgroup
constexpr int kTC = 128;            // columns of a tile
constexpr int kTT = 32;             // steps of t staged at a time
constexpr int kR = 8, kC = 8;       // a thread's block of sums
constexpr int kStride = kTR + 4;    // floats between two steps of a staged tile (16-byte aligned)
static_assert(kTR == kTC && kTR == 16 * kR && kTC == 16 * kC, "256 threads as 16 x 16");

__global__ void __launch_bounds__(256, 2)
rotate_kernel(const float* __restrict__ x, long long n, long long ld_x,
              const float* __restrict__ rm, int d, float* __restrict__ out, long long ld_out) {
    __shared__ __attribute__((aligned(16))) float xs[kTT * kStride];   // [t][row]
    __shared__ __attribute__((aligned(16))) float rs[kTT * kStride];   // [t][column]
    const int tid = threadIdx.x;
    const int tx = tid & 15, ty = tid >> 4;
    const int st = tid & 31, sr = tid >> 5;      // staging x: the thread's step, its first row
    const int rc = tid & 127, rt = tid >> 7;     // staging R: the thread's column, its first step
    const long long row0 = (long long)blockIdx.x * kTR;

#pragma unroll 1
    for (int c0 = 0; c0 < d; c0 += kTC) {
        float acc[kR][kC];
#pragma unroll
        for (int r = 0; r < kR; ++r)
#pragma unroll
            for (int c = 0; c < kC; ++c) acc[r][c] = 0.f;

#pragma unroll 1
        for (int t0 = 0; t0 < d; t0 += kTT) {
            const int tn = min(kTT, d - t0);
            __syncthreads();   // the reads of the stage before are done
            // nothing past d or n is read: the index is held at the last step, row and column
            // instead (no branch around a load), and what those slots hold is never summed
            // (t >= tn) or never stored (row >= n, column >= d)
            const int tt = t0 + min(st, tn - 1);
#pragma unroll 8
            for (int i = 0; i < kTR / 8; ++i) {
                const int r = sr + 8 * i;
                const long long xr = min(row0 + r, n - 1);
                xs[st * kStride + r] = x[xr * ld_x + tt];
            }
            const int cj = min(c0 + rc, d - 1);
#pragma unroll 8
            for (int i = 0; i < kTT / 2; ++i) {
                const int t = rt + 2 * i;
                rs[t * kStride + rc] = rm[(long long)(t0 + min(t, tn - 1)) * d + cj];
            }
            lds_barrier();
#pragma unroll 2
            for (int t = 0; t < tn; ++t) {
                const float4 xa = *reinterpret_cast<const float4*>(&xs[t * kStride + ty * kR]);
                const float4 xb = *reinterpret_cast<const float4*>(&xs[t * kStride + ty * kR + 4]);
                const float4 ca = *reinterpret_cast<const float4*>(&rs[t * kStride + tx * 4]);
                const float4 cb = *reinterpret_cast<const float4*>(&rs[t * kStride + 64 + tx * 4]);
                const float xv[kR] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w};
                const float cv[kC] = {ca.x, ca.y, ca.z, ca.w, cb.x, cb.y, cb.z, cb.w};
#pragma unroll
                for (int r = 0; r < kR; ++r)
#pragma unroll
                    for (int c = 0; c < kC; ++c) {
                        const float p = xv[r] * cv[c];
                        acc[r][c] = acc[r][c] + p;
                    }
            }
        }
#pragma unroll
        for (int r = 0; r < kR; ++r) {
            const long long row = row0 + ty * kR + r;
            if (row < n) {
                float* __restrict__ o = out + row * ld_out;
#pragma unroll
                for (int c = 0; c < kC; ++c) {
                    const int j = c0 + (c < 4 ? tx * 4 + c : 64 + tx * 4 + (c - 4));
                    if (j < d) o[j] = acc[r][c];
                }
            }
        }
    }
}

constexpr int kMT = 64;             // entries of M a workgroup owns, each way
constexpr int kMR = 32;             // rows staged at a time
constexpr int kMStride = kMT + 4;   // floats between two staged rows (16-byte aligned)

__global__ void __launch_bounds__(256)
moments_kernel(const float* __restrict__ x, long long n, long long ld_x, int dx,
               const float* __restrict__ y, long long ld_y, int dy, double scale,
               long long rows_per_group, long long* __restrict__ sums) {
    __shared__ __attribute__((aligned(16))) float xs[kMR * kMStride];   // [row][a]
    __shared__ __attribute__((aligned(16))) float ys[kMR * kMStride];   // [row][b]
    const int tid = threadIdx.x;
    const int tx = tid & 15, ty = tid >> 4;
    const int sc = tid & 63, sr = tid >> 6;      // staging: the thread's column, its first row
    const int a0 = blockIdx.y * kMT, b0 = blockIdx.z * kMT;
    const long long v0 = (long long)blockIdx.x * rows_per_group;
    const long long v1 = min(n, v0 + rows_per_group);
    // held at the last column: those entries are never flushed
    const int xa = min(a0 + sc, dx - 1), yb = min(b0 + sc, dy - 1);

    long long acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0;

#pragma unroll 1
    for (long long vs = v0; vs < v1; vs += kMR) {
        const int vn = (int)min<long long>(kMR, v1 - vs);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kMR / 4; ++i) {
            const int r = sr + 4 * i;
            const long long v = min(vs + r, v1 - 1);   // held at the last row: never summed
            xs[r * kMStride + sc] = x[v * ld_x + xa];
            ys[r * kMStride + sc] = y[v * ld_y + yb];
        }
        lds_barrier();
#pragma unroll 2
        for (int r = 0; r < vn; ++r) {
            const float4 xq = *reinterpret_cast<const float4*>(&xs[r * kMStride + ty * 4]);
            const float4 yq = *reinterpret_cast<const float4*>(&ys[r * kMStride + tx * 4]);
            const float xv[4] = {xq.x, xq.y, xq.z, xq.w};
            const float yv[4] = {yq.x, yq.y, yq.z, yq.w};
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const float p = xv[a] * yv[b];
                    // p * 2^s is exact in double (scale = 2^s, |s| <= 126): ldexp's value
                    acc[a][b] += __double2ll_rn((double)p * scale);
                }
        }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int ga = a0 + ty * 4 + a;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int gb = b0 + tx * 4 + b;
            if (ga < dx && gb < dy && acc[a][b])
                atomicAdd(reinterpret_cast<unsigned long long*>(&sums[(long long)ga * dy + gb]),
                          (unsigned long long)acc[a][b]);
        }
    }
}

// pqh_kmeans_fixed_shift's formula on the double max|x| * max|y| (the product of two floats is
// exact in double) and n
int moments_shift(float max_x, float max_y, long long n) {
    const double p = (double)max_x * (double)max_y;
    if (!(p > 0.0) || n <= 0) return 40;
    if (std::isinf(p)) return -126;
    const double b = p * (double)n;
    const int s = 61 - (int)std::ceil(std::log2(b));
    return std::max(-126, std::min(100, s));
}

}  // namespace

extern "C" {

int pqh_rotation_create(pqh_ctx_t* ctx, const float* R, int d, pqh_rotation_t** rot) {
    if (!rot) return PQH_ERR_ARG;
    *rot = nullptr;
    if (!R || d < 1) return PQH_ERR_ARG;
    if (d > PQH_ROT_MAX_D) return PQH_ERR_UNSUPPORTED;
    if (!ctx) return pqh_no_ctx_status();
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    const size_t count = (size_t)d * d;
    std::vector<float> t;
    pqh_rotation* r = new (std::nothrow) pqh_rotation();
    try {
        t.resize(count);
    } catch (const std::bad_alloc&) {
        delete r;
        r = nullptr;
    }
    if (!r) return pqh_set_error(ctx, PQH_ERR_NOMEM, "rotation: host memory");
    for (int a = 0; a < d; ++a)
        for (int b = 0; b < d; ++b) t[(size_t)b * d + a] = R[(size_t)a * d + b];
    r->ctx = ctx;
    r->d = d;
    if (hipMalloc(&r->d_r, count * 4) != hipSuccess ||
        hipMalloc(&r->d_rt, count * 4) != hipSuccess) {
        (void)hipGetLastError();
        pqh_rotation_destroy(r);
        return pqh_set_error(ctx, PQH_ERR_NOMEM, "rotation: cannot allocate %zu bytes", count * 8);
    }
    if (hipMemcpy(r->d_r, R, count * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(r->d_rt, t.data(), count * 4, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        pqh_rotation_destroy(r);
        return pqh_set_error(ctx, PQH_ERR_HIP, "rotation: upload failed");
    }
    *rot = r;
    return PQH_OK;
}

int pqh_rotation_destroy(pqh_rotation_t* rot) {
    if (!rot) return PQH_OK;
    if (rot->ctx) {
        (void)hipSetDevice(rot->ctx->device);
        (void)hipStreamSynchronize(rot->ctx->stream);   // no launch may still read them
    }
    if (rot->d_r) (void)hipFree(rot->d_r);
    if (rot->d_rt) (void)hipFree(rot->d_rt);
    delete rot;
    return PQH_OK;
}

int pqh_rotate(pqh_ctx_t* ctx, const pqh_rotation_t* rot, const float* d_x, long long n,
               long long ld_x, float* d_out, long long ld_out, int transpose) {
    if (!rot || n < 0 || ld_x < rot->d || ld_out < rot->d || (transpose != 0 && transpose != 1) ||
        (n > 0 && (!d_x || !d_out)))
        return PQH_ERR_ARG;
    if (!ctx) return pqh_no_ctx_status();
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    if (n == 0) return PQH_OK;
    const long long blocks = (n + kTR - 1) / kTR;
    if (blocks > 0x7FFFFFFFll) return PQH_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(rotate_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, d_x, n,
                       ld_x, transpose ? rot->d_rt : rot->d_r, rot->d, d_out, ld_out);
    PQH_LAUNCH_CHECK(ctx);
    return PQH_OK;
}

int pqh_cross_moments(pqh_ctx_t* ctx, const float* d_x, long long n, long long ld_x, int dx,
                      const float* d_y, long long ld_y, int dy, double* moments) {
    if (!moments || n < 0 || dx < 1 || dy < 1 || ld_x < dx || ld_y < dy ||
        (n > 0 && (!d_x || !d_y)))
        return PQH_ERR_ARG;
    if (dx > PQH_ROT_MAX_D || dy > PQH_ROT_MAX_D) return PQH_ERR_UNSUPPORTED;
    if (!ctx) return pqh_no_ctx_status();
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    const size_t cells = (size_t)dx * dy;
    if (n == 0) {
        std::fill(moments, moments + cells, 0.0);
        return PQH_OK;
    }
    long long* d_sums = nullptr;
    unsigned* d_max = nullptr;
    std::vector<long long> h;
    try {
        h.resize(cells);
    } catch (const std::bad_alloc&) {
        return pqh_set_error(ctx, PQH_ERR_NOMEM, "cross moments: host memory");
    }
    auto cleanup = [&] {
        (void)hipFree(d_sums);
        (void)hipFree(d_max);
    };
    if (hipMalloc(&d_sums, cells * 8) != hipSuccess || hipMalloc(&d_max, 8) != hipSuccess) {
        (void)hipGetLastError();
        cleanup();
        return pqh_set_error(ctx, PQH_ERR_NOMEM, "cross moments buffers");
    }
    // the fixed-point exponent from the two maxima
    unsigned hmax[2] = {0, 0};
    hipError_t e = hipMemsetAsync(d_max, 0, 8, ctx->stream);
    if (e == hipSuccess && (pqh_kmeans_absmax_launch(ctx, d_x, n, ld_x, dx, d_max) ||
                            pqh_kmeans_absmax_launch(ctx, d_y, n, ld_y, dy, d_max + 1)))
        e = hipErrorLaunchFailure;
    if (e == hipSuccess) e = hipMemcpyAsync(hmax, d_max, 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        cleanup();
        return pqh_set_error(ctx, PQH_ERR_HIP, "cross moments absmax: %s", hipGetErrorString(e));
    }
    float fx, fy;
    std::memcpy(&fx, &hmax[0], 4);
    std::memcpy(&fy, &hmax[1], 4);
    const int s = moments_shift(fx, fy, n);
    // about four workgroups a compute unit over all the tiles, 256 rows each at the least
    const unsigned ta = (unsigned)((dx + kMT - 1) / kMT), tb = (unsigned)((dy + kMT - 1) / kMT);
    const long long want = std::max<long long>(1, (4ll * ctx->num_cus) / ((long long)ta * tb));
    long long per = std::max<long long>(256, (n + want - 1) / want);
    per = (per + kMR - 1) / kMR * kMR;
    const long long groups = (n + per - 1) / per;
    e = hipMemsetAsync(d_sums, 0, cells * 8, ctx->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(moments_kernel, dim3((unsigned)groups, ta, tb), dim3(256), 0, ctx->stream,
                           d_x, n, ld_x, dx, d_y, ld_y, dy, std::ldexp(1.0, s), per, d_sums);
        e = hipGetLastError();
    }
    if (e == hipSuccess)
        e = hipMemcpyAsync(h.data(), d_sums, cells * 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    cleanup();
    if (e != hipSuccess)
        return pqh_set_error(ctx, PQH_ERR_HIP, "cross moments: %s", hipGetErrorString(e));
    for (size_t i = 0; i < cells; ++i) moments[i] = std::ldexp((double)h[i], -s);
    return PQH_OK;
}

}  // extern "C"
