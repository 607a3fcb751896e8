// pqh_flat_screen_dev.h -- what the two screens over all rows of a pqh_flat share (pqh_flat.hip,
// the top-k search; pqh_flat_range.hip, the range search): the object, the constants of a staged
// tile and of a lane's candidate buffer, the loads of eight values of a row, and the interleaved
// chains of a drain.
#pragma once

#include "pqh_flat_dev.h"
#include "pqh_internal.h"
#include "pqh_screen_dev.h"

struct pqh_flat {
    pqh_ctx* ctx = nullptr;
    const void* d_x = nullptr;    // the caller's rows, not owned
    int rows = PQH_ROWS_F32;      // their element type
    long long n = 0, ld_x = 0;
    int d = 0;
    float* d_norms = nullptr;     // [n], then Cmax
    unsigned* d_cmax = nullptr;
};

namespace {

constexpr int kRegPasses = 8;       // passes of a panel of 128 dimensions: B in 64 VGPRs
constexpr int kMaxPasses = 64;      // d <= 1024 is screened
constexpr int kFlatCand = 32;       // candidate entries per lane; drained once past half
constexpr int kChainU = 4;          // pairs a lane chains at once in a drain
constexpr int kDiagChains = 13, kDiagFallback = 14;   // pqh_ctx::d_diag slots of the counts
constexpr long long kMinSlab = 1024;

// U independent chains of one lane, interleaved (a chain alone is a string of dependent
// operations); vec: every row on 16 bytes and d % 4 == 0 (16-bit rows: d % 8 == 0, a 16-byte load
// is eight elements, converted per step)
template <bool IP, int U, typename T>
__device__ __forceinline__ void chains(const float* const (&qp)[U], const T* const (&xp)[U],
                                       int d, bool vec, float (&out)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) out[u] = 0.f;
    if constexpr (kRows16<T>) {
        if (vec) {
#pragma unroll 1
            for (int j = 0; j < d; j += 8) {
                float4 a[U][2];
                u32x4 b[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    a[u][0] = *reinterpret_cast<const float4*>(qp[u] + j);
                    a[u][1] = *reinterpret_cast<const float4*>(qp[u] + j + 4);
                    b[u] = *reinterpret_cast<const u32x4*>(xp[u] + j);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        chain_step<IP>(out[u], a[u][h].x, half_lo<T>(b[u][2 * h]));
                        chain_step<IP>(out[u], a[u][h].y, half_hi<T>(b[u][2 * h]));
                        chain_step<IP>(out[u], a[u][h].z, half_lo<T>(b[u][2 * h + 1]));
                        chain_step<IP>(out[u], a[u][h].w, half_hi<T>(b[u][2 * h + 1]));
                    }
                }
            }
        } else {
#pragma unroll 4
            for (int j = 0; j < d; ++j) {
#pragma unroll
                for (int u = 0; u < U; ++u) chain_step<IP>(out[u], qp[u][j], (float)xp[u][j]);
            }
        }
    } else if (vec) {
#pragma unroll 2
        for (int j = 0; j < d; j += 4) {
            float4 a[U], b[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                a[u] = *reinterpret_cast<const float4*>(qp[u] + j);
                b[u] = *reinterpret_cast<const float4*>(xp[u] + j);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                chain_step<IP>(out[u], a[u].x, b[u].x);
                chain_step<IP>(out[u], a[u].y, b[u].y);
                chain_step<IP>(out[u], a[u].z, b[u].z);
                chain_step<IP>(out[u], a[u].w, b[u].w);
            }
        }
    } else {
#pragma unroll 4
        for (int j = 0; j < d; ++j) {
#pragma unroll
            for (int u = 0; u < U; ++u) chain_step<IP>(out[u], qp[u][j], xp[u][j]);
        }
    }
}

// eight values of a row from dimension j0 on (zeros from d on)
__device__ __forceinline__ void load8(const float* __restrict__ xr, int j0, int d, bool vec,
                                      float* v) {
    if (vec) {   // d % 16 == 0 and every row on 16 bytes: j0 + 8 <= d
        const float4 a = *reinterpret_cast<const float4*>(xr + j0);
        const float4 b = *reinterpret_cast<const float4*>(xr + j0 + 4);
        v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
        v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = j0 + e < d ? xr[min(j0 + e, d - 1)] : 0.f;
    }
}

// the same eight values of a row of 16-bit elements, as they lie in memory: four packed dwords
// (zeros from d on); vec: d % 16 == 0 and every row on 16 bytes, one 16-byte load
template <typename T>
__device__ __forceinline__ u32x4 load8_packed(const T* __restrict__ xr, int j0, int d, bool vec) {
    if (vec) return *reinterpret_cast<const u32x4*>(xr + j0);
    const unsigned short* s = reinterpret_cast<const unsigned short*>(xr);
    u32x4 v;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int e = j0 + 2 * w;
        const unsigned lo = e < d ? (unsigned)s[min(e, d - 1)] : 0u;
        const unsigned hi = e + 1 < d ? (unsigned)s[min(e + 1, d - 1)] : 0u;
        v[w] = lo | hi << 16;
    }
    return v;
}

// a staged unit (one panel of one tile, P passes) in 16-byte words: xh | xl fragments, then the
// 32 norms, the mask word and the staging waves' low-bits flags
__host__ __device__ constexpr int flat_tile_u4(int P) { return 2 * P * 64 + 12; }

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace
