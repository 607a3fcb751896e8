// pqh_screen_dev.h -- what the two bf16-split MFMA screens share (pqh_coarse_screen.hip, the
// coarse quantizer; pqh_assign_screen.hip, the PQ sub-codebooks): the vector types of
// v_mfma_f32_32x32x16_bf16, a lane's candidate list, the wave combine of the finish and the
// bound's coefficient.
#pragma once

#include <cmath>

#include "pqh_internal.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int kCand = 16;          // candidate entries per lane

// the smallest (dist, list) of the wave, in every lane: coarse_assign's combine
__device__ __forceinline__ void wave_first_min(float& bd, int& bi) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const float od = __shfl_xor(bd, s);
        const int oi = __shfl_xor(bi, s);
        const bool take = (od < bd) | ((od == bd) & (oi < bi));
        bd = take ? od : bd;
        bi = take ? oi : bi;
    }
}

__device__ __forceinline__ float fmin2(float a, float b) {
    return __builtin_elementwise_minimum(a, b);
}

// a lane's candidate list: entry e of thread tid at [e * nthr + tid] (no bank conflicts)
struct Cands {
    float* s;
    int* l;
    int nthr, tid, cnt;
    bool ovf;
    // keep what is at or below thr
    __device__ __forceinline__ void prune(float thr) {
        int k = 0;
        for (int e = 0; e < cnt; ++e) {
            const float se = s[e * nthr + tid];
            const int le = l[e * nthr + tid];
            if (se <= thr) {
                s[k * nthr + tid] = se;
                l[k * nthr + tid] = le;
                ++k;
            }
        }
        cnt = k;
    }
    __device__ __forceinline__ void append(float sc, int li, float thr) {
        if (cnt == kCand) prune(thr);
        if (cnt == kCand) {
            ovf = true;
        } else {
            s[cnt * nthr + tid] = sc;
            l[cnt * nthr + tid] = li;
            ++cnt;
        }
    }
};

// tau = kq * (||x||^2 + Cmax) + 2^-100: the coefficient of DESIGN.md 4.5.16 for dp padded
// dimensions, times 1 + 2^-9 for the roundings of ||x||^2, Cmax and tau itself, rounded upwards
inline float screen_kq(int dp) {
    const double k = std::ldexp(115.0 + 14.6 * dp, -22) * (1.0 + std::ldexp(1.0, -9));
    return std::nextafterf((float)k, INFINITY);
}

}  // namespace
