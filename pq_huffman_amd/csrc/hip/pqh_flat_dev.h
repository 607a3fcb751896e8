// pqh_flat_dev.h -- what the exact searches over raw rows share (pqh_flat.hip, the screen over all
// rows, and pqh_flat_lists.hip, the direct scan of probed lists): one step of the definition's
// chain, the rule for the groups of a list scan (host code, shared with pqh_sq.hip), and a
// query's running list kept in LDS between the offers that change it.  Every list function is
// device code, called by a whole wave whose lane number is threadIdx.x.
#pragma once

#include <cmath>
#include <type_traits>

#include "pqh_internal.h"
#include "pqh_topk_dev.h"

namespace {

// ------------------------------------------------------------------- the definition's chain
template <bool IP>
__device__ __forceinline__ void chain_step(float& acc, float qv, float xv) {
    if constexpr (IP) {
        acc = acc - qv * xv;
    } else {
        const float t = qv - xv;
        acc = acc + t * t;
    }
}

// ------------------------------------------------------------------- rows of 16-bit values
// A row type is the compiler's own element type: float, _Float16 (PQH_ROWS_F16) or __bf16
// (PQH_ROWS_BF16).  Every 16-bit value is an fp32 value, so (float) of an element is exact; the
// fp16 conversion is the hardware's (v_cvt_f32_f16, subnormals kept), the bf16 one a shift.
template <typename T>
constexpr bool kRows16 = !std::is_same_v<T, float>;

// the low and the high half of a dword of a row, as fp32
template <typename T>
__device__ __forceinline__ float half_lo(unsigned w) {
    if constexpr (std::is_same_v<T, __bf16>) {
        return __uint_as_float(w << 16);
    } else {
        return (float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xFFFFu));
    }
}
template <typename T>
__device__ __forceinline__ float half_hi(unsigned w) {
    if constexpr (std::is_same_v<T, __bf16>) {
        return __uint_as_float(w & 0xFFFF0000u);
    } else {
        return (float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16));
    }
}

// ------------------------------------------------------------------- the groups of a list scan
// (host) The groups a unit of the list scans is cut into (flat_lists, sq_lists).  The lists'
// lengths are device data, so the plan goes by the mean list: a group per kSegRows rows of it;
// and where the units are fewer than the compute units, as many groups as fill them, two a tile
// of the mean list at the most.  The context's search_groups tuning sets them outright.
constexpr long long kSegRows = 2048;   // mean list length from which a unit is cut into groups
constexpr int kMaxGroups = 64;
inline long long lists_groups(const pqh_ctx* ctx, long long n, long long nlist, long long bound,
                              int tile) {
    const long long mean = (n + nlist - 1) / nlist;
    long long groups = (mean + kSegRows - 1) / kSegRows;
    if (bound * groups < ctx->num_cus) {
        const long long fill = (ctx->num_cus + bound - 1) / bound, most = 2 * ((mean + tile - 1) / tile);
        groups = fill < most ? fill : most;
    }
    groups = groups < 1 ? 1 : groups > kMaxGroups ? kMaxGroups : groups;
    if (ctx->tune_search_groups > 0) groups = ctx->tune_search_groups < 65535 ? ctx->tune_search_groups : 65535;
    return groups;
}

// ------------------------------------------------------------------- a query's list
template <int KR>
using ListT = std::conditional_t<KR == 1, TopK, TopKW>;

template <int KR>
__device__ __forceinline__ void list_reset(ListT<KR>& e) {
    if constexpr (KR == 1) {
        e.d = INFINITY;
        e.id = -1ll;
    } else {
        list_clear(e);
    }
}

template <int KR>
__device__ __forceinline__ float list_kth(const ListT<KR>& e, int kth) {
    if constexpr (KR == 1) {
        return lane_f(e.d, kth);
    } else {
        return e.td;
    }
}

// the k entries of a list in LDS (dist, row of the slab) into the lanes, padding behind them
template <int KR>
__device__ __forceinline__ void list_from_lds(ListT<KR>& e, const float* ld, const int* li, int k) {
    const int lane = threadIdx.x;
    list_reset<KR>(e);
    if constexpr (KR == 1) {
        if (lane < k) e.d = ld[lane], e.id = (long long)li[lane];
    } else {
#pragma unroll
        for (int b = 0; b < kWideKR; ++b)
            if (b * 64 + lane < k) e.d[b] = ld[b * 64 + lane], e.id[b] = (long long)li[b * 64 + lane];
        list_threshold(e, k - 1);
    }
}

template <int KR>
__device__ __forceinline__ void list_to_lds(const ListT<KR>& e, float* ld, int* li, int k) {
    const int lane = threadIdx.x;
    if constexpr (KR == 1) {
        if (lane < k) ld[lane] = e.d, li[lane] = (int)e.id;
    } else {
#pragma unroll
        for (int b = 0; b < kWideKR; ++b)
            if (b * 64 + lane < k) ld[b * 64 + lane] = e.d[b], li[b * 64 + lane] = (int)e.id[b];
    }
}

}  // namespace
