// pqh_ivf.hip -- the inverted-file front end of the probe search (pqh_search_*_ranges): a coarse
// quantizer over full vectors, the list layout, and the probe list of every query.
//
// Two metrics, the template parameter IP of the kernels that sum (the host picks the
// instantiation; an `if constexpr` stands around the lines of the sum and nowhere else):
//   L2  dist(x, y) = acc,  acc = +0.0f;  for j ascending:  t = x[j] - y[j];  acc = acc + t * t
//   IP  nip(x, y)  = acc,  acc = +0.0f;  for j ascending:  acc = acc - x[j] * y[j]
// The scan, the top-k lists, the radius compare and the mask order plain fp32 values with `<`, so
// an inner-product score is the NEGATED inner product and "smaller is nearer" holds as it does
// for L2: one fp32 multiply and one fp32 subtract per element, no contraction, no final negation.
//
//  coarse_assign<IP>  list[v] = the first l that minimises dist(x[v], c[l]) (nip for IP), the
//                 exact direct form (subtract, multiply, add per element -- multiply, subtract
//                 for IP -- j ascending, no contraction).  A workgroup of 256
//                 threads owns kTR = 128 rows and streams the centroids past them in tiles of
//                 kTC = 128, both staged kJT = 32 dimensions at a time into LDS with the
//                 dimension outermost; thread (ty, tx) keeps an 8 x 8 block of sums (rows
//                 8 ty .. 8 ty + 7, centroids 4 tx .. 4 tx + 3 and 64 + 4 tx .. + 3 of the tile)
//                 and reads 16 floats (four ds_read_b128) for 192 operations per dimension.
//                 The running best is a strict `<` in ascending list order; the 16 threads of
//                 a row combine by (dist, list).  The result does not depend on the grid: a
//                 row's sums and their order are the same wherever the row falls.
//  coarse_probe<IP>  one workgroup per query, lane = list (the centroids read from a transposed
//                 copy, so a wave's loads are contiguous), the nprobe smallest by (dist, list)
//                 through the wave-wide list of pqh_topk_dev.h, and the probe list in the CSR
//                 form the *_ranges calls take written straight from the offsets.
//  ivf_layout     rocPRIM's stable radix_sort_pairs of (list id, row number) over
//                 ceil(log2 nlist) bits, then one kernel: every offset by a binary search in
//                 the sorted ids, and the check of the ids.
//  mask_pack      a byte per caller row into the bit per stream row the *_masked searches take,
//                 through the layout's permutation.
// The residual form (the stream holds the PQ codes of x - c[list]):
//  ivf_residual   out[s] = x[perm[s]] - c[list[perm[s]]], the gather into list order and the
//                 subtract in one pass.  A half wave owns a row and reads 32 consecutive floats
//                 (or float4s) of it a step, kResRows rows in flight; the centroids come from L2.
//  adc_lut_residual  one workgroup per (query, probed list): the residual query q - c[l] staged
//                 in LDS once, then adc_lut's sum for every one of the m * K entries.
//  adc_lut_residual_ip  the same tables for the inner product, another shape: a workgroup per
//                 (query, slice of the table), the probe's bias folded into part 0.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include <algorithm>
#include <cmath>
#include <new>
#include <type_traits>
#include <vector>

#include "pqh_internal.h"
#include "pqh_topk_dev.h"

struct pqh_coarse {
    pqh_ctx* ctx = nullptr;
    int nlist = 0, d = 0;
    float* d_cent = nullptr;     // [nlist][d]
    float* d_cent_t = nullptr;   // [d][nlist]
};

namespace {

constexpr int kTR = 128;            // rows of a workgroup
constexpr int kTC = 128;            // centroids of a tile
constexpr int kJT = 32;             // dimensions staged at a time
constexpr int kR = 8, kC = 8;       // a thread's block of sums
constexpr int kStride = kTR + 4;    // floats between two dimensions of a staged tile (16-byte
                                    // aligned rows; kTR == kTC, so both tiles share it)
static_assert(kTR == kTC && kTR == 16 * kR && kTC == 16 * kC, "256 threads as 16 x 16");
constexpr int kResidualMaxD = PQH_ADC_RESIDUAL_MAX_D;   // the residual query in LDS: 64 KB

template <bool IP>
__global__ void __launch_bounds__(256, 2)
coarse_assign(const float* __restrict__ x, long long n, long long ld_x,
              const float* __restrict__ cent, int nlist, int d, int32_t* __restrict__ list,
              float* __restrict__ dist) {
    __shared__ __attribute__((aligned(16))) float xs[kJT * kStride];   // [j][row]
    __shared__ __attribute__((aligned(16))) float cs[kJT * kStride];   // [j][centroid]
    const int tid = threadIdx.x;
    const int tx = tid & 15, ty = tid >> 4;
    const int sj = tid & 31, sr = tid >> 5;   // staging: the thread's dimension, its first row
    const long long row0 = (long long)blockIdx.x * kTR;

    float best[kR];
    int bl[kR];
#pragma unroll
    for (int r = 0; r < kR; ++r) best[r] = INFINITY, bl[r] = 0;

#pragma unroll 1
    for (int c0 = 0; c0 < nlist; c0 += kTC) {
        float acc[kR][kC];
#pragma unroll
        for (int r = 0; r < kR; ++r)
#pragma unroll
            for (int c = 0; c < kC; ++c) acc[r][c] = 0.f;

#pragma unroll 1
        for (int j0 = 0; j0 < d; j0 += kJT) {
            const int jn = min(kJT, d - j0);
            __syncthreads();   // the reads of the stage before are done
            // a half wave loads 32 consecutive floats of one row.  Nothing past d, n or nlist
            // is read: the index is held at the last dimension, row and centroid instead (no
            // branch around a load), and what those slots hold is never summed (j >= jn),
            // never stored (row >= n) or never compared (list >= nlist)
            const int jj = j0 + min(sj, jn - 1);
#pragma unroll 8
            for (int i = 0; i < kTR / 8; ++i) {
                const int r = sr + 8 * i;
                const long long xr = min(row0 + r, n - 1);
                const int cr = min(c0 + r, nlist - 1);
                xs[sj * kStride + r] = x[xr * ld_x + jj];
                cs[sj * kStride + r] = cent[(long long)cr * d + jj];
            }
            lds_barrier();
#pragma unroll 2
            for (int j = 0; j < jn; ++j) {
                const float4 xa = *reinterpret_cast<const float4*>(&xs[j * kStride + ty * kR]);
                const float4 xb = *reinterpret_cast<const float4*>(&xs[j * kStride + ty * kR + 4]);
                const float4 ca = *reinterpret_cast<const float4*>(&cs[j * kStride + tx * 4]);
                const float4 cb = *reinterpret_cast<const float4*>(&cs[j * kStride + 64 + tx * 4]);
                const float xv[kR] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w};
                const float cv[kC] = {ca.x, ca.y, ca.z, ca.w, cb.x, cb.y, cb.z, cb.w};
#pragma unroll
                for (int r = 0; r < kR; ++r)
#pragma unroll
                    for (int c = 0; c < kC; ++c) {
                        if constexpr (IP) {
                            acc[r][c] = acc[r][c] - xv[r] * cv[c];
                        } else {
                            const float t = xv[r] - cv[c];
                            acc[r][c] = acc[r][c] + t * t;
                        }
                    }
            }
        }
        // the thread's centroids ascend with c, the tiles with c0: a strict `<` keeps the
        // first minimum
#pragma unroll
        for (int c = 0; c < kC; ++c) {
            const int l = c0 + (c < 4 ? tx * 4 + c : 64 + tx * 4 + (c - 4));
            if (l < nlist) {
#pragma unroll
                for (int r = 0; r < kR; ++r) {
                    const bool take = acc[r][c] < best[r];
                    best[r] = take ? acc[r][c] : best[r];
                    bl[r] = take ? l : bl[r];
                }
            }
        }
    }

    // the 16 threads of a row are 16 neighbouring lanes: the smallest by (dist, list)
#pragma unroll
    for (int r = 0; r < kR; ++r) {
        float bd = best[r];
        int bi = bl[r];
#pragma unroll
        for (int s = 1; s < 16; s <<= 1) {
            const float od = __shfl_xor(bd, s);
            const int oi = __shfl_xor(bi, s);
            const bool take = (od < bd) | ((od == bd) & (oi < bi));
            bd = take ? od : bd;
            bi = take ? oi : bi;
        }
        const long long row = row0 + ty * kR + r;
        if (tx == r && row < n) {
            list[row] = bi;
            if (dist) dist[row] = bd;
        }
    }
}

// sixteen waves: 1,024 lists are one step of every wave (the kernel is latency, not
// throughput: one query keeps one compute unit busy for the length of one list's sum)
constexpr int kProbeWaves = 16;
template <bool IP>
__global__ void __launch_bounds__(64 * kProbeWaves)
coarse_probe(const float* __restrict__ queries, long long nq, long long ld_q,
             const float* __restrict__ cent_t, int nlist, int d, int nprobe,
             const long long* __restrict__ offsets, long long* __restrict__ range_ptr,
             long long* __restrict__ ranges, long long* __restrict__ probes,
             float* __restrict__ probe_dist, unsigned long long* __restrict__ err) {
    __shared__ float xd[(kProbeWaves - 1) * 64];
    __shared__ long long xid[(kProbeWaves - 1) * 64];
    const int lane = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.y);
    const long long q = blockIdx.x;
    const float* __restrict__ x = queries + q * ld_q;
    const int kth = nprobe - 1;
    TopK e{INFINITY, -1ll};
#pragma unroll 1
    for (int base = wave * 64; base < nlist; base += 64 * kProbeWaves) {
        const int l = base + lane;
        const bool valid = l < nlist;
        const float* c = cent_t + (valid ? l : nlist - 1);
        float acc = 0.f;
#pragma unroll 8
        for (int j = 0; j < d; ++j) {
            if constexpr (IP) {
                acc = acc - x[j] * c[(long long)j * nlist];
            } else {
                const float t = x[j] - c[(long long)j * nlist];
                acc = acc + t * t;
            }
        }
        list_offer<false>(e, acc, (long long)l, valid, kth);
    }
    if (wave > 0) {
        xd[(wave - 1) * 64 + lane] = e.d;
        xid[(wave - 1) * 64 + lane] = e.id;
    }
    lds_barrier();
    if (wave != 0) return;
#pragma unroll 1
    for (int s = 0; s < kProbeWaves - 1; ++s) {
        const long long id = xid[s * 64 + lane];
        list_offer<true>(e, xd[s * 64 + lane], id, id >= 0, kth);
    }
    if (lane == 0) {
        range_ptr[q] = q * nprobe;
        if (q == nq - 1) range_ptr[nq] = nq * nprobe;
    }
    if (lane < nprobe) {
        const long long o = q * nprobe + lane;
        long long first = 0, count = 0;
        if (e.id >= 0) {   // (an entry of the list is a list the loop above offered: < nlist)
            const long long a = offsets[e.id], b = offsets[e.id + 1];
            if (b >= a)
                first = a, count = b - a;
            else
                atomicOr(err, 1ull);
        }
        ranges[2 * o] = first;
        ranges[2 * o + 1] = count;
        if (probes) probes[o] = e.id;
        if (probe_dist) probe_dist[o] = e.d;
    }
}

// offsets[l] = the first place of the sorted ids that holds l or more (thread l <= nlist), and
// the check of the ids themselves (thread i < n): one outside [0, nlist) sets the error word
__global__ void __launch_bounds__(256)
ivf_offsets(const int32_t* __restrict__ list, const uint32_t* __restrict__ sorted, long long n,
            int nlist, long long* __restrict__ offsets, unsigned long long* __restrict__ err) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (i < n) {
        const int v = list[i];
        bad = v < 0 || v >= nlist;
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(err, 1ull);
    if (i <= nlist) {
        long long lo = 0, hi = n;
        while (lo < hi) {
            const long long mid = lo + (hi - lo) / 2;
            if (sorted[mid] < (uint32_t)i)
                lo = mid + 1;
            else
                hi = mid;
        }
        offsets[i] = lo;
    }
}

// A workgroup owns 8 * kResRows consecutive rows of the output, half wave h the rows
// base + 8 u + h.  The kResRows rows' loads of a step are issued before the first subtract.  A row
// whose perm entry or list id is out of range reads nothing and is stored as zeros.
constexpr int kResRows = 4;
template <bool VEC>
__global__ void __launch_bounds__(256)
ivf_residual(const float* __restrict__ x, long long n, long long ld_x,
             const int32_t* __restrict__ list, const long long* __restrict__ perm,
             const float* __restrict__ cent, int nlist, int d, float* __restrict__ out,
             long long ld_out, unsigned long long* __restrict__ err) {
    using V = std::conditional_t<VEC, float4, float>;
    constexpr int W = VEC ? 4 : 1;
    const int hl = threadIdx.x & 31, hw = threadIdx.x >> 5;
    const long long base = (long long)blockIdx.x * (8 * kResRows);
    const float* xr[kResRows];
    const float* cr[kResRows];
    bool ok[kResRows];
    bool bad = false;
#pragma unroll
    for (int u = 0; u < kResRows; ++u) {
        const long long s = base + u * 8 + hw;
        long long p = -1;
        if (s < n) p = perm ? perm[s] : s;
        bool good = p >= 0 && p < n;
        int l = -1;
        if (good) l = list[p];
        good = good && l >= 0 && l < nlist;
        bad = bad || (s < n && !good);
        ok[u] = good;
        xr[u] = x + (good ? p : 0) * ld_x;
        cr[u] = cent + (long long)(good ? l : 0) * d;
    }
#pragma unroll 1
    for (int j = hl * W; j < d; j += 32 * W) {
        V xv[kResRows], cv[kResRows];
#pragma unroll
        for (int u = 0; u < kResRows; ++u) {
            xv[u] = V{};
            cv[u] = V{};
            if (ok[u]) {
                xv[u] = *reinterpret_cast<const V*>(xr[u] + j);
                cv[u] = *reinterpret_cast<const V*>(cr[u] + j);
            }
        }
#pragma unroll
        for (int u = 0; u < kResRows; ++u) {
            const long long s = base + u * 8 + hw;
            if (s < n) {
                V r;
                if constexpr (VEC)
                    r = make_float4(xv[u].x - cv[u].x, xv[u].y - cv[u].y, xv[u].z - cv[u].z,
                                    xv[u].w - cv[u].w);
                else
                    r = xv[u] - cv[u];
                *reinterpret_cast<V*>(out + s * ld_out + j) = r;
            }
        }
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(err, 1ull);
}

// lut[o] for o = q * nprobe + p: the table of q - c[probes[o]] against the PQ centroids, the
// sum of adc_lut (pqh_search.hip) with the residual read from LDS.  A list of -1 (the probe
// selection's padding) or outside [0, nlist) (the error bit) gives a table of +inf.
__global__ void __launch_bounds__(256)
adc_lut_residual(const float* __restrict__ queries, long long ld_q, int nprobe,
                 const long long* __restrict__ probes, const float* __restrict__ coarse,
                 int nlist, const float* __restrict__ cent, int m, int k, int dsub, int vec,
                 float* __restrict__ lut, unsigned long long* __restrict__ err) {
    extern __shared__ __attribute__((aligned(16))) float res[];   // [m * dsub]
    const int tid = threadIdx.x;
    const long long o = blockIdx.x;
    const long long l = probes[o];
    const int per = m * k, d = m * dsub;
    float* __restrict__ dst = lut + o * per;
    if (l < 0 || l >= nlist) {   // (the same for every thread of the workgroup)
        for (int e = tid; e < per; e += 256) dst[e] = INFINITY;
        if (l != -1 && tid == 0) atomicOr(err, 1ull);
        return;
    }
    const float* __restrict__ x = queries + (o / nprobe) * ld_q;
    const float* __restrict__ cl = coarse + l * d;
    for (int j = tid; j < d; j += 256) res[j] = x[j] - cl[j];
    lds_barrier();
    for (int e = tid; e < per; e += 256) {
        const float* r = res + (e / k) * dsub;
        const float* c = cent + (long long)e * dsub;
        float acc = 0.f;
        if (vec) {   // dsub a multiple of four and the centroids 16-byte aligned: the same sum
            for (int j = 0; j < dsub; j += 4) {
                const float4 cv = *reinterpret_cast<const float4*>(c + j);
                const float t0 = r[j] - cv.x, t1 = r[j + 1] - cv.y, t2 = r[j + 2] - cv.z,
                            t3 = r[j + 3] - cv.w;
                acc = acc + t0 * t0;
                acc = acc + t1 * t1;
                acc = acc + t2 * t2;
                acc = acc + t3 * t3;
            }
        } else {
            for (int j = 0; j < dsub; ++j) {
                const float t = r[j] - c[j];
                acc = acc + t * t;
            }
        }
        dst[e] = acc;
    }
}

// The inner-product tables of a residual index, lut[o] as above.  <q, c[l] + r> = <q, c[l]> +
// <q, r>: the second term is the plain table of the query, the same for every probe, the first
// one number per probe.  That number is folded into part 0 of the probe's table (bias + entry,
// one add), so the scan's sum over the parts carries it without a new scan form.
// Workgroup (q, s): query q, the table entries [s * kLutPer * 256, (s + 1) * kLutPer * 256): it
// computes their plain values once, keeps them in registers and writes them nprobe times.
// K <= 256 <= kLutPer * 256, so part 0 lies in the workgroups s == 0 and only they need the
// biases.  The probes go through LDS 256 at a time (nprobe has no upper bound here): thread t
// of a round owns probe p0 + t, runs its d-long chain (s == 0, the query staged in LDS) and
// leaves (bias, valid) for the workgroup, which then writes that round's tables, a wave storing
// 64 consecutive floats.
constexpr int kLutPer = 4;
__global__ void __launch_bounds__(256)
adc_lut_residual_ip(const float* __restrict__ queries, long long ld_q, int nprobe,
                    const long long* __restrict__ probes, const float* __restrict__ coarse,
                    int nlist, const float* __restrict__ cent, int m, int k, int dsub,
                    float* __restrict__ lut, unsigned long long* __restrict__ err) {
    extern __shared__ __attribute__((aligned(16))) float qs[];   // the query row, m * dsub floats
    __shared__ float bias[256];
    __shared__ unsigned char ok[256];
    const int tid = threadIdx.x;
    const long long q = blockIdx.x;
    const int s = blockIdx.y;
    const int per = m * k, d = m * dsub;
    const float* __restrict__ x = queries + q * ld_q;
    for (int j = tid; j < d; j += 256) qs[j] = x[j];
    lds_barrier();

    // the thread's entries of the plain table
    float val[kLutPer];
#pragma unroll
    for (int u = 0; u < kLutPer; ++u) {
        const int e = (s * kLutPer + u) * 256 + tid;
        float acc = 0.f;
        if (e < per) {
            const float* r = qs + (e / k) * dsub;
            const float* c = cent + (long long)e * dsub;
            for (int j = 0; j < dsub; ++j) acc = acc - r[j] * c[j];
        }
        val[u] = acc;
    }

#pragma unroll 1
    for (int p0 = 0; p0 < nprobe; p0 += 256) {
        const int pn = min(256, nprobe - p0);
        if (p0) __syncthreads();   // the round before has read bias and ok
        if (tid < pn) {
            const long long l = probes[q * nprobe + p0 + tid];
            const bool good = l >= 0 && l < nlist;
            float acc = 0.f;
            if (good && s == 0) {
                const float* __restrict__ cl = coarse + l * d;
#pragma unroll 8
                for (int j = 0; j < d; ++j) acc = acc - qs[j] * cl[j];
            }
            if (!good && l != -1 && s == 0) atomicOr(err, 1ull);
            bias[tid] = acc;
            ok[tid] = good;
        }
        lds_barrier();
#pragma unroll 1
        for (int p = 0; p < pn; ++p) {
            float* __restrict__ dst = lut + (q * nprobe + p0 + p) * per;
            const bool good = ok[p];
            const float b = bias[p];
#pragma unroll
            for (int u = 0; u < kLutPer; ++u) {
                const int e = (s * kLutPer + u) * 256 + tid;
                if (e < per) dst[e] = !good ? INFINITY : e < k ? b + val[u] : val[u];
            }
        }
    }
}

// bit i of the mask = keep[perm ? perm[i] : i] != 0: one lane per row, the wave's 64 bits by a
// ballot, its two words stored by lanes 0 and 1 (the bits from n on in the last word are zero).
// A perm entry outside [0, n) reads nothing, gives a zero bit and sets the error word.
__global__ void __launch_bounds__(256)
mask_pack(const unsigned char* __restrict__ keep, const long long* __restrict__ perm, long long n,
          uint32_t* __restrict__ bits, unsigned long long* __restrict__ err) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool bit = false, bad = false;
    if (i < n) {
        const long long p = perm ? perm[i] : i;
        bad = p < 0 || p >= n;
        if (!bad) bit = keep[p] != 0;
    }
    const unsigned long long b = __ballot(bit);
    const long long w = ((i - lane) >> 5) + lane;   // lanes 0 and 1: the wave's two words
    if (lane < 2 && w < (n + 31) >> 5) bits[w] = (uint32_t)(b >> (32 * lane));
    if (__ballot(bad) && lane == 0) atomicOr(err, 1ull);
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// the entry points that come in an L2 and an inner-product form: one text, the metric picks the
// instantiation
int coarse_assign_call(bool ip, pqh_ctx_t* ctx, const pqh_coarse_t* cq, const float* d_x,
                       long long n, long long ld_x, int32_t* d_list, float* d_dist) {
    if (!ctx) return pqh_no_ctx_status();
    if (!cq || n < 0 || ld_x < cq->d || (n > 0 && (!d_x || !d_list))) return PQH_ERR_ARG;
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    if (n == 0) return PQH_OK;
    const long long blocks = (n + kTR - 1) / kTR;
    if (blocks > 0x7FFFFFFFll) return PQH_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(ip ? coarse_assign<true> : coarse_assign<false>, dim3((unsigned)blocks),
                       dim3(256), 0, ctx->stream, d_x, n, ld_x, cq->d_cent, cq->nlist, cq->d,
                       d_list, d_dist);
    PQH_LAUNCH_CHECK(ctx);
    return PQH_OK;
}

int coarse_probe_call(bool ip, pqh_ctx_t* ctx, const pqh_coarse_t* cq, const float* d_queries,
                      long long nq, long long ld_q, int nprobe, const long long* d_offsets,
                      long long* d_range_ptr, long long* d_ranges, long long* d_probes,
                      float* d_probe_dist) {
    if (!ctx) return pqh_no_ctx_status();
    if (!cq || nq < 0 || ld_q < cq->d || nprobe < 1 || nprobe > PQH_IVF_MAX_NPROBE ||
        (nq > 0 && (!d_queries || !d_offsets || !d_range_ptr || !d_ranges)))
        return PQH_ERR_ARG;
    if (nq > 0x7FFFFFFFll) return PQH_ERR_UNSUPPORTED;
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    if (nq == 0) return PQH_OK;
    hipLaunchKernelGGL(ip ? coarse_probe<true> : coarse_probe<false>, dim3((unsigned)nq),
                       dim3(64, kProbeWaves), 0, ctx->stream, d_queries, nq, ld_q, cq->d_cent_t,
                       cq->nlist, cq->d, nprobe, d_offsets, d_range_ptr, d_ranges, d_probes,
                       d_probe_dist, ctx->d_diag + kDiagIvf);
    PQH_LAUNCH_CHECK(ctx);
    return PQH_OK;
}

int adc_tables_residual_call(bool ip, pqh_ctx_t* ctx, const pqh_pq_t* pq, const pqh_coarse_t* cq,
                             const float* d_queries, long long nq, long long ld_q,
                             const long long* d_probes, int nprobe, float* d_lut) {
    if (!ctx) return pqh_no_ctx_status();
    int m = 0, k = 0, dsub = 0;
    const float* d_cent = nullptr;
    if (pqh_pq_view(pq, &m, &k, &dsub, &d_cent) || !cq || (long long)m * dsub != cq->d || nq < 0 ||
        nprobe < 1 || ld_q < cq->d || (nq > 0 && (!d_queries || !d_probes || !d_lut)))
        return PQH_ERR_ARG;
    if (k > 256 || cq->d > kResidualMaxD || nq * nprobe > 0x7FFFFFFFll) return PQH_ERR_UNSUPPORTED;
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    if (nq == 0) return PQH_OK;
    if (ip) {
        const long long slices = ((long long)m * k + kLutPer * 256 - 1) / (kLutPer * 256);
        if (slices > 65535) return PQH_ERR_UNSUPPORTED;
        hipLaunchKernelGGL(adc_lut_residual_ip, dim3((unsigned)nq, (unsigned)slices), dim3(256),
                           (size_t)cq->d * 4, ctx->stream, d_queries, ld_q, nprobe, d_probes,
                           cq->d_cent, cq->nlist, d_cent, m, k, dsub, d_lut,
                           ctx->d_diag + kDiagIvf);
    } else {
        const int vec = dsub % 4 == 0 && !(reinterpret_cast<uintptr_t>(d_cent) & 15u);
        hipLaunchKernelGGL(adc_lut_residual, dim3((unsigned)(nq * nprobe)), dim3(256),
                           (size_t)cq->d * 4, ctx->stream, d_queries, ld_q, nprobe, d_probes,
                           cq->d_cent, cq->nlist, d_cent, m, k, dsub, vec, d_lut,
                           ctx->d_diag + kDiagIvf);
    }
    PQH_LAUNCH_CHECK(ctx);
    return PQH_OK;
}

}  // namespace

int pqh_coarse_view(const pqh_coarse_t* cq, int* nlist, int* d, const float** d_cent) {
    if (!cq) return PQH_ERR_ARG;
    *nlist = cq->nlist;
    *d = cq->d;
    *d_cent = cq->d_cent;
    return PQH_OK;
}

extern "C" {

int pqh_coarse_create(pqh_ctx_t* ctx, const float* centroids, int nlist, int d, pqh_coarse_t** cq) {
    if (!ctx) return pqh_no_ctx_status();
    if (!cq) return PQH_ERR_ARG;
    *cq = nullptr;
    if (!centroids || nlist < 1 || d < 1) return PQH_ERR_ARG;
    if (nlist > PQH_IVF_MAX_NLIST || d > PQH_IVF_MAX_D) return PQH_ERR_UNSUPPORTED;
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    const size_t count = (size_t)nlist * d;
    std::vector<float> t;
    pqh_coarse* c = new (std::nothrow) pqh_coarse();
    try {
        t.resize(count);
    } catch (const std::bad_alloc&) {
        delete c;
        c = nullptr;
    }
    if (!c) return pqh_set_error(ctx, PQH_ERR_NOMEM, "coarse quantizer: host memory");
    for (int l = 0; l < nlist; ++l)
        for (int j = 0; j < d; ++j) t[(size_t)j * nlist + l] = centroids[(size_t)l * d + j];
    c->ctx = ctx;
    c->nlist = nlist;
    c->d = d;
    if (hipMalloc(&c->d_cent, count * 4) != hipSuccess ||
        hipMalloc(&c->d_cent_t, count * 4) != hipSuccess) {
        (void)hipGetLastError();
        pqh_coarse_destroy(c);
        return pqh_set_error(ctx, PQH_ERR_NOMEM, "coarse quantizer: cannot allocate %zu bytes",
                             count * 8);
    }
    if (hipMemcpy(c->d_cent, centroids, count * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(c->d_cent_t, t.data(), count * 4, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        pqh_coarse_destroy(c);
        return pqh_set_error(ctx, PQH_ERR_HIP, "coarse quantizer: upload failed");
    }
    *cq = c;
    return PQH_OK;
}

int pqh_coarse_destroy(pqh_coarse_t* cq) {
    if (!cq) return PQH_OK;
    if (cq->ctx) {
        (void)hipSetDevice(cq->ctx->device);
        (void)hipStreamSynchronize(cq->ctx->stream);   // no launch may still read them
    }
    if (cq->d_cent) (void)hipFree(cq->d_cent);
    if (cq->d_cent_t) (void)hipFree(cq->d_cent_t);
    delete cq;
    return PQH_OK;
}

int pqh_coarse_assign(pqh_ctx_t* ctx, const pqh_coarse_t* cq, const float* d_x, long long n,
                      long long ld_x, int32_t* d_list, float* d_dist) {
    return coarse_assign_call(false, ctx, cq, d_x, n, ld_x, d_list, d_dist);
}

int pqh_coarse_assign_ip(pqh_ctx_t* ctx, const pqh_coarse_t* cq, const float* d_x, long long n,
                         long long ld_x, int32_t* d_list, float* d_dist) {
    return coarse_assign_call(true, ctx, cq, d_x, n, ld_x, d_list, d_dist);
}

int pqh_ivf_layout(pqh_ctx_t* ctx, const int32_t* d_list, long long n, int nlist,
                   long long* d_perm, long long* d_offsets) {
    if (!ctx) return pqh_no_ctx_status();
    if (n < 0 || nlist < 1 || !d_offsets || (n > 0 && (!d_list || !d_perm))) return PQH_ERR_ARG;
    if (n > 0x7FFFFFFFll || nlist > PQH_IVF_MAX_NLIST) return PQH_ERR_UNSUPPORTED;
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    unsigned bits = 1;
    while ((1ll << bits) < nlist) ++bits;
    const uint32_t* keys = reinterpret_cast<const uint32_t*>(d_list);
    uint32_t* sorted = nullptr;
    if (n > 0) {
        const rocprim::counting_iterator<long long> rows(0);
        size_t temp = 0;
        if (rocprim::radix_sort_pairs(nullptr, temp, keys, (uint32_t*)nullptr, rows,
                                      (long long*)nullptr, (size_t)n, 0u, bits,
                                      ctx->stream) != hipSuccess)
            return pqh_set_error(ctx, PQH_ERR_HIP, "ivf layout: temp storage query failed");
        const size_t kb = align256((size_t)n * 4);
        rc = pqh_ensure_ws(ctx, kb + align256(temp));
        if (rc) return rc;
        sorted = static_cast<uint32_t*>(ctx->ws);
        PQH_HIP(ctx, rocprim::radix_sort_pairs(static_cast<char*>(ctx->ws) + kb, temp, keys, sorted,
                                               rows, d_perm, (size_t)n, 0u, bits, ctx->stream));
    }
    const long long threads = std::max<long long>(n, (long long)nlist + 1);
    hipLaunchKernelGGL(ivf_offsets, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0,
                       ctx->stream, d_list, sorted, n, nlist, d_offsets, ctx->d_diag + kDiagIvf);
    PQH_LAUNCH_CHECK(ctx);
    return PQH_OK;
}

int pqh_coarse_probe(pqh_ctx_t* ctx, const pqh_coarse_t* cq, const float* d_queries, long long nq,
                     long long ld_q, int nprobe, const long long* d_offsets,
                     long long* d_range_ptr, long long* d_ranges, long long* d_probes,
                     float* d_probe_dist) {
    return coarse_probe_call(false, ctx, cq, d_queries, nq, ld_q, nprobe, d_offsets, d_range_ptr,
                             d_ranges, d_probes, d_probe_dist);
}

int pqh_coarse_probe_ip(pqh_ctx_t* ctx, const pqh_coarse_t* cq, const float* d_queries,
                        long long nq, long long ld_q, int nprobe, const long long* d_offsets,
                        long long* d_range_ptr, long long* d_ranges, long long* d_probes,
                        float* d_probe_dist) {
    return coarse_probe_call(true, ctx, cq, d_queries, nq, ld_q, nprobe, d_offsets, d_range_ptr,
                             d_ranges, d_probes, d_probe_dist);
}

int pqh_ivf_residuals(pqh_ctx_t* ctx, const pqh_coarse_t* cq, const float* d_x, long long n,
                      long long ld_x, const int32_t* d_list, const long long* d_perm, float* d_out,
                      long long ld_out) {
    if (!ctx) return pqh_no_ctx_status();
    if (!cq || n < 0 || ld_x < cq->d || ld_out < cq->d || (n > 0 && (!d_x || !d_list || !d_out)))
        return PQH_ERR_ARG;
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    if (n == 0) return PQH_OK;
    const long long blocks = (n + 8 * kResRows - 1) / (8 * kResRows);
    if (blocks > 0x7FFFFFFFll) return PQH_ERR_UNSUPPORTED;
    // float4 steps where every row of x, out and the centroids starts on 16 bytes
    const bool vec = cq->d % 4 == 0 && ld_x % 4 == 0 && ld_out % 4 == 0 &&
                     !((reinterpret_cast<uintptr_t>(d_x) | reinterpret_cast<uintptr_t>(d_out) |
                        reinterpret_cast<uintptr_t>(cq->d_cent)) & 15u);
    hipLaunchKernelGGL(vec ? ivf_residual<true> : ivf_residual<false>, dim3((unsigned)blocks),
                       dim3(256), 0, ctx->stream, d_x, n, ld_x, d_list, d_perm, cq->d_cent,
                       cq->nlist, cq->d, d_out, ld_out, ctx->d_diag + kDiagIvf);
    PQH_LAUNCH_CHECK(ctx);
    return PQH_OK;
}

int pqh_adc_tables_residual(pqh_ctx_t* ctx, const pqh_pq_t* pq, const pqh_coarse_t* cq,
                            const float* d_queries, long long nq, long long ld_q,
                            const long long* d_probes, int nprobe, float* d_lut) {
    return adc_tables_residual_call(false, ctx, pq, cq, d_queries, nq, ld_q, d_probes, nprobe,
                                    d_lut);
}

int pqh_adc_tables_residual_ip(pqh_ctx_t* ctx, const pqh_pq_t* pq, const pqh_coarse_t* cq,
                               const float* d_queries, long long nq, long long ld_q,
                               const long long* d_probes, int nprobe, float* d_lut) {
    return adc_tables_residual_call(true, ctx, pq, cq, d_queries, nq, ld_q, d_probes, nprobe,
                                    d_lut);
}

int pqh_mask_pack(pqh_ctx_t* ctx, const unsigned char* d_keep, const long long* d_perm, long long n,
                  unsigned int* d_bits) {
    if (!ctx) return pqh_no_ctx_status();
    if (n < 0 || (n > 0 && (!d_keep || !d_bits)) || (reinterpret_cast<uintptr_t>(d_bits) & 3u))
        return PQH_ERR_ARG;
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    if (n == 0) return PQH_OK;
    const long long blocks = (n + 255) / 256;
    if (blocks > 0x7FFFFFFFll) return PQH_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(mask_pack, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, d_keep, d_perm,
                       n, d_bits, ctx->d_diag + kDiagIvf);
    PQH_LAUNCH_CHECK(ctx);
    return PQH_OK;
}

int pqh_ivf_status(pqh_ctx_t* ctx) {
    if (!ctx) return pqh_no_ctx_status();
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    unsigned long long e = 0;
    PQH_HIP(ctx, hipMemcpyAsync(&e, ctx->d_diag + kDiagIvf, 8, hipMemcpyDeviceToHost, ctx->stream));
    PQH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (e) PQH_HIP(ctx, hipMemsetAsync(ctx->d_diag + kDiagIvf, 0, 8, ctx->stream));   // (sticky until read)
    return e ? PQH_ERR_ARG : PQH_OK;
}

}  // extern "C"
