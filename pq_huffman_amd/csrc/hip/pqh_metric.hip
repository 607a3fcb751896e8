// pqh_metric.hip -- the inner-product metric around the ADC scan: the tables, the coarse
// assignment, the probe selection and the per-probe tables of a residual index.  The scan, the
// top-k lists, the radius compare and the mask order plain fp32 values with `<`, so a score is
// the NEGATED inner product and "smaller is nearer" holds as it does for L2:
//   nip(x, y) = acc,  acc = +0.0f;  for j ascending:  acc = acc - x[j] * y[j]
// one fp32 multiply and one fp32 subtract per element, no contraction, no final negation.
//
//  adc_lut_ip        lut[q][i][c] = nip(q_i, cent[i][c]), one thread per entry, as adc_lut.
//  coarse_assign_ip  list[v] = the first l that minimises nip(x[v], c[l]): coarse_assign's
//                    tiling (128 rows x 128 centroids x 32 staged dimensions, 8 x 8 sums a
//                    thread, the same staging and the same combine by (score, list)), two
//                    operations per element where the L2 form has three.
//  coarse_probe_ip   coarse_probe's shape (16 waves, 1,024 lists a round, lane = list over the
//                    transposed centroids, the wave-wide list of pqh_topk_dev.h) with the score
//                    of this file.
//  adc_lut_residual_ip  one table per (query, probed list) for the *_range_tables and *_lists
//                    scans.  <q, c[l] + r> = <q, c[l]> + <q, r>: the second term is the plain
//                    table of the query, the same for every probe, the first one number per
//                    probe.  That number is folded into part 0 of the probe's table
//                    (bias + entry, one add), so the scan's sum over the parts carries it
//                    without a new scan form.  A workgroup owns a query and kLutPer * 256 table
//                    entries: it computes their plain values once, keeps them in registers and
//                    writes them nprobe times; the workgroups of part 0 first run the d-long
//                    bias chains, one probe a thread, the query staged in LDS.
#include <cmath>

#include "pqh_internal.h"
#include "pqh_topk_dev.h"

namespace {

// ------------------------------------------------------------------- the tables
__global__ void __launch_bounds__(256)
adc_lut_ip(const float* __restrict__ queries, long long nq, long long ld_q,
           const float* __restrict__ cent, int m, int k, int dsub, float* __restrict__ lut) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long per = (long long)m * k;
    if (idx >= nq * per) return;
    const long long q = idx / per;
    const int e = (int)(idx - q * per);   // i * k + c
    const float* x = queries + q * ld_q + (long long)(e / k) * dsub;
    const float* c = cent + (long long)e * dsub;
    float acc = 0.f;
    for (int j = 0; j < dsub; ++j) acc = acc - x[j] * c[j];
    lut[idx] = acc;
}

// ------------------------------------------------------------------- the assignment
constexpr int kTR = 128;            // rows of a workgroup
constexpr int kTC = 128;            // centroids of a tile
constexpr int kJT = 32;             // dimensions staged at a time
constexpr int kR = 8, kC = 8;       // a thread's block of sums
constexpr int kStride = kTR + 4;    // floats between two dimensions of a staged tile
static_assert(kTR == kTC && kTR == 16 * kR && kTC == 16 * kC, "256 threads as 16 x 16");

__global__ void __launch_bounds__(256, 2)
coarse_assign_ip(const float* __restrict__ x, long long n, long long ld_x,
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
            // nothing past d, n or nlist is read: the index is held at the last dimension, row
            // and centroid instead, and what those slots hold is never summed (j >= jn), never
            // stored (row >= n) or never compared (list >= nlist)
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
                    for (int c = 0; c < kC; ++c) acc[r][c] = acc[r][c] - xv[r] * cv[c];
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

    // the 16 threads of a row are 16 neighbouring lanes: the smallest by (score, list)
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

// ------------------------------------------------------------------- the probe selection
constexpr int kProbeWaves = 16;
__global__ void __launch_bounds__(64 * kProbeWaves)
coarse_probe_ip(const float* __restrict__ queries, long long nq, long long ld_q,
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
        for (int j = 0; j < d; ++j) acc = acc - x[j] * c[(long long)j * nlist];
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

// ------------------------------------------------------------------- the residual tables
// Workgroup (q, s): query q, the table entries [s * kLutPer * 256, (s + 1) * kLutPer * 256).
// K <= 256 <= kLutPer * 256, so part 0 lies in the workgroups s == 0 and only they need the
// biases.  The probes go through LDS 256 at a time (nprobe has no upper bound here): thread t
// of a round owns probe p0 + t, runs its chain (s == 0) and leaves (bias, valid) for the
// workgroup, which then writes that round's tables, a wave storing 64 consecutive floats.
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

}  // namespace

extern "C" {

int pqh_adc_tables_ip(pqh_ctx_t* ctx, const pqh_pq_t* pq, const float* d_queries, long long nq,
                      long long ld_q, float* d_lut) {
    if (!ctx) return pqh_no_ctx_status();
    int m = 0, k = 0, dsub = 0;
    const float* d_cent = nullptr;
    if (pqh_pq_view(pq, &m, &k, &dsub, &d_cent) || nq < 0 || ld_q < (long long)m * dsub ||
        (nq > 0 && (!d_queries || !d_lut)))
        return PQH_ERR_ARG;
    if (k > 256) return PQH_ERR_UNSUPPORTED;
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    if (nq == 0) return PQH_OK;
    const long long blocks = (nq * m * k + 255) / 256;
    if (blocks > 0x7FFFFFFFll) return PQH_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(adc_lut_ip, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, d_queries,
                       nq, ld_q, d_cent, m, k, dsub, d_lut);
    PQH_LAUNCH_CHECK(ctx);
    return PQH_OK;
}

int pqh_coarse_assign_ip(pqh_ctx_t* ctx, const pqh_coarse_t* cq, const float* d_x, long long n,
                         long long ld_x, int32_t* d_list, float* d_dist) {
    if (!ctx) return pqh_no_ctx_status();
    int nlist = 0, d = 0;
    const float* d_cent = nullptr;
    if (pqh_coarse_view(cq, &nlist, &d, &d_cent) || n < 0 || ld_x < d ||
        (n > 0 && (!d_x || !d_list)))
        return PQH_ERR_ARG;
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    if (n == 0) return PQH_OK;
    const long long blocks = (n + kTR - 1) / kTR;
    if (blocks > 0x7FFFFFFFll) return PQH_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(coarse_assign_ip, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, d_x, n,
                       ld_x, d_cent, nlist, d, d_list, d_dist);
    PQH_LAUNCH_CHECK(ctx);
    return PQH_OK;
}

int pqh_coarse_probe_ip(pqh_ctx_t* ctx, const pqh_coarse_t* cq, const float* d_queries,
                        long long nq, long long ld_q, int nprobe, const long long* d_offsets,
                        long long* d_range_ptr, long long* d_ranges, long long* d_probes,
                        float* d_probe_dist) {
    if (!ctx) return pqh_no_ctx_status();
    int nlist = 0, d = 0;
    const float *d_cent = nullptr, *d_cent_t = nullptr;
    if (pqh_coarse_view(cq, &nlist, &d, &d_cent) || pqh_coarse_view_t(cq, &d_cent_t) || nq < 0 ||
        ld_q < d || nprobe < 1 || nprobe > PQH_IVF_MAX_NPROBE ||
        (nq > 0 && (!d_queries || !d_offsets || !d_range_ptr || !d_ranges)))
        return PQH_ERR_ARG;
    if (nq > 0x7FFFFFFFll) return PQH_ERR_UNSUPPORTED;
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    if (nq == 0) return PQH_OK;
    hipLaunchKernelGGL(coarse_probe_ip, dim3((unsigned)nq), dim3(64, kProbeWaves), 0, ctx->stream,
                       d_queries, nq, ld_q, d_cent_t, nlist, d, nprobe, d_offsets, d_range_ptr,
                       d_ranges, d_probes, d_probe_dist, ctx->d_diag + kDiagIvf);
    PQH_LAUNCH_CHECK(ctx);
    return PQH_OK;
}

int pqh_adc_tables_residual_ip(pqh_ctx_t* ctx, const pqh_pq_t* pq, const pqh_coarse_t* cq,
                               const float* d_queries, long long nq, long long ld_q,
                               const long long* d_probes, int nprobe, float* d_lut) {
    if (!ctx) return pqh_no_ctx_status();
    int m = 0, k = 0, dsub = 0, nlist = 0, d = 0;
    const float *d_cent = nullptr, *d_coarse = nullptr;
    if (pqh_pq_view(pq, &m, &k, &dsub, &d_cent) || pqh_coarse_view(cq, &nlist, &d, &d_coarse) ||
        (long long)m * dsub != d || nq < 0 || nprobe < 1 || ld_q < d ||
        (nq > 0 && (!d_queries || !d_probes || !d_lut)))
        return PQH_ERR_ARG;
    if (k > 256 || d > PQH_ADC_RESIDUAL_MAX_D || nq * nprobe > 0x7FFFFFFFll)
        return PQH_ERR_UNSUPPORTED;
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    if (nq == 0) return PQH_OK;
    const long long slices = ((long long)m * k + kLutPer * 256 - 1) / (kLutPer * 256);
    if (slices > 65535) return PQH_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(adc_lut_residual_ip, dim3((unsigned)nq, (unsigned)slices), dim3(256),
                       (size_t)d * 4, ctx->stream, d_queries, ld_q, nprobe, d_probes, d_coarse,
                       nlist, d_cent, m, k, dsub, d_lut, ctx->d_diag + kDiagIvf);
    PQH_LAUNCH_CHECK(ctx);
    return PQH_OK;
}

}  // extern "C"
