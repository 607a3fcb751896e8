// pqh_refine.hip -- the re-rank of a search's candidates with a second, finer code
// (pqh_refine_stream, pqh_refine_codes): a row is stored twice, as the PQ code `a` of the
// vector (level 1) and as the PQ code `b` of what level 1 left over (level 2), and
//   dist(q, r) = sum_j (q[j] - (c1[a][j] + c2[b][j]))^2      (residual index: q - c[list(r)])
// in fp32, one add, one (or two) subtracts, one multiply and one add per dimension, j ascending
// over the whole vector, no contraction.
// The inner-product form (pqh_refine_*_ip, the IP instantiations) scores the same candidates by
//   nip(q, r) = acc,  acc = +0;  acc = acc - q[j] * (c1[a][j] + c2[b][j])
// (residual index: c[list(r)][j] + (c1[a][j] + c2[b][j])), the negated inner product of
// pqh_ivf.hip's header, one chain over d; decode, select and errors are shared with the L2 form.
//
//  refine_rows   one workgroup of two waves per query, one candidate per lane.
//                Decode: wave 0 reaches the lane's row of the level-1 stream and wave 1 the same
//                row of the level-2 stream, each as sel_rows (pqh_decode.hip) does: SelRd on the
//                global stream from the chunk's bit offset, in the chunk's stored context, the
//                rows of the chunk up to the one asked for through walk_parts (the context flag
//                is a run-time value, so one instantiation serves every shape).  The two walks
//                are independent, so a candidate costs the longer of them.  Over plain codes the
//                waves copy their level's row instead.  The code rows land in LDS.
//                Distance: wave 0, after the barrier.  The query row is staged in LDS; the
//                centroids (and the list's coarse centroid) are read from global memory, 16
//                bytes at a time where every sub-vector is a multiple of four floats.  The loads
//                do not depend on the running sum; the adds are one chain.
//                Select: list_merge<false> on an empty list sorts the wave's 64 (dist, row)
//                keys; the lanes below top_k store.
//                Errors are sel_rows': bit 1 for a chunk offset or a symbol past the stream or
//                an invalid code (the candidate takes no part), bit 2 for a row outside [0, n)
//                but the padding -1 (or a row past the last list of a residual index).
//  refine_rows_wide  the same for 64 < ncand <= 256 (a context whose limit was raised): a wave
//                pair per 64 candidates, up to eight waves, the keys sorted through the wide
//                list of pqh_topk_dev.h.
#include <cmath>

#include "pqh_decode_dev.h"
#include "pqh_topk_dev.h"

namespace {

constexpr int kRowStride = 20;   // bytes between two lanes' code rows in LDS (16 codes; 5 dwords:
                                 // odd, so the lanes' rows start on different banks)

// one level of the two: its stream and chunk index (or its plain codes) and its codebook
struct Level {
    const uint32_t* words;
    long long nwords;
    const unsigned long long* chunk_off;
    const uint8_t* chunk_prev;
    const uint8_t* codes;   // [n][m], the plain form
    const float* cent;      // [m][k][dsub]
    DecTabs T;
    int raw_first, chunk_vectors, ctx, m, k, dsub;
};
struct Levels {
    Level lv[2];
};

// row v of a level into `row`: false if it cannot be reached (a chunk offset or a symbol past
// the stream, an invalid code)
template <bool STREAM>
__device__ __forceinline__ bool level_row(const Level& L, long long v, uint8_t* row) {
    const int m = L.m;
    bool good = true;
    if constexpr (STREAM) {
        const long long j = v / L.chunk_vectors;
        const int steps = (int)(v - j * L.chunk_vectors) + 1;
        const bool ctx = L.ctx != 0;
        const bool raw = ctx && j == 0 && L.raw_first;
        SelRd rd;
        good = rd.init(L.words, L.nwords, L.chunk_off[j]);
        if (good) {
            for (int i = 0; i < m; ++i) row[i] = (ctx && !raw) ? L.chunk_prev[j * m + i] : (uint8_t)0;
            good = walk_parts<0>(rd.br, L.T, m, ctx, raw, steps,
                                 [&](int i) -> uint8_t& { return row[i]; }, [](int) {});
            good = good && rd.pos() <= (unsigned long long)L.nwords * 32;
        }
    } else {
        for (int i = 0; i < m; ++i) row[i] = L.codes[v * m + i];
    }
    // (a raw first row, a stored context row and plain codes are bytes nobody has checked)
    for (int i = 0; good && i < m; ++i) good = row[i] < L.k;
    return good;
}

template <bool STREAM, bool IP>
__global__ void __launch_bounds__(128)
refine_rows(Levels P, long long n, const float* __restrict__ coarse, int nlist,
            const long long* __restrict__ offsets, const float* __restrict__ queries,
            long long ld_q, const long long* __restrict__ rows, int ncand, int top_k,
            float* __restrict__ dist, long long* __restrict__ ids, long long ld_out,
            unsigned long long* __restrict__ err) {
    extern __shared__ __attribute__((aligned(16))) float qs[];   // the query row, d floats
    __shared__ __attribute__((aligned(4))) uint8_t code[2][64 * kRowStride];
    __shared__ unsigned char dead[2][64];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long q = blockIdx.x;
    const int d = P.lv[0].m * P.lv[0].dsub;
    const float* __restrict__ qrow = queries + q * ld_q;
    for (int j = threadIdx.x; j < d; j += 128) qs[j] = qrow[j];

    // ---- decode: wave w walks level w
    const long long v = lane < ncand ? rows[q * ncand + lane] : -1;
    const bool inside = v >= 0 && v < n;
    unsigned flag = (v < -1 || v >= n) ? 2u : 0u;
    bool good = false;
    if (inside) {
        const Level L = w ? P.lv[1] : P.lv[0];
        good = level_row<STREAM>(L, v, &code[w][lane * kRowStride]);
        if (!good) flag = 1;
    }
    dead[w][lane] = good ? 0 : 1;
    if (flag && (w == 0 || flag == 1)) atomicOr(err, (unsigned long long)flag);
    lds_barrier();
    if (w) return;

    // ---- distance: one chain over the d dimensions
    bool valid = inside && !dead[0][lane] && !dead[1][lane];
    const float* __restrict__ cl = nullptr;   // residual index: the centroid of the row's list
    if (coarse && valid) {
        // the last list with offsets[l] <= v: the entries of offsets[1 ... nlist] that are <= v
        int lo = 0, hi = nlist;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (offsets[1 + mid] <= v) lo = mid + 1; else hi = mid;
        }
        if (lo >= nlist) {   // (a row past the last list: the offsets do not cover the stream)
            valid = false;
            atomicOr(err, 2ull);
        }
        cl = coarse + (long long)lo * d;
    }
    float acc = 0.f;
    if (valid) {
        const uint8_t* a = &code[0][lane * kRowStride];
        const uint8_t* b = &code[1][lane * kRowStride];
        const int ds1 = P.lv[0].dsub, ds2 = P.lv[1].dsub;
        const long long k1 = P.lv[0].k, k2 = P.lv[1].k;
        const float* __restrict__ cent1 = P.lv[0].cent;
        const float* __restrict__ cent2 = P.lv[1].cent;
        const bool vec = !((ds1 | ds2) & 3) &&
                         !((reinterpret_cast<uintptr_t>(cent1) | reinterpret_cast<uintptr_t>(cent2) |
                            reinterpret_cast<uintptr_t>(coarse)) & 15u);
        int i1 = 0, j1 = 0, i2 = 0, j2 = 0;
        const float* c1 = cent1 + (long long)a[0] * ds1;
        const float* c2 = cent2 + (long long)b[0] * ds2;
        if (vec) {   // every sub-vector a multiple of four floats: the same sum, 16-byte loads
            for (int j = 0; j < d; j += 4) {
                const float4 u1 = *reinterpret_cast<const float4*>(c1 + j1);
                const float4 u2 = *reinterpret_cast<const float4*>(c2 + j2);
                float4 x = *reinterpret_cast<const float4*>(qs + j);
                if constexpr (IP) {
                    float4 y = make_float4(u1.x + u2.x, u1.y + u2.y, u1.z + u2.z, u1.w + u2.w);
                    if (cl) {
                        const float4 cv = *reinterpret_cast<const float4*>(cl + j);
                        y = make_float4(cv.x + y.x, cv.y + y.y, cv.z + y.z, cv.w + y.w);
                    }
                    acc = acc - x.x * y.x;
                    acc = acc - x.y * y.y;
                    acc = acc - x.z * y.z;
                    acc = acc - x.w * y.w;
                } else {
                    if (cl) {
                        const float4 cv = *reinterpret_cast<const float4*>(cl + j);
                        x = make_float4(x.x - cv.x, x.y - cv.y, x.z - cv.z, x.w - cv.w);
                    }
                    const float t0 = x.x - (u1.x + u2.x), t1 = x.y - (u1.y + u2.y),
                                t2 = x.z - (u1.z + u2.z), t3 = x.w - (u1.w + u2.w);
                    acc = acc + t0 * t0;
                    acc = acc + t1 * t1;
                    acc = acc + t2 * t2;
                    acc = acc + t3 * t3;
                }
                j1 += 4;
                j2 += 4;
                if (j1 == ds1 && j + 4 < d) ++i1, c1 = cent1 + (i1 * k1 + a[i1]) * ds1, j1 = 0;
                if (j2 == ds2 && j + 4 < d) ++i2, c2 = cent2 + (i2 * k2 + b[i2]) * ds2, j2 = 0;
            }
        } else {
            for (int j = 0; j < d; ++j) {
                float y = c1[j1] + c2[j2];
                float x = qs[j];
                if constexpr (IP) {
                    if (cl) y = cl[j] + y;
                    acc = acc - x * y;
                } else {
                    if (cl) x = x - cl[j];
                    const float t = x - y;
                    acc = acc + t * t;
                }
                if (++j1 == ds1 && j + 1 < d) ++i1, c1 = cent1 + (i1 * k1 + a[i1]) * ds1, j1 = 0;
                if (++j2 == ds2 && j + 1 < d) ++i2, c2 = cent2 + (i2 * k2 + b[i2]) * ds2, j2 = 0;
            }
        }
    }

    // ---- select: the wave's 64 keys sorted by (dist, row)
    TopK e{INFINITY, -1};
    list_merge<false>(e, valid ? TopK{acc, v} : TopK{INFINITY, 0x7FFFFFFFFFFFFFFFll});
    if (lane < top_k) {
        dist[q * ld_out + lane] = e.d;
        ids[q * ld_out + lane] = e.id;
    }
}

// refine_rows' distance phase for the wide kernel (refine_rows keeps its own text, and so its
// code): the distance of candidate row v, its code rows a and b in LDS, one chain over the d
// dimensions.  *valid is cleared (and error bit 2 set) for a row past the last list of a
// residual index.
template <bool IP>
__device__ __forceinline__ float cand_dist(const Levels& P, const float* coarse, int nlist,
                                           const long long* offsets, const float* qs, int d,
                                           long long v, const uint8_t* a, const uint8_t* b,
                                           bool& valid, unsigned long long* err) {
    const float* __restrict__ cl = nullptr;   // residual index: the centroid of the row's list
    if (coarse && valid) {
        // the last list with offsets[l] <= v: the entries of offsets[1 ... nlist] that are <= v
        int lo = 0, hi = nlist;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (offsets[1 + mid] <= v) lo = mid + 1; else hi = mid;
        }
        if (lo >= nlist) {   // (a row past the last list: the offsets do not cover the stream)
            valid = false;
            atomicOr(err, 2ull);
        }
        cl = coarse + (long long)lo * d;
    }
    float acc = 0.f;
    if (valid) {
        const int ds1 = P.lv[0].dsub, ds2 = P.lv[1].dsub;
        const long long k1 = P.lv[0].k, k2 = P.lv[1].k;
        const float* __restrict__ cent1 = P.lv[0].cent;
        const float* __restrict__ cent2 = P.lv[1].cent;
        const bool vec = !((ds1 | ds2) & 3) &&
                         !((reinterpret_cast<uintptr_t>(cent1) | reinterpret_cast<uintptr_t>(cent2) |
                            reinterpret_cast<uintptr_t>(coarse)) & 15u);
        int i1 = 0, j1 = 0, i2 = 0, j2 = 0;
        const float* c1 = cent1 + (long long)a[0] * ds1;
        const float* c2 = cent2 + (long long)b[0] * ds2;
        if (vec) {   // every sub-vector a multiple of four floats: the same sum, 16-byte loads
            for (int j = 0; j < d; j += 4) {
                const float4 u1 = *reinterpret_cast<const float4*>(c1 + j1);
                const float4 u2 = *reinterpret_cast<const float4*>(c2 + j2);
                float4 x = *reinterpret_cast<const float4*>(qs + j);
                if constexpr (IP) {
                    float4 y = make_float4(u1.x + u2.x, u1.y + u2.y, u1.z + u2.z, u1.w + u2.w);
                    if (cl) {
                        const float4 cv = *reinterpret_cast<const float4*>(cl + j);
                        y = make_float4(cv.x + y.x, cv.y + y.y, cv.z + y.z, cv.w + y.w);
                    }
                    acc = acc - x.x * y.x;
                    acc = acc - x.y * y.y;
                    acc = acc - x.z * y.z;
                    acc = acc - x.w * y.w;
                } else {
                    if (cl) {
                        const float4 cv = *reinterpret_cast<const float4*>(cl + j);
                        x = make_float4(x.x - cv.x, x.y - cv.y, x.z - cv.z, x.w - cv.w);
                    }
                    const float t0 = x.x - (u1.x + u2.x), t1 = x.y - (u1.y + u2.y),
                                t2 = x.z - (u1.z + u2.z), t3 = x.w - (u1.w + u2.w);
                    acc = acc + t0 * t0;
                    acc = acc + t1 * t1;
                    acc = acc + t2 * t2;
                    acc = acc + t3 * t3;
                }
                j1 += 4;
                j2 += 4;
                if (j1 == ds1 && j + 4 < d) ++i1, c1 = cent1 + (i1 * k1 + a[i1]) * ds1, j1 = 0;
                if (j2 == ds2 && j + 4 < d) ++i2, c2 = cent2 + (i2 * k2 + b[i2]) * ds2, j2 = 0;
            }
        } else {
            for (int j = 0; j < d; ++j) {
                float y = c1[j1] + c2[j2];
                float x = qs[j];
                if constexpr (IP) {
                    if (cl) y = cl[j] + y;
                    acc = acc - x * y;
                } else {
                    if (cl) x = x - cl[j];
                    const float t = x - y;
                    acc = acc + t * t;
                }
                if (++j1 == ds1 && j + 1 < d) ++i1, c1 = cent1 + (i1 * k1 + a[i1]) * ds1, j1 = 0;
                if (++j2 == ds2 && j + 1 < d) ++i2, c2 = cent2 + (i2 * k2 + b[i2]) * ds2, j2 = 0;
            }
        }
    }
    return acc;
}

// refine_rows for 64 < ncand <= 256: a wave pair per 64 candidates, so the pairs' row walks --
// the whole cost over streams -- run side by side.  Wave 2p walks level 1 and wave 2p + 1 level
// 2 of candidates [64p, 64p + 64); the even waves then compute their candidates' distances
// (the same one chain), and wave 0 sorts the workgroup's keys through the wide list.  The
// workgroup has 2 * ceil(ncand / 64) waves.
constexpr int kWidePairs = PQH_SEARCH_MAX_K_WIDE / 64;
static_assert(kWidePairs == kWideKR, "the wide list holds the candidates of every pair");
template <bool STREAM, bool IP>
__global__ void __launch_bounds__(128 * kWidePairs)
refine_rows_wide(Levels P, long long n, const float* __restrict__ coarse, int nlist,
                 const long long* __restrict__ offsets, const float* __restrict__ queries,
                 long long ld_q, const long long* __restrict__ rows, int ncand, int top_k,
                 float* __restrict__ dist, long long* __restrict__ ids, long long ld_out,
                 unsigned long long* __restrict__ err) {
    extern __shared__ __attribute__((aligned(16))) float qs[];   // the query row, d floats
    __shared__ __attribute__((aligned(4))) uint8_t code[2][64 * kWidePairs * kRowStride];
    __shared__ unsigned char dead[2][64 * kWidePairs];
    __shared__ float key_d[64 * kWidePairs];
    __shared__ long long key_id[64 * kWidePairs];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lv = w & 1;
    const int c = (w >> 1) * 64 + lane;   // the candidate: below 64 * pairs, the workgroup's waves
    const long long q = blockIdx.x;
    const int d = P.lv[0].m * P.lv[0].dsub;
    const float* __restrict__ qrow = queries + q * ld_q;
    for (int j = threadIdx.x; j < d; j += (int)blockDim.x) qs[j] = qrow[j];

    // ---- decode: wave 2p + l walks level l
    const long long v = c < ncand ? rows[q * ncand + c] : -1;
    const bool inside = v >= 0 && v < n;
    unsigned flag = (v < -1 || v >= n) ? 2u : 0u;
    bool good = false;
    if (inside) {
        const Level L = lv ? P.lv[1] : P.lv[0];
        good = level_row<STREAM>(L, v, &code[lv][c * kRowStride]);
        if (!good) flag = 1;
    }
    dead[lv][c] = good ? 0 : 1;
    if (flag && (lv == 0 || flag == 1)) atomicOr(err, (unsigned long long)flag);
    lds_barrier();

    // ---- distance: the even waves, one chain over the d dimensions each
    if (lv == 0) {
        bool valid = inside && !dead[0][c] && !dead[1][c];
        const float acc = cand_dist<IP>(P, coarse, nlist, offsets, qs, d, v, &code[0][c * kRowStride],
                                    &code[1][c * kRowStride], valid, err);
        key_d[c] = valid ? acc : INFINITY;
        key_id[c] = valid ? v : 0x7FFFFFFFFFFFFFFFll;
    }
    lds_barrier();
    if (w) return;

    // ---- select: the pairs' keys, 64 at a time, into the wide list
    const int kth = ncand - 1;
    TopKW e;
    list_clear(e);
#pragma unroll 1
    for (int b = 0; b <= (kth >> 6); ++b)
        list_merge<false>(e, TopK{key_d[b * 64 + lane], key_id[b * 64 + lane]}, kth);
#pragma unroll
    for (int b = 0; b < kWideKR; ++b) {
        if (b * 64 + lane < top_k) {
            dist[q * ld_out + b * 64 + lane] = e.d[b];
            ids[q * ld_out + b * 64 + lane] = e.id[b];
        }
    }
}

// the arguments of one level as the entry points take them
struct LevelArgs {
    const pqh_tables_t* t;
    const pqh_pq_t* pq;
    const unsigned char* stream;
    unsigned long long stream_bytes;
    int raw_first, chunk_vectors;
    const unsigned long long* chunk_off;
    const void* chunk_prev;
    const void* codes;
};

// PQH_ERR_ARG / PQH_ERR_UNSUPPORTED, or the level as the kernel sees it
int level_of(const LevelArgs& a, bool stream, long long n, bool run, Level* L) {
    int m = 0, k = 0, dsub = 0;
    const float* cent = nullptr;
    if (pqh_pq_view(a.pq, &m, &k, &dsub, &cent)) return PQH_ERR_ARG;
    *L = Level{};
    L->cent = cent;
    L->m = m;
    L->k = k;
    L->dsub = dsub;
    if (stream) {
        const pqh_tables_t* t = a.t;
        if (!t || t->m != m || t->k != k || a.chunk_vectors < 1) return PQH_ERR_ARG;
        if (run && n > 0 && (!a.stream || !a.chunk_off || a.stream_bytes < 4)) return PQH_ERR_ARG;
        if (reinterpret_cast<uintptr_t>(a.stream) & 3u) return PQH_ERR_ARG;
        if (t->context && !a.chunk_prev && (!a.raw_first || n > a.chunk_vectors)) return PQH_ERR_ARG;
        if (a.stream_bytes / 4 >= (1ull << 58)) return PQH_ERR_UNSUPPORTED;
        L->words = reinterpret_cast<const uint32_t*>(a.stream);
        L->nwords = (long long)(a.stream_bytes / 4);
        L->chunk_off = a.chunk_off;
        L->chunk_prev = static_cast<const uint8_t*>(a.chunk_prev);
        L->T = dec_tabs(t, 0);
        L->raw_first = a.raw_first;
        L->chunk_vectors = a.chunk_vectors;
        L->ctx = t->context;
    } else {
        if (run && n > 0 && !a.codes) return PQH_ERR_ARG;
        L->codes = static_cast<const uint8_t*>(a.codes);
    }
    if (m > 16 || k > 256) return PQH_ERR_UNSUPPORTED;
    return PQH_OK;
}

template <bool IP>
int refine(pqh_ctx_t* ctx, bool stream, const LevelArgs& a1, const LevelArgs& a2, long long n,
           const pqh_coarse_t* cq, const long long* d_offsets, const float* d_queries, long long nq,
           long long ld_q, const long long* d_rows, int ncand, int top_k, float* d_dist,
           long long* d_ids, long long ld_out) {
    if (!ctx) return pqh_no_ctx_status();
    if (n < 0 || nq < 0 || ncand < 1 || ncand > ctx->search_max_k || top_k < 1 || top_k > ncand ||
        ld_out < top_k || (cq != nullptr) != (d_offsets != nullptr))
        return PQH_ERR_ARG;
    const bool run = nq > 0;
    if (run && (!d_queries || !d_rows || !d_dist || !d_ids)) return PQH_ERR_ARG;
    Levels P;
    int rc = level_of(a1, stream, n, run, &P.lv[0]);
    if (rc == PQH_ERR_ARG) return rc;
    const int rc2 = level_of(a2, stream, n, run, &P.lv[1]);
    if (rc2 == PQH_ERR_ARG) return rc2;
    const long long d = (long long)P.lv[0].m * P.lv[0].dsub;
    if (d != (long long)P.lv[1].m * P.lv[1].dsub || ld_q < d) return PQH_ERR_ARG;
    int nlist = 0, dc = 0;
    const float* d_coarse = nullptr;
    if (cq && (pqh_coarse_view(cq, &nlist, &dc, &d_coarse) || dc != d)) return PQH_ERR_ARG;
    if (rc || rc2) return rc ? rc : rc2;
    // (the query row is staged in LDS, as the residual tables' is)
    if (d > PQH_ADC_RESIDUAL_MAX_D || nq > 0x7FFFFFFFll) return PQH_ERR_UNSUPPORTED;
    rc = pqh_use_device(ctx);
    if (rc) return rc;
    if (!run) return PQH_OK;
    // (no memset: d_diag[1] is sticky until pqh_decode_status reads it)
    const size_t lds = (size_t)d * 4;
    const bool wide = ncand > PQH_SEARCH_MAX_K;   // a wave pair per 64 candidates
    const dim3 block(wide ? 128 * ((ncand + 63) / 64) : 128);
    // (a name with a comma in it is two arguments to the launch macro: the parentheses)
    if (stream)
        hipLaunchKernelGGL((wide ? refine_rows_wide<true, IP> : refine_rows<true, IP>),
                           dim3((unsigned)nq), block, lds, ctx->stream, P, n, d_coarse, nlist,
                           d_offsets, d_queries, ld_q, d_rows, ncand, top_k, d_dist, d_ids, ld_out,
                           ctx->d_diag + 1);
    else
        hipLaunchKernelGGL((wide ? refine_rows_wide<false, IP> : refine_rows<false, IP>),
                           dim3((unsigned)nq), block, lds, ctx->stream, P, n, d_coarse, nlist,
                           d_offsets, d_queries, ld_q, d_rows, ncand, top_k, d_dist, d_ids, ld_out,
                           ctx->d_diag + 1);
    PQH_LAUNCH_CHECK(ctx);
    return PQH_OK;
}

}  // namespace

extern "C" {

int pqh_refine_stream(pqh_ctx_t* ctx, const pqh_tables_t* t1, const pqh_pq_t* pq1,
                      const unsigned char* d_stream1, unsigned long long stream_bytes1,
                      int raw_first1, int chunk_vectors1,
                      const unsigned long long* d_chunk_offsets1, const void* d_chunk_prev1,
                      const pqh_tables_t* t2, const pqh_pq_t* pq2, const unsigned char* d_stream2,
                      unsigned long long stream_bytes2, int raw_first2, int chunk_vectors2,
                      const unsigned long long* d_chunk_offsets2, const void* d_chunk_prev2,
                      long long n, const pqh_coarse_t* cq, const long long* d_offsets,
                      const float* d_queries, long long nq, long long ld_q,
                      const long long* d_rows, int ncand, int top_k, float* d_dist,
                      long long* d_ids, long long ld_out) {
    const LevelArgs a1{t1, pq1, d_stream1, stream_bytes1, raw_first1, chunk_vectors1,
                       d_chunk_offsets1, d_chunk_prev1, nullptr};
    const LevelArgs a2{t2, pq2, d_stream2, stream_bytes2, raw_first2, chunk_vectors2,
                       d_chunk_offsets2, d_chunk_prev2, nullptr};
    return refine<false>(ctx, true, a1, a2, n, cq, d_offsets, d_queries, nq, ld_q, d_rows, ncand, top_k,
                  d_dist, d_ids, ld_out);
}

int pqh_refine_codes(pqh_ctx_t* ctx, const pqh_pq_t* pq1, const void* d_codes1,
                     const pqh_pq_t* pq2, const void* d_codes2, long long n,
                     const pqh_coarse_t* cq, const long long* d_offsets, const float* d_queries,
                     long long nq, long long ld_q, const long long* d_rows, int ncand, int top_k,
                     float* d_dist, long long* d_ids, long long ld_out) {
    const LevelArgs a1{nullptr, pq1, nullptr, 0, 0, 0, nullptr, nullptr, d_codes1};
    const LevelArgs a2{nullptr, pq2, nullptr, 0, 0, 0, nullptr, nullptr, d_codes2};
    return refine<false>(ctx, false, a1, a2, n, cq, d_offsets, d_queries, nq, ld_q, d_rows, ncand, top_k,
                  d_dist, d_ids, ld_out);
}

int pqh_refine_stream_ip(pqh_ctx_t* ctx, const pqh_tables_t* t1, const pqh_pq_t* pq1,
                         const unsigned char* d_stream1, unsigned long long stream_bytes1,
                         int raw_first1, int chunk_vectors1,
                         const unsigned long long* d_chunk_offsets1, const void* d_chunk_prev1,
                         const pqh_tables_t* t2, const pqh_pq_t* pq2,
                         const unsigned char* d_stream2, unsigned long long stream_bytes2,
                         int raw_first2, int chunk_vectors2,
                         const unsigned long long* d_chunk_offsets2, const void* d_chunk_prev2,
                         long long n, const pqh_coarse_t* cq, const long long* d_offsets,
                         const float* d_queries, long long nq, long long ld_q,
                         const long long* d_rows, int ncand, int top_k, float* d_dist,
                         long long* d_ids, long long ld_out) {
    const LevelArgs a1{t1, pq1, d_stream1, stream_bytes1, raw_first1, chunk_vectors1,
                       d_chunk_offsets1, d_chunk_prev1, nullptr};
    const LevelArgs a2{t2, pq2, d_stream2, stream_bytes2, raw_first2, chunk_vectors2,
                       d_chunk_offsets2, d_chunk_prev2, nullptr};
    return refine<true>(ctx, true, a1, a2, n, cq, d_offsets, d_queries, nq, ld_q, d_rows, ncand,
                        top_k, d_dist, d_ids, ld_out);
}

int pqh_refine_codes_ip(pqh_ctx_t* ctx, const pqh_pq_t* pq1, const void* d_codes1,
                        const pqh_pq_t* pq2, const void* d_codes2, long long n,
                        const pqh_coarse_t* cq, const long long* d_offsets, const float* d_queries,
                        long long nq, long long ld_q, const long long* d_rows, int ncand,
                        int top_k, float* d_dist, long long* d_ids, long long ld_out) {
    const LevelArgs a1{nullptr, pq1, nullptr, 0, 0, 0, nullptr, nullptr, d_codes1};
    const LevelArgs a2{nullptr, pq2, nullptr, 0, 0, 0, nullptr, nullptr, d_codes2};
    return refine<true>(ctx, false, a1, a2, n, cq, d_offsets, d_queries, nq, ld_q, d_rows, ncand,
                        top_k, d_dist, d_ids, ld_out);
}

}  // extern "C"
