// pqh_sq.hip -- IVF-SQ8: rows as 8-bit codes, one scalar quantizer a dimension (DESIGN.md
// 4.5.19).  The definition is pqh.h's: vmin and step per dimension, code = rint((x - vmin) / step)
// clamped to [0, 255], dec = vmin + code * step, every operation one fp32 rounding; the search's
// distances are the chain of pqh_flat_search (chain_step) over the decoded rows.
//
//  sq_keys_init / sq_minmax / sq_params  training: the column minima and maxima of the finite
//                 values.  A workgroup takes a slab of rows and 64 columns, a wave every fourth
//                 row of the slab with consecutive lanes on consecutive floats of it; the four
//                 waves' results meet in LDS and go by integer atomicMin / atomicMax on
//                 order-preserving keys to 2 d words of the workspace; sq_params turns the keys
//                 into vmin and step.  Min and max do not depend on the grid.
//  sq_encode<PERM>  out row s = the codes of row perm[s] (or s): a thread makes four codes,
//                 consecutive threads consecutive quads of a row, one dword store where it may.
//  sq_decode      the rows a list names (or a range), a thread four floats.
//  sq_lists<IP, KR>  the scan: flat_lists' outer shape (the list-major plan, a unit = a list
//                 and up to QB of its pairs, four waves, tiles of 256 rows with lane = row, G
//                 groups of tiles, partial lists [pair][G][k] merged by adc_merge, the row mask
//                 and the tile skip), with another way of moving and consuming a tile.  A tile
//                 lies in LDS as bytes in chunks of kJC = 64 dimensions, [256 rows][17 dwords]:
//                 the lanes of a wave read one dword column of 64 consecutive rows, and the odd
//                 pitch keeps them in distinct banks.  A chunk comes from global memory 16 bytes
//                 a lane, four lanes a row's 64 bytes, four such loads a thread: the prefetch
//                 is 16 registers where the fp32 scan holds 32; the loads of chunk c + 1 are
//                 issued before the arithmetic of chunk c, one barrier a chunk.  Beside a chunk
//                 lie the unit's query values [j][QB] and the parameters [j][2], all read at one
//                 address by every lane (LDS broadcasts).  A lane reads a dword of its row,
//                 converts its four bytes, decodes each once, and runs the chain steps of the
//                 unit's pairs four at a time; the number of groups of four is a template value
//                 of the chunk's loop, so a group beyond the unit's pairs costs nothing.
//                 Dimensions from d to the chunk's end have zeros as parameters and query
//                 values: dec = 0 + code * 0 = 0 and the chain step adds 0 * 0, which changes
//                 no accumulator bit.
//                 2 (4,352 + 64 QB + 128) dwords and the lists, 4 QB k 8 bytes: 76,800 B at
//                 k = 64, two workgroups a CU.
#include <algorithm>
#include <atomic>
#include <type_traits>

#include "pqh_flat_dev.h"
#include "pqh_internal.h"
#include "pqh_topk_dev.h"

namespace {

// ------------------------------------------------------------------- the definition
__device__ __forceinline__ unsigned sq_code(float x, float vmin, float step) {
    const float t = (x - vmin) / step;   // (the correctly rounded division: hipcc's default)
    if (t != t) return 0u;
    return (unsigned)fminf(fmaxf(rintf(t), 0.f), 255.f);
}
__device__ __forceinline__ float sq_dec(float code, float vmin, float step) {
    return vmin + code * step;
}
// the bytes of a dword as floats: v_cvt_f32_ubyte0..3
__device__ __forceinline__ float sq_byte(unsigned w, int b) { return (float)((w >> (8 * b)) & 0xFFu); }

// ------------------------------------------------------------------- training
// key(a) < key(b) as unsigned iff a < b as floats, with -0 below +0
__device__ __forceinline__ unsigned sq_key(unsigned u) { return u & 0x80000000u ? ~u : u | 0x80000000u; }
__device__ __forceinline__ float sq_unkey(unsigned k) {
    return __uint_as_float(k & 0x80000000u ? k & 0x7FFFFFFFu : ~k);
}

__global__ void sq_keys_init(unsigned* keys, int d) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < d) keys[j] = 0xFFFFFFFFu, keys[d + j] = 0u;
}

constexpr int kMmUnroll = 4;   // rows a wave has in flight

__global__ void __launch_bounds__(256)
sq_minmax(const float* __restrict__ x, long long n, long long ld_x, int d, long long slab,
          unsigned* __restrict__ keys) {
    __shared__ unsigned part[2][4][64];
    const int lane = threadIdx.x, wave = threadIdx.y;
    const int j = blockIdx.x * 64 + lane;
    const long long r0 = blockIdx.y * slab, r1 = min(n, r0 + slab);
    unsigned lo = 0xFFFFFFFFu, hi = 0u;
    if (j < d) {
#pragma unroll 1
        for (long long r = r0 + wave; r < r1; r += 4 * kMmUnroll) {
            unsigned v[kMmUnroll];
#pragma unroll
            for (int u = 0; u < kMmUnroll; ++u)
                v[u] = r + 4 * u < r1 ? __float_as_uint(x[(r + 4 * u) * ld_x + j]) : 0x7F800000u;
#pragma unroll
            for (int u = 0; u < kMmUnroll; ++u) {
                if ((v[u] & 0x7F800000u) == 0x7F800000u) continue;   // not finite
                lo = min(lo, sq_key(v[u]));
                hi = max(hi, sq_key(v[u]));
            }
        }
    }
    part[0][wave][lane] = lo, part[1][wave][lane] = hi;
    lds_barrier();
    if (wave == 0 && j < d) {
#pragma unroll
        for (int w = 1; w < 4; ++w) lo = min(lo, part[0][w][lane]), hi = max(hi, part[1][w][lane]);
        if (lo <= hi) atomicMin(keys + j, lo), atomicMax(keys + d + j, hi);
    }
}

__global__ void sq_params(const unsigned* __restrict__ keys, int d, float* __restrict__ vmin,
                          float* __restrict__ step) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= d) return;
    const unsigned klo = keys[j], khi = keys[d + j];
    float lo = 0.f, st = 0.f;
    if (klo <= khi) {   // (else no finite value)
        lo = sq_unkey(klo);
        st = (sq_unkey(khi) - lo) / 255.0f;
    }
    vmin[j] = lo, step[j] = st;
}

// ------------------------------------------------------------------- encoder and decoder
struct CodecArgs {
    const float* x;            // encode: the rows; decode: unused
    unsigned char* codes;      // encode: out; decode: in
    float* out;                // decode: the rows
    long long n, ld_x, ld_c, ld_out;
    int d;
    const long long* sel;      // encode: perm or NULL; decode: rows or NULL
    long long first, count;    // decode: the range when sel is NULL, and the rows of out
    const float* vmin;
    const float* step;
    int vec_f;                 // float4 on x / out, vmin and step
    int vec_c;                 // whole quads of codes as dwords
    unsigned long long* err;
};

template <bool PERM>
__global__ void __launch_bounds__(256)
sq_encode(const CodecArgs a) {
    const int d = a.d, nqd = (d + 3) >> 2;
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= a.n * nqd) return;
    const long long s = g / nqd;
    const int j = 4 * (int)(g - s * nqd);
    long long p = s;
    if constexpr (PERM) p = a.sel[s];
    const bool good = p >= 0 && p < a.n;
    float xv[4] = {0.f, 0.f, 0.f, 0.f}, mn[4] = {0.f, 0.f, 0.f, 0.f}, st[4] = {0.f, 0.f, 0.f, 0.f};
    if (good) {
        const float* xr = a.x + p * a.ld_x + j;
        if (a.vec_f) {
            const float4 v = *reinterpret_cast<const float4*>(xr);
            const float4 m = *reinterpret_cast<const float4*>(a.vmin + j);
            const float4 t = *reinterpret_cast<const float4*>(a.step + j);
            xv[0] = v.x, xv[1] = v.y, xv[2] = v.z, xv[3] = v.w;
            mn[0] = m.x, mn[1] = m.y, mn[2] = m.z, mn[3] = m.w;
            st[0] = t.x, st[1] = t.y, st[2] = t.z, st[3] = t.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (j + i < d) xv[i] = xr[i], mn[i] = a.vmin[j + i], st[i] = a.step[j + i];
        }
    }
    unsigned c[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) c[i] = good ? sq_code(xv[i], mn[i], st[i]) : 0u;
    unsigned char* dst = a.codes + s * a.ld_c + j;
    if (a.vec_c && j + 4 <= d) {
        *reinterpret_cast<unsigned*>(dst) = c[0] | c[1] << 8 | c[2] << 16 | c[3] << 24;
    } else {   // (the bytes from d to ld_c are left alone)
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (j + i < d) dst[i] = (unsigned char)c[i];
    }
    if constexpr (PERM)
        if (__ballot(!good) && (threadIdx.x & 63) == __ffsll((long long)__ballot(true)) - 1)
            atomicOr(a.err, 1ull);
}

__global__ void __launch_bounds__(256)
sq_decode(const CodecArgs a) {
    const int d = a.d, nqd = (d + 3) >> 2;
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= a.count * nqd) return;
    const long long i = g / nqd;
    const int j = 4 * (int)(g - i * nqd);
    const long long r = a.sel ? a.sel[i] : a.first + i;
    const bool good = r >= 0 && r < a.n;
    float v[4] = {0.f, 0.f, 0.f, 0.f};   // (-1, and a row out of range: zeros)
    if (good) {
        const unsigned char* src = a.codes + r * a.ld_c + j;
        unsigned w = 0u;
        if (a.vec_c && j + 4 <= d) {
            w = *reinterpret_cast<const unsigned*>(src);
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (j + b < d) w |= (unsigned)src[b] << (8 * b);
        }
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (j + b < d) v[b] = sq_dec(sq_byte(w, b), a.vmin[j + b], a.step[j + b]);
    }
    float* dst = a.out + i * a.ld_out + j;
    if (a.vec_f) {
        *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (j + b < d) dst[b] = v[b];
    }
    if (__ballot(!good && r != -1ll) && (threadIdx.x & 63) == __ffsll((long long)__ballot(true)) - 1)
        atomicOr(a.err, 1ull);
}

// ------------------------------------------------------------------- the scan
constexpr int kTile = 256;          // rows a workgroup scores at once, lane = row
// Dimensions (bytes of a row) a staged chunk.  64 was measured against 128 (-DPQH_SQ_JC=128: pitch
// 33, one workgroup a CU, half the barriers) and kept: DESIGN.md 4.5.19.
#ifndef PQH_SQ_JC
#define PQH_SQ_JC 64
#endif
constexpr int kJC = PQH_SQ_JC;
static_assert(kJC == 64 || kJC == 128, "a chunk is 16 bytes a lane, 4 or 8 lanes a row");
// Rows kPitch dwords apart in LDS.  The lanes of a wave read one dword column of 64 consecutive
// rows: word addresses lane * kPitch + w, in distinct banks iff kPitch is odd.  kJC / 4 = 16
// would put them four ways in a bank; 17 is the smallest odd pitch.
constexpr int kPitch = kJC / 4 + 1;
constexpr int kWaves = 4;
constexpr int kChunkWords = kTile * kPitch;   // 4,352 dwords = 17,408 B
constexpr int kLR = kJC / 16;                 // lanes a row's chunk, 16 bytes each
constexpr int kPre = kTile * kLR / (64 * kWaves);   // such pieces a thread moves: 4

struct __attribute__((aligned(4))) Quad {   // 16 bytes of a row that lie on 4 bytes
    unsigned w[4];
};

struct SqListsArgs {
    const unsigned char* codes;
    long long ld_c;
    int d, nprobe;
    const float* vmin;
    const float* step;
    const long long* offsets;
    const long long* units;
    const long long* nunits;
    const int* pairs;
    const float* q;
    long long ld_q;
    int k, words;        // words: rows and base on 4 bytes, a chunk is read by dwords
    const unsigned* keep;
    float* part_d;       // [pairs][G][k]
    long long* part_id;
};

__host__ __device__ constexpr int sq_qb(int KR) { return KR == 1 ? 16 : 4; }
size_t sq_lds_bytes(int qb, int k) {
    return (size_t)2 * (kChunkWords + kJC * qb + 2 * kJC) * 4 + (size_t)kWaves * qb * k * 8;
}

template <bool IP, int KR>
__global__ void __launch_bounds__(64 * kWaves)
sq_lists(const SqListsArgs a) {
    constexpr int QB = sq_qb(KR);
    constexpr int QE = kJC * QB / (64 * kWaves);   // query values a thread stages: 4 or 1
    static_assert(QB * 64 <= 64 * kPitch, "a tile's distances fit the wave's rows of a chunk");
    extern __shared__ __attribute__((aligned(16))) unsigned smem[];
    const int lane = threadIdx.x, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.y);
    const int tid = wave * 64 + lane;
    // the grid is the host's bound of the units: a workgroup beyond those there are leaves as a
    // whole, before any barrier
    if ((long long)blockIdx.x >= a.nunits[0]) return;
    const long long u_list = a.units[3 * (long long)blockIdx.x];
    const long long u_first = a.units[3 * (long long)blockIdx.x + 1];
    const int u_cnt = (int)a.units[3 * (long long)blockIdx.x + 2];
    // (a good pair of offsets with rows, or the plan had made no unit of the list)
    const long long l_first = a.offsets[u_list];
    const int l_count = (int)(a.offsets[u_list + 1] - l_first);
    const int k = a.k, kth = k - 1, d = a.d;

    unsigned* const xbuf = smem;                                              // [2][kTile][kPitch]
    float* const qbuf = reinterpret_cast<float*>(smem + 2 * kChunkWords);     // [2][kJC][QB]
    float* const pbuf = qbuf + 2 * kJC * QB;                                  // [2][kJC][vmin, step]
    float* const ls_d = pbuf + 2 * kJC * 2;                                   // [kWaves][QB][k]
    int* const ls_i = reinterpret_cast<int*>(ls_d + kWaves * QB * k);
    for (int i = lane; i < QB * k; i += 64) ls_d[wave * QB * k + i] = INFINITY, ls_i[wave * QB * k + i] = -1;

    // the query values this thread stages per chunk: entry idx = e * 256 + tid of [QB][kJC]; and
    // its parameter: the first kJC threads a vmin, the next kJC a step
    const float* qrow[QE];
    int qat[QE], qj[QE];
#pragma unroll
    for (int e = 0; e < QE; ++e) {
        const int idx = e * 64 * kWaves + tid, qq = idx / kJC;
        qj[e] = idx % kJC;
        qat[e] = qj[e] * QB + qq;
        qrow[e] = qq < u_cnt ? a.q + (long long)(a.pairs[u_first + qq] / a.nprobe) * a.ld_q : nullptr;
    }
    const int pj = tid % kJC, pw = tid / kJC;
    const float* const prow = pw == 0 ? a.vmin : pw == 1 ? a.step : nullptr;

    // this group's tiles
    const int nt = (l_count + kTile - 1) / kTile;
    const int t_lo = (int)((long long)blockIdx.y * nt / gridDim.y);
    const int t_hi = (int)(((long long)blockIdx.y + 1) * nt / gridDim.y);
    // whether this thread's row of tile t takes part (the keep word of a row below n exists)
    auto row_live = [&](int t) -> bool {
        const int r = kTile * t + tid;
        if (r >= l_count) return false;
        if (!a.keep) return true;
        const long long v = l_first + r;
        return ((a.keep[v >> 5] >> (v & 31)) & 1u) != 0u;
    };
    // the first tile from t on with a kept row (workgroup-uniform; a barrier per tile looked at)
    auto next_live = [&](int t) -> int {
        if (a.keep)
            while (t < t_hi && !__syncthreads_or(row_live(t))) ++t;
        return t;
    };

    // The prefetch: kPre times 16 bytes of a row (kLR lanes a row's chunk, 256 / kLR rows a step), the
    // query values, a parameter.  A row past the list's end reads the list's last row; a byte
    // from d on is not read.
    unsigned pre[kPre][4];
    float preq[QE], prep;
    auto fetch = [&](int t, int c) {
        const long long r0 = l_first + (long long)kTile * t, last = l_first + l_count - 1;
        const int j0 = c * kJC + 16 * (tid % kLR);
#pragma unroll
        for (int i = 0; i < kPre; ++i) {
            const unsigned char* src = a.codes + min(r0 + kTile / kPre * i + tid / kLR, last) * a.ld_c + j0;
            if (a.words) {   // (a dword that begins below d ends inside the row: ld_c % 4 == 0)
                if (j0 + 16 <= d) {
                    const Quad v = *reinterpret_cast<const Quad*>(src);
                    pre[i][0] = v.w[0], pre[i][1] = v.w[1], pre[i][2] = v.w[2], pre[i][3] = v.w[3];
                } else {
#pragma unroll
                    for (int w = 0; w < 4; ++w)
                        pre[i][w] = j0 + 4 * w < d ? *reinterpret_cast<const unsigned*>(src + 4 * w) : 0u;
                }
            } else {
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    pre[i][w] = 0u;
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        if (j0 + 4 * w + b < d) pre[i][w] |= (unsigned)src[4 * w + b] << (8 * b);
                }
            }
        }
#pragma unroll
        for (int e = 0; e < QE; ++e) {
            const int j = c * kJC + qj[e];
            preq[e] = qrow[e] && j < d ? qrow[e][j] : 0.f;
        }
        prep = prow && c * kJC + pj < d ? prow[c * kJC + pj] : 0.f;
    };
    auto stash = [&](int b) {
#pragma unroll
        for (int i = 0; i < kPre; ++i) {
            unsigned* dst = xbuf + b * kChunkWords + (kTile / kPre * i + tid / kLR) * kPitch + 4 * (tid % kLR);
            dst[0] = pre[i][0], dst[1] = pre[i][1], dst[2] = pre[i][2], dst[3] = pre[i][3];
        }
#pragma unroll
        for (int e = 0; e < QE; ++e) qbuf[b * kJC * QB + qat[e]] = preq[e];
        if (pw < 2) pbuf[b * kJC * 2 + 2 * pj + pw] = prep;
    };

    const int nc = (d + kJC - 1) / kJC;
    const int ng = (min(u_cnt, QB) + 3) >> 2;   // the unit's groups of four pairs (wave-uniform)
    float acc[QB];
    // a chunk's arithmetic for NG groups of four pairs: per dword of the row four decodes, then
    // the chain steps of every pair, j ascending
    auto chunk = [&](auto ngc, const unsigned* xs, const float* qs, const float* ps, int nw) {
        constexpr int NG = decltype(ngc)::value;
#pragma unroll 2
        for (int w = 0; w < nw; ++w) {
            const unsigned cw = xs[w];
            const float4 p01 = *reinterpret_cast<const float4*>(ps + 8 * w);
            const float4 p23 = *reinterpret_cast<const float4*>(ps + 8 * w + 4);
            const float dec[4] = {sq_dec(sq_byte(cw, 0), p01.x, p01.y), sq_dec(sq_byte(cw, 1), p01.z, p01.w),
                                  sq_dec(sq_byte(cw, 2), p23.x, p23.y), sq_dec(sq_byte(cw, 3), p23.z, p23.w)};
#pragma unroll
            for (int g4 = 0; g4 < NG; ++g4) {
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const float4 qv = *reinterpret_cast<const float4*>(qs + (4 * w + b) * QB + 4 * g4);
                    chain_step<IP>(acc[4 * g4], qv.x, dec[b]);
                    chain_step<IP>(acc[4 * g4 + 1], qv.y, dec[b]);
                    chain_step<IP>(acc[4 * g4 + 2], qv.z, dec[b]);
                    chain_step<IP>(acc[4 * g4 + 3], qv.w, dec[b]);
                }
            }
        }
    };

    int t = next_live(t_lo), u = 0;
    if (t < t_hi) {
        fetch(t, 0);
        stash(0);
    }
    lds_barrier();
#pragma unroll 1
    while (t < t_hi) {
        int t1 = t;
#pragma unroll 1
        for (int c = 0; c < nc; ++c) {
            const bool end = c == nc - 1;
            if (end) t1 = next_live(t + 1);
            const bool more = !end || t1 < t_hi;
            if (more) fetch(end ? t1 : t, end ? 0 : c + 1);
            unsigned* const xc = xbuf + (u & 1) * kChunkWords;
            const unsigned* const xs = xc + tid * kPitch;
            const float* const qs = qbuf + (u & 1) * kJC * QB;
            const float* const ps = pbuf + (u & 1) * kJC * 2;
            const int nw = (min(kJC, d - c * kJC) + 3) >> 2;
            if (c == 0) {
#pragma unroll
                for (int qq = 0; qq < QB; ++qq) acc[qq] = 0.f;
            }
            if constexpr (QB == 4) {
                chunk(std::integral_constant<int, 1>{}, xs, qs, ps, nw);
            } else {
                switch (ng) {
                    case 1: chunk(std::integral_constant<int, 1>{}, xs, qs, ps, nw); break;
                    case 2: chunk(std::integral_constant<int, 2>{}, xs, qs, ps, nw); break;
                    case 3: chunk(std::integral_constant<int, 3>{}, xs, qs, ps, nw); break;
                    default: chunk(std::integral_constant<int, 4>{}, xs, qs, ps, nw); break;
                }
            }
            if (end) {
                // The tile's distances.  The wave's 64 rows of this buffer are read by no other
                // wave and written again only after the next barrier: they take the distances,
                // [pair][lane] (QB * 64 of the 64 * kPitch dwords), so that the pairs can be
                // walked by a loop
                const bool valid = row_live(t);
                const int rel = kTile * t + tid;   // the row inside the list
                float* const ds = reinterpret_cast<float*>(xc + wave * 64 * kPitch);
#pragma unroll
                for (int qq = 0; qq < QB; ++qq) ds[qq * 64 + lane] = acc[qq];
#pragma unroll 1
                for (int qq = 0; qq < u_cnt; ++qq) {
                    float* const ld = ls_d + (wave * QB + qq) * k;
                    int* const li = ls_i + (wave * QB + qq) * k;
                    const float dist = ds[qq * 64 + lane];
                    if (!__ballot(valid && lex_lt(dist, (long long)rel, ld[kth], (long long)li[kth])))
                        continue;   // (wave-uniform: nobody beats the k-th entry)
                    ListT<KR> e;
                    list_from_lds<KR>(e, ld, li, k);
                    list_offer<false>(e, dist, (long long)rel, valid, kth);
                    list_to_lds<KR>(e, ld, li, k);
                }
            }
            // the other buffer was last read before the barrier that ended the chunk before
            if (more) stash((u + 1) & 1);
            lds_barrier();
            ++u;
        }
        t = t1;
    }

    // ---- the four waves' lists of a pair into one, to the pair's slot of this group
#pragma unroll 1
    for (int qq = wave; qq < u_cnt; qq += kWaves) {
        ListT<KR> e;
        list_from_lds<KR>(e, ls_d + qq * k, ls_i + qq * k, k);
#pragma unroll 1
        for (int s = 1; s < kWaves; ++s) {
            const float* ld = ls_d + (s * QB + qq) * k;
            const int* li = ls_i + (s * QB + qq) * k;
#pragma unroll 1
            for (int b = 0; b <= (kth >> 6); ++b) {   // (a list ascends: 64 entries are sorted)
                const bool in = b * 64 + lane < k;
                const int id = in ? li[b * 64 + lane] : -1;
                list_offer<true>(e, in ? ld[b * 64 + lane] : INFINITY, (long long)id, id >= 0, kth);
            }
        }
        const long long at = ((long long)a.pairs[u_first + qq] * gridDim.y + blockIdx.y) * k;
        if constexpr (KR == 1) {
            if (lane < k) {
                a.part_d[at + lane] = e.d;
                a.part_id[at + lane] = e.id < 0 ? -1ll : l_first + e.id;
            }
        } else {
#pragma unroll
            for (int b = 0; b < kWideKR; ++b) {
                if (b * 64 + lane < k) {
                    a.part_d[at + b * 64 + lane] = e.d[b];
                    a.part_id[at + b * 64 + lane] = e.id[b] < 0 ? -1ll : l_first + e.id[b];
                }
            }
        }
    }
}

// ------------------------------------------------------------------- the host side
template <bool IP, int KR>
int sq_lists_launch(pqh_ctx* ctx, const SqListsArgs& a, long long units, int groups) {
    const size_t lds = sq_lds_bytes(sq_qb(KR), a.k);
    const auto fn = sq_lists<IP, KR>;
    // more than 64 KB of dynamic LDS is granted once per instantiation and device (the bitmap
    // holds devices 0 to 63; a device beyond them is granted again on every call)
    static std::atomic<unsigned long long> granted{0};
    const unsigned long long bit = ctx->device < 64 ? 1ull << ctx->device : 0ull;
    if (!(granted.load() & bit)) {
        const size_t most = sq_lds_bytes(sq_qb(KR), KR == 1 ? PQH_SEARCH_MAX_K : PQH_SEARCH_MAX_K_WIDE);
        PQH_HIP(ctx, hipFuncSetAttribute((const void*)fn,
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)most));
        granted.fetch_or(bit);
    }
    hipLaunchKernelGGL(fn, dim3((unsigned)units, (unsigned)groups), dim3(64, kWaves), lds,
                       ctx->stream, a);
    PQH_LAUNCH_CHECK(ctx);
    return PQH_OK;
}

int sq_search(bool ip, pqh_ctx_t* ctx, const unsigned char* d_codes, long long n, long long ld_c,
              int d, const float* d_vmin, const float* d_step, const long long* d_offsets,
              long long nlist, const long long* d_probes, const float* d_queries, long long nq,
              long long ld_q, int nprobe, int top_k, const unsigned int* d_keep_bits,
              long long id_base, float* d_dist, long long* d_ids) {
    // what is wrong whatever the context
    if (n < 0 || d < 1 || ld_c < d || nlist < 1 || nq < 0 || ld_q < d || nprobe < 1 ||
        nprobe > PQH_IVF_MAX_NPROBE || top_k < 1 || top_k > PQH_SEARCH_MAX_K_WIDE || id_base < 0 ||
        id_base > 0x7FFFFFFFFFFFFFFFll - n)
        return PQH_ERR_ARG;
    if (nq > 0 && (!d_offsets || !d_probes || !d_queries || !d_dist || !d_ids ||
                   (n > 0 && (!d_codes || !d_vmin || !d_step))))
        return PQH_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(d_keep_bits) & 3u) return PQH_ERR_ARG;
    if (!ctx) return pqh_no_ctx_status();
    if (top_k > ctx->search_max_k) return PQH_ERR_ARG;
    if (n > 0x7FFFFFFFll || nlist > 0x7FFFFFFFll || nq > 0x7FFFFFFFll / nprobe)
        return PQH_ERR_UNSUPPORTED;
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    if (nq == 0) return PQH_OK;
    if (n == 0) return pqh_lists_merge_launch(ctx, nullptr, nullptr, 0, nq, top_k, id_base, d_dist, d_ids);

    const bool wide = top_k > PQH_SEARCH_MAX_K;
    const int qb = sq_qb(wide ? kWideKR : 1);
    const long long npairs = nq * nprobe;
    const long long bound = std::min<long long>(npairs, nlist + npairs / qb);
    const long long groups = lists_groups(ctx, n, nlist, bound, kTile);

    const size_t entries = (size_t)npairs * groups * top_k;
    rc = pqh_ensure_ws(ctx, entries * 12 + 16 + pqh_list_plan_bytes(nlist, npairs, bound));
    if (rc) return rc;
    long long* part_id = static_cast<long long*>(ctx->ws);
    float* part_d = reinterpret_cast<float*>(part_id + entries);
    pqh_list_plan lp{};
    lp.offsets = d_offsets, lp.nlist = nlist, lp.probes = d_probes, lp.npairs = npairs, lp.n = n;
    lp.qb = qb, lp.pad = groups * top_k, lp.units_bound = bound;
    lp.mem = static_cast<long long*>(ctx->ws) + ((entries * 12 + 15) / 8);
    lp.part_d = part_d, lp.part_id = part_id, lp.err = ctx->d_diag + kDiagIvf;
    rc = pqh_list_plan_launch(ctx, &lp);
    if (rc) return rc;

    SqListsArgs a{};
    a.codes = d_codes, a.ld_c = ld_c, a.d = d, a.nprobe = nprobe, a.vmin = d_vmin, a.step = d_step;
    a.offsets = d_offsets, a.units = lp.units, a.nunits = lp.nunits, a.pairs = lp.pairs;
    a.q = d_queries, a.ld_q = ld_q, a.k = top_k, a.keep = d_keep_bits;
    a.words = ld_c % 4 == 0 && (reinterpret_cast<uintptr_t>(d_codes) & 3u) == 0;
    a.part_d = part_d, a.part_id = part_id;
    rc = ip ? (wide ? sq_lists_launch<true, kWideKR>(ctx, a, bound, (int)groups)
                    : sq_lists_launch<true, 1>(ctx, a, bound, (int)groups))
            : (wide ? sq_lists_launch<false, kWideKR>(ctx, a, bound, (int)groups)
                    : sq_lists_launch<false, 1>(ctx, a, bound, (int)groups));
    if (rc) return rc;
    return pqh_lists_merge_launch(ctx, part_d, part_id, nprobe * groups, nq, top_k, id_base, d_dist, d_ids);
}

bool on16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

extern "C" {

int pqh_sq_train(pqh_ctx_t* ctx, const float* d_x, long long n, long long ld_x, int d,
                 float* d_vmin, float* d_step) {
    if (n < 0 || d < 1 || ld_x < d || !d_vmin || !d_step || (n > 0 && !d_x)) return PQH_ERR_ARG;
    if (!ctx) return pqh_no_ctx_status();
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    rc = pqh_ensure_ws(ctx, (size_t)2 * d * 4);
    if (rc) return rc;
    unsigned* keys = static_cast<unsigned*>(ctx->ws);
    const unsigned db = (unsigned)((d + 255) / 256);
    hipLaunchKernelGGL(sq_keys_init, dim3(db), dim3(256), 0, ctx->stream, keys, d);
    PQH_LAUNCH_CHECK(ctx);
    if (n > 0) {
        // slabs: eight workgroups a compute unit and column block at the most, 256 rows at least
        const long long slabs = std::max<long long>(1, std::min<long long>((n + 255) / 256, 8ll * ctx->num_cus));
        const long long slab = (n + slabs - 1) / slabs;
        hipLaunchKernelGGL(sq_minmax, dim3((unsigned)((d + 63) / 64), (unsigned)((n + slab - 1) / slab)),
                           dim3(64, 4), 0, ctx->stream, d_x, n, ld_x, d, slab, keys);
        PQH_LAUNCH_CHECK(ctx);
    }
    hipLaunchKernelGGL(sq_params, dim3(db), dim3(256), 0, ctx->stream, keys, d, d_vmin, d_step);
    PQH_LAUNCH_CHECK(ctx);
    return PQH_OK;
}

int pqh_sq_encode(pqh_ctx_t* ctx, const float* d_x, long long n, long long ld_x, int d,
                  const long long* d_perm, const float* d_vmin, const float* d_step,
                  unsigned char* d_codes, long long ld_c) {
    if (n < 0 || d < 1 || ld_x < d || ld_c < d || (n > 0 && (!d_x || !d_vmin || !d_step || !d_codes)))
        return PQH_ERR_ARG;
    if (!ctx) return pqh_no_ctx_status();
    const long long blocks = n > 0x7FFFFFFFFFFFFFFFll / ((d + 3) / 4) ? -1
                                                                     : (n * ((d + 3) / 4) + 255) / 256;
    if (blocks < 0 || blocks > 0x7FFFFFFFll) return PQH_ERR_UNSUPPORTED;
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    if (n == 0) return PQH_OK;
    CodecArgs a{};
    a.x = d_x, a.codes = d_codes, a.n = n, a.ld_x = ld_x, a.ld_c = ld_c, a.d = d, a.sel = d_perm;
    a.vmin = d_vmin, a.step = d_step, a.err = ctx->d_diag + kDiagIvf;
    a.vec_f = d % 4 == 0 && ld_x % 4 == 0 && on16(d_x) && on16(d_vmin) && on16(d_step);
    a.vec_c = ld_c % 4 == 0 && (reinterpret_cast<uintptr_t>(d_codes) & 3u) == 0;
    hipLaunchKernelGGL(d_perm ? sq_encode<true> : sq_encode<false>, dim3((unsigned)blocks), dim3(256),
                       0, ctx->stream, a);
    PQH_LAUNCH_CHECK(ctx);
    return PQH_OK;
}

int pqh_sq_decode(pqh_ctx_t* ctx, const unsigned char* d_codes, long long n, long long ld_c, int d,
                  const float* d_vmin, const float* d_step, const long long* d_rows, long long first,
                  long long count, float* d_out, long long ld_out) {
    if (n < 0 || d < 1 || ld_c < d || ld_out < d || count < 0 ||
        (!d_rows && (first < 0 || first > n || count > n - first)) ||
        (count > 0 && (!d_out || !d_vmin || !d_step || (n > 0 && !d_codes))))
        return PQH_ERR_ARG;
    if (!ctx) return pqh_no_ctx_status();
    const long long blocks = count > 0x7FFFFFFFFFFFFFFFll / ((d + 3) / 4)
                                 ? -1 : (count * ((d + 3) / 4) + 255) / 256;
    if (blocks < 0 || blocks > 0x7FFFFFFFll) return PQH_ERR_UNSUPPORTED;
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    if (count == 0) return PQH_OK;
    CodecArgs a{};
    a.codes = const_cast<unsigned char*>(d_codes), a.out = d_out, a.n = n, a.ld_c = ld_c;
    a.ld_out = ld_out, a.d = d, a.sel = d_rows, a.first = first, a.count = count;
    a.vmin = d_vmin, a.step = d_step, a.err = ctx->d_diag + kDiagIvf;
    a.vec_f = d % 4 == 0 && ld_out % 4 == 0 && on16(d_out);
    a.vec_c = ld_c % 4 == 0 && (reinterpret_cast<uintptr_t>(d_codes) & 3u) == 0;
    hipLaunchKernelGGL(sq_decode, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, a);
    PQH_LAUNCH_CHECK(ctx);
    return PQH_OK;
}

int pqh_sq_search_lists(pqh_ctx_t* ctx, const unsigned char* d_codes, long long n, long long ld_c,
                        int d, const float* d_vmin, const float* d_step, const long long* d_offsets,
                        long long nlist, const long long* d_probes, const float* d_queries,
                        long long nq, long long ld_q, int nprobe, int top_k,
                        const unsigned int* d_keep_bits, long long id_base, float* d_dist,
                        long long* d_ids) {
    return sq_search(false, ctx, d_codes, n, ld_c, d, d_vmin, d_step, d_offsets, nlist, d_probes,
                     d_queries, nq, ld_q, nprobe, top_k, d_keep_bits, id_base, d_dist, d_ids);
}

int pqh_sq_search_lists_ip(pqh_ctx_t* ctx, const unsigned char* d_codes, long long n,
                           long long ld_c, int d, const float* d_vmin, const float* d_step,
                           const long long* d_offsets, long long nlist, const long long* d_probes,
                           const float* d_queries, long long nq, long long ld_q, int nprobe,
                           int top_k, const unsigned int* d_keep_bits, long long id_base,
                           float* d_dist, long long* d_ids) {
    return sq_search(true, ctx, d_codes, n, ld_c, d, d_vmin, d_step, d_offsets, nlist, d_probes,
                     d_queries, nq, ld_q, nprobe, top_k, d_keep_bits, id_base, d_dist, d_ids);
}

}  // extern "C"
