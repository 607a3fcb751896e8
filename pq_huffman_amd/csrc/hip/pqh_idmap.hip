// pqh_idmap.hip -- the compressed id map of an inverted file: Elias-Fano coding of
//   key(s) = (list(s) << B) | perm[s],   B = bit width of n_ids - 1,
// which is strictly ascending over the stream because a list's ids are (include/pqh.h, DESIGN.md
// section 4.5.12).  One device blob of 64-bit words:
//   header     kHdrWords words, the H_* fields below
//   low bits   n fields of L bits, field s at bit s * L, little endian within and across words
//   high bits  one set bit per row, row s at bit (key(s) >> L) + s
//   samples    one word per 256 rows: the high-bit position of row 256 * j
//   reverse    the list of every id: u16 (0xFFFF = none) for nlist <= 65535, else i32 (-1 = none)
// Every bit no field owns is zero, so two maps of the same input are equal byte for byte.
//
//  idmap_build   one thread per row (high bit by atomicOr into cleared words, sample, reverse
//                scatter, the checks) and per low word (the thread owns the word: no atomics)
//  idmap_ids     stream rows -> ids, one lane per row: sample, popcount scan, select in a word
//  idmap_decode  a wave per block of 256 rows: the block's high words a word per lane, a wave
//                prefix sum of their popcounts, then lane i of pass t resolves row 64 * t + i
//                (a search of the prefix by shuffles, a select in the word) -- rows in lane
//                order, so the store is coalesced and idmap_pack can ballot in its place
//  idmap_pack    pqh_mask_pack through the map: keep[id(s)] by the same decode, perm never exists
//  idmap_rows    ids -> stream rows: the list from the reverse part, a binary search over the
//                list's rows comparing keys read by the select
// No kernel uses LDS; the waves of a workgroup share nothing.
#include <algorithm>

#include "pqh_internal.h"

namespace {

typedef unsigned long long u64;

constexpr int kHdrWords = 16;
constexpr u64 kMagic = 0x3150414D44495150ull;   // "PQIDMAP1"
enum {
    H_MAGIC = 0, H_N, H_NIDS, H_NLIST, H_B, H_L, H_LOW, H_HIGH, H_HIGH_WORDS, H_SAMP, H_SAMPS,
    H_REV, H_REV_SIZE, H_WORDS
};

struct idmap_shape {
    long long n, n_ids, nlist;
    int B, L, rev_size;   // rev_size: bytes of a reverse entry, 0 = no reverse part
    u64 low, low_words, high, high_words, samp, samps, rev, rev_words, words;
};

int bit_width(u64 v) {
    int b = 0;
    while (v) {
        ++b;
        v >>= 1;
    }
    return b;
}

int shape_of(long long n, long long n_ids, long long nlist, int reverse, idmap_shape* s) {
    if (n < 0 || n_ids < n || nlist < 1) return PQH_ERR_ARG;
    if (n_ids > 0x7FFFFFFFll || nlist > PQH_IVF_MAX_NLIST) return PQH_ERR_UNSUPPORTED;
    s->n = n;
    s->n_ids = n_ids;
    s->nlist = nlist;
    s->B = n_ids > 0 ? bit_width((u64)n_ids - 1) : 0;
    const u64 universe = (u64)nlist << s->B;
    s->L = n > 0 && universe / (u64)n >= 1 ? bit_width(universe / (u64)n) - 1 : 0;
    s->rev_size = !reverse ? 0 : nlist <= 65535 ? 2 : 4;
    s->low = kHdrWords;
    s->low_words = ((u64)n * s->L + 63) / 64;
    s->high = s->low + s->low_words;
    s->high_words = n > 0 ? ((((universe - 1) >> s->L) + (u64)n) + 63) / 64 : 0;
    s->samp = s->high + s->high_words;
    s->samps = ((u64)n + 255) / 256;
    s->rev = s->samp + s->samps;
    s->rev_words = ((u64)n_ids * s->rev_size + 7) / 8;
    s->words = s->rev + s->rev_words;
    return PQH_OK;
}

// ---- the device's view of a blob --------------------------------------------------------
struct idmap_view {
    long long n, n_ids, nlist;
    int B, L, rev_size;
    const u64* low;
    const u64* high;
    u64 high_words;
    const u64* samp;
    const void* rev;
};

__device__ __forceinline__ idmap_view view_of(const u64* __restrict__ map) {
    idmap_view v;
    v.n = (long long)map[H_N];
    v.n_ids = (long long)map[H_NIDS];
    v.nlist = (long long)map[H_NLIST];
    v.B = (int)map[H_B];
    v.L = (int)map[H_L];
    v.rev_size = (int)map[H_REV_SIZE];
    v.low = map + map[H_LOW];
    v.high = map + map[H_HIGH];
    v.high_words = map[H_HIGH_WORDS];
    v.samp = map + map[H_SAMP];
    v.rev = map + map[H_REV];
    return v;
}

__device__ __forceinline__ u64 low_mask(int bits) { return bits ? (~0ull >> (64 - bits)) : 0ull; }

// the L low bits of row r (r < n; a field may straddle two words, then both lie in the part)
__device__ __forceinline__ u64 low_field(const idmap_view& v, long long r) {
    if (v.L == 0) return 0;
    const u64 off = (u64)r * v.L;
    const int sh = (int)(off & 63);
    u64 f = v.low[off >> 6] >> sh;
    if (sh + v.L > 64) f |= v.low[(off >> 6) + 1] << (64 - sh);
    return f & low_mask(v.L);
}

// position of the k-th (0-based) set bit of x, k < popcount(x): a bisection by popcounts
__device__ __forceinline__ int sel64(u64 x, int k) {
    int pos = 0;
    uint32_t w = (uint32_t)x;
    int c = __popc(w);
    if (k >= c) {
        k -= c;
        pos = 32;
        w = (uint32_t)(x >> 32);
    }
    c = __popc(w & 0xFFFFu);
    if (k >= c) {
        k -= c;
        pos += 16;
        w >>= 16;
    }
    c = __popc(w & 0xFFu);
    if (k >= c) {
        k -= c;
        pos += 8;
        w >>= 8;
    }
    c = __popc(w & 0xFu);
    if (k >= c) {
        k -= c;
        pos += 4;
        w >>= 4;
    }
    c = __popc(w & 0x3u);
    if (k >= c) {
        k -= c;
        pos += 2;
        w >>= 2;
    }
    if (k >= (int)(w & 1u)) pos += 1;
    return pos;
}

// key of row r (0 <= r < n): the sample of the row's block, popcounts up to the wanted bit's
// word, the select in that word, the low field.  false: the bit is not there (a map whose build
// reported an error); nothing is read outside the parts either way.
__device__ __forceinline__ bool select_key(const idmap_view& v, long long r, u64* key) {
    const u64 pos0 = v.samp[r >> 8];
    u64 w = pos0 >> 6;
    if (w >= v.high_words) return false;
    u64 word = v.high[w] & (~0ull << (pos0 & 63));
    int rem = (int)(r & 255);
    for (;;) {
        const int c = __popcll(word);
        if (rem < c) break;
        rem -= c;
        if (++w >= v.high_words) return false;
        word = v.high[w];
    }
    const u64 pos = w * 64 + (u64)sel64(word, rem);
    *key = ((pos - (u64)r) << v.L) | low_field(v, r);
    return true;
}

// id of a key, -1 where the map holds an id it cannot hold (a build that reported an error)
__device__ __forceinline__ long long id_of_key(const idmap_view& v, u64 key) {
    const long long id = (long long)(key & low_mask(v.B));
    return id < v.n_ids ? id : -1;
}

// ---- build ------------------------------------------------------------------------------
// the last list l of [0, nlist) with offsets[l] <= s: the list of row s where offsets cover
// the stream (empty lists before it are passed over)
__device__ __forceinline__ long long list_of(const long long* __restrict__ offsets, long long nlist,
                                             long long s) {
    long long lo = 0, hi = nlist - 1;
    while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if (offsets[mid] <= s) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

struct row_key {
    u64 key;
    long long id, list;   // id: -1 = out of range
    bool bad;
};

__device__ __forceinline__ row_key key_of_row(const long long* __restrict__ perm,
                                              const long long* __restrict__ offsets,
                                              long long nlist, long long n_ids, int B, long long s) {
    row_key k;
    const long long p = perm[s];
    k.list = list_of(offsets, nlist, s);
    k.bad = p < 0 || p >= n_ids || offsets[k.list] > s || offsets[k.list + 1] <= s;
    k.id = p < 0 || p >= n_ids ? -1 : p;
    k.key = ((u64)k.list << B) | (u64)(k.id < 0 ? 0 : k.id);
    return k;
}

__global__ void __launch_bounds__(256)
idmap_build(const long long* __restrict__ perm, const long long* __restrict__ offsets,
            idmap_shape sh, u64* __restrict__ map, u64* __restrict__ err) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    if (t == 0) {
        map[H_MAGIC] = kMagic;
        map[H_N] = (u64)sh.n;
        map[H_NIDS] = (u64)sh.n_ids;
        map[H_NLIST] = (u64)sh.nlist;
        map[H_B] = (u64)sh.B;
        map[H_L] = (u64)sh.L;
        map[H_LOW] = sh.low;
        map[H_HIGH] = sh.high;
        map[H_HIGH_WORDS] = sh.high_words;
        map[H_SAMP] = sh.samp;
        map[H_SAMPS] = sh.samps;
        map[H_REV] = sh.rev;
        map[H_REV_SIZE] = (u64)sh.rev_size;
        map[H_WORDS] = sh.words;
    }
    row_key k;
    k.key = 0;
    k.id = -1;
    k.list = 0;
    k.bad = false;
    if (t < sh.n) k = key_of_row(perm, offsets, sh.nlist, sh.n_ids, sh.B, t);
    u64 prev = __shfl_up(k.key, 1);
    bool bad = k.bad;
    if (t < sh.n) {
        if (t > 0) {
            if (lane == 0) prev = key_of_row(perm, offsets, sh.nlist, sh.n_ids, sh.B, t - 1).key;
            bad |= k.key <= prev;   // neighbours of a list not ascending, or lists out of order
        }
        // key < nlist << B, so pos < high_words * 64
        const u64 pos = (k.key >> sh.L) + (u64)t;
        atomicOr(map + sh.high + (pos >> 6), 1ull << (pos & 63));
        if ((t & 255) == 0) map[sh.samp + (u64)(t >> 8)] = pos;
        if (k.id >= 0) {
            if (sh.rev_size == 2)
                reinterpret_cast<uint16_t*>(map + sh.rev)[k.id] = (uint16_t)k.list;
            else if (sh.rev_size == 4)
                reinterpret_cast<int32_t*>(map + sh.rev)[k.id] = (int32_t)k.list;
        }
    }
    if ((u64)t < sh.low_words) {   // this thread owns low word t: the fields that touch it
        const u64 first_bit = (u64)t * 64;
        const long long s0 = (long long)(first_bit / (u64)sh.L);
        const long long s1 = std::min<long long>((long long)((first_bit + 63) / (u64)sh.L), sh.n - 1);
        const u64 mask = low_mask(sh.L);
        u64 word = 0;
        for (long long s = s0; s <= s1; ++s) {
            const u64 f = key_of_row(perm, offsets, sh.nlist, sh.n_ids, sh.B, s).key & mask;
            const long long off = (long long)((u64)s * sh.L) - (long long)first_bit;
            word |= off >= 0 ? f << off : f >> -off;
        }
        map[sh.low + (u64)t] = word;
    }
    if (bad) atomicOr(err, 1ull);
}

// ---- ids of given rows ------------------------------------------------------------------
__global__ void __launch_bounds__(256)
idmap_ids(const u64* __restrict__ map, const long long* __restrict__ rows, long long count,
          long long* __restrict__ ids, u64* __restrict__ err) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const idmap_view v = view_of(map);
    const long long r = rows[i];
    long long out = r;   // a negative row (the padding of a search result) is copied through
    if (r >= 0) {
        u64 key = 0;
        out = r < v.n && select_key(v, r, &key) ? id_of_key(v, key) : -1;
        if (out < 0) atomicOr(err, 1ull);
    }
    ids[i] = out;
}

// ---- the streaming decode ---------------------------------------------------------------
// ids of the rows 256 * j + 64 * t + lane, t = 0 .. 3, of block j (256 * j < n), by one wave;
// -1 for a row from n on, and for a row whose bit is missing.  The block's high bits lie from
// its own sample up to the next block's (the end of the part for the last block): 64 words a
// step, a word per lane, the count of the rows before the step carried along.
__device__ __forceinline__ void decode_block(const idmap_view& v, long long j, int lane,
                                             long long ids[4]) {
    const long long base = j * 256;
    const int rows_in = (int)std::min<long long>(256, v.n - base);
    const u64 pos0 = v.samp[j];
    const u64 wfirst = pos0 >> 6;
    u64 wlast = base + 256 < v.n ? v.samp[j + 1] >> 6 : v.high_words - 1;
    if (wlast >= v.high_words) wlast = v.high_words - 1;
#pragma unroll
    for (int t = 0; t < 4; ++t) ids[t] = -1;
    int carried = 0;
    for (u64 w0 = wfirst; w0 <= wlast && carried < rows_in; w0 += 64) {
        const u64 w = w0 + (u64)lane;
        u64 word = w <= wlast ? v.high[w] : 0ull;
        if (w == wfirst) word &= ~0ull << (pos0 & 63);
        int incl = __popcll(word);
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        const int total = __shfl(incl, 63);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            // (carried and total are the same in every lane, so the whole pass is skipped
            // or taken by the wave as one: every shuffle below has all 64 lanes)
            if (64 * t + 63 < carried || 64 * t >= carried + total) continue;
            const int k = 64 * t + lane - carried;   // this lane's row, counted from the step's first
            int x = 0;                               // the lane whose word holds it: the first
            for (int step = 32; step; step >>= 1)    // with an inclusive count above k
                if (__shfl(incl, (x + step - 1) & 63) <= k) x += step;
            const u64 xw = __shfl(word, x & 63);
            const int before = __shfl(incl, x & 63) - __popcll(xw);
            if (k >= 0 && k < total && 64 * t + lane < rows_in) {
                const long long r = base + 64 * t + lane;
                const u64 pos = (w0 + (u64)x) * 64 + (u64)sel64(xw, k - before);
                ids[t] = id_of_key(v, ((pos - (u64)r) << v.L) | low_field(v, r));
            }
        }
        carried += total;
    }
}

__global__ void __launch_bounds__(256)
idmap_decode(const u64* __restrict__ map, long long first, long long count,
             long long* __restrict__ out, u64* __restrict__ err) {
    const idmap_view v = view_of(map);
    const int lane = threadIdx.x & 63;
    const long long j = (first >> 8) + (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j * 256 >= first + count) return;   // (the same for the whole wave)
    long long ids[4] = {-1, -1, -1, -1};
    if (j * 256 < v.n) decode_block(v, j, lane, ids);
    bool bad = false;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const long long r = j * 256 + 64 * t + lane;
        if (r >= first && r < first + count) {
            out[r - first] = ids[t];
            bad |= ids[t] < 0;   // a row from n on, or a bit that is missing
        }
    }
    if (bad) atomicOr(err, 1ull);
}

// bit s of the mask = keep[id(s)] != 0: idmap_decode with a ballot in place of the store; the
// wave's block of 256 rows is eight words, two per pass, stored by lanes 0 and 1
__global__ void __launch_bounds__(256)
idmap_pack(const unsigned char* __restrict__ keep, const u64* __restrict__ map, long long n,
           uint32_t* __restrict__ bits, u64* __restrict__ err) {
    const idmap_view v = view_of(map);
    const int lane = threadIdx.x & 63;
    const long long j = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j * 256 >= n) return;   // (the same for the whole wave)
    long long ids[4] = {-1, -1, -1, -1};
    if (n == v.n) decode_block(v, j, lane, ids);   // another n: no bit is set, and the error
    bool bad = false;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const long long r = j * 256 + 64 * t + lane;
        bool bit = false;
        if (r < n) {
            if (ids[t] >= 0) bit = keep[ids[t]] != 0;
            else bad = true;
        }
        const u64 b = __ballot(bit);
        const long long w = ((r - lane) >> 5) + lane;
        if (lane < 2 && w < (n + 31) >> 5) bits[w] = (uint32_t)(b >> (32 * lane));
    }
    if (bad) atomicOr(err, 1ull);
}

// ---- rows of given ids ------------------------------------------------------------------
__global__ void __launch_bounds__(256)
idmap_rows(const u64* __restrict__ map, const long long* __restrict__ offsets,
           const long long* __restrict__ ids, long long count, long long* __restrict__ rows,
           u64* __restrict__ err) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const idmap_view v = view_of(map);
    const long long id = ids[i];
    long long out = -1;
    bool bad = v.rev_size == 0 || id < 0 || id >= v.n_ids;
    if (!bad) {
        const long long l = v.rev_size == 2
            ? (long long)reinterpret_cast<const uint16_t*>(v.rev)[id]
            : (long long)reinterpret_cast<const int32_t*>(v.rev)[id];
        const bool none = v.rev_size == 2 ? l == 0xFFFF : l < 0;
        if (!none && l < v.nlist) {
            // the list's rows, cut to the stream whatever the offsets hold
            long long lo = std::min(std::max(offsets[l], 0ll), v.n);
            long long hi = std::min(std::max(offsets[l + 1], lo), v.n);
            const long long end = hi;
            const u64 want = ((u64)l << v.B) | (u64)id;
            while (lo < hi && !bad) {   // the first row of the list with a key >= want
                const long long mid = (lo + hi) >> 1;
                u64 key = 0;
                if (!select_key(v, mid, &key)) bad = true;
                else if (key < want) lo = mid + 1;
                else hi = mid;
            }
            u64 key = 0;
            if (!bad && lo < end && select_key(v, lo, &key) && key == want) out = lo;
        } else if (!none) {
            bad = true;
        }
    }
    rows[i] = out;
    if (bad) atomicOr(err, 1ull);
}

int check_map(const void* d_map) {
    return !d_map || (reinterpret_cast<uintptr_t>(d_map) & 7u) ? PQH_ERR_ARG : PQH_OK;
}

}  // namespace

extern "C" {

int pqh_idmap_bytes(long long n, long long n_ids, long long nlist, int reverse,
                    unsigned long long* bytes) {
    if (!bytes) return PQH_ERR_ARG;
    idmap_shape s;
    const int rc = shape_of(n, n_ids, nlist, reverse, &s);
    if (rc) return rc;
    *bytes = s.words * 8;
    return PQH_OK;
}

int pqh_idmap_build(pqh_ctx_t* ctx, const long long* d_perm, const long long* d_offsets,
                    long long n, long long nlist, long long n_ids, int reverse, void* d_map,
                    unsigned long long map_bytes) {
    if (!ctx) return pqh_no_ctx_status();
    idmap_shape s;
    int rc = shape_of(n, n_ids, nlist, reverse, &s);
    if (rc) return rc;
    if (check_map(d_map) || (n > 0 && (!d_perm || !d_offsets))) return PQH_ERR_ARG;
    if (map_bytes < s.words * 8) return PQH_ERR_CAPACITY;
    rc = pqh_use_device(ctx);
    if (rc) return rc;
    u64* map = static_cast<u64*>(d_map);
    // the cleared words the high bits are ORed into, every bit no field owns, and "none" in
    // every reverse entry (0xFFFF and -1 are both all ones)
    PQH_HIP(ctx, hipMemsetAsync(map, 0, s.words * 8, ctx->stream));
    if (s.rev_size && n_ids > 0)
        PQH_HIP(ctx, hipMemsetAsync(map + s.rev, 0xFF, (size_t)n_ids * s.rev_size, ctx->stream));
    const long long threads = std::max<long long>(n, 1);   // (n == 0: the header)
    hipLaunchKernelGGL(idmap_build, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0,
                       ctx->stream, d_perm, d_offsets, s, map, ctx->d_diag + kDiagIvf);
    PQH_LAUNCH_CHECK(ctx);
    return PQH_OK;
}

int pqh_idmap_ids(pqh_ctx_t* ctx, const void* d_map, const long long* d_rows, long long count,
                  long long* d_ids) {
    if (!ctx) return pqh_no_ctx_status();
    if (check_map(d_map) || count < 0 || (count > 0 && (!d_rows || !d_ids))) return PQH_ERR_ARG;
    const long long blocks = (count + 255) / 256;
    if (blocks > 0x7FFFFFFFll) return PQH_ERR_UNSUPPORTED;
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    if (count == 0) return PQH_OK;
    hipLaunchKernelGGL(idmap_ids, dim3((unsigned)blocks), dim3(256), 0, ctx->stream,
                       static_cast<const u64*>(d_map), d_rows, count, d_ids,
                       ctx->d_diag + kDiagIvf);
    PQH_LAUNCH_CHECK(ctx);
    return PQH_OK;
}

int pqh_idmap_decode(pqh_ctx_t* ctx, const void* d_map, long long first, long long count,
                     long long* d_ids) {
    if (!ctx) return pqh_no_ctx_status();
    if (check_map(d_map) || first < 0 || count < 0 || first > 0x7FFFFFFFll ||
        count > 0x7FFFFFFFll || (count > 0 && !d_ids))
        return PQH_ERR_ARG;
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    if (count == 0) return PQH_OK;
    const long long waves = ((first + count + 255) >> 8) - (first >> 8);
    hipLaunchKernelGGL(idmap_decode, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, ctx->stream,
                       static_cast<const u64*>(d_map), first, count, d_ids,
                       ctx->d_diag + kDiagIvf);
    PQH_LAUNCH_CHECK(ctx);
    return PQH_OK;
}

int pqh_idmap_rows(pqh_ctx_t* ctx, const void* d_map, const long long* d_offsets,
                   const long long* d_ids, long long count, long long* d_rows) {
    if (!ctx) return pqh_no_ctx_status();
    if (check_map(d_map) || count < 0 || (count > 0 && (!d_offsets || !d_ids || !d_rows)))
        return PQH_ERR_ARG;
    const long long blocks = (count + 255) / 256;
    if (blocks > 0x7FFFFFFFll) return PQH_ERR_UNSUPPORTED;
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    if (count == 0) return PQH_OK;
    hipLaunchKernelGGL(idmap_rows, dim3((unsigned)blocks), dim3(256), 0, ctx->stream,
                       static_cast<const u64*>(d_map), d_offsets, d_ids, count, d_rows,
                       ctx->d_diag + kDiagIvf);
    PQH_LAUNCH_CHECK(ctx);
    return PQH_OK;
}

int pqh_mask_pack_idmap(pqh_ctx_t* ctx, const unsigned char* d_keep, const void* d_map,
                        long long n, unsigned int* d_bits) {
    if (!ctx) return pqh_no_ctx_status();
    if (check_map(d_map) || n < 0 || n > 0x7FFFFFFFll || (n > 0 && (!d_keep || !d_bits)) ||
        (reinterpret_cast<uintptr_t>(d_bits) & 3u))
        return PQH_ERR_ARG;
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    if (n == 0) return PQH_OK;
    const long long waves = (n + 255) >> 8;
    hipLaunchKernelGGL(idmap_pack, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, ctx->stream,
                       d_keep, static_cast<const u64*>(d_map), n, d_bits, ctx->d_diag + kDiagIvf);
    PQH_LAUNCH_CHECK(ctx);
    return PQH_OK;
}

}  // extern "C"
