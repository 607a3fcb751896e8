// pqh_merge.hip -- the merge of several top-k results into one (pqh_topk_merge), and the
// collective of the sharded search built on it (pqh_shard_search_merge; include/pqh.h "sharded
// search").
//
//  topk_merge  one wave per query, kMergeQueries queries a workgroup: the wave walks the parts'
//              entries of its query 64 at a time through the list code of the search kernels
//              (pqh_topk_dev.h), kMergeLoads loads in flight a lane, and writes the list.  No
//              order is assumed inside a part (an IVF result is ordered by (dist, stream row),
//              not by id), so every offer takes the unsorted network or the serial inserts.
//              No LDS, no barrier: a wave never waits for another, and the result is the top_k
//              of a total order, whatever the launch shape.
//
// The sharded search: every rank's record travels in ONE all-gather,
//     bytes 0..7    int64 id_base
//     bytes 8..15   int64 status (0 = this rank's part is good)
//     bytes 16..    float dist[nq * k], padded with one zero float when nq * k is odd
//     then          int64 ids[nq * k]
// so that every field of every record is 8-byte aligned in the gathered buffer; the merge reads
// the records where the gather left them, the bases from the headers.
#include <type_traits>

#include "pqh_internal.h"
#include "pqh_topk_dev.h"

namespace {

constexpr int kMergeQueries = 4;   // waves a workgroup, a query each
constexpr int kMergeLoads = 4;     // offers whose loads are issued before the first offer

// where the parts lie: part p's entries of query q at d[p * d_stride + q * k_in ...] (and id
// likewise), its base at base[p * base_stride] (base NULL: zero).  fail (may be NULL): a
// non-zero word makes every output padding.
struct MergeSrc {
    const float* d;
    const long long* id;
    const long long* base;
    const long long* fail;
    long long d_stride, id_stride, base_stride;
};

template <bool WIDE>
__global__ void __launch_bounds__(64 * kMergeQueries)
topk_merge(MergeSrc s, int parts, long long nq, int k_in, int top_k, float* __restrict__ dist,
           long long* __restrict__ ids) {
    const int lane = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.y);
    const long long q = (long long)blockIdx.x * kMergeQueries + wave;
    if (q >= nq) return;   // (wave-uniform; no barrier follows)
    const int kth = top_k - 1;
    std::conditional_t<WIDE, TopKW, TopK> e;
    if constexpr (WIDE) {
        list_clear(e);
    } else {
        e.d = INFINITY;
        e.id = -1ll;
    }
    const bool failed = s.fail && *s.fail != 0;
    // an offer = 64 entries of one part: (p, c) counts them, c the 64-entry piece inside part p
    const int pieces = (int)(((long long)k_in + 63) >> 6);
    int p = failed ? parts : 0, c = 0;
#pragma unroll 1
    while (p < parts) {
        float d[kMergeLoads];
        long long id[kMergeLoads];
#pragma unroll
        for (int u = 0; u < kMergeLoads; ++u) {
            d[u] = INFINITY;
            id[u] = -1ll;
            if (p < parts) {   // (wave-uniform)
                const long long idx = (long long)c * 64 + lane;
                const long long base = s.base ? s.base[(long long)p * s.base_stride] : 0ll;
                if (idx < k_in) {
                    const long long at = q * k_in + idx;
                    d[u] = s.d[(long long)p * s.d_stride + at];
                    const long long v = s.id[(long long)p * s.id_stride + at];
                    id[u] = v < 0 ? -1ll : v + base;
                }
                if (++c == pieces) c = 0, ++p;
            }
        }
#pragma unroll
        for (int u = 0; u < kMergeLoads; ++u) list_offer<false>(e, d[u], id[u], id[u] >= 0, kth);
    }
    if constexpr (WIDE) {
#pragma unroll
        for (int b = 0; b < kWideKR; ++b) {
            if (b * 64 + lane < top_k) {
                dist[q * top_k + b * 64 + lane] = e.d[b];
                ids[q * top_k + b * 64 + lane] = e.id[b];
            }
        }
    } else if (lane < top_k) {
        dist[q * top_k + lane] = e.d;
        ids[q * top_k + lane] = e.id;
    }
}

int merge_launch(pqh_ctx_t* ctx, const MergeSrc& s, int parts, long long nq, int k_in, int top_k,
                 float* d_out_dist, long long* d_out_ids) {
    const dim3 grid((unsigned)((nq + kMergeQueries - 1) / kMergeQueries)), block(64, kMergeQueries);
    if (top_k > PQH_SEARCH_MAX_K)
        hipLaunchKernelGGL(topk_merge<true>, grid, block, 0, ctx->stream, s, parts, nq, k_in, top_k,
                           d_out_dist, d_out_ids);
    else
        hipLaunchKernelGGL(topk_merge<false>, grid, block, 0, ctx->stream, s, parts, nq, k_in,
                           top_k, d_out_dist, d_out_ids);
    PQH_LAUNCH_CHECK(ctx);
    return PQH_OK;
}

// ------------------------------------------------------------------- the sharded search
constexpr long long kRecHeader = 16;   // id_base, status

__host__ __device__ long long rec_dist_bytes(long long count) { return ((count * 4 + 7) / 8) * 8; }
long long rec_bytes(long long count) { return kRecHeader + rec_dist_bytes(count) + count * 8; }
// the scratch: [this rank's record][world records][the failure word, 8 B], padded to 256 B
unsigned long long search_scratch(int world, long long count) {
    return (unsigned long long)((rec_bytes(count) * (world + 1) + 8 + 255) / 256) * 256;
}

// this rank's record: the header, and with status == 0 the result behind it (otherwise the
// body is not read by anyone)
__global__ void shard_search_pack(const float* __restrict__ dist, const long long* __restrict__ ids,
                                  long long count, long long id_base, long long status,
                                  unsigned char* __restrict__ rec) {
    long long* const head = reinterpret_cast<long long*>(rec);
    float* const rd = reinterpret_cast<float*>(rec + kRecHeader);
    long long* const ri = reinterpret_cast<long long*>(rec + kRecHeader + rec_dist_bytes(count));
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0) {
        head[0] = id_base;
        head[1] = status;
        if (count & 1) rd[count] = 0.0f;
    }
    if (status != 0) return;
    for (long long i = t; i < count; i += (long long)gridDim.x * blockDim.x) {
        rd[i] = dist[i];
        ri[i] = ids[i];
    }
}

// the failure word from the gathered headers, for the merge and (state non-NULL) the caller
__global__ void shard_search_state(const unsigned char* __restrict__ recs, long long recb, int world,
                                   long long* __restrict__ fail, long long* __restrict__ state) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    long long bad = 0;
    for (int r = 0; r < world; ++r)
        bad |= reinterpret_cast<const long long*>(recs + r * recb)[1] != 0 ? 1ll : 0ll;
    *fail = bad;
    if (state) *state = bad;
}

}  // namespace

extern "C" {

int pqh_topk_merge(pqh_ctx_t* ctx, const float* d_dist, const long long* d_ids, int parts,
                   long long nq, int k_in, const long long* d_id_base, int top_k,
                   float* d_out_dist, long long* d_out_ids) {
    if (!ctx) return pqh_no_ctx_status();
    if (parts < 1 || k_in < 1 || nq < 0 || top_k < 1 || top_k > ctx->search_max_k)
        return PQH_ERR_ARG;
    if (nq > 0 && (!d_dist || !d_ids || !d_out_dist || !d_out_ids)) return PQH_ERR_ARG;
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    if (nq == 0) return PQH_OK;
    if (nq > 0x7FFFFFFFll) return PQH_ERR_UNSUPPORTED;
    const long long stride = nq * k_in;
    const MergeSrc s{d_dist, d_ids, d_id_base, nullptr, stride, stride, 1};
    return merge_launch(ctx, s, parts, nq, k_in, top_k, d_out_dist, d_out_ids);
}

unsigned long long pqh_shard_search_scratch_bytes(int world, long long nq, int k) {
    if (world < 1 || nq < 0 || nq > 0x7FFFFFFFll || k < 1 || k > PQH_SEARCH_MAX_K_WIDE) return 0;
    return search_scratch(world, nq * k);
}

int pqh_shard_search_merge(pqh_ctx_t* ctx, const pqh_shard_comm_t* comm, const float* d_dist,
                           const long long* d_ids, long long nq, int k, long long id_base,
                           int status, void* d_scratch, unsigned long long scratch_bytes,
                           float* d_out_dist, long long* d_out_ids, long long* d_state) {
    if (!ctx) return pqh_no_ctx_status();
    // without these the gather itself cannot run, or would not match the other ranks' sizes
    // (nq and k are the same on every rank, so every rank returns here together)
    if (!comm || comm->world <= 0 || comm->rank < 0 || comm->rank >= comm->world ||
        !comm->all_gather || nq < 0 || k < 1 || k > PQH_SEARCH_MAX_K_WIDE)
        return PQH_ERR_ARG;
    if (nq > 0x7FFFFFFFll) return PQH_ERR_UNSUPPORTED;
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    // everything else is local: the rank stays in the gather, its header says so
    int err = status;
    if (!err && (k > ctx->search_max_k || !d_out_dist || !d_out_ids || !d_state ||
                 (nq > 0 && (!d_dist || !d_ids)) || !d_scratch ||
                 (reinterpret_cast<uintptr_t>(d_scratch) & 7u)))
        err = PQH_ERR_ARG;
    const int world = comm->world;
    const long long count = nq * k, recb = rec_bytes(count);
    const unsigned long long need = search_scratch(world, count);
    if (!err && scratch_bytes < need) err = PQH_ERR_CAPACITY;
    unsigned char* sc = static_cast<unsigned char*>(d_scratch);
    if (!d_scratch || (reinterpret_cast<uintptr_t>(d_scratch) & 7u) || scratch_bytes < need) {
        // the gather still needs room for every rank's record: the context's own scratch
        rc = pqh_ensure_ws(ctx, (size_t)need);
        if (rc) return rc;
        sc = static_cast<unsigned char*>(ctx->ws);
    }
    unsigned char* const recs = sc + recb;
    long long* const fail = reinterpret_cast<long long*>(sc + recb * (world + 1));
    auto local = [&](int r) {   // the first local failure is kept
        if (r && !err) err = r;
    };
    const long long copy = err ? 0 : count;
    const unsigned blocks = (unsigned)(copy < 256 ? 1 : copy > 256ll * 1024 ? 1024 : (copy + 255) / 256);
    hipLaunchKernelGGL(shard_search_pack, dim3(blocks), dim3(256), 0, ctx->stream, d_dist, d_ids,
                       count, id_base, (long long)err, sc);
    // (a failed launch leaves a record nobody wrote: not sent as good -- the rank leaves here)
    PQH_LAUNCH_CHECK(ctx);
    if (comm->all_gather(comm->user, sc, recs, recb, ctx->stream))
        return pqh_set_error(ctx, PQH_ERR_COMM, "shard search all-gather failed");
    hipLaunchKernelGGL(shard_search_state, dim3(1), dim3(64), 0, ctx->stream, recs, recb, world,
                       fail, d_state);
    local(hipGetLastError() == hipSuccess ? PQH_OK : PQH_ERR_HIP);
    if (nq > 0 && d_out_dist && d_out_ids) {
        const MergeSrc s{reinterpret_cast<const float*>(recs + kRecHeader),
                         reinterpret_cast<const long long*>(recs + kRecHeader + rec_dist_bytes(count)),
                         reinterpret_cast<const long long*>(recs), fail, recb / 4, recb / 8,
                         recb / 8};
        local(merge_launch(ctx, s, world, nq, k, k, d_out_dist, d_out_ids));
    }
    return err;
}

int pqh_shard_search_status(pqh_ctx_t* ctx, const long long* d_state) {
    if (!ctx) return pqh_no_ctx_status();
    if (!d_state) return PQH_ERR_ARG;
    int rc = pqh_use_device(ctx);
    if (rc) return rc;
    long long bad = 0;
    PQH_HIP(ctx, hipMemcpyAsync(&bad, d_state, 8, hipMemcpyDeviceToHost, ctx->stream));
    PQH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return bad ? pqh_set_error(ctx, PQH_ERR_REMOTE, "a rank's part of the sharded search failed")
               : PQH_OK;
}

}  // extern "C"
