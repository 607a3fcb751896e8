/*
 * pqh.h -- the GPU batch boundary of pq_huffman_amd (C ABI, plain pointers and sizes).
 *
 * The reference has no FFI layer: its boundary is its C headers + CLI + file formats
 * (SURVEY.md 8b).  Its hot loops become the calls below; each names the reference code
 * it replaces.  All d_* pointers are DEVICE pointers owned by the caller; every call is
 * asynchronous on the context's HIP stream unless it says otherwise.  Calls return 0
 * (PQH_OK) or a negative pqh_status_t -- never assert or exit.  There is no CPU fallback:
 * without a usable GPU the calls return PQH_ERR_NO_DEVICE.
 *
 * Device data formats (shared with the CLI tools and the Python layer):
 *   codes        n x m row-major, uint8 (K <= 256) or uint16 (K <= 65536)
 *   counts       uint32 [m][K] (non-context) or [m][K*K] (context, index prev*K + cur)
 *   stream       byte stream exactly as huffman_indices.bin after its 8-byte header:
 *                vector-major, part-minor, MSB-first, zero padded at the end
 *   chunk index  (sidecar for parallel decode; not part of huffman_indices.bin)
 *                u64 bit offset of vector j*C for every chunk j, and in context mode
 *                the m codes of vector j*C-1 (row of chunk_prev) for j > 0
 */
#ifndef _PQH_H
#define _PQH_H

#include <stddef.h>
#include <stdint.h>

#include "fast_nn_block.h"
#include "huffman.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    PQH_OK = 0,
    PQH_ERR_ARG = -1,
    PQH_ERR_NO_DEVICE = -2,
    PQH_ERR_HIP = -3,
    PQH_ERR_UNSUPPORTED = -4,
    PQH_ERR_CODE_TOO_LONG = -5,  /* a Huffman code longer than 56 bits (needs N >= F(58)) */
    PQH_ERR_CORRUPT = -6,        /* invalid code in a stream */
    PQH_ERR_NOMEM = -7,
    PQH_ERR_CAPACITY = -8,       /* output buffer too small */
    PQH_ERR_REMOTE = -9,         /* another rank's part of a sharded call failed */
    PQH_ERR_COMM = -10           /* a collective hook of a sharded call failed */
} pqh_status_t;

typedef struct pqh_ctx pqh_ctx_t;

/* ---- context: one per device, one host thread per context ----------------------- */
/* creates the context with a private non-blocking stream */
int pqh_ctx_create(pqh_ctx_t** ctx, int device);
/* Like pqh_ctx_create, but the context's own stream may only use `cus` compute units,
 * spread evenly over the device (hipExtStreamCreateWithCUMask) -- for running the
 * latency-bound code-table build beside the next batch's assignment. */
int pqh_ctx_create_cu_limited(pqh_ctx_t** ctx, int device, int cus);
/* As pqh_ctx_create_cu_limited; complement != 0 takes every compute unit the cus-subset does
 * NOT use, so two contexts (cus, 0) and (cus, 1) run side by side on disjoint CUs.
 * cus < 0: every compute unit on a CU-masked stream, which HIP gives a hardware queue of its
 * own (streams without a mask share GPU_MAX_HW_QUEUES queues). */
int pqh_ctx_create_cu_split(pqh_ctx_t** ctx, int device, int cus, int complement);
/* the context's current HIP stream (e.g. for torch.cuda.ExternalStream) */
void* pqh_ctx_stream(const pqh_ctx_t* ctx);
int pqh_ctx_destroy(pqh_ctx_t* ctx);
/* Free the context's grow-only device scratch (workspace, the tiled encoder's tile images,
 * the one-pass encoder's look-back state, the sort's state) after synchronising its stream;
 * later calls allocate again as needed.  The largest is the encoder's: ~56 B per encoded
 * row (one worst-case image per 256-row tile) for pqh_encode_write*. */
int pqh_ctx_release_scratch(pqh_ctx_t* ctx);
/* run all later calls on hip_stream, taken literally: NULL is the device's default
 * (legacy, synchronising) stream -- what torch's current stream usually is. */
int pqh_ctx_set_stream(pqh_ctx_t* ctx, void* hip_stream);
int pqh_ctx_sync(pqh_ctx_t* ctx);
/* Per-context launch shapes of the kernels this context launches (results never change;
 * 0 restores the library default, which the PQH_* environment variable of the same name
 * can set process-wide):
 *   PQH_TUNE_ASSIGN_WGS_PER_CU  workgroups per CU of the K = 256 assignment grid (<= its
 *                               occupancy limit, 3): fewer leave SIMD room for kernels
 *                               running beside it on other streams (PQH_ASSIGN_WGS_PER_CU);
 *   PQH_TUNE_HIST_SPLIT         the context histogram's split of the previous-symbol range
 *                               (1, 2, 4 or 8): LDS per workgroup = 128 KB / split at K = 256
 *                               (PQH_HIST_SPLIT);
 *   PQH_TUNE_HIST_BLOCK         its workgroup size, 256 or 1024 threads (PQH_HIST_BLOCK);
 *   PQH_TUNE_ENC_IMPL           the whole-stream encoder of pqh_encode_write*: 1 = tiled
 *                               (tiles in context scratch, scan, placement), 2 = one pass
 *                               with a decoupled look-back (PQH_ENC_IMPL=onepass);
 *   PQH_TUNE_SEARCH_GROUPS      workgroups per query batch of the ADC scan (pqh_search_*;
 *                               default: the context's compute units over the batches).
 * A histogram that runs beside the assignment grid (on another stream) fits best at
 * split 4, 256 threads. */
enum { PQH_TUNE_ASSIGN_WGS_PER_CU = 1, PQH_TUNE_HIST_SPLIT = 2, PQH_TUNE_HIST_BLOCK = 3,
       PQH_TUNE_ENC_IMPL = 4, PQH_TUNE_SEARCH_GROUPS = 5 };
int pqh_ctx_set_tuning(pqh_ctx_t* ctx, int key, double value);
const char* pqh_status_string(int status);
const char* pqh_ctx_last_error(const pqh_ctx_t* ctx);
int pqh_device_count(int* count);

/* ---- PQ assignment (replaces yael kmeans' assignment, pq_encoder.c:270-273, and
 *      copy_cluster_indices :192-205) ----------------------------------------------- */
typedef struct pqh_pq pqh_pq_t;

/* centroids: host [m][k][dsub] fp32 (pq_centroids.fvecsl order). */
int pqh_pq_create(pqh_ctx_t* ctx, const float* centroids, int m, int k, int dsub, pqh_pq_t** pq);
int pqh_pq_destroy(pqh_pq_t* pq);

/* codes[v][i] = argmin_k sum_j (x[v][i*dsub+j] - c[i][k][j])^2, fp32 direct form, j
 * order, first minimum wins (oracle definition).  x rows are ld_x floats apart.
 * d_counts (optional, may be NULL): uint32 [m][k] non-context histogram accumulated
 * (+=) from the produced codes (huffman_encoder.c:139-164) -- fused in the kernel.
 * mode: 0 = MFMA screening + exact re-rank (default), 1 = exact VALU kernel only.
 * ctx: any context of the codebook's device; the launch uses its stream and scratch, so
 * contexts on different streams may assign concurrently. */
int pqh_pq_assign(pqh_ctx_t* ctx, const pqh_pq_t* pq, const float* d_x, long long n,
                  long long ld_x, void* d_codes, uint32_t* d_counts, int mode);
/* pqh_pq_assign writing the codes PART-MAJOR: codes of part i at d_codes[i * ld_codes + v]
 * (ld_codes >= n elements): each subspace's codes are contiguous, so the kernel stores
 * whole 128-byte lines (when d_codes is 128-byte aligned and ld_codes a multiple of 128
 * codes; any layout is correct) and a part's histogram reads one contiguous run (pqh_histogram_parts,
 * pqh_encode_write_parts consume this layout; pqh_transpose_codes converts to rows).
 * d_counts: as pqh_pq_assign (K <= 256 only). */
int pqh_pq_assign_parts(pqh_ctx_t* ctx, const pqh_pq_t* pq, const float* d_x, long long n,
                        long long ld_x, void* d_codes, long long ld_codes, uint32_t* d_counts,
                        int mode);
/* diagnostics of the last pqh_pq_assign (synchronises): vectors x parts re-ranked
 * exactly because the screening could not separate the best two centroids. */
int pqh_pq_last_rerank_count(pqh_ctx_t* ctx, unsigned long long* count);

/* mean squared reconstruction error (pq_encoder.c:82-119); synchronises. */
int pqh_pq_error(pqh_ctx_t* ctx, const pqh_pq_t* pq, const float* d_x, long long n,
                 long long ld_x, const void* d_codes, double* error_out);
/* x_hat[v] = concat_i c[i][codes[v][i]] (decode codes -> floats). */
int pqh_pq_reconstruct(pqh_ctx_t* ctx, const pqh_pq_t* pq, const void* d_codes, long long n,
                       float* d_out, long long ld_out);

/* ---- k-means training (replaces the training half of yael kmeans, pq_encoder.c:265-274) */
/* `iters` Lloyd iterations per subspace on the GPU: exact fp32 assignment (as
 * pqh_pq_assign) then centroid means; an empty cluster keeps its centroid.  Sums are
 * 64-bit fixed point (x * 2^s, s = 61 - ceil(log2(max|x| * n))), so the result is exact
 * and the same on every run.  centroids: host [m][k][dsub], initial in, trained out.
 * d_x rows are ld_x floats apart (subspace i = columns [i*dsub, (i+1)*dsub)).  Synchronous. */
int pqh_kmeans_train(pqh_ctx_t* ctx, const float* d_x, long long n, long long ld_x, int m,
                     int k, int dsub, int iters, float* centroids);

/* ---- symbol histograms (huffman_encoder.c:139-205) ------------------------------- */
/* counts += histogram of codes.  context: pairs (codes[v-1][i], codes[v][i]) for v >= 1,
 * plus (d_prev_row[i], codes[0][i]) when d_prev_row != NULL (the one-vector halo of a
 * shard boundary).  d_counts must be zeroed by the caller before the first call. */
int pqh_histogram(pqh_ctx_t* ctx, const void* d_codes, long long n, int m, int k, int context,
                  const void* d_prev_row, uint32_t* d_counts);
/* counts = histogram of codes (overwrites; no zeroing by the caller).  Same arguments. */
int pqh_histogram_set(pqh_ctx_t* ctx, const void* d_codes, long long n, int m, int k,
                      int context, const void* d_prev_row, uint32_t* d_counts);
/* The context histogram in two halves, for a pipelined caller that keeps the short first
 * half on its critical stream and moves the reduce to another (ordered by an event): the
 * per-chunk partial counts of the (prev, cur) pairs into d_partials (device,
 * pqh_histogram_partial_bytes(n, m, k) bytes, K <= 256), then counts (+)= their sum
 * (set != 0: overwrite).  Same pairs as pqh_histogram with context = 1. */
long long pqh_histogram_partial_bytes(long long n, int m, int k);
/* The same histograms over PART-MAJOR codes (pqh_pq_assign_parts: part i's codes at
 * d_codes[i * ld_codes + v]); set != 0 overwrites the counts.  d_prev_row stays a row of m
 * codes. */
int pqh_histogram_parts(pqh_ctx_t* ctx, const void* d_codes, long long ld_codes, long long n,
                        int m, int k, int context, const void* d_prev_row, uint32_t* d_counts,
                        int set);
int pqh_histogram_partial_parts(pqh_ctx_t* ctx, const void* d_codes, long long ld_codes,
                                long long n, int m, int k, const void* d_prev_row,
                                void* d_partials);
int pqh_histogram_partial(pqh_ctx_t* ctx, const void* d_codes, long long n, int m, int k,
                          const void* d_prev_row, void* d_partials);
int pqh_histogram_reduce(pqh_ctx_t* ctx, const void* d_partials, long long n, int m, int k,
                         uint32_t* d_counts, int set);

/* ---- code tables ------------------------------------------------------------------ */
/* Device-resident Huffman code tables of m parts: encode entries + decode lookup tables. */
typedef struct pqh_tables pqh_tables_t;

/* allocate tables for m parts of alphabet k (context: k must be 256) */
int pqh_tables_alloc(pqh_ctx_t* ctx, int m, int k, int context, pqh_tables_t** tables);
int pqh_tables_destroy(pqh_tables_t* tables);
/* Build every code on the GPU from device counts (pqh_histogram layout) -- the reference
 * codebook construction (huffman_codebook_[context_]encode_init, huffman_encode.c:141-269)
 * with its exact heap tie-breaks, one lane per alphabet; asynchronous, no host round trip.
 * Codes longer than 56 bits set an error reported by pqh_tables_status.  `ctx` may be any
 * context on the tables' device; the build is ordered on ctx's stream. */
int pqh_tables_build(pqh_ctx_t* ctx, pqh_tables_t* tables, const uint32_t* d_counts);
/* pqh_tables_build with the tree builder chosen by the caller (PQH_TREES_DEFAULT: the
 * PQH_TREE_IMPL environment choice, "lane" | "wave" | "grp").  K <= 256: GROUP = 16 lanes per
 * tree, four trees per wavefront, at most 32 VGPRs so it runs beside the assignment grid (the
 * default); LANE = one lane per tree; WAVE = one wavefront per tree with the heap in
 * registers.  K > 256: LANE = one lane per tree, otherwise one wavefront per tree.  Every
 * choice builds the same tables. */
enum { PQH_TREES_DEFAULT = 0, PQH_TREES_LANE = 1, PQH_TREES_WAVE = 2, PQH_TREES_GROUP = 3 };
int pqh_tables_build_impl(pqh_ctx_t* ctx, pqh_tables_t* t, const uint32_t* d_counts, int which);
/* The two halves of pqh_tables_build_impl, for callers that run them on different streams:
 * the Huffman trees (code table) on ctx's stream, then -- after the caller orders it behind
 * the trees (an event) -- the decode tables and the encoder's gather copy on ctx's stream.
 * With the K <= 256 group builder (PQH_TREES_GROUP, the default) the tree build writes the
 * encoder's gather copy itself, so pqh_encode* may run as soon as pqh_tables_build_trees is
 * done, concurrently with pqh_tables_build_luts (pqh_tables_encode_ready says which case
 * holds); pqh_decode always needs pqh_tables_build_luts. */
int pqh_tables_build_trees(pqh_ctx_t* ctx, pqh_tables_t* t, const uint32_t* d_counts, int which);
int pqh_tables_build_luts(pqh_ctx_t* ctx, pqh_tables_t* t);
/* 1 if the last pqh_tables_build_trees completed the encoder's tables (no LUT build needed
 * before pqh_encode*), else 0. */
int pqh_tables_encode_ready(const pqh_tables_t* t);
/* Two table sets (same m, K, mode) built by one launch of the default tree build (K <= 256:
 * the group builder, K > 256: one wavefront per tree): twice the trees in one latency-bound
 * pass, for a caller whose table builds are the bound; then both sets' decode tables.  Same
 * tables as two pqh_tables_build calls. */
int pqh_tables_build_pair(pqh_ctx_t* ctx, pqh_tables_t* t, const uint32_t* d_counts,
                          pqh_tables_t* t2, const uint32_t* d_counts2);
/* Load codes from m host codebooks (e.g. huffman_codebooks.bin read by huffman_codebook_load). */
int pqh_tables_upload(pqh_ctx_t* ctx, pqh_tables_t* tables, const huffman_codebook_t* codebooks);
/* alloc + upload */
int pqh_tables_create(pqh_ctx_t* ctx, const huffman_codebook_t* codebooks, int m,
                      pqh_tables_t** tables);
/* Synchronises; PQH_ERR_CODE_TOO_LONG if a GPU build of these tables since the last call
 * produced a code > 56 bits (the error is sticky until read here: a build issues no
 * zeroing dispatch of its own). */
int pqh_tables_status(pqh_ctx_t* ctx, const pqh_tables_t* tables);
/* Synchronises; fills m caller-provided structs with malloc'd host codebooks equal to the
 * tables (free with huffman_codebook_destroy) -- for huffman_codebook_save and stats. */
int pqh_tables_codebooks(pqh_ctx_t* ctx, const pqh_tables_t* tables, huffman_codebook_t* codebooks);

/* counts (host, double [m][items], huffman_encoder.c layout) -> host codebooks, built with
 * the reference's exact heap tie-breaks (huffman_encode.c:141-269).  Threads over parts
 * and context rows; codebooks must hold m uninitialised structs. */
int pqh_codebooks_build(const double* counts, int m, int k, int context,
                        huffman_codebook_t* codebooks, int num_threads);

/* ---- encode (huffman_encoder.c:207-238 + bitstream.c:71-150) --------------------- */
/* Total bits of the stream (device, u64) without writing it -- for placing shards before
 * they are written (multi-GPU); pqh_encode_write does not need it.
 * raw_first: context mode writes row 0 raw (8 bits per part, huffman_encoder.c:234) --
 * set for the shard holding global row 0; other shards pass d_prev_row instead. */
int pqh_encode_size(pqh_ctx_t* ctx, const pqh_tables_t* t, const void* d_codes, long long n,
                    int raw_first, const void* d_prev_row, unsigned long long* d_total_bits);
/* Write the stream at bit offset `bit_offset` of d_out (no pqh_encode_size needed): every
 * word of [bit_offset, bit_offset + bits) is stored exactly once, zero padding the last word
 * -- the buffer needs no zeroing.  By default 256-row tiles are coded into context scratch
 * (~56 B per row, grow-only; pqh_ctx_release_scratch frees it), scanned and placed; when that
 * scratch cannot be allocated (or PQH_ENC_IMPL=onepass) one pass whose workgroups find their
 * offsets by a decoupled look-back, with O(n / 256) state.  Bits of d_out before bit_offset in the first word are kept (they are
 * merged), so shards written at adjacent offsets into one buffer compose.
 * chunk_vectors > 0 also emits the chunk index: d_chunk_offsets[ceil(n/C)] (bit offsets
 * relative to d_out bit 0) and, in context mode, d_chunk_prev[ceil(n/C)][m] codes.
 * d_total_bits (optional, device u64): the number of bits written. */
int pqh_encode_write(pqh_ctx_t* ctx, const pqh_tables_t* t, const void* d_codes, long long n,
                     int raw_first, const void* d_prev_row, unsigned long long bit_offset,
                     unsigned char* d_out, unsigned long long out_bytes, int chunk_vectors,
                     unsigned long long* d_chunk_offsets, void* d_chunk_prev,
                     unsigned long long* d_total_bits);

/* pqh_encode_write for one shard of a multi-GPU stream, with the shard's GLOBAL bit offset
 * read from device memory (the exclusive scan of the shards' pqh_encode_size totals, e.g.
 * an all-gather + prefix sum on the device): no host round trip.  The shard is written at
 * bit (offset % 32) of d_out, whose word 0 is the global stream's word offset / 32, so the
 * shards' buffers compose by OR-ing their boundary words. */
int pqh_encode_write_at(pqh_ctx_t* ctx, const pqh_tables_t* t, const void* d_codes, long long n,
                        int raw_first, const void* d_prev_row,
                        const unsigned long long* d_global_bit_offset, unsigned char* d_out,
                        unsigned long long out_bytes, int chunk_vectors,
                        unsigned long long* d_chunk_offsets, void* d_chunk_prev,
                        unsigned long long* d_total_bits);

/* pqh_encode_write over PART-MAJOR codes (pqh_pq_assign_parts; part i of vector v at
 * d_codes[i * ld_codes + v]): the same stream, chunk index and chunk_prev rows.  The row
 * encoder only: K <= 256 and m = 8 or 16 (else PQH_ERR_UNSUPPORTED). */
int pqh_encode_write_parts(pqh_ctx_t* ctx, const pqh_tables_t* t, const void* d_codes,
                           long long ld_codes, long long n, int raw_first, const void* d_prev_row,
                           unsigned long long bit_offset, unsigned char* d_out,
                           unsigned long long out_bytes, int chunk_vectors,
                           unsigned long long* d_chunk_offsets, void* d_chunk_prev,
                           unsigned long long* d_total_bits);
/* part-major codes [m][ld_parts] -> rows [n][m] (pq_indices.bvecsl order); code_bytes 1 or 2. */
int pqh_transpose_codes(pqh_ctx_t* ctx, const void* d_parts, long long ld_parts, long long n, int m,
                        int code_bytes, void* d_rows);

/* Synchronises; PQH_ERR_CAPACITY if a pqh_encode_write since the last call had to drop
 * words because out_bytes was too small (nothing is written out of bounds). */
int pqh_encode_status(pqh_ctx_t* ctx);

/* ---- decode (huffman_decoder.c:211-255, huffman_decode.c:137-191) ---------------- */
/* Decodes n vectors from d_stream using the chunk index (C = chunk_vectors).  Context
 * mode: chunk 0 starts raw when raw_first, else from d_chunk_prev row 0.
 * Returns PQH_ERR_CORRUPT (after synchronising) if an invalid code was met. */
int pqh_decode(pqh_ctx_t* ctx, const pqh_tables_t* t, const unsigned char* d_stream,
               unsigned long long stream_bytes, long long n, int raw_first, int chunk_vectors,
               const unsigned long long* d_chunk_offsets, const void* d_chunk_prev,
               void* d_codes);
/* Synchronises; PQH_ERR_CORRUPT if a pqh_decode / pqh_decode_tree / random-access decode
 * (below) on this context since the last call met an invalid code (sticky until read here,
 * like pqh_encode_status); PQH_ERR_ARG if none did but a pqh_decode_select /
 * pqh_fetch_vectors was given a row id outside [0, n), or a pqh_decode_scatter a destination
 * outside [-1, n_out). */
int pqh_decode_status(pqh_ctx_t* ctx);

/* ---- random access through the chunk index (huffman_decoder.c:211-255 and
 *      huffman_decode.c:137-191 for the rows asked for only) --------------------------
 * The reference decoder reads a stream from its first bit; the chunk index lets a row be
 * reached from the start of its chunk: bit offset d_chunk_offsets[v / C], context
 * d_chunk_prev[v / C] (the raw first row for chunk 0 when raw_first), then the rows of the
 * chunk up to v.  Stream, index and raw_first are pqh_decode's arguments (so a shard written
 * with d_prev_row, raw_first = 0, is addressed by its own rows 0 ... n - 1); stream_bytes is
 * the readable length in whole 32-bit words, and nothing is read outside it.  The shapes of
 * pqh_decode: m <= 16 parts (else PQH_ERR_UNSUPPORTED), K <= 4096, context or not, any
 * C >= 1.  Asynchronous; errors are reported by pqh_decode_status: an invalid code, a chunk
 * offset or a symbol past stream_bytes * 8 bits is PQH_ERR_CORRUPT (the rows concerned are
 * zeroed), which takes precedence over a bad id.  count == 0 returns PQH_OK and launches
 * nothing.  Tree-mode streams (pqh_decode_tree) are out of scope: there a row's context is
 * its parent, not its predecessor, so the chunk index does not lead to it. */
/* d_codes[q] = row d_ids[q] of the stream, for q < count: one lane per id, ids in any order
 * and repeated at will (device int64).  An id outside [0, n) gives a zero row and
 * PQH_ERR_ARG from pqh_decode_status. */
int pqh_decode_select(pqh_ctx_t* ctx, const pqh_tables_t* t, const unsigned char* d_stream,
                      unsigned long long stream_bytes, long long n, int raw_first,
                      int chunk_vectors, const unsigned long long* d_chunk_offsets,
                      const void* d_chunk_prev, const long long* d_ids, long long count,
                      void* d_codes /* [count][m] */);
/* d_codes = rows [first, first + count) of the stream; first need not be a multiple of C.
 * One lane per chunk: the whole chunks of the range run pqh_decode's kernels, the cut ones
 * at its ends store only their rows inside the range.  first < 0 or first + count > n
 * returns PQH_ERR_ARG at once. */
int pqh_decode_range(pqh_ctx_t* ctx, const pqh_tables_t* t, const unsigned char* d_stream,
                     unsigned long long stream_bytes, long long n, int raw_first, int chunk_vectors,
                     const unsigned long long* d_chunk_offsets, const void* d_chunk_prev,
                     long long first, long long count, void* d_codes /* [count][m] */);
/* pqh_decode_select fused with pqh_pq_reconstruct: d_out[q] = concat_i c[i][code_i] of row
 * d_ids[q] in fp32, rows ld_out floats apart (the floats between rows are left alone); the
 * codes are not written to memory.  pq and t must agree in m and K.  A bad id gives a row
 * of zeros. */
int pqh_fetch_vectors(pqh_ctx_t* ctx, const pqh_tables_t* t, const pqh_pq_t* pq,
                      const unsigned char* d_stream, unsigned long long stream_bytes, long long n,
                      int raw_first, int chunk_vectors, const unsigned long long* d_chunk_offsets,
                      const void* d_chunk_prev, const long long* d_ids, long long count,
                      float* d_out, long long ld_out);
/* ---- search: asymmetric distance (ADC) top-k over a stream or over plain codes ---------
 * A PQ store is searched with one table per query, lut[i][c] = the distance part of
 * sub-vector i to centroid c; a row's distance is the sum of its m entries and the top_k
 * smallest win.  pqh_search_stream decodes the stream chunk by chunk as pqh_decode does and
 * scores every row where pqh_decode would store it: the codes are never written.  Its ids go
 * straight into pqh_fetch_vectors for an exact re-rank.
 * Device pointers, asynchronous on the context's stream.  A NULL context -- all a process
 * without a GPU can have -- returns PQH_ERR_NO_DEVICE when no HIP device is visible and
 * PQH_ERR_ARG otherwise; that check comes first, every other argument check after it.
 * PQH_ERR_ARG: a null pointer, top_k < 1 or > the context's limit (PQH_SEARCH_MAX_K unless
 * pqh_ctx_set_search_max_k raised it), chunk_vectors < 1, a negative count.  PQH_ERR_UNSUPPORTED: K > 256 (a K = 4096 table is 128 KB per query: no
 * batch of them fits the LDS), m > 16, a chunk of more than ~90 KB of codes (C * m).
 * Tree-mode streams are out of scope, as for random access.  nq == 0 launches nothing; n == 0
 * fills the outputs with the padding.  The tables may hold any finite floats (negative ones,
 * inner products); the result for NaN entries is unspecified.
 * Scratch: 12 bytes * nq * top_k per workgroup of the scan grid, in the context workspace. */
#define PQH_SEARCH_MAX_K 64
/* The limit of top_k (and of pqh_refine_*'s ncand) is the context's: PQH_SEARCH_MAX_K for a new
 * context, up to PQH_SEARCH_MAX_K_WIDE after pqh_ctx_set_search_max_k (64 <= max_k <= 256,
 * else PQH_ERR_ARG).  Calls with top_k <= 64 launch the same kernels whatever the limit is;
 * above 64 a scan keeps four entries a lane (a list of 256 per wave), scores four queries a
 * workgroup at the most, and the scratch grows with top_k as stated above.  The results have
 * the same definition at every width.  Not a pqh_ctx_set_tuning key: tuning never changes
 * what a call returns, and this changes which calls are accepted.  pqh_ctx_search_max_k
 * returns the limit.  A NULL context answers as in the search calls. */
#define PQH_SEARCH_MAX_K_WIDE 256
int pqh_ctx_set_search_max_k(pqh_ctx_t* ctx, int max_k);
int pqh_ctx_search_max_k(const pqh_ctx_t* ctx);

/* lut[q][i][c] = sum_j (query[q][i*dsub+j] - cent[i][c][j])^2: fp32, j order, no contraction
 * (the oracle arithmetic of pqh_pq_assign).  d_lut: device float [nq][m][K].  K <= 256.
 * Query rows are ld_q >= m * dsub floats apart. */
int pqh_adc_tables(pqh_ctx_t* ctx, const pqh_pq_t* pq, const float* d_queries, long long nq,
                   long long ld_q, float* d_lut);

/* For each query q < nq: the top_k rows of the stream with the smallest
 * dist(v) = ((lut[q][0][c_0] + lut[q][1][c_1]) + ...) + lut[q][m-1][c_{m-1}]
 * (fp32, parts added left to right), ordered by (dist, row id) ascending -- fp32 `<` on the
 * value, then on the id, so the result is unique; ids are row numbers in the stream plus
 * id_base.  d_dist float [nq][top_k], d_ids int64 [nq][top_k]; when n < top_k the tail is
 * (+inf, -1).  Stream, index and raw_first are pqh_decode's.
 * Decode errors are pqh_decode_select's: an invalid code, a chunk offset or a symbol past
 * stream_bytes * 8 bits make pqh_decode_status answer PQH_ERR_CORRUPT, and the rows of the
 * failed chunk take no part in the result; a start past the stream is refused before
 * anything is read, and nothing is read outside the stream. */
int pqh_search_stream(pqh_ctx_t* ctx, const pqh_tables_t* t, const unsigned char* d_stream,
                      unsigned long long stream_bytes, long long n, int raw_first,
                      int chunk_vectors, const unsigned long long* d_chunk_offsets,
                      const void* d_chunk_prev, const float* d_lut, long long nq, int top_k,
                      long long id_base, float* d_dist, long long* d_ids);

/* The same scan over plain row-major u8 codes [n][m]; k = the table width K. */
int pqh_search_codes(pqh_ctx_t* ctx, const void* d_codes, long long n, int m, int k,
                     const float* d_lut, long long nq, int top_k, long long id_base,
                     float* d_dist, long long* d_ids);

/* The probe search: the same top_k, but query q looks only at its own row ranges, the way an
 * inverted file is searched -- the rows stored list by list and a query probing the few lists
 * nearest to it.  The probe list is in CSR form, all of it device data (a coarse quantizer on
 * the GPU hands it over without a host round trip): query q scans the ranges
 * d_range_ptr[q] ... d_range_ptr[q + 1] - 1, and range r is the rows
 * [d_ranges[2r], d_ranges[2r] + d_ranges[2r + 1]) of the stream.  d_range_ptr int64 [nq + 1],
 * d_ranges int64 [nr][2].  Arithmetic, order, padding and id_base are pqh_search_stream's, and
 * the result does not depend on the grid.
 * A range need not start or end on a chunk boundary: a chunk that is cut is decoded from its
 * start (chunk 0 with its raw first row) as far as the range goes, and only its rows inside
 * the range are scored.  A chunk with no row in any range of a query is neither read nor
 * decoded for that query, so the sound part of a damaged stream can be searched without
 * PQH_ERR_CORRUPT; the decode errors are pqh_search_stream's for the chunks that are walked.
 * The ranges of a query may overlap: a row is offered once for every range that holds it and
 * may appear that many times in the result (no dedup).  count == 0 is an empty range, a query
 * without ranges gets the padding.
 * Bad values are reported as pqh_decode_select reports a bad id, by PQH_ERR_ARG from
 * pqh_decode_status (PQH_ERR_CORRUPT takes precedence): a range with first < 0, count < 0,
 * first > n or count > n - first is skipped as a whole; a query whose
 * [d_range_ptr[q], d_range_ptr[q + 1]) is reversed or leaves [0, nr] scans nothing.  Every
 * other range and query gives its exact result.
 * PQH_ERR_ARG at once: the cases of pqh_search_stream, nr < 0, a null d_range_ptr when
 * nq > 0, a null d_ranges when nq > 0 and nr > 0.  nq == 0 launches nothing; n == 0 or
 * nr == 0 fills the outputs with the padding.
 * Scratch: 12 bytes * nq * top_k per workgroup of the scan grid and 8 * (nr + 1) bytes. */
int pqh_search_stream_ranges(pqh_ctx_t* ctx, const pqh_tables_t* t, const unsigned char* d_stream,
                             unsigned long long stream_bytes, long long n, int raw_first,
                             int chunk_vectors, const unsigned long long* d_chunk_offsets,
                             const void* d_chunk_prev, const float* d_lut, long long nq,
                             const long long* d_range_ptr /* [nq + 1] */,
                             const long long* d_ranges /* [nr][2] */, long long nr, int top_k,
                             long long id_base, float* d_dist, long long* d_ids);

/* The same over plain row-major u8 codes [n][m]. */
int pqh_search_codes_ranges(pqh_ctx_t* ctx, const void* d_codes, long long n, int m, int k,
                            const float* d_lut, long long nq, const long long* d_range_ptr,
                            const long long* d_ranges, long long nr, int top_k, long long id_base,
                            float* d_dist, long long* d_ids);

/* The probe search with one table per range instead of one per query: d_lut is float
 * [nr][m][K] and range r is scored with table r -- what a residual inverted file needs, where
 * the table of a (query, list) pair is that of query - centroid[list]
 * (pqh_adc_tables_residual).  Everything else is pqh_search_stream_ranges': the arguments,
 * arithmetic, order (dist, stream row), padding, id_base, cut chunks, overlapping ranges, the
 * bad values that are skipped and reported by pqh_decode_status, the chunks that are never
 * read, the independence of the grid and the scratch.  With d_lut[r] = the table of the query
 * that owns range r the result is pqh_search_stream_ranges' bit for bit.  The table of a range
 * without rows (empty or bad) is never read. */
int pqh_search_stream_range_tables(pqh_ctx_t* ctx, const pqh_tables_t* t,
                                   const unsigned char* d_stream, unsigned long long stream_bytes,
                                   long long n, int raw_first, int chunk_vectors,
                                   const unsigned long long* d_chunk_offsets,
                                   const void* d_chunk_prev, const float* d_lut /* [nr][m][K] */,
                                   long long nq, const long long* d_range_ptr /* [nq + 1] */,
                                   const long long* d_ranges /* [nr][2] */, long long nr,
                                   int top_k, long long id_base, float* d_dist, long long* d_ids);

/* The same over plain row-major u8 codes [n][m]. */
int pqh_search_codes_range_tables(pqh_ctx_t* ctx, const void* d_codes, long long n, int m, int k,
                                  const float* d_lut /* [nr][m][K] */, long long nq,
                                  const long long* d_range_ptr, const long long* d_ranges,
                                  long long nr, int top_k, long long id_base, float* d_dist,
                                  long long* d_ids);

/* The probe search in list-major order: the same result, but a list that several queries
 * probe is decoded once per batch of them instead of once per query -- the schedule for many
 * queries, when nq * nprobe exceeds nlist and the same lists are probed again and again.
 * The probe list is given as pqh_coarse_probe writes it: d_offsets int64 [nlist + 1] (list l is
 * the stream rows [d_offsets[l], d_offsets[l + 1])) and d_probes int64 [nq][nprobe], -1 = none.
 * tables_per_probe == 0: d_lut is float [nq][m][K] and the result is
 * pqh_search_stream_ranges' for the ranges of these probes (range q * nprobe + p = list
 * d_probes[q][p]); tables_per_probe != 0: d_lut is float [nq * nprobe][m][K], pair (q, p)
 * scored with table q * nprobe + p, and the result is pqh_search_stream_range_tables' --
 * either way id for id and bit for bit, since the order (dist, stream row) is total and dist
 * the same sum.  A list that appears twice in a query's probes offers its rows twice (each
 * time with its own table, if there is one per probe); a probe of -1 contributes nothing and
 * its table is never read, nor is that of a list without rows.
 * On the device the probes are turned round (for every list the pairs that probe it), cut
 * into work units of a list and up to 8 pairs (4 when m > 8), and a unit's workgroups decode
 * the list's chunks once and score every row against the unit's tables.  Chunks under no
 * probed list are neither read nor walked.
 * Bad device data is reported by PQH_ERR_ARG from pqh_decode_status (PQH_ERR_CORRUPT takes
 * precedence) and contributes no rows: a probe below -1 or >= nlist, a probed list whose
 * offsets are not 0 <= d_offsets[l] <= d_offsets[l + 1] <= n.  Decode errors are
 * pqh_search_stream_ranges' for the chunks that are walked.
 * PQH_ERR_ARG at once: the cases of pqh_search_stream, nlist < 1, nprobe < 1, a null
 * d_offsets or d_probes when nq > 0.  PQH_ERR_UNSUPPORTED: those of pqh_search_stream,
 * nq * nprobe >= 2^31, nlist >= 2^31.  nq == 0 launches nothing; n == 0 fills the outputs with
 * the padding.  The call never waits for the device.
 * Scratch: 12 bytes * nq * nprobe * top_k per workgroup row of the scan grid, and
 * 4 * (nq * nprobe + nlist) + 24 * min(nq * nprobe, nlist + nq * nprobe / 4) bytes. */
int pqh_search_stream_lists(pqh_ctx_t* ctx, const pqh_tables_t* t, const unsigned char* d_stream,
                            unsigned long long stream_bytes, long long n, int raw_first,
                            int chunk_vectors, const unsigned long long* d_chunk_offsets,
                            const void* d_chunk_prev, const long long* d_offsets /* [nlist + 1] */,
                            long long nlist, const long long* d_probes /* [nq][nprobe] */,
                            long long nq, int nprobe, const float* d_lut, int tables_per_probe,
                            int top_k, long long id_base, float* d_dist, long long* d_ids);

/* The same over plain row-major u8 codes [n][m]. */
int pqh_search_codes_lists(pqh_ctx_t* ctx, const void* d_codes, long long n, int m, int k,
                           const long long* d_offsets, long long nlist, const long long* d_probes,
                           long long nq, int nprobe, const float* d_lut, int tables_per_probe,
                           int top_k, long long id_base, float* d_dist, long long* d_ids);

/* Filtered search: every search call above has a _masked counterpart that takes a row mask,
 * d_keep, after d_ids and returns the call's result restricted to the rows the mask keeps.
 * The mask is a device array of ceil(n / 32) 32-bit words, one per call and shared by all its
 * queries: bit r & 31 of word r >> 5 is set when stream row r may be returned.  The bits from
 * n on in the last word may hold anything and are ignored; the words need 4-byte alignment
 * only (PQH_ERR_ARG otherwise) and are only read.  pqh_mask_pack makes one from a byte per row.
 * The result is the unfiltered call's definition over the kept rows: the top_k by (dist, id)
 * among the rows that are kept and -- in the probe forms -- inside the query's ranges or lists,
 * dist the same fp32 sum, padded with (+inf, -1), ids moved by id_base, independent of the
 * grid.  It is not the unfiltered result with the dropped rows taken out: a query gets top_k
 * kept rows whenever that many are in its reach.
 * d_keep == NULL is no filter: the call is then the unfiltered one, launch for launch.  The
 * argument checks, the limits, the scratch and the behaviour of nq == 0, n == 0 and nr == 0 are
 * the unfiltered call's.
 * What is not kept is not decoded: a chunk is walked only as far as its last kept row (inside
 * the range or list, in the probe forms), a chunk without a kept row is neither read nor
 * walked, and a step of 64 chunks without a kept row costs the read of its mask words.  So the
 * decode errors (PQH_ERR_CORRUPT from pqh_decode_status) are raised only for the chunks that
 * are walked, and within them only up to the last kept row, as the range forms raise them only
 * for the chunks under a range: a damaged chunk whose rows are all masked out is not reported,
 * and an all-zero mask reports nothing.  The bad ranges, range_ptr entries, probes and offsets
 * of the probe forms are reported whatever the mask holds. */
int pqh_search_stream_masked(pqh_ctx_t* ctx, const pqh_tables_t* t, const unsigned char* d_stream,
                             unsigned long long stream_bytes, long long n, int raw_first,
                             int chunk_vectors, const unsigned long long* d_chunk_offsets,
                             const void* d_chunk_prev, const float* d_lut, long long nq, int top_k,
                             long long id_base, float* d_dist, long long* d_ids,
                             const unsigned int* d_keep /* [ceil(n / 32)] or NULL */);
int pqh_search_codes_masked(pqh_ctx_t* ctx, const void* d_codes, long long n, int m, int k,
                            const float* d_lut, long long nq, int top_k, long long id_base,
                            float* d_dist, long long* d_ids, const unsigned int* d_keep);
int pqh_search_stream_ranges_masked(pqh_ctx_t* ctx, const pqh_tables_t* t,
                                    const unsigned char* d_stream, unsigned long long stream_bytes,
                                    long long n, int raw_first, int chunk_vectors,
                                    const unsigned long long* d_chunk_offsets,
                                    const void* d_chunk_prev, const float* d_lut, long long nq,
                                    const long long* d_range_ptr, const long long* d_ranges,
                                    long long nr, int top_k, long long id_base, float* d_dist,
                                    long long* d_ids, const unsigned int* d_keep);
int pqh_search_codes_ranges_masked(pqh_ctx_t* ctx, const void* d_codes, long long n, int m, int k,
                                   const float* d_lut, long long nq, const long long* d_range_ptr,
                                   const long long* d_ranges, long long nr, int top_k,
                                   long long id_base, float* d_dist, long long* d_ids,
                                   const unsigned int* d_keep);
int pqh_search_stream_range_tables_masked(pqh_ctx_t* ctx, const pqh_tables_t* t,
                                          const unsigned char* d_stream,
                                          unsigned long long stream_bytes, long long n,
                                          int raw_first, int chunk_vectors,
                                          const unsigned long long* d_chunk_offsets,
                                          const void* d_chunk_prev, const float* d_lut,
                                          long long nq, const long long* d_range_ptr,
                                          const long long* d_ranges, long long nr, int top_k,
                                          long long id_base, float* d_dist, long long* d_ids,
                                          const unsigned int* d_keep);
int pqh_search_codes_range_tables_masked(pqh_ctx_t* ctx, const void* d_codes, long long n, int m,
                                         int k, const float* d_lut, long long nq,
                                         const long long* d_range_ptr, const long long* d_ranges,
                                         long long nr, int top_k, long long id_base, float* d_dist,
                                         long long* d_ids, const unsigned int* d_keep);
int pqh_search_stream_lists_masked(pqh_ctx_t* ctx, const pqh_tables_t* t,
                                   const unsigned char* d_stream, unsigned long long stream_bytes,
                                   long long n, int raw_first, int chunk_vectors,
                                   const unsigned long long* d_chunk_offsets,
                                   const void* d_chunk_prev, const long long* d_offsets,
                                   long long nlist, const long long* d_probes, long long nq,
                                   int nprobe, const float* d_lut, int tables_per_probe, int top_k,
                                   long long id_base, float* d_dist, long long* d_ids,
                                   const unsigned int* d_keep);
int pqh_search_codes_lists_masked(pqh_ctx_t* ctx, const void* d_codes, long long n, int m, int k,
                                  const long long* d_offsets, long long nlist,
                                  const long long* d_probes, long long nq, int nprobe,
                                  const float* d_lut, int tables_per_probe, int top_k,
                                  long long id_base, float* d_dist, long long* d_ids,
                                  const unsigned int* d_keep);

/* Range search: every scanned row v with dist(q, v) < d_radius[q] (strict), as many as there
 * are -- what no fixed top_k can give.  dist is the searches' own fp32 sum, ((lut[0][c_0] +
 * lut[1][c_1]) + ...) without contraction.  A NaN radius or a NaN distance gives no hit;
 * radius = +inf gives every row whose distance is below +inf.
 * The rows scanned are those of the searches above, by the probe list:
 *   d_range_ptr == NULL, d_ranges == NULL, nr == -1, tables_per_range == 0: the whole stream,
 *     d_lut [nq][m][K] (pqh_search_stream / pqh_search_codes);
 *   else query q's ranges d_ranges[r] = (first row, count), r in [d_range_ptr[q],
 *     d_range_ptr[q + 1]), with d_lut [nq][m][K] (tables_per_range == 0, pqh_search_*_ranges) or
 *     one table per range, d_lut [nr][m][K] (tables_per_range != 0, pqh_search_*_range_tables).
 * d_keep: the row mask of the _masked calls ([ceil(n / 32)] words, only kept rows are hits and
 * what is not kept is not decoded) or NULL.
 * The result is CSR: d_lims [nq + 1] (int64, d_lims[0] = 0), and d_dist / d_ids entries
 * [d_lims[q], d_lims[q + 1]) for query q, ids = stream rows + id_base, in scan order: ascending
 * stream row for the whole stream; in the probe forms range by range in the order of the
 * query's list, ascending row inside a range, and a row under two overlapping or repeated
 * ranges once per range.  Bits and order do not depend on the grid or on
 * PQH_TUNE_SEARCH_GROUPS.
 * Two passes over a plan in the CALLER's device memory (8-byte aligned, at least
 * pqh_range_plan_bytes bytes: a header, 8 bytes per query, workgroup and wave of the scan, and
 * 8 per batch of queries, workgroup and wave):
 *   pqh_range_count_*  scans, counts every wave's hits per query into the plan, turns the counts
 *                      into offsets and writes d_lims.  The header records the launch geometry.
 *   pqh_range_fill_*   takes the same arguments, the plan and d_lims as the count left them, and
 *                      scans again: every wave writes its hits from its offset on.  Entry p is
 *                      written only if p < capacity, so a buffer that is too small holds the
 *                      first `capacity` entries of the full result and nothing past it is
 *                      touched; d_lims always holds the full counts, and truncation is no error
 *                      (compare d_lims[nq] with capacity).  A wave whose share of the scan
 *                      counted no hit decodes nothing, and one that has written all it counted
 *                      stops.  The fill may be repeated.
 * Nothing on the context has to survive between the two calls.  A fill whose own geometry is
 * not the plan's (the tuning changed in between, another n or nq) writes nothing and sets the
 * sticky bit that pqh_decode_status reports as PQH_ERR_ARG.
 * Async.  The checks, limits (K <= 256, m <= 16, else PQH_ERR_UNSUPPORTED) and errors are the
 * searches': a NULL context is answered first; a chunk offset or symbol past the stream or an
 * invalid code gives PQH_ERR_CORRUPT from pqh_decode_status and the rows of that chunk are no
 * hits; a bad range or d_range_ptr entry gives PQH_ERR_ARG there and no steps; plan_bytes below
 * pqh_range_plan_bytes is PQH_ERR_ARG.  nq == 0, n == 0 and nr == 0 launch at most the write of
 * d_lims (all zero).
 * pqh_range_plan_bytes: chunk_vectors = 0 for the *_codes calls. */
int pqh_range_plan_bytes(pqh_ctx_t* ctx, long long n, int m, int k, int chunk_vectors,
                         long long nq, long long nr /* -1: the whole stream */,
                         int tables_per_range, unsigned long long* bytes);
int pqh_range_count_stream(pqh_ctx_t* ctx, const pqh_tables_t* t, const unsigned char* d_stream,
                           unsigned long long stream_bytes, long long n, int raw_first,
                           int chunk_vectors, const unsigned long long* d_chunk_offsets,
                           const void* d_chunk_prev, const float* d_lut, long long nq,
                           const long long* d_range_ptr, const long long* d_ranges, long long nr,
                           int tables_per_range, const float* d_radius /* [nq] */,
                           const unsigned int* d_keep /* [ceil(n / 32)] or NULL */, void* d_plan,
                           unsigned long long plan_bytes, long long* d_lims /* [nq + 1] */);
int pqh_range_fill_stream(pqh_ctx_t* ctx, const pqh_tables_t* t, const unsigned char* d_stream,
                          unsigned long long stream_bytes, long long n, int raw_first,
                          int chunk_vectors, const unsigned long long* d_chunk_offsets,
                          const void* d_chunk_prev, const float* d_lut, long long nq,
                          const long long* d_range_ptr, const long long* d_ranges, long long nr,
                          int tables_per_range, const float* d_radius, const unsigned int* d_keep,
                          const void* d_plan, unsigned long long plan_bytes,
                          const long long* d_lims, long long capacity, long long id_base,
                          float* d_dist /* [capacity] */, long long* d_ids /* [capacity] */);
int pqh_range_count_codes(pqh_ctx_t* ctx, const void* d_codes, long long n, int m, int k,
                          const float* d_lut, long long nq, const long long* d_range_ptr,
                          const long long* d_ranges, long long nr, int tables_per_range,
                          const float* d_radius, const unsigned int* d_keep, void* d_plan,
                          unsigned long long plan_bytes, long long* d_lims);
int pqh_range_fill_codes(pqh_ctx_t* ctx, const void* d_codes, long long n, int m, int k,
                         const float* d_lut, long long nq, const long long* d_range_ptr,
                         const long long* d_ranges, long long nr, int tables_per_range,
                         const float* d_radius, const unsigned int* d_keep, const void* d_plan,
                         unsigned long long plan_bytes, const long long* d_lims,
                         long long capacity, long long id_base, float* d_dist, long long* d_ids);

/* ---- inverted file: coarse quantizer, list layout, probe selection ---------------------
 * The front end of the probe search: rows are assigned to the nearest of nlist coarse
 * centroids (full d-dimensional vectors), stored list by list, and a query probes the nprobe
 * lists nearest to it.  pqh_coarse_probe writes the CSR probe list pqh_search_*_ranges take,
 * on the device, so the whole path from queries to neighbour ids runs without a host round
 * trip.
 * Conventions of the search calls: device pointers unless said otherwise, asynchronous on the
 * context's stream; a NULL context returns PQH_ERR_NO_DEVICE when no HIP device is visible and
 * PQH_ERR_ARG otherwise, checked before anything else.
 * The distance is dist(x, c) = sum_j (x[j] - c[j])^2 in fp32, the direct form: one subtract,
 * one multiply and one add per element, j ascending, no contraction -- the arithmetic of
 * pqh_pq_assign and pqh_adc_tables.  The order is (dist, list id) ascending, so the first of
 * several equal minima wins and every result is unique and independent of the launch shape.
 * Results for NaN or infinite inputs (or sums that overflow) are unspecified; nothing is read
 * or written out of bounds in any case.
 * Limits: 1 <= d <= PQH_IVF_MAX_D and 1 <= nlist <= PQH_IVF_MAX_NLIST, any d (no multiple of
 * anything); beyond them PQH_ERR_UNSUPPORTED.  pqh_ivf_layout takes n < 2^31 rows,
 * pqh_coarse_probe nq < 2^31 queries. */
typedef struct pqh_coarse pqh_coarse_t;
#define PQH_IVF_MAX_NPROBE 64          /* = PQH_SEARCH_MAX_K: the same wave-wide list */
#define PQH_IVF_MAX_NLIST (1 << 24)
#define PQH_IVF_MAX_D 65536

/* centroids: HOST [nlist][d] fp32.  The device keeps two copies, [nlist][d] for the assignment
 * and [d][nlist] for the probe selection (8 * nlist * d bytes); synchronous. */
int pqh_coarse_create(pqh_ctx_t* ctx, const float* centroids, int nlist, int d, pqh_coarse_t** cq);
/* Synchronises the stream of the context it was made with, which must still exist. */
int pqh_coarse_destroy(pqh_coarse_t* cq);

/* d_list[v] = argmin_l dist(x[v], c[l]), the first minimum.  d_list int32 [n]; rows ld_x >= d
 * floats apart, the floats between rows never read.  d_dist (optional, may be NULL): float
 * [n], the winning distance.  n == 0 launches nothing. */
int pqh_coarse_assign(pqh_ctx_t* ctx, const pqh_coarse_t* cq, const float* d_x, long long n,
                      long long ld_x, int32_t* d_list, float* d_dist);

/* Stable order of the rows by list: d_perm int64 [n] (stream row s holds caller row perm[s]),
 * d_offsets int64 [nlist + 1] (list l = stream rows [offsets[l], offsets[l+1])).  A list id
 * outside [0, nlist) writes nothing out of bounds and makes pqh_ivf_status answer PQH_ERR_ARG
 * (d_perm is then still a permutation of the rows, otherwise unspecified, as d_offsets).
 * n == 0: offsets all zero.
 * Scratch: 4 * n bytes and rocPRIM's sort storage (about 12 * n) in the context workspace,
 * freed by pqh_ctx_release_scratch. */
int pqh_ivf_layout(pqh_ctx_t* ctx, const int32_t* d_list, long long n, int nlist,
                   long long* d_perm, long long* d_offsets);

/* For each query the nprobe nearest lists by (dist, l) ascending, written as the CSR probe
 * list pqh_search_*_ranges take: d_range_ptr[q] = q * nprobe (int64 [nq + 1]);
 * d_ranges[q * nprobe + p] = (offsets[l], offsets[l+1] - offsets[l]) (int64 [nq * nprobe][2]).
 * Optional (may be NULL): d_probes int64 [nq][nprobe] and d_probe_dist float [nq][nprobe].
 * nprobe > nlist: the tail is list -1, +inf, range (0, 0).  1 <= nprobe <= PQH_IVF_MAX_NPROBE,
 * else PQH_ERR_ARG.  d_offsets (int64 [nlist + 1]) is device data and is not validated beyond
 * what safety needs: an entry pair that is reversed gives the range (0, 0) and PQH_ERR_ARG
 * from pqh_ivf_status; whether the ranges fit the stream is checked by the search that takes
 * them.  Query rows are ld_q >= d floats apart.  nq == 0 launches nothing.
 * One workgroup per query: the time grows with nlist * d per query. */
int pqh_coarse_probe(pqh_ctx_t* ctx, const pqh_coarse_t* cq, const float* d_queries, long long nq,
                     long long ld_q, int nprobe, const long long* d_offsets,
                     long long* d_range_ptr, long long* d_ranges, long long* d_probes,
                     float* d_probe_dist);

/* The residual form of an inverted file: the stream holds the PQ codes of x - c[list], and a
 * (query, probed list) pair is scored with the table of query - c[list].  The PQ codebook must
 * then be trained on residuals (the output of pqh_ivf_residuals), not on x.
 *
 * d_out[s][j] = x[p][j] - c[d_list[p]][j] with p = d_perm ? d_perm[s] : s: the rows in list
 * order and their residuals in one pass (one fp32 subtract per element).  d_list int32 [n] is
 * indexed by caller row (pqh_coarse_assign's output), d_perm int64 [n] is pqh_ivf_layout's, or
 * NULL for the identity.  Rows of x are ld_x >= d floats apart and rows of d_out ld_out >= d;
 * the floats between rows of x are never read, those between rows of d_out never written.
 * d_out must not overlap x.  A d_perm entry outside [0, n) or a list id outside [0, nlist)
 * gives a row of zeros and PQH_ERR_ARG from pqh_ivf_status.  n == 0 launches nothing. */
int pqh_ivf_residuals(pqh_ctx_t* ctx, const pqh_coarse_t* cq, const float* d_x, long long n,
                      long long ld_x, const int32_t* d_list /* [n], by caller row */,
                      const long long* d_perm /* [n] or NULL */, float* d_out, long long ld_out);

/* One ADC table per (query, probed list): with l = d_probes[q][p] and r = query[q] - c[l] (one
 * fp32 subtract per element), d_lut[q * nprobe + p][i][c] = sum_j (r[i*dsub+j] - cent[i][c][j])^2
 * in pqh_adc_tables' arithmetic -- bit-equal to pqh_adc_tables run on r.  d_probes int64
 * [nq][nprobe] is pqh_coarse_probe's; d_lut float [nq * nprobe][m][K] is what
 * pqh_search_*_range_tables take beside pqh_coarse_probe's ranges.  l == -1 (the padding of
 * pqh_coarse_probe) gives a table of +inf; any other l outside [0, nlist) the same and
 * PQH_ERR_ARG from pqh_ivf_status.  PQH_ERR_ARG at once: pq's m * dsub != cq's d, nprobe < 1,
 * ld_q < d, a null pointer when nq > 0.  PQH_ERR_UNSUPPORTED: K > 256,
 * d > PQH_ADC_RESIDUAL_MAX_D (the residual is staged in LDS), nq * nprobe >= 2^31.
 * nq == 0 launches nothing. */
#define PQH_ADC_RESIDUAL_MAX_D 16384
int pqh_adc_tables_residual(pqh_ctx_t* ctx, const pqh_pq_t* pq, const pqh_coarse_t* cq,
                            const float* d_queries, long long nq, long long ld_q,
                            const long long* d_probes /* [nq][nprobe] */, int nprobe,
                            float* d_lut /* [nq * nprobe][m][K] */);

/* The row mask of the *_masked searches from a byte per row: bit i of d_bits (bit i & 31 of
 * word i >> 5) = d_keep[p] != 0 with p = d_perm ? d_perm[i] : i -- with pqh_ivf_layout's
 * d_perm, a predicate over the caller's rows becomes the mask over the stream's.  d_keep u8
 * [n], d_perm int64 [n] or NULL, d_bits [ceil(n / 32)] words (4-byte aligned, else
 * PQH_ERR_ARG), all of them written, the bits from n on in the last one as zeros.  A d_perm
 * entry outside [0, n) reads nothing, gives a zero bit and PQH_ERR_ARG from pqh_ivf_status.
 * n == 0 launches nothing. */
int pqh_mask_pack(pqh_ctx_t* ctx, const unsigned char* d_keep /* [n], nonzero = keep */,
                  const long long* d_perm /* [n] or NULL */, long long n, unsigned int* d_bits);

/* Synchronises; PQH_ERR_ARG if a pqh_ivf_layout / pqh_coarse_probe / pqh_ivf_residuals /
 * pqh_mask_pack / pqh_adc_tables_residual / pqh_ivf_regroup / pqh_idmap_* / pqh_mask_pack_idmap
 * (or the _ip form of one of them) on this context since the last call met a bad value (sticky until read, like
 * pqh_decode_status). */
int pqh_ivf_status(pqh_ctx_t* ctx);

/* ---- rotated index: a linear map in front of the quantizers (OPQ) ------------------------
 * A d x d matrix R applied to every row before the coarse quantizer and the PQ see it, and the
 * two sums the training of such a matrix needs (codec.opq_train).  Any matrix is accepted: the
 * library applies a linear map, that it is orthonormal is the caller's property
 * (codec.Rotation.defect).
 * Argument checks need no device and come first in these calls; a NULL context is answered next
 * (PQH_ERR_NO_DEVICE when no HIP device is visible, else PQH_ERR_ARG).
 * 1 <= d <= PQH_ROT_MAX_D, no multiple of anything required; beyond it PQH_ERR_UNSUPPORTED. */
typedef struct pqh_rotation pqh_rotation_t;
#define PQH_ROT_MAX_D 1024

/* R: HOST [d][d] fp32.  The device keeps R and its transpose (8 * d * d bytes), as
 * pqh_coarse_create keeps two copies; synchronous.  PQH_ERR_ARG: a null pointer, d < 1. */
int pqh_rotation_create(pqh_ctx_t* ctx, const float* R /* HOST [d][d] */, int d,
                        pqh_rotation_t** rot);
/* Synchronises the stream of the context it was made with, which must still exist. */
int pqh_rotation_destroy(pqh_rotation_t* rot);

/* d_out[v][j] = sum_t x[v][t] * R[t][j]; transpose = 1: R[j][t] in place of R[t][j].  Each
 * output is one fp32 chain from +0.0 with t ascending, one multiply and one add per element, no
 * contraction -- the arithmetic of pqh_coarse_assign, so float32 array operations of numpy give
 * the same bits.  Rows of x are ld_x >= d floats apart and rows of d_out ld_out >= d; the floats
 * between rows of x are never read, those between rows of d_out never written.  d_out must not
 * overlap x.  The bits do not depend on the grid.  n == 0 launches nothing.  Asynchronous on the
 * context's stream.  PQH_ERR_ARG: a null pointer (d_x and d_out may be NULL when n == 0), n < 0,
 * ld_x < d, ld_out < d, transpose not 0 or 1. */
int pqh_rotate(pqh_ctx_t* ctx, const pqh_rotation_t* rot, const float* d_x, long long n,
               long long ld_x, float* d_out, long long ld_out, int transpose);

/* moments[a][b] = sum_v x[v][a] * y[v][b], deterministic and exact in the way
 * pqh_kmeans_train's sums are: each product is one fp32 multiply p, f = rn(p * 2^s) is an int64
 * (__double2ll_rn(ldexp((double)p, s))), the f are added as integers -- so neither the order nor
 * the grid can matter -- and moments[a][b] = ldexp((double)sum, -s).
 * s = 61 - ceil(log2(max|x| * max|y| * n)) with the product in double, clamped to [-126, 100],
 * 40 when the product is 0: pqh_kmeans_train's exponent with max|x| * max|y| for max|x|.
 * x [n][dx] and y [n][dy] are device rows ld_x >= dx and ld_y >= dy floats apart (x and y may be
 * the same buffer); moments is HOST [dx][dy].  1 <= dx, dy <= PQH_ROT_MAX_D, else
 * PQH_ERR_UNSUPPORTED.  n == 0 gives zeros.  Synchronous, as pqh_kmeans_train is.
 * PQH_ERR_ARG: a null pointer (d_x and d_y may be NULL when n == 0), n < 0, dx or dy < 1,
 * ld_x < dx, ld_y < dy. */
int pqh_cross_moments(pqh_ctx_t* ctx, const float* d_x, long long n, long long ld_x, int dx,
                      const float* d_y, long long ld_y, int dy,
                      double* moments /* HOST [dx][dy] */);

/* ---- inner-product search: the metric around the scan -----------------------------------
 * The scans order plain fp32 sums with `<`, so a maximum-inner-product search scores a pair with
 * the NEGATED inner product: smaller is nearer, results are ordered by (score, id) ascending
 * and padded with (+inf, -1) as everywhere else, pqh_range_*'s strict `dist < radius` reads
 * `ip > -radius`, and a caller's score is -dist.  The arithmetic, for a query slice x and a
 * vector y of length L:
 *   nip(x, y):  acc = +0.0f;  for j = 0 ... L - 1 ascending:  acc = acc - x[j] * y[j]
 * one fp32 multiply and one fp32 subtract per element, no contraction, no final negation, no
 * reordering (so the sign of a zero is defined too).
 * Each call takes the arguments of its L2 twin and has the twin's conventions, limits, argument
 * errors and device errors (pqh_ivf_status, pqh_decode_status); nq == 0 or n == 0 launches
 * nothing.  The scan calls (pqh_search_*, pqh_range_*) take these tables unchanged. */
/* lut[q][i][c] = nip(query[q][i*dsub ...], cent[i][c]) -- see pqh_adc_tables. */
int pqh_adc_tables_ip(pqh_ctx_t* ctx, const pqh_pq_t* pq, const float* d_queries, long long nq,
                      long long ld_q, float* d_lut);
/* d_list[v] = the first l that minimises nip(x[v], c[l]), one chain over all d dimensions (ties
 * go to the smaller l); d_dist (optional) that value -- see pqh_coarse_assign. */
int pqh_coarse_assign_ip(pqh_ctx_t* ctx, const pqh_coarse_t* cq, const float* d_x, long long n,
                         long long ld_x, int32_t* d_list, float* d_dist);
/* The nprobe lists by (nip(q, c[l]), l) ascending; the four outputs and the padding of
 * pqh_coarse_probe, d_probe_dist holding the nip values (bit-equal to pqh_coarse_assign_ip's
 * d_dist for nprobe == 1). */
int pqh_coarse_probe_ip(pqh_ctx_t* ctx, const pqh_coarse_t* cq, const float* d_queries,
                        long long nq, long long ld_q, int nprobe, const long long* d_offsets,
                        long long* d_range_ptr, long long* d_ranges, long long* d_probes,
                        float* d_probe_dist);
/* One table per (query, probed list) of a residual index (the stream holds the codes of
 * x - c[list]) for pqh_search_*_range_tables and pqh_search_*_lists: <q, c[l] + r> is
 * <q, c[l]> + <q, r>, so with l = d_probes[q][p], bias = nip(query[q], c[l]) over all d
 * dimensions and plain = pqh_adc_tables_ip's table of query q,
 *   d_lut[q * nprobe + p][i][c] = plain[q][i][c]                 for i >= 1
 *   d_lut[q * nprobe + p][0][c] = bias + plain[q][0][c]          (one fp32 add)
 * bias is pqh_coarse_probe_ip's d_probe_dist for that pair on every bit.  l == -1 gives a table
 * of +inf; any other l outside [0, nlist) the same and PQH_ERR_ARG from pqh_ivf_status.
 * Argument errors and limits are pqh_adc_tables_residual's. */
int pqh_adc_tables_residual_ip(pqh_ctx_t* ctx, const pqh_pq_t* pq, const pqh_coarse_t* cq,
                               const float* d_queries, long long nq, long long ld_q,
                               const long long* d_probes /* [nq][nprobe] */, int nprobe,
                               float* d_lut /* [nq * nprobe][m][K] */);

/* ---- a mutable inverted file: a list-ordered stream taken to a new list order ------------
 * The streams hold everything an index is rebuilt from.  pqh_ivf_regroup plans the new order
 * (rows dropped, gaps left for new rows), pqh_decode_scatter decodes the old stream straight
 * into it; the new rows' codes are stored into the gaps and the whole is encoded again.
 * Conventions of the inverted-file calls: device pointers, asynchronous on the context's
 * stream, a NULL context answered first (PQH_ERR_NO_DEVICE or PQH_ERR_ARG). */
/* With kept(l) = the rows r of [d_offsets[l], d_offsets[l + 1]) whose bit of d_keep is set
 * (pqh_mask_pack's format; NULL: all of them) and add(l) = d_add_offsets[l + 1] -
 * d_add_offsets[l] (NULL: 0):
 *   d_new_offsets[0] = 0, d_new_offsets[l + 1] = d_new_offsets[l] + kept(l) + add(l)
 *   d_dest[r] = d_new_offsets[l] + (kept rows of list l before r), or -1 for a dropped row
 *   d_add_base[l] = d_new_offsets[l] + kept(l)                       (NULL: not wanted)
 * so within a list the kept old rows keep their order and come first, the gap for the added
 * rows behind them.  d_offsets int64 [nlist + 1] must cover the stream (d_offsets[0] == 0,
 * d_offsets[nlist] == n, never decreasing), d_add_offsets -- pqh_ivf_layout's offsets of the
 * new batch -- must start at 0 and never decrease; otherwise pqh_ivf_status answers PQH_ERR_ARG
 * and the outputs hold unspecified values, written in bounds.  Limits are pqh_ivf_layout's
 * (n < 2^31, nlist <= PQH_IVF_MAX_NLIST, else PQH_ERR_UNSUPPORTED).  n == 0 is valid: with
 * d_add_offsets it plans a pure insertion (d_keep and d_dest are then not looked at).  Uses the
 * context's scratch when d_keep is given. */
int pqh_ivf_regroup(pqh_ctx_t* ctx, const long long* d_offsets /* [nlist + 1] */, long long nlist,
                    long long n, const unsigned int* d_keep /* [ceil(n / 32)] or NULL = all */,
                    const long long* d_add_offsets /* [nlist + 1] or NULL = none */,
                    long long* d_new_offsets /* [nlist + 1] */, long long* d_dest /* [n] */,
                    long long* d_add_base /* [nlist] or NULL */);
/* pqh_decode through a row map: row r of the stream is stored at d_out[d_dest[r]] where
 * d_dest[r] >= 0; rows of d_out that are no row's destination are not written.  Stream, index,
 * code type and shapes are pqh_decode_select's (tree-mode streams out of scope); a chunk of more
 * than 96 KB of codes is PQH_ERR_UNSUPPORTED.  What is not wanted is not decoded: a chunk is
 * walked up to its last row with a destination, one without such a row is neither read nor
 * walked.  Errors are reported by pqh_decode_status: a destination below -1 or >= n_out writes
 * nothing and gives PQH_ERR_ARG; an invalid code, a chunk offset or a symbol past the stream
 * gives PQH_ERR_CORRUPT, which takes precedence, and leaves the rows of that chunk unwritten.
 * Of two rows with the same destination one wins, unspecified which.  n == 0 launches
 * nothing. */
int pqh_decode_scatter(pqh_ctx_t* ctx, const pqh_tables_t* t, const unsigned char* d_stream,
                       unsigned long long stream_bytes, long long n, int raw_first, int chunk_vectors,
                       const unsigned long long* d_chunk_offsets, const void* d_chunk_prev,
                       const long long* d_dest /* [n] */, void* d_out /* [n_out][m] codes */,
                       long long n_out);

/* ---- compressed ids: an Elias-Fano id map for the inverted file --------------------------
 * pqh_ivf_layout's d_perm is a stable order by list, pqh_ivf_regroup keeps a list's old rows in
 * their order in front of the new ones, and new rows get ids above every old one: within a list
 * the ids ascend strictly, so with B = the bit width of n_ids - 1
 *   key(s) = (list(s) << B) | d_perm[s]
 * ascends strictly over the stream.  The map stores the n keys below nlist << B in Elias-Fano
 * form -- about 2 + log2(nlist) bits a row, with random access -- as one device blob of 64-bit
 * words (8-byte aligned, else PQH_ERR_ARG), L = max(0, floor(log2((nlist << B) / n))):
 *   header   16 words: a magic word, n, n_ids, nlist, B, L, the word offset of the low bits,
 *            that of the high bits and their words, that of the samples and their count, that
 *            of the reverse part and the bytes of one of its entries (0: no reverse part), the
 *            words of the blob, two words of zeros
 *   low      n fields of L bits (L <= 55), field s at bit s * L counted from bit 0 of word 0 of
 *            the part: a field may straddle two words; L == 0: no words
 *   high     bit (key(s) >> L) + s is set for every row s, ((nlist << B) - 1 >> L) + n bits
 *            (fewer than 3 n + 1)
 *   samples  one word per 256 rows: (key(256 j) >> L) + 256 j, the high-bit position of row 256 j
 *   reverse  (optional) the list of every id of [0, n_ids): u16 where nlist <= 65535, 0xFFFF =
 *            the id has no row; int32 otherwise, -1 = no row; padded to a word
 * Every part is padded to whole words and every bit that no field owns is zero, so two maps of
 * the same (d_perm, d_offsets, n_ids, nlist) are equal byte for byte.  n == 0 is a valid map: the
 * header (and the reverse part, all "no row").
 * Conventions of the inverted-file calls: device pointers, asynchronous on the context's stream,
 * a NULL context answered first, bad device data reported by pqh_ivf_status (sticky PQH_ERR_ARG)
 * with nothing read or written out of bounds; count == 0 launches nothing.  d_map of every call
 * but pqh_idmap_build is a blob that call wrote. */
/* The bytes of the blob: host arithmetic only, no GPU.  0 <= n <= n_ids and nlist >= 1, else
 * PQH_ERR_ARG; n_ids < 2^31 and nlist <= PQH_IVF_MAX_NLIST, else PQH_ERR_UNSUPPORTED.  Without
 * the reverse part the blob is at most n * (L + 3) / 8 + n / 32 + 4096 bytes. */
int pqh_idmap_bytes(long long n, long long n_ids, long long nlist, int reverse,
                    unsigned long long* bytes);
/* Writes the blob of d_perm int64 [n] and d_offsets int64 [nlist + 1] as pqh_ivf_layout gives
 * them (after pqh_ivf_regroup: the new order's).  map_bytes below pqh_idmap_bytes is
 * PQH_ERR_CAPACITY.  Checks what it codes: a d_perm entry outside [0, n_ids), a row outside the
 * list d_offsets puts it in, or two neighbouring rows whose keys do not ascend (two equal ids,
 * a descending pair in a list) make pqh_ivf_status answer PQH_ERR_ARG; the map is then
 * unspecified, but every later call on it stays in bounds.  Two memsets and one launch (n == 0:
 * the launch writes the header). */
int pqh_idmap_build(pqh_ctx_t* ctx, const long long* d_perm /* [n] */,
                    const long long* d_offsets /* [nlist + 1] */, long long n, long long nlist,
                    long long n_ids, int reverse, void* d_map, unsigned long long map_bytes);
/* d_ids[i] = the id of stream row d_rows[i], one lane per row, rows in any order and repeated
 * at will.  A row < 0 is copied through (the -1 padding of a search result); a row >= n gives
 * -1 and PQH_ERR_ARG from pqh_ivf_status. */
int pqh_idmap_ids(pqh_ctx_t* ctx, const void* d_map, const long long* d_rows /* [count] */,
                  long long count, long long* d_ids /* [count] */);
/* The ids of the rows [first, first + count), any first and count: the streaming form, a wave per
 * block of 256 rows.  A row >= n gives -1 and PQH_ERR_ARG from pqh_ivf_status; first < 0 or
 * count < 0 is PQH_ERR_ARG at once. */
int pqh_idmap_decode(pqh_ctx_t* ctx, const void* d_map, long long first, long long count,
                     long long* d_ids /* [count] */);
/* d_rows[i] = the stream row of id d_ids[i], or -1 where the id has none (a row dropped from
 * the index): the id's list from the reverse part, then a binary search over the rows
 * d_offsets[l] ... d_offsets[l + 1] of that list (cut to [0, n] whatever they hold).  An id
 * outside [0, n_ids) gives -1 and PQH_ERR_ARG from pqh_ivf_status; so does every id on a map
 * built without a reverse part (the header lives on the device and the call does not wait for
 * it: codec.IdMap.rows refuses such a map at once). */
int pqh_idmap_rows(pqh_ctx_t* ctx, const void* d_map, const long long* d_offsets /* [nlist + 1] */,
                   const long long* d_ids /* [count] */, long long count,
                   long long* d_rows /* [count] */);
/* pqh_mask_pack through the map: bit s & 31 of d_bits[s >> 5] = d_keep[id(s)] != 0 for the n
 * rows of the map, the words pqh_mask_pack(d_keep, d_perm) writes in every bit below n, the bits
 * from n on in the last word zeros; d_perm is never materialised.  d_keep u8 [n_ids], d_bits
 * [ceil(n / 32)] words (4-byte aligned).  n is the map's (the grid is sized by it): another n
 * writes zeros and gives PQH_ERR_ARG from pqh_ivf_status.  n == 0 launches nothing. */
int pqh_mask_pack_idmap(pqh_ctx_t* ctx, const unsigned char* d_keep /* [n_ids] */,
                        const void* d_map, long long n, unsigned int* d_bits);

/* ---- refinement codes: a second compressed stream and a fused re-rank -------------------
 * A row is stored twice: as the PQ code a of the vector (level 1, the stream the searches
 * scan) and as the PQ code b of what level 1 left over, x - reconstruction (level 2, a stream
 * of its own with its own tables and chunk index).  A search's candidates are re-ranked by
 *   y = concat_i cent1[i][a_i] + concat_i cent2[i][b_i]      (one add per dimension)
 *   t = q - y         (residual index: t = (q - c[l]) - y, l the list of the row)
 *   dist = sum_j t[j] * t[j]
 * in fp32, j ascending over all d = m1 * dsub1 = m2 * dsub2 dimensions as ONE chain (m1 and m2
 * may differ), no contraction: the arithmetic of pqh_coarse_assign.  The list of stream row r
 * is the last l with d_offsets[l] <= r, so empty lists are passed over.
 * For each query q < nq: of the candidates d_rows[q][0 .. ncand) (int64 stream rows; -1 is
 * padding and never an error; a row may be given twice and then appears twice) the top_k
 * smallest by (dist, row) ascending, padded with (+inf, -1), into d_dist[q][0 .. top_k) and
 * d_ids[q][0 .. top_k); the rows of both outputs are ld_out >= top_k elements apart and what
 * lies between them is left alone.  1 <= ncand <= the context's limit (PQH_SEARCH_MAX_K, or what
 * pqh_ctx_set_search_max_k set, 256 at the most), 1 <= top_k <= ncand.
 * Query rows are ld_q >= d floats apart.  (cq, d_offsets): the coarse quantizer and the
 * int64 [nlist + 1] list offsets of a residual index, both NULL for a plain one.
 * Conventions of the search calls: device pointers, asynchronous on the context's stream; a
 * NULL context returns PQH_ERR_NO_DEVICE when no HIP device is visible and PQH_ERR_ARG
 * otherwise, checked before anything else.  PQH_ERR_ARG: a null pointer, the two levels (or
 * cq) disagreeing in d, tables and codebook of a level disagreeing in m or K, ncand or top_k
 * out of range, only one of cq and d_offsets given.  PQH_ERR_UNSUPPORTED: m > 16 or K > 256 at
 * either level, d > PQH_ADC_RESIDUAL_MAX_D (the query row is staged in LDS), nq >= 2^31.  Any
 * dsub, d need not be a multiple of four.  nq == 0 launches nothing.
 * Errors on the device are pqh_decode_select's, reported by pqh_decode_status: a row outside
 * [0, n) other than -1 (or, with d_offsets, at or past d_offsets[nlist]) is dropped and gives
 * PQH_ERR_ARG; a chunk offset or a symbol past stream_bytes * 8 bits or an invalid code at
 * either level drops that candidate and gives PQH_ERR_CORRUPT, which takes precedence.  Only
 * the chunks of the candidates are read, and nothing outside stream_bytes at either level.
 * Results for NaN inputs are unspecified.  Tree-mode streams are out of scope. */
/* Both levels read from their streams: per level the tables, the codebook and the stream and
 * index arguments of pqh_fetch_vectors (chunk sizes and context modes are independent). */
int pqh_refine_stream(pqh_ctx_t* ctx, const pqh_tables_t* t1, const pqh_pq_t* pq1,
                      const unsigned char* d_stream1, unsigned long long stream_bytes1,
                      int raw_first1, int chunk_vectors1,
                      const unsigned long long* d_chunk_offsets1, const void* d_chunk_prev1,
                      const pqh_tables_t* t2, const pqh_pq_t* pq2, const unsigned char* d_stream2,
                      unsigned long long stream_bytes2, int raw_first2, int chunk_vectors2,
                      const unsigned long long* d_chunk_offsets2, const void* d_chunk_prev2,
                      long long n, const pqh_coarse_t* cq, const long long* d_offsets,
                      const float* d_queries, long long nq, long long ld_q,
                      const long long* d_rows /* [nq][ncand] */, int ncand, int top_k,
                      float* d_dist, long long* d_ids, long long ld_out);
/* The same over plain row-major u8 codes [n][m1] and [n][m2]: the yardstick of the stream form,
 * as pqh_search_codes is of the scan.  A code >= K drops the candidate (PQH_ERR_CORRUPT). */
int pqh_refine_codes(pqh_ctx_t* ctx, const pqh_pq_t* pq1, const void* d_codes1,
                     const pqh_pq_t* pq2, const void* d_codes2, long long n,
                     const pqh_coarse_t* cq, const long long* d_offsets, const float* d_queries,
                     long long nq, long long ld_q, const long long* d_rows /* [nq][ncand] */,
                     int ncand, int top_k, float* d_dist, long long* d_ids, long long ld_out);

/* The re-rank by inner product: y = cent1[..][j] + cent2[..][j] (one add; residual index:
 * y[j] = c[l][j] + y[j], one more add, l the row's list as above) and dist = nip(query, y), one
 * chain over d (the definition of nip is with pqh_adc_tables_ip).  Candidate checks, padding,
 * ld_out, both candidate widths, limits and error precedence are pqh_refine_stream's and
 * pqh_refine_codes'. */
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
                         const long long* d_rows /* [nq][ncand] */, int ncand, int top_k,
                         float* d_dist, long long* d_ids, long long ld_out);
int pqh_refine_codes_ip(pqh_ctx_t* ctx, const pqh_pq_t* pq1, const void* d_codes1,
                        const pqh_pq_t* pq2, const void* d_codes2, long long n,
                        const pqh_coarse_t* cq, const long long* d_offsets, const float* d_queries,
                        long long nq, long long ld_q, const long long* d_rows /* [nq][ncand] */,
                        int ncand, int top_k, float* d_dist, long long* d_ids, long long ld_out);

/* Build the chunk index of an existing stream (one produced without a sidecar, e.g. by
 * the reference encoder) with a sequential table walk on the HOST copy of the stream
 * (index building only; the symbols themselves are decoded on the GPU). */
int pqh_chunk_index_host(const pqh_tables_t* t, const unsigned char* stream,
                         unsigned long long stream_bytes, long long n, int raw_first,
                         int chunk_vectors, unsigned long long* chunk_offsets,
                         void* chunk_prev);

/* ---- sort mode (huffman_encoder.c:301-317: qsort + strncmp) ---------------------- */
/* Stable sort of the n rows by key(row) = row with every byte after its first 0 zeroed
 * (strncmp order), uint8 codes only.
 * Workspace (grown in the context, kept between calls): the in-tree radix sort (2 <= m
 * <= 8, n < 2^31) takes 32 bytes per row + 8 KB plus a persistent 2 KB-per-8192-row
 * tile-state array, and sorts in place (d_tmp unused, may be NULL).  Other shapes, or
 * PQH_SORT_IMPL=rocprim, use rocPRIM's radix_sort_pairs: 24 bytes per row + its temp
 * storage, plus n*m bytes for the gathered rows unless d_tmp (n*m bytes) is given.
 * If the in-tree sort cannot allocate its workspace it retries on the rocPRIM path
 * before returning PQH_ERR_NOMEM. */
int pqh_sort_rows(pqh_ctx_t* ctx, void* d_codes, long long n, int m, void* d_tmp);

/* ---- multi-GPU row shards ------------------------------------------
 * One process per GPU; rank r owns a contiguous row range, described by a block_t
 * (src/fast_nn_block.h:4-25: id = first global row, size = rows; data / indices unused on
 * the device path).  The only exchanges are small: the one-row halo (context mode), the
 * histogram all-reduce that feeds the shared code tables (huffman_encoder.c:139-205 over
 * the whole input), and an all-gather of the shards' bit lengths whose exclusive scan places
 * every shard in the global stream (the bit cursor of bitstream.c:71-101).  The transport is
 * the caller's communicator, passed as hooks (RCCL, MPI, torch.distributed, gloo ...). */

/* rank `rank`'s rows of n_total over `world` ranks: sizes differ by at most one row.
 * Fills block->id / size (capacity = size, num_dimensions 0, data / indices NULL). */
int pqh_shard_block(long long n_total, int world, int rank, block_t* block);

/* Collective hooks over DEVICE buffers, ordered on `stream` (the context's): return 0 on
 * success.  all_reduce_sum_u32: in-place sum over ranks; all_gather: d_recv[world][bytes]
 * = every rank's d_send[bytes], in rank order. */
typedef struct {
    void* user;
    int world, rank;
    int (*all_reduce_sum_u32)(void* user, uint32_t* d_buf, long long count, void* stream);
    int (*all_gather)(void* user, const void* d_send, void* d_recv, long long bytes,
                      void* stream);
} pqh_shard_comm_t;

/* Scratch bytes pqh_shard_encode needs in d_scratch (device, 16-byte aligned). */
long long pqh_shard_scratch_bytes(int world, int m);

/* One rank's encode of its shard (uint8 codes, K <= 256 -- context mode needs K = 256):
 *   context mode: all-gather of every rank's (non-empty flag, last row) -> on the device,
 *     the halo of this shard = the last row of the nearest non-empty rank before it, and the
 *     raw first row (huffman_encoder.c:234) belongs to the first non-empty rank (a shard may
 *     be empty, e.g. a slice of the distributed sort);
 *   histogram of the shard (+ the halo pair) -> all_reduce_sum_u32 -> GPU code tables
 *   (identical on every rank: no broadcast) -> the shard's exact bit length -> all_gather
 *   of the lengths -> exclusive scan on the device -> pqh_encode_write_at.
 * Asynchronous: no host round trip (unless raw_first is non-NULL, which reads back at the
 * end whether this shard wrote the raw first row).
 * Outputs: d_counts [m][items] the GLOBAL histogram; tables built from it; d_out holds the
 * shard's bits at (global offset % 32) with word 0 = the global stream's word offset / 32
 * (buffers compose by OR-ing boundary words: pqh_shard_stitch); d_offsets[2] (device u64) =
 * {this shard's global bit offset, the global stream's length in bits}; the chunk index
 * (optional, chunk_vectors > 0) is relative to d_out bit 0.
 * Errors: PQH_ERR_ARG at once (before any collective) when ctx, comm, m, k, context,
 * d_counts, d_offsets or d_scratch are unusable -- the arguments the collectives need.  Any
 * other failure of this rank (its shard, tables or output arguments, or a library call)
 * keeps the rank in the collective sequence with an empty contribution and the sentinel
 * length ~0, and is returned here; every rank's d_offsets then reads {0, ~0}, which
 * pqh_shard_status reports as PQH_ERR_REMOTE -- no rank is left waiting in a collective. */
int pqh_shard_encode(pqh_ctx_t* ctx, const pqh_shard_comm_t* comm, const block_t* shard,
                     const void* d_codes, int m, int k, int context, pqh_tables_t* tables,
                     uint32_t* d_counts, unsigned char* d_out, unsigned long long out_bytes,
                     int chunk_vectors, unsigned long long* d_chunk_offsets, void* d_chunk_prev,
                     unsigned long long* d_offsets, void* d_scratch, int* raw_first);
/* pqh_shard_encode in two phases, for a caller that pipelines batches (bench.py): phase 1
 * (halo, histogram, all-reduce, code tables) and phase 2 (length, all-gather, offsets,
 * write) may run on different streams -- ordered by the caller -- with other batches'
 * collectives between them.  Both take the same d_scratch; phase 2's `status` is phase 1's
 * return value (a nonzero status sends the sentinel length).  pqh_shard_encode = phase 1 +
 * phase 2.  A collective hook failure returns PQH_ERR_COMM. */
int pqh_shard_encode_tables(pqh_ctx_t* ctx, const pqh_shard_comm_t* comm, const block_t* shard,
                            const void* d_codes, int m, int k, int context,
                            pqh_tables_t* tables, uint32_t* d_counts, void* d_scratch);
int pqh_shard_encode_write(pqh_ctx_t* ctx, const pqh_shard_comm_t* comm, const block_t* shard,
                           const void* d_codes, int m, int k, int context, pqh_tables_t* tables,
                           unsigned char* d_out, unsigned long long out_bytes, int chunk_vectors,
                           unsigned long long* d_chunk_offsets, void* d_chunk_prev,
                           unsigned long long* d_offsets, void* d_scratch, int status,
                           int* raw_first);
/* The two phases for PART-MAJOR codes (pqh_pq_assign_parts: part i's codes at
 * d_codes[i * ld_codes + v], ld_codes >= the shard's rows), so a multi-rank pipeline runs the
 * single-rank one (bench.py): phase 2 takes m = 8 or 16 (the row encoder reading part runs).
 * d_partials (phase 1, optional, context mode): the shard's partial pair counts taken by
 * pqh_histogram_partial_parts(d_codes, ld_codes, n, m, k, NULL, d_partials) -- e.g. on the
 * assignment stream, ordered before this call by the caller; phase 1 then reduces them and
 * adds the shard-boundary pair itself instead of running the histogram.  NULL: phase 1 runs
 * the part-major histogram (with the halo pair).  Same errors and outputs as above. */
int pqh_shard_encode_tables_parts(pqh_ctx_t* ctx, const pqh_shard_comm_t* comm,
                                  const block_t* shard, const void* d_codes, long long ld_codes,
                                  int m, int k, int context, pqh_tables_t* tables,
                                  uint32_t* d_counts, void* d_scratch, const void* d_partials);
int pqh_shard_encode_write_parts(pqh_ctx_t* ctx, const pqh_shard_comm_t* comm,
                                 const block_t* shard, const void* d_codes, long long ld_codes,
                                 int m, int k, int context, pqh_tables_t* tables,
                                 unsigned char* d_out, unsigned long long out_bytes,
                                 int chunk_vectors, unsigned long long* d_chunk_offsets,
                                 void* d_chunk_prev, unsigned long long* d_offsets, void* d_scratch,
                                 int status, int* raw_first);
/* Synchronises; PQH_ERR_REMOTE if some rank's pqh_shard_encode behind d_offsets failed. */
int pqh_shard_status(pqh_ctx_t* ctx, const unsigned long long* d_offsets);

/* ---- sharded search: several top-k results into one ---------------------------------
 * pqh_topk_merge: for every query the top_k smallest of all entries of all parts with
 * id >= 0, each id moved by its part's base, ascending by (dist, moved id), padded with
 * (+inf, -1) -- the order and the padding of every search here.  d_dist / d_ids are
 * [parts][nq][k_in], what an all-gather of each rank's (nq, k) result leaves; d_id_base is DEVICE
 * int64 [parts], or NULL for zeros.  No order is assumed inside a part and padding may sit
 * anywhere; an entry with id < 0 is ignored whatever its distance; moved ids may exceed 2^32.
 * What NaN or +inf distances with id >= 0 give is unspecified, but nothing is read or written
 * out of bounds.  Async on the context's stream.  parts >= 1 and k_in >= 1 (no upper limit),
 * 1 <= top_k <= the context's limit (PQH_SEARCH_MAX_K, or what pqh_ctx_set_search_max_k set),
 * else PQH_ERR_ARG; nq == 0 launches nothing; nq >= 2^31 is PQH_ERR_UNSUPPORTED.  A NULL
 * context answers as in the search calls.
 * The result over the searches of row blocks of one data set: without a re-rank, dist equals
 * the dist of one index over all rows bit for bit (the same rows get the same codes and tables
 * and the same lists are probed; the k smallest of a union are the k smallest of its parts' k
 * smallest), and ids are equal wherever a query's distances are distinct.  Among equal
 * distances this result is ordered by global id, the single index by (list, id), and at a tie
 * across position k each part first chose by its own stream order. */
int pqh_topk_merge(pqh_ctx_t* ctx,
                   const float* d_dist, const long long* d_ids /* [parts][nq][k_in] */,
                   int parts, long long nq, int k_in,
                   const long long* d_id_base /* DEVICE int64 [parts], or NULL = zeros */,
                   int top_k, float* d_out_dist, long long* d_out_ids /* [nq][top_k] */);

/* Scratch bytes of pqh_shard_search_merge (device, 8-byte aligned): this rank's record, the
 * world gathered ones and a word.  0 for arguments the call refuses at once. */
unsigned long long pqh_shard_search_scratch_bytes(int world, long long nq, int k);
/* The collective of a search over a row-sharded index: every rank passes the (nq, k) result of
 * its own rows (local ids), the id of its first row (id_base) and the status of its local
 * search; every rank gets the same merged result, pqh_topk_merge of all ranks' results with
 * their bases.  ONE comm->all_gather of a record per rank,
 *     int64 id_base | int64 status | float dist[nq * k] (+ one zero float when nq * k is odd)
 *     | int64 ids[nq * k]
 * so that every field is 8-byte aligned in the gathered buffer; the merge reads the records
 * where the gather left them and the bases from the headers: no host round trip.  Async.
 * nq and k must be equal on every rank, as with any collective.
 * Errors: a NULL context answers as in the search calls; PQH_ERR_ARG at once (before the
 * gather) when comm, nq < 0 or k outside [1, PQH_SEARCH_MAX_K_WIDE] are unusable and
 * PQH_ERR_UNSUPPORTED for nq >= 2^31 -- arguments every rank shares.  Any other failure of this
 * rank keeps it in the gather with a non-zero status in its header and is returned here: a
 * non-zero `status`, k above this context's limit, a null or misaligned pointer (PQH_ERR_ARG),
 * scratch_bytes below pqh_shard_search_scratch_bytes (PQH_ERR_CAPACITY; the gather then lands
 * in the context's own scratch).  If any header carries a non-zero status every rank's outputs
 * are padding and d_state[0] is set, which pqh_shard_search_status reports as PQH_ERR_REMOTE
 * -- no rank waits in a collective.  A hook that fails returns PQH_ERR_COMM. */
int pqh_shard_search_merge(pqh_ctx_t* ctx, const pqh_shard_comm_t* comm,
                           const float* d_dist, const long long* d_ids /* this rank's [nq][k] */,
                           long long nq, int k, long long id_base, int status,
                           void* d_scratch, unsigned long long scratch_bytes,
                           float* d_out_dist, long long* d_out_ids /* [nq][k], the same on every rank */,
                           long long* d_state /* DEVICE int64[1] */);
/* Synchronises; PQH_ERR_REMOTE if some rank's part of the pqh_shard_search_merge behind d_state
 * failed. */
int pqh_shard_search_status(pqh_ctx_t* ctx, const long long* d_state);

/* Host: (this rank's global bit offset, the global length) from every rank's bit length. */
int pqh_shard_offsets(const unsigned long long* lengths, int world, int rank,
                      unsigned long long* offset, unsigned long long* total);
/* Host: the global stream (huffman_indices.bin after its 8-byte header) from the ranks'
 * shard buffers: buffer r holds its bits at offsets[r] % 32, its byte 0 being global byte
 * (offsets[r] / 32) * 4; bits outside each range are zero.  out (zeroed here) needs
 * ceil(sum(bits) / 8) bytes. */
int pqh_shard_stitch(int world, const unsigned char* const* bufs,
                     const unsigned long long* offsets, const unsigned long long* bits,
                     unsigned char* out, unsigned long long out_bytes);
/* Host: for shards that may be empty (sorted slices): the rank whose last row is this
 * shard's halo (-1: none) and whether this shard writes the raw first row. */
int pqh_shard_halo_source(const int* nonempty, int world, int rank, int* prev_rank,
                          int* raw_first);

/* ---- forest builder of tree mode (compute_nn_fast.c + mst_builder.c) ---- */
/* compute_nn_fast's block geometry (blocks_info_init / dimension_info_build,
 * fast_nn_blocks_info.c:52-112) over n device rows of d floats (row stride ld_x): split i
 * is coordinate num_split-1-i; h_starts / h_ends [num_split][blocks_per_dim] receive the
 * block ranges the reference stores in dimension_infos[i].block_starts / block_ends.
 * blocks_per_dim <= 32, num_split <= 8. */
int pqh_knn_blocks_info(pqh_ctx_t* ctx, const float* d_x, long long n, long long ld_x, int d,
                        int num_split, int blocks_per_dim, double overlap, float* h_starts,
                        float* h_ends);
/* compute_nn_fast with one block per pass (run, compute_nn_fast.c:510-620; the CLI's
 * --num-dimensions-at-pass 0): every block's exact kNN among its rows, merged per row in
 * block order into a num_nn max-heap (fast_nn_heap_push) and sorted -- d_indices / d_dists
 * [n][num_nn] as nn_indices.ivecsl / nn_dist.fvecsl hold them (never-filled slots:
 * 0xFFFFFFFF / +inf).  The in-block neighbours are the smallest direct-form fp32 squared
 * distances (get_real_dist, :304-311), lower block position first on ties (the reference
 * calls yael's knn_full_thread here: parity unpinned at that call).  d <= 128,
 * num_nn <= 63.  h_block_sizes (may be NULL): [blocks_per_dim^num_split] rows per block. */
int pqh_knn_fast(pqh_ctx_t* ctx, const float* d_x, long long n, long long ld_x, int d,
                 int num_nn, int num_split, int blocks_per_dim, const float* h_starts,
                 const float* h_ends, uint32_t* d_indices, float* d_dists,
                 long long* h_block_sizes);
/* mst_builder's forest (load_mst_edges_from_nn_files + minimum_spanning_tree,
 * mst.c:80-236): the first `take` neighbours of each of the n rows of the kNN lists
 * (num_nn per row, device), re-scored first when penalty > 0 (Hamming distance of the
 * device PQ codes d_pq [n][pq_m] times penalty, or the Hamming distance alone when
 * infinite), Kruskal in distance order.  Outputs tree_save_file's arrays (mst.c:253-265):
 * h_targets [*num_edges <= 2 (n - 1)] grouped by source, h_counts [n].  Synchronises.
 * PQH_ERR_ARG for a neighbour id outside the rows. */
int pqh_mst_build(pqh_ctx_t* ctx, const uint32_t* d_indices, const float* d_dists, long long n,
                  int num_nn, int take, const uint8_t* d_pq, int pq_m, float penalty,
                  uint32_t* h_targets, int* h_counts, long long* num_edges);

/* compute_nn_fast as a whole (the CLI, csrc/tools/compute_nn_fast.c): .fvecs rows in,
 * <out_template>nn_indices.ivecsl / nn_dist.fvecsl out.  options may be NULL (the reference
 * CLI's defaults, compute_nn_fast.c:164-175: 5 splits, 3 blocks, overlap 0.3).  A
 * blocks_info_cache that loads supplies the geometry; otherwise it is written
 * (fast_nn_blocks_info.c:124-172 layout).  with_blocks_stat writes blocks_stat.txt. */
typedef struct {
    int num_split;               /* --num-dims */
    int blocks_per_dim;          /* --num-blocks-per-dim */
    double overlap;              /* --block-overlap-fraction */
    const char* blocks_info_cache;
    int with_blocks_stat;
} pqh_knn_options_t;
int pqh_knn_fast_files(const char* input_fvecs, const char* out_template, int num_nn,
                       const pqh_knn_options_t* options);
/* mst_builder as a whole (mst_builder.c:98-131): <nn_template>nn_indices.ivecsl +
 * nn_dist.fvecsl (+ <pq_template>pq_indices.bvecsl, may be NULL) in; <out_template>mst.tree,
 * and with PQ codes stats.json / stats_num_children.json (appended) plus the indices stats
 * line on stdout. */
int pqh_mst_files(const char* nn_template, const char* out_template, int take,
                  const char* pq_template, float penalty);

/* ---- tree-ordered context coding (huffman_encoder.c --tree: :240-286, :321-375) ---- */
/* DFS order of a stored forest (mst.tree: tree_load_file, mst.c:273-288 -- num_edges
 * u32 targets grouped by source, children_counts[v] of them per vertex) exactly as
 * tree_collect_vertices_dfs (mst.c:290-364), plus each stream row's coding context, the
 * traverser's active parent (mst.c:366-405): parents[p] = the parent's vertex id, or -1 for
 * a root.  Host; returns num_roots (>= 1 when num_vertices > 0) or PQH_ERR_ARG.
 * parents may be NULL. */
int pqh_tree_order(long long num_vertices, long long num_edges, const uint32_t* edge_targets,
                   const int* children_counts, uint32_t* vertices, int* num_children,
                   long long* parents);
/* pqh_tree_order on the device, for a forest (no self-loop, every edge stored in both
 * directions once, no cycle): device counts/targets in, device vertices / num_children /
 * parents (may be NULL) out, *num_roots on the host.  PQH_ERR_UNSUPPORTED for a graph that is
 * not such a forest (nothing written; pqh_tree_order walks any graph), PQH_ERR_ARG for
 * counts that are negative or do not sum to num_edges.  Synchronises. */
int pqh_tree_order_device(pqh_ctx_t* ctx, long long num_vertices, long long num_edges,
                          const uint32_t* d_edge_targets, const int* d_children_counts,
                          uint32_t* d_vertices, int* d_num_children, long long* d_parents,
                          int* num_roots);
/* d_rows[p] = d_codes[d_vertices[p]] (stream order) and d_tree_prev[p][i] =
 * d_codes[d_parents[p]][i], 0xFFFF for a root.  Ids outside [0, n) are reported by
 * pqh_tree_status (nothing is read for them). */
int pqh_tree_gather(pqh_ctx_t* ctx, const void* d_codes, long long n, int m, int k,
                    const uint32_t* d_vertices, const long long* d_parents, void* d_rows,
                    uint16_t* d_tree_prev);
/* Synchronises; PQH_ERR_ARG if the last pqh_tree_gather met an id outside the rows. */
int pqh_tree_status(pqh_ctx_t* ctx);
/* counts[i][prev][cur] += pairs (d_tree_prev[p][i], d_rows[p][i]) of the non-root rows
 * (tree_collect_indices_stats, mst.c:442-490); K = 256, u8 rows. */
int pqh_histogram_tree(pqh_ctx_t* ctx, const void* d_rows, const uint16_t* d_tree_prev,
                       long long n, int m, int k, uint32_t* d_counts);
/* encode_tree_data (huffman_encoder.c:240-286): context tables, each row coded in its
 * d_tree_prev context, roots raw 8 bits per part.  Same buffer rules as pqh_encode_write;
 * chunk_vectors > 0 emits the chunk bit offsets (the tree decoder's index). */
int pqh_encode_tree_write(pqh_ctx_t* ctx, const pqh_tables_t* t, const void* d_rows,
                          const uint16_t* d_tree_prev, long long n,
                          unsigned long long bit_offset, unsigned char* d_out,
                          unsigned long long out_bytes, int chunk_vectors,
                          unsigned long long* d_chunk_offsets, unsigned long long* d_total_bits);
/* Decode-side index from the child counts (decoded children stream): parent_pos[p] = the
 * stream position of row p's context (-1: root; huffman_decoder.c:214-247), and per chunk
 * of C rows the rows whose context precedes the chunk: ext_offsets[chunks + 1] into
 * ext_positions (may be NULL to count).  Host; returns the ext count or PQH_ERR_ARG. */
long long pqh_tree_ext_index(long long n, const int* num_children, int chunk_vectors,
                             long long* parent_pos, long long* ext_offsets,
                             long long* ext_positions);
/* pqh_tree_ext_index on the device, from device child counts (child_bytes 1, 2 or 4: u8,
 * u16 or i32): d_parent_pos[n], d_ext_offsets[chunks + 1] and, unless NULL,
 * d_ext_positions (room for n); returns the ext count or a negative status.  Same results
 * as the host walk for any counts.  Synchronises. */
long long pqh_tree_ext_index_device(pqh_ctx_t* ctx, long long n, const void* d_num_children,
                                    int child_bytes, int chunk_vectors, long long* d_parent_pos,
                                    long long* d_ext_offsets, long long* d_ext_positions);
/* huffman_decoder --tree on the GPU: rows in stream order.  One lane per chunk (offsets
 * from pqh_encode_tree_write); a context inside the chunk is read from the chunk's own
 * decoded rows, one before it from d_ext_rows[d_ext_offsets[j]...] (m codes each, the rows
 * at ext_positions).  stream_bytes is the stream's exact length (d_stream readable up to the
 * next multiple of 4 bytes); a chunk whose offset or symbols pass stream_bytes * 8 bits (a
 * truncated file, a stale sidecar) is an error.  Errors are reported by pqh_decode_status. */
int pqh_decode_tree(pqh_ctx_t* ctx, const pqh_tables_t* t, const unsigned char* d_stream,
                    unsigned long long stream_bytes, long long n, int chunk_vectors,
                    const unsigned long long* d_chunk_offsets, const long long* d_parent_pos,
                    const long long* d_ext_offsets, const unsigned char* d_ext_rows,
                    void* d_rows);

/* ---- whole-file host helpers used by the CLI tools ------------------------------- */
typedef struct {
    int context;           /* order-1 context coding (default 1) */
    int sort;              /* 0 none, 1 strncmp sort (default 1) */
    int chunk_vectors;     /* decode chunk size for the sidecar (default 64) */
    int only_estimate;     /* stats only (huffman_encoder --only-estimate) */
} pqh_encode_options_t;

/* Runs histogram -> GPU codebooks -> encode on host codes (n x m, K=256).  Produces the
 * reference files under out_prefix: huffman_codebooks.bin, huffman_indices.bin,
 * huffman_stats.txt (appended), and the decode sidecar huffman_chunks.bin. */
int pqh_encode_files(const unsigned char* codes, long long n, int m,
                     const pqh_encode_options_t* options, const char* out_prefix);
/* huffman_encoder --tree <tree_path>: tree-ordered context coding of host codes (n x m,
 * K = 256) over the forest stored in mst.tree (sorted first when sort != 0, as the CLI
 * does).  Writes the reference's tree-mode files under out_prefix: huffman_codebooks.bin,
 * huffman_indices.bin, huffman_stats.txt, huffman_children_codebooks.bin,
 * huffman_children.bin, huffman_children_stats.txt, plus the decode sidecar
 * huffman_tree_chunks.bin (pqh extension: chunk bit offsets + ext context rows). */
int pqh_encode_tree_files(const unsigned char* codes, long long n, int m, int sort,
                          const char* tree_path, const char* out_prefix);
/* huffman_decoder --tree: decodes the tree-mode files under in_prefix into rows in stream
 * (DFS) order, as the reference decoder writes them.  Needs the decode sidecar
 * huffman_tree_chunks.bin that pqh_encode_tree_files writes (PQH_ERR_ARG without it). */
int pqh_decode_tree_files(const char* in_prefix, unsigned char** codes_out, long long* n_out,
                          int* m_out);
/* Decodes huffman_indices.bin (+ sidecar when present) under in_prefix into codes
 * (n x m host buffer, n from the file header). */
int pqh_decode_files(const char* in_prefix, unsigned char** codes_out, long long* n_out,
                     int* m_out);
/* Rows [first, first + count) of huffman_indices.bin under in_prefix, in stream order (the
 * encoder's order: sorted unless it ran with sort = 0), into a malloc'd count x m host buffer
 * (huffman_decoder.c:211-255 for those rows only).  Reads the code books, the sidecar's index
 * entries of the range's chunks and only those chunks' bytes of the stream, and decodes them
 * with pqh_decode_range.  The sidecar huffman_chunks.bin is required: without it (or with one
 * that does not match the stream) the call returns PQH_ERR_ARG and names the file on stderr --
 * there is no fall-back to a full decode.  A range outside the file's rows, or count <= 0, is
 * PQH_ERR_ARG.  Non-tree streams only. */
int pqh_decode_files_range(const char* in_prefix, long long first, long long count,
                           unsigned char** codes_out, int* m_out);

#ifdef __cplusplus
}
#endif

#endif /* _PQH_H */
