/*
 * bitnuc_hip.h -- C ABI of libbitnuc_hip.so: the MI355X (gfx950) replacement for
 * bitnuc's 2-bit pack/unpack + bulk encode/decode hot path.
 *
 * The reference (drbh/bitnuc, a pure-Rust crate) has no FFI of its own; the
 * drop-in boundary is its public Rust API (src/lib.rs:214-220).  Each entry point
 * below names the reference function it replaces.  A Rust `extern "C"` binding
 * for every symbol is shown in INTEGRATION.md / rust/src/ffi.rs; include/bitnuc.hpp
 * is the compiled C++ host layer with the reference's names and Vec semantics.
 *
 * All bulk compute happens in hand-written HIP kernels (bitnuc_amd/csrc/).  There is
 * no CPU fallback: without a usable HIP device context creation fails and every
 * device-pointer call and every bulk call at or above the host cutoff returns
 * BITNUC_BACKEND_ERROR / BITNUC_UNSUPPORTED.
 *
 * Size dispatch: the reference's as_2bit / from_2bit / hdist_scalar are
 * #[inline(always)] nanosecond functions, and a kernel launch with its copies costs
 * ~35 us, so the three single-word entry points and bulk HOST-POINTER calls below
 * `host_cutoff` bases (default: the measured host / GPU crossover, 1 Mi bases for encode and hdist, 512 Ki for decode; bitnuc_ctx_set_variant(ctx, "host_cutoff", n) or
 * BITNUC_HOST_CUTOFF) run as the library's own SWAR host code (csrc/host_word.h) and
 * accept ctx == NULL.  bitnuc_ctx_set_variant(ctx, "force_gpu", 1) or BITNUC_FORCE_GPU=1
 * sends every call MADE WITH THAT CONTEXT to the kernels (batches of one) -- the GPU parity
 * tests run that way; calls with ctx == NULL have no context to carry the flag and stay on the host.
 *
 * Asynchronous launches and their data errors.  Every _dev launch that can meet an invalid base owns
 * one device-resident error slot; bitnuc_ctx_sync() waits for the stream and reports the first latched
 * error: ordinary launches in launch order, then launches recorded into a hipGraph in capture order.
 *   - The slot ring starts at 4096 launches and GROWS (device + pinned allocation, no stream
 *     synchronisation) when more are queued between two syncs; only past 2 Mi unsynced launches does a
 *     _dev call drain the stream itself (the error it finds is kept for the next bitnuc_ctx_sync).
 *   - While the context's stream is being CAPTURED (hipStreamBeginCapture / torch.cuda.graph) a launch
 *     gets a persistent slot instead: the captured kernel runs again at every replay, so every later
 *     bitnuc_ctx_sync() examines that slot and re-arms it.  An InvalidBase met by a replay is therefore
 *     reported by the first sync after it, and never against another launch.  A context holds at most
 *     1024 captured launches over its life (BITNUC_UNSUPPORTED, err.value = 1024 beyond that); replay the
 *     graph on the context's stream, or order it before the sync yourself.  Entry points documented as
 *     synchronous (word offsets, plan build, every host-pointer call, bitnuc_ctx_sync) cannot be captured.
 *   - The table-driven batch calls (bitnuc_encode_batch_dev / bitnuc_decode_batch_dev) keep their layout plan in context scratch,
 *     sized by the largest batch seen.  A call that would have to GROW it while the stream is being captured returns
 *     BITNUC_UNSUPPORTED (err.value = the bytes needed) before anything is touched -- warm up with the largest batch, or use a
 *     bitnuc_batch_plan; a scratch buffer that a recorded launch was handed stays alive until bitnuc_ctx_destroy (a later,
 *     larger ordinary call allocates a new one), so replays never write into freed memory.
 *   - Data errors found by implicit drains (a host-pointer call starts from an empty slot ring, and so does the 2 Mi limit above) are
 *     kept in launch order, oldest first, one per bitnuc_ctx_sync: with errors A and B kept from two such drains and a third one, C,
 *     that only the sync's own drain finds, three syncs report A, B, C (at most 64 are kept between syncs).
 *
 * Conventions
 *   - plain pointers + sizes, no torch / C++ types in signatures;
 *   - return value == err->status (err may be NULL);
 *   - "host" entry points take host pointers and are synchronous; large encode / decode
 *     calls (>= 8 Mi bases) are pipelined in 32 Mi-base chunks: the calling thread copies chunk c from the
 *     caller's memory to the device and launches on it while ONE helper thread of the context copies chunk
 *     c-1's output into the caller's memory (the runtime pins pageable buffers in place: both copies run at
 *     the DMA rate, each blocks only the thread that issued it); bitnuc_host_pipe_info reports the chunk size;
 *     bitnuc_as_2bit_batch, bitnuc_kmer_hdist_scan, bitnuc_encode_fixed and (back-to-back reads) bitnuc_decode_fixed
 *     ride the same engine from 8 MiB of input; the other host entry points (and smaller inputs) stage through
 *     device scratch in 128 Mbase chunks;
 *     "_dev" entry points take device pointers, are enqueued
 *     on the context's stream and return immediately -- data-dependent errors
 *     (InvalidBase) are latched on the device and reported by bitnuc_ctx_sync(); the "_async" entry points
 *     (bitnuc_kmer_hdist_best[_packed]_async, bitnuc_kmer_pattern_*_async, bitnuc_kmer_edist_*_async, bitnuc_reads_*_async) have exactly the "_dev" contract under another suffix;
 *   - a bitnuc_ctx owns one device + stream + scratch and must not be used from
 *     two threads at once; separate contexts are independent.
 */
#ifndef BITNUC_HIP_H
#define BITNUC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* NucleotideError, src/error.rs:3-18, plus a backend status that has no reference
 * counterpart (HIP runtime failure). */
typedef enum bitnuc_status {
    BITNUC_OK = 0,
    BITNUC_INVALID_BASE = 1,        /* InvalidBase(u8)         -> err.byte, err.index */
    BITNUC_SEQUENCE_TOO_LONG = 2,   /* SequenceTooLong(usize)  -> err.value */
    BITNUC_INVALID_LENGTH = 3,      /* InvalidLength(usize)    -> err.value */
    BITNUC_INDEX_OUT_OF_BOUNDS = 4, /* IndexOutOfBounds{index,length} -> err.index, err.value (split_packed) */
    BITNUC_INVALID_RANGE = 5,       /* decreasing offsets in the ragged-batch entry points -> err.value = index */
    BITNUC_UNSUPPORTED = 6,         /* Unsupported (bad argument combination) */
    BITNUC_BACKEND_ERROR = 100      /* hipError_t in err.backend_code */
} bitnuc_status;

typedef struct bitnuc_err {
    int32_t status;       /* bitnuc_status */
    int32_t backend_code; /* hipError_t when status == BITNUC_BACKEND_ERROR */
    uint64_t value;       /* offending length for TOO_LONG / INVALID_LENGTH */
    uint64_t index;       /* absolute byte index of the first invalid base */
    uint8_t byte;         /* the first invalid base */
    uint8_t _pad[7];
} bitnuc_err;

typedef struct bitnuc_ctx bitnuc_ctx;

/* ---- context ------------------------------------------------------------------ */
/* Create a context on HIP device `device` with its own non-blocking stream. */
int bitnuc_ctx_create(int device, bitnuc_ctx **out, bitnuc_err *err);
/* Same, but enqueue on a caller-owned hipStream_t (e.g. torch's current stream;
 * NULL = the default stream).  The stream is not destroyed with the context. */
int bitnuc_ctx_create_on_stream(int device, void *hip_stream, bitnuc_ctx **out, bitnuc_err *err);
void bitnuc_ctx_destroy(bitnuc_ctx *ctx);
/* Wait for everything enqueued on the context's stream, then report (and clear)
 * the first latched data error of the launches since the last sync. */
int bitnuc_ctx_sync(bitnuc_ctx *ctx, bitnuc_err *err);
/* The context's hipStream_t, for callers that order their own work against it. */
void *bitnuc_ctx_stream(bitnuc_ctx *ctx);
/* Library / build identification: "bitnuc_hip <ver> gfx950 csrc:<16 hex digits>[ sweep]" -- the hex digits are the SHA-256 prefix of the
 * sources the library was compiled from (csrc/ incl. csrc/evidence/, this header), passed by bitnuc_amd/build.py as -DBITNUC_CSRC_SHA
 * ("csrc:unknown" for a build without it); " sweep" marks the evidence build (-DBITNUC_SWEEP_VARIANTS). */
const char *bitnuc_version(void);

/* ---- single-word API (host code, ctx may be NULL; see "Size dispatch" above) ------------------ */
/* as_2bit(seq:&[u8]) -> Result<u64>          src/utils/packing/mod.rs:80-110
 * len > 32 -> SEQUENCE_TOO_LONG(len) before any base is looked at; first bad byte
 * -> INVALID_BASE(byte, index); len == 0 -> OK, 0.  For many k-mers use bitnuc_as_2bit_batch. */
int bitnuc_as_2bit(bitnuc_ctx *ctx, const uint8_t *seq, size_t len, uint64_t *out, bitnuc_err *err);
/* from_2bit(packed, expected_size, &mut Vec<u8>)  src/utils/unpacking/mod.rs:119-147
 * n > 32 -> INVALID_LENGTH(n).  Writes exactly n bytes at out (the Vec append
 * offset is the caller's: include/bitnuc.hpp, rust/src/lib.rs). */
int bitnuc_from_2bit(bitnuc_ctx *ctx, uint64_t packed, size_t n, uint8_t *out, bitnuc_err *err);
/* hdist_scalar(u, v, len) -> Result<u32>     src/utils/functions/hamming/scalar.rs:11-48 */
int bitnuc_hdist_scalar(bitnuc_ctx *ctx, uint64_t u, uint64_t v, size_t len, uint32_t *out, bitnuc_err *err);

/* ---- bulk API, host pointers (synchronous) ------------------------------------ */
/* encode(sequence, &mut Vec<u64>)            src/utils/mod.rs:22-25 -> packing/avx.rs:130-151
 * out must hold ceil(len/32) words.  On success *n_words = ceil(len/32), last word
 * zero-padded high.  On INVALID_BASE: err.byte/err.index = first invalid byte of
 * the whole sequence and *n_words = err.index/32 (the words the reference's Vec
 * holds at that point); out[*n_words..] is unspecified.  len == 0 -> OK with 0
 * words (the reference panics there; shims may mirror that). */
int bitnuc_encode(bitnuc_ctx *ctx, const uint8_t *seq, size_t len, uint64_t *out, size_t *n_words, bitnuc_err *err);
/* decode(ebuf, n_bases, &mut Vec<u8>)        src/utils/mod.rs:60-62 -> unpacking/avx.rs:116-153
 * Writes n_bases bytes at out.  n_words < ceil(n_bases/32) -> INVALID_LENGTH(n_bases)
 * (the rule of unpacking/mod.rs:40-45; the AVX2 path panics there). */
int bitnuc_decode(bitnuc_ctx *ctx, const uint64_t *ebuf, size_t n_words, size_t n_bases, uint8_t *out, bitnuc_err *err);
/* hdist(ebuf1, ebuf2, n_bases) -> Result<u32>  src/utils/functions/hamming/multi.rs:121-160 */
int bitnuc_hdist(bitnuc_ctx *ctx, const uint64_t *a, size_t na, const uint64_t *b, size_t nb, size_t n_bases, uint32_t *out, bitnuc_err *err);
/* Batched as_2bit over `count` k-mers, k-mer j at kmers + j*stride (README.md:52-56
 * host-loop idiom; stride 1 = every window of a sequence, src/lib.rs:170-173).
 * k > 32 -> SEQUENCE_TOO_LONG(k).  First invalid examined byte -> INVALID_BASE.
 * Any stride >= 1 works; stride == k (dense) and every stride <= k below 32 (overlapping windows; 1 = all
 * windows of a sequence) have dedicated kernels and run about 3x faster than the general one. */
int bitnuc_as_2bit_batch(bitnuc_ctx *ctx, const uint8_t *kmers, size_t k, size_t stride, size_t count, uint64_t *out, bitnuc_err *err);
/* Sliding-window k-mer pack + Hamming distance to a packed query: dist[i] =
 * hdist_scalar(as_2bit(ref[i..i+k]), query, k) for i in 0..n-k+1
 * (composition of packing/mod.rs:80-110 and hamming/scalar.rs:11-48). */
int bitnuc_kmer_hdist_scan(bitnuc_ctx *ctx, const uint8_t *ref, size_t n, size_t k, uint64_t query, uint8_t *dist, bitnuc_err *err);

/* ---- bulk API, device pointers (asynchronous on the context's stream) ------------ */
/* The roofline entry points: inputs and outputs stay resident in HBM.  d_seq /
 * d_out may have any alignment (16-byte aligned input is the fast path).
 * Argument errors are returned immediately; InvalidBase is latched for
 * bitnuc_ctx_sync(). */
int bitnuc_encode_dev(bitnuc_ctx *ctx, const uint8_t *d_seq, size_t len, uint64_t *d_out, bitnuc_err *err);
int bitnuc_decode_dev(bitnuc_ctx *ctx, const uint64_t *d_ebuf, size_t n_words, size_t n_bases, uint8_t *d_out, bitnuc_err *err);
int bitnuc_as_2bit_batch_dev(bitnuc_ctx *ctx, const uint8_t *d_kmers, size_t k, size_t stride, size_t count, uint64_t *d_out, bitnuc_err *err);
int bitnuc_kmer_hdist_scan_dev(bitnuc_ctx *ctx, const uint8_t *d_ref, size_t n, size_t k, uint64_t query, uint8_t *d_dist, bitnuc_err *err);
/* The same scan with the fused threshold of SURVEY 8(d) cfg 5: *d_count (one uint64 in device memory) = number of windows i with
 * hdist_scalar(as_2bit(ref[i..i+k]), query, k) <= tau.  No distance bytes are written: 1 byte read per window. */
int bitnuc_kmer_hdist_count_dev(bitnuc_ctx *ctx, const uint8_t *d_ref, size_t n, size_t k, uint64_t query, unsigned tau, uint64_t *d_count, bitnuc_err *err);
/* The scan and its fused count on a PACKED sequence: words[0 .. n_words) hold n bases (base i at bits 2 (i mod 32) of words[i / 32]), window j is
 * as_2bit(decode(words, n)[j .. j+k]); the results are byte-identical to the ASCII forms on decode(words, n).  Bits above 2n in the last word and the
 * query's bits above 2k are ignored.  Checks, in this order: k > 32 -> SEQUENCE_TOO_LONG(k); n_words < ceil(n/32) -> INVALID_LENGTH(n); k == 0 or
 * n < k -> OK with no windows (the count writes 0); a NULL pointer, words not 8-byte aligned or a count not 8-byte aligned -> UNSUPPORTED.  Packed
 * input holds no invalid base.  d_words 16-byte aligned or at 8 mod 16 run the same kernels at the same speed; d_dist may have any byte offset.
 * The _dev forms are asynchronous on the context's stream and can be captured into a hipGraph. */
int bitnuc_kmer_hdist_scan_packed_dev(bitnuc_ctx *ctx, const uint64_t *d_words, size_t n_words, size_t n, size_t k, uint64_t query, uint8_t *d_dist, bitnuc_err *err);
int bitnuc_kmer_hdist_count_packed_dev(bitnuc_ctx *ctx, const uint64_t *d_words, size_t n_words, size_t n, size_t k, uint64_t query, unsigned tau, uint64_t *d_count, bitnuc_err *err);
/* Host-pointer forms, sized like bitnuc_hdist: below the host cutoff they run on the host (ctx may be NULL), above it through the context. */
int bitnuc_kmer_hdist_scan_packed(bitnuc_ctx *ctx, const uint64_t *words, size_t n_words, size_t n, size_t k, uint64_t query, uint8_t *dist, bitnuc_err *err);
int bitnuc_kmer_hdist_count_packed(bitnuc_ctx *ctx, const uint64_t *words, size_t n_words, size_t n, size_t k, uint64_t query, unsigned tau, uint64_t *count, bitnuc_err *err);
/* The POSITIONS of the windows the count counts (a hit list).  *n_hits = the number of windows i with hdist_scalar(as_2bit(ref[i..i+k]), query, k) <= tau
 * -- exactly the count's value for the same arguments, and it may exceed cap.  pos[0 .. min(cap, *n_hits)) = the first such windows in ASCENDING
 * order; hit_dist[j] = the distance of window pos[j] (hit_dist may be NULL: not written).  Nothing at or beyond index cap is written in either array.
 * The result is deterministic.  tau >= k makes every window a hit (any unsigned tau is valid); k == 0 or n < k -> OK with *n_hits = 0.
 * Checks, in this order: the count's (ASCII: k > 32 -> SEQUENCE_TOO_LONG(k); packed: as the packed scan above), then n_hits NULL or not 8-byte aligned,
 * pos not 8-byte aligned or NULL with cap > 0 -> UNSUPPORTED (host forms: NULL only), then no windows -> OK, then a NULL ref -> UNSUPPORTED.
 * An invalid base -> INVALID_BASE with the first invalid byte in sequence order, as the count (the _dev forms latch it for bitnuc_ctx_sync(); pos
 * and hit_dist are then unspecified).  d_ref may have any alignment at the same speed (the up to 15 windows before its first 16-byte aligned base take
 * the tail's path); d_words 16-byte aligned or at 8 mod 16.  The _dev forms are asynchronous on the context's stream (no host synchronisation: three
 * launches, the per-trip counts in context scratch) and can be captured into a hipGraph; d_n_hits is one uint64 in device memory.  The host forms
 * are synchronous: below the host cutoff on the host (ctx may be NULL), above it through the context in chunks of 128 M windows. */
int bitnuc_kmer_hdist_hits_dev(bitnuc_ctx *ctx, const uint8_t *d_ref, size_t n, size_t k, uint64_t query, unsigned tau, uint64_t *d_pos, uint8_t *d_hit_dist,
                               size_t cap, uint64_t *d_n_hits, bitnuc_err *err);
int bitnuc_kmer_hdist_hits_packed_dev(bitnuc_ctx *ctx, const uint64_t *d_words, size_t n_words, size_t n, size_t k, uint64_t query, unsigned tau, uint64_t *d_pos,
                                      uint8_t *d_hit_dist, size_t cap, uint64_t *d_n_hits, bitnuc_err *err);
int bitnuc_kmer_hdist_hits(bitnuc_ctx *ctx, const uint8_t *ref, size_t n, size_t k, uint64_t query, unsigned tau, uint64_t *pos, uint8_t *hit_dist, size_t cap,
                           uint64_t *n_hits, bitnuc_err *err);
int bitnuc_kmer_hdist_hits_packed(bitnuc_ctx *ctx, const uint64_t *words, size_t n_words, size_t n, size_t k, uint64_t query, unsigned tau, uint64_t *pos,
                                  uint8_t *hit_dist, size_t cap, uint64_t *n_hits, bitnuc_err *err);
/* The fused count for MANY queries in one pass over the reference: counts[q] = the number of windows i with
 * hdist_scalar(as_2bit(ref[i..i+k]), queries[q], k) <= taus[q] -- exactly what bitnuc_kmer_hdist_count[_packed]_dev returns for (ref, n, k, queries[q],
 * taus[q]).  Query bits above 2k are ignored; any uint32_t tau is valid (tau >= k counts every window), and a per-query tau costs nothing (a query repeated
 * with tau = 0, 1, 2, 3 gives its mismatch profile in one call; bitnuc_kmer_hdist_hist* below gives the whole profile, up to 16 bins, from ONE query per
 * profile and without the subtraction).  counts[0 .. n_queries) is written and nothing after it.
 * Checks, in this order: (1) ctx NULL -> UNSUPPORTED (_dev forms; the host forms below the cutoff accept NULL); (2) k > 32 -> SEQUENCE_TOO_LONG(k);
 * (3) packed: n_words < ceil(n/32) -> INVALID_LENGTH(n); (4) n_queries == 0 -> OK, nothing written; (5) n_queries > BITNUC_MAX_QUERIES -> UNSUPPORTED
 * (err.value = n_queries); (6) counts, queries or taus NULL or not 8-, 8-, 4-byte aligned -> UNSUPPORTED; (7) k == 0 or n < k -> OK, every count 0;
 * (8) a NULL reference, or packed words not 8-byte aligned -> UNSUPPORTED.
 * ASCII: an invalid base -> INVALID_BASE with the first invalid byte in sequence order, as the single count (the _dev forms latch it once per call for
 * bitnuc_ctx_sync(); the counts are then unspecified).  d_ref may have any alignment (the up to 15 windows before its first 16-byte aligned base take the
 * tail's path); packed words 16-byte aligned or at 8 mod 16.
 * The _dev forms are asynchronous on the context's stream; queries, taus and counts are in device memory.  They build one table per query in context
 * scratch (3 KiB each) and can be captured into a hipGraph, but scratch cannot grow during a capture (BITNUC_UNSUPPORTED, err.value = the bytes needed):
 * warm up with the same (or a larger) n_queries first.
 * The host forms are synchronous.  When windows x n_queries is below the host cutoff (as the single-query host forms judge their bases) they run on the
 * host and ctx may be NULL; above it they run through the context in chunks of 128 M windows that overlap by k - 1 bases, summing per query. */
#define BITNUC_MAX_QUERIES 65536
int bitnuc_kmer_hdist_count_multi_dev(bitnuc_ctx *ctx, const uint8_t *d_ref, size_t n, size_t k, const uint64_t *d_queries, const uint32_t *d_taus,
                                      size_t n_queries, uint64_t *d_counts, bitnuc_err *err);
int bitnuc_kmer_hdist_count_multi_packed_dev(bitnuc_ctx *ctx, const uint64_t *d_words, size_t n_words, size_t n, size_t k, const uint64_t *d_queries,
                                             const uint32_t *d_taus, size_t n_queries, uint64_t *d_counts, bitnuc_err *err);
int bitnuc_kmer_hdist_count_multi(bitnuc_ctx *ctx, const uint8_t *ref, size_t n, size_t k, const uint64_t *queries, const uint32_t *taus, size_t n_queries,
                                  uint64_t *counts, bitnuc_err *err);
int bitnuc_kmer_hdist_count_multi_packed(bitnuc_ctx *ctx, const uint64_t *words, size_t n_words, size_t n, size_t k, const uint64_t *queries,
                                         const uint32_t *taus, size_t n_queries, uint64_t *counts, bitnuc_err *err);
/* The BEST MATCH per query in one pass over the reference: dist[q] = the minimum over the windows i in 0..n-k+1 of
 * hdist_scalar(as_2bit(ref[i..i+k]), queries[q], k) and pos[q] = the smallest i that attains it -- what an arg-min over bitnuc_kmer_hdist_scan's distance
 * bytes gives per query (composition of packing/mod.rs:80-110 and hamming/scalar.rs:11-48), without writing or reading those bytes: one byte read per
 * window whatever the number of queries.  The result is deterministic.  Query bits above 2k are ignored.  With no windows (k == 0 or n < k) every
 * pos[q] = UINT64_MAX and every dist[q] = 0xFF.  pos[0 .. n_queries) and dist[0 .. n_queries) are written and nothing after them.
 * Checks, in this order: (1) ctx NULL -> UNSUPPORTED (_async forms; the host forms below the cutoff accept NULL); (2) k > 32 -> SEQUENCE_TOO_LONG(k);
 * (3) packed: n_words < ceil(n/32) -> INVALID_LENGTH(n); (4) n_queries == 0 -> OK, nothing written; (5) n_queries > BITNUC_MAX_QUERIES -> UNSUPPORTED
 * (err.value = n_queries); (6) pos or queries NULL or not 8-byte aligned, or dist NULL -> UNSUPPORTED (dist may have any byte offset); (7) k == 0 or
 * n < k -> OK with the values above; (8) a NULL reference, or packed words not 8-byte aligned -> UNSUPPORTED.
 * ASCII: an invalid base -> INVALID_BASE with the first invalid byte in sequence order (the _async forms latch it once per call for bitnuc_ctx_sync();
 * pos and dist are then unspecified).  d_ref may have any alignment (the up to 15 windows before its first 16-byte aligned base take the tail's path);
 * packed words 16-byte aligned or at 8 mod 16.
 * The _async forms have the _dev contract: device pointers (queries, pos and dist included), enqueued on the context's stream, no host synchronisation
 * (with the one exception below), InvalidBase latched for bitnuc_ctx_sync().  They keep one key per query and one table per query (2.5 KiB) in context scratch and can be captured into
 * a hipGraph, but scratch cannot grow during a capture (BITNUC_UNSUPPORTED, err.value = the bytes needed): warm up with the same (or a larger)
 * n_queries first.  Outside a capture a call that needs more scratch than the context holds (a larger n_queries than any call before it) waits for the
 * stream before it replaces the allocation, as the multi-query count does: a queue that must never wait starts with its largest n_queries.
 * The host forms are synchronous.  When windows x n_queries is below the host cutoff (as the multi-query count judges it) they run on the host and ctx
 * may be NULL; above it they run through the context in chunks of 128 M windows that overlap by k - 1 bases, merged by the smallest (dist, pos). */
int bitnuc_kmer_hdist_best_async(bitnuc_ctx *ctx, const uint8_t *d_ref, size_t n, size_t k, const uint64_t *d_queries, size_t n_queries, uint64_t *d_pos,
                                 uint8_t *d_dist, bitnuc_err *err);
int bitnuc_kmer_hdist_best_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, size_t n_words, size_t n, size_t k, const uint64_t *d_queries,
                                        size_t n_queries, uint64_t *d_pos, uint8_t *d_dist, bitnuc_err *err);
int bitnuc_kmer_hdist_best(bitnuc_ctx *ctx, const uint8_t *ref, size_t n, size_t k, const uint64_t *queries, size_t n_queries, uint64_t *pos, uint8_t *dist,
                           bitnuc_err *err);
int bitnuc_kmer_hdist_best_packed(bitnuc_ctx *ctx, const uint64_t *words, size_t n_words, size_t n, size_t k, const uint64_t *queries, size_t n_queries,
                                  uint64_t *pos, uint8_t *dist, bitnuc_err *err);
/* PATTERN queries for the multi-query count, the best match and the hit lists: position i < k of a pattern accepts a SET S_i of bases instead of one base,
 * and the distance of window j is pdist(j) = #{ i < k : ref[j+i] not in S_i }.  A guide search NNNNNNNNNNNNNNNNNNNNNGG is twenty positions whose
 * mismatches are counted (their exact bases), one that never counts (N) and two that must match; primers and adapters use R, Y, N.  A pattern of
 * singletons S_i = {q_i} makes pdist equal to hdist_scalar(as_2bit(ref[j..j+k]), q, k), what the exact entry points compute; an empty set mismatches every
 * base and is legal.  Only the query's side of the matrix-core product changes (its table and the accumulators' start values): a pattern costs what an
 * exact query costs. */
typedef struct bitnuc_pattern { uint32_t allow[4]; } bitnuc_pattern;
/* allow[c] bit i set <=> base code c (A=0, C=1, G=2, T=3) matches at position i; bits at positions >= k are ignored */
/* The converters are host code and take no context.  _from_iupac: k letters of ACGTU RYSWKM BDHV N in either case (U = T); k > 32 ->
 * SEQUENCE_TOO_LONG(k) before any letter is read; any other byte -> INVALID_BASE(byte, index); out NULL (or letters NULL with k > 0) -> UNSUPPORTED.
 * _from_2bit: the singletons of a packed exact query (query bits above 2k are ignored); k > 32 -> SEQUENCE_TOO_LONG(k). */
int bitnuc_pattern_from_iupac(const uint8_t *letters, size_t k, bitnuc_pattern *out, bitnuc_err *err);
int bitnuc_pattern_from_2bit(uint64_t query, size_t k, bitnuc_pattern *out, bitnuc_err *err);
/* The pattern twins of bitnuc_kmer_hdist_count_multi*, _best* and _hits*: `const bitnuc_pattern *patterns` (n_queries of them) stands where
 * `const uint64_t *queries` stood, `const bitnuc_pattern *pattern` (one, by HOST pointer in every form) where `uint64_t query` stood, pdist where
 * hdist_scalar stood.  Everything else is the twin's contract word for word: the same checks in the same order with "queries NULL or not 8-byte aligned"
 * read as "patterns NULL or not 4-byte aligned", the same BITNUC_MAX_QUERIES, the same results with no windows, the same chunking of the host forms above
 * the cutoff, the same freedom of alignment for d_ref / d_words, the same context scratch.  tau >= k counts (or hits) every window.  A non-ACGT byte in
 * the REFERENCE is still INVALID_BASE: the sets are on the query's side only.  A single-pattern count is count_multi with one pattern.  The distance-byte
 * scan has no pattern form.
 * The _async forms have exactly the _dev contract (as bitnuc_kmer_hdist_best_async): device pointers (patterns, taus and outputs included), enqueued on the
 * context's stream, no host synchronisation except the documented growth of context scratch, InvalidBase latched for bitnuc_ctx_sync(), capturable into a
 * hipGraph after a warm-up with the same (or a larger) n_queries.
 * Hit lists: *n_hits = the number of windows j with pdist(j) <= tau (it may exceed cap); pos[0 .. min(cap, *n_hits)) = the first such windows in ascending
 * order, hit_dist[r] = pdist(pos[r]) (hit_dist may be NULL); nothing at or beyond index cap is written.  A NULL pattern -> UNSUPPORTED, checked where pos
 * is checked. */
int bitnuc_kmer_pattern_count_multi_async(bitnuc_ctx *ctx, const uint8_t *d_ref, size_t n, size_t k, const bitnuc_pattern *d_patterns, const uint32_t *d_taus,
                                          size_t n_queries, uint64_t *d_counts, bitnuc_err *err);
int bitnuc_kmer_pattern_count_multi_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, size_t n_words, size_t n, size_t k, const bitnuc_pattern *d_patterns,
                                                 const uint32_t *d_taus, size_t n_queries, uint64_t *d_counts, bitnuc_err *err);
int bitnuc_kmer_pattern_count_multi(bitnuc_ctx *ctx, const uint8_t *ref, size_t n, size_t k, const bitnuc_pattern *patterns, const uint32_t *taus, size_t n_queries,
                                    uint64_t *counts, bitnuc_err *err);
int bitnuc_kmer_pattern_count_multi_packed(bitnuc_ctx *ctx, const uint64_t *words, size_t n_words, size_t n, size_t k, const bitnuc_pattern *patterns,
                                           const uint32_t *taus, size_t n_queries, uint64_t *counts, bitnuc_err *err);
int bitnuc_kmer_pattern_best_async(bitnuc_ctx *ctx, const uint8_t *d_ref, size_t n, size_t k, const bitnuc_pattern *d_patterns, size_t n_queries, uint64_t *d_pos,
                                   uint8_t *d_dist, bitnuc_err *err);
int bitnuc_kmer_pattern_best_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, size_t n_words, size_t n, size_t k, const bitnuc_pattern *d_patterns,
                                          size_t n_queries, uint64_t *d_pos, uint8_t *d_dist, bitnuc_err *err);
int bitnuc_kmer_pattern_best(bitnuc_ctx *ctx, const uint8_t *ref, size_t n, size_t k, const bitnuc_pattern *patterns, size_t n_queries, uint64_t *pos, uint8_t *dist,
                             bitnuc_err *err);
int bitnuc_kmer_pattern_best_packed(bitnuc_ctx *ctx, const uint64_t *words, size_t n_words, size_t n, size_t k, const bitnuc_pattern *patterns, size_t n_queries,
                                    uint64_t *pos, uint8_t *dist, bitnuc_err *err);
int bitnuc_kmer_pattern_hits_async(bitnuc_ctx *ctx, const uint8_t *d_ref, size_t n, size_t k, const bitnuc_pattern *pattern, unsigned tau, uint64_t *d_pos,
                                   uint8_t *d_hit_dist, size_t cap, uint64_t *d_n_hits, bitnuc_err *err);
int bitnuc_kmer_pattern_hits_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, size_t n_words, size_t n, size_t k, const bitnuc_pattern *pattern, unsigned tau,
                                          uint64_t *d_pos, uint8_t *d_hit_dist, size_t cap, uint64_t *d_n_hits, bitnuc_err *err);
int bitnuc_kmer_pattern_hits(bitnuc_ctx *ctx, const uint8_t *ref, size_t n, size_t k, const bitnuc_pattern *pattern, unsigned tau, uint64_t *pos, uint8_t *hit_dist,
                             size_t cap, uint64_t *n_hits, bitnuc_err *err);
int bitnuc_kmer_pattern_hits_packed(bitnuc_ctx *ctx, const uint64_t *words, size_t n_words, size_t n, size_t k, const bitnuc_pattern *pattern, unsigned tau,
                                    uint64_t *pos, uint8_t *hit_dist, size_t cap, uint64_t *n_hits, bitnuc_err *err);
/* The MISMATCH HISTOGRAM per query in one pass over the reference: hist[q * n_bins + d] = the number of windows i in 0..n-k+1 with
 * hdist_scalar(as_2bit(ref[i..i+k]), queries[q], k) == d, for d < n_bins (pattern forms: pdist(i) == d).  A window at distance n_bins or more is counted
 * nowhere.  Exactly hist[0 .. n_queries * n_bins) is written and nothing after it.  Query bits above 2k are ignored.  The result is deterministic
 * (integer sums).  With no windows (k == 0 or n < k) every entry is 0.  It is the profile an off-target report asks of a guide and a barcode or primer
 * check asks of a probe: one query and one table per profile where bitnuc_kmer_hdist_count_multi* needs one per bin and a subtraction afterwards.
 * Identities: the sum over d <= t of hist[q][d] equals bitnuc_kmer_hdist_count_multi*'s counts[q] with taus[q] = t (t < n_bins); the first non-zero bin is
 * bitnuc_kmer_hdist_best*'s dist[q] when that distance is below n_bins; with n_bins > k the bins of a query sum to n - k + 1.
 * Checks, in this order: (1) ctx NULL -> UNSUPPORTED (_async forms; the host forms below the cutoff accept NULL); (2) k > 32 -> SEQUENCE_TOO_LONG(k);
 * (3) packed: n_words < ceil(n/32) -> INVALID_LENGTH(n); (4) n_bins == 0 or n_bins > BITNUC_HIST_MAX_BINS -> UNSUPPORTED (err.value = n_bins);
 * (5) n_queries == 0 -> OK, nothing written; (6) n_queries > BITNUC_MAX_QUERIES -> UNSUPPORTED (err.value = n_queries); (7) hist or queries NULL or not
 * 8-byte aligned (patterns: NULL or not 4-byte aligned) -> UNSUPPORTED; (8) k == 0 or n < k -> OK, every entry 0; (9) a NULL reference, or packed words
 * not 8-byte aligned -> UNSUPPORTED.
 * ASCII: an invalid base -> INVALID_BASE with the first invalid byte in sequence order (the _async forms latch it once per call for bitnuc_ctx_sync();
 * hist is then unspecified; the host forms below the cutoff leave hist untouched).  d_ref may have any alignment (the up to 15 windows before its first
 * 16-byte aligned base take the tail's path); packed words 16-byte aligned or at 8 mod 16.
 * The _async forms have the _dev contract: device pointers (d_queries / d_patterns and d_hist included), enqueued on the context's stream, no host
 * synchronisation (with the one exception below), InvalidBase latched for bitnuc_ctx_sync().  They keep one table per query (2.5 KiB) in the context
 * scratch the best match uses and can be captured into a hipGraph, but scratch cannot grow during a capture (BITNUC_UNSUPPORTED, err.value = the bytes
 * needed): warm up with the same (or a larger) n_queries first.  Outside a capture a call that needs more scratch than the context holds waits for the
 * stream before it replaces the allocation, as the best match does.
 * The host forms are synchronous.  When windows x n_queries is below the host cutoff (as the multi-query count judges it) they run on the host and ctx
 * may be NULL; above it they run through the context in chunks of 128 M windows that overlap by k - 1 bases, summing per bin.
 * Cost: the best match's four matrix instructions per 1024 windows and query, then three vector instructions per window for every eight bins: n_bins <= 8
 * costs one such tier, 9 - 16 two.  Measured on 10^9 bases in one process (profiles/r12_kmer_hist.json; ASCII and packed, exact and pattern
 * queries alike): against count_multi with every query repeated n_bins times it takes 0.48 - 0.53 x the time at n_bins = 4, 0.24 - 0.27 x at 8 and
 * 0.20 - 0.22 x at 16 for 8 queries and more (one query: 0.69 - 0.72, 0.39 - 0.43, 0.30 - 0.40 x), so it pays from n_bins = 4, the smallest measured;
 * against the best match at the same number of queries 1.6 - 1.7 x with one tier and 2.6 - 2.9 x with two (one query: 1.5 and 2.1 - 2.6 x). */
#define BITNUC_HIST_MAX_BINS 16
int bitnuc_kmer_hdist_hist_async(bitnuc_ctx *ctx, const uint8_t *d_ref, size_t n, size_t k, const uint64_t *d_queries, size_t n_queries, size_t n_bins,
                                 uint64_t *d_hist, bitnuc_err *err);
int bitnuc_kmer_hdist_hist_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, size_t n_words, size_t n, size_t k, const uint64_t *d_queries,
                                        size_t n_queries, size_t n_bins, uint64_t *d_hist, bitnuc_err *err);
int bitnuc_kmer_hdist_hist(bitnuc_ctx *ctx, const uint8_t *ref, size_t n, size_t k, const uint64_t *queries, size_t n_queries, size_t n_bins, uint64_t *hist,
                           bitnuc_err *err);
int bitnuc_kmer_hdist_hist_packed(bitnuc_ctx *ctx, const uint64_t *words, size_t n_words, size_t n, size_t k, const uint64_t *queries, size_t n_queries,
                                  size_t n_bins, uint64_t *hist, bitnuc_err *err);
int bitnuc_kmer_pattern_hist_async(bitnuc_ctx *ctx, const uint8_t *d_ref, size_t n, size_t k, const bitnuc_pattern *d_patterns, size_t n_queries, size_t n_bins,
                                   uint64_t *d_hist, bitnuc_err *err);
int bitnuc_kmer_pattern_hist_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, size_t n_words, size_t n, size_t k, const bitnuc_pattern *d_patterns,
                                          size_t n_queries, size_t n_bins, uint64_t *d_hist, bitnuc_err *err);
int bitnuc_kmer_pattern_hist(bitnuc_ctx *ctx, const uint8_t *ref, size_t n, size_t k, const bitnuc_pattern *patterns, size_t n_queries, size_t n_bins, uint64_t *hist,
                             bitnuc_err *err);
int bitnuc_kmer_pattern_hist_packed(bitnuc_ctx *ctx, const uint64_t *words, size_t n_words, size_t n, size_t k, const bitnuc_pattern *patterns, size_t n_queries,
                                    size_t n_bins, uint64_t *hist, bitnuc_err *err);
/* d_result: one uint32 in device memory, overwritten with the distance. */
int bitnuc_hdist_dev(bitnuc_ctx *ctx, const uint64_t *d_a, size_t na, const uint64_t *d_b, size_t nb, size_t n_bases, uint32_t *d_result, bitnuc_err *err);

/* ---- ragged batches of independent sequences (reads, contigs) ----------------------------- */
/* The reference's idiom is a host loop `for s in seqs { encode(s, &mut ebuf)? }` /
 * `decode(&ebuf, len, &mut dbuf)?` (src/utils/mod.rs:22-25,60-62), each sequence padding its
 * own last word (packing/avx.rs:147-148).  Here the `count` sequences sit back to back:
 * sequence i = seq[offsets[i] .. offsets[i+1]) (offsets has count+1 non-decreasing entries)
 * and its ceil(len_i/32) words start at out[word_offsets[i]], where
 * word_offsets[i] = sum_{j<i} ceil(len_j/32) and word_offsets[count] = total words.
 * Zero-length sequences produce no words (the reference panics on them).  The first
 * invalid byte in buffer order -> INVALID_BASE{byte, index = byte offset in seq}.
 * Memory access: the batch and fixed-length kernels LOAD whole 16-byte aligned chunks, so up to
 * 15 bytes before seq[offsets[0]] and after seq[offsets[count]-1] are read (never validated, never
 * part of a word; an aligned 16-byte chunk cannot cross a page, so this cannot fault).  Stores
 * touch exactly the bytes of the batch: neighbours of an unaligned output are never written. */
/* Compute word_offsets (count+1 entries, device memory) from device offsets; synchronous;
 * *total_words = word_offsets[count]. */
int bitnuc_batch_word_offsets_dev(bitnuc_ctx *ctx, const uint64_t *d_offsets, size_t count, uint64_t *d_word_offsets, size_t *total_words, bitnuc_err *err);
int bitnuc_encode_batch_dev(bitnuc_ctx *ctx, const uint8_t *d_seq, const uint64_t *d_offsets, const uint64_t *d_word_offsets, size_t count, size_t total_words, uint64_t *d_out, bitnuc_err *err);
/* Writes sequence i's bases at d_out[offsets[i] .. offsets[i+1]) (the layout encode_batch read). */
int bitnuc_decode_batch_dev(bitnuc_ctx *ctx, const uint64_t *d_words, const uint64_t *d_word_offsets, const uint64_t *d_offsets, size_t count, size_t total_words, uint8_t *d_out, bitnuc_err *err);
/* Host-pointer forms (synchronous).  encode: out must hold sum ceil(len_i/32) words
 * (<= (offsets[count]-offsets[0])/32 + count); word_offsets (count+1 entries) is an output.
 * offsets that decrease -> INVALID_RANGE{value = index of the offending entry}; decode: a word_offsets
 * table that is not the one encode_batch produces for these offsets -> INVALID_RANGE likewise (the
 * _dev forms trust their tables: they are the caller's device memory). */
int bitnuc_encode_batch(bitnuc_ctx *ctx, const uint8_t *seq, const uint64_t *offsets, size_t count, uint64_t *out, size_t out_cap_words, uint64_t *word_offsets, size_t *n_words, bitnuc_err *err);
int bitnuc_decode_batch(bitnuc_ctx *ctx, const uint64_t *words, const uint64_t *word_offsets, const uint64_t *offsets, size_t count, uint8_t *out, bitnuc_err *err);

/* Layout plan: everything about a ragged batch that depends only on its offsets table, computed once and used by
 * every encode / decode of that layout (a layout is used at least twice: encode now, decode later).  The plan holds
 * the word offsets, one byte offset per 64-word tile and one pad byte per word; with it a lane finds its word's bytes
 * with one byte load and a prefix sum -- no offsets window, no search, no per-call pre-kernel -- and the ragged
 * kernels run at the speed of the fixed-length ones.  _build_dev reads d_offsets (count+1 non-decreasing entries,
 * device memory) once, is synchronous and may be called again on the same plan for the next batch (memory is reused).
 * encode / decode take the buffers the table-driven entry points take: sequence i's bases at d_seq + offsets[i], its
 * words at d_out + word_offsets[i].  Same words, same InvalidBase rule (first invalid byte in buffer order). */
typedef struct bitnuc_batch_plan bitnuc_batch_plan;
int bitnuc_batch_plan_create(bitnuc_ctx *ctx, bitnuc_batch_plan **out, bitnuc_err *err);
int bitnuc_batch_plan_build_dev(bitnuc_ctx *ctx, bitnuc_batch_plan *plan, const uint64_t *d_offsets, size_t count, size_t *total_words, bitnuc_err *err);
void bitnuc_batch_plan_destroy(bitnuc_batch_plan *plan);
size_t bitnuc_batch_plan_total_words(const bitnuc_batch_plan *plan);
size_t bitnuc_batch_plan_count(const bitnuc_batch_plan *plan);
const uint64_t *bitnuc_batch_plan_word_offsets_dev(const bitnuc_batch_plan *plan); /* count+1 entries, device memory owned by the plan */
int bitnuc_encode_batch_plan_dev(bitnuc_ctx *ctx, const bitnuc_batch_plan *plan, const uint8_t *d_seq, uint64_t *d_out, bitnuc_err *err);
int bitnuc_decode_batch_plan_dev(bitnuc_ctx *ctx, const bitnuc_batch_plan *plan, const uint64_t *d_words, uint8_t *d_out, bitnuc_err *err);

/* Fixed-length reads (the common sequencing layout): `count` reads of `read_len` bases, read r
 * at byte r*stride (stride >= read_len; stride == read_len: back to back; stride == read_len+1:
 * newline-separated, ...).  Read r's ceil(read_len/32) words are out[r*wpr .. (r+1)*wpr), its
 * last word zero-padded high -- the same words as `encode(read_r)` per read.  Separator bytes
 * are never examined.  No offsets tables and no lookup: the fastest batch form. */
int bitnuc_encode_fixed_dev(bitnuc_ctx *ctx, const uint8_t *d_seq, size_t read_len, size_t stride, size_t count, uint64_t *d_out, bitnuc_err *err);
/* Inverse: read r's bases are written at d_out[r*stride .. r*stride + read_len); bytes between
 * reads are left untouched. */
int bitnuc_decode_fixed_dev(bitnuc_ctx *ctx, const uint64_t *d_words, size_t read_len, size_t stride, size_t count, uint8_t *d_out, bitnuc_err *err);
int bitnuc_encode_fixed(bitnuc_ctx *ctx, const uint8_t *seq, size_t read_len, size_t stride, size_t count, uint64_t *out, bitnuc_err *err);
int bitnuc_decode_fixed(bitnuc_ctx *ctx, const uint64_t *words, size_t read_len, size_t stride, size_t count, uint8_t *out, bitnuc_err *err);

/* ---- best match per read of a fixed-length batch (demultiplexing: which of Q barcodes / adapters / primers a read carries, where, and
 * with how many mismatches) ----
 * For every read r: best_dist[r] = the minimum over q < n_queries and 0 <= i <= read_len - k of hdist_scalar(as_2bit(read_r[i .. i+k]),
 * queries[q], k) -- only windows that lie wholly inside the read; a window never crosses into the next read --, ties by the smallest q, then the
 * smallest i; best_query[r] and best_pos[r] are that q and i.  Query bits above 2k are ignored.  Deterministic.  Exactly [0, count) of each output is
 * written; best_dist may have any byte offset.  A read without a window, or no queries (k == 0, read_len < k, n_queries == 0): UINT32_MAX,
 * UINT32_MAX, 0xFF.
 * Input.  ASCII: read r is reads[r*read_len .. (r+1)*read_len), back to back, at any byte alignment, either case.  Reads with separators between them
 * (newline-separated, ...) go through bitnuc_encode_fixed_dev, which skips the separators, and then the packed form.  Packed: what encode_fixed
 * writes -- read r's wpr = ceil(read_len/32) words at words[r*wpr ..], 8-byte aligned; the bits above 2*read_len in a read's last word are ignored.
 * As decode_fixed, the call trusts that count*wpr words are present.
 * Checks, in this order: (1) ctx NULL -> UNSUPPORTED (the host forms accept NULL below the host cutoff); (2) k > 32 -> SEQUENCE_TOO_LONG(k);
 * (3) read_len >= 2^32 - 1, or count*read_len or count*wpr*32 not below 2^58 -> UNSUPPORTED (value = read_len); (4) n_queries > BITNUC_MAX_QUERIES
 * -> UNSUPPORTED (value = n_queries); (5) count == 0 -> OK, nothing written; (6) an output NULL, best_query / best_pos not 4-byte aligned, queries
 * NULL with n_queries > 0 or not 8-byte aligned -> UNSUPPORTED; (7) no windows -> OK with the fill above in every read, nothing read or validated;
 * (8) reads NULL, or words NULL or not 8-byte aligned -> UNSUPPORTED.
 * ASCII: a non-ACGT byte -> INVALID_BASE with the first invalid byte in buffer order (index = its byte offset in reads); the _async form latches
 * it once per call for bitnuc_ctx_sync(), the outputs are then unspecified.
 * The _async forms have the _dev contract (device pointers for everything, the context's stream, no host synchronisation but the growth of context
 * scratch) and can be captured into a hipGraph after a warm-up with the same or larger (count, n_queries).  The host forms judge
 * windows x n_queries against the host cutoff; above it they run through the context in chunks of whole reads. */
int bitnuc_reads_hdist_best_async(bitnuc_ctx *ctx, const uint8_t *d_reads, size_t read_len, size_t count, size_t k, const uint64_t *d_queries, size_t n_queries,
                                  uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist, bitnuc_err *err);
int bitnuc_reads_hdist_best_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, size_t read_len, size_t count, size_t k, const uint64_t *d_queries,
                                         size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist, bitnuc_err *err);
int bitnuc_reads_hdist_best(bitnuc_ctx *ctx, const uint8_t *reads, size_t read_len, size_t count, size_t k, const uint64_t *queries, size_t n_queries,
                            uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, bitnuc_err *err);
int bitnuc_reads_hdist_best_packed(bitnuc_ctx *ctx, const uint64_t *words, size_t read_len, size_t count, size_t k, const uint64_t *queries, size_t n_queries,
                                   uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, bitnuc_err *err);

/* ---- best match AND runner-up per read of a fixed-length batch (ambiguous barcodes: a read is assigned only if its best barcode is close enough and
 * no OTHER barcode is nearly as close) -- the twins of the block above with three more outputs ----
 * Results.  best_query / best_pos / best_dist are exactly what bitnuc_reads_hdist_best* writes, byte for byte.  second_*[r] is the lexicographically
 * smallest (distance, query, offset) over all queries q != best_query[r] and all windows wholly inside read r: ties by the smallest q, then the
 * smallest i.  A second window of the winning query is never the runner-up.  Two equal entries of the query list are two queries: the first of them
 * wins and the second is then the runner-up, at the same distance (and the same offset).  Deterministic.  Exactly [0, count) of each of the six
 * outputs is written; the two dist arrays may have any byte offset.
 * Fills (UINT32_MAX, UINT32_MAX, 0xFF).  No window in the read, or no queries (k == 0, read_len < k, n_queries == 0): all six outputs.
 * n_queries == 1: the second_* triple only; the best triple is real.
 * Input layouts, alignment, either-case ASCII, pad bits and the trust in count*wpr words: those of bitnuc_reads_hdist_best*, word for word.
 * Checks, in the order of bitnuc_reads_hdist_best*; check (6) covers all six outputs: any of them NULL, or best_query / best_pos / second_query /
 * second_pos not 4-byte aligned -> UNSUPPORTED.  Nothing is written on an argument error.
 * ASCII: a non-ACGT byte -> INVALID_BASE with the first invalid byte in buffer order; the _async form latches it once per call for bitnuc_ctx_sync()
 * (one call leaves nothing for a second sync), the outputs are then unspecified; the host form below the cutoff leaves all six outputs untouched.
 * The _async forms have the _dev contract (device pointers for everything, the context's stream, no host synchronisation but the growth of context
 * scratch) and can be captured into a hipGraph after a warm-up of THIS call with the same or larger (count, n_queries); the reads and the queries are
 * read at every replay.  The host forms are synchronous and judge windows x n_queries against the host cutoff exactly as bitnuc_reads_hdist_best
 * does: below it they run on the host (ctx may be NULL), above it through the context in chunks of whole reads, of the twins' sizes; INVALID_BASE
 * indices stay absolute.
 * Cost: two passes over the reads in one call (the best match's kernels, then their exclusion form that leaves out each read's winning query, then
 * one kernel for the six outputs), none with one query.  Measured against bitnuc_reads_hdist_best*_async on the same data (6,666,667 x 150-base
 * reads, k = 31, one MI355X; profiles/r14_reads_best2.json): 2.02 - 2.03 x its time at 8, 64 and 512 queries, 1.05 x at one.
 * The pattern twins: bitnuc_reads_pattern_best2* below.  Out of scope: the ragged twins (*_best_batch*), a per-read exclusion list as an argument, more than two ranks. */
int bitnuc_reads_hdist_best2_async(bitnuc_ctx *ctx, const uint8_t *d_reads, size_t read_len, size_t count, size_t k, const uint64_t *d_queries, size_t n_queries,
                                   uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist, uint32_t *d_second_query, uint32_t *d_second_pos,
                                   uint8_t *d_second_dist, bitnuc_err *err);
int bitnuc_reads_hdist_best2_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, size_t read_len, size_t count, size_t k, const uint64_t *d_queries,
                                          size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist, uint32_t *d_second_query,
                                          uint32_t *d_second_pos, uint8_t *d_second_dist, bitnuc_err *err);
int bitnuc_reads_hdist_best2(bitnuc_ctx *ctx, const uint8_t *reads, size_t read_len, size_t count, size_t k, const uint64_t *queries, size_t n_queries,
                             uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_pos, uint8_t *second_dist,
                             bitnuc_err *err);
int bitnuc_reads_hdist_best2_packed(bitnuc_ctx *ctx, const uint64_t *words, size_t read_len, size_t count, size_t k, const uint64_t *queries, size_t n_queries,
                                    uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_pos,
                                    uint8_t *second_dist, bitnuc_err *err);

/* ---- ANCHORED best match and runner-up per read of a fixed-length batch (a barcode, index or adapter at a known place: offset 0, 0..3 behind staggered
 * spacers, the last k bases) -- the best2 twins above restricted to an offset range ----
 * Windows.  The admissible windows of read r are the offsets i with pos_lo <= i <= hi_eff, hi_eff = min(pos_hi, read_len - k).  pos_hi = SIZE_MAX: to the
 * end of the read; a 3' anchor with slack w: pos_lo = read_len - k - w, pos_hi = SIZE_MAX.  An empty range (pos_lo > hi_eff, k == 0, read_len < k,
 * n_queries == 0) has no window: all written outputs get the fill (UINT32_MAX, UINT32_MAX, 0xFF).
 * Span.  span = hi_eff - pos_lo + k is the number of bases of each read the call looks at.  span > BITNUC_ANCHOR_MAX_SPAN -> UNSUPPORTED (err.value =
 * span); wider searches are what bitnuc_reads_hdist_best2* is for.
 * The span is judged on (read_len, k, pos_lo, pos_hi) alone: a range wider than that is UNSUPPORTED with n_queries == 0 as well, although such a call
 * would write only fills.
 * Results.  best_*[r] is the lexicographically smallest (distance, query, offset) over all queries and the admissible windows; second_*[r] the smallest
 * over the queries other than best_query[r], with the semantics of bitnuc_reads_hdist_best2* word for word: another window of the winner is never the
 * runner-up, an equal duplicate query at a higher index is (at the same distance and offset), one query gives the fill in the second triple.  best_pos /
 * second_pos are offsets in the read, not relative to pos_lo.  Deterministic.  Exactly [0, count) of each output is written; the dist arrays may have
 * any byte offset.
 * Second triple.  second_query, second_pos and second_dist may ALL be NULL: only the best triple is computed and written.  One or two of them NULL ->
 * UNSUPPORTED.
 * Identity.  With pos_lo = 0, pos_hi = SIZE_MAX and read_len <= 64 all six outputs equal bitnuc_reads_hdist_best2*'s byte for byte.
 * Input layouts, alignment freedom, either-case ASCII and ignored pad bits: those of bitnuc_reads_hdist_best*.  Checks, in order: (1) ctx (_async forms,
 * and the host forms above the cutoff), (2) k > 32 -> SEQUENCE_TOO_LONG, (3) read_len / count limits as bitnuc_reads_hdist_best*, (4) n_queries >
 * BITNUC_MAX_QUERIES -> UNSUPPORTED (value = n_queries), (5) span > BITNUC_ANCHOR_MAX_SPAN -> UNSUPPORTED (value = span), (6) count == 0 -> OK, nothing
 * written, (7) best_* NULL or best_query / best_pos not 4-byte aligned, queries NULL with n_queries > 0 or not 8-byte aligned, the second triple partly
 * NULL or second_query / second_pos not 4-byte aligned -> UNSUPPORTED, (8) with a window: reads / words NULL (words not 8-byte aligned) -> UNSUPPORTED.
 * Nothing is written on an argument error.
 * Validation -- the one deliberate difference.  Only the span bytes [pos_lo, hi_eff + k) of each read are read and validated; bytes outside are never
 * examined (as separators are not by bitnuc_encode_fixed).  The first invalid byte in buffer order among the span bytes -> INVALID_BASE with its absolute
 * index.  The _async forms latch it once per call for bitnuc_ctx_sync(), the outputs are then unspecified; the host forms below the cutoff leave the
 * outputs untouched.  A call with no window reads and validates nothing.  (The ASCII kernel loads aligned 4-byte words: at most 3 bytes before and after
 * a span are touched, never examined.)
 * The _async forms have the _dev contract (device pointers for everything, the context's stream, no host synchronisation but the growth of context
 * scratch) and can be captured into a hipGraph after a warm-up of THIS call with the same or larger (count, n_queries).  Context scratch: 256 bytes per
 * query; no per-read or per-(query, offset) arrays -- one kernel writes the outputs itself.  The host forms are synchronous and judge count x offsets x
 * n_queries against the host cutoff: below it they run on the host (ctx may be NULL), above it through the context in chunks of whole reads, of the best2
 * forms' sizes; INVALID_BASE indices stay absolute.
 * Cost: one pass, ceil(span / 16) matrix instructions per (32 reads, 32 (query, offset) rows, offsets rounded up to a power of two); the runner-up comes
 * with it.   Measured on 6,666,667 x 150-base reads, one MI355X
 * (profiles/r15_reads_anchored.json), ASCII / packed with the second triple: k = 16, four offsets: 0.28 / 0.20 ms at 1 query, 0.27 / 0.19 at 8, 0.56 /
 * 0.46 at 64, 2.8 / 2.6 at 512; one offset: 0.25 / 0.17, 0.25 / 0.17, 0.27 / 0.20, 0.90 / 0.77 ms; 0.003 - 0.84 x the time of a copy of the spans plus
 * bitnuc_reads_hdist_best2*_async on it.
 * The ragged twins: bitnuc_reads_hdist_anchored_batch* below; the pattern (IUPAC) twins: bitnuc_reads_pattern_anchored*.  Out of scope: indels (every window is compared base against base; the
 * edit-distance form is bitnuc_reads_edist_anchored* below), a per-read offset table, spans above 64 bases, reverse-complement queries (callers add the
 * reverse complements to the query list themselves). */
#define BITNUC_ANCHOR_MAX_SPAN 64
int bitnuc_reads_hdist_anchored_async(bitnuc_ctx *ctx, const uint8_t *d_reads, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi,
                                      const uint64_t *d_queries, size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist,
                                      uint32_t *d_second_query, uint32_t *d_second_pos, uint8_t *d_second_dist, bitnuc_err *err);
int bitnuc_reads_hdist_anchored_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi,
                                             const uint64_t *d_queries, size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist,
                                             uint32_t *d_second_query, uint32_t *d_second_pos, uint8_t *d_second_dist, bitnuc_err *err);
int bitnuc_reads_hdist_anchored(bitnuc_ctx *ctx, const uint8_t *reads, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi, const uint64_t *queries,
                                size_t n_queries, uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_pos,
                                uint8_t *second_dist, bitnuc_err *err);
int bitnuc_reads_hdist_anchored_packed(bitnuc_ctx *ctx, const uint64_t *words, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi,
                                       const uint64_t *queries, size_t n_queries, uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, uint32_t *second_query,
                                       uint32_t *second_pos, uint8_t *second_dist, bitnuc_err *err);

/* ---- ANCHORED best match and runner-up per read of a RAGGED batch (a barcode or adapter in the first or the last k (+ slack) bases of trimmed, merged or
 * long reads): the twins of the block above for the layout of bitnuc_reads_hdist_best_batch*, with an anchor that follows each read's own end ----
 * Layout: that of bitnuc_reads_hdist_best_batch* (below), word for word: read r is seq[offsets[r] .. offsets[r+1]), packed its words start at
 * words[word_offsets[r]]; bits above a read's last base are ignored; a zero-length read has no words.
 * Windows.  len_r is the read's length, last_r = len_r - k.  BITNUC_ANCHOR_START: the admissible offsets are the i with pos_lo <= i <= min(pos_hi,
 * last_r).  BITNUC_ANCHOR_END: offsets are measured from the read's end: e = last_r - i is the number of bases behind the window, admissible are the i
 * with pos_lo <= e <= pos_hi and i >= 0 -- END, 0, 0 is the last k bases, END, 0, 3 the last k bases with three bases of slack.  In both modes best_pos /
 * second_pos are offsets from the read's start.  Ties: the smallest query, then the smallest i.
 * Span.  offsets = pos_hi - pos_lo + 1 and span = offsets + k - 1, judged on the arguments alone (computed without overflow; a value that does not fit is
 * reported as SIZE_MAX).  span > BITNUC_ANCHOR_MAX_SPAN -> UNSUPPORTED (err.value = span): pos_hi = SIZE_MAX does NOT mean "to the end of the read" here
 * -- the END anchor serves that purpose.  pos_hi < pos_lo is an empty range: every read gets the fill.
 * Results: the six outputs of bitnuc_reads_hdist_anchored*, word for word (another window of the winner is never the runner-up, an equal duplicate query
 * at a higher index is, one query gives the fill in the second triple).  A read without an admissible window (len_r < k, too short for pos_lo, empty)
 * gets the fill (UINT32_MAX, UINT32_MAX, 0xFF) in all six.  The second triple may be ALL NULL; one or two of its pointers NULL -> UNSUPPORTED.  Exactly
 * [0, count) of each output is written; the dist arrays may have any byte offset.  On a batch of equal lengths L, START (lo, hi) equals
 * bitnuc_reads_hdist_anchored*(read_len = L, lo, hi) byte for byte, and END (e_lo, e_hi) equals it with pos_lo = L - k - e_hi, pos_hi = L - k - e_lo
 * (L - k >= e_hi).
 * Validation follows the fixed anchored form, not best_batch: of a read with n_r admissible offsets only the n_r + k - 1 span bytes are read and
 * validated, never a byte of another read or behind the batch; a read without a window is not validated at all.  The first invalid span byte in buffer
 * order -> INVALID_BASE with its absolute index, latched once per call for bitnuc_ctx_sync() by the _async forms (outputs then unspecified); the host
 * forms below the cutoff leave the outputs untouched.  (The ASCII kernel loads aligned 4-byte words that hold a span byte: at most 3 bytes before and
 * after a span are touched, never examined.)
 * Checks, in order: (1) ctx NULL (_async forms always, host forms above the cutoff) -> UNSUPPORTED; (2) k > 32 -> SEQUENCE_TOO_LONG; (3) _async forms:
 * total_bases, or 32*total_words, not below 2^58 -> UNSUPPORTED (value = that total); (4) n_queries > BITNUC_MAX_QUERIES -> UNSUPPORTED (value =
 * n_queries); (5) anchor not 0 or 1 -> UNSUPPORTED (value = anchor), then span > BITNUC_ANCHOR_MAX_SPAN -> UNSUPPORTED (value = span); (6) count == 0 ->
 * OK, nothing written; (7) outputs and queries as bitnuc_reads_hdist_anchored*, the tables as bitnuc_reads_hdist_best_batch* (NULL or not 8-byte aligned
 * -> UNSUPPORTED); (8) host forms only: the tables' faults exactly as bitnuc_reads_hdist_best_batch reports them; (9) no window possible from the
 * host-known arguments (k == 0, n_queries == 0, an empty range, fewer than k + pos_lo bases in the whole batch) -> OK with the fill, nothing is read;
 * (10) seq NULL, or words NULL or not 8-byte aligned -> UNSUPPORTED.  Nothing is written on an argument error.
 * The _async forms TRUST their tables (as bitnuc_reads_hdist_best_batch*_async), have the _dev contract, use the context's stream, do no host
 * synchronisation but the growth of context scratch (256 bytes per query, as the fixed form) and can be captured into a hipGraph after a warm-up; the
 * tables are read on the device at every replay, so a replay after the lengths changed (same count and totals) gives the new answers.  The host forms
 * judge count x offsets x n_queries (saturated) against the host cutoff: below it they run on the host (ctx may be NULL), above it through the context
 * in chunks of whole reads with rebased tables; INVALID_BASE indices stay absolute.
 * Cost: the fixed form's kernel under a ragged layout policy -- every lane loads its own read's two table entries, start values of the accumulators
 * carry each read's own number of admissible offsets, the tile loop is the fixed form's.  Measured on 6,666,667 reads of 100 .. 200 bases (10^9 bases), one
 * MI355X (profiles/r16_reads_anchored_batch.json), ASCII / packed, all six outputs, END anchor: k = 16, one offset: 0.30 / 0.26 ms at 1 and at 8 queries,
 * 0.32 / 0.28 at 64, 0.95 / 0.91 at 512; four offsets: 0.33 / 0.29, 0.30 / 0.27, 0.62 / 0.58, 2.90 / 2.88 ms; 0.17 - 0.83 x the time of a device gather of the
 * spans into a compact batch plus bitnuc_reads_hdist_anchored*_async on it, at every measured point.  On equal-length reads the fixed form above gives the
 * same answers in less time (this form takes 1.02 - 1.45 x of it, 0.03 - 0.27 ms more): a fixed-length batch belongs there.
 * The pattern (IUPAC) twins: bitnuc_reads_pattern_anchored_batch* below.  Out of scope: a per-read offset table as an argument, spans above 64 bases,
 * reverse-complement queries, a whole-read ragged best2. */
#define BITNUC_ANCHOR_START 0
#define BITNUC_ANCHOR_END 1
int bitnuc_reads_hdist_anchored_batch_async(bitnuc_ctx *ctx, const uint8_t *d_seq, const uint64_t *d_offsets, size_t count, size_t total_bases, size_t k, int anchor,
                                            size_t pos_lo, size_t pos_hi, const uint64_t *d_queries, size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_pos,
                                            uint8_t *d_best_dist, uint32_t *d_second_query, uint32_t *d_second_pos, uint8_t *d_second_dist, bitnuc_err *err);
int bitnuc_reads_hdist_anchored_batch_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, const uint64_t *d_word_offsets, const uint64_t *d_offsets, size_t count,
                                                   size_t total_words, size_t k, int anchor, size_t pos_lo, size_t pos_hi, const uint64_t *d_queries, size_t n_queries,
                                                   uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist, uint32_t *d_second_query,
                                                   uint32_t *d_second_pos, uint8_t *d_second_dist, bitnuc_err *err);
int bitnuc_reads_hdist_anchored_batch(bitnuc_ctx *ctx, const uint8_t *seq, const uint64_t *offsets, size_t count, size_t k, int anchor, size_t pos_lo, size_t pos_hi,
                                      const uint64_t *queries, size_t n_queries, uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, uint32_t *second_query,
                                      uint32_t *second_pos, uint8_t *second_dist, bitnuc_err *err);
int bitnuc_reads_hdist_anchored_batch_packed(bitnuc_ctx *ctx, const uint64_t *words, const uint64_t *word_offsets, const uint64_t *offsets, size_t count, size_t k,
                                             int anchor, size_t pos_lo, size_t pos_hi, const uint64_t *queries, size_t n_queries, uint32_t *best_query,
                                             uint32_t *best_pos, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_pos, uint8_t *second_dist, bitnuc_err *err);

/* ---- best match per read of a RAGGED batch (reads after trimming, merged pairs, amplicons, long reads, contigs): the twins of the block above for
 * the layout the ragged batch entry points read and write ----
 * Layout.  Read r is seq[offsets[r] .. offsets[r+1]) -- `offsets` has count + 1 non-decreasing entries and offsets[0] == 0 (a batch cut out of a larger
 * table passes a rebased table) --, and packed its ceil(len_r/32) words start at words[word_offsets[r]]: exactly what bitnuc_encode_batch* writes.  The
 * bits above a read's last base are ignored; a zero-length read has no words.  total_bases == offsets[count] and total_words == word_offsets[count]:
 * the caller knows both, as for bitnuc_encode_batch_dev.
 * Result.  For every read r the minimum over q < n_queries and 0 <= i <= len_r - k of hdist_scalar(as_2bit(read_r[i .. i+k]), queries[q], k), ties by
 * the smallest q, then the smallest i; a window never crosses into the next read; query bits above 2k are ignored; deterministic.  Exactly [0, count) of
 * each output is written; best_dist may have any byte offset.  A read without a window (len_r < k, empty), and every read when k == 0 or
 * n_queries == 0: UINT32_MAX, UINT32_MAX, 0xFF.  On a batch whose reads all have length L the results equal bitnuc_reads_hdist_best* with
 * read_len = L, byte for byte.
 * Checks, in this order: (1) ctx NULL -> UNSUPPORTED (the host forms accept NULL below the host cutoff); (2) k > 32 -> SEQUENCE_TOO_LONG(k);
 * (3) total_bases, or 32*total_words, not below 2^58 -> UNSUPPORTED (value = that total; the host forms have no such argument and bound their tables'
 * totals at the end of check 7); (4) n_queries > BITNUC_MAX_QUERIES -> UNSUPPORTED (value = n_queries); (5) count == 0 -> OK, nothing written; (6) an
 * output NULL, best_query / best_pos not 4-byte aligned, queries NULL with n_queries > 0 or not 8-byte aligned, an offsets table NULL or not 8-byte
 * aligned -> UNSUPPORTED; (7) host forms only, the tables: decreasing offsets -> INVALID_RANGE exactly as bitnuc_encode_batch reports it,
 * offsets[0] != 0 -> INVALID_RANGE (value 0), a word_offsets table that is not the one encode_batch produces for these offsets -> INVALID_RANGE as
 * bitnuc_decode_batch, a read of 2^32 - 1 bases or more -> UNSUPPORTED (value = its length); (8) no window is possible from the host-known arguments
 * (k == 0, n_queries == 0, total_bases < k; packed _async: total_words == 0) -> OK with the fill above in every read, nothing read or validated;
 * (9) seq NULL, or words NULL or not 8-byte aligned -> UNSUPPORTED.
 * The _async forms TRUST their tables, as the _dev batch forms do: the caller promises tables as above (non-decreasing from 0, word_offsets the table
 * encode_batch produces for offsets, the totals their last entries) and reads below 2^32 - 1 bases; anything else is undefined.
 * ASCII: every byte of seq[0 .. total_bases) is validated, whether or not its read is long enough to hold a window; a non-ACGT byte (either case is
 * valid) -> INVALID_BASE with the first invalid byte in buffer order (index = its offset in seq), latched once per call for bitnuc_ctx_sync(), the
 * outputs are then unspecified; the host forms below the cutoff leave the outputs untouched.
 * The _async forms have the _dev contract (device pointers for everything, the context's stream, no host synchronisation but the growth of context
 * scratch) and can be captured into a hipGraph after a warm-up with the same or larger (count, n_queries); the tables are read on the device at every
 * replay, so a replay after the lengths changed (same count and totals) gives the new answers.  d_seq may have any alignment; d_words must be 8-byte
 * aligned (0 or 8 mod 16).  The host forms judge the sum over the reads of max(0, len_r - k + 1), times n_queries, saturated, against the host cutoff;
 * above it they run through the context in chunks of whole reads (the longest run of whole reads within the chunk budget, at least one), each with
 * its rebased tables; INVALID_BASE indices stay absolute.
 * Speed: packed words run on the matrix cores throughout; ASCII wherever 1024 consecutive windows touch no read of 1 .. 31 bases (those windows take
 * an exact one-window-per-thread path with the same result, as does a stretch of 4096 windows that touches more than 132 reads, empty ones included). */
int bitnuc_reads_hdist_best_batch_async(bitnuc_ctx *ctx, const uint8_t *d_seq, const uint64_t *d_offsets, size_t count, size_t total_bases, size_t k,
                                        const uint64_t *d_queries, size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist, bitnuc_err *err);
int bitnuc_reads_hdist_best_batch_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, const uint64_t *d_word_offsets, const uint64_t *d_offsets, size_t count,
                                               size_t total_words, size_t k, const uint64_t *d_queries, size_t n_queries,
                                               uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist, bitnuc_err *err);
int bitnuc_reads_hdist_best_batch(bitnuc_ctx *ctx, const uint8_t *seq, const uint64_t *offsets, size_t count, size_t k, const uint64_t *queries, size_t n_queries,
                                  uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, bitnuc_err *err);
int bitnuc_reads_hdist_best_batch_packed(bitnuc_ctx *ctx, const uint64_t *words, const uint64_t *word_offsets, const uint64_t *offsets, size_t count, size_t k,
                                         const uint64_t *queries, size_t n_queries, uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, bitnuc_err *err);

/* ---- PATTERN (IUPAC) queries for the per-read matchers: inline barcodes with N (UMI) positions, degenerate primers (R Y M K W ...), index reads with a
 * masked cycle, guide + NGG -- one pattern per barcode / primer instead of all its exact instances ----
 * pdist(window) = #{ i < k : window[i] not in S_i } for a pattern with sets S_i: bitnuc_pattern's definition, unchanged (bits of allow[c] at positions
 * >= k are ignored; an empty set mismatches every base and is legal; an all-N pattern has distance 0 at every window).
 * Each of the twenty entry points below is its exact twin's contract WORD FOR WORD with three substitutions: `const bitnuc_pattern *patterns`
 * (n_queries of them) stands where `const uint64_t *queries` stood; "patterns NULL with n_queries > 0, or not 4-byte aligned" where "queries NULL ... or
 * not 8-byte aligned" stood; pdist where hdist_scalar stood.  Everything else is the twin's: the checks in the same order, the same fills (UINT32_MAX,
 * UINT32_MAX, 0xFF), the same BITNUC_MAX_QUERIES, ties by the smallest query index and then the smallest offset, the same validation of the READS (the
 * sets are on the query's side only: an N in a read is still INVALID_BASE), the same chunking of the host forms above the host cutoff, the same context
 * scratch and hipGraph contract of the _async forms (d_patterns is read on the device at every replay).  Runner-up: two equal patterns are two
 * queries (the one at the higher index is the runner-up at the same distance); a second window of the winner never is.  A list of singleton patterns
 * (bitnuc_pattern_from_2bit) gives the exact twin's outputs byte for byte.
 * Cost: the twins' kernels; only the per-query tables are built from 16 instead of 8 bytes per query (profiles/r17_reads_pattern.json). */
/* the twins of bitnuc_reads_hdist_best* */
int bitnuc_reads_pattern_best_async(bitnuc_ctx *ctx, const uint8_t *d_reads, size_t read_len, size_t count, size_t k, const bitnuc_pattern *d_patterns, size_t n_queries,
                                    uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist, bitnuc_err *err);
int bitnuc_reads_pattern_best_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, size_t read_len, size_t count, size_t k, const bitnuc_pattern *d_patterns,
                                           size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist, bitnuc_err *err);
int bitnuc_reads_pattern_best(bitnuc_ctx *ctx, const uint8_t *reads, size_t read_len, size_t count, size_t k, const bitnuc_pattern *patterns, size_t n_queries,
                              uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, bitnuc_err *err);
int bitnuc_reads_pattern_best_packed(bitnuc_ctx *ctx, const uint64_t *words, size_t read_len, size_t count, size_t k, const bitnuc_pattern *patterns, size_t n_queries,
                                     uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, bitnuc_err *err);
/* the twins of bitnuc_reads_hdist_best2* */
int bitnuc_reads_pattern_best2_async(bitnuc_ctx *ctx, const uint8_t *d_reads, size_t read_len, size_t count, size_t k, const bitnuc_pattern *d_patterns, size_t n_queries,
                                     uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist, uint32_t *d_second_query, uint32_t *d_second_pos,
                                     uint8_t *d_second_dist, bitnuc_err *err);
int bitnuc_reads_pattern_best2_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, size_t read_len, size_t count, size_t k, const bitnuc_pattern *d_patterns,
                                            size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist, uint32_t *d_second_query,
                                            uint32_t *d_second_pos, uint8_t *d_second_dist, bitnuc_err *err);
int bitnuc_reads_pattern_best2(bitnuc_ctx *ctx, const uint8_t *reads, size_t read_len, size_t count, size_t k, const bitnuc_pattern *patterns, size_t n_queries,
                               uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_pos, uint8_t *second_dist,
                               bitnuc_err *err);
int bitnuc_reads_pattern_best2_packed(bitnuc_ctx *ctx, const uint64_t *words, size_t read_len, size_t count, size_t k, const bitnuc_pattern *patterns, size_t n_queries,
                                      uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_pos,
                                      uint8_t *second_dist, bitnuc_err *err);
/* the twins of bitnuc_reads_hdist_anchored*: the same matrix-core GEMM; a pattern's table entry holds -1.0 in every channel of its position's set */
int bitnuc_reads_pattern_anchored_async(bitnuc_ctx *ctx, const uint8_t *d_reads, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi,
                                        const bitnuc_pattern *d_patterns, size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist,
                                        uint32_t *d_second_query, uint32_t *d_second_pos, uint8_t *d_second_dist, bitnuc_err *err);
int bitnuc_reads_pattern_anchored_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi,
                                               const bitnuc_pattern *d_patterns, size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist,
                                               uint32_t *d_second_query, uint32_t *d_second_pos, uint8_t *d_second_dist, bitnuc_err *err);
int bitnuc_reads_pattern_anchored(bitnuc_ctx *ctx, const uint8_t *reads, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi,
                                  const bitnuc_pattern *patterns, size_t n_queries, uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, uint32_t *second_query,
                                  uint32_t *second_pos, uint8_t *second_dist, bitnuc_err *err);
int bitnuc_reads_pattern_anchored_packed(bitnuc_ctx *ctx, const uint64_t *words, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi,
                                         const bitnuc_pattern *patterns, size_t n_queries, uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist,
                                         uint32_t *second_query, uint32_t *second_pos, uint8_t *second_dist, bitnuc_err *err);
/* the twins of bitnuc_reads_hdist_anchored_batch* */
int bitnuc_reads_pattern_anchored_batch_async(bitnuc_ctx *ctx, const uint8_t *d_seq, const uint64_t *d_offsets, size_t count, size_t total_bases, size_t k, int anchor,
                                              size_t pos_lo, size_t pos_hi, const bitnuc_pattern *d_patterns, size_t n_queries, uint32_t *d_best_query,
                                              uint32_t *d_best_pos, uint8_t *d_best_dist, uint32_t *d_second_query, uint32_t *d_second_pos, uint8_t *d_second_dist,
                                              bitnuc_err *err);
int bitnuc_reads_pattern_anchored_batch_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, const uint64_t *d_word_offsets, const uint64_t *d_offsets, size_t count,
                                                     size_t total_words, size_t k, int anchor, size_t pos_lo, size_t pos_hi, const bitnuc_pattern *d_patterns,
                                                     size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist, uint32_t *d_second_query,
                                                     uint32_t *d_second_pos, uint8_t *d_second_dist, bitnuc_err *err);
int bitnuc_reads_pattern_anchored_batch(bitnuc_ctx *ctx, const uint8_t *seq, const uint64_t *offsets, size_t count, size_t k, int anchor, size_t pos_lo, size_t pos_hi,
                                        const bitnuc_pattern *patterns, size_t n_queries, uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist,
                                        uint32_t *second_query, uint32_t *second_pos, uint8_t *second_dist, bitnuc_err *err);
int bitnuc_reads_pattern_anchored_batch_packed(bitnuc_ctx *ctx, const uint64_t *words, const uint64_t *word_offsets, const uint64_t *offsets, size_t count, size_t k,
                                               int anchor, size_t pos_lo, size_t pos_hi, const bitnuc_pattern *patterns, size_t n_queries, uint32_t *best_query,
                                               uint32_t *best_pos, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_pos, uint8_t *second_dist,
                                               bitnuc_err *err);
/* the twins of bitnuc_reads_hdist_best_batch* */
int bitnuc_reads_pattern_best_batch_async(bitnuc_ctx *ctx, const uint8_t *d_seq, const uint64_t *d_offsets, size_t count, size_t total_bases, size_t k,
                                          const bitnuc_pattern *d_patterns, size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_pos, uint8_t *d_best_dist,
                                          bitnuc_err *err);
int bitnuc_reads_pattern_best_batch_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, const uint64_t *d_word_offsets, const uint64_t *d_offsets, size_t count,
                                                 size_t total_words, size_t k, const bitnuc_pattern *d_patterns, size_t n_queries, uint32_t *d_best_query,
                                                 uint32_t *d_best_pos, uint8_t *d_best_dist, bitnuc_err *err);
int bitnuc_reads_pattern_best_batch(bitnuc_ctx *ctx, const uint8_t *seq, const uint64_t *offsets, size_t count, size_t k, const bitnuc_pattern *patterns,
                                    size_t n_queries, uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist, bitnuc_err *err);
int bitnuc_reads_pattern_best_batch_packed(bitnuc_ctx *ctx, const uint64_t *words, const uint64_t *word_offsets, const uint64_t *offsets, size_t count, size_t k,
                                           const bitnuc_pattern *patterns, size_t n_queries, uint32_t *best_query, uint32_t *best_pos, uint8_t *best_dist,
                                           bitnuc_err *err);

/* ---- INDEL-TOLERANT anchored best match and runner-up per read of a fixed-length batch (a barcode, adapter or primer with an inserted or deleted base:
 * long-read platforms, synthesised oligos) -- bitnuc_reads_hdist_anchored* with the EDIT (Levenshtein) distance instead of the Hamming distance ----
 * Arguments: those of bitnuc_reads_hdist_anchored* (read_len, count, k, pos_lo, pos_hi, queries, n_queries; ASCII or packed), with best_end / second_end
 * where best_pos / second_pos stood.
 * Span.  hi_eff = min(pos_hi, read_len - k); the span of read r is its bases t_1 .. t_n = read_r[pos_lo .. hi_eff + k), n = hi_eff - pos_lo + k >= k --
 * exactly the bases the Hamming form looks at.  pos_hi = SIZE_MAX: to the end of the read.  An empty range (pos_lo > hi_eff, k == 0, read_len < k,
 * n_queries == 0) has no span: all written outputs get the fill (UINT32_MAX, UINT32_MAX, 0xFF).  n > BITNUC_ANCHOR_MAX_SPAN -> UNSUPPORTED (err.value =
 * n), judged on (read_len, k, pos_lo, pos_hi) alone: with n_queries == 0 as well, although such a call would write only fills.
 * Distance.  For a query q_1 .. q_k: D[0][j] = 0 (0 <= j <= n), D[i][0] = i, D[i][j] = min(D[i-1][j-1] + [t_j does not match q_i], D[i-1][j] + 1,
 * D[i][j-1] + 1).  edist(r, q) = min over 1 <= j <= n of D[k][j]: the Levenshtein distance of the query to the best SUBSTRING of the span, which may
 * start and end anywhere in the span.  end(r, q) = pos_lo + (the smallest such j): an offset in the read, one past the last aligned read base.  "Matches"
 * is equality for an exact query and t_j in S_i for a pattern (bitnuc_reads_pattern_edist_anchored*; an empty set never matches).  edist <= k <= 32, so
 * it fits the uint8_t outputs and never collides with the fill.  The START of the alignment: bitnuc_reads_edist_start* (the family's second stage, below) with (START, pos_lo).
 * Results.  best_query / best_end / best_dist [r] is the lexicographically smallest (edist, query, end) over all queries; second_*[r] the smallest over
 * the queries other than best_query[r]: an equal duplicate query at a higher index is the runner-up (at the same distance and end), one query gives the
 * fill in the second triple.  For equal arguments best_dist here is <= bitnuc_reads_hdist_anchored*'s best_dist: every window is a substring of the
 * span, and the Levenshtein distance is <= the Hamming distance.  Deterministic.  Exactly [0, count) of each output is written; the dist arrays may have
 * any byte offset.
 * Second triple.  second_query, second_end and second_dist may ALL be NULL: only the best triple is computed and written.  One or two of them NULL ->
 * UNSUPPORTED.
 * Input layouts: ASCII reads back to back, read r at reads + r * read_len, any alignment, either case; packed reads of ceil(read_len / 32) 64-bit words
 * each (what bitnuc_encode_fixed writes), 8-byte aligned, base b of a read at bits 2 (b % 32) of its word b / 32, bits above a read's last base ignored.
 * Limits: k <= 32; read_len < 2^32 - 1 and count x 32 ceil(read_len / 32) < 2^58 (UNSUPPORTED, value = read_len); n_queries <= BITNUC_MAX_QUERIES.
 * Checks, in order: (1) ctx (_async forms, and the host forms above the cutoff), (2) k > 32 -> SEQUENCE_TOO_LONG (value = k), (3) the read_len / count
 * limits, (4) n_queries > BITNUC_MAX_QUERIES -> UNSUPPORTED (value = n_queries), (5) n > BITNUC_ANCHOR_MAX_SPAN -> UNSUPPORTED (value = n), (6) count == 0
 * -> OK, nothing written, (7) best_* NULL or best_query / best_end not 4-byte aligned, queries NULL with n_queries > 0 or not 8-byte aligned (patterns:
 * not 4-byte aligned), the second triple partly NULL or second_query / second_end not 4-byte aligned -> UNSUPPORTED, (8) with a span: reads / words NULL
 * (words not 8-byte aligned) -> UNSUPPORTED.  Nothing is written on an argument error.
 * Validation.  Only the span bytes [pos_lo, hi_eff + k) of each read are read and validated; bytes outside are never examined.  The first invalid byte
 * in buffer order among the span bytes -> INVALID_BASE with its absolute index.  The _async forms latch it once per call for bitnuc_ctx_sync() (one call
 * leaves nothing for a second sync), the outputs are then unspecified; the host forms below the cutoff leave the outputs untouched.  A call with no span
 * reads and validates nothing.  (The ASCII kernel loads aligned 4-byte words: at most 3 bytes before and after a span are touched, never examined.)
 * The _async forms have the _dev contract (device pointers for everything, the context's stream, no host synchronisation but the growth of context
 * scratch) and can be captured into a hipGraph after a warm-up of THIS call with the same or larger (count, n_queries); the reads and the queries are
 * read at every replay.  Context scratch: 16 bytes per query; no per-read arrays -- one kernel writes the outputs itself.  The host forms are synchronous
 * and judge count x n x n_queries (saturated) against the host cutoff: below it they run on the host (ctx may be NULL), above it through the context in
 * chunks of whole reads, of the anchored forms' sizes; INVALID_BASE indices stay absolute.
 * Cost: a vector-ALU kernel, one read per lane, n steps of the bit-parallel recurrence (Myers 1999 in Hyyro's form; one 32-bit add is the carry chain)
 * per (read, query), 20 vector instructions a step; no matrix instructions, no LDS, no atomics but the invalid-byte latch.  Measured on 6,666,667 x
 * 150-base reads, one MI355X (profiles/r18_reads_edist.json), ASCII / packed, six outputs, 3' anchor: k = 16, four offsets (n = 19): 0.28 / 0.10 ms at 1
 * query, 0.55 / 0.50 at 8, 4.0 / 3.9 at 64, 31.5 / 30.8 at 512; k = 31, eight offsets (n = 38): 0.39 / 0.17, 1.04 / 0.98, 7.8 / 7.7, 62.3 / 61.7 ms:
 * 0.47 - 1.2 x the time of bitnuc_reads_hdist_anchored*_async on the same arguments at 1 query, 2.0 - 3.5 x at 8, 5.5 - 12.3 x at 64, 7.1 - 18.9 x at 512
 * (another answer: the price of indel tolerance); the pattern twins cost what the exact forms cost.
 * The ragged twins (offsets tables): bitnuc_reads_edist_anchored_batch* below.  The whole-read (unanchored) form, for reads of any length: bitnuc_reads_edist_best* below.  The alignment's start: bitnuc_reads_edist_start* below.  Out of scope:
 * k > 32, anchored spans above 64 bases, affine gaps, reverse-complement queries (callers add the reverse complements to the query list
 * themselves). */
int bitnuc_reads_edist_anchored_async(bitnuc_ctx *ctx, const uint8_t *d_reads, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi,
                                      const uint64_t *d_queries, size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_end, uint8_t *d_best_dist,
                                      uint32_t *d_second_query, uint32_t *d_second_end, uint8_t *d_second_dist, bitnuc_err *err);
int bitnuc_reads_edist_anchored_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi,
                                             const uint64_t *d_queries, size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_end, uint8_t *d_best_dist,
                                             uint32_t *d_second_query, uint32_t *d_second_end, uint8_t *d_second_dist, bitnuc_err *err);
int bitnuc_reads_edist_anchored(bitnuc_ctx *ctx, const uint8_t *reads, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi, const uint64_t *queries,
                                size_t n_queries, uint32_t *best_query, uint32_t *best_end, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_end,
                                uint8_t *second_dist, bitnuc_err *err);
int bitnuc_reads_edist_anchored_packed(bitnuc_ctx *ctx, const uint64_t *words, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi,
                                       const uint64_t *queries, size_t n_queries, uint32_t *best_query, uint32_t *best_end, uint8_t *best_dist, uint32_t *second_query,
                                       uint32_t *second_end, uint8_t *second_dist, bitnuc_err *err);
/* the pattern twins: a set of bases per query position (bitnuc_pattern), t_j matches position i when it is in S_i; everything else as above */
int bitnuc_reads_pattern_edist_anchored_async(bitnuc_ctx *ctx, const uint8_t *d_reads, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi,
                                              const bitnuc_pattern *d_patterns, size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_end, uint8_t *d_best_dist,
                                              uint32_t *d_second_query, uint32_t *d_second_end, uint8_t *d_second_dist, bitnuc_err *err);
int bitnuc_reads_pattern_edist_anchored_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi,
                                                     const bitnuc_pattern *d_patterns, size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_end,
                                                     uint8_t *d_best_dist, uint32_t *d_second_query, uint32_t *d_second_end, uint8_t *d_second_dist, bitnuc_err *err);
int bitnuc_reads_pattern_edist_anchored(bitnuc_ctx *ctx, const uint8_t *reads, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi,
                                        const bitnuc_pattern *patterns, size_t n_queries, uint32_t *best_query, uint32_t *best_end, uint8_t *best_dist,
                                        uint32_t *second_query, uint32_t *second_end, uint8_t *second_dist, bitnuc_err *err);
int bitnuc_reads_pattern_edist_anchored_packed(bitnuc_ctx *ctx, const uint64_t *words, size_t read_len, size_t count, size_t k, size_t pos_lo, size_t pos_hi,
                                               const bitnuc_pattern *patterns, size_t n_queries, uint32_t *best_query, uint32_t *best_end, uint8_t *best_dist,
                                               uint32_t *second_query, uint32_t *second_end, uint8_t *second_dist, bitnuc_err *err);

/* ---- INDEL-TOLERANT anchored best match and runner-up per read of a RAGGED batch (a 3' barcode, adapter or primer with an inserted or deleted base in
 * the last k (+ slack) bases of trimmed or long reads): the layout and window rule of bitnuc_reads_hdist_anchored_batch* with the distance and results
 * of bitnuc_reads_edist_anchored* ----
 * Arguments: exactly those of the corresponding bitnuc_reads_hdist_anchored_batch* / bitnuc_reads_pattern_anchored_batch* function, with best_end /
 * second_end where best_pos / second_pos stood.
 * Layout: that of bitnuc_reads_hdist_anchored_batch*, word for word: `offsets` has count + 1 entries, packed reads start at words[word_offsets[r]], bits
 * above a read's last base are ignored, a zero-length read has no words.
 * Span of read r.  len_r is its length, last_r = len_r - k.  The admissible window offsets are those of the ragged Hamming form: START: pos_lo <= i <=
 * min(pos_hi, last_r); END: pos_lo <= last_r - i <= pos_hi and i >= 0.  With a_r the first admissible offset and n_r their number, the span is
 * read_r[a_r .. a_r + n_r + k - 1): exactly the bases the Hamming form looks at.  A read with n_r == 0 (len_r < k, too short for pos_lo, empty) has no
 * span and gets the fill (UINT32_MAX, UINT32_MAX, 0xFF) in all written outputs.  The widest span, pos_hi - pos_lo + k, is judged on the arguments alone
 * (computed without overflow; a value that does not fit is reported as SIZE_MAX): above BITNUC_ANCHOR_MAX_SPAN -> UNSUPPORTED (err.value = that span).
 * pos_hi = SIZE_MAX does NOT mean "to the end of the read" here -- the END anchor serves that purpose.  pos_hi < pos_lo is an empty range: every read
 * gets the fill.
 * Distance and results: the definition of the bitnuc_reads_edist_anchored* block, applied to each read's own span t_1 .. t_n, n = n_r + k - 1:
 * D[0][j] = 0, so the substring starts and ends anywhere in the span; end = a_r + (the smallest j with the smallest D[k][j]), one past the last aligned
 * base, counted from the read's START in both anchor modes.  The best triple is the lexicographic minimum of (edist, query, end), the second triple the
 * minimum over the other queries (an equal duplicate query at a higher index is the runner-up, one query gives the fill in the second triple).  The
 * second triple's pointers may be ALL NULL; one or two NULL -> UNSUPPORTED.  Exactly [0, count) of each output is written; the dist arrays may have any
 * byte offset.  Deterministic.
 * Identities.  On a batch of equal lengths L, START (lo, hi) equals bitnuc_reads_edist_anchored*(read_len = L, lo, hi) byte for byte, and END (e_lo,
 * e_hi) equals it with pos_lo = L - k - e_hi, pos_hi = L - k - e_lo, provided L - k >= e_hi.  For equal arguments best_dist <= the best_dist of
 * bitnuc_reads_hdist_anchored_batch* on every read.  The pattern forms on singleton patterns (bitnuc_pattern_from_2bit) equal the exact forms byte
 * for byte.
 * Validation.  Of a read with a span only its n_r + k - 1 span bytes are read and validated; a read without a span is neither read nor validated.  The
 * first invalid span byte in buffer order -> INVALID_BASE with its absolute index, latched once per call for bitnuc_ctx_sync() by the _async forms
 * (outputs then unspecified); the host forms below the cutoff leave the outputs untouched.  (The ASCII kernel loads aligned 4-byte words that hold a
 * span byte: at most 3 bytes before and after a span are touched, never examined; a word that holds no span byte is never touched.)
 * Checks, in order: (1) - (10) of the bitnuc_reads_hdist_anchored_batch* block, word for word.  Nothing is written on an argument error.
 * The _async forms TRUST their tables (as bitnuc_reads_hdist_best_batch*_async), have the _dev contract, use the context's stream, do no host
 * synchronisation but the growth of context scratch (16 bytes per query, as the fixed edit-distance form) and can be captured into a hipGraph after a
 * warm-up; the tables, the reads and the queries are read on the device at every replay, so a replay after the lengths changed (same count and totals)
 * gives the new answers.  The host forms judge count x the widest span x n_queries (saturated) against the host cutoff: below it they run on the host
 * (ctx may be NULL), above it through the context in chunks of whole reads with rebased tables; INVALID_BASE indices stay absolute.
 * Cost: the fixed form's kernel under a ragged layout policy -- every lane loads its own read's table entries (one trip ahead) and its own span; the
 * recurrence loop runs, wave-uniformly, over the widest span among the wave's 64 reads, with Eq forced to 0 behind a shorter span (one more vector
 * select per (query, step) and one compare per step: 21.25 vector instructions instead of 20); a wave whose reads all have the widest span the arguments allow runs the fixed form's loop.
 * Measured on 6,666,667 reads of 100 .. 200 bases (10^9 bases), one MI355X (profiles/r19_reads_edist_batch.json), ASCII / packed, six outputs, END anchor:
 * k = 16, four offsets: 0.26 / 0.12 ms at 1 query, 0.58 / 0.55 at 8, 4.0 / 4.2 at 64, 31.6 / 33.2 at 512; k = 31, eight offsets: 0.36 / 0.18, 1.07 / 1.05,
 * 7.9 / 8.2, 62.5 / 65.5 ms: 0.11 - 0.89 x the time of a device gather of the spans into a compact batch plus bitnuc_reads_edist_anchored*_async on it up
 * to 64 queries, 0.97 (ASCII) and 1.03 - 1.05 (packed) x at 512, where the recurrence is all there is.  On equal-length reads the fixed form above gives
 * the same answers; this form takes 1.00 - 1.01 x (ASCII) and 1.06 - 1.08 x (packed) of its time at 64 queries and more: a fixed-length batch belongs
 * there.
 * Out of scope: a per-read offset table as an argument, anchored spans above 64 bases (the whole read: bitnuc_reads_edist_best_batch* below; the alignment's start: bitnuc_reads_edist_start_batch* below with (START, pos_lo) or (END, pos_hi)),
 * reverse-complement queries. */
int bitnuc_reads_edist_anchored_batch_async(bitnuc_ctx *ctx, const uint8_t *d_seq, const uint64_t *d_offsets, size_t count, size_t total_bases, size_t k, int anchor,
                                            size_t pos_lo, size_t pos_hi, const uint64_t *d_queries, size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_end,
                                            uint8_t *d_best_dist, uint32_t *d_second_query, uint32_t *d_second_end, uint8_t *d_second_dist, bitnuc_err *err);
int bitnuc_reads_edist_anchored_batch_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, const uint64_t *d_word_offsets, const uint64_t *d_offsets, size_t count,
                                                   size_t total_words, size_t k, int anchor, size_t pos_lo, size_t pos_hi, const uint64_t *d_queries, size_t n_queries,
                                                   uint32_t *d_best_query, uint32_t *d_best_end, uint8_t *d_best_dist, uint32_t *d_second_query,
                                                   uint32_t *d_second_end, uint8_t *d_second_dist, bitnuc_err *err);
int bitnuc_reads_edist_anchored_batch(bitnuc_ctx *ctx, const uint8_t *seq, const uint64_t *offsets, size_t count, size_t k, int anchor, size_t pos_lo, size_t pos_hi,
                                      const uint64_t *queries, size_t n_queries, uint32_t *best_query, uint32_t *best_end, uint8_t *best_dist, uint32_t *second_query,
                                      uint32_t *second_end, uint8_t *second_dist, bitnuc_err *err);
int bitnuc_reads_edist_anchored_batch_packed(bitnuc_ctx *ctx, const uint64_t *words, const uint64_t *word_offsets, const uint64_t *offsets, size_t count, size_t k,
                                             int anchor, size_t pos_lo, size_t pos_hi, const uint64_t *queries, size_t n_queries, uint32_t *best_query,
                                             uint32_t *best_end, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_end, uint8_t *second_dist, bitnuc_err *err);
/* the pattern twins: a set of bases per query position (bitnuc_pattern); everything else as above */
int bitnuc_reads_pattern_edist_anchored_batch_async(bitnuc_ctx *ctx, const uint8_t *d_seq, const uint64_t *d_offsets, size_t count, size_t total_bases, size_t k,
                                                    int anchor, size_t pos_lo, size_t pos_hi, const bitnuc_pattern *d_patterns, size_t n_queries, uint32_t *d_best_query,
                                                    uint32_t *d_best_end, uint8_t *d_best_dist, uint32_t *d_second_query, uint32_t *d_second_end,
                                                    uint8_t *d_second_dist, bitnuc_err *err);
int bitnuc_reads_pattern_edist_anchored_batch_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, const uint64_t *d_word_offsets, const uint64_t *d_offsets,
                                                           size_t count, size_t total_words, size_t k, int anchor, size_t pos_lo, size_t pos_hi,
                                                           const bitnuc_pattern *d_patterns, size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_end,
                                                           uint8_t *d_best_dist, uint32_t *d_second_query, uint32_t *d_second_end, uint8_t *d_second_dist,
                                                           bitnuc_err *err);
int bitnuc_reads_pattern_edist_anchored_batch(bitnuc_ctx *ctx, const uint8_t *seq, const uint64_t *offsets, size_t count, size_t k, int anchor, size_t pos_lo,
                                              size_t pos_hi, const bitnuc_pattern *patterns, size_t n_queries, uint32_t *best_query, uint32_t *best_end,
                                              uint8_t *best_dist, uint32_t *second_query, uint32_t *second_end, uint8_t *second_dist, bitnuc_err *err);
int bitnuc_reads_pattern_edist_anchored_batch_packed(bitnuc_ctx *ctx, const uint64_t *words, const uint64_t *word_offsets, const uint64_t *offsets, size_t count,
                                                     size_t k, int anchor, size_t pos_lo, size_t pos_hi, const bitnuc_pattern *patterns, size_t n_queries,
                                                     uint32_t *best_query, uint32_t *best_end, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_end,
                                                     uint8_t *second_dist, bitnuc_err *err);
/* ---- INDEL-TOLERANT best match and runner-up per read over the WHOLE read of a fixed-length batch (which of Q adapters, primers or linkers a read carries,
 * where it ends and with how many edits: an adapter inside a long or merged read, a linker between two barcodes, a primer at an unknown offset, read-through
 * into the 3' adapter) -- the twin of bitnuc_reads_hdist_best* / _best2* with the EDIT distance of bitnuc_reads_edist_anchored*, the span being the whole
 * read ----
 * Arguments: those of bitnuc_reads_hdist_best* (read_len, count, k, queries, n_queries; ASCII or packed) with the six outputs of
 * bitnuc_reads_edist_anchored*: best_end / second_end hold ends.  Each function below is the twin of the bitnuc_reads_hdist_best* function of the same
 * suffix (bitnuc_reads_pattern_edist_best*: of bitnuc_reads_pattern_best*).
 * Distance and results: the definition of the bitnuc_reads_edist_anchored* block with t_1 .. t_n = read_r and n = read_len: D[0][j] = 0, D[i][0] = i,
 * edist(r, q) = min over 1 <= j <= n of D[k][j], end(r, q) = the smallest such j: one past the last aligned base, counted from the read's start.  The best
 * triple is the lexicographic minimum of (edist, query, end); the second triple the minimum over the other queries (an equal duplicate query at a higher
 * index is the runner-up, one query gives the fill in the second triple).  second_query, second_end and second_dist may ALL be NULL: only the best triple
 * is written; one or two of them NULL -> UNSUPPORTED.  read_len < k, k == 0 or n_queries == 0: every read gets the fill (UINT32_MAX, UINT32_MAX, 0xFF) in
 * all written outputs (the family's rule, although the distance is defined there).  Deterministic.  Exactly [0, count) of each output is written; the dist
 * arrays may have any byte offset.
 * Identities.  On reads of k <= read_len <= 64 bases this form equals bitnuc_reads_edist_anchored*(pos_lo = 0, pos_hi = SIZE_MAX) byte for byte.  The
 * pattern forms on singleton patterns (bitnuc_pattern_from_2bit) equal the exact forms byte for byte.  best_dist <= the best_dist of
 * bitnuc_reads_hdist_best* on every read (every window is a substring).  Truncating every read to its first m >= k bases never lowers best_dist.
 * Validation.  Every byte of every read is validated (read_len >= k); the first invalid byte in buffer order -> INVALID_BASE with its absolute index,
 * latched once per call for bitnuc_ctx_sync() by the _async forms (outputs then unspecified); the host forms below the cutoff leave the outputs untouched.
 * A call that writes only fills reads and validates nothing.  (The ASCII kernel loads aligned 4-byte words that hold a byte of a read: at most 3 bytes
 * before and after the batch are touched, never examined.)  Packed: bits above a read's last base are ignored.
 * Limits: k <= 32; read_len < 2^32 - 1 and count x 32 ceil(read_len / 32) < 2^58 (UNSUPPORTED, value = read_len); n_queries <= BITNUC_MAX_QUERIES;
 * read_len > BITNUC_EDIST_MAX_READ -> UNSUPPORTED (value = read_len): the bound keeps (distance, end - 1) one 32-bit running minimum in the kernel's step.
 * Checks, in order: those of the bitnuc_reads_edist_anchored* block with (5) read as: read_len > BITNUC_EDIST_MAX_READ -> UNSUPPORTED (value = read_len).
 * Nothing is written on an argument error.
 * The _async forms have the contract of bitnuc_reads_edist_anchored*_async: device pointers for everything, the context's stream, no host synchronisation
 * but the growth of context scratch (16 bytes per query; no per-read scratch, no finish kernel), capturable into a hipGraph after a warm-up of THIS call
 * with the same or larger n_queries; reads and queries are read at every replay.  The host forms are synchronous and judge count x read_len x n_queries
 * (saturated) against the host cutoff: below it they run on the host (ctx may be NULL), above it through the context in chunks of whole reads; INVALID_BASE
 * indices stay absolute.
 * Cost: the vector-ALU kernel of bitnuc_reads_edist_anchored*, one read per lane, the same step of 20 vector instructions per (read, query, base); the lane
 * walks its read in pieces of 64 bases and carries the columns of four queries from piece to piece; the read is re-read once per four queries.  No LDS, no
 * atomics but the invalid-byte latch.  Measured on 6,666,667 x 150-base reads, one MI355X (profiles/r22_reads_edist_best.json), ASCII / packed, six
 * outputs, k = 16 and 31 alike: 0.87 / 0.64 ms at 1 query, 4.03 / 3.91 at 8, 32.0 / 31.1 at 64, 255.7 / 248.7 at 512: 0.499 / 0.486 ps per (read, query,
 * base), 1.040 - 1.044 (ASCII) and 1.030 - 1.032 (packed) x that of bitnuc_reads_edist_anchored*_async at span 64 in the same queues; 3.8 - 4.2 x the time
 * of bitnuc_reads_hdist_best*_async on the same arguments at 64 queries and more, 3.1 - 3.4 x at 8, 1.1 - 1.6 x at 1 (another answer: the price of indel
 * tolerance); the pattern twins cost what the exact forms cost (0.995 - 1.002 x).
 * The alignment's start: bitnuc_reads_edist_start* below with (START, 0).  Partial adapters overhanging the 3' end with a minimum-overlap rule: bitnuc_reads_edist_adapter* below.  Out of scope: k > 32, affine gaps,
 * reverse-complement queries. */
#define BITNUC_EDIST_MAX_READ 67108864 /* 2^26 bases */
int bitnuc_reads_edist_best_async(bitnuc_ctx *ctx, const uint8_t *d_reads, size_t read_len, size_t count, size_t k, const uint64_t *d_queries, size_t n_queries,
                                  uint32_t *d_best_query, uint32_t *d_best_end, uint8_t *d_best_dist, uint32_t *d_second_query, uint32_t *d_second_end,
                                  uint8_t *d_second_dist, bitnuc_err *err);
int bitnuc_reads_edist_best_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, size_t read_len, size_t count, size_t k, const uint64_t *d_queries, size_t n_queries,
                                         uint32_t *d_best_query, uint32_t *d_best_end, uint8_t *d_best_dist, uint32_t *d_second_query, uint32_t *d_second_end,
                                         uint8_t *d_second_dist, bitnuc_err *err);
int bitnuc_reads_edist_best(bitnuc_ctx *ctx, const uint8_t *reads, size_t read_len, size_t count, size_t k, const uint64_t *queries, size_t n_queries,
                            uint32_t *best_query, uint32_t *best_end, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_end, uint8_t *second_dist,
                            bitnuc_err *err);
int bitnuc_reads_edist_best_packed(bitnuc_ctx *ctx, const uint64_t *words, size_t read_len, size_t count, size_t k, const uint64_t *queries, size_t n_queries,
                                   uint32_t *best_query, uint32_t *best_end, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_end, uint8_t *second_dist,
                                   bitnuc_err *err);
/* the pattern twins: a set of bases per query position (bitnuc_pattern); everything else as above */
int bitnuc_reads_pattern_edist_best_async(bitnuc_ctx *ctx, const uint8_t *d_reads, size_t read_len, size_t count, size_t k, const bitnuc_pattern *d_patterns,
                                          size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_end, uint8_t *d_best_dist, uint32_t *d_second_query,
                                          uint32_t *d_second_end, uint8_t *d_second_dist, bitnuc_err *err);
int bitnuc_reads_pattern_edist_best_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, size_t read_len, size_t count, size_t k, const bitnuc_pattern *d_patterns,
                                                 size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_end, uint8_t *d_best_dist, uint32_t *d_second_query,
                                                 uint32_t *d_second_end, uint8_t *d_second_dist, bitnuc_err *err);
int bitnuc_reads_pattern_edist_best(bitnuc_ctx *ctx, const uint8_t *reads, size_t read_len, size_t count, size_t k, const bitnuc_pattern *patterns, size_t n_queries,
                                    uint32_t *best_query, uint32_t *best_end, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_end, uint8_t *second_dist,
                                    bitnuc_err *err);
int bitnuc_reads_pattern_edist_best_packed(bitnuc_ctx *ctx, const uint64_t *words, size_t read_len, size_t count, size_t k, const bitnuc_pattern *patterns,
                                           size_t n_queries, uint32_t *best_query, uint32_t *best_end, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_end,
                                           uint8_t *second_dist, bitnuc_err *err);

/* ---- ... of a RAGGED batch: the layout, tables and checks of bitnuc_reads_hdist_best_batch* with the distance and results of the block above, per read ----
 * Arguments: those of the bitnuc_reads_hdist_best_batch* / bitnuc_reads_pattern_best_batch* function of the same suffix, which each function below is the
 * twin of, with the six outputs of the block above.
 * Distance and results: as above with t_1 .. t_n = read_r, n = len_r = offsets[r + 1] - offsets[r]; ends count from the read's start.  A read with
 * len_r < k gets the fill, and so does every read when k == 0 or n_queries == 0.
 * Identities.  On a batch of equal lengths this form equals the fixed form above byte for byte; the other identities of the block above hold per read.
 * Validation.  A read with len_r >= k has all its bytes validated; the first invalid byte in buffer order -> INVALID_BASE with its absolute index (latched
 * once per call by the _async forms; the host forms leave the outputs untouched).  A read shorter than k is neither read nor validated (the rule of
 * bitnuc_reads_edist_anchored_batch*, not that of bitnuc_reads_hdist_best_batch*).  No aligned 4-byte word (packed: 8-byte word) that holds no base of a
 * read of at least k bases is touched.
 * Limits: k <= 32, n_queries <= BITNUC_MAX_QUERIES, the totals below 2^58 as in bitnuc_reads_hdist_best_batch*; a read of more than BITNUC_EDIST_MAX_READ
 * bases -> UNSUPPORTED (value = its length): the host forms judge it when they validate the tables (after the tables' own checks, before the fill and
 * before any data pointer is looked at); the _async forms TRUST their tables, as their twins do.
 * Checks, in order: those of the bitnuc_reads_hdist_best_batch* block, with the second triple's rule (all three NULL or none) at the pointer check.
 * Nothing is written on an argument error.
 * The _async forms: as above; the tables, the reads and the queries are read on the device at every replay.  The host forms judge (the sum of len_r over
 * the reads with len_r >= k) x n_queries (saturated) against the host cutoff; above it: chunks of whole reads with rebased tables, absolute indices.
 * Cost: the kernel above under the ragged layout policy: every lane loads its own read's table entries one trip ahead; the loop over the bases is
 * wave-uniform over the LONGEST read among the wave's 64, with Eq forced to 0 behind a lane's own length (21.25 vector instructions a step instead of 20);
 * a wave of equal lengths runs the fixed form's loop.  Measured on one MI355X (the same profile): on 6,666,667 equal-length reads 1.035 - 1.037 (ASCII)
 * and 1.009 - 1.010 (packed) x the fixed form's time at 64 queries and more; on reads of 100 .. 200 bases (10^9 bases) 1.40 - 1.43 x the time of equal-length
 * reads of the same total, where the longest read of each wave of 64 consecutive reads predicts 1.41: 46.5 / 44.8 ms at 64 queries, 372 / 359 at 512; 4.6 -
 * 5.1 x bitnuc_reads_hdist_best_batch*_async there.  Sorting or binning reads by length is the caller's.
 * Out of scope: as above, and per-read offset tables. */
int bitnuc_reads_edist_best_batch_async(bitnuc_ctx *ctx, const uint8_t *d_seq, const uint64_t *d_offsets, size_t count, size_t total_bases, size_t k,
                                        const uint64_t *d_queries, size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_end, uint8_t *d_best_dist,
                                        uint32_t *d_second_query, uint32_t *d_second_end, uint8_t *d_second_dist, bitnuc_err *err);
int bitnuc_reads_edist_best_batch_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, const uint64_t *d_word_offsets, const uint64_t *d_offsets, size_t count,
                                               size_t total_words, size_t k, const uint64_t *d_queries, size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_end,
                                               uint8_t *d_best_dist, uint32_t *d_second_query, uint32_t *d_second_end, uint8_t *d_second_dist, bitnuc_err *err);
int bitnuc_reads_edist_best_batch(bitnuc_ctx *ctx, const uint8_t *seq, const uint64_t *offsets, size_t count, size_t k, const uint64_t *queries, size_t n_queries,
                                  uint32_t *best_query, uint32_t *best_end, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_end, uint8_t *second_dist,
                                  bitnuc_err *err);
int bitnuc_reads_edist_best_batch_packed(bitnuc_ctx *ctx, const uint64_t *words, const uint64_t *word_offsets, const uint64_t *offsets, size_t count, size_t k,
                                         const uint64_t *queries, size_t n_queries, uint32_t *best_query, uint32_t *best_end, uint8_t *best_dist, uint32_t *second_query,
                                         uint32_t *second_end, uint8_t *second_dist, bitnuc_err *err);
/* the pattern twins: a set of bases per query position (bitnuc_pattern); everything else as above */
int bitnuc_reads_pattern_edist_best_batch_async(bitnuc_ctx *ctx, const uint8_t *d_seq, const uint64_t *d_offsets, size_t count, size_t total_bases, size_t k,
                                                const bitnuc_pattern *d_patterns, size_t n_queries, uint32_t *d_best_query, uint32_t *d_best_end, uint8_t *d_best_dist,
                                                uint32_t *d_second_query, uint32_t *d_second_end, uint8_t *d_second_dist, bitnuc_err *err);
int bitnuc_reads_pattern_edist_best_batch_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, const uint64_t *d_word_offsets, const uint64_t *d_offsets, size_t count,
                                                       size_t total_words, size_t k, const bitnuc_pattern *d_patterns, size_t n_queries, uint32_t *d_best_query,
                                                       uint32_t *d_best_end, uint8_t *d_best_dist, uint32_t *d_second_query, uint32_t *d_second_end,
                                                       uint8_t *d_second_dist, bitnuc_err *err);
int bitnuc_reads_pattern_edist_best_batch(bitnuc_ctx *ctx, const uint8_t *seq, const uint64_t *offsets, size_t count, size_t k, const bitnuc_pattern *patterns,
                                          size_t n_queries, uint32_t *best_query, uint32_t *best_end, uint8_t *best_dist, uint32_t *second_query, uint32_t *second_end,
                                          uint8_t *second_dist, bitnuc_err *err);
int bitnuc_reads_pattern_edist_best_batch_packed(bitnuc_ctx *ctx, const uint64_t *words, const uint64_t *word_offsets, const uint64_t *offsets, size_t count, size_t k,
                                                 const bitnuc_pattern *patterns, size_t n_queries, uint32_t *best_query, uint32_t *best_end, uint8_t *best_dist,
                                                 uint32_t *second_query, uint32_t *second_end, uint8_t *second_dist, bitnuc_err *err);

/* ---- The 3' ADAPTER per read: of Q adapters, which one a read carries IN FULL anywhere or as a PREFIX OVERHANGING the read's end, with how many edits,
 * and the base to cut at -- the search stage of an adapter trimmer in one call (bitnuc_reads_edist_best* finds only full adapters: a 150-base read that
 * ends with the first 10 bases of a k-base adapter is at distance about k - 10 there) ----
 * Arguments (fixed form): read_len, count, k, queries | patterns, n_queries as in bitnuc_reads_edist_best*, then size_t min_overlap, size_t err_num,
 * size_t err_den and five outputs.  The ragged forms (_batch*) take the tables of bitnuc_reads_edist_best_batch* of the same suffix instead of read_len;
 * there n = len_r = offsets[r + 1] - offsets[r] per read.
 * Allowance: allowed(i) = floor(i x err_num / err_den), the trimmers' error-rate rule as an exact rational (1 / 10 with min_overlap = 3 is the usual
 * default).
 * Distance: D of the bitnuc_reads_edist_anchored* block over the whole read: D[0][j] = 0, D[i][0] = i, n = the read's bases; a pattern position matches
 * when the base is in its set.
 * Candidates of (read, query) are pairs (i, j).  FULL: i = k and any 1 <= j <= n.  OVERHANG: min_overlap <= i < k and j = n (the read ends inside the
 * adapter: its last bases align to the adapter's first i positions).  A candidate is admissible when D[i][j] <= allowed(i); min_overlap <= k, so a full
 * candidate always meets the overlap rule.  Per candidate d = D[i][j], matches = i - d, misses = k - matches.  The read's result is the admissible
 * candidate, over all queries, with the lexicographically smallest (misses, d, query, j): most matched adapter positions, then fewest edits, then the
 * lower query index, then the first end.  With i = k this is the family's (dist, query, end).
 * Cut: with the winner's (q, i, e = j, d), cut = s is the lexicographic minimum over s in [e - min(e, 2i - 1), e] of (Lev(q_1 .. q_i, t[s, e)), e - s):
 * the rule of bitnuc_reads_edist_start* applied to the prefix; its distance equals d.  read[0, cut) is what a trimmer keeps.
 * Outputs, exactly [0, count) of each: adapter (u32, the query index), cut (u32), end (u32, = j), overlap (u8, = i), dist (u8, = d).  The fill is
 * UINT32_MAX x 3 and 0xFF x 2: written when no candidate is admissible, and for every read when k == 0 or n_queries == 0.  Fixed form: every read gets it
 * when read_len < k.  Ragged form: a read with len_r < k gets it and is neither read nor validated.  Deterministic.
 * Identities.  With min_overlap = k and rate 1 / 1: (adapter, end, dist) equals the best triple of bitnuc_reads_edist_best* byte for byte, overlap = k, and
 * (cut, dist) equals bitnuc_reads_edist_start* with (START, 0) on that triple.  With rate 0 / 1 and min_overlap = 1 the result is plain string matching:
 * the first exact occurrence, else the longest i with the read ending in q_1 .. q_i; cut = end - overlap, dist = 0.  The pattern twins on singleton
 * patterns equal the exact forms; the ragged forms on equal lengths equal the fixed forms; ASCII and packed agree; dist = Lev(q_1 .. q_overlap,
 * read[cut, end)).
 * Validation: that of bitnuc_reads_edist_best* / _best_batch*: every byte of every read of at least k bases; the first invalid byte in buffer order ->
 * INVALID_BASE with its absolute index, latched once per call for bitnuc_ctx_sync() by the _async forms (outputs then unspecified); the host forms below
 * the cutoff leave the outputs untouched.  A call that writes only fills reads and validates nothing.  Packed: bits above a read's last base are ignored.
 * Limits: those of bitnuc_reads_edist_best* / _best_batch*, BITNUC_EDIST_MAX_READ included (the ragged host forms judge it at the table check, the ragged
 * _async forms trust their tables).
 * Checks, in order: (1) ctx (_async forms, and the host forms above the cutoff), (2) k > 32 -> SEQUENCE_TOO_LONG (value = k), (3) the layout's size limits
 * (UNSUPPORTED), (4) n_queries > BITNUC_MAX_QUERIES -> UNSUPPORTED (value = n_queries), then with k >= 1: (5) min_overlap == 0 or min_overlap > k ->
 * UNSUPPORTED (value = min_overlap), (6) err_den == 0 or err_num > err_den -> UNSUPPORTED (value = err_num); (7) fixed: read_len > BITNUC_EDIST_MAX_READ ->
 * UNSUPPORTED (value = read_len), (8) count == 0 -> OK, nothing written, (9) any of the five outputs NULL, adapter, cut or end not 4-byte aligned (overlap
 * and dist may have any byte offset), queries NULL with n_queries > 0 or not 8-byte aligned (patterns: 4-byte), an offsets table NULL or not 8-byte
 * aligned -> UNSUPPORTED, (10) ragged host forms: the tables' validation and the read length limit, (11) where a read is looked at: reads / words NULL
 * (words not 8-byte aligned) -> UNSUPPORTED.  Nothing is written on an argument error.
 * The _async forms have the contract of bitnuc_reads_edist_best*_async: device pointers for everything, the context's stream, no host synchronisation but
 * the growth of context scratch (16 bytes per query, the family's table slot; the allowances travel in the kernel's arguments), capturable into a
 * hipGraph after a warm-up of THIS call with the same or larger n_queries; reads, tables and queries are read at every replay.  The host forms are
 * synchronous and judge the work of bitnuc_reads_edist_best* / _best_batch* against the host cutoff: below it they run on the host (ctx may be NULL), above
 * it through the context in chunks of whole reads; INVALID_BASE indices stay absolute.
 * Cost: the kernel of bitnuc_reads_edist_best* (one read per lane, the same step of 20 vector instructions per (read, query, base)) with, per (read,
 * query), a decode of the walk's LAST COLUMN -- after the read's last base the column (Pv, Mv) holds D[i][n] for every prefix length i at once, so the
 * overhang costs no second pass over the read -- and per read one backward walk of at most 2 x overlap - 1 bases for the cut.  The ragged forms' masked
 * loop snapshots the column at a lane's own last base (two selects per query and step).  No LDS, no atomics but the invalid-byte latch.
 * Measured on 6,666,667 x 150-base reads and on reads of 100 .. 200 bases (10^9 bases each), one MI355X (profiles/r25_reads_edist_adapter.json), rate 1 / 10,
 * min_overlap 3, against today's nearest route in the same queues -- bitnuc_reads_edist_best*_async with the second triple NULL followed by
 * bitnuc_reads_edist_start*_async, which finds no overhang: a yardstick of cost only.  Fixed, ASCII / packed, k = 16: 0.92 / 0.68 ms at 1 adapter, 4.29 / 4.12
 * at 8, 33.6 / 32.6 at 64, 268 / 260 at 512 (k = 31: 0.94 / 0.71, 4.47 / 4.31, 35.0 / 33.9, 279 / 270): 0.71 - 0.86 x the route at 1 adapter (one launch
 * instead of two), 0.99 - 1.03 x at 8, 1.04 x (k = 16) and 1.08 - 1.09 x (k = 31) at 64 and 512, where the decode's 9 vector instructions per (read, query,
 * prefix length) over the walk's 20 per base predict 1.045 and 1.09.  Ragged: 1.41 / 1.05 ms at 1 adapter, 6.9 / 6.6 at 8, 54 / 52 at 64, 434 / 416 at 512
 * (k = 16): 0.88 - 1.04 x the ragged route at 1, 1.12 - 1.14 x at 8, 1.16 - 1.20 x at 64 and 512 -- the snapshot makes the masked step 24 vector instructions
 * where the route's has 21.25 (predicted 1.16 at k = 16, 1.19 at k = 31).  26 of the 32 points are inside the bound from the disassembly, 6 outside it by at
 * most 0.005.  Not tuned.
 * Out of scope: reads shorter than k (the fill), a runner-up, 5' and anchored adapters, adapters that overhang the read's START, k > 32, per-adapter
 * rates, reverse complements. */
int bitnuc_reads_edist_adapter_async(bitnuc_ctx *ctx, const uint8_t *d_reads, size_t read_len, size_t count, size_t k, const uint64_t *d_queries, size_t n_queries,
                                     size_t min_overlap, size_t err_num, size_t err_den, uint32_t *d_adapter, uint32_t *d_cut, uint32_t *d_end, uint8_t *d_overlap,
                                     uint8_t *d_dist, bitnuc_err *err);
int bitnuc_reads_edist_adapter_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, size_t read_len, size_t count, size_t k, const uint64_t *d_queries,
                                            size_t n_queries, size_t min_overlap, size_t err_num, size_t err_den, uint32_t *d_adapter, uint32_t *d_cut, uint32_t *d_end,
                                            uint8_t *d_overlap, uint8_t *d_dist, bitnuc_err *err);
int bitnuc_reads_edist_adapter_batch_async(bitnuc_ctx *ctx, const uint8_t *d_seq, const uint64_t *d_offsets, size_t count, size_t total_bases, size_t k,
                                           const uint64_t *d_queries, size_t n_queries, size_t min_overlap, size_t err_num, size_t err_den, uint32_t *d_adapter,
                                           uint32_t *d_cut, uint32_t *d_end, uint8_t *d_overlap, uint8_t *d_dist, bitnuc_err *err);
int bitnuc_reads_edist_adapter_batch_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, const uint64_t *d_word_offsets, const uint64_t *d_offsets, size_t count,
                                                  size_t total_words, size_t k, const uint64_t *d_queries, size_t n_queries, size_t min_overlap, size_t err_num,
                                                  size_t err_den, uint32_t *d_adapter, uint32_t *d_cut, uint32_t *d_end, uint8_t *d_overlap, uint8_t *d_dist,
                                                  bitnuc_err *err);
int bitnuc_reads_edist_adapter(bitnuc_ctx *ctx, const uint8_t *reads, size_t read_len, size_t count, size_t k, const uint64_t *queries, size_t n_queries,
                               size_t min_overlap, size_t err_num, size_t err_den, uint32_t *adapter, uint32_t *cut, uint32_t *end, uint8_t *overlap, uint8_t *dist,
                               bitnuc_err *err);
int bitnuc_reads_edist_adapter_packed(bitnuc_ctx *ctx, const uint64_t *words, size_t read_len, size_t count, size_t k, const uint64_t *queries, size_t n_queries,
                                      size_t min_overlap, size_t err_num, size_t err_den, uint32_t *adapter, uint32_t *cut, uint32_t *end, uint8_t *overlap,
                                      uint8_t *dist, bitnuc_err *err);
int bitnuc_reads_edist_adapter_batch(bitnuc_ctx *ctx, const uint8_t *seq, const uint64_t *offsets, size_t count, size_t k, const uint64_t *queries, size_t n_queries,
                                     size_t min_overlap, size_t err_num, size_t err_den, uint32_t *adapter, uint32_t *cut, uint32_t *end, uint8_t *overlap,
                                     uint8_t *dist, bitnuc_err *err);
int bitnuc_reads_edist_adapter_batch_packed(bitnuc_ctx *ctx, const uint64_t *words, const uint64_t *word_offsets, const uint64_t *offsets, size_t count, size_t k,
                                            const uint64_t *queries, size_t n_queries, size_t min_overlap, size_t err_num, size_t err_den, uint32_t *adapter,
                                            uint32_t *cut, uint32_t *end, uint8_t *overlap, uint8_t *dist, bitnuc_err *err);
/* the pattern twins: a set of bases per adapter position (bitnuc_pattern); everything else as above */
int bitnuc_reads_pattern_edist_adapter_async(bitnuc_ctx *ctx, const uint8_t *d_reads, size_t read_len, size_t count, size_t k, const bitnuc_pattern *d_patterns,
                                             size_t n_queries, size_t min_overlap, size_t err_num, size_t err_den, uint32_t *d_adapter, uint32_t *d_cut, uint32_t *d_end,
                                             uint8_t *d_overlap, uint8_t *d_dist, bitnuc_err *err);
int bitnuc_reads_pattern_edist_adapter_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, size_t read_len, size_t count, size_t k, const bitnuc_pattern *d_patterns,
                                                    size_t n_queries, size_t min_overlap, size_t err_num, size_t err_den, uint32_t *d_adapter, uint32_t *d_cut,
                                                    uint32_t *d_end, uint8_t *d_overlap, uint8_t *d_dist, bitnuc_err *err);
int bitnuc_reads_pattern_edist_adapter_batch_async(bitnuc_ctx *ctx, const uint8_t *d_seq, const uint64_t *d_offsets, size_t count, size_t total_bases, size_t k,
                                                   const bitnuc_pattern *d_patterns, size_t n_queries, size_t min_overlap, size_t err_num, size_t err_den,
                                                   uint32_t *d_adapter, uint32_t *d_cut, uint32_t *d_end, uint8_t *d_overlap, uint8_t *d_dist, bitnuc_err *err);
int bitnuc_reads_pattern_edist_adapter_batch_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, const uint64_t *d_word_offsets, const uint64_t *d_offsets,
                                                          size_t count, size_t total_words, size_t k, const bitnuc_pattern *d_patterns, size_t n_queries,
                                                          size_t min_overlap, size_t err_num, size_t err_den, uint32_t *d_adapter, uint32_t *d_cut, uint32_t *d_end,
                                                          uint8_t *d_overlap, uint8_t *d_dist, bitnuc_err *err);
int bitnuc_reads_pattern_edist_adapter(bitnuc_ctx *ctx, const uint8_t *reads, size_t read_len, size_t count, size_t k, const bitnuc_pattern *patterns, size_t n_queries,
                                       size_t min_overlap, size_t err_num, size_t err_den, uint32_t *adapter, uint32_t *cut, uint32_t *end, uint8_t *overlap,
                                       uint8_t *dist, bitnuc_err *err);
int bitnuc_reads_pattern_edist_adapter_packed(bitnuc_ctx *ctx, const uint64_t *words, size_t read_len, size_t count, size_t k, const bitnuc_pattern *patterns,
                                              size_t n_queries, size_t min_overlap, size_t err_num, size_t err_den, uint32_t *adapter, uint32_t *cut, uint32_t *end,
                                              uint8_t *overlap, uint8_t *dist, bitnuc_err *err);
int bitnuc_reads_pattern_edist_adapter_batch(bitnuc_ctx *ctx, const uint8_t *seq, const uint64_t *offsets, size_t count, size_t k, const bitnuc_pattern *patterns,
                                             size_t n_queries, size_t min_overlap, size_t err_num, size_t err_den, uint32_t *adapter, uint32_t *cut, uint32_t *end,
                                             uint8_t *overlap, uint8_t *dist, bitnuc_err *err);
int bitnuc_reads_pattern_edist_adapter_batch_packed(bitnuc_ctx *ctx, const uint64_t *words, const uint64_t *word_offsets, const uint64_t *offsets, size_t count,
                                                    size_t k, const bitnuc_pattern *patterns, size_t n_queries, size_t min_overlap, size_t err_num, size_t err_den,
                                                    uint32_t *adapter, uint32_t *cut, uint32_t *end, uint8_t *overlap, uint8_t *dist, bitnuc_err *err);

/* The INDEL-TOLERANT search ALONG A REFERENCE: the best match and the count per query by EDIT distance, where bitnuc_kmer_hdist_best* and
 * bitnuc_kmer_hdist_count_multi* use the Hamming distance.  A guide or primer that sits in the reference with one bulge (one inserted or deleted base)
 * is at distance 1 here and at about 3k/4 there.
 * Definition.  The reference is t_1 .. t_n, a query has 1 <= k <= 32 positions.  D[0][j] = 0, D[i][0] = i, D[i][j] = min(D[i-1][j-1] + [t_j does not
 * match position i], D[i-1][j] + 1, D[i][j-1] + 1); E(j) = D[k][j] is the edit distance of the query to the best substring of the reference that ends at
 * base j (the substring may start anywhere and may be empty, so E(j) <= k).  "Matches" is equality of the 2-bit codes for an exact query (query bits
 * above 2k are ignored) and membership in position i's set for a bitnuc_pattern (the bitnuc_kmer_pattern_edist_* twins; an empty set matches no base and
 * is legal).  This is bitnuc_reads_edist_anchored's distance with the whole reference as the span, and `end` follows its convention: one past the last
 * aligned base, 1 <= end <= n.  The start of the alignment: bitnuc_ref_edist_start* (the family's second stage, below).
 * _best:        dist[q] = the minimum over 1 <= j <= n of E_q(j), end[q] = the smallest j that attains it.  end[0 .. n_queries) and
 *               dist[0 .. n_queries) are written and nothing after them; dist may have any byte offset.  dist[q] <= bitnuc_kmer_hdist_best's.
 * _count_multi: counts[q] = #{ 1 <= j <= n : E_q(j) <= taus[q] }, the number of END POSITIONS of approximate occurrences (one occurrence usually ends
 *               at several neighbouring j); any uint32_t tau is valid, tau >= k counts every j (n).  counts[0 .. n_queries) is written and nothing
 *               after it.  counts[q] >= bitnuc_kmer_hdist_count_multi's at the same tau.
 * The results are deterministic.  With k == 0 or n < k the family's rule holds although E(j) is defined for n < k: OK, every end UINT64_MAX and every
 * dist 0xFF, every count 0, and nothing is validated.
 * Checks, in this order (those of bitnuc_kmer_hdist_best* / _count_multi*): (1) ctx NULL -> UNSUPPORTED (_async forms; the host forms below the cutoff
 * accept NULL); (2) k > 32 -> SEQUENCE_TOO_LONG(k); (3) packed: n_words < ceil(n/32) -> INVALID_LENGTH(n); (4) n_queries == 0 -> OK, nothing written;
 * (5) n_queries > BITNUC_MAX_QUERIES -> UNSUPPORTED (err.value = n_queries); (6) _best: end or queries NULL or not 8-byte aligned, or dist NULL;
 * _count_multi: counts, queries or taus NULL or not 8-, 8-, 4-byte aligned -> UNSUPPORTED (patterns: 4-byte aligned); (7) k == 0 or n < k -> OK with
 * the values above; (8) a NULL reference, or packed words not 8-byte aligned -> UNSUPPORTED.
 * ASCII: bytes in either letter case at any byte alignment; an invalid base -> INVALID_BASE with the first invalid byte of all n in sequence order (the
 * _async forms latch it once per call for bitnuc_ctx_sync(); the outputs are then unspecified; the host forms leave them untouched below the cutoff).
 * Packed words 8-byte aligned; bits above 2n of the last word do not matter.
 * The _async forms have the _dev contract: device pointers (queries / patterns, taus and outputs included), enqueued on the context's stream, InvalidBase
 * latched for bitnuc_ctx_sync().  They keep one 8-byte key and one 16-byte table per query in context scratch (where the Hamming best match keeps its
 * own, under the same growth rule: a call that needs more than the context holds waits for the stream before it replaces the allocation) and can be
 * captured into a hipGraph after a warm-up with the same (or a larger) n_queries; during a capture scratch cannot grow (BITNUC_UNSUPPORTED, err.value =
 * the bytes needed).
 * The host forms are synchronous.  When n x n_queries is below the host cutoff they run on the host and ctx may be NULL; above it they run through the
 * context in chunks of 128 M end positions, each behind the 2k bases before it (packed: rounded up to whole words), which are run but not reported:
 * every end position is reported by exactly one chunk.  Best merges by the smallest (dist, end), count sums per query. */
int bitnuc_kmer_edist_best_async(bitnuc_ctx *ctx, const uint8_t *d_ref, size_t n, size_t k, const uint64_t *d_queries, size_t n_queries, uint64_t *d_end,
                                 uint8_t *d_dist, bitnuc_err *err);
int bitnuc_kmer_edist_best_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, size_t n_words, size_t n, size_t k, const uint64_t *d_queries,
                                        size_t n_queries, uint64_t *d_end, uint8_t *d_dist, bitnuc_err *err);
int bitnuc_kmer_edist_best(bitnuc_ctx *ctx, const uint8_t *ref, size_t n, size_t k, const uint64_t *queries, size_t n_queries, uint64_t *end, uint8_t *dist,
                           bitnuc_err *err);
int bitnuc_kmer_edist_best_packed(bitnuc_ctx *ctx, const uint64_t *words, size_t n_words, size_t n, size_t k, const uint64_t *queries, size_t n_queries,
                                  uint64_t *end, uint8_t *dist, bitnuc_err *err);
int bitnuc_kmer_edist_count_multi_async(bitnuc_ctx *ctx, const uint8_t *d_ref, size_t n, size_t k, const uint64_t *d_queries, const uint32_t *d_taus,
                                        size_t n_queries, uint64_t *d_counts, bitnuc_err *err);
int bitnuc_kmer_edist_count_multi_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, size_t n_words, size_t n, size_t k, const uint64_t *d_queries,
                                               const uint32_t *d_taus, size_t n_queries, uint64_t *d_counts, bitnuc_err *err);
int bitnuc_kmer_edist_count_multi(bitnuc_ctx *ctx, const uint8_t *ref, size_t n, size_t k, const uint64_t *queries, const uint32_t *taus, size_t n_queries,
                                  uint64_t *counts, bitnuc_err *err);
int bitnuc_kmer_edist_count_multi_packed(bitnuc_ctx *ctx, const uint64_t *words, size_t n_words, size_t n, size_t k, const uint64_t *queries,
                                         const uint32_t *taus, size_t n_queries, uint64_t *counts, bitnuc_err *err);
/* ... and under PATTERN queries: `const bitnuc_pattern *patterns` where `const uint64_t *queries` stood (4-byte aligned), everything else word for word.
 * One main kernel serves both kinds (the 16-byte table IS the pattern's sets), so a pattern costs what an exact query costs. */
int bitnuc_kmer_pattern_edist_best_async(bitnuc_ctx *ctx, const uint8_t *d_ref, size_t n, size_t k, const bitnuc_pattern *d_patterns, size_t n_queries,
                                         uint64_t *d_end, uint8_t *d_dist, bitnuc_err *err);
int bitnuc_kmer_pattern_edist_best_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, size_t n_words, size_t n, size_t k, const bitnuc_pattern *d_patterns,
                                                size_t n_queries, uint64_t *d_end, uint8_t *d_dist, bitnuc_err *err);
int bitnuc_kmer_pattern_edist_best(bitnuc_ctx *ctx, const uint8_t *ref, size_t n, size_t k, const bitnuc_pattern *patterns, size_t n_queries, uint64_t *end,
                                   uint8_t *dist, bitnuc_err *err);
int bitnuc_kmer_pattern_edist_best_packed(bitnuc_ctx *ctx, const uint64_t *words, size_t n_words, size_t n, size_t k, const bitnuc_pattern *patterns,
                                          size_t n_queries, uint64_t *end, uint8_t *dist, bitnuc_err *err);
int bitnuc_kmer_pattern_edist_count_multi_async(bitnuc_ctx *ctx, const uint8_t *d_ref, size_t n, size_t k, const bitnuc_pattern *d_patterns,
                                                const uint32_t *d_taus, size_t n_queries, uint64_t *d_counts, bitnuc_err *err);
int bitnuc_kmer_pattern_edist_count_multi_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, size_t n_words, size_t n, size_t k,
                                                       const bitnuc_pattern *d_patterns, const uint32_t *d_taus, size_t n_queries, uint64_t *d_counts,
                                                       bitnuc_err *err);
int bitnuc_kmer_pattern_edist_count_multi(bitnuc_ctx *ctx, const uint8_t *ref, size_t n, size_t k, const bitnuc_pattern *patterns, const uint32_t *taus,
                                          size_t n_queries, uint64_t *counts, bitnuc_err *err);
int bitnuc_kmer_pattern_edist_count_multi_packed(bitnuc_ctx *ctx, const uint64_t *words, size_t n_words, size_t n, size_t k, const bitnuc_pattern *patterns,
                                                 const uint32_t *taus, size_t n_queries, uint64_t *counts, bitnuc_err *err);
/* The indel-tolerant HIT LIST: WHERE the ends within tau are, for one query per call (a host value, as in bitnuc_kmer_hdist_hits*).  With E(j) as above:
 *   *n_hits = #{ 1 <= j <= n : E(j) <= tau }, exactly what bitnuc_kmer_edist_count_multi* returns for the same single query and tau; it may exceed cap;
 *   end[0 .. min(cap, *n_hits)) = those j in ascending order; hit_dist[r] = E(end[r]); hit_dist may be NULL and is then not written.
 * Nothing is written at or beyond cap; cap == 0 with end == NULL is valid and gives the count only.  Any unsigned tau is valid; tau >= k makes every end a
 * hit.  Neighbouring ends of a good match are hits too (E(j +- 1) <= E(j) + 1), so an exact copy shows as a run of up to 2 tau + 1 ends; the list is not
 * collapsed to local minima.  With k == 0 or n < k: OK, *n_hits = 0, nothing validated.  The result is deterministic.
 * Checks, in this order: (1) ctx NULL -> UNSUPPORTED (_async forms; the host forms below the cutoff accept NULL); (2) k > 32 -> SEQUENCE_TOO_LONG(k);
 * (3) packed: n_words < ceil(n/32) -> INVALID_LENGTH(n); (4) patterns: pattern NULL or not 4-byte aligned -> UNSUPPORTED; (5) n_hits NULL or not 8-byte
 * aligned, end not 8-byte aligned, or end NULL with cap > 0 -> UNSUPPORTED; (6) k == 0 or n < k -> OK, *n_hits = 0; (7) a NULL reference, or packed words
 * not 8-byte aligned -> UNSUPPORTED.  ASCII: an invalid base -> INVALID_BASE with the first invalid byte of all n in sequence order (the _async forms latch
 * it once per call for bitnuc_ctx_sync(); the outputs are then unspecified; the host forms leave them untouched below the cutoff).
 * The _async forms have the _dev contract for the reference and the outputs (device pointers, the context's stream); `pattern` is read from HOST memory
 * during the call.  Three launches (count per chunk of 1024 ends, scan, emit; the emit pass is skipped for cap == 0 and walks only chunks that hold a
 * hit); the per-chunk counts live in context scratch, shared with the Hamming hit list in stream order; capturable into a hipGraph after a warm-up with
 * the same (or a larger) n.  The host forms are synchronous; below the host cutoff (judged on n) they run on the host and ctx may be NULL, above it in
 * chunks of 128 M ends behind their 2k lead bases: every end is reported by exactly one chunk. */
int bitnuc_kmer_edist_hits_async(bitnuc_ctx *ctx, const uint8_t *d_ref, size_t n, size_t k, uint64_t query, unsigned tau, uint64_t *d_end, uint8_t *d_hit_dist,
                                 size_t cap, uint64_t *d_n_hits, bitnuc_err *err);
int bitnuc_kmer_edist_hits_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, size_t n_words, size_t n, size_t k, uint64_t query, unsigned tau,
                                        uint64_t *d_end, uint8_t *d_hit_dist, size_t cap, uint64_t *d_n_hits, bitnuc_err *err);
int bitnuc_kmer_edist_hits(bitnuc_ctx *ctx, const uint8_t *ref, size_t n, size_t k, uint64_t query, unsigned tau, uint64_t *end, uint8_t *hit_dist, size_t cap,
                           uint64_t *n_hits, bitnuc_err *err);
int bitnuc_kmer_edist_hits_packed(bitnuc_ctx *ctx, const uint64_t *words, size_t n_words, size_t n, size_t k, uint64_t query, unsigned tau, uint64_t *end,
                                  uint8_t *hit_dist, size_t cap, uint64_t *n_hits, bitnuc_err *err);
int bitnuc_kmer_pattern_edist_hits_async(bitnuc_ctx *ctx, const uint8_t *d_ref, size_t n, size_t k, const bitnuc_pattern *pattern, unsigned tau, uint64_t *d_end,
                                         uint8_t *d_hit_dist, size_t cap, uint64_t *d_n_hits, bitnuc_err *err);
int bitnuc_kmer_pattern_edist_hits_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, size_t n_words, size_t n, size_t k, const bitnuc_pattern *pattern,
                                                unsigned tau, uint64_t *d_end, uint8_t *d_hit_dist, size_t cap, uint64_t *d_n_hits, bitnuc_err *err);
int bitnuc_kmer_pattern_edist_hits(bitnuc_ctx *ctx, const uint8_t *ref, size_t n, size_t k, const bitnuc_pattern *pattern, unsigned tau, uint64_t *end,
                                   uint8_t *hit_dist, size_t cap, uint64_t *n_hits, bitnuc_err *err);
int bitnuc_kmer_pattern_edist_hits_packed(bitnuc_ctx *ctx, const uint64_t *words, size_t n_words, size_t n, size_t k, const bitnuc_pattern *pattern,
                                          unsigned tau, uint64_t *end, uint8_t *hit_dist, size_t cap, uint64_t *n_hits, bitnuc_err *err);

/* ---- The INDEL-TOLERANT family's SECOND STAGE: WHERE the alignment that ends at a given base STARTS -- bitnuc_reads_edist_start*, bitnuc_ref_edist_start*
 * and their pattern twins.  Every forward form of the family (the anchored, whole-read and ragged per-read forms; best match, count and hit list along a
 * reference) reports a distance and an END, one past the last aligned base.  With indels the start does not follow from the end: the aligned substring has
 * between k - dist and k + dist bases.  These calls take (query index, end) per item and write (start, dist); they compose with every forward form, and none
 * of those changes.  Uses: cutting a read in front of a 3' adapter, cutting out the linker between two barcodes, reporting an off-target site as an
 * interval, clipping a primer with a bulge.
 * Definition.  An item has a text t of len bases, a floor a, a query q of 1 <= k <= 32 positions (exact 2-bit, or a bitnuc_pattern) and an end e with
 * a <= e <= len.  Let w = min(e - a, 2k - 1).  (dist, start) = the lexicographic minimum over s in [e - w, e] of (Lev(q, t[s, e)), e - s), reported as
 * start = s: the smallest distance and, among the substrings that attain it, the SHORTEST.  Lev is the family's distance (the Levenshtein distance of the
 * query to that substring; "matches" is equality for an exact query and set membership for a pattern; an empty set matches nothing).  dist <= k;
 * start == e is legal: the empty substring, dist = k.
 * The window bound.  A substring of c bases costs at least |c - k| edits, so c >= 2k costs at least k -- what the empty substring (c = 0) costs already, and
 * a tie goes to the shorter substring: no substring of more than 2k - 1 <= 63 bases can be the answer, and none is looked at.
 * Identity.  If (q, e, d) is a triple that any forward form wrote and the floor is that form's span start (below), then dist == d: the forward
 * E(e) = D[k][e] is the minimum over s of Lev(q, t[s, e)) with s at or behind the span's start, and by the window bound that minimum is attained inside
 * the window.
 * How it is computed.  No traceback matrix: the family's bit-parallel column step runs BACKWARDS from base e - 1, with the query reversed and a carry-in of 1
 * on the horizontal delta (row 0 is D'[0][c] = c), so D'[k][c] = Lev(q, t[e - c, e)); the first minimum over c = 0 .. w is the answer.
 * Reading and validation.  Only the w bases t[e - w, e) of an item are read.  ASCII bytes are validated under bitnuc_reads_edist_anchored*'s rule for span
 * bytes: the first invalid walked byte in buffer order -> INVALID_BASE with its absolute index, latched once per call for bitnuc_ctx_sync() by the _async
 * forms (outputs then unspecified; the host forms on the host leave the outputs untouched).  (The ASCII kernel loads the aligned 4-byte words that hold a
 * walked byte: at most 3 bytes before or after a walked range are touched, never examined.)
 * Skipped items.  An item is skipped when query >= n_queries (this covers the UINT32_MAX fill of the forward forms), e > len, or e < a; every item is
 * skipped when k == 0 or n_queries == 0.  A skipped item writes the fill (start UINT32_MAX / UINT64_MAX, dist 0xFF), has nothing read or validated, and no
 * address is formed from its values.  This is a rule of the contract: the hit list leaves end[*n_hits .. cap) unwritten, and the forward forms write fills
 * for reads without a window.
 *
 * PER READ -- bitnuc_reads_edist_start[_packed], bitnuc_reads_edist_start_batch[_packed], each _async and host, and the bitnuc_reads_pattern_edist_start*
 * twins.  Layout arguments: those of bitnuc_reads_edist_best* / bitnuc_reads_edist_best_batch* of the same suffix.  Then k, anchor, pos, the queries /
 * patterns and n_queries of the forward call, and per read: query[r] (the query index, e.g. best_query or second_query), end[r] (e.g. best_end), start[r],
 * dist[r].  dist may be NULL and is then not written; query, end and start are 4-byte aligned, dist may have any byte offset.  Exactly [0, count) of each
 * output is written.  Ends and starts count from the read's start.  One (query, end) pair per read and call: the runner-up takes a second call.
 * Floor of read r, with len its length: BITNUC_ANCHOR_START: a = pos; BITNUC_ANCHOR_END: a = len - k - pos, saturating at 0.  To get the forward form's span
 * start pass: after the whole-read forms (START, 0); after the fixed anchored forms (START, pos_lo); after the ragged anchored forms (START, pos_lo) or
 * (END, pos_hi) -- the ragged form's first admissible offset a_r is pos_lo counted from the start, and max(0, len_r - k - pos_hi) counted from the end.
 * Checks, in order: (1) ctx (_async forms, and the host forms above the cutoff), (2) k > 32 -> SEQUENCE_TOO_LONG (value = k), (3) the layout's size limits
 * (those of bitnuc_reads_edist_best* / _best_batch*: UNSUPPORTED), (4) n_queries > BITNUC_MAX_QUERIES -> UNSUPPORTED (value = n_queries), (5) anchor neither
 * BITNUC_ANCHOR_START nor BITNUC_ANCHOR_END -> UNSUPPORTED (value = anchor), (6) count == 0 -> OK, nothing written, (7) query, end or start NULL or not
 * 4-byte aligned, queries NULL with n_queries > 0 or not 8-byte aligned (patterns: 4-byte), an offsets table NULL or not 8-byte aligned -> UNSUPPORTED,
 * (8) ragged host forms: the tables' validation, as in bitnuc_reads_hdist_best_batch*, (9) with k >= 1 and n_queries >= 1: reads / words NULL (words not
 * 8-byte aligned) -> UNSUPPORTED.  Nothing is written on an argument error.
 * The _async forms have the _dev contract of their family (device pointers for everything, the context's stream, no host synchronisation but the growth of
 * context scratch; the ragged forms TRUST their tables) and can be captured into a hipGraph after a warm-up with the same or larger n_queries; reads,
 * queries, query[] and end[] are read at every replay.  Context scratch: 16 bytes per query, in the per-read family's table slot under the same growth rule
 * -- the forward call and this call share it in stream order.  The host forms are synchronous and judge count x 2k (saturated) against the host cutoff:
 * below it they run on the host (ctx may be NULL), above it through the context in the layout's chunks of whole reads, with the chunk's query / end staged
 * in and its start / dist staged out; INVALID_BASE indices stay absolute.
 *
 * ALONG A REFERENCE -- bitnuc_ref_edist_start[_packed], each _async and host, and the bitnuc_ref_pattern_edist_start* twins (bitnuc_ref_*, not
 * bitnuc_kmer_*: those 56 names are the SEARCHES along a reference, one family of arguments and checks; these calls take items).  The text is the reference
 * (ref, n | words, n_words, n), the floor is 0.  m items: query_index[i] (NULL: every item belongs to query 0 -- the hit list's case; after _best pass
 * 0 .. n_queries - 1), end[i] (64-bit), start[i] (64-bit), dist[i] (may be NULL).  end and start are 8-byte aligned, query_index 4-byte aligned.  d_m (the
 * _async forms only) is NULL or a DEVICE count: only the items below min(m, *d_m) are processed and written, nothing at or beyond it is touched -- so
 * bitnuc_kmer_edist_hits*_async with d_n_hits, followed by this call with m = cap and d_m = d_n_hits, is one capturable chain with no host round trip.
 * Checks, in order: (1) ctx (_async forms only), (2) k > 32 -> SEQUENCE_TOO_LONG (value = k), (3) packed: n_words < ceil(n / 32) -> INVALID_LENGTH (value =
 * n), (4) m == 0 -> OK, nothing written, (5) n_queries > BITNUC_MAX_QUERIES -> UNSUPPORTED (value = n_queries), (6) end or start NULL or not 8-byte aligned,
 * query_index not 4-byte aligned, d_m not 8-byte aligned, queries NULL with n_queries > 0 or not 8-byte aligned (patterns: 4-byte) -> UNSUPPORTED, (7) with
 * k >= 1 and n_queries >= 1: a NULL reference, or packed words not 8-byte aligned -> UNSUPPORTED.  Nothing is written on an argument error.
 * The _async forms: the _dev contract; 16 bytes per query of context scratch in the slot the searches along a reference keep their tables in; capturable
 * after a warm-up with the same or larger n_queries.  The HOST forms always run on the host (ctx is not used and may be NULL): an item reads at most 63
 * bases, so moving a reference to the device would cost more than the work.
 * Cost: a vector-ALU kernel, ONE ITEM PER LANE: the lane loads its own query's 16-byte table entry, reverses the four masks within k bits, gathers its w
 * bases as the anchored kernel gathers a span, and runs at most 63 steps of the recurrence; the loop is wave-uniform over the wave's largest w with Eq
 * forced to 0 behind a lane's own w, and a wave of equal w runs the unmasked loop.  No LDS, no atomics but the invalid-byte latch.  Measured on 6,666,667
 * reads (10^9 bases), one MI355X (profiles/r24_edist_start.json), ASCII / packed, against bitnuc_reads_edist_anchored*_async with one query and span 2k - 1
 * on the same reads: k = 16: 0.29 / 0.16 ms (0.85 / 1.20 x), k = 31: 0.42 / 0.30 ms (0.82 / 1.15 x); behind a forward call of 64 queries the start adds 0.6 -
 * 4.8 %, behind a hit list along 10^9 bases 0.9 - 1.9 %.
 * Out of scope: a CIGAR or edit script, collapsing hit runs to local minima, k > 32, affine gaps, reverse-complement queries. */
int bitnuc_reads_edist_start_async(bitnuc_ctx *ctx, const uint8_t *d_reads, size_t read_len, size_t count, size_t k, int anchor, size_t pos, const uint64_t *d_queries,
                                   size_t n_queries, const uint32_t *d_query, const uint32_t *d_end, uint32_t *d_start, uint8_t *d_dist, bitnuc_err *err);
int bitnuc_reads_edist_start_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, size_t read_len, size_t count, size_t k, int anchor, size_t pos, const uint64_t
                                          *d_queries, size_t n_queries, const uint32_t *d_query, const uint32_t *d_end, uint32_t *d_start, uint8_t *d_dist, bitnuc_err
                                          *err);
int bitnuc_reads_edist_start_batch_async(bitnuc_ctx *ctx, const uint8_t *d_seq, const uint64_t *d_offsets, size_t count, size_t total_bases, size_t k, int anchor, size_t
                                         pos, const uint64_t *d_queries, size_t n_queries, const uint32_t *d_query, const uint32_t *d_end, uint32_t *d_start, uint8_t
                                         *d_dist, bitnuc_err *err);
int bitnuc_reads_edist_start_batch_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, const uint64_t *d_word_offsets, const uint64_t *d_offsets, size_t count, size_t
                                                total_words, size_t k, int anchor, size_t pos, const uint64_t *d_queries, size_t n_queries, const uint32_t *d_query, const
                                                uint32_t *d_end, uint32_t *d_start, uint8_t *d_dist, bitnuc_err *err);
int bitnuc_reads_edist_start(bitnuc_ctx *ctx, const uint8_t *reads, size_t read_len, size_t count, size_t k, int anchor, size_t pos, const uint64_t *queries, size_t
                             n_queries, const uint32_t *query, const uint32_t *end, uint32_t *start, uint8_t *dist, bitnuc_err *err);
int bitnuc_reads_edist_start_packed(bitnuc_ctx *ctx, const uint64_t *words, size_t read_len, size_t count, size_t k, int anchor, size_t pos, const uint64_t *queries,
                                    size_t n_queries, const uint32_t *query, const uint32_t *end, uint32_t *start, uint8_t *dist, bitnuc_err *err);
int bitnuc_reads_edist_start_batch(bitnuc_ctx *ctx, const uint8_t *seq, const uint64_t *offsets, size_t count, size_t k, int anchor, size_t pos, const uint64_t *queries,
                                   size_t n_queries, const uint32_t *query, const uint32_t *end, uint32_t *start, uint8_t *dist, bitnuc_err *err);
int bitnuc_reads_edist_start_batch_packed(bitnuc_ctx *ctx, const uint64_t *words, const uint64_t *word_offsets, const uint64_t *offsets, size_t count, size_t k, int
                                          anchor, size_t pos, const uint64_t *queries, size_t n_queries, const uint32_t *query, const uint32_t *end, uint32_t *start,
                                          uint8_t *dist, bitnuc_err *err);
/* the pattern twins */
int bitnuc_reads_pattern_edist_start_async(bitnuc_ctx *ctx, const uint8_t *d_reads, size_t read_len, size_t count, size_t k, int anchor, size_t pos, const bitnuc_pattern
                                           *d_patterns, size_t n_queries, const uint32_t *d_query, const uint32_t *d_end, uint32_t *d_start, uint8_t *d_dist, bitnuc_err
                                           *err);
int bitnuc_reads_pattern_edist_start_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, size_t read_len, size_t count, size_t k, int anchor, size_t pos, const
                                                  bitnuc_pattern *d_patterns, size_t n_queries, const uint32_t *d_query, const uint32_t *d_end, uint32_t *d_start, uint8_t
                                                  *d_dist, bitnuc_err *err);
int bitnuc_reads_pattern_edist_start_batch_async(bitnuc_ctx *ctx, const uint8_t *d_seq, const uint64_t *d_offsets, size_t count, size_t total_bases, size_t k, int anchor,
                                                 size_t pos, const bitnuc_pattern *d_patterns, size_t n_queries, const uint32_t *d_query, const uint32_t *d_end, uint32_t
                                                 *d_start, uint8_t *d_dist, bitnuc_err *err);
int bitnuc_reads_pattern_edist_start_batch_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, const uint64_t *d_word_offsets, const uint64_t *d_offsets, size_t count,
                                                        size_t total_words, size_t k, int anchor, size_t pos, const bitnuc_pattern *d_patterns, size_t n_queries, const
                                                        uint32_t *d_query, const uint32_t *d_end, uint32_t *d_start, uint8_t *d_dist, bitnuc_err *err);
int bitnuc_reads_pattern_edist_start(bitnuc_ctx *ctx, const uint8_t *reads, size_t read_len, size_t count, size_t k, int anchor, size_t pos, const bitnuc_pattern
                                     *patterns, size_t n_queries, const uint32_t *query, const uint32_t *end, uint32_t *start, uint8_t *dist, bitnuc_err *err);
int bitnuc_reads_pattern_edist_start_packed(bitnuc_ctx *ctx, const uint64_t *words, size_t read_len, size_t count, size_t k, int anchor, size_t pos, const bitnuc_pattern
                                            *patterns, size_t n_queries, const uint32_t *query, const uint32_t *end, uint32_t *start, uint8_t *dist, bitnuc_err *err);
int bitnuc_reads_pattern_edist_start_batch(bitnuc_ctx *ctx, const uint8_t *seq, const uint64_t *offsets, size_t count, size_t k, int anchor, size_t pos, const
                                           bitnuc_pattern *patterns, size_t n_queries, const uint32_t *query, const uint32_t *end, uint32_t *start, uint8_t *dist,
                                           bitnuc_err *err);
int bitnuc_reads_pattern_edist_start_batch_packed(bitnuc_ctx *ctx, const uint64_t *words, const uint64_t *word_offsets, const uint64_t *offsets, size_t count, size_t k,
                                                  int anchor, size_t pos, const bitnuc_pattern *patterns, size_t n_queries, const uint32_t *query, const uint32_t *end,
                                                  uint32_t *start, uint8_t *dist, bitnuc_err *err);
/* ... along a reference */
int bitnuc_ref_edist_start_async(bitnuc_ctx *ctx, const uint8_t *d_ref, size_t n, size_t k, const uint64_t *d_queries, size_t n_queries, const uint32_t *d_query_index,
                                  const uint64_t *d_end, size_t m, const uint64_t *d_m, uint64_t *d_start, uint8_t *d_dist, bitnuc_err *err);
int bitnuc_ref_edist_start_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, size_t n_words, size_t n, size_t k, const uint64_t *d_queries, size_t n_queries, const
                                         uint32_t *d_query_index, const uint64_t *d_end, size_t m, const uint64_t *d_m, uint64_t *d_start, uint8_t *d_dist, bitnuc_err
                                         *err);
int bitnuc_ref_edist_start(bitnuc_ctx *ctx, const uint8_t *ref, size_t n, size_t k, const uint64_t *queries, size_t n_queries, const uint32_t *query_index, const
                            uint64_t *end, size_t m, uint64_t *start, uint8_t *dist, bitnuc_err *err);
int bitnuc_ref_edist_start_packed(bitnuc_ctx *ctx, const uint64_t *words, size_t n_words, size_t n, size_t k, const uint64_t *queries, size_t n_queries, const uint32_t
                                   *query_index, const uint64_t *end, size_t m, uint64_t *start, uint8_t *dist, bitnuc_err *err);
/* the pattern twins */
int bitnuc_ref_pattern_edist_start_async(bitnuc_ctx *ctx, const uint8_t *d_ref, size_t n, size_t k, const bitnuc_pattern *d_patterns, size_t n_queries, const uint32_t
                                          *d_query_index, const uint64_t *d_end, size_t m, const uint64_t *d_m, uint64_t *d_start, uint8_t *d_dist, bitnuc_err *err);
int bitnuc_ref_pattern_edist_start_packed_async(bitnuc_ctx *ctx, const uint64_t *d_words, size_t n_words, size_t n, size_t k, const bitnuc_pattern *d_patterns, size_t
                                                 n_queries, const uint32_t *d_query_index, const uint64_t *d_end, size_t m, const uint64_t *d_m, uint64_t *d_start,
                                                 uint8_t *d_dist, bitnuc_err *err);
int bitnuc_ref_pattern_edist_start(bitnuc_ctx *ctx, const uint8_t *ref, size_t n, size_t k, const bitnuc_pattern *patterns, size_t n_queries, const uint32_t
                                    *query_index, const uint64_t *end, size_t m, uint64_t *start, uint8_t *dist, bitnuc_err *err);
int bitnuc_ref_pattern_edist_start_packed(bitnuc_ctx *ctx, const uint64_t *words, size_t n_words, size_t n, size_t k, const bitnuc_pattern *patterns, size_t n_queries,
                                           const uint32_t *query_index, const uint64_t *end, size_t m, uint64_t *start, uint8_t *dist, bitnuc_err *err);

/* ---- analysis on packed words (the callers just above the codec) ------ */
/* BaseCount::base_counts / GCContent::gc_content of a packed sequence
 * (src/utils/analysis.rs:7-39: the reference decodes to ASCII, then counts bytes): counts[] =
 * {A, C, G, T} of the first n_bases bases.  n_words < ceil(n_bases/32) -> INVALID_LENGTH.
 * gc_content = (counts[1] + counts[2]) as f64 / n_bases as f64 * 100.0 is left to the caller. */
int bitnuc_base_counts(bitnuc_ctx *ctx, const uint64_t *words, size_t n_words, size_t n_bases, uint64_t counts[4], bitnuc_err *err);
int bitnuc_base_counts_dev(bitnuc_ctx *ctx, const uint64_t *d_words, size_t n_words, size_t n_bases, uint64_t *d_counts /* 4, device */, bitnuc_err *err);
/* Many-pair / one-query Hamming distance of packed <=32-mers: dist[i] = hdist_scalar(a[i], b[i], len)
 * or hdist_scalar(query, targets[i], len) (src/utils/functions/hamming/scalar.rs:11-48).
 * len > 32 -> INVALID_LENGTH(len). */
int bitnuc_hdist_pairs_dev(bitnuc_ctx *ctx, const uint64_t *d_a, const uint64_t *d_b, size_t count, size_t len, uint8_t *d_dist, bitnuc_err *err);
int bitnuc_hdist_query_dev(bitnuc_ctx *ctx, uint64_t query, const uint64_t *d_targets, size_t count, size_t len, uint8_t *d_dist, bitnuc_err *err);
int bitnuc_hdist_pairs(bitnuc_ctx *ctx, const uint64_t *a, const uint64_t *b, size_t count, size_t len, uint8_t *dist, bitnuc_err *err);
int bitnuc_hdist_query(bitnuc_ctx *ctx, uint64_t query, const uint64_t *targets, size_t count, size_t len, uint8_t *dist, bitnuc_err *err);

/* ---- split_packed ----------------------------------------------------- */
/* split_packed(ebuf, slen, idx, &mut lbuf, &mut rbuf)   src/utils/functions/split.rs:15-99
 * Cut a packed sequence of slen bases at base idx (idx goes to the right part).
 * idx > slen -> INDEX_OUT_OF_BOUNDS{err.index = idx, err.value = slen} (split.rs:23-28).
 * flags:
 *   BITNUC_SPLIT_AS_WRITTEN  the reference's output, word for word: idx == 0 -> right = ebuf;
 *       idx == slen -> left = ebuf; otherwise left = ebuf[..idx/32] + the masked split word
 *       (idx/32 + 1 words, a zero word when idx % 32 == 0) and right = n_words - idx/32 words,
 *       right[j] = ebuf[idx/32 + j] >> s | ebuf[idx/32 + j - 1] << (64 - s), s = 2*(idx % 32)
 *       (split.rs:84-94 ORs in the low bits of the PREVIOUS word, so a right part longer than
 *       one word is not the shifted sequence unless s == 0; the reference's tests only cover
 *       one-word right parts and s == 0).
 *   BITNUC_SPLIT_CANONICAL   the funnel shift the function documents: left == encode(seq[..idx])
 *       (ceil(idx/32) words) and right == encode(seq[idx..]) (ceil((slen-idx)/32) words), bits
 *       above the last base cleared.  Agrees with AS_WRITTEN (up to trailing words / the zero
 *       word) wherever the reference's own tests look.
 * n_words < ceil(slen/32) -> INVALID_LENGTH(slen) (the reference panics or returns a
 * data-dependent length there).  lbuf / rbuf must not overlap ebuf.  _sizes returns the word
 * counts a call will write; the host form returns them too. */
#define BITNUC_SPLIT_AS_WRITTEN 0
#define BITNUC_SPLIT_CANONICAL 1
int bitnuc_split_packed_sizes(size_t n_words, size_t slen, size_t idx, int flags, size_t *n_left, size_t *n_right, bitnuc_err *err);
int bitnuc_split_packed(bitnuc_ctx *ctx, const uint64_t *ebuf, size_t n_words, size_t slen, size_t idx, int flags, uint64_t *lbuf, size_t *n_left, uint64_t *rbuf, size_t *n_right, bitnuc_err *err);
int bitnuc_split_packed_dev(bitnuc_ctx *ctx, const uint64_t *d_ebuf, size_t n_words, size_t slen, size_t idx, int flags, uint64_t *d_lbuf, uint64_t *d_rbuf, bitnuc_err *err);

/* ---- multi-GPU: shard + concatenate (BASELINE config 4) ------------------------------------ */
/* u64 words never share state (packing/avx.rs:138-145 has no carry), so a sequence split at
 * multiples of 32 bases encodes shard by shard with no communication; the only exchange is the
 * optional concatenation of the packed words, one RCCL all-gather over xGMI.  A communicator
 * rank is bound to one context (one device + stream).  librccl.so is loaded on first use.
 *   - one process (or thread) per GPU: rank 0 calls bitnuc_comm_get_unique_id, hands the 128 bytes to the
 *     other ranks (env, file, MPI, torch.distributed ...), every rank calls bitnuc_comm_init_rank and then
 *     the per-rank entry points (bitnuc_allgather_words_dev, bitnuc_encode_sharded_allgather_dev,
 *     bitnuc_encode_sharded_allgather_overlapped_dev), EACH RANK FROM ITS OWN THREAD OR PROCESS: like every
 *     collective they complete only when all ranks have called them, and RCCL may block the calling thread
 *     until its peers have;
 *   - one thread, all GPUs: bitnuc_comm_init_all[_devices] creates n contexts + communicators at once; that
 *     thread then drives all ranks with the _all entry points (bitnuc_encode_sharded_allgather_all,
 *     bitnuc_encode_sharded_allgather_overlapped_all), which issue every rank's part of an exchange inside one
 *     ncclGroupStart / ncclGroupEnd.  The per-rank entry points REFUSE such a communicator of more than one
 *     rank (BITNUC_UNSUPPORTED): called rank after rank from the one thread, the first call would wait for
 *     peers that thread has not reached yet.  bitnuc_comm_single_process() tells the two kinds apart. */
typedef struct bitnuc_comm bitnuc_comm;
#define BITNUC_UNIQUE_ID_BYTES 128
int bitnuc_comm_get_unique_id(uint8_t id[BITNUC_UNIQUE_ID_BYTES], bitnuc_err *err);
int bitnuc_comm_init_rank(bitnuc_ctx *ctx, int nranks, int rank, const uint8_t id[BITNUC_UNIQUE_ID_BYTES], bitnuc_comm **out, bitnuc_err *err);
int bitnuc_comm_init_all(int n_gpus, bitnuc_ctx **ctxs /* out: n_gpus */, bitnuc_comm **comms /* out: n_gpus */, bitnuc_err *err);
/* ... on the HIP devices devices[0..n_gpus) instead of 0..n_gpus-1 (rank i on devices[i]; NULL = the identity). */
int bitnuc_comm_init_all_devices(int n_gpus, const int *devices, bitnuc_ctx **ctxs, bitnuc_comm **comms, bitnuc_err *err);
void bitnuc_comm_destroy(bitnuc_comm *comm);
int bitnuc_comm_nranks(const bitnuc_comm *comm);
int bitnuc_comm_rank(const bitnuc_comm *comm);
/* 1: made by bitnuc_comm_init_all[_devices] (use the _all entry points), 0: by bitnuc_comm_init_rank, -1: NULL. */
int bitnuc_comm_single_process(const bitnuc_comm *comm);
/* All-gather `count` packed words per rank: d_all[r*count .. (r+1)*count) = rank r's d_local.
 * d_local may alias d_all + rank*count (in place).  Asynchronous on the context's stream. */
int bitnuc_allgather_words_dev(bitnuc_ctx *ctx, bitnuc_comm *comm, const uint64_t *d_local, size_t count, uint64_t *d_all, bitnuc_err *err);
/* Encode this rank's shard (shard_len bases, the same multiple of 32 on every rank) straight
 * into its slot of d_all and all-gather in place: every rank ends with the packed words of the
 * whole nranks*shard_len-base sequence, bit-identical to a single-GPU encode of it. */
int bitnuc_encode_sharded_allgather_dev(bitnuc_ctx *ctx, bitnuc_comm *comm, const uint8_t *d_seq_shard, size_t shard_len, uint64_t *d_all, bitnuc_err *err);
/* The same result with the exchange hidden behind the encode (SURVEY 8e iii): the shard is encoded in
 * n_chunks pieces on the context's stream while a second stream moves each finished piece IN PLACE
 * (grouped ncclSend / ncclRecv straight into d_all + peer*count + w0: no staging buffer, no strided copy;
 * BITNUC_GATHER_MODE=bcast uses grouped in-place ncclBroadcast instead).  The context's stream waits for
 * the exchange, so bitnuc_ctx_sync() covers the whole call; an InvalidBase index is relative to the shard. */
int bitnuc_encode_sharded_allgather_overlapped_dev(bitnuc_ctx *ctx, bitnuc_comm *comm, const uint8_t *d_seq_shard, size_t shard_len, int n_chunks, uint64_t *d_all, bitnuc_err *err);
/* Single-process forms over bitnuc_comm_init_all's contexts and communicators (all n of them, in rank order):
 * one call drives all n GPUs and synchronises every stream before it returns.  _all: encode on every device,
 * then one grouped ncclAllGather.  _overlapped_all: the chunked in-place exchange above -- per piece, the encode
 * on every device's stream, then ONE group holding every rank's sends and receives on that rank's transfer stream.
 * An InvalidBase is reported for the lowest rank that has one: err.index relative to that rank's shard,
 * err.value = the rank; the other ranks' slots are still exchanged. */
int bitnuc_encode_sharded_allgather_all(int n_gpus, bitnuc_ctx **ctxs, bitnuc_comm **comms, const uint8_t *const *d_seq_shards, size_t shard_len, uint64_t *const *d_alls, bitnuc_err *err);
int bitnuc_encode_sharded_allgather_overlapped_all(int n_gpus, bitnuc_ctx **ctxs, bitnuc_comm **comms, const uint8_t *const *d_seq_shards, size_t shard_len, int n_chunks, uint64_t *const *d_alls, bitnuc_err *err);

/* ---- a RAGGED BATCH across ranks ("for a batch of independent sequences of unequal length the partition is by whole
 * sequences with an offsets table; the final word of each sequence is padded independently" -- packing/avx.rs:147-148 is that
 * padding rule, src/utils/mod.rs:22-25 the per-sequence loop the batch replaces).
 * bitnuc_batch_shard_ranges: host arithmetic only, no device.  Sequence i holds bases [offsets[i], offsets[i+1]) and packs into
 * ceil(len / 32) words of its own.  Rank r of nranks gets the run of WHOLE sequences [seq_first[r], seq_first[r+1]), balanced by
 * word count: seq_first[r] = the first i whose word prefix W[i] >= floor(r * W[count] / nranks) (so a sequence longer than a fair
 * share stays whole and the ranks it covers get empty runs; seq_first[0] = 0, seq_first[nranks] = count).  word_first[r] =
 * W[seq_first[r]] = where rank r's words start in the concatenation; word_first[nranks] = the batch's total words.
 * Each rank then rebases its run's offsets to 0 and encodes it with the batch entry points above (bitnuc_batch_plan_build_dev +
 * bitnuc_encode_batch_plan_dev) straight into d_all + word_first[rank]; the global word_offsets table is word_first[rank] + the
 * rank's own table. */
int bitnuc_batch_shard_ranges(const uint64_t *offsets /* count+1 */, size_t count, int nranks, size_t *seq_first /* nranks+1 */, uint64_t *word_first /* nranks+1 */, bitnuc_err *err);
/* All-gather of UNEQUAL word counts, in place: counts[r] words of rank r live at d_all + sum(counts[0..r)) on rank r before the
 * call and on every rank after it (grouped ncclSend / ncclRecv with per-peer counts on the context's stream -- all P-1 links of a
 * GPU at once; BITNUC_GATHER_MODE=bcast: one grouped in-place ncclBroadcast per non-empty rank).  counts must be the same array
 * on every rank; a rank with counts[r] == 0 sends nothing.  Asynchronous like every _dev call. */
int bitnuc_allgatherv_words_dev(bitnuc_ctx *ctx, bitnuc_comm *comm, const size_t *counts /* nranks */, uint64_t *d_all, bitnuc_err *err);
/* ... for a thread that holds every rank (bitnuc_comm_init_all[_devices]): one group with every rank's sends and receives, then
 * every stream is synchronised (a data error latched by the encodes queued before it is reported like the other _all forms). */
int bitnuc_allgatherv_words_all(int n_gpus, bitnuc_ctx **ctxs, bitnuc_comm **comms, const size_t *counts /* n_gpus */, uint64_t *const *d_alls, bitnuc_err *err);
/* A communicator made by bitnuc_comm_init_all[_devices] is taken to be driven by ONE thread, and the per-rank entry points refuse
 * it (they would block in RCCL waiting for peers that thread has not issued).  A host that gives every rank of such a communicator
 * its own thread -- ordinary NCCL usage -- says so here (threaded = 1) and may then use the per-rank entry points; the _all forms
 * refuse the communicator from then on.  Returns the previous setting, -1 for NULL. */
int bitnuc_comm_set_threaded(bitnuc_comm *comm, int threaded);

/* xGMI link probe (no reference counterpart; SURVEY section 5 asks for the measured per-link rate before any
 * fabric fraction is quoted): hipMemcpyPeerAsync of `bytes` from src_device to each of dst_devices[0..n), one
 * link at a time (gb_s_each[i], best of reps) and then all n at once (*gb_s_all, the aggregate outbound rate).
 * All devices must be visible in this process and peer-accessible; fewer than two devices -> BITNUC_UNSUPPORTED
 * with err.value = the device count. */
int bitnuc_peer_link_probe(int src_device, const int *dst_devices, int n, size_t bytes, int reps, double *gb_s_each, double *gb_s_all, bitnuc_err *err);

/* ---- synthetic input (the reference's tests use nucgen::Sequence::fill_buffer,
 * src/utils/mod.rs:116-121; its stream is unpinned, so the build ships its own) ---- */
/* Fill d_out[0..len) with bases first..first+len of the seeded stream
 * base(i) = "ACGT"[(splitmix64(seed + (i/32+1)*0x9E3779B97F4A7C15) >> 2*(i%32)) & 3];
 * flags bit0: the benches' cyclic "ACGT"[i%4] pattern (benches/simd_comparison.rs:4-7);
 * bit1: lower-case mix, p = 0.25 (SURVEY 8d parity variant): base i is lower case iff 2-bit field i%32 of
 * splitmix64((seed ^ 0xC0FFEE5EEDC0DE55) + (i/32+1)*0x9E3779B97F4A7C15) is zero. */
int bitnuc_nucgen_dev(bitnuc_ctx *ctx, uint8_t *d_out, size_t len, uint64_t seed, uint64_t first, int flags, bitnuc_err *err);

/* ---- tuning / diagnostics (not part of the drop-in surface) ---------------------- */
/* Knobs: key in {"force_gpu", "host_cutoff", "host_pipeline"} (see "Size dispatch"), kernel-variant
 * selectors {"encode", "decode", "grid_mult", ...} for experiments.  A negative value only queries.
 * Returns the previous value, -1 for an unknown key, -2 for a variant this build does not hold (the
 * product library ships 4 of the 47 encode/decode variants; libbitnuc_hip_sweep.so, built with
 * -DBITNUC_SWEEP_VARIANTS, holds all of them plus the ballot formulation). */
int bitnuc_ctx_set_variant(bitnuc_ctx *ctx, const char *key, int value);
/* Pure streaming kernels used to measure the box's HBM ceiling next to the codec:
 * mode bits 0-2: 0 = read-only sum of `bytes` from d_src; 1 = copy d_src -> d_dst;
 * 2 = write-only fill of d_dst; 3 = encode_kernel's access shape (16 B nt load + 4 B store per lane, 2 in
 * flight, 128-thread workgroups) and 4 = decode_kernel's (4 B load + 16 B nt store, 256-thread workgroups),
 * both without arithmetic, `bytes` = ASCII-side bytes.  bit 3: nt loads, bit 4: nt stores, bit 5: 2 (not 4)
 * 16-byte groups in flight per lane (modes 0-2). */
int bitnuc_stream_probe_dev(bitnuc_ctx *ctx, int mode, const void *d_src, void *d_dst, size_t bytes, bitnuc_err *err);

/* Mean ns per call of the HOST path (op 0 as_2bit, 1 from_2bit, 2 encode, 3 decode, 4 hdist_scalar) on n bases of the
 * reference's bench input (benches/simd_comparison.rs:4-7), timed inside the library over `iters` calls; < 0 = bad argument. */
double bitnuc_selftime_small(int op, size_t n, size_t iters);
/* Configuration of this context's pipelined host-pointer path (creates it if needed): out[0..n) = chunk_bases (bases per
 * chunk), depth (chunks in flight); 0.0 past them. */
int bitnuc_host_pipe_info(bitnuc_ctx *ctx, double *out, int n, bitnuc_err *err);

#ifdef __cplusplus
}
#endif
#endif /* BITNUC_HIP_H */
