// reads_batch_host.h -- the best match per read of a RAGGED batch on the host (bitnuc_reads_hdist_best_batch / _batch_packed below the cutoff), the
// validation of the two offsets tables and the cut of a batch into chunks of whole reads.  Plain C++ (no HIP):
// tests/c/reads_batch_host_sanitize.cpp runs them under ASan + UBSan.  Written once for both kinds of query (reads_best_window).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "reads_best_host.h" // reads_best_window, reads_best_fill

namespace bitnuc_host {

inline size_t batch_words_for(uint64_t n_bases) { return (size_t)(n_bases / 32 + (n_bases % 32 != 0)); }

// What is wrong with a batch's tables, in the order the calls report it.  kind: 0 nothing; 1 offsets decrease at entry `value` (encode_batch's report);
// 2 offsets[0] != 0 (value 0); 3 word_offsets is not encode_batch's table for these offsets, first at entry `value` (decode_batch's report);
// 4 read `value`-long is too long (2^32 - 1 bases or more); 5 the batch is too long (`value` = total bases: 2^58 or more, or as many windows of words).
struct BatchFault { int kind; uint64_t value; };
inline BatchFault batch_check_tables(const uint64_t *offsets, const uint64_t *word_offsets, size_t count) {
    for (size_t i = 0; i < count; ++i)
        if (offsets[i + 1] < offsets[i]) return BatchFault{1, (uint64_t)i + 1};
    if (offsets[0] != 0) return BatchFault{2, 0};
    if (word_offsets) {
        if (word_offsets[0] != 0) return BatchFault{3, 0};
        for (size_t i = 0; i < count; ++i)
            if (word_offsets[i + 1] < word_offsets[i] || word_offsets[i + 1] - word_offsets[i] != batch_words_for(offsets[i + 1] - offsets[i]))
                return BatchFault{3, (uint64_t)i + 1};
    }
    for (size_t i = 0; i < count; ++i)
        if (offsets[i + 1] - offsets[i] >= 0xFFFFFFFFull) return BatchFault{4, offsets[i + 1] - offsets[i]};
    constexpr uint64_t kLimit = (uint64_t)1 << 58;
    if (offsets[count] >= kLimit || (word_offsets && word_offsets[count] >= kLimit / 32)) return BatchFault{5, offsets[count]};
    return BatchFault{0, 0};
}

// the windows of a batch, saturated: the sum over the reads of max(0, len - k + 1) (k >= 1)
inline size_t batch_windows(const uint64_t *offsets, size_t count, size_t k) {
    size_t total = 0;
    for (size_t r = 0; r < count; ++r) {
        const uint64_t len = offsets[r + 1] - offsets[r];
        if (len < k) continue;
        const size_t w = (size_t)(len - k + 1);
        total = total + w < total ? (size_t)-1 : total + w;
    }
    return total;
}

// The chunk of whole reads that starts at read r0: the longest run whose size(r0, r1) fits `budget`, at least one read.  size(r0, r1): what the reads
// [r0, r1) occupy (bases or words; it does not decrease in r1).
template <class Size>
inline size_t batch_chunk_end(size_t r0, size_t count, uint64_t budget, Size size) {
    size_t lo = r0 + 1, hi = count; // the largest r1 in [r0 + 1, count] with size(r0, r1) <= budget, or r0 + 1
    if (size(r0, lo) > budget) return lo;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo + 1) / 2;
        if (size(r0, mid) <= budget) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// packed reads behind validated tables (1 <= k <= 32, nq >= 1); the bits above a read's last base are never part of a window
template <class Q>
static inline void reads_hdist_best_batch_packed_small(const uint64_t *words, const uint64_t *word_offsets, const uint64_t *offsets, size_t count, size_t k,
                                                       const Q *queries, size_t nq, uint32_t *query, uint32_t *pos, uint8_t *dist) {
    reads_best_fill(count, query, pos, dist);
    for (size_t r = 0; r < count; ++r) {
        const size_t len = (size_t)(offsets[r + 1] - offsets[r]);
        for (size_t i = 0; i + k <= len; ++i)
            reads_best_window(packed_window(words + word_offsets[r], i, k), i, k, queries, nq, query + r, pos + r, dist + r);
    }
}

// back-to-back ASCII reads behind a validated table (offsets[0] == 0; 1 <= k <= 32, nq >= 1): -1 with the outputs written, or the index of the first
// invalid byte of seq[0 .. offsets[count]) (outputs untouched) -- every byte counts, also those of reads too short for a window
template <class Q>
static inline long long reads_hdist_best_batch_small(const uint8_t *seq, const uint64_t *offsets, size_t count, size_t k, const Q *queries, size_t nq,
                                                     uint32_t *query, uint32_t *pos, uint8_t *dist) {
    for (size_t i = 0; i < (size_t)offsets[count]; ++i) {
        const unsigned u = seq[i] & 0xDFu;
        if (u != 'A' && u != 'C' && u != 'G' && u != 'T') return (long long)i;
    }
    reads_best_fill(count, query, pos, dist);
    for (size_t r = 0; r < count; ++r) {
        const uint8_t *s = seq + offsets[r];
        const size_t len = (size_t)(offsets[r + 1] - offsets[r]);
        uint64_t w = 0;
        for (size_t i = 0; i < len; ++i) {
            const uint64_t code = ((s[i] >> 1) ^ (s[i] >> 2)) & 3u; // A 0, C 1, G 2, T 3, either case
            w = (w >> 2) | (code << (2 * (k - 1)));                  // window i + 1 - k, base b at bits 2 b
            if (i + 1 >= k) reads_best_window(w, i + 1 - k, k, queries, nq, query + r, pos + r, dist + r);
        }
    }
    return -1;
}

} // namespace bitnuc_host
