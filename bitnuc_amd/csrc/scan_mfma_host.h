// scan_mfma_host.h -- the host side of the matrix-core scan and count (scan_mfma_device.h): the query's operand tables the kernels take
// as arguments, and the query's bit-planes of the bit-plane scan.  Plain C++ (no HIP): tests/c/host_sanitize.cpp runs the builders
// under AddressSanitizer / UndefinedBehaviorSanitizer.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

// The three-channel count's table builders (Count3Rule, count3_mfma_table, count3_packed_table) run on the host for the single-query counts and on the
// device for the multi-query counts (scan_multi_device.h builds one table per query in-stream): one source for both.  Plain g++ sees nothing.
#if defined(__HIP__)
#define BITNUC_HD __host__ __device__
#else
#define BITNUC_HD
#endif

namespace bitnuc_dev {
struct CountMfmaTable { uint32_t w[40][16]; float c[4]; }; // c[r & 3]: where result register r's accumulator starts
struct Count3MfmaTable { uint32_t w[64][12]; float c[4]; };
struct PackedScanTable { uint32_t w[34][16]; float c[4]; }; // w[m - 2 h + 2]: the packed scan's rows only depend on m - 2 h (scan_packed_table)
constexpr int kBestRows = 40;                             // rows of a best-match table: CountMfmaTable's 40 (ASCII), PackedScanTable's 34 (packed)
struct BestTable { uint32_t w[kBestRows][16]; };           // one query's operand rows of the best-match kernels (scan_best_device.h); no start values
// A pattern query: position i < k accepts the SET S_i of bases, allow[c] bit i set <=> base code c (A 0, C 1, G 2, T 3) is in S_i; bits at positions >= k are
// ignored.  The layout of bitnuc_pattern (include/bitnuc_hip.h).  An exact query is the pattern of singletons (pattern_of_2bit).
struct PatternSets { uint32_t allow[4]; };
BITNUC_HD inline PatternSets pattern_of_2bit(uint64_t query, size_t k) {
    PatternSets p = {{0u, 0u, 0u, 0u}};
    for (size_t i = 0; i < k && i < 32; ++i) p.allow[(query >> (2 * i)) & 3] |= 1u << i;
    return p;
}
BITNUC_HD inline bool pattern_has(const PatternSets &p, unsigned c, int i) { return (p.allow[c] >> i) & 1u; }
} // namespace bitnuc_dev

namespace bitnuc_dev {
// Whole rounds of 1024 windows in n bases whose first `skip` are left to the tail threads: round r reads bases [skip + 1024 r, skip + 1024 r + 1056).
// constexpr: the launchers and the kernels both call it.
constexpr unsigned long long scan_rounds(unsigned long long n, unsigned skip = 0) {
    const unsigned long long nr = n > skip ? n - skip : 0; // the bases the rounds see
    return nr >= 1056 ? (nr - 32) >> 10 : 0;
}
} // namespace bitnuc_dev

namespace bitnuc_host {
using bitnuc_dev::CountMfmaTable;
using bitnuc_dev::Count3MfmaTable;
using bitnuc_dev::PackedScanTable;
using bitnuc_dev::PatternSets;
using bitnuc_dev::pattern_of_2bit;
using bitnuc_dev::pattern_has;

// The accumulators of the distance pack and of the thresholded count start at 2^23 (plus their fields): the integer results then sit in the low mantissa
// bits (scan_mfma_device.h: dist_row_scale, count_row_scale).
constexpr float kPackBias = 8388608.f;

// de-interleave a packed query into its two bit-planes (bit i = low / high code bit of base i)
inline void query_planes(uint64_t query, size_t k, uint32_t *ql, uint32_t *qh) {
    *ql = *qh = 0;
    for (unsigned i = 0; i < k; ++i) {
        *ql |= (uint32_t)((query >> (2 * i)) & 1) << i;
        *qh |= (uint32_t)((query >> (2 * i + 1)) & 1) << i;
    }
}

// The query's operand of the segment tiling with four channels per base (CountMfmaTable below; the shipped scan, the four-channel count of the
// evidence build): row m of K-block h only depends on delta = m - 8 h.
// thresholded (kmer_count_mfma_kernel's EMIT 1, 2): result register r (rows with m & 3 = r & 3 = j) must end at 2^23 + (32 + tau - d) 2^(6 j) for j < 3 and at
// 2 d - 2 tau - 1 for j = 3 (scan_mfma_device.h).  match = false: the entries mark the channels that DIFFER from the query's base (-1.0 for j < 3, +1.0 for j = 3)
// and the accumulators start at 2^23 + (32 + tau) 2^(6 j) / -(2 tau + 1).  match = true: they mark the channel that EQUALS it (+1.0 / -1.0: a third of the non-zero
// entries), d = k - matches, and the accumulators start at 2^23 + (32 + tau - k) 2^(6 j) / 2 k - 2 tau - 1.  A threshold no window can miss (tau >= k) gets the
// all-zero table and the start values of tau = k: every field reads 32, every j = 3 result -1.
// (the rows and start values from the per-position bytes lo[32 + i] = channels (A, C), hi[32 + i] = channels (G, T) of query position i)
inline void count_mfma_rows(const uint8_t *lo, const uint8_t *hi, size_t k, CountMfmaTable *t, bool thresholded, unsigned tau, bool match) {
    const bool all = thresholded && tau >= k;
    const unsigned te = all ? (unsigned)k : tau; // tau < k <= 32 otherwise
    for (int j = 0; j < 4; ++j) {
        if (!thresholded) t->c[j] = 0.f;
        else if (j < 3) t->c[j] = kPackBias + (float)((match ? 32u + te - (unsigned)k : 32u + te) << (6 * j));
        else t->c[j] = match ? (float)(2 * (int)k - 2 * (int)te - 1) : -(float)(2 * te + 1);
    }
    if (all) for (int j = 0; j < 3; ++j) t->c[j] = kPackBias + (float)(32u << (6 * j)), t->c[3] = -1.f;
    for (int d = -8; d < 32; ++d)
        for (int j = 0; j < 4; ++j)
            for (int i = 0; i < 4; ++i) {
                const int p0 = 16 * j + 4 * (i >> 1); // position of byte 0 of this dword, relative to 32 n + 8 h
                const uint8_t *src = (i & 1) ? hi : lo;
                uint32_t w = 0;
                for (int b = 0; b < 4; ++b) w |= (uint32_t)src[32 + p0 + b - d] << (8 * b);
                // the sign bit of every non-zero nibble (0b0010 -> 0b1010) where the row counts DOWN: j < 3 with differing channels, j = 3 with equal ones
                if (thresholded && ((((d + 8) & 3) != 3) != match)) w |= w << 2;
                t->w[d + 8][4 * j + i] = w;
            }
}
inline void count_mfma_table(uint64_t query, size_t k, CountMfmaTable *t, bool thresholded = false, unsigned tau = 0, bool match = false) {
    uint8_t lo[128], hi[128]; // [32 + i]
    memset(lo, 0, sizeof lo);
    memset(hi, 0, sizeof hi);
    const bool all = thresholded && tau >= k;
    for (size_t i = 0; i < k && !all; ++i) {
        const unsigned q = (unsigned)((query >> (2 * i)) & 3);
        if (thresholded && match) {
            lo[32 + i] = (uint8_t)((q == 0 ? 0x02 : 0) | (q == 1 ? 0x20 : 0));
            hi[32 + i] = (uint8_t)((q == 2 ? 0x02 : 0) | (q == 3 ? 0x20 : 0));
        } else {
            lo[32 + i] = (uint8_t)((q != 0 ? 0x02 : 0) | (q != 1 ? 0x20 : 0));
            hi[32 + i] = (uint8_t)((q != 2 ? 0x02 : 0) | (q != 3 ? 0x20 : 0));
        }
    }
    count_mfma_rows(lo, hi, k, t, thresholded, tau, match);
}
// ... for a pattern: the entries mark the channels that are NOT in the position's set (the "differs" form; a set has no "equals" form: d = k - matches
// only holds for singletons).  count_mfma_table(pattern_of_2bit(q, k), ...) == count_mfma_table(q, ..., match = false), byte for byte.
inline void count_mfma_table(const PatternSets &p, size_t k, CountMfmaTable *t, bool thresholded = false, unsigned tau = 0) {
    uint8_t lo[128], hi[128]; // [32 + i]
    memset(lo, 0, sizeof lo);
    memset(hi, 0, sizeof hi);
    const bool all = thresholded && tau >= k;
    for (size_t i = 0; i < k && !all; ++i) {
        lo[32 + i] = (uint8_t)((pattern_has(p, 0, (int)i) ? 0 : 0x02) | (pattern_has(p, 1, (int)i) ? 0 : 0x20));
        hi[32 + i] = (uint8_t)((pattern_has(p, 2, (int)i) ? 0 : 0x02) | (pattern_has(p, 3, (int)i) ? 0 : 0x20));
    }
    count_mfma_rows(lo, hi, k, t, thresholded, tau, false);
}

// Row delta of count_mfma_table's plain (not thresholded) form, straight from the query: dword 4 j + i, byte b meets query base
// 16 j + 4 (i >> 1) + b - delta on channels (A, C) (i even) or (G, T) (i odd), 1.0 where the channel differs from the query's base.  The best-match
// kernels build their tables with it on the device, one thread per row (scan_best_device.h).
// A pattern marks the channels that are not in the position's set; an exact query is its pattern of singletons.
BITNUC_HD inline void scan_seg_row(const PatternSets &pat, size_t k, int delta, uint32_t *row) {
    for (int j = 0; j < 4; ++j)
        for (int i = 0; i < 4; ++i) {
            uint32_t w = 0;
            for (int b = 0; b < 4; ++b) {
                const int p = 16 * j + 4 * (i >> 1) + b - delta;
                if (p < 0 || p >= (int)k) continue;
                const unsigned lo = (i & 1) ? 2u : 0u, hi = lo + 1u; // (A, C) or (G, T)
                w |= ((pattern_has(pat, lo, p) ? 0u : 0x02u) | (pattern_has(pat, hi, p) ? 0u : 0x20u)) << (8 * b);
            }
            row[4 * j + i] = w;
        }
}
BITNUC_HD inline void scan_seg_row(uint64_t query, size_t k, int delta, uint32_t *row) { scan_seg_row(pattern_of_2bit(query, k), k, delta, row); }

// The three-channel code (A, C, G one-hot, T = 0) of both count tables (count3_mfma_table, count3_packed_table): d = #(q_i != T) + sum over the window
// of v(q_i, channel) x[channel], v = -1 on channel q for q in {A, C, G}, +1 on all three for q = T.  Rows with m & 3 < 3 carry -v and start at
// 2^23 + (32 + tau - #(q_i != T)) 2^(6 j) (they end at 32 + tau - d), rows with m & 3 = 3 carry v at scale 2 and start at 2 #(q_i != T) - 2 tau - 1.
// distance = true (evidence build's three-channel scan): every row carries v and starts at 2^23 + #(q_i != T) 2^(8 j) (j = 3: 2^23 + #): the product is d
// itself.  A threshold no window can miss (tau >= k) gets all-zero entries and the start values of an empty query (every field 32, every j = 3 result -1).
// For a PATTERN (position i accepts the set S_i) the mismatch at position i is [T not in S_i] + sum over c in {A, C, G} of ([T in S_i] - [c in S_i]) x_c:
// v(S_i, channel) = [T in S_i] - [channel in S_i], still in {-1, 0, +1}, and the constant #(q_i != T) becomes #{i : T not in S_i}.  S = {A}, {T}, N, {}
// and {A, T} give 1 - x_A, x_A + x_C + x_G, 0, 1 and x_C + x_G.  An exact query is the pattern of singletons: the same nibbles and start values.
struct Count3Rule {
    PatternSets pat;
    size_t k;
    unsigned tau;
    bool distance, all;
    unsigned non_t;
    BITNUC_HD Count3Rule(const PatternSets &pat, size_t k, unsigned tau, bool distance) : pat(pat), k(k), tau(tau), distance(distance), all(!distance && tau >= k), non_t(0) {
        for (size_t i = 0; i < k; ++i) non_t += !pattern_has(pat, 3, (int)i);
    }
    BITNUC_HD Count3Rule(uint64_t query, size_t k, unsigned tau, bool distance) : Count3Rule(pattern_of_2bit(query, k), k, tau, distance) {}
    // the nibble row m meets at segment position p on channel ch (0 = A, 1 = C, 2 = G): 0, +1.0 (0x2) or -1.0 (0xA)
    BITNUC_HD uint32_t nibble(int m, int p, unsigned ch) const {
        const int i = p - m;
        if (all || i < 0 || i >= (int)k) return 0u;
        const int v = (int)pattern_has(pat, 3, i) - (int)pattern_has(pat, ch, i);
        const int e = distance || (m & 3) == 3 ? v : -v;
        return e == 0 ? 0u : e > 0 ? 0x2u : 0xAu;
    }
    BITNUC_HD void start(float *c) const {
        if (distance) {
            for (int j = 0; j < 4; ++j) c[j] = kPackBias + (float)(non_t << (j == 3 ? 0 : 8 * j));
            return;
        }
        for (int j = 0; j < 3; ++j) c[j] = kPackBias + (float)((all ? 32u : 32u + tau - non_t) << (6 * j));
        c[3] = all ? -1.f : (float)(2 * (int)non_t - 2 * (int)tau - 1);
    }
};

// ... its table in the ASCII K order: per lane (row m = lane & 31, K-block h = lane >> 5) and K-step, the 32 nibbles that meet the lane's operand --
// K-steps 0 / 1: the (A, C) bytes of positions 32 s + 16 h + b; K-step 2: the G nibbles of positions 32 h .. + 31, byte b holding positions 8 (b >> 2) + (b & 3)
// and that + 4.
// (one lane's 12 dwords: count3_mfma_lane; the device builder runs one thread per lane)
BITNUC_HD inline void count3_mfma_lane(const Count3Rule &r, int lane, uint32_t *row) {
    const int m = lane & 31, h = lane >> 5;
    for (int s = 0; s < 3; ++s)
        for (int i = 0; i < 4; ++i) {
            uint32_t w = 0;
            for (int bb = 0; bb < 4; ++bb) {
                const int b = 4 * i + bb;
                const int gp = 32 * h + 8 * (b >> 2) + (b & 3); // K-step 2, byte b of the lane's 16: bases gp (low nibble) and gp + 4 (high nibble) of positions 32 h .. + 31
                const uint32_t lo = s < 2 ? r.nibble(m, 32 * s + 16 * h + b, 0) : r.nibble(m, gp, 2);
                const uint32_t hi = s < 2 ? r.nibble(m, 32 * s + 16 * h + b, 1) : r.nibble(m, gp + 4, 2);
                w |= (lo | hi << 4) << (8 * bb);
            }
            row[4 * s + i] = w;
        }
}
BITNUC_HD inline void count3_mfma_table(uint64_t query, size_t k, unsigned tau, Count3MfmaTable *t, bool distance = false) {
    const Count3Rule r(query, k, tau, distance);
    for (int lane = 0; lane < 64; ++lane) count3_mfma_lane(r, lane, t->w[lane]);
    r.start(t->c);
}
BITNUC_HD inline void count3_mfma_table(const PatternSets &p, size_t k, unsigned tau, Count3MfmaTable *t) {
    const Count3Rule r(p, k, tau, false);
    for (int lane = 0; lane < 64; ++lane) count3_mfma_lane(r, lane, t->w[lane]);
    r.start(t->c);
}

// ---- the packed scan and count (scan_packed_device.h): the same products, with the one-hot operand built from 2-bit codes ----------------------------
// A packed dword holds 16 bases; s_t = (x >> 2 t) & 0x03030303 puts bases t, t + 4, t + 8, t + 12 into its byte lanes, and one v_perm LUT per
// channel pair turns those codes into nibbles.  The K order below is the order that front end produces.

// The scan (four channels per base).  Lane (row m, K-block h), K-step j, dword d, byte q: position 16 j + 4 q + 2 h + (d >> 1) of the segment (half h of a
// 16-base group is its bases with (b & 3) >> 1 == h), low nibble channel A (d even) / G (d odd), high nibble C / T.  The query offset is that position
// minus m, so a row only depends on m - 2 h: w[m - 2 h + 2].  Entries mark the channels that differ from the query's base; the accumulators start at the
// 2^23 pack bias (kmer_scan_seg_mfma_kernel's pack).
// (one row: scan_packed_row; the best-match kernels build theirs on the device, one thread per row: scan_best_device.h)
BITNUC_HD inline void scan_packed_row(const PatternSets &pat, size_t k, int delta, uint32_t *row) {
    for (int j = 0; j < 4; ++j)
        for (int d = 0; d < 4; ++d) {
            uint32_t w = 0;
            for (int q = 0; q < 4; ++q) {
                const int i = 16 * j + 4 * q + (d >> 1) - delta;
                if (i < 0 || i >= (int)k) continue;
                const unsigned lo = (d & 1) ? 2u : 0u, hi = lo + 1u; // (A, C) or (G, T)
                w |= ((pattern_has(pat, lo, i) ? 0u : 0x02u) | (pattern_has(pat, hi, i) ? 0u : 0x20u)) << (8 * q);
            }
            row[4 * j + d] = w;
        }
}
BITNUC_HD inline void scan_packed_row(uint64_t query, size_t k, int delta, uint32_t *row) { scan_packed_row(pattern_of_2bit(query, k), k, delta, row); }
inline void scan_packed_table(const PatternSets &pat, size_t k, PackedScanTable *t) {
    for (int delta = -2; delta < 32; ++delta) scan_packed_row(pat, k, delta, t->w[delta + 2]);
    for (int j = 0; j < 4; ++j) t->c[j] = kPackBias;
}
inline void scan_packed_table(uint64_t query, size_t k, PackedScanTable *t) { scan_packed_table(pattern_of_2bit(query, k), k, t); }

// The count (three channels per base: A, C, G one-hot, T = 0), as count3_mfma_table but in the packed K order.  K-steps 0 / 1: dword t, byte q holds
// the (A, C) nibbles of position 16 (2 s + h) + 4 q + t; K-step 2: dword d, nibble p (byte p >> 1, high nibble when p is odd) holds the G nibble of
// position 32 h + 16 (d >> 1) + 2 p + (d & 1).  Rows, signs, row scales and start values: Count3Rule.
BITNUC_HD inline void count3_packed_lane(const Count3Rule &r, int lane, uint32_t *row) {
    const int m = lane & 31, h = lane >> 5;
    for (int s = 0; s < 3; ++s)
        for (int d = 0; d < 4; ++d) {
            uint32_t w = 0;
            for (int b = 0; b < 4; ++b) {
                uint32_t lo, hi;
                if (s < 2) {
                    const int p = 16 * (2 * s + h) + 4 * b + d;
                    lo = r.nibble(m, p, 0), hi = r.nibble(m, p, 1);
                } else {
                    const int p = 32 * h + 16 * (d >> 1) + 4 * b + (d & 1); // nibble 2 b; nibble 2 b + 1 is two positions later
                    lo = r.nibble(m, p, 2), hi = r.nibble(m, p + 2, 2);
                }
                w |= (lo | hi << 4) << (8 * b);
            }
            row[4 * s + d] = w;
        }
}
BITNUC_HD inline void count3_packed_table(uint64_t query, size_t k, unsigned tau, Count3MfmaTable *t) {
    const Count3Rule r(query, k, tau, false);
    for (int lane = 0; lane < 64; ++lane) count3_packed_lane(r, lane, t->w[lane]);
    r.start(t->c);
}
BITNUC_HD inline void count3_packed_table(const PatternSets &p, size_t k, unsigned tau, Count3MfmaTable *t) {
    const Count3Rule r(p, k, tau, false);
    for (int lane = 0; lane < 64; ++lane) count3_packed_lane(r, lane, t->w[lane]);
    r.start(t->c);
}

} // namespace bitnuc_host
