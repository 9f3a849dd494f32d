// pattern_host.h -- the host side of the pattern queries (bitnuc_pattern, include/bitnuc_hip.h): the converters from IUPAC letters and from a packed
// exact query, and pdist of one window word, pdist = #{ i < k : base i of the window is not in S_i }.  The *_small forms of scan_multi_host.h,
// scan_best_host.h and scan_hits_host.h take either query kind through window_dist.  Plain C++ (no HIP): tests/c/pattern_host_sanitize.cpp runs all of
// it under ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "host_word.h"      // hdist_word
#include "scan_mfma_host.h" // PatternSets, pattern_of_2bit

namespace bitnuc_host {

// the set of an IUPAC letter as a mask over (A, C, G, T) = bits (0, 1, 2, 3), either case; 0xFF for a byte that is none
static inline unsigned iupac_set(uint8_t byte) {
    switch (byte & 0xDFu) { // upper case; the letters' own bit 5 is clear
    case 'A': return 0x1;
    case 'C': return 0x2;
    case 'G': return 0x4;
    case 'T': case 'U': return 0x8;
    case 'R': return 0x5; // A G
    case 'Y': return 0xA; // C T
    case 'S': return 0x6; // C G
    case 'W': return 0x9; // A T
    case 'K': return 0xC; // G T
    case 'M': return 0x3; // A C
    case 'B': return 0xE; // not A
    case 'D': return 0xD; // not C
    case 'H': return 0xB; // not G
    case 'V': return 0x7; // not T
    case 'N': return 0xF;
    default: return 0xFF;
    }
}

// k <= 32 letters -> the pattern; -1, or the index of the first byte that is no IUPAC letter (*out untouched)
static inline long long pattern_from_iupac(const uint8_t *letters, size_t k, PatternSets *out) {
    PatternSets p = {{0u, 0u, 0u, 0u}};
    for (size_t i = 0; i < k; ++i) {
        // (a letter's lower case differs in bit 5 only, but so do '[' - 0x20 and friends: only letters pass)
        const uint8_t b = letters[i];
        const bool letter = (b >= 'A' && b <= 'Z') || (b >= 'a' && b <= 'z');
        const unsigned s = letter ? iupac_set(b) : 0xFFu;
        if (s == 0xFFu) return (long long)i;
        for (unsigned c = 0; c < 4; ++c) p.allow[c] |= ((s >> c) & 1u) << i;
    }
    *out = p;
    return -1;
}

// de-interleave a window word into its bit-planes: bit i of *lo / *hi = the low / high code bit of base i
static inline void word_planes(uint64_t w, uint32_t *lo, uint32_t *hi) {
    uint64_t x[2] = {w & 0x5555555555555555ull, (w >> 1) & 0x5555555555555555ull};
    for (int h = 0; h < 2; ++h) {
        uint64_t v = x[h];
        v = (v | (v >> 1)) & 0x3333333333333333ull;
        v = (v | (v >> 2)) & 0x0F0F0F0F0F0F0F0Full;
        v = (v | (v >> 4)) & 0x00FF00FF00FF00FFull;
        v = (v | (v >> 8)) & 0x0000FFFF0000FFFFull;
        x[h] = (v | (v >> 16)) & 0xFFFFFFFFull;
    }
    *lo = (uint32_t)x[0];
    *hi = (uint32_t)x[1];
}

// pdist of the window word w (base i at bits 2 i; bits above 2 k are junk) under the pattern
static inline uint32_t pattern_dist_word(uint64_t w, const PatternSets &p, size_t k) {
    uint32_t lo, hi;
    word_planes(w, &lo, &hi);
    const uint32_t ones = k >= 32 ? ~0u : ((1u << k) - 1);
    const uint32_t match = (~hi & ~lo & p.allow[0]) | (~hi & lo & p.allow[1]) | (hi & ~lo & p.allow[2]) | (hi & lo & p.allow[3]);
    return (uint32_t)__builtin_popcount(ones & ~match);
}

// a window's distance to a query of either kind
static inline uint32_t window_dist(uint64_t w, uint64_t query, size_t k) { return hdist_word(w, query, k); }
static inline uint32_t window_dist(uint64_t w, const PatternSets &p, size_t k) { return pattern_dist_word(w, p, k); }

} // namespace bitnuc_host
