// The host side of the pattern queries under AddressSanitizer + UBSan (built and run by tests/test_kmer_pattern_host.py; plain C++, no HIP):
//   1. for every k in 1..32, tau in {0, 1, k-1, k, k+1, 2^32-1} and 50 seeded queries, the table builders of scan_mfma_host.h on pattern_of_2bit(q) give
//      tables and start values byte-identical to the exact query's rule, which is restated here as it stood before the builders took sets (old_*): both
//      count orders, both scan-row orders and the four-channel thresholded table;
//   2. for seeded random patterns (with empty sets, N and PAM shapes) an integer emulation of the contraction -- 0x2 = +1, 0xA = -1, the row scales, the
//      start values, the hit_bits mask and the hit lists' byte compare -- in the K orders the builders document: the distance fields equal pdist, the
//      kept bits equal pdist <= tau, every partial sum stays below 2^24;
//   3. the *_small forms of scan_multi_host.h, scan_best_host.h and scan_hits_host.h under patterns against brute force, and the IUPAC converter.
#include "../../bitnuc_amd/csrc/pattern_host.h"
#include "../../bitnuc_amd/csrc/scan_best_host.h"
#include "../../bitnuc_amd/csrc/scan_hits_host.h"
#include "../../bitnuc_amd/csrc/scan_mfma_host.h"
#include "../../bitnuc_amd/csrc/scan_multi_host.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

using namespace bitnuc_host;
using bitnuc_dev::BestTable;

namespace {

uint64_t rng_state = 0x243F6A8885A308D3ull;
uint64_t rnd64() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

// ---- 1. the exact query's rule as it was written for one base per position ------------------------------------------------------------------
struct OldRule {
    uint64_t query; size_t k; unsigned tau; bool all; unsigned non_t;
    OldRule(uint64_t q, size_t k, unsigned tau) : query(q), k(k), tau(tau), all(tau >= k), non_t(0) {
        for (size_t i = 0; i < k; ++i) non_t += ((q >> (2 * i)) & 3) != 3;
    }
    uint32_t nibble(int m, int p, unsigned ch) const {
        const int i = p - m;
        if (all || i < 0 || i >= (int)k) return 0u;
        const unsigned q = (unsigned)((query >> (2 * i)) & 3);
        const int v = q == 3 ? 1 : (ch == q ? -1 : 0);
        const int e = (m & 3) == 3 ? v : -v;
        return e == 0 ? 0u : e > 0 ? 0x2u : 0xAu;
    }
    void start(float *c) const {
        for (int j = 0; j < 3; ++j) c[j] = kPackBias + (float)((all ? 32u : 32u + tau - non_t) << (6 * j));
        c[3] = all ? -1.f : (float)(2 * (int)non_t - 2 * (int)tau - 1);
    }
};
void old_count3_ascii(const OldRule &r, Count3MfmaTable *t) {
    for (int lane = 0; lane < 64; ++lane) {
        const int m = lane & 31, h = lane >> 5;
        for (int s = 0; s < 3; ++s)
            for (int i = 0; i < 4; ++i) {
                uint32_t w = 0;
                for (int bb = 0; bb < 4; ++bb) {
                    const int b = 4 * i + bb, gp = 32 * h + 8 * (b >> 2) + (b & 3);
                    const uint32_t lo = s < 2 ? r.nibble(m, 32 * s + 16 * h + b, 0) : r.nibble(m, gp, 2);
                    const uint32_t hi = s < 2 ? r.nibble(m, 32 * s + 16 * h + b, 1) : r.nibble(m, gp + 4, 2);
                    w |= (lo | hi << 4) << (8 * bb);
                }
                t->w[lane][4 * s + i] = w;
            }
    }
    r.start(t->c);
}
void old_count3_packed(const OldRule &r, Count3MfmaTable *t) {
    for (int lane = 0; lane < 64; ++lane) {
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
                        const int p = 32 * h + 16 * (d >> 1) + 4 * b + (d & 1);
                        lo = r.nibble(m, p, 2), hi = r.nibble(m, p + 2, 2);
                    }
                    w |= (lo | hi << 4) << (8 * b);
                }
                t->w[lane][4 * s + d] = w;
            }
    }
    r.start(t->c);
}
uint32_t old_differs(uint64_t query, size_t k, int p, bool gt) { // the byte of query position p on channels (A, C) or (G, T)
    if (p < 0 || p >= (int)k) return 0u;
    const unsigned qb = (unsigned)((query >> (2 * p)) & 3), lo = gt ? 2u : 0u, hi = lo + 1u;
    return (qb != lo ? 0x02u : 0u) | (qb != hi ? 0x20u : 0u);
}
void old_seg_row(uint64_t query, size_t k, int delta, uint32_t *row) {
    for (int j = 0; j < 4; ++j)
        for (int i = 0; i < 4; ++i) {
            uint32_t w = 0;
            for (int b = 0; b < 4; ++b) w |= old_differs(query, k, 16 * j + 4 * (i >> 1) + b - delta, i & 1) << (8 * b);
            row[4 * j + i] = w;
        }
}
void old_packed_row(uint64_t query, size_t k, int delta, uint32_t *row) {
    for (int j = 0; j < 4; ++j)
        for (int d = 0; d < 4; ++d) {
            uint32_t w = 0;
            for (int q = 0; q < 4; ++q) w |= old_differs(query, k, 16 * j + 4 * q + (d >> 1) - delta, d & 1) << (8 * q);
            row[4 * j + d] = w;
        }
}

void check_singletons(uint64_t query, size_t k, unsigned tau, bool rows) {
    const PatternSets p = pattern_of_2bit(query, k);
    const OldRule r(query, k, tau);
    Count3MfmaTable a, b, c;
    memset(&a, 0xEE, sizeof a), memset(&b, 0xDD, sizeof b), memset(&c, 0xCC, sizeof c);
    old_count3_ascii(r, &a), count3_mfma_table(p, k, tau, &b), count3_mfma_table(query, k, tau, &c);
    CHECK(!memcmp(&a, &b, sizeof a) && !memcmp(&a, &c, sizeof a));
    old_count3_packed(r, &a), count3_packed_table(p, k, tau, &b), count3_packed_table(query, k, tau, &c);
    CHECK(!memcmp(&a, &b, sizeof a) && !memcmp(&a, &c, sizeof a));
    CountMfmaTable x, y;
    memset(&x, 0xEE, sizeof x), memset(&y, 0xDD, sizeof y);
    count_mfma_table(query, k, &x, true, tau, false), count_mfma_table(p, k, &y, true, tau);
    CHECK(!memcmp(&x, &y, sizeof x));
    if (!rows) return; // the rest does not depend on tau
    count_mfma_table(query, k, &x), count_mfma_table(p, k, &y);
    CHECK(!memcmp(&x, &y, sizeof x));
    uint32_t ra[16], rb[16], rc[16];
    for (int delta = -8; delta < 32; ++delta) {
        old_seg_row(query, k, delta, ra), scan_seg_row(p, k, delta, rb), scan_seg_row(query, k, delta, rc);
        CHECK(!memcmp(ra, rb, sizeof ra) && !memcmp(ra, rc, sizeof ra));
        CHECK(!memcmp(ra, x.w[delta + 8], sizeof ra)); // the plain table's row delta is that row
    }
    PackedScanTable s, t;
    memset(&s, 0xEE, sizeof s), memset(&t, 0xDD, sizeof t);
    scan_packed_table(query, k, &s), scan_packed_table(p, k, &t);
    CHECK(!memcmp(&s, &t, sizeof s));
    for (int delta = -2; delta < 32; ++delta) {
        old_packed_row(query, k, delta, ra), scan_packed_row(p, k, delta, rb);
        CHECK(!memcmp(ra, rb, sizeof ra) && !memcmp(ra, s.w[delta + 2], sizeof ra));
    }
    for (int j = 0; j < 4; ++j) CHECK(s.c[j] == kPackBias);
    uint32_t ql, qh; // the converter against the bit-plane builder
    query_planes(query, k, &ql, &qh);
    CHECK(p.allow[0] == (~ql & ~qh & (k == 32 ? ~0u : (1u << k) - 1)) && p.allow[3] == (ql & qh) && p.allow[1] == (ql & ~qh) && p.allow[2] == (~ql & qh));
}

// ---- 2. the contraction in integers ---------------------------------------------------------------------------------------------------------
bool in_set(const PatternSets &p, unsigned c, size_t i) { return (p.allow[c] >> i) & 1u; }
unsigned pdist_at(const std::vector<uint8_t> &codes, size_t j, const PatternSets &p, size_t k) {
    unsigned d = 0;
    for (size_t i = 0; i < k; ++i) d += !in_set(p, codes[j + i], i);
    return d;
}
int fp4(uint32_t nib) {
    CHECK(nib == 0 || nib == 0x2 || nib == 0xA);
    return nib == 0 ? 0 : nib == 0x2 ? 1 : -1;
}
struct Acc { // an accumulator whose every partial sum is checked
    long long v;
    void add(long long scale, uint32_t nib, bool x) {
        v += scale * fp4(nib) * (x ? 1 : 0);
        CHECK(v < (1ll << 24) && v > -(1ll << 24));
    }
};
uint32_t f32_bits(long long v) { float f = (float)v; CHECK((long long)f == v); uint32_t u; memcpy(&u, &f, 4); return u; }
long long start_of(float c) { const long long v = (long long)c; CHECK((float)v == c); return v; }

// the segment position and channel that nibble `nib` (0..7) of dword `dw` (0..3) of K-step s of the lane of K-block h meets, as the builders document it
struct Slot { int pos; unsigned ch; };
Slot count3_ascii_slot(int h, int s, int dw, int nib) {
    const int b = 4 * dw + (nib >> 1), gp = 32 * h + 8 * (b >> 2) + (b & 3);
    if (s < 2) return Slot{32 * s + 16 * h + b, (unsigned)(nib & 1)};
    return Slot{gp + 4 * (nib & 1), 2u};
}
Slot count3_packed_slot(int h, int s, int dw, int nib) {
    const int b = nib >> 1;
    if (s < 2) return Slot{16 * (2 * s + h) + 4 * b + dw, (unsigned)(nib & 1)};
    return Slot{32 * h + 16 * (dw >> 1) + 4 * b + (dw & 1) + 2 * (nib & 1), 2u};
}
Slot seg_slot(int h, int j, int i, int nib) { return Slot{16 * j + 4 * (i >> 1) + (nib >> 1) + 8 * h, (unsigned)(2 * (i & 1) + (nib & 1))}; }
Slot packed_slot(int h, int j, int d, int nib) { return Slot{16 * j + 4 * (nib >> 1) + 2 * h + (d >> 1), (unsigned)(2 * (d & 1) + (nib & 1))}; }

// one (row m, column n) result of `steps` K-steps: start + scale * sum of A x one-hot(B)
template <class SlotOf, class RowOf>
long long contract(const std::vector<uint8_t> &codes, int n, int steps, long long start, long long scale, SlotOf slot_of, RowOf row_of) {
    Acc a{start};
    for (int h = 0; h < 2; ++h) {
        const uint32_t *row = row_of(h);
        for (int s = 0; s < steps; ++s)
            for (int dw = 0; dw < 4; ++dw)
                for (int nib = 0; nib < 8; ++nib) {
                    const Slot sl = slot_of(h, s, dw, nib);
                    CHECK(sl.pos >= 0 && sl.pos < 64); // a segment and its halo
                    a.add(scale, (row[4 * s + dw] >> (4 * nib)) & 0xF, codes[32 * n + sl.pos] == sl.ch);
                }
    }
    return a.v;
}

void check_contraction(const std::vector<uint8_t> &codes, int columns, const PatternSets &p, size_t k, unsigned tau) {
    const bool all = tau >= k;
    Count3MfmaTable *c3[2] = {new Count3MfmaTable, new Count3MfmaTable};
    count3_mfma_table(p, k, tau, c3[0]);
    count3_packed_table(p, k, tau, c3[1]);
    CountMfmaTable *ct = new CountMfmaTable, *cth = new CountMfmaTable;
    count_mfma_table(p, k, ct);             // the hit lists' table (the accumulators start at the pack bias: kmer.hip, scan_seg_table)
    count_mfma_table(p, k, cth, true, tau); // its thresholded form
    PackedScanTable *pt = new PackedScanTable;
    scan_packed_table(p, k, pt);
    const uint32_t tcap = tau < 32u ? tau : 32u, bias = 0x7Fu - tcap; // hits_bias per byte
    for (int n = 0; n < columns; ++n) {
        for (int order = 0; order < 2; ++order) { // the three-channel count, ASCII and packed K order
            for (int g = 0; g < 8; ++g) {        // rows 4 g .. 4 g + 3: one hit_bits group
                uint32_t bits = 0;
                unsigned want = 0;
                for (int jr = 0; jr < 4; ++jr) {
                    const int m = 4 * g + jr;
                    const unsigned d = pdist_at(codes, 32 * n + m, p, k);
                    const long long scale = jr == 3 ? 2 : 1ll << (6 * jr);
                    const long long acc = order == 0 ? contract(codes, n, 3, start_of(c3[0]->c[jr]), scale, count3_ascii_slot, [&](int h) { return c3[0]->w[m + 32 * h]; })
                                                     : contract(codes, n, 3, start_of(c3[1]->c[jr]), scale, count3_packed_slot, [&](int h) { return c3[1]->w[m + 32 * h]; });
                    const bool hit = d <= tau;
                    want += hit;
                    if (jr < 3) {
                        const long long field = (acc - (1ll << 23)) >> (6 * jr);
                        CHECK(((acc - (1ll << 23)) & ((1ll << (6 * jr)) - 1)) == 0 && field >= 0 && field < 64);
                        CHECK(field == (all ? 32 : 32 + (long long)tau - d)); // the distance field
                        CHECK(((field >> 5) & 1) == (long long)hit);
                    } else {
                        CHECK(acc == (all ? -1 : 2 * (long long)d - 2 * (long long)tau - 1));
                        CHECK((acc < 0) == hit);
                    }
                    bits |= f32_bits(acc);
                }
                CHECK((unsigned)__builtin_popcount(bits & 0x80020820u) == want);
            }
        }
        for (int m = 0; m < 32; ++m) { // the four-channel tables: the distance itself
            const unsigned d = pdist_at(codes, 32 * n + m, p, k);
            const int jr = m & 3;
            const long long dscale = jr == 3 ? 1 : 1ll << (8 * jr); // dist_row_scale
            const long long seg = contract(codes, n, 4, start_of(kPackBias), dscale, seg_slot, [&](int h) { return ct->w[m - 8 * h + 8]; });
            const long long pk = contract(codes, n, 4, start_of(pt->c[jr]), dscale, packed_slot, [&](int h) { return pt->w[m - 2 * h + 2]; });
            CHECK(seg == (1ll << 23) + (long long)d * dscale && pk == seg);
            const uint32_t byte = (uint32_t)((seg - (1ll << 23)) / dscale); // pack_distances' byte
            CHECK((((~(byte + bias)) & 0x80u) != 0) == (d <= tau));          // hits_of4: the kept bit
            const long long best = contract(codes, n, 4, (1ll << 23) + 5, 16, seg_slot, [&](int h) { return ct->w[m - 8 * h + 8]; });
            CHECK(best == (1ll << 23) + 16 * (long long)d + 5); // the best match's key: 2^23 + 16 d + r
            const long long cscale = jr == 3 ? 2 : 1ll << (6 * jr);
            const long long th = contract(codes, n, 4, start_of(cth->c[jr]), cscale, seg_slot, [&](int h) { return cth->w[m - 8 * h + 8]; });
            if (jr < 3) CHECK(th == (1ll << 23) + ((all ? 32 : 32 + (long long)tau - d) << (6 * jr)));
            else CHECK(th == (all ? -1 : 2 * (long long)d - 2 * (long long)tau - 1));
        }
    }
    delete c3[0], delete c3[1], delete ct, delete cth, delete pt;
}

PatternSets random_pattern(size_t k, int kind) {
    PatternSets p = {{0, 0, 0, 0}};
    for (size_t i = 0; i < k; ++i) {
        unsigned s;
        switch (kind) {
        case 0: s = (unsigned)(rnd64() & 15); break;                                  // any set, the empty one and N included
        case 1: s = 15; break;                                                        // all N
        case 2: s = 0; break;                                                         // all empty
        case 3: s = 8; break;                                                         // {T}
        case 4: s = 9; break;                                                         // {A, T}
        case 5: s = i + 3 < k ? 1u << (rnd64() & 3) : i + 3 == k ? 15u : 4u; break;   // exact + NGG
        default: s = i + 3 < k ? 1u << (rnd64() & 3) : i + 3 == k ? 15u : i + 2 == k ? 5u : 4u; break; // exact + NRG
        }
        for (unsigned c = 0; c < 4; ++c) p.allow[c] |= ((s >> c) & 1u) << i;
    }
    for (unsigned c = 0; c < 4; ++c) p.allow[c] |= k < 32 ? (uint32_t)rnd64() << k : 0u; // junk at positions >= k: ignored
    return p;
}

std::vector<uint8_t> sequence_for(const PatternSets &p, size_t k, size_t n, bool near) {
    std::vector<uint8_t> codes(n);
    for (size_t i = 0; i < n; ++i) {
        uint8_t c = (uint8_t)(rnd64() & 3);
        if (near && rnd64() % 8 != 0) // mostly a base the pattern accepts at position i % k: small distances
            for (int t = 0; t < 4 && !in_set(p, c, i % k); ++t) c = (uint8_t)((c + 1) & 3);
        codes[i] = c;
    }
    return codes;
}

bool same(const void *a, const void *b, size_t bytes) { return bytes == 0 || !memcmp(a, b, bytes); } // (an empty vector's data() may be null)

// ---- 3. the small forms -----------------------------------------------------------------------------------------------------------------------
void check_small(size_t k, size_t n) {
    const size_t nq = 5;
    std::vector<PatternSets> pats(nq);
    for (size_t q = 0; q < nq; ++q) pats[q] = random_pattern(k, q == 0 ? 5 : q == 1 ? 2 : 0);
    std::vector<uint8_t> codes = sequence_for(pats[0], k, n, true);
    std::vector<uint8_t> ascii(n);
    std::vector<uint64_t> words((n + 31) / 32 + 1, 0); // (+ 1: an n of 0 still has a word to point at)
    for (size_t i = 0; i < n; ++i) {
        ascii[i] = (uint8_t)("ACGT"[codes[i]] | ((rnd64() & 1) ? 0x20 : 0));
        words[i / 32] |= (uint64_t)codes[i] << (2 * (i % 32));
    }
    if (n % 32) words[n / 32] |= rnd64() << (2 * (n % 32)); // junk above the last base
    const uint32_t taus[nq] = {1u, (uint32_t)k - 1, 0u, (uint32_t)k / 2, 0xFFFFFFFFu};
    const size_t nwin = n + 1 - k;
    std::vector<uint64_t> want_counts(nq, 0), want_pos(nq, ~0ull);
    std::vector<uint8_t> want_dist(nq, 0xFF);
    for (size_t q = 0; q < nq; ++q)
        for (size_t j = 0; j < nwin; ++j) {
            const unsigned d = pdist_at(codes, j, pats[q], k);
            want_counts[q] += d <= taus[q];
            if (d < want_dist[q]) want_dist[q] = (uint8_t)d, want_pos[q] = j;
        }
    std::vector<uint64_t> counts(nq + 1, 0xABABABABABABABABull), pos(nq + 1, 0xABABABABABABABABull);
    std::vector<uint8_t> dist(nq + 1, 0xAB);
    CHECK(kmer_hdist_count_multi_small(ascii.data(), n, k, pats.data(), taus, nq, counts.data()) == -1);
    CHECK(same(counts.data(), want_counts.data(), nq * 8) && counts[nq] == 0xABABABABABABABABull);
    kmer_hdist_count_multi_packed_small(words.data(), n, k, pats.data(), taus, nq, counts.data());
    CHECK(same(counts.data(), want_counts.data(), nq * 8) && counts[nq] == 0xABABABABABABABABull);
    CHECK(kmer_hdist_best_small(ascii.data(), n, k, pats.data(), nq, pos.data(), dist.data()) == -1);
    CHECK(same(pos.data(), want_pos.data(), nq * 8) && same(dist.data(), want_dist.data(), nq) && pos[nq] == 0xABABABABABABABABull && dist[nq] == 0xAB);
    kmer_hdist_best_packed_small(words.data(), n, k, pats.data(), nq, pos.data(), dist.data());
    CHECK(same(pos.data(), want_pos.data(), nq * 8) && same(dist.data(), want_dist.data(), nq));
    for (size_t q = 0; q < nq; ++q) {
        std::vector<uint64_t> hp;
        std::vector<uint8_t> hd;
        for (size_t j = 0; j < nwin; ++j) {
            const unsigned d = pdist_at(codes, j, pats[q], k);
            if (d <= taus[q]) hp.push_back(j), hd.push_back((uint8_t)d);
        }
        const size_t caps[4] = {0, hp.size() ? hp.size() - 1 : 0, hp.size(), hp.size() + 5};
        for (size_t cap : caps) {
            std::vector<uint64_t> gp(cap + 1, 0xABABABABABABABABull);
            std::vector<uint8_t> gd(cap + 1, 0xAB);
            uint64_t total = ~0ull;
            CHECK(kmer_hdist_hits_small(ascii.data(), n, k, pats[q], taus[q], cap ? gp.data() : nullptr, cap ? gd.data() : nullptr, cap, &total) == -1);
            const size_t kept = cap < hp.size() ? cap : hp.size();
            CHECK(total == hp.size() && same(gp.data(), hp.data(), kept * 8) && same(gd.data(), hd.data(), kept));
            CHECK(gp[kept] == 0xABABABABABABABABull && gd[kept] == 0xAB);
            std::fill(gp.begin(), gp.end(), 0xABABABABABABABABull);
            CHECK(kmer_hdist_hits_packed_small(words.data(), n, k, pats[q], taus[q], gp.data(), nullptr, cap) == hp.size()); // no distances wanted
            CHECK(same(gp.data(), hp.data(), kept * 8) && gp[kept] == 0xABABABABABABABABull);
        }
    }
    if (n > 3) { // an invalid reference byte: its index, nothing written
        ascii[n - 2] = 'N';
        ascii[n / 2] = '-';
        counts.assign(nq + 1, 7);
        CHECK(kmer_hdist_count_multi_small(ascii.data(), n, k, pats.data(), taus, nq, counts.data()) == (long long)(n / 2 < n - 2 ? n / 2 : n - 2) && counts[0] == 7);
        CHECK(kmer_hdist_best_small(ascii.data(), n, k, pats.data(), nq, pos.data(), dist.data()) >= 0);
        uint64_t total = 99;
        CHECK(kmer_hdist_hits_small(ascii.data(), n, k, pats[0], 0u, nullptr, nullptr, 0, &total) >= 0 && total == 99);
    }
}

void check_iupac() {
    const char *letters = "ACGTURYSWKMBDHVN";
    const unsigned sets[16] = {1, 2, 4, 8, 8, 5, 10, 6, 9, 12, 3, 14, 13, 11, 7, 15};
    for (int lower = 0; lower < 2; ++lower) {
        uint8_t buf[32];
        for (int i = 0; i < 32; ++i) buf[i] = (uint8_t)(letters[i % 16] | (lower ? 0x20 : 0));
        for (size_t k = 0; k <= 32; ++k) {
            PatternSets p = {{9, 9, 9, 9}};
            CHECK(pattern_from_iupac(buf, k, &p) == -1);
            for (size_t i = 0; i < 32; ++i)
                for (unsigned c = 0; c < 4; ++c) CHECK(((p.allow[c] >> i) & 1u) == (i < k ? (sets[i % 16] >> c) & 1u : 0u));
        }
    }
    for (int b = 0; b < 256; ++b) {
        const uint8_t buf[3] = {'N', 'n', (uint8_t)b};
        PatternSets p = {{9, 9, 9, 9}};
        const bool ok = strchr(letters, b & 0xDF) != nullptr && b != 0 && ((b >= 'A' && b <= 'Z') || (b >= 'a' && b <= 'z'));
        CHECK(pattern_from_iupac(buf, 3, &p) == (ok ? -1 : 2));
        CHECK(ok || p.allow[0] == 9);
    }
}

} // namespace

int main() {
    unsigned long long singles = 0, contractions = 0, smalls = 0;
    for (size_t k = 1; k <= 32; ++k) {
        const unsigned taus[6] = {0u, 1u, (unsigned)k - 1, (unsigned)k, (unsigned)k + 1, 0xFFFFFFFFu};
        for (int rep = 0; rep < 50; ++rep) {
            const uint64_t query = rep == 0 ? ~0ull : rep == 1 ? 0ull : rnd64(); // all T, all A, junk above 2 k
            for (int t = 0; t < 6; ++t) check_singletons(query, k, taus[t], t == 0), ++singles;
        }
        for (int kind = 0; kind < 7; ++kind) {
            if (kind >= 5 && k < 4) continue;
            const PatternSets p = random_pattern(k, kind);
            const int columns = 3;
            const std::vector<uint8_t> codes = sequence_for(p, k, 32 * columns + 64, kind != 1);
            for (unsigned tau : taus) check_contraction(codes, columns, p, k, tau), ++contractions;
        }
        const size_t ns[5] = {k - 1, k, k + 1, 97, 1100};
        for (size_t n : ns) {
            if (n < k) continue; // the callers handle "no windows" before the small forms
            check_small(k, n), ++smalls;
        }
    }
    check_iupac();
    printf("pattern host ok: %llu singleton tables, %llu contractions, %llu small cases\n", singles, contractions, smalls);
    return 0;
}
