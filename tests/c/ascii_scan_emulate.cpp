// CPU emulation of the ASCII three-channel count on the matrix cores (kmer_count3_mfma_kernel, scan_mfma_device.h; and the multi-query count,
// scan_multi_device.h, which runs the same contraction once per query), built by tests/test_kmer_multi_host.py under AddressSanitizer + UBSan.  For
// one trip of m = 1..4 rounds of ASCII bytes (mixed case) it expands every lane's 16 bytes the way expand3 does (the (A, C) byte LUT and the G nibble
// LUT of v_perm on byte & 7, two G nibbles per byte), writes the (A, C) bytes by group parity and the G nibbles into the wave-private strip at the
// kernel's offsets (the halo after the last valid round included), reads each lane's three K-step operands back at the kernel's offsets, then applies
// count3_mfma_table (scan_mfma_host.h), the E8M0 row scales and the accumulator start values in integers, in the MFMA's register layout.  It asserts,
// against hdist_scalar of every window:
//   * the threshold bits equal d <= tau, and the kernel's hit mask (v_or3 + v_bitop3 + v_bcnt) counts exactly the windows with d <= tau;
//   * every partial sum stays an integer of magnitude below 2^24 (f32-exact).
#include "../../bitnuc_amd/csrc/scan_mfma_host.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

namespace {

uint64_t rng_state = 0x6A09E667F3BCC909ull;
uint64_t rnd64() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

constexpr int U = 4;                         // kCountRounds / kMultiRounds
constexpr int kAc = (32 * U + 1) * 16 + 48; // kmer_count3_mfma_kernel: one parity's (A, C) region
constexpr int kG = (32 * U + 1) * 16;       // ... the G nibbles

// v_perm_b32(src0, src1, sel) for selector bytes 0..7: byte sel of the 64-bit value src0:src1
uint32_t perm(uint32_t src0, uint32_t src1, uint32_t sel) {
    const uint64_t v = ((uint64_t)src0 << 32) | src1;
    uint32_t r = 0;
    for (int b = 0; b < 4; ++b) {
        const unsigned s = (sel >> (8 * b)) & 0xFF;
        CHECK(s < 8);
        r |= (uint32_t)((v >> (8 * s)) & 0xFF) << (8 * b);
    }
    return r;
}

// expand3: 16 ASCII bytes (four dwords) -> 16 (A, C) bytes and two dwords of G nibbles
void expand3(const uint32_t x[4], uint32_t ac[4], uint32_t &g0, uint32_t &g1) {
    uint32_t g[4];
    for (int i = 0; i < 4; ++i) {
        const uint32_t si = x[i] & 0x07070707u;
        ac[i] = perm(0u, 0x20000200u, si);
        g[i] = perm(0x02000000u, 0u, si);
    }
    g0 = (g[1] << 4) | g[0];
    g1 = (g[3] << 4) | g[2];
}

int fp4(uint32_t nib) { // E2M1: the operands only hold 0, 1.0 (0b0010) and -1.0 (0b1010)
    CHECK(nib == 0 || nib == 0x2 || nib == 0xA);
    return nib == 0 ? 0 : nib == 0x2 ? 1 : -1;
}

struct Trip {
    std::vector<uint8_t> bytes; // ASCII bytes of the trip's rounds + the 32-byte halo
    std::vector<uint8_t> codes;
    unsigned m;                 // valid rounds
    void load(unsigned u, unsigned lane, uint32_t x[4]) const { // lane's 16 bytes of round u (rounds past m clamped to m - 1)
        const unsigned uc = u < m ? u : m - 1;
        memcpy(x, &bytes[1024 * uc + 16 * lane], 16);
    }
    void halo(unsigned lane, uint32_t x[4]) const { memcpy(x, &bytes[1024 * m + 16 * lane], 16); }
};

Trip make_trip(unsigned m, uint64_t query, size_t k, bool hits) {
    Trip t;
    t.m = m;
    const size_t nb = 1024 * (size_t)m + 32;
    t.bytes.resize(nb);
    t.codes.resize(nb);
    for (size_t i = 0; i < nb; ++i) {
        uint8_t c = (uint8_t)(rnd64() & 3);
        if (hits && rnd64() % 8 != 0) c = (uint8_t)((query >> (2 * (i % k))) & 3); // mostly the query repeated: small distances
        t.codes[i] = c;
        t.bytes[i] = (uint8_t)("ACGT"[c] | ((rnd64() & 1) ? 0x20 : 0));
    }
    return t;
}

unsigned dist_at(const Trip &t, size_t j, uint64_t query, size_t k) {
    unsigned d = 0;
    for (size_t i = 0; i < k; ++i) d += t.codes[j + i] != ((query >> (2 * i)) & 3);
    return d;
}

void store(std::vector<uint8_t> &s, size_t off, const uint32_t *v, size_t nbytes) { CHECK(off + nbytes <= s.size()); memcpy(&s[off], v, nbytes); }
void load16(const std::vector<uint8_t> &s, size_t off, uint32_t v[4]) { CHECK(off + 16 <= s.size()); memcpy(v, &s[off], 16); }

// one MFMA row: start + scale * sum over K of A x B, every partial sum checked
long long mac_row(long long start, long long scale, const uint32_t *a, const uint32_t *b, int dwords) {
    long long acc = start;
    for (int i = 0; i < dwords; ++i)
        for (int p = 0; p < 8; ++p) {
            acc += scale * fp4((a[i] >> (4 * p)) & 0xF) * fp4((b[i] >> (4 * p)) & 0xF);
            CHECK(acc < (1ll << 24) && acc > -(1ll << 24));
        }
    return acc;
}

uint32_t f32_bits(long long v) { float f = (float)v; CHECK((long long)f == v); uint32_t u; memcpy(&u, &f, 4); return u; }

void check_count(const Trip &t, uint64_t query, size_t k, unsigned tau) {
    bitnuc_dev::Count3MfmaTable *tab = new bitnuc_dev::Count3MfmaTable;
    bitnuc_host::count3_mfma_table(query, k, tau, tab);
    std::vector<uint8_t> strip(2 * kAc + kG, 0xEE);
    for (unsigned u = 0; u < U; ++u) // every round of the trip is written (a clamped copy repeats round m - 1)
        for (unsigned lane = 0; lane < 64; ++lane) {
            uint32_t x[4], ac[4], g[2];
            t.load(u, lane, x);
            expand3(x, ac, g[0], g[1]);
            store(strip, (lane & 1) * kAc + 16 * (lane >> 1) + 512 * u, ac, 16);
            store(strip, 2 * kAc + 8 * lane + 512 * u, g, 8);
        }
    for (unsigned lane = 0; lane < 2; ++lane) { // the halo after the last valid round, written last
        uint32_t x[4], ac[4], g[2];
        t.halo(lane, x);
        expand3(x, ac, g[0], g[1]);
        store(strip, lane * kAc + 512 * t.m, ac, 16);
        store(strip, 2 * kAc + 512 * t.m + 8 * lane, g, 8);
    }
    for (unsigned u = 0; u < t.m; ++u) {
        unsigned long long hits = 0, want = 0;
        for (unsigned n = 0; n < 32; ++n)
            for (unsigned hh = 0; hh < 2; ++hh)
                for (unsigned q = 0; q < 4; ++q) {
                    // lane (n, hh), registers 4 q .. 4 q + 3 = rows 8 q + 4 hh + (0..3): the kernel's v_or3 + v_bitop3 + v_bcnt group
                    uint32_t bits[4];
                    for (unsigned jr = 0; jr < 4; ++jr) {
                        const unsigned row = 8 * q + 4 * hh + jr;
                        long long acc = (long long)tab->c[jr];
                        CHECK((float)acc == tab->c[jr]);
                        const long long scale = jr == 3 ? 2 : 1ll << (6 * jr);
                        for (unsigned h = 0; h < 2; ++h) { // K-block h: A lane row + 32 h, B lane n + 32 h
                            const unsigned lane_a = row + 32 * h;
                            for (unsigned s = 0; s < 3; ++s) {
                                uint32_t b[4];
                                const unsigned rd_ac = h * kAc + 16 * n, rd_g = 2 * kAc + 16 * (n + h);
                                load16(strip, (s < 2 ? rd_ac + 16 * s : rd_g) + 512 * u, b);
                                acc = mac_row(acc, scale, &tab->w[lane_a][4 * s], b, 4);
                            }
                        }
                        const unsigned d = dist_at(t, 1024 * u + 32 * n + row, query, k);
                        const bool hit = d <= tau;
                        want += hit;
                        if (jr < 3) {
                            CHECK(acc >= (1ll << 23) && acc < (1ll << 24));
                            const long long field = (acc - (1ll << 23)) >> (6 * jr);
                            CHECK(((acc - (1ll << 23)) & ((1ll << (6 * jr)) - 1)) == 0 && field < 64);
                            CHECK(((field >> 5) & 1) == (long long)hit); // the field's top bit says d <= tau
                        } else {
                            CHECK((acc & 1) && acc < 64 && acc > -64);
                            CHECK((acc < 0) == hit); // the sign says d <= tau
                        }
                        bits[jr] = f32_bits(acc);
                    }
                    hits += (unsigned)__builtin_popcount((bits[0] | bits[1] | bits[2] | bits[3]) & 0x80020820u);
                }
        CHECK(hits == want);
    }
    delete tab;
}

} // namespace

int main() {
    unsigned long long cases = 0;
    for (size_t k = 1; k <= 32; ++k)
        for (int rep = 0; rep < 2; ++rep) {
            const uint64_t query = rnd64(); // junk above 2 k: the tables must ignore it
            const uint64_t kmask = k == 32 ? ~0ull : (1ull << (2 * k)) - 1;
            for (unsigned m = 1; m <= 4; m += 3) {
                const Trip t = make_trip(m, query & kmask, k, rep == 1);
                const unsigned taus[6] = {0u, 1u, (unsigned)k - 1, (unsigned)k, (unsigned)k + 1, 0xFFFFFFFFu};
                for (unsigned tau : taus) check_count(t, query, k, tau), ++cases;
            }
        }
    printf("ascii scan emulation ok: %llu count cases\n", cases);
    return 0;
}
