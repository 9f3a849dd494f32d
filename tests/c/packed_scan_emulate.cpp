// CPU emulation of the packed scan and count on the matrix cores (bitnuc_amd/csrc/scan_packed_device.h), built by tests/test_packed_scan_host.py
// under AddressSanitizer + UBSan.  For one trip of m = 1..4 rounds it builds the one-hot operands from packed 2-bit codes the way the kernels do
// (s_t = (x >> 2 t) & 0x03030303, the v_perm LUTs, the G-nibble bit trick), writes them into the wave-private strip and reads them back at the
// kernels' offsets, then applies the host tables of scan_mfma_host.h (scan_packed_table, count3_packed_table), the E8M0 row scales and the accumulator
// start values in integers, in the MFMA's register layout.  It asserts, against hdist_scalar of every window:
//   * the scan's distance byte fields equal the scalar distances;
//   * the count's threshold bits equal d <= tau, and the kernel's hit mask counts exactly the windows with d <= tau;
//   * every partial sum stays an integer of magnitude below 2^24 (f32-exact).
#include "../../bitnuc_amd/csrc/scan_mfma_host.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

namespace {

uint64_t rng_state = 0x2545F4914F6CDD1Dull;
uint64_t rnd64() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

constexpr int kRegion = 65 * 16 + 16, kGRegion = 65 * 16 + 48; // scan_packed_device.h: kPackedRegion, kPackedGRegion

// v_perm_b32 with selector bytes 0..3 (the only ones the LUTs see): byte sel of src1
uint32_t perm_lut(uint32_t src1, uint32_t s) {
    uint32_t r = 0;
    for (int b = 0; b < 4; ++b) r |= ((src1 >> (8 * ((s >> (8 * b)) & 0xFF))) & 0xFF) << (8 * b);
    return r;
}
uint32_t codes_at(uint32_t x, int t) { return (x >> (2 * t)) & 0x03030303u; }
uint32_t lut_ac(uint32_t s) { return perm_lut(0x00002002u, s); }
uint32_t lut_gt(uint32_t s) { return perm_lut(0x20020000u, s); }
void g_nibbles(uint32_t x, uint32_t &ge, uint32_t &go) {
    const uint32_t y = x & ~(x << 1) & 0xAAAAAAAAu;
    ge = y & 0x22222222u;
    go = (y >> 2) & 0x22222222u;
}

int fp4(uint32_t nib) { // E2M1: the operands only hold 0, 1.0 (0b0010) and -1.0 (0b1010)
    CHECK(nib == 0 || nib == 0x2 || nib == 0xA);
    return nib == 0 ? 0 : nib == 0x2 ? 1 : -1;
}

struct Trip {
    std::vector<uint8_t> codes;  // 2-bit codes of the trip's bases + the halo
    std::vector<uint32_t> dw;    // the same, packed: dword D = bases 16 D .. 16 D + 15
    unsigned m;                  // valid rounds
    uint32_t load(unsigned lane, int i) const { // dword i of lane's 16-byte load (rounds past m clamped to m - 1)
        const unsigned ul = lane >> 4, uc = ul < m ? ul : m - 1;
        return dw[64 * uc + 4 * (lane & 15) + i];
    }
    uint32_t halo(unsigned lane) const { return dw[64 * m + lane]; }
};

Trip make_trip(unsigned m, uint64_t query, size_t k, bool hits) {
    Trip t;
    t.m = m;
    const size_t nb = 1024 * (size_t)m + 32;
    t.codes.resize(nb);
    for (size_t i = 0; i < nb; ++i) {
        if (hits && rnd64() % 8 != 0) t.codes[i] = (uint8_t)((query >> (2 * (i % k))) & 3); // mostly the query repeated: small distances
        else t.codes[i] = (uint8_t)(rnd64() & 3);
    }
    t.dw.assign((nb + 15) / 16, 0);
    for (size_t i = 0; i < nb; ++i) t.dw[i / 16] |= (uint32_t)t.codes[i] << (2 * (i % 16));
    return t;
}

unsigned dist_at(const Trip &t, size_t j, uint64_t query, size_t k) {
    unsigned d = 0;
    for (size_t i = 0; i < k; ++i) d += t.codes[j + i] != ((query >> (2 * i)) & 3);
    return d;
}

void store16(std::vector<uint8_t> &s, size_t off, const uint32_t v[4]) { CHECK(off + 16 <= s.size()); memcpy(&s[off], v, 16); }
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

void check_scan(const Trip &t, uint64_t query, size_t k) {
    bitnuc_dev::PackedScanTable *tab = new bitnuc_dev::PackedScanTable;
    bitnuc_host::scan_packed_table(query, k, tab);
    std::vector<uint8_t> strip(8 * kRegion, 0xEE);
    for (unsigned lane = 0; lane < 64; ++lane)
        for (int i = 0; i < 4; ++i) {
            const uint32_t x = t.load(lane, i);
            const uint32_t s0 = codes_at(x, 0), s1 = codes_at(x, 1), s2 = codes_at(x, 2), s3 = codes_at(x, 3);
            const uint32_t e0[4] = {lut_ac(s0), lut_gt(s0), lut_ac(s1), lut_gt(s1)}, e1[4] = {lut_ac(s2), lut_gt(s2), lut_ac(s3), lut_gt(s3)};
            store16(strip, i * kRegion + 16 * lane, e0);
            store16(strip, (4 + i) * kRegion + 16 * lane, e1);
        }
    for (unsigned lane = 0; lane < 2; ++lane) {
        const uint32_t x = t.halo(lane);
        const uint32_t s0 = codes_at(x, 0), s1 = codes_at(x, 1), s2 = codes_at(x, 2), s3 = codes_at(x, 3);
        const uint32_t e0[4] = {lut_ac(s0), lut_gt(s0), lut_ac(s1), lut_gt(s1)}, e1[4] = {lut_ac(s2), lut_gt(s2), lut_ac(s3), lut_gt(s3)};
        store16(strip, lane * kRegion + 256 * t.m, e0);
        store16(strip, (4 + lane) * kRegion + 256 * t.m, e1);
    }
    for (unsigned u = 0; u < t.m; ++u)
        for (unsigned n = 0; n < 32; ++n)
            for (unsigned row = 0; row < 32; ++row) {
                const unsigned j3 = row & 3;
                long long acc = (long long)tab->c[j3];
                CHECK(acc == (1ll << 23));
                const long long scale = j3 == 3 ? 1 : 1ll << (8 * j3);
                for (unsigned h = 0; h < 2; ++h)
                    for (unsigned j = 0; j < 4; ++j) {
                        const unsigned g = 2 * n + j;
                        uint32_t b[4];
                        load16(strip, (4 * h + (g & 3)) * kRegion + 16 * (g >> 2) + 256 * u, b);
                        const uint32_t *a = &tab->w[row + 2 - 2 * h][4 * j];
                        acc = mac_row(acc, scale, a, b, 4);
                    }
                const unsigned d = dist_at(t, 1024 * u + 32 * n + row, query, k);
                CHECK(acc - (1ll << 23) == (long long)d << (j3 == 3 ? 0 : 8 * j3)); // the byte field of this row holds d, nothing else
            }
    delete tab;
}

void check_count(const Trip &t, uint64_t query, size_t k, unsigned tau) {
    bitnuc_dev::Count3MfmaTable *tab = new bitnuc_dev::Count3MfmaTable;
    bitnuc_host::count3_packed_table(query, k, tau, tab);
    const int kG0 = 4 * kRegion;
    std::vector<uint8_t> strip(4 * kRegion + 2 * kGRegion, 0xEE);
    for (unsigned lane = 0; lane < 64; ++lane) {
        uint32_t ge[4], go[4];
        for (int i = 0; i < 4; ++i) {
            const uint32_t x = t.load(lane, i);
            const uint32_t ac[4] = {lut_ac(codes_at(x, 0)), lut_ac(codes_at(x, 1)), lut_ac(codes_at(x, 2)), lut_ac(codes_at(x, 3))};
            store16(strip, i * kRegion + 16 * lane, ac);
            g_nibbles(x, ge[i], go[i]);
        }
        const uint32_t g0[4] = {ge[0], go[0], ge[1], go[1]}, g1[4] = {ge[2], go[2], ge[3], go[3]};
        store16(strip, kG0 + 16 * lane, g0);
        store16(strip, kG0 + kGRegion + 16 * lane, g1);
    }
    for (unsigned lane = 0; lane < 2; ++lane) {
        const uint32_t x = t.halo(lane);
        const uint32_t ac[4] = {lut_ac(codes_at(x, 0)), lut_ac(codes_at(x, 1)), lut_ac(codes_at(x, 2)), lut_ac(codes_at(x, 3))};
        store16(strip, lane * kRegion + 256 * t.m, ac);
        uint32_t he, ho;
        g_nibbles(x, he, ho);
        CHECK(kG0 + 256 * t.m + 8 * lane + 8 <= strip.size());
        memcpy(&strip[kG0 + 256 * t.m + 8 * lane], &he, 4);
        memcpy(&strip[kG0 + 256 * t.m + 8 * lane + 4], &ho, 4);
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
                        for (unsigned h = 0; h < 2; ++h) {
                            const unsigned lane_a = row + 32 * h;
                            for (unsigned s = 0; s < 3; ++s) {
                                uint32_t b[4];
                                if (s < 2) {
                                    const unsigned g = 2 * n + 2 * s + h;
                                    load16(strip, (g & 3) * kRegion + 16 * (g >> 2) + 256 * u, b);
                                } else {
                                    load16(strip, kG0 + ((n + h) & 1) * kGRegion + 16 * ((n + h) >> 1) + 256 * u, b);
                                }
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
                check_scan(t, query, k);
                const unsigned taus[6] = {0u, 1u, (unsigned)k - 1, (unsigned)k, (unsigned)k + 1, 0xFFFFFFFFu};
                for (unsigned tau : taus) check_count(t, query, k, tau), ++cases;
            }
        }
    printf("packed scan emulation ok: %llu count cases\n", cases);
    return 0;
}
