// CPU-only sanitizer harness for the PRODUCT's own host code (sanitizers used to stop at the oracle):
//   * csrc/host_word.h   -- the SWAR single-word / below-cutoff codec (what bitnuc_as_2bit, bitnuc_from_2bit, bitnuc_hdist_scalar
//                           and small host-pointer bitnuc_encode / bitnuc_decode / bitnuc_hdist run), on exact-size heap buffers
//                           so that any over-read / over-write is caught, checked against the oracle;
//   * csrc/host_pool.h   -- the mover thread of the pipelined host-pointer path (TaskThread: a task queue, a mutex and two
//                           condition variables), in the call pattern of pipe_run: tickets, early drains, destruction with tasks queued;
//   * csrc/scan_mfma_host.h -- the query operand tables of the matrix-core scan and count (count_mfma_table, count3_mfma_table),
//                           built into exact-size heap objects for every k, the threshold edges and random queries.
// Built twice by tests/test_sanitizers.py: -fsanitize=address,undefined and -fsanitize=thread.  No header needs HIP.
// The reference's single-thread contract is src/utils/unpacking/avx.rs:37 (its only static); the mover thread only moves bytes.
#include "../../bitnuc_amd/csrc/host_pool.h"
#include "../../bitnuc_amd/csrc/host_word.h"
#include "../../bitnuc_amd/csrc/scan_mfma_host.h"
#include "../../oracle/bitnuc_oracle.h"

#include <atomic>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 32); }

static void host_word_checks() {
    orc_err e;
    // single words: every length 0..32, every byte value at every position (validity + first-invalid-byte index)
    for (size_t len = 0; len <= 32; ++len) {
        uint8_t *s = static_cast<uint8_t *>(malloc(len ? len : 1));
        for (size_t i = 0; i < len; ++i) s[i] = "ACGTacgt"[rnd() & 7];
        uint64_t w = 0, ow = 0;
        CHECK(bitnuc_host::pack_word(s, len, &w) == -1);
        CHECK(orc_as_2bit(s, len, &ow, &e) == ORC_OK && w == ow);
        uint8_t *back = static_cast<uint8_t *>(malloc(len ? len : 1)), *oback = static_cast<uint8_t *>(malloc(len ? len : 1));
        bitnuc_host::unpack_word(w, len, back);
        CHECK(orc_from_2bit(w, len, oback, &e) == ORC_OK && memcmp(back, oback, len) == 0);
        uint32_t d = 0;
        const uint64_t v = w ^ (((uint64_t)rnd() << 32) | rnd());
        CHECK(orc_hdist_scalar(w, v, len, &d, &e) == ORC_OK && d == bitnuc_host::hdist_word(w, v, len));
        for (size_t pos = 0; pos < len; ++pos)
            for (unsigned b = 0; b < 256; ++b) {
                const uint8_t keep = s[pos];
                s[pos] = (uint8_t)b;
                const int st = orc_as_2bit(s, len, &ow, &e);
                const int bad = bitnuc_host::pack_word(s, len, &w);
                if (st == ORC_OK) CHECK(bad == -1 && w == ow);
                else CHECK(bad == (int)e.index && s[bad] == e.byte);
                s[pos] = keep;
            }
        free(s); free(back); free(oback);
    }
    // bulk below the cutoff: every length 1..=1000 round trip (src/utils/mod.rs:113-133) + a few larger, exact-size buffers
    for (size_t n = 1; n <= 1400; n = n < 1000 ? n + 1 : n + 97) {
        uint8_t *s = static_cast<uint8_t *>(malloc(n));
        for (size_t i = 0; i < n; ++i) s[i] = "ACGTacgt"[rnd() & 7];
        const size_t nw = (n + 31) / 32;
        uint64_t *words = static_cast<uint64_t *>(malloc(nw * 8)), *owords = static_cast<uint64_t *>(malloc(nw * 8));
        size_t got = 0;
        CHECK(bitnuc_host::encode_small(s, n, words) == -1);
        CHECK(orc_encode(s, n, owords, &got, &e) == ORC_OK && got == nw && memcmp(words, owords, nw * 8) == 0);
        uint8_t *back = static_cast<uint8_t *>(malloc(n)), *oback = static_cast<uint8_t *>(malloc(n));
        bitnuc_host::decode_small(words, n, back);
        CHECK(orc_decode(words, nw, n, oback, &e) == ORC_OK && memcmp(back, oback, n) == 0);
        uint32_t hd = 0;
        for (size_t i = 0; i < nw; ++i) owords[i] = words[i] ^ (((uint64_t)rnd() << 32) | rnd());
        CHECK(orc_hdist(words, nw, owords, nw, n, &hd, &e) == ORC_OK && hd == bitnuc_host::hdist_small(words, owords, n));
        // first invalid byte in sequence order, and the words before the failing chunk (packing/avx.rs:86-91,142-143)
        const size_t p1 = rnd() % n, p2 = p1 + (rnd() % (n - p1));
        s[p2] = 'X';
        s[p1] = 'N';
        memset(words, 0xEE, nw * 8);
        const long long bad = bitnuc_host::encode_small(s, n, words);
        CHECK(orc_encode(s, n, owords, &got, &e) == ORC_INVALID_BASE);
        CHECK(bad == (long long)e.index && (size_t)bad == p1 && got == p1 / 32 && memcmp(words, owords, got * 8) == 0);
        free(s); free(words); free(owords); free(back); free(oback);
    }
}

// the call pattern of pipe_run (csrc/host_pipe.h): the poster fills device-buffer stand-in b = ci % depth itself ("H2D"), posts the
// chunk's hand-back to the mover, and before it refills b waits for the ticket of the chunk that used b; an error code travels
// back through an atomic the tasks write; leaving early drains; destruction runs what is still queued.
static void task_thread_checks() {
    using bitnuc_host::TaskThread;
    const size_t sizes[] = {0, 1, 4097, (1u << 20) + 1, (3u << 20) + 5};
    TaskThread w;
    for (size_t n : sizes) {
        const int depth = 3, nchunks = 11;
        uint8_t *src = static_cast<uint8_t *>(malloc(n * nchunks + 1)), *dst = static_cast<uint8_t *>(malloc(n * nchunks + 1));
        for (size_t i = 0; i < n * nchunks; ++i) src[i] = (uint8_t)(i * 29 + (i >> 7));
        memset(dst, 0, n * nchunks + 1);
        uint8_t *devbuf[3];
        for (int b = 0; b < depth; ++b) devbuf[b] = static_cast<uint8_t *>(malloc(n + 1));
        std::atomic<int> rc{0};
        const uint64_t base = w.tickets();
        for (int ci = 0; ci < nchunks; ++ci) {
            const int b = ci % depth;
            if (ci >= depth) w.wait_done(base + (uint64_t)(ci - depth) + 1);
            memcpy(devbuf[b], src + (size_t)ci * n, n);
            uint8_t *from = devbuf[b], *to = dst + (size_t)ci * n;
            const uint64_t t = w.post([=, &rc] { memcpy(to, from, n); if (ci == 7) rc.store(7); });
            CHECK(t == base + (uint64_t)ci + 1);
        }
        w.drain();
        CHECK(rc.load() == 7 && memcmp(src, dst, n * nchunks) == 0);
        for (int b = 0; b < depth; ++b) free(devbuf[b]);
        free(src); free(dst);
    }
    w.drain(); // nothing outstanding: returns at once
    std::atomic<int> ran{0};
    {
        TaskThread tmp;
        for (int i = 0; i < 50; ++i) tmp.post([&ran] { ++ran; });
    } // ~TaskThread runs what is queued, then joins
    CHECK(ran.load() == 50);
    { TaskThread idle; } // never used
}

// The table builders index the query's planes at src[32 + p0 + b - d] (d = -8 .. 31) and the lanes' operand positions: every k, the
// threshold's edges and random queries, into exact-size heap objects.  A threshold no window can miss (tau >= k) gives all-zero words and
// the start values of tau = k: 2^23 + 32 * 2^(6 j) for j < 3, -1 for j = 3.
static void table_checks() {
    using bitnuc_host::CountMfmaTable;
    using bitnuc_host::Count3MfmaTable;
    CountMfmaTable *t = static_cast<CountMfmaTable *>(malloc(sizeof(CountMfmaTable)));
    Count3MfmaTable *t3 = static_cast<Count3MfmaTable *>(malloc(sizeof(Count3MfmaTable)));
    for (size_t k = 1; k <= 32; ++k) {
        const unsigned taus[] = {0u, 1u, (unsigned)k - 1, (unsigned)k, (unsigned)k + 1, 0xFFFFFFFFu};
        for (int qi = 0; qi < 8; ++qi) {
            const uint64_t query = qi == 0 ? 0 : qi == 1 ? ~0ull : (((uint64_t)rnd() << 32) | rnd());
            uint32_t ql, qh;
            bitnuc_host::query_planes(query, k, &ql, &qh);
            for (size_t i = 0; i < k; ++i) CHECK(((ql >> i) & 1) == ((query >> (2 * i)) & 1) && ((qh >> i) & 1) == ((query >> (2 * i + 1)) & 1));
            bitnuc_host::count_mfma_table(query, k, t); // the scan's operand: no threshold, accumulators from 0
            for (int j = 0; j < 4; ++j) CHECK(t->c[j] == 0.f);
            for (unsigned tau : taus)
                for (int match = 0; match < 2; ++match) {
                    bitnuc_host::count_mfma_table(query, k, t, true, tau, match != 0);
                    bitnuc_host::count3_mfma_table(query, k, tau, t3);
                    if (tau < k) continue;
                    for (int j = 0; j < 4; ++j) {
                        const float want = j < 3 ? 8388608.f + (float)(32u << (6 * j)) : -1.f;
                        CHECK(t->c[j] == want && t3->c[j] == want);
                    }
                    for (size_t r = 0; r < 40; ++r) for (uint32_t w : t->w[r]) CHECK(w == 0);
                    for (size_t r = 0; r < 64; ++r) for (uint32_t w : t3->w[r]) CHECK(w == 0);
                }
            bitnuc_host::count3_mfma_table(query, k, 0u, t3, true); // the evidence build's three-channel scan
        }
    }
    free(t);
    free(t3);
}

int main() {
    host_word_checks();
    table_checks();
    task_thread_checks();
    printf("host sanitizer harness ok\n");
    return 0;
}
