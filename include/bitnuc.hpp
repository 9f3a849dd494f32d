// bitnuc.hpp -- compiled host layer over the C ABI (include/bitnuc_hip.h) that mirrors
// bitnuc's public Rust API (src/lib.rs:214-220) in C++: same names, argument meaning,
// Vec clear/append conventions and error values, so that code (and tests) written
// against the reference read the same here.  north_star asks for this layer in Rust;
// the image has no rustc/cargo, so the Rust shim is source-only (rust/) and this
// header is the layer that is compiled and tested.  Header-only; link -lbitnuc_hip.
//
//   Rust                                               C++
//   as_2bit(&[u8]) -> Result<u64, NucleotideError>     Result<uint64_t> as_2bit(bytes)
//   from_2bit(u64, usize, &mut Vec<u8>) -> Result<()>  Result<void> from_2bit(p, n, std::vector<uint8_t>&)
//   from_2bit_alloc(u64, usize) -> Result<Vec<u8>>     Result<std::vector<uint8_t>> from_2bit_alloc(p, n)
//   encode(&[u8], &mut Vec<u64>) -> Result<()>         Result<void> encode(bytes, std::vector<uint64_t>&)
//   encode_alloc(&[u8]) -> Result<Vec<u64>>            Result<std::vector<uint64_t>> encode_alloc(bytes)
//   decode(&[u64], usize, &mut Vec<u8>) -> Result<()>  Result<void> decode(words, n, std::vector<uint8_t>&)
//   hdist_scalar(u64, u64, usize) -> Result<u32>       Result<uint32_t> hdist_scalar(u, v, len)
//   hdist(&[u64], &[u64], usize) -> Result<u32>        Result<uint32_t> hdist(a, b, n)
//   split_packed(&[u64], usize, usize, &mut Vec<u64>, &mut Vec<u64>) -> Result<()>
//                                                      Result<void> split_packed(words, slen, idx, lbuf&, rbuf&)
//
// Every function computes on the GPU through libbitnuc_hip.so; there is no CPU path.
#pragma once

#include "bitnuc_hip.h"

#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <string_view>
#include <utility>
#include <vector>

namespace bitnuc {

// src/error.rs:3-18
struct NucleotideError {
    enum Kind { InvalidBase, SequenceTooLong, InvalidLength, IndexOutOfBounds, InvalidRange, Unsupported, Backend };
    Kind kind = Unsupported;
    uint8_t base = 0;       // InvalidBase(u8)
    size_t len = 0;         // SequenceTooLong(usize) / InvalidLength(usize)
    uint64_t index = 0;     // extra: absolute index of the invalid base
    int backend_code = 0;   // extra: hipError_t for Backend
    size_t start = 0, end = 0, length = 0, oob_index = 0; // IndexOutOfBounds{index,length} / InvalidRange{start,end,length}

    static NucleotideError invalid_base(uint8_t b) { NucleotideError e; e.kind = InvalidBase; e.base = b; return e; }
    static NucleotideError sequence_too_long(size_t n) { NucleotideError e; e.kind = SequenceTooLong; e.len = n; return e; }
    static NucleotideError invalid_length(size_t n) { NucleotideError e; e.kind = InvalidLength; e.len = n; return e; }
    static NucleotideError unsupported() { NucleotideError e; e.kind = Unsupported; return e; }

    // derive(PartialEq, Eq): variant + payload
    bool operator==(const NucleotideError &o) const {
        if (kind != o.kind) return false;
        if (kind == InvalidBase) return base == o.base;
        if (kind == SequenceTooLong || kind == InvalidLength) return len == o.len;
        if (kind == IndexOutOfBounds) return oob_index == o.oob_index && length == o.length;
        if (kind == InvalidRange) return start == o.start && end == o.end && length == o.length;
        return true;
    }
    bool operator!=(const NucleotideError &o) const { return !(*this == o); }

    std::string to_string() const { // Display, src/error.rs:20-45
        switch (kind) {
        case InvalidBase: return "Invalid nucleotide base: " + std::to_string(base);
        case SequenceTooLong: return "Sequence length " + std::to_string(len) + " exceeds maximum";
        case InvalidLength: return "Invalid length: " + std::to_string(len);
        case IndexOutOfBounds: return "Index " + std::to_string(oob_index) + " out of bounds for sequence of length " + std::to_string(length);
        case InvalidRange: return "Invalid range " + std::to_string(start) + ".." + std::to_string(end) + " for sequence of length " + std::to_string(length);
        case Unsupported: return "Unsupported architecture";
        case Backend: return "HIP backend error " + std::to_string(backend_code);
        default: return "NucleotideError";
        }
    }

    static NucleotideError from_c(const bitnuc_err &e) {
        NucleotideError r;
        switch (e.status) {
        case BITNUC_INVALID_BASE: r.kind = InvalidBase; r.base = e.byte; r.index = e.index; break;
        case BITNUC_SEQUENCE_TOO_LONG: r.kind = SequenceTooLong; r.len = (size_t)e.value; break;
        case BITNUC_INVALID_LENGTH: r.kind = InvalidLength; r.len = (size_t)e.value; break;
        case BITNUC_INDEX_OUT_OF_BOUNDS: r.kind = IndexOutOfBounds; r.oob_index = (size_t)e.index; r.length = (size_t)e.value; break;
        case BITNUC_INVALID_RANGE: r.kind = InvalidRange; break;
        case BITNUC_BACKEND_ERROR: r.kind = Backend; r.backend_code = e.backend_code; break;
        default: r.kind = Unsupported; break;
        }
        return r;
    }
};

// A small Result<T, NucleotideError>.
template <class T> class Result {
  public:
    Result(T v) : ok_(true), val_(std::move(v)) {}
    Result(NucleotideError e) : ok_(false), err_(e) {}
    bool is_ok() const { return ok_; }
    bool is_err() const { return !ok_; }
    T &unwrap() { if (!ok_) throw std::runtime_error("called unwrap() on an Err value: " + err_.to_string()); return val_; }
    const NucleotideError &unwrap_err() const { if (ok_) throw std::runtime_error("called unwrap_err() on an Ok value"); return err_; }
    bool operator==(const Result &o) const { return ok_ == o.ok_ && (ok_ ? val_ == o.val_ : err_ == o.err_); }
  private:
    bool ok_;
    T val_{};
    NucleotideError err_{};
};
template <> class Result<void> {
  public:
    Result() : ok_(true) {}
    Result(NucleotideError e) : ok_(false), err_(e) {}
    bool is_ok() const { return ok_; }
    bool is_err() const { return !ok_; }
    void unwrap() const { if (!ok_) throw std::runtime_error("called unwrap() on an Err value: " + err_.to_string()); }
    const NucleotideError &unwrap_err() const { if (ok_) throw std::runtime_error("called unwrap_err() on an Ok value"); return err_; }
  private:
    bool ok_;
    NucleotideError err_{};
};
template <class T> Result<T> Ok(T v) { return Result<T>(std::move(v)); }
inline Result<void> Ok() { return Result<void>(); }

// &[u8]
struct Bytes {
    const uint8_t *ptr;
    size_t len;
    Bytes(const uint8_t *p, size_t n) : ptr(p), len(n) {}
    Bytes(const std::vector<uint8_t> &v) : ptr(v.data()), len(v.size()) {}
    Bytes(std::string_view s) : ptr(reinterpret_cast<const uint8_t *>(s.data())), len(s.size()) {}
    Bytes(const char *s) : Bytes(std::string_view(s)) {}
    Bytes(const std::string &s) : Bytes(std::string_view(s)) {}
};
// &[u64]
struct Words {
    const uint64_t *ptr;
    size_t len;
    Words(const uint64_t *p, size_t n) : ptr(p), len(n) {}
    Words(const std::vector<uint64_t> &v) : ptr(v.data()), len(v.size()) {}
};

// One device + stream + scratch.  Not shareable between threads concurrently.
class Context {
  public:
    explicit Context(int device = 0) {
        bitnuc_err e;
        if (bitnuc_ctx_create(device, &ctx_, &e) != BITNUC_OK)
            throw std::runtime_error("bitnuc: cannot create a HIP context (" + NucleotideError::from_c(e).to_string() +
                                     "); there is no CPU fallback");
    }
    ~Context() { bitnuc_ctx_destroy(ctx_); }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    bitnuc_ctx *raw() const { return ctx_; }

    Result<uint64_t> as_2bit(Bytes seq) const { // src/utils/packing/mod.rs:80-110
        uint64_t out = 0;
        bitnuc_err e;
        if (bitnuc_as_2bit(ctx_, seq.ptr, seq.len, &out, &e) != BITNUC_OK) return NucleotideError::from_c(e);
        return out;
    }
    Result<void> from_2bit(uint64_t packed, size_t expected_size, std::vector<uint8_t> &sequence) const { // unpacking/mod.rs:119-147
        uint8_t tmp[32];
        bitnuc_err e;
        if (bitnuc_from_2bit(ctx_, packed, expected_size, tmp, &e) != BITNUC_OK) return NucleotideError::from_c(e);
        sequence.insert(sequence.end(), tmp, tmp + expected_size); // appends (unpacking/avx.rs:59,73)
        return Ok();
    }
    Result<std::vector<uint8_t>> from_2bit_alloc(uint64_t packed, size_t expected_size) const { // unpacking/mod.rs:178-182
        std::vector<uint8_t> v;
        v.reserve(expected_size <= 32 ? expected_size : 0);
        Result<void> r = from_2bit(packed, expected_size, v);
        if (r.is_err()) return r.unwrap_err();
        return v;
    }
    Result<void> encode(Bytes sequence, std::vector<uint64_t> &ebuf) const { // src/utils/mod.rs:22-25
        ebuf.clear();                                                         // packing/avx.rs:132
        if (sequence.len == 0) // packing/avx.rs:138: `0..n_chunks - 1` underflows -> panic
            throw std::logic_error("attempt to subtract with overflow (encode of an empty sequence panics in the reference)");
        ebuf.resize((sequence.len + 31) / 32);
        size_t nw = 0;
        bitnuc_err e;
        int st = bitnuc_encode(ctx_, sequence.ptr, sequence.len, ebuf.data(), &nw, &e);
        ebuf.resize(nw); // on Err: the words pushed before the failing chunk (avx.rs:142-143)
        if (st != BITNUC_OK) return NucleotideError::from_c(e);
        return Ok();
    }
    Result<std::vector<uint64_t>> encode_alloc(Bytes sequence) const { // src/utils/mod.rs:38-42
        std::vector<uint64_t> ebuf;
        Result<void> r = encode(sequence, ebuf);
        if (r.is_err()) return r.unwrap_err();
        return ebuf;
    }
    Result<void> decode(Words ebuf, size_t n_bases, std::vector<uint8_t> &dbuf) const { // src/utils/mod.rs:60-62
        const size_t old = dbuf.size();
        dbuf.resize(old + n_bases); // appends (unpacking/avx.rs:122,140)
        bitnuc_err e;
        if (bitnuc_decode(ctx_, ebuf.ptr, ebuf.len, n_bases, dbuf.data() + old, &e) != BITNUC_OK) {
            dbuf.resize(old);
            return NucleotideError::from_c(e);
        }
        return Ok();
    }
    Result<uint32_t> hdist_scalar(uint64_t u, uint64_t v, size_t len) const { // hamming/scalar.rs:11-48
        uint32_t out = 0;
        bitnuc_err e;
        if (bitnuc_hdist_scalar(ctx_, u, v, len, &out, &e) != BITNUC_OK) return NucleotideError::from_c(e);
        return out;
    }
    Result<uint32_t> hdist(Words a, Words b, size_t n_bases) const { // hamming/multi.rs:121-160
        uint32_t out = 0;
        bitnuc_err e;
        if (bitnuc_hdist(ctx_, a.ptr, a.len, b.ptr, b.len, n_bases, &out, &e) != BITNUC_OK) return NucleotideError::from_c(e);
        return out;
    }
    // split_packed(ebuf, slen, idx, &mut lbuf, &mut rbuf)  functions/split.rs:15-99: validates, clears both
    // vectors, fills them.  canonical = false: the reference's words as written; true: encode(seq[..idx]) /
    // encode(seq[idx..]) (see include/bitnuc_hip.h).
    Result<void> split_packed(Words ebuf, size_t slen, size_t idx, std::vector<uint64_t> &lbuf, std::vector<uint64_t> &rbuf,
                              bool canonical = false) const {
        const int flags = canonical ? BITNUC_SPLIT_CANONICAL : BITNUC_SPLIT_AS_WRITTEN;
        size_t nl = 0, nr = 0;
        bitnuc_err e;
        if (bitnuc_split_packed_sizes(ebuf.len, slen, idx, flags, &nl, &nr, &e) != BITNUC_OK) return NucleotideError::from_c(e);
        lbuf.assign(nl, 0);
        rbuf.assign(nr, 0);
        if (bitnuc_split_packed(ctx_, ebuf.ptr, ebuf.len, slen, idx, flags, lbuf.data(), &nl, rbuf.data(), &nr, &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return Result<void>();
    }
    // batched forms of the README.md:52-56 / src/lib.rs:170-173 host loops
    Result<std::vector<uint64_t>> as_2bit_batch(Bytes kmers, size_t k, size_t stride, size_t count) const {
        std::vector<uint64_t> out(count);
        bitnuc_err e;
        if (count && k && k <= 32 && (count - 1) * stride + k > kmers.len) return NucleotideError::unsupported(); // slice too short for the batch
        if (bitnuc_as_2bit_batch(ctx_, kmers.ptr, k, stride, count, out.data(), &e) != BITNUC_OK) return NucleotideError::from_c(e);
        return out;
    }
    Result<std::vector<uint8_t>> kmer_hdist_scan(Bytes ref, size_t k, uint64_t query) const {
        std::vector<uint8_t> out((k && ref.len >= k) ? ref.len - k + 1 : 0);
        bitnuc_err e;
        if (bitnuc_kmer_hdist_scan(ctx_, ref.ptr, ref.len, k, query, out.data(), &e) != BITNUC_OK) return NucleotideError::from_c(e);
        return out;
    }
    // the same scan and its fused count on a packed sequence of n bases (as encode writes it), without decoding it
    Result<std::vector<uint8_t>> kmer_hdist_scan_packed(Words words, size_t n, size_t k, uint64_t query) const {
        std::vector<uint8_t> out((k && n >= k) ? n - k + 1 : 0);
        bitnuc_err e;
        if (bitnuc_kmer_hdist_scan_packed(ctx_, words.ptr, words.len, n, k, query, out.data(), &e) != BITNUC_OK) return NucleotideError::from_c(e);
        return out;
    }
    Result<uint64_t> kmer_hdist_count_packed(Words words, size_t n, size_t k, uint64_t query, unsigned tau) const {
        uint64_t count = 0;
        bitnuc_err e;
        if (bitnuc_kmer_hdist_count_packed(ctx_, words.ptr, words.len, n, k, query, tau, &count, &e) != BITNUC_OK) return NucleotideError::from_c(e);
        return count;
    }
    // the positions (ascending) of the windows with distance <= tau, sized by a first call with cap 0; hit_dist, when given, gets their distances
    Result<std::vector<uint64_t>> kmer_hdist_hits(Bytes ref, size_t k, uint64_t query, unsigned tau, std::vector<uint8_t> *hit_dist = nullptr) const {
        uint64_t total = 0;
        bitnuc_err e;
        if (bitnuc_kmer_hdist_hits(ctx_, ref.ptr, ref.len, k, query, tau, nullptr, nullptr, 0, &total, &e) != BITNUC_OK) return NucleotideError::from_c(e);
        std::vector<uint64_t> pos((size_t)total);
        if (hit_dist) hit_dist->assign((size_t)total, 0);
        if (total && bitnuc_kmer_hdist_hits(ctx_, ref.ptr, ref.len, k, query, tau, pos.data(), hit_dist ? hit_dist->data() : nullptr, pos.size(), &total, &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return pos;
    }
    // counts[q] = windows with distance <= taus[q] to queries[q], every query in one pass (taus.size() == queries.size())
    Result<std::vector<uint64_t>> kmer_hdist_count_multi(Bytes ref, size_t k, const std::vector<uint64_t> &queries, const std::vector<uint32_t> &taus) const {
        if (taus.size() != queries.size()) return NucleotideError::unsupported();
        std::vector<uint64_t> counts(queries.size());
        bitnuc_err e;
        if (bitnuc_kmer_hdist_count_multi(ctx_, ref.ptr, ref.len, k, queries.data(), taus.data(), queries.size(), counts.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return counts;
    }
    Result<std::vector<uint64_t>> kmer_hdist_count_multi_packed(Words words, size_t n, size_t k, const std::vector<uint64_t> &queries, const std::vector<uint32_t> &taus) const {
        if (taus.size() != queries.size()) return NucleotideError::unsupported();
        std::vector<uint64_t> counts(queries.size());
        bitnuc_err e;
        if (bitnuc_kmer_hdist_count_multi_packed(ctx_, words.ptr, words.len, n, k, queries.data(), taus.data(), queries.size(), counts.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return counts;
    }
    // the best match per query in one pass: (pos[q], dist[q]) = the leftmost window with the smallest distance to queries[q] and that distance
    // (no windows: UINT64_MAX / 0xFF)
    Result<std::pair<std::vector<uint64_t>, std::vector<uint8_t>>> kmer_hdist_best(Bytes ref, size_t k, const std::vector<uint64_t> &queries) const {
        std::vector<uint64_t> pos(queries.size());
        std::vector<uint8_t> dist(queries.size());
        bitnuc_err e;
        if (bitnuc_kmer_hdist_best(ctx_, ref.ptr, ref.len, k, queries.data(), queries.size(), pos.data(), dist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return std::make_pair(std::move(pos), std::move(dist));
    }
    Result<std::pair<std::vector<uint64_t>, std::vector<uint8_t>>> kmer_hdist_best_packed(Words words, size_t n, size_t k, const std::vector<uint64_t> &queries) const {
        std::vector<uint64_t> pos(queries.size());
        std::vector<uint8_t> dist(queries.size());
        bitnuc_err e;
        if (bitnuc_kmer_hdist_best_packed(ctx_, words.ptr, words.len, n, k, queries.data(), queries.size(), pos.data(), dist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return std::make_pair(std::move(pos), std::move(dist));
    }
    // the mismatch histogram per query in one pass: hist[q * n_bins + d] = the windows at distance exactly d < n_bins (<= BITNUC_HIST_MAX_BINS) from
    // queries[q]; a window at n_bins or more mismatches is counted nowhere
    Result<std::vector<uint64_t>> kmer_hdist_hist(Bytes ref, size_t k, const std::vector<uint64_t> &queries, size_t n_bins) const {
        std::vector<uint64_t> hist(queries.size() * (n_bins < BITNUC_HIST_MAX_BINS ? n_bins : BITNUC_HIST_MAX_BINS)); // (a refused n_bins writes nothing)
        bitnuc_err e;
        if (bitnuc_kmer_hdist_hist(ctx_, ref.ptr, ref.len, k, queries.data(), queries.size(), n_bins, hist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return hist;
    }
    Result<std::vector<uint64_t>> kmer_hdist_hist_packed(Words words, size_t n, size_t k, const std::vector<uint64_t> &queries, size_t n_bins) const {
        std::vector<uint64_t> hist(queries.size() * (n_bins < BITNUC_HIST_MAX_BINS ? n_bins : BITNUC_HIST_MAX_BINS)); // (a refused n_bins writes nothing)
        bitnuc_err e;
        if (bitnuc_kmer_hdist_hist_packed(ctx_, words.ptr, words.len, n, k, queries.data(), queries.size(), n_bins, hist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return hist;
    }
    // the best match per read of a fixed-length batch: (query, pos, dist) per read, the smallest (distance, query, offset) over the windows inside it
    struct ReadsBest { std::vector<uint32_t> query, pos; std::vector<uint8_t> dist; };
    Result<ReadsBest> reads_hdist_best(Bytes reads, size_t read_len, size_t k, const std::vector<uint64_t> &queries) const {
        const size_t count = read_len ? reads.len / read_len : 0;
        ReadsBest b{std::vector<uint32_t>(count), std::vector<uint32_t>(count), std::vector<uint8_t>(count)};
        bitnuc_err e;
        if (bitnuc_reads_hdist_best(ctx_, reads.ptr, read_len, count, k, queries.data(), queries.size(), b.query.data(), b.pos.data(), b.dist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return b;
    }
    // ... of the packed words encode_fixed writes: words.len >= count * ceil(read_len / 32)
    Result<ReadsBest> reads_hdist_best_packed(Words words, size_t read_len, size_t count, size_t k, const std::vector<uint64_t> &queries) const {
        ReadsBest b{std::vector<uint32_t>(count), std::vector<uint32_t>(count), std::vector<uint8_t>(count)};
        bitnuc_err e;
        if (bitnuc_reads_hdist_best_packed(ctx_, words.ptr, read_len, count, k, queries.data(), queries.size(), b.query.data(), b.pos.data(), b.dist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return b;
    }
    // the best match and the runner-up per read: `second` is the smallest (distance, query, offset) over the queries other than the winner's (with one
    // query: UINT32_MAX, UINT32_MAX, 0xFF)
    struct ReadsBest2 { ReadsBest best, second; };
    Result<ReadsBest2> reads_hdist_best2(Bytes reads, size_t read_len, size_t k, const std::vector<uint64_t> &queries) const {
        const size_t count = read_len ? reads.len / read_len : 0;
        ReadsBest2 b{{std::vector<uint32_t>(count), std::vector<uint32_t>(count), std::vector<uint8_t>(count)},
                     {std::vector<uint32_t>(count), std::vector<uint32_t>(count), std::vector<uint8_t>(count)}};
        bitnuc_err e;
        if (bitnuc_reads_hdist_best2(ctx_, reads.ptr, read_len, count, k, queries.data(), queries.size(), b.best.query.data(), b.best.pos.data(), b.best.dist.data(),
                                     b.second.query.data(), b.second.pos.data(), b.second.dist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return b;
    }
    Result<ReadsBest2> reads_hdist_best2_packed(Words words, size_t read_len, size_t count, size_t k, const std::vector<uint64_t> &queries) const {
        ReadsBest2 b{{std::vector<uint32_t>(count), std::vector<uint32_t>(count), std::vector<uint8_t>(count)},
                     {std::vector<uint32_t>(count), std::vector<uint32_t>(count), std::vector<uint8_t>(count)}};
        bitnuc_err e;
        if (bitnuc_reads_hdist_best2_packed(ctx_, words.ptr, read_len, count, k, queries.data(), queries.size(), b.best.query.data(), b.best.pos.data(),
                                            b.best.dist.data(), b.second.query.data(), b.second.pos.data(), b.second.dist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return b;
    }
    // the anchored best match and runner-up per read: reads_hdist_best2 over the offsets pos_lo <= i <= min(pos_hi, read_len - k) only (pos_hi = SIZE_MAX:
    // to the end of the read; the span hi - pos_lo + k may not exceed BITNUC_ANCHOR_MAX_SPAN); positions are offsets in the read
    Result<ReadsBest2> reads_hdist_anchored(Bytes reads, size_t read_len, size_t k, const std::vector<uint64_t> &queries, size_t pos_lo = 0,
                                            size_t pos_hi = SIZE_MAX) const {
        const size_t count = read_len ? reads.len / read_len : 0;
        ReadsBest2 b{{std::vector<uint32_t>(count), std::vector<uint32_t>(count), std::vector<uint8_t>(count)},
                     {std::vector<uint32_t>(count), std::vector<uint32_t>(count), std::vector<uint8_t>(count)}};
        bitnuc_err e;
        if (bitnuc_reads_hdist_anchored(ctx_, reads.ptr, read_len, count, k, pos_lo, pos_hi, queries.data(), queries.size(), b.best.query.data(), b.best.pos.data(),
                                        b.best.dist.data(), b.second.query.data(), b.second.pos.data(), b.second.dist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return b;
    }
    Result<ReadsBest2> reads_hdist_anchored_packed(Words words, size_t read_len, size_t count, size_t k, const std::vector<uint64_t> &queries, size_t pos_lo = 0,
                                                   size_t pos_hi = SIZE_MAX) const {
        ReadsBest2 b{{std::vector<uint32_t>(count), std::vector<uint32_t>(count), std::vector<uint8_t>(count)},
                     {std::vector<uint32_t>(count), std::vector<uint32_t>(count), std::vector<uint8_t>(count)}};
        bitnuc_err e;
        if (bitnuc_reads_hdist_anchored_packed(ctx_, words.ptr, read_len, count, k, pos_lo, pos_hi, queries.data(), queries.size(), b.best.query.data(),
                                               b.best.pos.data(), b.best.dist.data(), b.second.query.data(), b.second.pos.data(), b.second.dist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return b;
    }
    // ... of a ragged batch: read r is seq[offsets[r] .. offsets[r + 1]) (offsets: count + 1 non-decreasing entries from 0, seq.len >= offsets.back())
    Result<ReadsBest> reads_hdist_best_batch(Bytes seq, const std::vector<uint64_t> &offsets, size_t k, const std::vector<uint64_t> &queries) const {
        const size_t count = offsets.empty() ? 0 : offsets.size() - 1;
        if (count && seq.len < offsets.back()) return NucleotideError::invalid_length(seq.len); // seq does not hold offsets.back() bases
        ReadsBest b{std::vector<uint32_t>(count), std::vector<uint32_t>(count), std::vector<uint8_t>(count)};
        bitnuc_err e;
        if (bitnuc_reads_hdist_best_batch(ctx_, seq.ptr, offsets.data(), count, k, queries.data(), queries.size(), b.query.data(), b.pos.data(), b.dist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return b;
    }
    // ... of the packed words encode_batch writes: read r's words start at words[word_offsets[r]] (word_offsets.size() == offsets.size())
    Result<ReadsBest> reads_hdist_best_batch_packed(Words words, const std::vector<uint64_t> &word_offsets, const std::vector<uint64_t> &offsets, size_t k,
                                                    const std::vector<uint64_t> &queries) const {
        const size_t count = offsets.empty() ? 0 : offsets.size() - 1;
        if (word_offsets.size() != offsets.size()) return NucleotideError::unsupported(); // one word offset per base offset: the call reads count + 1 of each
        if (count && words.len < word_offsets.back()) return NucleotideError::invalid_length(words.len); // words does not hold word_offsets.back() words
        ReadsBest b{std::vector<uint32_t>(count), std::vector<uint32_t>(count), std::vector<uint8_t>(count)};
        bitnuc_err e;
        if (bitnuc_reads_hdist_best_batch_packed(ctx_, words.ptr, word_offsets.data(), offsets.data(), count, k, queries.data(), queries.size(), b.query.data(), b.pos.data(),
                                                 b.dist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return b;
    }
    // the anchored best match and runner-up per read of a ragged batch: anchor = BITNUC_ANCHOR_START admits pos_lo <= i <= min(pos_hi, len_r - k),
    // BITNUC_ANCHOR_END the i with pos_lo <= len_r - k - i <= pos_hi (END, 0, 3: the last k bases with three bases of slack); pos_hi - pos_lo + k may not
    // exceed BITNUC_ANCHOR_MAX_SPAN; a read without an admissible window gets the fill; positions are offsets from the read's start
    Result<ReadsBest2> reads_hdist_anchored_batch(Bytes seq, const std::vector<uint64_t> &offsets, size_t k, const std::vector<uint64_t> &queries, size_t pos_lo = 0,
                                                  size_t pos_hi = 0, int anchor = BITNUC_ANCHOR_START) const {
        const size_t count = offsets.empty() ? 0 : offsets.size() - 1;
        if (count && seq.len < offsets.back()) return NucleotideError::invalid_length(seq.len); // seq does not hold offsets.back() bases
        ReadsBest2 b{{std::vector<uint32_t>(count), std::vector<uint32_t>(count), std::vector<uint8_t>(count)},
                     {std::vector<uint32_t>(count), std::vector<uint32_t>(count), std::vector<uint8_t>(count)}};
        bitnuc_err e;
        if (bitnuc_reads_hdist_anchored_batch(ctx_, seq.ptr, offsets.data(), count, k, anchor, pos_lo, pos_hi, queries.data(), queries.size(), b.best.query.data(),
                                              b.best.pos.data(), b.best.dist.data(), b.second.query.data(), b.second.pos.data(), b.second.dist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return b;
    }
    Result<ReadsBest2> reads_hdist_anchored_batch_packed(Words words, const std::vector<uint64_t> &word_offsets, const std::vector<uint64_t> &offsets, size_t k,
                                                         const std::vector<uint64_t> &queries, size_t pos_lo = 0, size_t pos_hi = 0,
                                                         int anchor = BITNUC_ANCHOR_START) const {
        const size_t count = offsets.empty() ? 0 : offsets.size() - 1;
        if (word_offsets.size() != offsets.size()) return NucleotideError::unsupported(); // one word offset per base offset: the call reads count + 1 of each
        if (count && words.len < word_offsets.back()) return NucleotideError::invalid_length(words.len); // words does not hold word_offsets.back() words
        ReadsBest2 b{{std::vector<uint32_t>(count), std::vector<uint32_t>(count), std::vector<uint8_t>(count)},
                     {std::vector<uint32_t>(count), std::vector<uint32_t>(count), std::vector<uint8_t>(count)}};
        bitnuc_err e;
        if (bitnuc_reads_hdist_anchored_batch_packed(ctx_, words.ptr, word_offsets.data(), offsets.data(), count, k, anchor, pos_lo, pos_hi, queries.data(),
                                                     queries.size(), b.best.query.data(), b.best.pos.data(), b.best.dist.data(), b.second.query.data(),
                                                     b.second.pos.data(), b.second.dist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return b;
    }
    // the per-read matchers under PATTERN queries (a set of bases per position: bitnuc_pattern_from_iupac / _from_2bit): the ten methods above with
    // `patterns` where `queries` stood and pdist where the Hamming distance stood; ties, fills, runner-up rule and the validation of the reads unchanged
    static ReadsBest reads_outputs(size_t count) { return ReadsBest{std::vector<uint32_t>(count), std::vector<uint32_t>(count), std::vector<uint8_t>(count)}; }
    Result<ReadsBest> reads_pattern_best(Bytes reads, size_t read_len, size_t k, const std::vector<bitnuc_pattern> &patterns) const {
        const size_t count = read_len ? reads.len / read_len : 0;
        ReadsBest b = reads_outputs(count);
        bitnuc_err e;
        if (bitnuc_reads_pattern_best(ctx_, reads.ptr, read_len, count, k, patterns.data(), patterns.size(), b.query.data(), b.pos.data(), b.dist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return b;
    }
    Result<ReadsBest> reads_pattern_best_packed(Words words, size_t read_len, size_t count, size_t k, const std::vector<bitnuc_pattern> &patterns) const {
        ReadsBest b = reads_outputs(count);
        bitnuc_err e;
        if (bitnuc_reads_pattern_best_packed(ctx_, words.ptr, read_len, count, k, patterns.data(), patterns.size(), b.query.data(), b.pos.data(), b.dist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return b;
    }
    Result<ReadsBest2> reads_pattern_best2(Bytes reads, size_t read_len, size_t k, const std::vector<bitnuc_pattern> &patterns) const {
        const size_t count = read_len ? reads.len / read_len : 0;
        ReadsBest2 b{reads_outputs(count), reads_outputs(count)};
        bitnuc_err e;
        if (bitnuc_reads_pattern_best2(ctx_, reads.ptr, read_len, count, k, patterns.data(), patterns.size(), b.best.query.data(), b.best.pos.data(), b.best.dist.data(),
                                       b.second.query.data(), b.second.pos.data(), b.second.dist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return b;
    }
    Result<ReadsBest2> reads_pattern_best2_packed(Words words, size_t read_len, size_t count, size_t k, const std::vector<bitnuc_pattern> &patterns) const {
        ReadsBest2 b{reads_outputs(count), reads_outputs(count)};
        bitnuc_err e;
        if (bitnuc_reads_pattern_best2_packed(ctx_, words.ptr, read_len, count, k, patterns.data(), patterns.size(), b.best.query.data(), b.best.pos.data(),
                                              b.best.dist.data(), b.second.query.data(), b.second.pos.data(), b.second.dist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return b;
    }
    Result<ReadsBest2> reads_pattern_anchored(Bytes reads, size_t read_len, size_t k, const std::vector<bitnuc_pattern> &patterns, size_t pos_lo = 0,
                                              size_t pos_hi = SIZE_MAX) const {
        const size_t count = read_len ? reads.len / read_len : 0;
        ReadsBest2 b{reads_outputs(count), reads_outputs(count)};
        bitnuc_err e;
        if (bitnuc_reads_pattern_anchored(ctx_, reads.ptr, read_len, count, k, pos_lo, pos_hi, patterns.data(), patterns.size(), b.best.query.data(), b.best.pos.data(),
                                          b.best.dist.data(), b.second.query.data(), b.second.pos.data(), b.second.dist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return b;
    }
    Result<ReadsBest2> reads_pattern_anchored_packed(Words words, size_t read_len, size_t count, size_t k, const std::vector<bitnuc_pattern> &patterns,
                                                     size_t pos_lo = 0, size_t pos_hi = SIZE_MAX) const {
        ReadsBest2 b{reads_outputs(count), reads_outputs(count)};
        bitnuc_err e;
        if (bitnuc_reads_pattern_anchored_packed(ctx_, words.ptr, read_len, count, k, pos_lo, pos_hi, patterns.data(), patterns.size(), b.best.query.data(),
                                                 b.best.pos.data(), b.best.dist.data(), b.second.query.data(), b.second.pos.data(), b.second.dist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return b;
    }
    // the indel-tolerant anchored match (bitnuc_reads_edist_anchored*): the edit distance of each query to the best substring of the read's span
    // [pos_lo, min(pos_hi, read_len - k) + k); ReadsBest::pos holds the END of the alignment, an offset in the read one past its last aligned base
    Result<ReadsBest2> reads_edist_anchored(Bytes reads, size_t read_len, size_t k, const std::vector<uint64_t> &queries, size_t pos_lo = 0,
                                            size_t pos_hi = SIZE_MAX) const {
        const size_t count = read_len ? reads.len / read_len : 0;
        ReadsBest2 b{reads_outputs(count), reads_outputs(count)};
        bitnuc_err e;
        if (bitnuc_reads_edist_anchored(ctx_, reads.ptr, read_len, count, k, pos_lo, pos_hi, queries.data(), queries.size(), b.best.query.data(), b.best.pos.data(),
                                        b.best.dist.data(), b.second.query.data(), b.second.pos.data(), b.second.dist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return b;
    }
    Result<ReadsBest2> reads_edist_anchored_packed(Words words, size_t read_len, size_t count, size_t k, const std::vector<uint64_t> &queries, size_t pos_lo = 0,
                                                   size_t pos_hi = SIZE_MAX) const {
        ReadsBest2 b{reads_outputs(count), reads_outputs(count)};
        bitnuc_err e;
        if (bitnuc_reads_edist_anchored_packed(ctx_, words.ptr, read_len, count, k, pos_lo, pos_hi, queries.data(), queries.size(), b.best.query.data(),
                                               b.best.pos.data(), b.best.dist.data(), b.second.query.data(), b.second.pos.data(), b.second.dist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return b;
    }
    Result<ReadsBest2> reads_pattern_edist_anchored(Bytes reads, size_t read_len, size_t k, const std::vector<bitnuc_pattern> &patterns, size_t pos_lo = 0,
                                                    size_t pos_hi = SIZE_MAX) const {
        const size_t count = read_len ? reads.len / read_len : 0;
        ReadsBest2 b{reads_outputs(count), reads_outputs(count)};
        bitnuc_err e;
        if (bitnuc_reads_pattern_edist_anchored(ctx_, reads.ptr, read_len, count, k, pos_lo, pos_hi, patterns.data(), patterns.size(), b.best.query.data(),
                                                b.best.pos.data(), b.best.dist.data(), b.second.query.data(), b.second.pos.data(), b.second.dist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return b;
    }
    Result<ReadsBest2> reads_pattern_edist_anchored_packed(Words words, size_t read_len, size_t count, size_t k, const std::vector<bitnuc_pattern> &patterns,
                                                           size_t pos_lo = 0, size_t pos_hi = SIZE_MAX) const {
        ReadsBest2 b{reads_outputs(count), reads_outputs(count)};
        bitnuc_err e;
        if (bitnuc_reads_pattern_edist_anchored_packed(ctx_, words.ptr, read_len, count, k, pos_lo, pos_hi, patterns.data(), patterns.size(), b.best.query.data(),
                                                       b.best.pos.data(), b.best.dist.data(), b.second.query.data(), b.second.pos.data(), b.second.dist.data(), &e) !=
            BITNUC_OK)
            return NucleotideError::from_c(e);
        return b;
    }
    Result<ReadsBest> reads_pattern_best_batch(Bytes seq, const std::vector<uint64_t> &offsets, size_t k, const std::vector<bitnuc_pattern> &patterns) const {
        const size_t count = offsets.empty() ? 0 : offsets.size() - 1;
        if (count && seq.len < offsets.back()) return NucleotideError::invalid_length(seq.len);
        ReadsBest b = reads_outputs(count);
        bitnuc_err e;
        if (bitnuc_reads_pattern_best_batch(ctx_, seq.ptr, offsets.data(), count, k, patterns.data(), patterns.size(), b.query.data(), b.pos.data(), b.dist.data(), &e) !=
            BITNUC_OK)
            return NucleotideError::from_c(e);
        return b;
    }
    Result<ReadsBest> reads_pattern_best_batch_packed(Words words, const std::vector<uint64_t> &word_offsets, const std::vector<uint64_t> &offsets, size_t k,
                                                      const std::vector<bitnuc_pattern> &patterns) const {
        const size_t count = offsets.empty() ? 0 : offsets.size() - 1;
        if (word_offsets.size() != offsets.size()) return NucleotideError::unsupported();
        if (count && words.len < word_offsets.back()) return NucleotideError::invalid_length(words.len);
        ReadsBest b = reads_outputs(count);
        bitnuc_err e;
        if (bitnuc_reads_pattern_best_batch_packed(ctx_, words.ptr, word_offsets.data(), offsets.data(), count, k, patterns.data(), patterns.size(), b.query.data(),
                                                   b.pos.data(), b.dist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return b;
    }
    Result<ReadsBest2> reads_pattern_anchored_batch(Bytes seq, const std::vector<uint64_t> &offsets, size_t k, const std::vector<bitnuc_pattern> &patterns,
                                                    size_t pos_lo = 0, size_t pos_hi = 0, int anchor = BITNUC_ANCHOR_START) const {
        const size_t count = offsets.empty() ? 0 : offsets.size() - 1;
        if (count && seq.len < offsets.back()) return NucleotideError::invalid_length(seq.len);
        ReadsBest2 b{reads_outputs(count), reads_outputs(count)};
        bitnuc_err e;
        if (bitnuc_reads_pattern_anchored_batch(ctx_, seq.ptr, offsets.data(), count, k, anchor, pos_lo, pos_hi, patterns.data(), patterns.size(), b.best.query.data(),
                                                b.best.pos.data(), b.best.dist.data(), b.second.query.data(), b.second.pos.data(), b.second.dist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return b;
    }
    Result<ReadsBest2> reads_pattern_anchored_batch_packed(Words words, const std::vector<uint64_t> &word_offsets, const std::vector<uint64_t> &offsets, size_t k,
                                                           const std::vector<bitnuc_pattern> &patterns, size_t pos_lo = 0, size_t pos_hi = 0,
                                                           int anchor = BITNUC_ANCHOR_START) const {
        const size_t count = offsets.empty() ? 0 : offsets.size() - 1;
        if (word_offsets.size() != offsets.size()) return NucleotideError::unsupported();
        if (count && words.len < word_offsets.back()) return NucleotideError::invalid_length(words.len);
        ReadsBest2 b{reads_outputs(count), reads_outputs(count)};
        bitnuc_err e;
        if (bitnuc_reads_pattern_anchored_batch_packed(ctx_, words.ptr, word_offsets.data(), offsets.data(), count, k, anchor, pos_lo, pos_hi, patterns.data(),
                                                       patterns.size(), b.best.query.data(), b.best.pos.data(), b.best.dist.data(), b.second.query.data(),
                                                       b.second.pos.data(), b.second.dist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return b;
    }
    // the indel-tolerant anchored match of a ragged batch (bitnuc_reads_edist_anchored_batch*): reads_hdist_anchored_batch's arguments and window rule, the
    // edit distance of each query to the best substring of each read's own span; `pos` of the result holds the END, counted from the read's start
    Result<ReadsBest2> reads_edist_anchored_batch(Bytes seq, const std::vector<uint64_t> &offsets, size_t k, const std::vector<uint64_t> &queries,
                                                    size_t pos_lo = 0, size_t pos_hi = 0, int anchor = BITNUC_ANCHOR_START) const {
        const size_t count = offsets.empty() ? 0 : offsets.size() - 1;
        if (count && seq.len < offsets.back()) return NucleotideError::invalid_length(seq.len);
        ReadsBest2 b{reads_outputs(count), reads_outputs(count)};
        bitnuc_err e;
        if (bitnuc_reads_edist_anchored_batch(ctx_, seq.ptr, offsets.data(), count, k, anchor, pos_lo, pos_hi, queries.data(), queries.size(), b.best.query.data(),
                                                b.best.pos.data(), b.best.dist.data(), b.second.query.data(), b.second.pos.data(), b.second.dist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return b;
    }
    Result<ReadsBest2> reads_edist_anchored_batch_packed(Words words, const std::vector<uint64_t> &word_offsets, const std::vector<uint64_t> &offsets, size_t k,
                                                           const std::vector<uint64_t> &queries, size_t pos_lo = 0, size_t pos_hi = 0,
                                                           int anchor = BITNUC_ANCHOR_START) const {
        const size_t count = offsets.empty() ? 0 : offsets.size() - 1;
        if (word_offsets.size() != offsets.size()) return NucleotideError::unsupported();
        if (count && words.len < word_offsets.back()) return NucleotideError::invalid_length(words.len);
        ReadsBest2 b{reads_outputs(count), reads_outputs(count)};
        bitnuc_err e;
        if (bitnuc_reads_edist_anchored_batch_packed(ctx_, words.ptr, word_offsets.data(), offsets.data(), count, k, anchor, pos_lo, pos_hi, queries.data(),
                                                       queries.size(), b.best.query.data(), b.best.pos.data(), b.best.dist.data(), b.second.query.data(),
                                                       b.second.pos.data(), b.second.dist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return b;
    }
    Result<ReadsBest2> reads_pattern_edist_anchored_batch(Bytes seq, const std::vector<uint64_t> &offsets, size_t k, const std::vector<bitnuc_pattern> &patterns,
                                                    size_t pos_lo = 0, size_t pos_hi = 0, int anchor = BITNUC_ANCHOR_START) const {
        const size_t count = offsets.empty() ? 0 : offsets.size() - 1;
        if (count && seq.len < offsets.back()) return NucleotideError::invalid_length(seq.len);
        ReadsBest2 b{reads_outputs(count), reads_outputs(count)};
        bitnuc_err e;
        if (bitnuc_reads_pattern_edist_anchored_batch(ctx_, seq.ptr, offsets.data(), count, k, anchor, pos_lo, pos_hi, patterns.data(), patterns.size(), b.best.query.data(),
                                                b.best.pos.data(), b.best.dist.data(), b.second.query.data(), b.second.pos.data(), b.second.dist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return b;
    }
    Result<ReadsBest2> reads_pattern_edist_anchored_batch_packed(Words words, const std::vector<uint64_t> &word_offsets, const std::vector<uint64_t> &offsets, size_t k,
                                                           const std::vector<bitnuc_pattern> &patterns, size_t pos_lo = 0, size_t pos_hi = 0,
                                                           int anchor = BITNUC_ANCHOR_START) const {
        const size_t count = offsets.empty() ? 0 : offsets.size() - 1;
        if (word_offsets.size() != offsets.size()) return NucleotideError::unsupported();
        if (count && words.len < word_offsets.back()) return NucleotideError::invalid_length(words.len);
        ReadsBest2 b{reads_outputs(count), reads_outputs(count)};
        bitnuc_err e;
        if (bitnuc_reads_pattern_edist_anchored_batch_packed(ctx_, words.ptr, word_offsets.data(), offsets.data(), count, k, anchor, pos_lo, pos_hi, patterns.data(),
                                                       patterns.size(), b.best.query.data(), b.best.pos.data(), b.best.dist.data(), b.second.query.data(),
                                                       b.second.pos.data(), b.second.dist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return b;
    }
    // the indel-tolerant best match over the WHOLE read (bitnuc_reads_edist_best*, _best_batch*): the edit distance of each query to the best substring of the
    // read, of any length up to BITNUC_EDIST_MAX_READ bases; ReadsBest::pos holds the END of the alignment, counted from the read's start, one past its last
    // aligned base; a read shorter than k gets the fill
    Result<ReadsBest2> reads_edist_best(Bytes reads, size_t read_len, size_t k, const std::vector<uint64_t> &queries) const {
        const size_t count = read_len ? reads.len / read_len : 0;
        ReadsBest2 b{reads_outputs(count), reads_outputs(count)};
        bitnuc_err e;
        if (bitnuc_reads_edist_best(ctx_, reads.ptr, read_len, count, k, queries.data(), queries.size(), b.best.query.data(), b.best.pos.data(), b.best.dist.data(),
            b.second.query.data(), b.second.pos.data(), b.second.dist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return b;
    }
    Result<ReadsBest2> reads_edist_best_packed(Words words, size_t read_len, size_t count, size_t k, const std::vector<uint64_t> &queries) const {
        ReadsBest2 b{reads_outputs(count), reads_outputs(count)};
        bitnuc_err e;
        if (bitnuc_reads_edist_best_packed(ctx_, words.ptr, read_len, count, k, queries.data(), queries.size(), b.best.query.data(), b.best.pos.data(), b.best.dist.data(),
            b.second.query.data(), b.second.pos.data(), b.second.dist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return b;
    }
    Result<ReadsBest2> reads_pattern_edist_best(Bytes reads, size_t read_len, size_t k, const std::vector<bitnuc_pattern> &patterns) const {
        const size_t count = read_len ? reads.len / read_len : 0;
        ReadsBest2 b{reads_outputs(count), reads_outputs(count)};
        bitnuc_err e;
        if (bitnuc_reads_pattern_edist_best(ctx_, reads.ptr, read_len, count, k, patterns.data(), patterns.size(), b.best.query.data(), b.best.pos.data(), b.best.dist.data(),
            b.second.query.data(), b.second.pos.data(), b.second.dist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return b;
    }
    Result<ReadsBest2> reads_pattern_edist_best_packed(Words words, size_t read_len, size_t count, size_t k, const std::vector<bitnuc_pattern> &patterns) const {
        ReadsBest2 b{reads_outputs(count), reads_outputs(count)};
        bitnuc_err e;
        if (bitnuc_reads_pattern_edist_best_packed(ctx_, words.ptr, read_len, count, k, patterns.data(), patterns.size(), b.best.query.data(), b.best.pos.data(), b.best.dist.data(),
            b.second.query.data(), b.second.pos.data(), b.second.dist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return b;
    }
    Result<ReadsBest2> reads_edist_best_batch(Bytes seq, const std::vector<uint64_t> &offsets, size_t k, const std::vector<uint64_t> &queries) const {
        const size_t count = offsets.empty() ? 0 : offsets.size() - 1;
        if (count && seq.len < offsets.back()) return NucleotideError::invalid_length(seq.len);
        ReadsBest2 b{reads_outputs(count), reads_outputs(count)};
        bitnuc_err e;
        if (bitnuc_reads_edist_best_batch(ctx_, seq.ptr, offsets.data(), count, k, queries.data(), queries.size(), b.best.query.data(), b.best.pos.data(), b.best.dist.data(),
            b.second.query.data(), b.second.pos.data(), b.second.dist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return b;
    }
    Result<ReadsBest2> reads_edist_best_batch_packed(Words words, const std::vector<uint64_t> &word_offsets, const std::vector<uint64_t> &offsets, size_t k, const std::vector<uint64_t> &queries) const {
        const size_t count = offsets.empty() ? 0 : offsets.size() - 1;
        if (word_offsets.size() != offsets.size()) return NucleotideError::unsupported();
        if (count && words.len < word_offsets.back()) return NucleotideError::invalid_length(words.len);
        ReadsBest2 b{reads_outputs(count), reads_outputs(count)};
        bitnuc_err e;
        if (bitnuc_reads_edist_best_batch_packed(ctx_, words.ptr, word_offsets.data(), offsets.data(), count, k, queries.data(), queries.size(), b.best.query.data(), b.best.pos.data(), b.best.dist.data(),
            b.second.query.data(), b.second.pos.data(), b.second.dist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return b;
    }
    Result<ReadsBest2> reads_pattern_edist_best_batch(Bytes seq, const std::vector<uint64_t> &offsets, size_t k, const std::vector<bitnuc_pattern> &patterns) const {
        const size_t count = offsets.empty() ? 0 : offsets.size() - 1;
        if (count && seq.len < offsets.back()) return NucleotideError::invalid_length(seq.len);
        ReadsBest2 b{reads_outputs(count), reads_outputs(count)};
        bitnuc_err e;
        if (bitnuc_reads_pattern_edist_best_batch(ctx_, seq.ptr, offsets.data(), count, k, patterns.data(), patterns.size(), b.best.query.data(), b.best.pos.data(), b.best.dist.data(),
            b.second.query.data(), b.second.pos.data(), b.second.dist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return b;
    }
    Result<ReadsBest2> reads_pattern_edist_best_batch_packed(Words words, const std::vector<uint64_t> &word_offsets, const std::vector<uint64_t> &offsets, size_t k, const std::vector<bitnuc_pattern> &patterns) const {
        const size_t count = offsets.empty() ? 0 : offsets.size() - 1;
        if (word_offsets.size() != offsets.size()) return NucleotideError::unsupported();
        if (count && words.len < word_offsets.back()) return NucleotideError::invalid_length(words.len);
        ReadsBest2 b{reads_outputs(count), reads_outputs(count)};
        bitnuc_err e;
        if (bitnuc_reads_pattern_edist_best_batch_packed(ctx_, words.ptr, word_offsets.data(), offsets.data(), count, k, patterns.data(), patterns.size(), b.best.query.data(), b.best.pos.data(), b.best.dist.data(),
            b.second.query.data(), b.second.pos.data(), b.second.dist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return b;
    }
    // the 3' adapter per read (bitnuc_reads_edist_adapter*, _adapter_batch*): of the adapters the one a read carries in full anywhere or as a prefix of
    // min_overlap <= overlap < k positions overhanging its end, within floor(overlap x err_num / err_den) edits; reads[0, cut) is what a trimmer keeps.  No
    // admissible candidate, or a read shorter than k: UINT32_MAX x 3, 0xFF x 2
    struct ReadsAdapter { std::vector<uint32_t> adapter, cut, end; std::vector<uint8_t> overlap, dist; };
    Result<ReadsAdapter> reads_edist_adapter(Bytes reads, size_t read_len, size_t k, const std::vector<uint64_t> &queries, size_t min_overlap = 3, size_t err_num = 1,
                                             size_t err_den = 10) const {
        return adapter_(read_len ? reads.len / read_len : 0, [&](size_t count, ReadsAdapter &a, bitnuc_err *e) {
            return bitnuc_reads_edist_adapter(ctx_, reads.ptr, read_len, count, k, queries.data(), queries.size(), min_overlap, err_num, err_den, a.adapter.data(),
                                              a.cut.data(), a.end.data(), a.overlap.data(), a.dist.data(), e);
        });
    }
    Result<ReadsAdapter> reads_edist_adapter_packed(Words words, size_t read_len, size_t count, size_t k, const std::vector<uint64_t> &queries, size_t min_overlap = 3,
                                                    size_t err_num = 1, size_t err_den = 10) const {
        return adapter_(count, [&](size_t count, ReadsAdapter &a, bitnuc_err *e) {
            return bitnuc_reads_edist_adapter_packed(ctx_, words.ptr, read_len, count, k, queries.data(), queries.size(), min_overlap, err_num, err_den, a.adapter.data(),
                                                     a.cut.data(), a.end.data(), a.overlap.data(), a.dist.data(), e);
        });
    }
    Result<ReadsAdapter> reads_pattern_edist_adapter(Bytes reads, size_t read_len, size_t k, const std::vector<bitnuc_pattern> &patterns, size_t min_overlap = 3,
                                                     size_t err_num = 1, size_t err_den = 10) const {
        return adapter_(read_len ? reads.len / read_len : 0, [&](size_t count, ReadsAdapter &a, bitnuc_err *e) {
            return bitnuc_reads_pattern_edist_adapter(ctx_, reads.ptr, read_len, count, k, patterns.data(), patterns.size(), min_overlap, err_num, err_den,
                                                      a.adapter.data(), a.cut.data(), a.end.data(), a.overlap.data(), a.dist.data(), e);
        });
    }
    Result<ReadsAdapter> reads_pattern_edist_adapter_packed(Words words, size_t read_len, size_t count, size_t k, const std::vector<bitnuc_pattern> &patterns,
                                                            size_t min_overlap = 3, size_t err_num = 1, size_t err_den = 10) const {
        return adapter_(count, [&](size_t count, ReadsAdapter &a, bitnuc_err *e) {
            return bitnuc_reads_pattern_edist_adapter_packed(ctx_, words.ptr, read_len, count, k, patterns.data(), patterns.size(), min_overlap, err_num, err_den,
                                                             a.adapter.data(), a.cut.data(), a.end.data(), a.overlap.data(), a.dist.data(), e);
        });
    }
    Result<ReadsAdapter> reads_edist_adapter_batch(Bytes seq, const std::vector<uint64_t> &offsets, size_t k, const std::vector<uint64_t> &queries,
                                                   size_t min_overlap = 3, size_t err_num = 1, size_t err_den = 10) const {
        const size_t n = offsets.empty() ? 0 : offsets.size() - 1;
        if (n && seq.len < offsets.back()) return NucleotideError::invalid_length(seq.len);
        return adapter_(n, [&](size_t count, ReadsAdapter &a, bitnuc_err *e) {
            return bitnuc_reads_edist_adapter_batch(ctx_, seq.ptr, offsets.data(), count, k, queries.data(), queries.size(), min_overlap, err_num, err_den,
                                                    a.adapter.data(), a.cut.data(), a.end.data(), a.overlap.data(), a.dist.data(), e);
        });
    }
    Result<ReadsAdapter> reads_edist_adapter_batch_packed(Words words, const std::vector<uint64_t> &word_offsets, const std::vector<uint64_t> &offsets, size_t k,
                                                          const std::vector<uint64_t> &queries, size_t min_overlap = 3, size_t err_num = 1, size_t err_den = 10) const {
        const size_t n = offsets.empty() ? 0 : offsets.size() - 1;
        if (word_offsets.size() != offsets.size()) return NucleotideError::unsupported();
        if (n && words.len < word_offsets.back()) return NucleotideError::invalid_length(words.len);
        return adapter_(n, [&](size_t count, ReadsAdapter &a, bitnuc_err *e) {
            return bitnuc_reads_edist_adapter_batch_packed(ctx_, words.ptr, word_offsets.data(), offsets.data(), count, k, queries.data(), queries.size(), min_overlap,
                                                           err_num, err_den, a.adapter.data(), a.cut.data(), a.end.data(), a.overlap.data(), a.dist.data(), e);
        });
    }
    Result<ReadsAdapter> reads_pattern_edist_adapter_batch(Bytes seq, const std::vector<uint64_t> &offsets, size_t k, const std::vector<bitnuc_pattern> &patterns,
                                                           size_t min_overlap = 3, size_t err_num = 1, size_t err_den = 10) const {
        const size_t n = offsets.empty() ? 0 : offsets.size() - 1;
        if (n && seq.len < offsets.back()) return NucleotideError::invalid_length(seq.len);
        return adapter_(n, [&](size_t count, ReadsAdapter &a, bitnuc_err *e) {
            return bitnuc_reads_pattern_edist_adapter_batch(ctx_, seq.ptr, offsets.data(), count, k, patterns.data(), patterns.size(), min_overlap, err_num, err_den,
                                                            a.adapter.data(), a.cut.data(), a.end.data(), a.overlap.data(), a.dist.data(), e);
        });
    }
    Result<ReadsAdapter> reads_pattern_edist_adapter_batch_packed(Words words, const std::vector<uint64_t> &word_offsets, const std::vector<uint64_t> &offsets, size_t k,
                                                                  const std::vector<bitnuc_pattern> &patterns, size_t min_overlap = 3, size_t err_num = 1,
                                                                  size_t err_den = 10) const {
        const size_t n = offsets.empty() ? 0 : offsets.size() - 1;
        if (word_offsets.size() != offsets.size()) return NucleotideError::unsupported();
        if (n && words.len < word_offsets.back()) return NucleotideError::invalid_length(words.len);
        return adapter_(n, [&](size_t count, ReadsAdapter &a, bitnuc_err *e) {
            return bitnuc_reads_pattern_edist_adapter_batch_packed(ctx_, words.ptr, word_offsets.data(), offsets.data(), count, k, patterns.data(), patterns.size(),
                                                                   min_overlap, err_num, err_den, a.adapter.data(), a.cut.data(), a.end.data(), a.overlap.data(),
                                                                   a.dist.data(), e);
        });
    }
    Result<std::vector<uint64_t>> kmer_hdist_hits_packed(Words words, size_t n, size_t k, uint64_t query, unsigned tau, std::vector<uint8_t> *hit_dist = nullptr) const {
        uint64_t total = 0;
        bitnuc_err e;
        if (bitnuc_kmer_hdist_hits_packed(ctx_, words.ptr, words.len, n, k, query, tau, nullptr, nullptr, 0, &total, &e) != BITNUC_OK) return NucleotideError::from_c(e);
        std::vector<uint64_t> pos((size_t)total);
        if (hit_dist) hit_dist->assign((size_t)total, 0);
        if (total && bitnuc_kmer_hdist_hits_packed(ctx_, words.ptr, words.len, n, k, query, tau, pos.data(), hit_dist ? hit_dist->data() : nullptr, pos.size(), &total, &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return pos;
    }

    // ---- pattern queries: a set of bases per position (bitnuc_pattern), pdist(j) = #{ i < k : ref[j+i] not in S_i }.  The converters need no context.
    static Result<bitnuc_pattern> pattern_from_iupac(Bytes letters) { // ACGTU RYSWKM BDHV N, either case; at most 32
        bitnuc_pattern p;
        bitnuc_err e;
        if (bitnuc_pattern_from_iupac(letters.ptr, letters.len, &p, &e) != BITNUC_OK) return NucleotideError::from_c(e);
        return p;
    }
    static Result<bitnuc_pattern> pattern_from_2bit(uint64_t query, size_t k) { // the singletons of an exact query: the exact entry points' results
        bitnuc_pattern p;
        bitnuc_err e;
        if (bitnuc_pattern_from_2bit(query, k, &p, &e) != BITNUC_OK) return NucleotideError::from_c(e);
        return p;
    }
    // counts[q] = windows with pdist <= taus[q] under patterns[q], every pattern in one pass (taus.size() == patterns.size())
    Result<std::vector<uint64_t>> kmer_pattern_count_multi(Bytes ref, size_t k, const std::vector<bitnuc_pattern> &patterns, const std::vector<uint32_t> &taus) const {
        if (taus.size() != patterns.size()) return NucleotideError::unsupported();
        std::vector<uint64_t> counts(patterns.size());
        bitnuc_err e;
        if (bitnuc_kmer_pattern_count_multi(ctx_, ref.ptr, ref.len, k, patterns.data(), taus.data(), patterns.size(), counts.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return counts;
    }
    Result<std::vector<uint64_t>> kmer_pattern_count_multi_packed(Words words, size_t n, size_t k, const std::vector<bitnuc_pattern> &patterns,
                                                                  const std::vector<uint32_t> &taus) const {
        if (taus.size() != patterns.size()) return NucleotideError::unsupported();
        std::vector<uint64_t> counts(patterns.size());
        bitnuc_err e;
        if (bitnuc_kmer_pattern_count_multi_packed(ctx_, words.ptr, words.len, n, k, patterns.data(), taus.data(), patterns.size(), counts.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return counts;
    }
    // (pos[q], dist[q]) = the leftmost window with the smallest pdist under patterns[q] and that pdist (no windows: UINT64_MAX / 0xFF)
    Result<std::pair<std::vector<uint64_t>, std::vector<uint8_t>>> kmer_pattern_best(Bytes ref, size_t k, const std::vector<bitnuc_pattern> &patterns) const {
        std::vector<uint64_t> pos(patterns.size());
        std::vector<uint8_t> dist(patterns.size());
        bitnuc_err e;
        if (bitnuc_kmer_pattern_best(ctx_, ref.ptr, ref.len, k, patterns.data(), patterns.size(), pos.data(), dist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return std::make_pair(std::move(pos), std::move(dist));
    }
    Result<std::pair<std::vector<uint64_t>, std::vector<uint8_t>>> kmer_pattern_best_packed(Words words, size_t n, size_t k,
                                                                                            const std::vector<bitnuc_pattern> &patterns) const {
        std::vector<uint64_t> pos(patterns.size());
        std::vector<uint8_t> dist(patterns.size());
        bitnuc_err e;
        if (bitnuc_kmer_pattern_best_packed(ctx_, words.ptr, words.len, n, k, patterns.data(), patterns.size(), pos.data(), dist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return std::make_pair(std::move(pos), std::move(dist));
    }
    // the indel-tolerant search along a reference (bitnuc_kmer_edist_*): E(j) = the edit distance of a query to the best substring of the reference
    // that ends at base j.  _best: (end[q], dist[q]) = the smallest j with the smallest E_q(j) and that distance, end one past the last aligned base
    // (k == 0 or n < k: UINT64_MAX / 0xFF); _count_multi: counts[q] = the ends j with E_q(j) <= taus[q] (taus.size() == queries.size())
    using EndDist = std::pair<std::vector<uint64_t>, std::vector<uint8_t>>;
    Result<EndDist> kmer_edist_best(Bytes ref, size_t k, const std::vector<uint64_t> &queries) const {
        return edist_best_(queries.size(), [&](uint64_t *end, uint8_t *dist, bitnuc_err *e) {
            return bitnuc_kmer_edist_best(ctx_, ref.ptr, ref.len, k, queries.data(), queries.size(), end, dist, e);
        });
    }
    Result<EndDist> kmer_edist_best_packed(Words words, size_t n, size_t k, const std::vector<uint64_t> &queries) const {
        return edist_best_(queries.size(), [&](uint64_t *end, uint8_t *dist, bitnuc_err *e) {
            return bitnuc_kmer_edist_best_packed(ctx_, words.ptr, words.len, n, k, queries.data(), queries.size(), end, dist, e);
        });
    }
    Result<EndDist> kmer_pattern_edist_best(Bytes ref, size_t k, const std::vector<bitnuc_pattern> &patterns) const {
        return edist_best_(patterns.size(), [&](uint64_t *end, uint8_t *dist, bitnuc_err *e) {
            return bitnuc_kmer_pattern_edist_best(ctx_, ref.ptr, ref.len, k, patterns.data(), patterns.size(), end, dist, e);
        });
    }
    Result<EndDist> kmer_pattern_edist_best_packed(Words words, size_t n, size_t k, const std::vector<bitnuc_pattern> &patterns) const {
        return edist_best_(patterns.size(), [&](uint64_t *end, uint8_t *dist, bitnuc_err *e) {
            return bitnuc_kmer_pattern_edist_best_packed(ctx_, words.ptr, words.len, n, k, patterns.data(), patterns.size(), end, dist, e);
        });
    }
    Result<std::vector<uint64_t>> kmer_edist_count_multi(Bytes ref, size_t k, const std::vector<uint64_t> &queries, const std::vector<uint32_t> &taus) const {
        return edist_count_(queries.size(), taus.size(), [&](uint64_t *counts, bitnuc_err *e) {
            return bitnuc_kmer_edist_count_multi(ctx_, ref.ptr, ref.len, k, queries.data(), taus.data(), queries.size(), counts, e);
        });
    }
    Result<std::vector<uint64_t>> kmer_edist_count_multi_packed(Words words, size_t n, size_t k, const std::vector<uint64_t> &queries,
                                                                const std::vector<uint32_t> &taus) const {
        return edist_count_(queries.size(), taus.size(), [&](uint64_t *counts, bitnuc_err *e) {
            return bitnuc_kmer_edist_count_multi_packed(ctx_, words.ptr, words.len, n, k, queries.data(), taus.data(), queries.size(), counts, e);
        });
    }
    Result<std::vector<uint64_t>> kmer_pattern_edist_count_multi(Bytes ref, size_t k, const std::vector<bitnuc_pattern> &patterns,
                                                                 const std::vector<uint32_t> &taus) const {
        return edist_count_(patterns.size(), taus.size(), [&](uint64_t *counts, bitnuc_err *e) {
            return bitnuc_kmer_pattern_edist_count_multi(ctx_, ref.ptr, ref.len, k, patterns.data(), taus.data(), patterns.size(), counts, e);
        });
    }
    Result<std::vector<uint64_t>> kmer_pattern_edist_count_multi_packed(Words words, size_t n, size_t k, const std::vector<bitnuc_pattern> &patterns,
                                                                        const std::vector<uint32_t> &taus) const {
        return edist_count_(patterns.size(), taus.size(), [&](uint64_t *counts, bitnuc_err *e) {
            return bitnuc_kmer_pattern_edist_count_multi_packed(ctx_, words.ptr, words.len, n, k, patterns.data(), taus.data(), patterns.size(), counts, e);
        });
    }
    // the ends j (ascending, one past the last aligned base) with E(j) <= tau, sized by a first call with cap 0; hit_dist, when given, gets E(end[r]).
    // Neighbouring ends of a good match are hits too: the list is not collapsed to local minima
    Result<std::vector<uint64_t>> kmer_edist_hits(Bytes ref, size_t k, uint64_t query, unsigned tau, std::vector<uint8_t> *hit_dist = nullptr) const {
        return edist_hits_(hit_dist, [&](uint64_t *end, uint8_t *hd, size_t cap, uint64_t *total, bitnuc_err *e) {
            return bitnuc_kmer_edist_hits(ctx_, ref.ptr, ref.len, k, query, tau, end, hd, cap, total, e);
        });
    }
    Result<std::vector<uint64_t>> kmer_edist_hits_packed(Words words, size_t n, size_t k, uint64_t query, unsigned tau, std::vector<uint8_t> *hit_dist = nullptr) const {
        return edist_hits_(hit_dist, [&](uint64_t *end, uint8_t *hd, size_t cap, uint64_t *total, bitnuc_err *e) {
            return bitnuc_kmer_edist_hits_packed(ctx_, words.ptr, words.len, n, k, query, tau, end, hd, cap, total, e);
        });
    }
    Result<std::vector<uint64_t>> kmer_pattern_edist_hits(Bytes ref, size_t k, const bitnuc_pattern &pattern, unsigned tau, std::vector<uint8_t> *hit_dist = nullptr) const {
        return edist_hits_(hit_dist, [&](uint64_t *end, uint8_t *hd, size_t cap, uint64_t *total, bitnuc_err *e) {
            return bitnuc_kmer_pattern_edist_hits(ctx_, ref.ptr, ref.len, k, &pattern, tau, end, hd, cap, total, e);
        });
    }
    Result<std::vector<uint64_t>> kmer_pattern_edist_hits_packed(Words words, size_t n, size_t k, const bitnuc_pattern &pattern, unsigned tau, std::vector<uint8_t> *hit_dist = nullptr) const {
        return edist_hits_(hit_dist, [&](uint64_t *end, uint8_t *hd, size_t cap, uint64_t *total, bitnuc_err *e) {
            return bitnuc_kmer_pattern_edist_hits_packed(ctx_, words.ptr, words.len, n, k, &pattern, tau, end, hd, cap, total, e);
        });
    }
    // hist[q * n_bins + d] = the windows with pdist exactly d < n_bins under patterns[q]
    Result<std::vector<uint64_t>> kmer_pattern_hist(Bytes ref, size_t k, const std::vector<bitnuc_pattern> &patterns, size_t n_bins) const {
        std::vector<uint64_t> hist(patterns.size() * (n_bins < BITNUC_HIST_MAX_BINS ? n_bins : BITNUC_HIST_MAX_BINS));
        bitnuc_err e;
        if (bitnuc_kmer_pattern_hist(ctx_, ref.ptr, ref.len, k, patterns.data(), patterns.size(), n_bins, hist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return hist;
    }
    Result<std::vector<uint64_t>> kmer_pattern_hist_packed(Words words, size_t n, size_t k, const std::vector<bitnuc_pattern> &patterns, size_t n_bins) const {
        std::vector<uint64_t> hist(patterns.size() * (n_bins < BITNUC_HIST_MAX_BINS ? n_bins : BITNUC_HIST_MAX_BINS));
        bitnuc_err e;
        if (bitnuc_kmer_pattern_hist_packed(ctx_, words.ptr, words.len, n, k, patterns.data(), patterns.size(), n_bins, hist.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return hist;
    }
    // the positions (ascending) of the windows with pdist <= tau, sized by a first call with cap 0; hit_dist, when given, gets their distances
    Result<std::vector<uint64_t>> kmer_pattern_hits(Bytes ref, size_t k, const bitnuc_pattern &pattern, unsigned tau, std::vector<uint8_t> *hit_dist = nullptr) const {
        uint64_t total = 0;
        bitnuc_err e;
        if (bitnuc_kmer_pattern_hits(ctx_, ref.ptr, ref.len, k, &pattern, tau, nullptr, nullptr, 0, &total, &e) != BITNUC_OK) return NucleotideError::from_c(e);
        std::vector<uint64_t> pos((size_t)total);
        if (hit_dist) hit_dist->assign((size_t)total, 0);
        if (total && bitnuc_kmer_pattern_hits(ctx_, ref.ptr, ref.len, k, &pattern, tau, pos.data(), hit_dist ? hit_dist->data() : nullptr, pos.size(), &total, &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return pos;
    }
    Result<std::vector<uint64_t>> kmer_pattern_hits_packed(Words words, size_t n, size_t k, const bitnuc_pattern &pattern, unsigned tau,
                                                           std::vector<uint8_t> *hit_dist = nullptr) const {
        uint64_t total = 0;
        bitnuc_err e;
        if (bitnuc_kmer_pattern_hits_packed(ctx_, words.ptr, words.len, n, k, &pattern, tau, nullptr, nullptr, 0, &total, &e) != BITNUC_OK) return NucleotideError::from_c(e);
        std::vector<uint64_t> pos((size_t)total);
        if (hit_dist) hit_dist->assign((size_t)total, 0);
        if (total && bitnuc_kmer_pattern_hits_packed(ctx_, words.ptr, words.len, n, k, &pattern, tau, pos.data(), hit_dist ? hit_dist->data() : nullptr, pos.size(), &total,
                                                     &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return pos;
    }

    // Ragged batch: `for s in seqs { encode(s, &mut ebuf)? }` in one launch.  Sequence i =
    // seq[offsets[i] .. offsets[i+1]); returns the concatenated words and fills word_offsets
    // (count+1 entries, word_offsets[i] = first word of sequence i).
    Result<std::vector<uint64_t>> encode_batch(Bytes seq, const std::vector<uint64_t> &offsets,
                                               std::vector<uint64_t> &word_offsets) const {
        const size_t count = offsets.empty() ? 0 : offsets.size() - 1;
        word_offsets.assign(count + 1, 0);
        std::vector<uint64_t> out(count ? (size_t)((offsets[count] - offsets[0]) / 32 + count) : 0);
        size_t nw = 0;
        bitnuc_err e;
        if (count && seq.len < offsets[count]) return NucleotideError::unsupported(); // offsets point past the slice
        int st = bitnuc_encode_batch(ctx_, seq.ptr, offsets.data(), count, out.data(), out.size(), word_offsets.data(), &nw, &e);
        if (st != BITNUC_OK) return NucleotideError::from_c(e);
        out.resize(nw);
        return out;
    }
    // Fixed-length reads: `count` reads of read_len bases, read r at seq[r*stride ..]; returns
    // count*ceil(read_len/32) words, row r == encode_alloc(read r).
    Result<std::vector<uint64_t>> encode_fixed(Bytes seq, size_t read_len, size_t stride, size_t count) const {
        std::vector<uint64_t> out(count * ((read_len + 31) / 32));
        bitnuc_err e;
        if (count && (stride < read_len || (count - 1) * stride + read_len > seq.len)) return NucleotideError::unsupported();
        if (bitnuc_encode_fixed(ctx_, seq.ptr, read_len, stride, count, out.data(), &e) != BITNUC_OK) return NucleotideError::from_c(e);
        return out;
    }
    // Inverse: sequence i's bases are written at out[offsets[i] .. offsets[i+1]).
    Result<std::vector<uint8_t>> decode_batch(Words words, const std::vector<uint64_t> &word_offsets,
                                              const std::vector<uint64_t> &offsets) const {
        const size_t count = offsets.empty() ? 0 : offsets.size() - 1;
        std::vector<uint8_t> out(count ? (size_t)offsets[count] : 0);
        bitnuc_err e;
        if (word_offsets.size() != offsets.size() || (count && words.len < word_offsets[count])) return NucleotideError::unsupported();
        if (bitnuc_decode_batch(ctx_, words.ptr, word_offsets.data(), offsets.data(), count, out.data(), &e) != BITNUC_OK)
            return NucleotideError::from_c(e);
        return out;
    }

  private:
    bitnuc_ctx *ctx_ = nullptr;
    // the five output vectors of the reads_*edist_adapter* methods around one C call
    template <class Call> static Result<ReadsAdapter> adapter_(size_t count, Call call) {
        ReadsAdapter a{std::vector<uint32_t>(count), std::vector<uint32_t>(count), std::vector<uint32_t>(count), std::vector<uint8_t>(count), std::vector<uint8_t>(count)};
        bitnuc_err e;
        if (call(count, a, &e) != BITNUC_OK) return NucleotideError::from_c(e);
        return a;
    }
    // the output vectors of the kmer_*edist_* methods around one C call
    template <class Call> static Result<EndDist> edist_best_(size_t nq, Call call) {
        std::vector<uint64_t> end(nq);
        std::vector<uint8_t> dist(nq);
        bitnuc_err e;
        if (call(end.data(), dist.data(), &e) != BITNUC_OK) return NucleotideError::from_c(e);
        return std::make_pair(std::move(end), std::move(dist));
    }
    template <class Call> static Result<std::vector<uint64_t>> edist_count_(size_t nq, size_t ntaus, Call call) {
        if (ntaus != nq) return NucleotideError::unsupported();
        std::vector<uint64_t> counts(nq);
        bitnuc_err e;
        if (call(counts.data(), &e) != BITNUC_OK) return NucleotideError::from_c(e);
        return counts;
    }
    // a hit list around two C calls: the first with cap 0 sizes the vectors
    template <class Call> static Result<std::vector<uint64_t>> edist_hits_(std::vector<uint8_t> *hit_dist, Call call) {
        uint64_t total = 0;
        bitnuc_err e;
        if (call(nullptr, nullptr, 0, &total, &e) != BITNUC_OK) return NucleotideError::from_c(e);
        std::vector<uint64_t> end((size_t)total);
        if (hit_dist) hit_dist->assign((size_t)total, 0);
        if (total && call(end.data(), hit_dist ? hit_dist->data() : nullptr, end.size(), &total, &e) != BITNUC_OK) return NucleotideError::from_c(e);
        return end;
    }
};

// Free functions with the reference's names, on a per-thread default context (device 0).
inline Context &default_context() {
    thread_local Context ctx(0);
    return ctx;
}

// PackedSequence (src/sequence.rs:5-262) over GPU-encoded data, with the GCContent / BaseCount
// traits of src/utils/analysis.rs:3-39.  `new_` encodes on the GPU; slice / to_vec / get decode
// only the words the range touches, on the GPU; the traits count on the packed words.
class PackedSequence {
  public:
    static Result<PackedSequence> new_(Bytes seq) { // sequence.rs:40-52
        PackedSequence p;
        if (seq.len != 0) { // sequence.rs:42-44: skip encoding for empty sequences
            Result<void> r = default_context().encode(seq, p.data_);
            if (r.is_err()) return r.unwrap_err();
        }
        p.length_ = seq.len;
        return p;
    }
    size_t len() const { return length_; }
    bool is_empty() const { return length_ == 0; }
    const std::vector<uint64_t> &data() const { return data_; }
    Result<uint8_t> get(size_t index) const { // sequence.rs:116-135
        if (index >= length_) {
            NucleotideError e; e.kind = NucleotideError::IndexOutOfBounds; e.oob_index = index; e.length = length_;
            return e;
        }
        // the reference's shift + mask + match (sequence.rs:121-134): no call into the library
        return static_cast<uint8_t>("ACGT"[(data_[index / 32] >> (2 * (index % 32))) & 3]);
    }
    Result<std::vector<uint8_t>> slice(size_t start, size_t end) const { // sequence.rs:198-212
        if (start > end || end > length_) {
            NucleotideError e; e.kind = NucleotideError::InvalidRange; e.start = start; e.end = end; e.length = length_;
            return e;
        }
        std::vector<uint8_t> out;
        if (start == end) return out;
        const size_t w0 = start / 32, w1 = (end + 31) / 32;
        const size_t n = (length_ < w1 * 32 ? length_ : w1 * 32) - w0 * 32;
        std::vector<uint8_t> chunk;
        Result<void> r = default_context().decode(Words(data_.data() + w0, w1 - w0), n, chunk);
        if (r.is_err()) return r.unwrap_err();
        out.assign(chunk.begin() + (start - w0 * 32), chunk.begin() + (end - w0 * 32));
        return out;
    }
    Result<std::vector<uint8_t>> to_vec() const { return slice(0, length_); } // sequence.rs:260-262
    bool operator==(const PackedSequence &o) const { return length_ == o.length_ && data_ == o.data_; }
    bool operator!=(const PackedSequence &o) const { return !(*this == o); }
    // traits (analysis.rs)
    std::array<size_t, 4> base_counts() const {
        uint64_t c[4] = {0, 0, 0, 0};
        bitnuc_err e;
        if (bitnuc_base_counts(default_context().raw(), data_.data(), data_.size(), length_, c, &e) != BITNUC_OK)
            throw std::runtime_error("bitnuc: base_counts failed: " + NucleotideError::from_c(e).to_string());
        return {(size_t)c[0], (size_t)c[1], (size_t)c[2], (size_t)c[3]};
    }
    double gc_content() const { // analysis.rs:7-16
        if (length_ == 0) return 0.0;
        const auto c = base_counts();
        return ((double)(c[1] + c[2]) / (double)length_) * 100.0;
    }

  private:
    std::vector<uint64_t> data_;
    size_t length_ = 0;
};
inline Result<uint64_t> as_2bit(Bytes seq) { return default_context().as_2bit(seq); }
inline Result<void> from_2bit(uint64_t packed, size_t n, std::vector<uint8_t> &sequence) { return default_context().from_2bit(packed, n, sequence); }
inline Result<std::vector<uint8_t>> from_2bit_alloc(uint64_t packed, size_t n) { return default_context().from_2bit_alloc(packed, n); }
inline Result<void> encode(Bytes sequence, std::vector<uint64_t> &ebuf) { return default_context().encode(sequence, ebuf); }
inline Result<std::vector<uint64_t>> encode_alloc(Bytes sequence) { return default_context().encode_alloc(sequence); }
inline Result<void> decode(Words ebuf, size_t n_bases, std::vector<uint8_t> &dbuf) { return default_context().decode(ebuf, n_bases, dbuf); }
inline Result<uint32_t> hdist_scalar(uint64_t u, uint64_t v, size_t len) { return default_context().hdist_scalar(u, v, len); }
inline Result<uint32_t> hdist(Words a, Words b, size_t n_bases) { return default_context().hdist(a, b, n_bases); }
inline Result<void> split_packed(Words ebuf, size_t slen, size_t idx, std::vector<uint64_t> &lbuf, std::vector<uint64_t> &rbuf,
                                 bool canonical = false) {
    return default_context().split_packed(ebuf, slen, idx, lbuf, rbuf, canonical);
}

} // namespace bitnuc
