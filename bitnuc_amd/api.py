"""Host-side mirror of bitnuc's public API over the C ABI (Python flavour).

Same names, argument meaning and error behaviour as the reference's
`pub use` list (src/lib.rs:214-220):

    as_2bit, from_2bit, from_2bit_alloc, encode, encode_alloc, decode,
    hdist_scalar, hdist, NucleotideError

`Vec<u64>` / `Vec<u8>` arguments map to Python mutable sequences:
  * `encode(seq, ebuf)` CLEARS `ebuf` then fills it     (packing/avx.rs:132)
  * `decode(ebuf, n, dbuf)` / `from_2bit(p, n, seq)` APPEND (unpacking/avx.rs:122,140)
`ebuf` may be a list or array('Q'); `dbuf` a bytearray.

All bulk arithmetic runs on the GPU through libbitnuc_hip.so; single words and host-pointer calls
below the library's host cutoff are the library's own host code (include/bitnuc_hip.h, "Size dispatch").
The module-level single-word functions need no GPU context, like the reference's.
"""
import ctypes as C

import numpy as np

from . import _lib as L


class NucleotideError(Exception):
    """src/error.rs:3-18.  `kind` is the variant name; payload fields as in Rust."""

    def __init__(self, kind, **payload):
        self.kind = kind
        self.payload = payload
        for k, v in payload.items():
            setattr(self, k, v)
        super().__init__(self._display())

    def _display(self):  # Display impl, src/error.rs:20-45
        p = self.payload
        if self.kind == "InvalidBase":
            return f"Invalid nucleotide base: {p['byte']}"
        if self.kind == "SequenceTooLong":
            return f"Sequence length {p['len']} exceeds maximum"
        if self.kind == "InvalidLength":
            return f"Invalid length: {p['len']}"
        if self.kind == "IndexOutOfBounds":
            return f"Index {p['index']} out of bounds for sequence of length {p['length']}"
        if self.kind == "InvalidRange" and "start" in p:
            return f"Invalid range {p['start']}..{p['end']} for sequence of length {p['length']}"
        if self.kind == "Unsupported":
            return "Unsupported architecture"
        return self.kind

    def __eq__(self, other):  # derive(PartialEq, Eq), src/error.rs:3
        return isinstance(other, NucleotideError) and self.kind == other.kind and \
            self._cmp_payload() == other._cmp_payload()

    def _cmp_payload(self):  # InvalidBase carries an extra byte index that Rust's variant does not have
        return {k: v for k, v in self.payload.items() if not (self.kind == "InvalidBase" and k == "index")}

    __hash__ = Exception.__hash__


class BackendError(RuntimeError):
    """HIP runtime failure (no reference counterpart)."""


def _raise(err):
    st = err.status
    if st == L.INVALID_BASE:
        raise NucleotideError("InvalidBase", byte=int(err.byte), index=int(err.index))
    if st == L.SEQUENCE_TOO_LONG:
        raise NucleotideError("SequenceTooLong", len=int(err.value))
    if st == L.INVALID_LENGTH:
        raise NucleotideError("InvalidLength", len=int(err.value))
    if st == L.INDEX_OUT_OF_BOUNDS:
        raise NucleotideError("IndexOutOfBounds", index=int(err.index), length=int(err.value))
    if st == L.INVALID_RANGE:  # decreasing offsets in a ragged batch: err.value = the sequence whose end lies before its start
        raise NucleotideError("InvalidRange", index=int(err.value))
    if st == L.UNSUPPORTED:
        raise NucleotideError("Unsupported")
    if st == L.BACKEND_ERROR:
        raise BackendError(f"HIP error {err.backend_code} (is a gfx950 device visible? bitnuc_amd has no CPU fallback)")
    raise RuntimeError(f"bitnuc status {st}")


def _as_u8(buf):
    a = np.frombuffer(buf, dtype=np.uint8) if not isinstance(buf, np.ndarray) else buf
    if a.dtype != np.uint8:
        raise TypeError("sequence must be bytes-like / uint8")
    return np.ascontiguousarray(a)


def _as_u64(buf):
    if isinstance(buf, np.ndarray):
        if buf.dtype != np.uint64:
            raise TypeError("ebuf must be uint64")
        return np.ascontiguousarray(buf)
    return np.asarray(list(buf), dtype=np.uint64)


_SIZE_MAX = C.c_size_t(-1).value  # pos_hi of the anchored calls: to the end of the read


def _ptr(a):
    return C.c_void_p(a.ctypes.data if a.size else 0)


def _dev_ptr(x):
    """int device address, or anything with .data_ptr() (torch tensor)."""
    if x is None:
        return C.c_void_p(0)
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    return C.c_void_p(int(x))


class Context:
    """One device + stream + scratch (bitnuc_ctx).  Not thread-safe; make one per thread."""

    def __init__(self, device=0, stream=None, lib_path=None):
        self._lib = L.load(lib_path)
        self._h = C.c_void_p()
        err = L.BitnucErr()
        if stream is None:
            st = self._lib.bitnuc_ctx_create(device, C.byref(self._h), C.byref(err))
        else:
            st = self._lib.bitnuc_ctx_create_on_stream(device, C.c_void_p(int(stream)), C.byref(self._h), C.byref(err))
        if st != L.OK:
            self._h = C.c_void_p()
            _raise(err)
        self.device = device

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            if not getattr(self, "_borrowed", False):  # CommGroup.context(): the handle is the group's
                self._lib.bitnuc_ctx_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- tuning --------------------------------------------------------------------
    def set_variant(self, key, value, strict=False):
        """Previous value, or -2 when this build does not hold `value` (the product refuses every formulation but the shipped one).
        strict=True raises instead of returning -2 / leaving the knob where it was: an A/B that ignores a refusal times a kernel against
        itself, so tools/ and the variant tests use require_variant()."""
        prev = self._lib.bitnuc_ctx_set_variant(self._h, key.encode(), int(value))
        if strict and int(value) >= 0 and (prev == -2 or self.get(key) != int(value)):
            raise ValueError(f"bitnuc_ctx_set_variant({key!r}, {value}): refused by this build ({prev}); the knob stays at {self.get(key)}"
                             + ("" if self.get("sweep_build") == 1 else " -- alternative formulations live in the evidence build (build.ensure_built(sweep=True))"))
        return prev

    def require_variant(self, key, value):
        return self.set_variant(key, value, strict=True)

    def get(self, key):
        return self._lib.bitnuc_ctx_set_variant(self._h, key.encode(), -1)

    @property
    def stream(self):
        return self._lib.bitnuc_ctx_stream(self._h)

    def sync(self):
        err = L.BitnucErr()
        if self._lib.bitnuc_ctx_sync(self._h, C.byref(err)) != L.OK:
            _raise(err)

    # -- host-pointer API -------------------------------------------------------------
    def as_2bit(self, seq):
        s = _as_u8(seq)
        out = C.c_uint64(0)
        err = L.BitnucErr()
        if self._lib.bitnuc_as_2bit(self._h, _ptr(s), s.size, C.byref(out), C.byref(err)) != L.OK:
            _raise(err)
        return out.value

    def from_2bit_alloc(self, packed, expected_size):
        out = np.empty(min(int(expected_size), 32), dtype=np.uint8)
        err = L.BitnucErr()
        if self._lib.bitnuc_from_2bit(self._h, C.c_uint64(packed), int(expected_size), _ptr(out), C.byref(err)) != L.OK:
            _raise(err)
        return out.tobytes()

    def from_2bit(self, packed, expected_size, sequence):
        sequence += self.from_2bit_alloc(packed, expected_size)  # append (unpacking/avx.rs:59,73)

    def encode_array(self, sequence):
        """-> (words ndarray[uint64]) or raises; on InvalidBase the exception carries
        `.words`, the words the reference's Vec holds at that point."""
        s = _as_u8(sequence)
        if s.size == 0:
            # packing/avx.rs:138: `0..n_chunks - 1` underflows -> the reference panics
            raise RuntimeError("encode of an empty sequence panics in the reference (attempt to subtract with overflow)")
        out = np.empty((s.size + 31) // 32, dtype=np.uint64)
        nw = C.c_size_t(0)
        err = L.BitnucErr()
        st = self._lib.bitnuc_encode(self._h, _ptr(s), s.size, _ptr(out), C.byref(nw), C.byref(err))
        if st != L.OK:
            try:
                _raise(err)
            except NucleotideError as e:
                e.words = out[: nw.value].copy()
                raise
        return out

    def encode_into(self, sequence, out):
        """encode into a caller-owned uint64 array of >= ceil(len/32) words (no allocation: a pipeline reuses its buffers,
        and a freshly allocated output would be timed by its page faults, not by the codec).  -> number of words."""
        s = _as_u8(sequence)
        if not (isinstance(out, np.ndarray) and out.dtype == np.uint64 and out.flags.c_contiguous and out.size >= (s.size + 31) // 32):
            raise ValueError("out must be a contiguous uint64 array of at least ceil(len/32) words")
        nw = C.c_size_t(0)
        err = L.BitnucErr()
        if self._lib.bitnuc_encode(self._h, _ptr(s), s.size, _ptr(out), C.byref(nw), C.byref(err)) != L.OK:
            _raise(err)
        return nw.value

    def decode_into(self, ebuf, n_bases, out):
        """decode into a caller-owned uint8 array of >= n_bases bytes (see encode_into)."""
        e = _as_u64(ebuf)
        if not (isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.flags.c_contiguous and out.size >= n_bases):
            raise ValueError("out must be a contiguous uint8 array of at least n_bases bytes")
        err = L.BitnucErr()
        if self._lib.bitnuc_decode(self._h, _ptr(e), e.size, int(n_bases), _ptr(out), C.byref(err)) != L.OK:
            _raise(err)

    def encode(self, sequence, ebuf):
        del ebuf[:]  # ebuf.clear(), packing/avx.rs:132
        try:
            words = self.encode_array(sequence)
        except NucleotideError as e:
            ebuf.extend(int(w) for w in getattr(e, "words", ()))
            raise
        ebuf.extend(words.tolist())

    def encode_alloc(self, sequence):
        ebuf = []
        self.encode(sequence, ebuf)
        return ebuf

    def decode_array(self, ebuf, n_bases):
        e = _as_u64(ebuf)
        out = np.empty(int(n_bases), dtype=np.uint8)
        err = L.BitnucErr()
        if self._lib.bitnuc_decode(self._h, _ptr(e), e.size, int(n_bases), _ptr(out), C.byref(err)) != L.OK:
            _raise(err)
        return out

    def decode(self, ebuf, n_bases, dbuf):
        dbuf += self.decode_array(ebuf, n_bases).tobytes()  # append (unpacking/avx.rs:122,140)

    def hdist_scalar(self, u, v, length):
        out = C.c_uint32(0)
        err = L.BitnucErr()
        if self._lib.bitnuc_hdist_scalar(self._h, C.c_uint64(u), C.c_uint64(v), int(length), C.byref(out), C.byref(err)) != L.OK:
            _raise(err)
        return out.value

    def hdist(self, ebuf1, ebuf2, n_bases):
        a, b = _as_u64(ebuf1), _as_u64(ebuf2)
        out = C.c_uint32(0)
        err = L.BitnucErr()
        if self._lib.bitnuc_hdist(self._h, _ptr(a), a.size, _ptr(b), b.size, int(n_bases), C.byref(out), C.byref(err)) != L.OK:
            _raise(err)
        return out.value

    def as_2bit_batch(self, kmers, k, stride=None, count=None):
        s = _as_u8(kmers)
        stride = k if stride is None else stride
        if count is None:
            count = 0 if s.size < k else (s.size - k) // stride + 1
        elif count and 0 < k <= 32 and (count - 1) * stride + k > s.size:  # the C ABI trusts the caller's sizes
            raise ValueError("kmers holds fewer than (count-1)*stride + k bytes")
        out = np.empty(count, dtype=np.uint64)
        err = L.BitnucErr()
        if self._lib.bitnuc_as_2bit_batch(self._h, _ptr(s), int(k), int(stride), int(count), _ptr(out), C.byref(err)) != L.OK:
            _raise(err)
        return out

    def kmer_hdist_scan(self, ref, k, query):
        s = _as_u8(ref)
        nwin = s.size - k + 1 if (s.size >= k and k > 0) else 0
        out = np.empty(nwin, dtype=np.uint8)
        err = L.BitnucErr()
        if self._lib.bitnuc_kmer_hdist_scan(self._h, _ptr(s), s.size, int(k), C.c_uint64(query), _ptr(out), C.byref(err)) != L.OK:
            _raise(err)
        return out

    def kmer_hdist_scan_packed(self, words, n_bases, k, query):
        """kmer_hdist_scan of the packed sequence `words` holding `n_bases` bases, without decoding it -> np.uint8 distances."""
        w = _as_u64(words)
        n = int(n_bases)
        nwin = n - k + 1 if (n >= k and k > 0) else 0
        out = np.empty(nwin, dtype=np.uint8)
        err = L.BitnucErr()
        if self._lib.bitnuc_kmer_hdist_scan_packed(self._h, _ptr(w), w.size, n, int(k), C.c_uint64(query), _ptr(out), C.byref(err)) != L.OK:
            _raise(err)
        return out

    def kmer_hdist_count_packed(self, words, n_bases, k, query, tau):
        """Number of windows of the packed sequence `words` (`n_bases` bases) with Hamming distance <= tau to the query."""
        w = _as_u64(words)
        out = C.c_uint64(0)
        err = L.BitnucErr()
        if self._lib.bitnuc_kmer_hdist_count_packed(self._h, _ptr(w), w.size, int(n_bases), int(k), C.c_uint64(query), int(tau), C.byref(out), C.byref(err)) != L.OK:
            _raise(err)
        return out.value

    def _hits(self, fn, args, with_dist):
        """A hit-list call sized by a first call with cap 0 (its *n_hits), then filled."""
        err = L.BitnucErr()
        total = C.c_uint64(0)
        if fn(self._h, *args, None, None, 0, C.byref(total), C.byref(err)) != L.OK:
            _raise(err)
        pos = np.empty(total.value, dtype=np.uint64)
        dist = np.empty(total.value if with_dist else 0, dtype=np.uint8)
        if total.value and fn(self._h, *args, _ptr(pos), _ptr(dist) if with_dist else None, pos.size, C.byref(total), C.byref(err)) != L.OK:
            _raise(err)
        return (pos, dist) if with_dist else pos

    def kmer_hdist_hits(self, ref, k, query, tau, with_dist=False):
        """Positions (np.uint64, ascending) of the windows of `ref` with Hamming distance <= tau to the query; with_dist: (positions, np.uint8 distances)."""
        s = _as_u8(ref)
        return self._hits(self._lib.bitnuc_kmer_hdist_hits, (_ptr(s), s.size, int(k), C.c_uint64(query), int(tau)), with_dist)

    def kmer_hdist_hits_packed(self, words, n_bases, k, query, tau, with_dist=False):
        """kmer_hdist_hits of the packed sequence `words` holding `n_bases` bases, without decoding it."""
        w = _as_u64(words)
        return self._hits(self._lib.bitnuc_kmer_hdist_hits_packed, (_ptr(w), w.size, int(n_bases), int(k), C.c_uint64(query), int(tau)), with_dist)

    @staticmethod
    def _multi_args(queries, taus):
        """(queries as np.uint64, taus as np.uint32): taus may be a scalar, broadcast to every query"""
        q = np.ascontiguousarray(np.asarray(queries, dtype=np.uint64).reshape(-1))
        t = np.asarray(taus, dtype=np.int64)
        if t.ndim == 0:
            t = np.full(q.size, int(t), dtype=np.int64)
        t = t.reshape(-1)
        if t.size != q.size:
            raise ValueError("taus must be a scalar or hold one threshold per query")
        if t.size and (t.min() < 0 or t.max() > 2**32 - 1):
            raise ValueError("thresholds are uint32")
        return q, np.ascontiguousarray(t.astype(np.uint32))

    def kmer_hdist_count_multi(self, ref, k, queries, taus):
        """counts[q] = the number of windows of `ref` with Hamming distance <= taus[q] to queries[q], one pass for all queries -> np.uint64"""
        s = _as_u8(ref)
        q, t = self._multi_args(queries, taus)
        out = np.empty(q.size, dtype=np.uint64)
        err = L.BitnucErr()
        if self._lib.bitnuc_kmer_hdist_count_multi(self._h, _ptr(s), s.size, int(k), _ptr(q), _ptr(t), q.size, _ptr(out), C.byref(err)) != L.OK:
            _raise(err)
        return out

    def kmer_hdist_count_multi_packed(self, words, n_bases, k, queries, taus):
        """kmer_hdist_count_multi of the packed sequence `words` holding `n_bases` bases, without decoding it."""
        w = _as_u64(words)
        q, t = self._multi_args(queries, taus)
        out = np.empty(q.size, dtype=np.uint64)
        err = L.BitnucErr()
        if self._lib.bitnuc_kmer_hdist_count_multi_packed(self._h, _ptr(w), w.size, int(n_bases), int(k), _ptr(q), _ptr(t), q.size, _ptr(out),
                                                          C.byref(err)) != L.OK:
            _raise(err)
        return out

    def _best(self, fn, head, queries):
        q = np.ascontiguousarray(np.asarray(queries, dtype=np.uint64).reshape(-1))  # a scalar query: Q = 1
        pos = np.empty(q.size, dtype=np.uint64)
        dist = np.empty(q.size, dtype=np.uint8)
        err = L.BitnucErr()
        if fn(self._h, *head, _ptr(q), q.size, _ptr(pos), _ptr(dist), C.byref(err)) != L.OK:
            _raise(err)
        return pos, dist

    def kmer_hdist_best(self, ref, k, queries):
        """The best match per query in one pass: (pos, dist) with dist[q] = the smallest Hamming distance of a window of `ref` to queries[q] (np.uint8)
        and pos[q] = the leftmost window that attains it (np.uint64); without windows every pos is 2^64 - 1 and every dist 255."""
        s = _as_u8(ref)
        return self._best(self._lib.bitnuc_kmer_hdist_best, (_ptr(s), s.size, int(k)), queries)

    def kmer_hdist_best_packed(self, words, n_bases, k, queries):
        """kmer_hdist_best of the packed sequence `words` holding `n_bases` bases, without decoding it."""
        w = _as_u64(words)
        return self._best(self._lib.bitnuc_kmer_hdist_best_packed, (_ptr(w), w.size, int(n_bases), int(k)), queries)

    def _reads_queries(self, queries, pattern_k):
        """(array, Q) of a per-read call's queries: exact 2-bit words, or (pattern_k not None) patterns as _patterns takes them"""
        if pattern_k is not None:
            p = self._patterns(queries, pattern_k)
            return p, p.shape[0]
        q = np.ascontiguousarray(np.asarray(queries, dtype=np.uint64).reshape(-1))  # a scalar query: Q = 1
        return q, q.size

    def _reads_best(self, fn, head, count, queries, pattern_k=None):
        q, nq = self._reads_queries(queries, pattern_k)
        query = np.empty(count, dtype=np.uint32)
        pos = np.empty(count, dtype=np.uint32)
        dist = np.empty(count, dtype=np.uint8)
        err = L.BitnucErr()
        if fn(self._h, *head, _ptr(q), nq, _ptr(query), _ptr(pos), _ptr(dist), C.byref(err)) != L.OK:
            _raise(err)
        return query, pos, dist

    def reads_hdist_best(self, reads, read_len, k, queries, count=None):
        """The best match per read of back-to-back reads of `read_len` bases (`reads` holds a whole number of them): (query, pos, dist) with, per
        read, the smallest (distance, query index, offset) over all queries and the windows that lie wholly inside the read (np.uint32, np.uint32,
        np.uint8); a read without a window, or no queries: 2^32 - 1, 2^32 - 1, 255.  `count` defaults to len(reads) / read_len."""
        s = _as_u8(reads)
        read_len = int(read_len)
        if count is None:
            if read_len <= 0 or s.size % read_len:
                raise ValueError("reads must hold a whole number of reads of read_len bases")
            count = s.size // read_len
        count = int(count)
        if s.size < count * read_len:
            raise ValueError("reads must hold count reads of read_len bases")
        return self._reads_best(self._lib.bitnuc_reads_hdist_best, (_ptr(s), read_len, count, int(k)), count, queries)

    def reads_hdist_best_packed(self, words, read_len, count, k, queries):
        """reads_hdist_best of the packed words encode_fixed writes (ceil(read_len / 32) words per read), without decoding them."""
        w = _as_u64(words)
        if w.size < int(count) * ((int(read_len) + 31) // 32):
            raise ValueError("words must hold count reads of ceil(read_len / 32) words each")
        return self._reads_best(self._lib.bitnuc_reads_hdist_best_packed, (_ptr(w), int(read_len), int(count), int(k)), int(count), queries)

    def _reads_best2(self, fn, head, count, queries, pattern_k=None):
        q, nq = self._reads_queries(queries, pattern_k)
        out = [np.empty(count, dtype=t) for t in (np.uint32, np.uint32, np.uint8, np.uint32, np.uint32, np.uint8)]
        err = L.BitnucErr()
        if fn(self._h, *head, _ptr(q), nq, *(_ptr(a) for a in out), C.byref(err)) != L.OK:
            _raise(err)
        return tuple(out)

    def reads_hdist_best2(self, reads, read_len, k, queries, count=None):
        """The best match per read as reads_hdist_best, and the runner-up: (query, pos, dist, second_query, second_pos, second_dist), the second triple
        the smallest (distance, query index, offset) over the queries other than the winner's -- another window of the winning query is never the
        runner-up; with one query it is 2^32 - 1, 2^32 - 1, 255.  `count` defaults to len(reads) / read_len."""
        s = _as_u8(reads)
        read_len = int(read_len)
        if count is None:
            if read_len <= 0 or s.size % read_len:
                raise ValueError("reads must hold a whole number of reads of read_len bases")
            count = s.size // read_len
        count = int(count)
        if s.size < count * read_len:
            raise ValueError("reads must hold count reads of read_len bases")
        return self._reads_best2(self._lib.bitnuc_reads_hdist_best2, (_ptr(s), read_len, count, int(k)), count, queries)

    def reads_hdist_best2_packed(self, words, read_len, count, k, queries):
        """reads_hdist_best2 of the packed words encode_fixed writes (ceil(read_len / 32) words per read), without decoding them."""
        w = _as_u64(words)
        if w.size < int(count) * ((int(read_len) + 31) // 32):
            raise ValueError("words must hold count reads of ceil(read_len / 32) words each")
        return self._reads_best2(self._lib.bitnuc_reads_hdist_best2_packed, (_ptr(w), int(read_len), int(count), int(k)), int(count), queries)

    def _reads_anchored(self, fn, head, count, queries, pos_lo, pos_hi, second, pattern_k=None):
        q, nq = self._reads_queries(queries, pattern_k)
        types = (np.uint32, np.uint32, np.uint8) * (2 if second else 1)
        out = [np.empty(count, dtype=t) for t in types]
        ptrs = [_ptr(a) for a in out] + [None] * (6 - len(out))
        err = L.BitnucErr()
        if fn(self._h, *head, int(pos_lo), _SIZE_MAX if pos_hi is None else int(pos_hi), _ptr(q), nq, *ptrs, C.byref(err)) != L.OK:
            _raise(err)
        return tuple(out)

    def reads_hdist_anchored(self, reads, read_len, k, queries, pos_lo=0, pos_hi=None, count=None, second=True):
        """The best match and the runner-up per read as reads_hdist_best2, over the offsets pos_lo <= i <= min(pos_hi, read_len - k) only (pos_hi None: to
        the end of the read; the span hi - pos_lo + k may not exceed 64 bases).  (query, pos, dist, second_query, second_pos, second_dist), positions
        counted in the read; second=False: the best triple only.  Only the span's bytes of each read are read and validated."""
        s = _as_u8(reads)
        read_len = int(read_len)
        if count is None:
            if read_len <= 0 or s.size % read_len:
                raise ValueError("reads must hold a whole number of reads of read_len bases")
            count = s.size // read_len
        count = int(count)
        if s.size < count * read_len:
            raise ValueError("reads must hold count reads of read_len bases")
        return self._reads_anchored(self._lib.bitnuc_reads_hdist_anchored, (_ptr(s), read_len, count, int(k)), count, queries, pos_lo, pos_hi, second)

    def reads_hdist_anchored_packed(self, words, read_len, count, k, queries, pos_lo=0, pos_hi=None, second=True):
        """reads_hdist_anchored of the packed words encode_fixed writes (ceil(read_len / 32) words per read), without decoding them."""
        w = _as_u64(words)
        if w.size < int(count) * ((int(read_len) + 31) // 32):
            raise ValueError("words must hold count reads of ceil(read_len / 32) words each")
        return self._reads_anchored(self._lib.bitnuc_reads_hdist_anchored_packed, (_ptr(w), int(read_len), int(count), int(k)), int(count), queries, pos_lo, pos_hi,
                                    second)

    @staticmethod
    def _anchor(anchor):
        """BITNUC_ANCHOR_START / _END of "start" / "end" (or of 0 / 1)"""
        if anchor in ("start", "end"):
            return 0 if anchor == "start" else 1
        if isinstance(anchor, str):
            raise ValueError('anchor must be "start" or "end"')
        return int(anchor)

    def reads_hdist_anchored_batch(self, seq, offsets, k, queries, pos_lo=0, pos_hi=0, anchor="start", second=True):
        """reads_hdist_anchored of a ragged batch (read r is seq[offsets[r]:offsets[r + 1]]).  anchor="start": the offsets pos_lo <= i <= min(pos_hi,
        len_r - k); anchor="end": those with pos_lo <= len_r - k - i <= pos_hi, measured from each read's own end ("end", 0, 3: the last k bases with
        three bases of slack).  pos_hi - pos_lo + k may not exceed 64.  (query, pos, dist, second_query, second_pos, second_dist), positions counted
        from the read's start; a read without an admissible window: the fill; second=False: the best triple only.  Only span bytes are validated."""
        s = _as_u8(seq)
        off = _as_u64(offsets)
        if off.size == 0:
            raise ValueError("offsets must hold count + 1 entries")
        if s.size < int(off[-1]):
            raise ValueError("seq must hold offsets[-1] bases")
        count = off.size - 1
        return self._reads_anchored(self._lib.bitnuc_reads_hdist_anchored_batch, (_ptr(s), _ptr(off), count, int(k), self._anchor(anchor)), count, queries, pos_lo,
                                    int(pos_hi), second)

    def reads_hdist_anchored_batch_packed(self, words, word_offsets, offsets, k, queries, pos_lo=0, pos_hi=0, anchor="start", second=True):
        """reads_hdist_anchored_batch of the packed words encode_batch writes (read r's ceil(len_r / 32) words start at words[word_offsets[r]]), without
        decoding them."""
        w = _as_u64(words)
        woff = _as_u64(word_offsets)
        off = _as_u64(offsets)
        if off.size == 0 or woff.size != off.size:
            raise ValueError("offsets and word_offsets must hold count + 1 entries each")
        if w.size < int(woff[-1]):
            raise ValueError("words must hold word_offsets[-1] words")
        count = off.size - 1
        return self._reads_anchored(self._lib.bitnuc_reads_hdist_anchored_batch_packed, (_ptr(w), _ptr(woff), _ptr(off), count, int(k), self._anchor(anchor)), count,
                                    queries, pos_lo, int(pos_hi), second)

    def reads_hdist_best_batch(self, seq, offsets, k, queries):
        """The best match per read of a ragged batch: read r is seq[offsets[r]:offsets[r + 1]] (`offsets`: count + 1 non-decreasing entries from 0).
        (query, pos, dist) as reads_hdist_best; an empty read, or one shorter than k: 2^32 - 1, 2^32 - 1, 255."""
        s = _as_u8(seq)
        off = _as_u64(offsets)
        if off.size == 0:
            raise ValueError("offsets must hold count + 1 entries")
        if s.size < int(off[-1]):
            raise ValueError("seq must hold offsets[-1] bases")
        count = off.size - 1
        return self._reads_best(self._lib.bitnuc_reads_hdist_best_batch, (_ptr(s), _ptr(off), count, int(k)), count, queries)

    def reads_hdist_best_batch_packed(self, words, word_offsets, offsets, k, queries):
        """reads_hdist_best_batch of the packed words encode_batch writes (read r's ceil(len_r / 32) words start at words[word_offsets[r]]), without
        decoding them."""
        w = _as_u64(words)
        woff = _as_u64(word_offsets)
        off = _as_u64(offsets)
        if off.size == 0 or woff.size != off.size:
            raise ValueError("offsets and word_offsets must hold count + 1 entries each")
        if w.size < int(woff[-1]):
            raise ValueError("words must hold word_offsets[-1] words")
        count = off.size - 1
        return self._reads_best(self._lib.bitnuc_reads_hdist_best_batch_packed, (_ptr(w), _ptr(woff), _ptr(off), count, int(k)), count, queries)

    # -- pattern queries: a set of bases per position (bitnuc_pattern) -------------------------
    @staticmethod
    def _patterns(patterns, k):
        """(Q, 4) np.uint32 from a (Q, 4) / (4,) uint32 array, one IUPAC string or a list of IUPAC strings of length k"""
        if isinstance(patterns, (str, bytes)):
            patterns = [patterns]
        if isinstance(patterns, (list, tuple)) and patterns and all(isinstance(x, (str, bytes)) for x in patterns):
            for x in patterns:
                if len(x) != int(k):
                    raise ValueError(f"an IUPAC pattern of {len(x)} letters for k = {k}")
            return np.ascontiguousarray(np.stack([pattern_from_iupac(x) for x in patterns]))
        p = np.ascontiguousarray(np.asarray(patterns, dtype=np.uint32).reshape(-1, 4))
        return p

    def kmer_pattern_count_multi(self, ref, k, patterns, taus):
        """counts[q] = the number of windows j of `ref` with pdist(j) = #{i < k : ref[j+i] not in S_i of patterns[q]} <= taus[q] -> np.uint64.
        patterns: a (Q, 4) np.uint32 array (pattern_from_iupac / pattern_from_2bit) or a list of IUPAC strings of length k."""
        s = _as_u8(ref)
        p = self._patterns(patterns, k)
        _, t = self._multi_args(np.zeros(p.shape[0], dtype=np.uint64), taus)
        out = np.empty(p.shape[0], dtype=np.uint64)
        err = L.BitnucErr()
        if self._lib.bitnuc_kmer_pattern_count_multi(self._h, _ptr(s), s.size, int(k), _ptr(p), _ptr(t), p.shape[0], _ptr(out), C.byref(err)) != L.OK:
            _raise(err)
        return out

    def kmer_pattern_count_multi_packed(self, words, n_bases, k, patterns, taus):
        """kmer_pattern_count_multi of the packed sequence `words` holding `n_bases` bases, without decoding it."""
        w = _as_u64(words)
        p = self._patterns(patterns, k)
        _, t = self._multi_args(np.zeros(p.shape[0], dtype=np.uint64), taus)
        out = np.empty(p.shape[0], dtype=np.uint64)
        err = L.BitnucErr()
        if self._lib.bitnuc_kmer_pattern_count_multi_packed(self._h, _ptr(w), w.size, int(n_bases), int(k), _ptr(p), _ptr(t), p.shape[0], _ptr(out),
                                                            C.byref(err)) != L.OK:
            _raise(err)
        return out

    def _pattern_best(self, fn, head, patterns, k):
        p = self._patterns(patterns, k)
        pos = np.empty(p.shape[0], dtype=np.uint64)
        dist = np.empty(p.shape[0], dtype=np.uint8)
        err = L.BitnucErr()
        if fn(self._h, *head, _ptr(p), p.shape[0], _ptr(pos), _ptr(dist), C.byref(err)) != L.OK:
            _raise(err)
        return pos, dist

    def kmer_pattern_best(self, ref, k, patterns):
        """The best match per pattern in one pass: (pos, dist) with dist[q] = the smallest pdist of a window of `ref` under patterns[q] (np.uint8) and
        pos[q] = the leftmost window that attains it (np.uint64); without windows every pos is 2^64 - 1 and every dist 255."""
        s = _as_u8(ref)
        return self._pattern_best(self._lib.bitnuc_kmer_pattern_best, (_ptr(s), s.size, int(k)), patterns, k)

    def kmer_pattern_best_packed(self, words, n_bases, k, patterns):
        """kmer_pattern_best of the packed sequence `words` holding `n_bases` bases, without decoding it."""
        w = _as_u64(words)
        return self._pattern_best(self._lib.bitnuc_kmer_pattern_best_packed, (_ptr(w), w.size, int(n_bases), int(k)), patterns, k)

    # -- the indel-tolerant search along a reference: E(j) = the edit distance of a query to the best substring of `ref` that ends at base j (1 <= j <= n,
    # the substring starts anywhere); `end` is one past the last aligned base, as reads_edist_anchored's --
    def _edist_count(self, fn, head, q, nq, taus):
        _, t = self._multi_args(np.zeros(nq, dtype=np.uint64), taus)
        out = np.empty(nq, dtype=np.uint64)
        err = L.BitnucErr()
        if fn(self._h, *head, _ptr(q), _ptr(t), nq, _ptr(out), C.byref(err)) != L.OK:
            _raise(err)
        return out

    def kmer_edist_best(self, ref, k, queries, with_start=False):
        """The best match per query by EDIT distance: (end, dist) with dist[q] = the smallest E_q(j) over the ends j of `ref` (np.uint8) and end[q] = the
        smallest j that attains it (np.uint64); with k == 0 or len(ref) < k every end is 2^64 - 1 and every dist 255."""
        s = _as_u8(ref)
        res = self._best(self._lib.bitnuc_kmer_edist_best, (_ptr(s), s.size, int(k)), queries)
        return res + (self.kmer_edist_start(s, k, queries, res[0], np.arange(len(res[0]), dtype=np.uint32))[0],) if with_start else res

    def kmer_edist_best_packed(self, words, n_bases, k, queries, with_start=False):
        """kmer_edist_best of the packed sequence `words` holding `n_bases` bases, without decoding it."""
        w = _as_u64(words)
        res = self._best(self._lib.bitnuc_kmer_edist_best_packed, (_ptr(w), w.size, int(n_bases), int(k)), queries)
        return res + (self.kmer_edist_start_packed(w, n_bases, k, queries, res[0], np.arange(len(res[0]), dtype=np.uint32))[0],) if with_start else res

    def kmer_edist_count_multi(self, ref, k, queries, taus):
        """counts[q] = the number of ends j of `ref` with E_q(j) <= taus[q] (the end positions of approximate occurrences) -> np.uint64"""
        s = _as_u8(ref)
        q = np.ascontiguousarray(np.asarray(queries, dtype=np.uint64).reshape(-1))
        return self._edist_count(self._lib.bitnuc_kmer_edist_count_multi, (_ptr(s), s.size, int(k)), q, q.size, taus)

    def kmer_edist_count_multi_packed(self, words, n_bases, k, queries, taus):
        """kmer_edist_count_multi of the packed sequence `words` holding `n_bases` bases, without decoding it."""
        w = _as_u64(words)
        q = np.ascontiguousarray(np.asarray(queries, dtype=np.uint64).reshape(-1))
        return self._edist_count(self._lib.bitnuc_kmer_edist_count_multi_packed, (_ptr(w), w.size, int(n_bases), int(k)), q, q.size, taus)

    def kmer_pattern_edist_best(self, ref, k, patterns, with_start=False):
        """kmer_edist_best under pattern queries ((Q, 4) np.uint32, or IUPAC strings of length k): a base matches a position when it is in its set."""
        s = _as_u8(ref)
        res = self._pattern_best(self._lib.bitnuc_kmer_pattern_edist_best, (_ptr(s), s.size, int(k)), patterns, k)
        return res + (self.kmer_pattern_edist_start(s, k, patterns, res[0], np.arange(len(res[0]), dtype=np.uint32))[0],) if with_start else res

    def kmer_pattern_edist_best_packed(self, words, n_bases, k, patterns, with_start=False):
        """kmer_pattern_edist_best of the packed sequence `words` holding `n_bases` bases."""
        w = _as_u64(words)
        res = self._pattern_best(self._lib.bitnuc_kmer_pattern_edist_best_packed, (_ptr(w), w.size, int(n_bases), int(k)), patterns, k)
        return res + (self.kmer_pattern_edist_start_packed(w, n_bases, k, patterns, res[0], np.arange(len(res[0]), dtype=np.uint32))[0],) if with_start else res

    def kmer_pattern_edist_count_multi(self, ref, k, patterns, taus):
        """kmer_edist_count_multi under pattern queries."""
        s = _as_u8(ref)
        p = self._patterns(patterns, k)
        return self._edist_count(self._lib.bitnuc_kmer_pattern_edist_count_multi, (_ptr(s), s.size, int(k)), p, p.shape[0], taus)

    def kmer_pattern_edist_count_multi_packed(self, words, n_bases, k, patterns, taus):
        """kmer_pattern_edist_count_multi of the packed sequence `words` holding `n_bases` bases."""
        w = _as_u64(words)
        p = self._patterns(patterns, k)
        return self._edist_count(self._lib.bitnuc_kmer_pattern_edist_count_multi_packed, (_ptr(w), w.size, int(n_bases), int(k)), p, p.shape[0], taus)

    def kmer_edist_hits(self, ref, k, query, tau, with_dist=False, with_start=False):
        """Ends (np.uint64, ascending, 1 <= end <= n: one past the last aligned base) of the substrings of `ref` within edit distance tau of the query: the
        j with E(j) <= tau; with_dist: (ends, np.uint8 distances).  Neighbouring ends of a good match are hits too: the list is not collapsed to minima."""
        s = _as_u8(ref)
        res = self._hits(self._lib.bitnuc_kmer_edist_hits, (_ptr(s), s.size, int(k), C.c_uint64(query), int(tau)), with_dist)
        if not with_start:
            return res
        start = self.kmer_edist_start(s, k, [query], res[0] if with_dist else res)[0]
        return res + (start,) if with_dist else (res, start)

    def kmer_edist_hits_packed(self, words, n_bases, k, query, tau, with_dist=False, with_start=False):
        """kmer_edist_hits of the packed sequence `words` holding `n_bases` bases, without decoding it."""
        w = _as_u64(words)
        res = self._hits(self._lib.bitnuc_kmer_edist_hits_packed, (_ptr(w), w.size, int(n_bases), int(k), C.c_uint64(query), int(tau)), with_dist)
        if not with_start:
            return res
        start = self.kmer_edist_start_packed(w, n_bases, k, [query], res[0] if with_dist else res)[0]
        return res + (start,) if with_dist else (res, start)

    def kmer_pattern_edist_hits(self, ref, k, pattern, tau, with_dist=False, with_start=False):
        """kmer_edist_hits under a pattern query (a (4,) np.uint32 array or an IUPAC string of length k)."""
        s = _as_u8(ref)
        p = self._patterns(pattern, k)[:1]
        res = self._hits(self._lib.bitnuc_kmer_pattern_edist_hits, (_ptr(s), s.size, int(k), _ptr(p), int(tau)), with_dist)
        if not with_start:
            return res
        start = self.kmer_pattern_edist_start(s, k, p, res[0] if with_dist else res)[0]
        return res + (start,) if with_dist else (res, start)

    def kmer_pattern_edist_hits_packed(self, words, n_bases, k, pattern, tau, with_dist=False, with_start=False):
        """kmer_pattern_edist_hits of the packed sequence `words` holding `n_bases` bases."""
        w = _as_u64(words)
        p = self._patterns(pattern, k)[:1]
        res = self._hits(self._lib.bitnuc_kmer_pattern_edist_hits_packed, (_ptr(w), w.size, int(n_bases), int(k), _ptr(p), int(tau)), with_dist)
        if not with_start:
            return res
        start = self.kmer_pattern_edist_start_packed(w, n_bases, k, p, res[0] if with_dist else res)[0]
        return res + (start,) if with_dist else (res, start)

    # -- pattern queries for the per-read matchers: the reads_hdist_* methods with `patterns` ((Q, 4) np.uint32, or IUPAC strings of length k) where
    # `queries` stood and pdist where the Hamming distance stood; everything else as their exact twins --
    @staticmethod
    def _fixed_reads(reads, read_len, count):
        s = _as_u8(reads)
        read_len = int(read_len)
        if count is None:
            if read_len <= 0 or s.size % read_len:
                raise ValueError("reads must hold a whole number of reads of read_len bases")
            count = s.size // read_len
        count = int(count)
        if s.size < count * read_len:
            raise ValueError("reads must hold count reads of read_len bases")
        return s, read_len, count

    @staticmethod
    def _fixed_words(words, read_len, count):
        w = _as_u64(words)
        if w.size < int(count) * ((int(read_len) + 31) // 32):
            raise ValueError("words must hold count reads of ceil(read_len / 32) words each")
        return w, int(read_len), int(count)

    @staticmethod
    def _ragged_reads(seq, offsets):
        s = _as_u8(seq)
        off = _as_u64(offsets)
        if off.size == 0:
            raise ValueError("offsets must hold count + 1 entries")
        if s.size < int(off[-1]):
            raise ValueError("seq must hold offsets[-1] bases")
        return s, off, off.size - 1

    @staticmethod
    def _ragged_words(words, word_offsets, offsets):
        w = _as_u64(words)
        woff = _as_u64(word_offsets)
        off = _as_u64(offsets)
        if off.size == 0 or woff.size != off.size:
            raise ValueError("offsets and word_offsets must hold count + 1 entries each")
        if w.size < int(woff[-1]):
            raise ValueError("words must hold word_offsets[-1] words")
        return w, woff, off, off.size - 1

    def reads_pattern_best(self, reads, read_len, k, patterns, count=None):
        """reads_hdist_best under pattern queries: per read the smallest (pdist, pattern index, offset) -> (query, pos, dist).  An N in a READ is still
        an invalid base: the sets are on the query's side only."""
        s, read_len, count = self._fixed_reads(reads, read_len, count)
        return self._reads_best(self._lib.bitnuc_reads_pattern_best, (_ptr(s), read_len, count, int(k)), count, patterns, int(k))

    def reads_pattern_best_packed(self, words, read_len, count, k, patterns):
        """reads_pattern_best of the packed words encode_fixed writes (ceil(read_len / 32) words per read), without decoding them."""
        w, read_len, count = self._fixed_words(words, read_len, count)
        return self._reads_best(self._lib.bitnuc_reads_pattern_best_packed, (_ptr(w), read_len, count, int(k)), count, patterns, int(k))

    def reads_pattern_best2(self, reads, read_len, k, patterns, count=None):
        """reads_hdist_best2 under pattern queries: two equal patterns are two queries (the one at the higher index is the runner-up), another window of
        the winning pattern never is."""
        s, read_len, count = self._fixed_reads(reads, read_len, count)
        return self._reads_best2(self._lib.bitnuc_reads_pattern_best2, (_ptr(s), read_len, count, int(k)), count, patterns, int(k))

    def reads_pattern_best2_packed(self, words, read_len, count, k, patterns):
        """reads_pattern_best2 of the packed words encode_fixed writes, without decoding them."""
        w, read_len, count = self._fixed_words(words, read_len, count)
        return self._reads_best2(self._lib.bitnuc_reads_pattern_best2_packed, (_ptr(w), read_len, count, int(k)), count, patterns, int(k))

    def reads_pattern_anchored(self, reads, read_len, k, patterns, pos_lo=0, pos_hi=None, count=None, second=True):
        """reads_hdist_anchored under pattern queries (the offsets pos_lo <= i <= min(pos_hi, read_len - k); span at most 64 bases)."""
        s, read_len, count = self._fixed_reads(reads, read_len, count)
        return self._reads_anchored(self._lib.bitnuc_reads_pattern_anchored, (_ptr(s), read_len, count, int(k)), count, patterns, pos_lo, pos_hi, second, int(k))

    def reads_pattern_anchored_packed(self, words, read_len, count, k, patterns, pos_lo=0, pos_hi=None, second=True):
        """reads_pattern_anchored of the packed words encode_fixed writes, without decoding them."""
        w, read_len, count = self._fixed_words(words, read_len, count)
        return self._reads_anchored(self._lib.bitnuc_reads_pattern_anchored_packed, (_ptr(w), read_len, count, int(k)), count, patterns, pos_lo, pos_hi, second,
                                    int(k))

    def reads_edist_anchored(self, reads, read_len, k, queries, pos_lo=0, pos_hi=None, count=None, second=True, with_start=False):
        """The indel-tolerant anchored match: as reads_hdist_anchored, with the EDIT (Levenshtein) distance of each query to the best substring of the
        read's span [pos_lo, min(pos_hi, read_len - k) + k) (at most 64 bases; the substring starts and ends anywhere in it).  (query, end, dist,
        second_query, second_end, second_dist): the smallest (dist, query, end) and the smallest over the other queries; end is an offset in the read,
        one past the last aligned base (with_start=True appends the start arrays: reads_edist_start).  dist is never above reads_hdist_anchored's.  second=False: the best triple only."""
        s, read_len, count = self._fixed_reads(reads, read_len, count)
        res = self._reads_anchored(self._lib.bitnuc_reads_edist_anchored, (_ptr(s), read_len, count, int(k)), count, queries, pos_lo, pos_hi, second)
        return self._append_starts(res, lambda q, e: self.reads_edist_start(s, read_len, k, queries, q, e, "start", pos_lo, count)) if with_start else res

    def reads_edist_anchored_packed(self, words, read_len, count, k, queries, pos_lo=0, pos_hi=None, second=True, with_start=False):
        """reads_edist_anchored of the packed words encode_fixed writes (ceil(read_len / 32) words per read), without decoding them."""
        w, read_len, count = self._fixed_words(words, read_len, count)
        res = self._reads_anchored(self._lib.bitnuc_reads_edist_anchored_packed, (_ptr(w), read_len, count, int(k)), count, queries, pos_lo, pos_hi, second)
        return self._append_starts(res, lambda q, e: self.reads_edist_start_packed(w, read_len, count, k, queries, q, e, "start", pos_lo)) if with_start else res

    def reads_pattern_edist_anchored(self, reads, read_len, k, patterns, pos_lo=0, pos_hi=None, count=None, second=True, with_start=False):
        """reads_edist_anchored under pattern queries: a read base matches query position i when it is in the position's set."""
        s, read_len, count = self._fixed_reads(reads, read_len, count)
        res = self._reads_anchored(self._lib.bitnuc_reads_pattern_edist_anchored, (_ptr(s), read_len, count, int(k)), count, patterns, pos_lo, pos_hi, second,
                                    int(k))
        return self._append_starts(res, lambda q, e: self.reads_pattern_edist_start(s, read_len, k, patterns, q, e, "start", pos_lo, count)) if with_start else res

    def reads_pattern_edist_anchored_packed(self, words, read_len, count, k, patterns, pos_lo=0, pos_hi=None, second=True, with_start=False):
        """reads_pattern_edist_anchored of the packed words encode_fixed writes, without decoding them."""
        w, read_len, count = self._fixed_words(words, read_len, count)
        res = self._reads_anchored(self._lib.bitnuc_reads_pattern_edist_anchored_packed, (_ptr(w), read_len, count, int(k)), count, patterns, pos_lo, pos_hi,
                                    second, int(k))
        return self._append_starts(res, lambda q, e: self.reads_pattern_edist_start_packed(w, read_len, count, k, patterns, q, e, "start", pos_lo)) if with_start else res

    def reads_edist_anchored_batch(self, seq, offsets, k, queries, pos_lo=0, pos_hi=0, anchor="start", second=True, with_start=False):
        """reads_edist_anchored of a ragged batch (read r is seq[offsets[r]:offsets[r + 1]]): the EDIT distance of each query to the best substring of the
        read's own span, the bases reads_hdist_anchored_batch looks at for the same (anchor, pos_lo, pos_hi) -- a short read gets its shortened span, a
        read without a window the fill.  pos_hi - pos_lo + k may not exceed 64.  (query, end, dist, second_query, second_end, second_dist); end is
        counted from the read's start in both anchor modes, one past the last aligned base.  second=False: the best triple only."""
        s, off, count = self._ragged_reads(seq, offsets)
        res = self._reads_anchored(self._lib.bitnuc_reads_edist_anchored_batch, (_ptr(s), _ptr(off), count, int(k), self._anchor(anchor)), count, queries, pos_lo,
                                    int(pos_hi), second)
        return self._append_starts(res, lambda q, e: self.reads_edist_start_batch(s, off, k, queries, q, e, *self._start_floor(anchor, pos_lo, pos_hi))) if with_start else res

    def reads_edist_anchored_batch_packed(self, words, word_offsets, offsets, k, queries, pos_lo=0, pos_hi=0, anchor="start", second=True, with_start=False):
        """reads_edist_anchored_batch of the packed words encode_batch writes (read r's ceil(len_r / 32) words start at words[word_offsets[r]])."""
        w, woff, off, count = self._ragged_words(words, word_offsets, offsets)
        res = self._reads_anchored(self._lib.bitnuc_reads_edist_anchored_batch_packed, (_ptr(w), _ptr(woff), _ptr(off), count, int(k), self._anchor(anchor)), count,
                                    queries, pos_lo, int(pos_hi), second)
        return self._append_starts(res, lambda q, e: self.reads_edist_start_batch_packed(w, woff, off, k, queries, q, e, *self._start_floor(anchor, pos_lo, pos_hi))) if with_start else res

    def reads_pattern_edist_anchored_batch(self, seq, offsets, k, patterns, pos_lo=0, pos_hi=0, anchor="start", second=True, with_start=False):
        """reads_edist_anchored_batch under pattern queries: a read base matches query position i when it is in the position's set."""
        s, off, count = self._ragged_reads(seq, offsets)
        res = self._reads_anchored(self._lib.bitnuc_reads_pattern_edist_anchored_batch, (_ptr(s), _ptr(off), count, int(k), self._anchor(anchor)), count, patterns,
                                    pos_lo, int(pos_hi), second, int(k))
        return self._append_starts(res, lambda q, e: self.reads_pattern_edist_start_batch(s, off, k, patterns, q, e, *self._start_floor(anchor, pos_lo, pos_hi))) if with_start else res

    def reads_pattern_edist_anchored_batch_packed(self, words, word_offsets, offsets, k, patterns, pos_lo=0, pos_hi=0, anchor="start", second=True, with_start=False):
        """reads_pattern_edist_anchored_batch of the packed words encode_batch writes, without decoding them."""
        w, woff, off, count = self._ragged_words(words, word_offsets, offsets)
        res = self._reads_anchored(self._lib.bitnuc_reads_pattern_edist_anchored_batch_packed, (_ptr(w), _ptr(woff), _ptr(off), count, int(k), self._anchor(anchor)),
                                    count, patterns, pos_lo, int(pos_hi), second, int(k))
        return self._append_starts(res, lambda q, e: self.reads_pattern_edist_start_batch_packed(w, woff, off, k, patterns, q, e, *self._start_floor(anchor, pos_lo, pos_hi))) if with_start else res

    def _reads_edist_best(self, fn, head, count, queries, second, pattern_k=None):
        q, nq = self._reads_queries(queries, pattern_k)
        types = (np.uint32, np.uint32, np.uint8) * (2 if second else 1)
        out = [np.empty(count, dtype=t) for t in types]
        ptrs = [_ptr(a) for a in out] + [None] * (6 - len(out))
        err = L.BitnucErr()
        if fn(self._h, *head, _ptr(q), nq, *ptrs, C.byref(err)) != L.OK:
            _raise(err)
        return tuple(out)

    def reads_edist_best(self, reads, read_len, k, queries, count=None, second=True, with_start=False):
        """The indel-tolerant best match over the WHOLE read: per read the smallest (edit distance, query, end) over the queries, the EDIT (Levenshtein)
        distance of a query being that to the best substring of the read (it starts and ends anywhere; reads of up to 2^26 bases), and the smallest over
        the other queries.  (query, end, dist, second_query, second_end, second_dist); end is one past the last aligned base, counted from the read's
        start (with_start=True appends the start arrays: reads_edist_start).  dist is never above reads_hdist_best's.  second=False: the best triple only."""
        s, read_len, count = self._fixed_reads(reads, read_len, count)
        res = self._reads_edist_best(self._lib.bitnuc_reads_edist_best, (_ptr(s), read_len, count, int(k)), count, queries, second)
        return self._append_starts(res, lambda q, e: self.reads_edist_start(s, read_len, k, queries, q, e, "start", 0, count)) if with_start else res

    def reads_edist_best_packed(self, words, read_len, count, k, queries, second=True, with_start=False):
        """reads_edist_best of the packed words encode_fixed writes (ceil(read_len / 32) words per read), without decoding them."""
        w, read_len, count = self._fixed_words(words, read_len, count)
        res = self._reads_edist_best(self._lib.bitnuc_reads_edist_best_packed, (_ptr(w), read_len, count, int(k)), count, queries, second)
        return self._append_starts(res, lambda q, e: self.reads_edist_start_packed(w, read_len, count, k, queries, q, e, "start", 0)) if with_start else res

    def reads_pattern_edist_best(self, reads, read_len, k, patterns, count=None, second=True, with_start=False):
        """reads_edist_best under pattern queries: a read base matches query position i when it is in the position's set."""
        s, read_len, count = self._fixed_reads(reads, read_len, count)
        res = self._reads_edist_best(self._lib.bitnuc_reads_pattern_edist_best, (_ptr(s), read_len, count, int(k)), count, patterns, second, int(k))
        return self._append_starts(res, lambda q, e: self.reads_pattern_edist_start(s, read_len, k, patterns, q, e, "start", 0, count)) if with_start else res

    def reads_pattern_edist_best_packed(self, words, read_len, count, k, patterns, second=True, with_start=False):
        """reads_pattern_edist_best of the packed words encode_fixed writes, without decoding them."""
        w, read_len, count = self._fixed_words(words, read_len, count)
        res = self._reads_edist_best(self._lib.bitnuc_reads_pattern_edist_best_packed, (_ptr(w), read_len, count, int(k)), count, patterns, second, int(k))
        return self._append_starts(res, lambda q, e: self.reads_pattern_edist_start_packed(w, read_len, count, k, patterns, q, e, "start", 0)) if with_start else res

    def reads_edist_best_batch(self, seq, offsets, k, queries, second=True, with_start=False):
        """reads_edist_best of a ragged batch (read r is seq[offsets[r]:offsets[r + 1]]): each read against every query over its own whole length; a
        read shorter than k gets the fill and is neither read nor validated.  Ends are counted from the read's start."""
        s, off, count = self._ragged_reads(seq, offsets)
        res = self._reads_edist_best(self._lib.bitnuc_reads_edist_best_batch, (_ptr(s), _ptr(off), count, int(k)), count, queries, second)
        return self._append_starts(res, lambda q, e: self.reads_edist_start_batch(s, off, k, queries, q, e, "start", 0)) if with_start else res

    def reads_edist_best_batch_packed(self, words, word_offsets, offsets, k, queries, second=True, with_start=False):
        """reads_edist_best_batch of the packed words encode_batch writes (read r's ceil(len_r / 32) words start at words[word_offsets[r]])."""
        w, woff, off, count = self._ragged_words(words, word_offsets, offsets)
        res = self._reads_edist_best(self._lib.bitnuc_reads_edist_best_batch_packed, (_ptr(w), _ptr(woff), _ptr(off), count, int(k)), count, queries, second)
        return self._append_starts(res, lambda q, e: self.reads_edist_start_batch_packed(w, woff, off, k, queries, q, e, "start", 0)) if with_start else res

    def reads_pattern_edist_best_batch(self, seq, offsets, k, patterns, second=True, with_start=False):
        """reads_edist_best_batch under pattern queries."""
        s, off, count = self._ragged_reads(seq, offsets)
        res = self._reads_edist_best(self._lib.bitnuc_reads_pattern_edist_best_batch, (_ptr(s), _ptr(off), count, int(k)), count, patterns, second, int(k))
        return self._append_starts(res, lambda q, e: self.reads_pattern_edist_start_batch(s, off, k, patterns, q, e, "start", 0)) if with_start else res

    def reads_pattern_edist_best_batch_packed(self, words, word_offsets, offsets, k, patterns, second=True, with_start=False):
        """reads_pattern_edist_best_batch of the packed words encode_batch writes, without decoding them."""
        w, woff, off, count = self._ragged_words(words, word_offsets, offsets)
        res = self._reads_edist_best(self._lib.bitnuc_reads_pattern_edist_best_batch_packed, (_ptr(w), _ptr(woff), _ptr(off), count, int(k)), count, patterns,
                                      second, int(k))
        return self._append_starts(res, lambda q, e: self.reads_pattern_edist_start_batch_packed(w, woff, off, k, patterns, q, e, "start", 0)) if with_start else res

    # -- the 3' adapter per read: of Q adapters the one a read carries in full anywhere or as a prefix overhanging its end, within floor(i x num / den)
    # edits over i matched-against adapter positions, and the base to cut at.  (adapter, cut, end, overlap, dist); no admissible candidate: 2^32 - 1 x 3, 255 x 2 --
    def _reads_adapter(self, fn, head, count, queries, min_overlap, rate, pattern_k=None):  # rate: (err_num, err_den)
        q, nq = self._reads_queries(queries, pattern_k)
        num, den = rate
        out = [np.empty(count, dtype=t) for t in (np.uint32, np.uint32, np.uint32, np.uint8, np.uint8)]
        err = L.BitnucErr()
        if fn(self._h, *head, _ptr(q), nq, int(min_overlap), int(num), int(den), *(_ptr(a) for a in out), C.byref(err)) != L.OK:
            _raise(err)
        return tuple(out)

    def reads_edist_adapter(self, reads, read_len, k, queries, min_overlap=3, err_num=1, err_den=10, count=None):
        """The 3' adapter per read of a fixed-length batch: (adapter, cut, end, overlap, dist).  A candidate is a FULL adapter ending at any base of the
        read (overlap = k) or its first `overlap` positions, min_overlap <= overlap < k, aligned to the read's END; it is admissible within
        floor(overlap x err_num / err_den) edits.  The winner has the most matched adapter positions, then the fewest edits, the lower index, the first
        end; read[:cut] is what a trimmer keeps, dist the edit distance of the adapter's prefix to read[cut:end]."""
        s, read_len, count = self._fixed_reads(reads, read_len, count)
        return self._reads_adapter(self._lib.bitnuc_reads_edist_adapter, (_ptr(s), read_len, count, int(k)), count, queries, min_overlap, (err_num, err_den))

    def reads_edist_adapter_packed(self, words, read_len, count, k, queries, min_overlap=3, err_num=1, err_den=10):
        """reads_edist_adapter of the packed words encode_fixed writes (ceil(read_len / 32) words per read), without decoding them."""
        w, read_len, count = self._fixed_words(words, read_len, count)
        return self._reads_adapter(self._lib.bitnuc_reads_edist_adapter_packed, (_ptr(w), read_len, count, int(k)), count, queries, min_overlap, (err_num, err_den))

    def reads_pattern_edist_adapter(self, reads, read_len, k, patterns, min_overlap=3, err_num=1, err_den=10, count=None):
        """reads_edist_adapter under pattern queries: a read base matches adapter position i when it is in the position's set."""
        s, read_len, count = self._fixed_reads(reads, read_len, count)
        return self._reads_adapter(self._lib.bitnuc_reads_pattern_edist_adapter, (_ptr(s), read_len, count, int(k)), count, patterns, min_overlap, (err_num, err_den), int(k))

    def reads_pattern_edist_adapter_packed(self, words, read_len, count, k, patterns, min_overlap=3, err_num=1, err_den=10):
        """reads_pattern_edist_adapter of the packed words encode_fixed writes, without decoding them."""
        w, read_len, count = self._fixed_words(words, read_len, count)
        return self._reads_adapter(self._lib.bitnuc_reads_pattern_edist_adapter_packed, (_ptr(w), read_len, count, int(k)), count, patterns, min_overlap,
                                   (err_num, err_den), int(k))

    def reads_edist_adapter_batch(self, seq, offsets, k, queries, min_overlap=3, err_num=1, err_den=10):
        """reads_edist_adapter of a ragged batch (read r is seq[offsets[r]:offsets[r + 1]]): each read over its own length; a read shorter than k gets
        the fill and is neither read nor validated."""
        s, off, count = self._ragged_reads(seq, offsets)
        return self._reads_adapter(self._lib.bitnuc_reads_edist_adapter_batch, (_ptr(s), _ptr(off), count, int(k)), count, queries, min_overlap, (err_num, err_den))

    def reads_edist_adapter_batch_packed(self, words, word_offsets, offsets, k, queries, min_overlap=3, err_num=1, err_den=10):
        """reads_edist_adapter_batch of the packed words encode_batch writes (read r's ceil(len_r / 32) words start at words[word_offsets[r]])."""
        w, woff, off, count = self._ragged_words(words, word_offsets, offsets)
        return self._reads_adapter(self._lib.bitnuc_reads_edist_adapter_batch_packed, (_ptr(w), _ptr(woff), _ptr(off), count, int(k)), count, queries,
                                   min_overlap, (err_num, err_den))

    def reads_pattern_edist_adapter_batch(self, seq, offsets, k, patterns, min_overlap=3, err_num=1, err_den=10):
        """reads_edist_adapter_batch under pattern queries."""
        s, off, count = self._ragged_reads(seq, offsets)
        return self._reads_adapter(self._lib.bitnuc_reads_pattern_edist_adapter_batch, (_ptr(s), _ptr(off), count, int(k)), count, patterns, min_overlap,
                                   (err_num, err_den), int(k))

    def reads_pattern_edist_adapter_batch_packed(self, words, word_offsets, offsets, k, patterns, min_overlap=3, err_num=1, err_den=10):
        """reads_pattern_edist_adapter_batch of the packed words encode_batch writes, without decoding them."""
        w, woff, off, count = self._ragged_words(words, word_offsets, offsets)
        return self._reads_adapter(self._lib.bitnuc_reads_pattern_edist_adapter_batch_packed, (_ptr(w), _ptr(woff), _ptr(off), count, int(k)), count, patterns,
                                   min_overlap, (err_num, err_den), int(k))

    # -- the indel-tolerant family's second stage: WHERE the alignment that ends at end[r] starts.  Per item (query index, end) -> (start, dist): the smallest
    # edit distance of the query to a substring t[s, end) with s at or behind the floor and, among those, the shortest; dist equals the forward form's when
    # the floor is its span start.  A skipped item (query >= Q, end beyond the read or in front of the floor) gets 2^32 - 1 (2^64 - 1), 255 --
    def _reads_start(self, fn, head, count, k, queries, query, end, anchor, pos, pattern_k=None):
        q, nq = self._reads_queries(queries, pattern_k)
        qi = np.ascontiguousarray(np.asarray(query, dtype=np.uint32).reshape(-1))
        en = np.ascontiguousarray(np.asarray(end, dtype=np.uint32).reshape(-1))
        if qi.size < count or en.size < count:
            raise ValueError("query and end must hold one entry per read")
        start = np.empty(count, dtype=np.uint32)
        dist = np.empty(count, dtype=np.uint8)
        err = L.BitnucErr()
        if fn(self._h, *head, int(k), self._anchor(anchor), int(pos), _ptr(q), nq, _ptr(qi), _ptr(en), _ptr(start), _ptr(dist), C.byref(err)) != L.OK:
            _raise(err)
        return start, dist

    def reads_edist_start(self, reads, read_len, k, queries, query, end, anchor="start", pos=0, count=None):
        """(start, dist) per read of a fixed-length batch: the alignment of queries[query[r]] that ends at end[r] (one past its last base) starts at
        start[r].  The floor: anchor="start": pos; "end": read_len - k - pos (at least 0).  After reads_edist_best: ("start", 0); after
        reads_edist_anchored: ("start", pos_lo)."""
        s, read_len, count = self._fixed_reads(reads, read_len, count)
        return self._reads_start(self._lib.bitnuc_reads_edist_start, (_ptr(s), read_len, count), count, k, queries, query, end, anchor, pos)

    def reads_edist_start_packed(self, words, read_len, count, k, queries, query, end, anchor="start", pos=0):
        """reads_edist_start of the packed words encode_fixed writes."""
        w, read_len, count = self._fixed_words(words, read_len, count)
        return self._reads_start(self._lib.bitnuc_reads_edist_start_packed, (_ptr(w), read_len, count), count, k, queries, query, end, anchor, pos)

    def reads_pattern_edist_start(self, reads, read_len, k, patterns, query, end, anchor="start", pos=0, count=None):
        """reads_edist_start under pattern queries."""
        s, read_len, count = self._fixed_reads(reads, read_len, count)
        return self._reads_start(self._lib.bitnuc_reads_pattern_edist_start, (_ptr(s), read_len, count), count, k, patterns, query, end, anchor, pos, int(k))

    def reads_pattern_edist_start_packed(self, words, read_len, count, k, patterns, query, end, anchor="start", pos=0):
        """reads_pattern_edist_start of the packed words encode_fixed writes."""
        w, read_len, count = self._fixed_words(words, read_len, count)
        return self._reads_start(self._lib.bitnuc_reads_pattern_edist_start_packed, (_ptr(w), read_len, count), count, k, patterns, query, end, anchor, pos, int(k))

    def reads_edist_start_batch(self, seq, offsets, k, queries, query, end, anchor="start", pos=0):
        """reads_edist_start of a ragged batch; the floor of read r: "start": pos; "end": len_r - k - pos (at least 0).  After reads_edist_best_batch:
        ("start", 0); after reads_edist_anchored_batch: ("start", pos_lo) or ("end", pos_hi)."""
        s, off, count = self._ragged_reads(seq, offsets)
        return self._reads_start(self._lib.bitnuc_reads_edist_start_batch, (_ptr(s), _ptr(off), count), count, k, queries, query, end, anchor, pos)

    def reads_edist_start_batch_packed(self, words, word_offsets, offsets, k, queries, query, end, anchor="start", pos=0):
        """reads_edist_start_batch of the packed words encode_batch writes."""
        w, woff, off, count = self._ragged_words(words, word_offsets, offsets)
        return self._reads_start(self._lib.bitnuc_reads_edist_start_batch_packed, (_ptr(w), _ptr(woff), _ptr(off), count), count, k, queries, query, end, anchor, pos)

    def reads_pattern_edist_start_batch(self, seq, offsets, k, patterns, query, end, anchor="start", pos=0):
        """reads_edist_start_batch under pattern queries."""
        s, off, count = self._ragged_reads(seq, offsets)
        return self._reads_start(self._lib.bitnuc_reads_pattern_edist_start_batch, (_ptr(s), _ptr(off), count), count, k, patterns, query, end, anchor, pos, int(k))

    def reads_pattern_edist_start_batch_packed(self, words, word_offsets, offsets, k, patterns, query, end, anchor="start", pos=0):
        """reads_pattern_edist_start_batch of the packed words encode_batch writes."""
        w, woff, off, count = self._ragged_words(words, word_offsets, offsets)
        return self._reads_start(self._lib.bitnuc_reads_pattern_edist_start_batch_packed, (_ptr(w), _ptr(woff), _ptr(off), count), count, k, patterns, query, end,
                                 anchor, pos, int(k))

    def _kmer_start(self, fn, head, q, nq, end, query_index):
        en = np.ascontiguousarray(np.asarray(end, dtype=np.uint64).reshape(-1))
        qi = None if query_index is None else np.ascontiguousarray(np.asarray(query_index, dtype=np.uint32).reshape(-1))
        if qi is not None and qi.size < en.size:
            raise ValueError("query_index must hold one entry per end")
        start = np.empty(en.size, dtype=np.uint64)
        dist = np.empty(en.size, dtype=np.uint8)
        err = L.BitnucErr()
        if fn(self._h, *head, _ptr(q), nq, None if qi is None else _ptr(qi), _ptr(en), en.size, _ptr(start), _ptr(dist), C.byref(err)) != L.OK:
            _raise(err)
        return start, dist

    def kmer_edist_start(self, ref, k, queries, end, query_index=None):
        """(start, dist) per item along `ref`: the alignment of queries[query_index[i]] (None: queries[0], the hit list's case) that ends at end[i] starts
        at start[i] (np.uint64).  After kmer_edist_best pass query_index = arange(Q).  Always host code: an item reads at most 63 bases."""
        s = _as_u8(ref)
        q = np.ascontiguousarray(np.asarray(queries, dtype=np.uint64).reshape(-1))
        return self._kmer_start(self._lib.bitnuc_ref_edist_start, (_ptr(s), s.size, int(k)), q, q.size, end, query_index)

    def kmer_edist_start_packed(self, words, n_bases, k, queries, end, query_index=None):
        """kmer_edist_start of the packed sequence `words` holding `n_bases` bases."""
        w = _as_u64(words)
        q = np.ascontiguousarray(np.asarray(queries, dtype=np.uint64).reshape(-1))
        return self._kmer_start(self._lib.bitnuc_ref_edist_start_packed, (_ptr(w), w.size, int(n_bases), int(k)), q, q.size, end, query_index)

    def kmer_pattern_edist_start(self, ref, k, patterns, end, query_index=None):
        """kmer_edist_start under pattern queries."""
        s = _as_u8(ref)
        p = self._patterns(patterns, k)
        return self._kmer_start(self._lib.bitnuc_ref_pattern_edist_start, (_ptr(s), s.size, int(k)), p, p.shape[0], end, query_index)

    def kmer_pattern_edist_start_packed(self, words, n_bases, k, patterns, end, query_index=None):
        """kmer_pattern_edist_start of the packed sequence `words` holding `n_bases` bases."""
        w = _as_u64(words)
        p = self._patterns(patterns, k)
        return self._kmer_start(self._lib.bitnuc_ref_pattern_edist_start_packed, (_ptr(w), w.size, int(n_bases), int(k)), p, p.shape[0], end, query_index)

    def _start_floor(self, anchor, pos_lo, pos_hi):
        """the floor a ragged anchored form's span starts at, as (anchor, pos) of reads_edist_start_batch: its first admissible offset is pos_lo from the
        read's start, or pos_hi (saturating) from its end"""
        return ("end", int(pos_hi)) if self._anchor(anchor) == 1 else ("start", int(pos_lo))

    @staticmethod
    def _append_starts(res, starter):
        """a per-read forward result (query, end, dist[, second_query, second_end, second_dist]) with the start arrays as extra trailing results: one
        starter(query, end) -> (start, dist) call per triple"""
        starts = tuple(starter(res[i], res[i + 1])[0] for i in range(0, len(res), 3))
        return tuple(res) + starts

    def reads_pattern_anchored_batch(self, seq, offsets, k, patterns, pos_lo=0, pos_hi=0, anchor="start", second=True):
        """reads_hdist_anchored_batch under pattern queries (a ragged batch; the range counted from each read's start or end)."""
        s, off, count = self._ragged_reads(seq, offsets)
        return self._reads_anchored(self._lib.bitnuc_reads_pattern_anchored_batch, (_ptr(s), _ptr(off), count, int(k), self._anchor(anchor)), count, patterns, pos_lo,
                                    int(pos_hi), second, int(k))

    def reads_pattern_anchored_batch_packed(self, words, word_offsets, offsets, k, patterns, pos_lo=0, pos_hi=0, anchor="start", second=True):
        """reads_pattern_anchored_batch of the packed words encode_batch writes, without decoding them."""
        w, woff, off, count = self._ragged_words(words, word_offsets, offsets)
        return self._reads_anchored(self._lib.bitnuc_reads_pattern_anchored_batch_packed, (_ptr(w), _ptr(woff), _ptr(off), count, int(k), self._anchor(anchor)), count,
                                    patterns, pos_lo, int(pos_hi), second, int(k))

    def reads_pattern_best_batch(self, seq, offsets, k, patterns):
        """reads_hdist_best_batch under pattern queries (a ragged batch, every window of every read)."""
        s, off, count = self._ragged_reads(seq, offsets)
        return self._reads_best(self._lib.bitnuc_reads_pattern_best_batch, (_ptr(s), _ptr(off), count, int(k)), count, patterns, int(k))

    def reads_pattern_best_batch_packed(self, words, word_offsets, offsets, k, patterns):
        """reads_pattern_best_batch of the packed words encode_batch writes, without decoding them."""
        w, woff, off, count = self._ragged_words(words, word_offsets, offsets)
        return self._reads_best(self._lib.bitnuc_reads_pattern_best_batch_packed, (_ptr(w), _ptr(woff), _ptr(off), count, int(k)), count, patterns, int(k))

    # -- the mismatch histogram per query: windows at each distance 0 .. n_bins - 1 in one pass --
    def _hist(self, fn, head, q, nq, n_bins):
        n_bins = int(n_bins)
        out = np.empty((nq, min(max(n_bins, 0), 16)), dtype=np.uint64)  # (a refused n_bins writes nothing)
        err = L.BitnucErr()
        if fn(self._h, *head, _ptr(q), nq, n_bins, _ptr(out), C.byref(err)) != L.OK:
            _raise(err)
        return out

    def kmer_hdist_hist(self, ref, k, queries, n_bins):
        """hist[q, d] = the number of windows of `ref` at Hamming distance exactly d from queries[q], d < n_bins <= 16, one pass for all queries
        -> (n_queries, n_bins) np.uint64; a window at n_bins or more mismatches is counted nowhere."""
        s = _as_u8(ref)
        q = np.ascontiguousarray(np.asarray(queries, dtype=np.uint64).reshape(-1))  # a scalar query: Q = 1
        return self._hist(self._lib.bitnuc_kmer_hdist_hist, (_ptr(s), s.size, int(k)), q, q.size, n_bins)

    def kmer_hdist_hist_packed(self, words, n_bases, k, queries, n_bins):
        """kmer_hdist_hist of the packed sequence `words` holding `n_bases` bases, without decoding it."""
        w = _as_u64(words)
        q = np.ascontiguousarray(np.asarray(queries, dtype=np.uint64).reshape(-1))
        return self._hist(self._lib.bitnuc_kmer_hdist_hist_packed, (_ptr(w), w.size, int(n_bases), int(k)), q, q.size, n_bins)

    def kmer_pattern_hist(self, ref, k, patterns, n_bins):
        """hist[q, d] = the number of windows j of `ref` with pdist(j) == d under patterns[q], d < n_bins <= 16 -> (n_queries, n_bins) np.uint64.
        patterns: a (Q, 4) np.uint32 array (pattern_from_iupac / pattern_from_2bit) or a list of IUPAC strings of length k."""
        s = _as_u8(ref)
        p = self._patterns(patterns, k)
        return self._hist(self._lib.bitnuc_kmer_pattern_hist, (_ptr(s), s.size, int(k)), p, p.shape[0], n_bins)

    def kmer_pattern_hist_packed(self, words, n_bases, k, patterns, n_bins):
        """kmer_pattern_hist of the packed sequence `words` holding `n_bases` bases, without decoding it."""
        w = _as_u64(words)
        p = self._patterns(patterns, k)
        return self._hist(self._lib.bitnuc_kmer_pattern_hist_packed, (_ptr(w), w.size, int(n_bases), int(k)), p, p.shape[0], n_bins)

    def kmer_pattern_hits(self, ref, k, pattern, tau, with_dist=False):
        """Positions (np.uint64, ascending) of the windows of `ref` with pdist <= tau under the pattern (a (4,) np.uint32 array or an IUPAC string);
        with_dist: (positions, np.uint8 distances)."""
        s = _as_u8(ref)
        p = self._patterns(pattern, k)[:1]
        return self._hits(self._lib.bitnuc_kmer_pattern_hits, (_ptr(s), s.size, int(k), _ptr(p), int(tau)), with_dist)

    def kmer_pattern_hits_packed(self, words, n_bases, k, pattern, tau, with_dist=False):
        """kmer_pattern_hits of the packed sequence `words` holding `n_bases` bases, without decoding it."""
        w = _as_u64(words)
        p = self._patterns(pattern, k)[:1]
        return self._hits(self._lib.bitnuc_kmer_pattern_hits_packed, (_ptr(w), w.size, int(n_bases), int(k), _ptr(p), int(tau)), with_dist)

    # -- analysis on packed words (src/utils/analysis.rs, hamming/scalar.rs) ------------------
    def base_counts(self, words, n_bases):
        """[A, C, G, T] counts of a packed sequence (BaseCount::base_counts, analysis.rs:23-39)."""
        w = _as_u64(words)
        out = np.zeros(4, dtype=np.uint64)
        err = L.BitnucErr()
        if self._lib.bitnuc_base_counts(self._h, _ptr(w), w.size, int(n_bases), _ptr(out), C.byref(err)) != L.OK:
            _raise(err)
        return [int(x) for x in out]

    def gc_content(self, words, n_bases):
        """GCContent::gc_content (analysis.rs:7-16): percent, 0.0 for an empty sequence."""
        if n_bases == 0:
            return 0.0
        c = self.base_counts(words, n_bases)
        return (float(c[1] + c[2]) / float(n_bases)) * 100.0

    def hdist_pairs(self, a, b, length):
        a, b = _as_u64(a), _as_u64(b)
        if a.size != b.size:
            raise ValueError("a and b must hold the same number of words")
        out = np.empty(a.size, dtype=np.uint8)
        err = L.BitnucErr()
        if self._lib.bitnuc_hdist_pairs(self._h, _ptr(a), _ptr(b), a.size, int(length), _ptr(out), C.byref(err)) != L.OK:
            _raise(err)
        return out

    def hdist_query(self, query, targets, length):
        t = _as_u64(targets)
        out = np.empty(t.size, dtype=np.uint8)
        err = L.BitnucErr()
        if self._lib.bitnuc_hdist_query(self._h, C.c_uint64(query), _ptr(t), t.size, int(length), _ptr(out), C.byref(err)) != L.OK:
            _raise(err)
        return out

    def split_packed(self, ebuf, slen, idx, lbuf, rbuf, canonical=False):
        """split_packed(ebuf, slen, idx, &mut lbuf, &mut rbuf) (functions/split.rs:15-99): clears both
        lists, then fills them.  canonical=False reproduces the reference word for word (see
        include/bitnuc_hip.h); canonical=True gives encode(seq[:idx]) / encode(seq[idx:])."""
        e = _as_u64(ebuf)
        flags = L.SPLIT_CANONICAL if canonical else L.SPLIT_AS_WRITTEN
        nl, nr = C.c_size_t(0), C.c_size_t(0)
        err = L.BitnucErr()
        if self._lib.bitnuc_split_packed_sizes(e.size, int(slen), int(idx), flags, C.byref(nl), C.byref(nr), C.byref(err)) != L.OK:
            _raise(err)  # the reference validates before it clears (split.rs:23-32)
        lo, ro = np.empty(nl.value, dtype=np.uint64), np.empty(nr.value, dtype=np.uint64)
        if self._lib.bitnuc_split_packed(self._h, _ptr(e), e.size, int(slen), int(idx), flags, _ptr(lo), C.byref(nl),
                                         _ptr(ro), C.byref(nr), C.byref(err)) != L.OK:
            _raise(err)
        del lbuf[:]
        del rbuf[:]
        lbuf.extend(int(x) for x in lo[: nl.value])
        rbuf.extend(int(x) for x in ro[: nr.value])

    def split_packed_sizes(self, n_words, slen, idx, canonical=False):
        nl, nr = C.c_size_t(0), C.c_size_t(0)
        err = L.BitnucErr()
        if self._lib.bitnuc_split_packed_sizes(int(n_words), int(slen), int(idx), L.SPLIT_CANONICAL if canonical else L.SPLIT_AS_WRITTEN,
                                               C.byref(nl), C.byref(nr), C.byref(err)) != L.OK:
            _raise(err)
        return nl.value, nr.value

    def split_packed_dev(self, d_ebuf, n_words, slen, idx, d_lbuf, d_rbuf, canonical=False):
        self._call_dev(self._lib.bitnuc_split_packed_dev, _dev_ptr(d_ebuf), int(n_words), int(slen), int(idx),
                       L.SPLIT_CANONICAL if canonical else L.SPLIT_AS_WRITTEN, _dev_ptr(d_lbuf), _dev_ptr(d_rbuf))

    def base_counts_dev(self, d_words, n_words, n_bases, d_counts):
        self._call_dev(self._lib.bitnuc_base_counts_dev, _dev_ptr(d_words), int(n_words), int(n_bases), _dev_ptr(d_counts))

    def hdist_pairs_dev(self, d_a, d_b, count, length, d_dist):
        self._call_dev(self._lib.bitnuc_hdist_pairs_dev, _dev_ptr(d_a), _dev_ptr(d_b), int(count), int(length), _dev_ptr(d_dist))

    def hdist_query_dev(self, query, d_targets, count, length, d_dist):
        err = L.BitnucErr()
        if self._lib.bitnuc_hdist_query_dev(self._h, C.c_uint64(query), _dev_ptr(d_targets), int(count), int(length), _dev_ptr(d_dist), C.byref(err)) != L.OK:
            _raise(err)

    # -- ragged batches of independent sequences ---------------------------------------------
    def encode_batch(self, seq, offsets):
        """Encode `count` back-to-back sequences (sequence i = seq[offsets[i]:offsets[i+1]]).
        -> (words ndarray[uint64], word_offsets ndarray[uint64] of count+1 entries)."""
        s = _as_u8(seq)
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        count = off.size - 1
        if count < 0:
            raise ValueError("offsets needs count+1 entries")
        if count and int(off.max()) > s.size:
            raise ValueError("offsets point past the end of seq")
        cap = int((int(off[-1]) - int(off[0])) // 32 + count) if count else 0
        out = np.empty(cap, dtype=np.uint64)
        wo = np.zeros(count + 1, dtype=np.uint64)
        nw = C.c_size_t(0)
        err = L.BitnucErr()
        if self._lib.bitnuc_encode_batch(self._h, _ptr(s), _ptr(off), count, _ptr(out), cap, _ptr(wo), C.byref(nw), C.byref(err)) != L.OK:
            if err.status == L.INVALID_RANGE:
                raise NucleotideError("InvalidRange", index=int(err.value))
            _raise(err)
        return out[: nw.value], wo

    def encode_fixed(self, seq, read_len, stride=None, count=None):
        """Encode `count` reads of `read_len` bases, read r at seq[r*stride:]. -> ndarray[uint64] of
        shape (count, ceil(read_len/32)): row r == encode(read r)."""
        s = _as_u8(seq)
        stride = read_len if stride is None else stride
        if count is None:
            count = 0 if s.size < read_len else (s.size - read_len) // stride + 1
        elif count and (count - 1) * stride + read_len > s.size:
            raise ValueError("seq holds fewer than (count-1)*stride + read_len bytes")
        wpr = (read_len + 31) // 32
        out = np.empty((count, wpr), dtype=np.uint64)
        err = L.BitnucErr()
        if self._lib.bitnuc_encode_fixed(self._h, _ptr(s), int(read_len), int(stride), int(count), _ptr(out), C.byref(err)) != L.OK:
            _raise(err)
        return out

    def decode_fixed(self, words, read_len, stride=None, out=None):
        """Inverse of encode_fixed: -> ndarray[uint8]; read r at [r*stride, r*stride+read_len).
        With stride > read_len pass `out` to keep its separator bytes."""
        w = np.ascontiguousarray(words, dtype=np.uint64)
        wpr = (read_len + 31) // 32
        count = w.size // wpr if wpr else 0
        stride = read_len if stride is None else stride
        nbytes = (count - 1) * stride + read_len if count else 0
        if out is None:
            out = np.zeros(nbytes, dtype=np.uint8)
        elif not (isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.flags.c_contiguous and out.size >= nbytes):
            raise ValueError("out must be a contiguous uint8 array of at least (count-1)*stride + read_len bytes")
        err = L.BitnucErr()
        if self._lib.bitnuc_decode_fixed(self._h, _ptr(w), int(read_len), int(stride), int(count), _ptr(out), C.byref(err)) != L.OK:
            _raise(err)
        return out

    def encode_fixed_dev(self, d_seq, read_len, stride, count, d_out):
        self._call_dev(self._lib.bitnuc_encode_fixed_dev, _dev_ptr(d_seq), int(read_len), int(stride), int(count), _dev_ptr(d_out))

    def decode_fixed_dev(self, d_words, read_len, stride, count, d_out):
        self._call_dev(self._lib.bitnuc_decode_fixed_dev, _dev_ptr(d_words), int(read_len), int(stride), int(count), _dev_ptr(d_out))

    def encode_many(self, seqs):
        """`[encode_alloc(s) for s in seqs]` in one launch: seqs is an iterable of bytes-like
        sequences.  -> list of uint64 arrays (views into one buffer), one per sequence."""
        seqs = [bytes(s) for s in seqs]
        off = np.zeros(len(seqs) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
        words, wo = self.encode_batch(b"".join(seqs), off)
        return [words[int(wo[i]):int(wo[i + 1])] for i in range(len(seqs))]

    def decode_batch(self, words, word_offsets, offsets):
        """Inverse of encode_batch: -> ndarray[uint8] of offsets[-1] bytes, sequence i at
        [offsets[i], offsets[i+1]) (bytes before offsets[0] are zero)."""
        w = _as_u64(words)
        wo = np.ascontiguousarray(word_offsets, dtype=np.uint64)
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        count = off.size - 1
        if count < 0 or wo.size != off.size:
            raise ValueError("offsets and word_offsets need count+1 entries each")
        if w.size < int(wo[-1]):
            raise ValueError("words holds fewer than word_offsets[-1] entries")
        out = np.zeros(int(off[-1]), dtype=np.uint8)
        err = L.BitnucErr()
        if self._lib.bitnuc_decode_batch(self._h, _ptr(w), _ptr(wo), _ptr(off), count, _ptr(out), C.byref(err)) != L.OK:
            if err.status == L.INVALID_RANGE:
                raise NucleotideError("InvalidRange", index=int(err.value))
            _raise(err)
        return out

    def batch_word_offsets_dev(self, d_offsets, count, d_word_offsets):
        total = C.c_size_t(0)
        err = L.BitnucErr()
        if self._lib.bitnuc_batch_word_offsets_dev(self._h, _dev_ptr(d_offsets), int(count), _dev_ptr(d_word_offsets), C.byref(total), C.byref(err)) != L.OK:
            _raise(err)
        return total.value

    def encode_batch_dev(self, d_seq, d_offsets, d_word_offsets, count, total_words, d_out):
        self._call_dev(self._lib.bitnuc_encode_batch_dev, _dev_ptr(d_seq), _dev_ptr(d_offsets), _dev_ptr(d_word_offsets), int(count), int(total_words), _dev_ptr(d_out))

    def decode_batch_dev(self, d_words, d_word_offsets, d_offsets, count, total_words, d_out):
        self._call_dev(self._lib.bitnuc_decode_batch_dev, _dev_ptr(d_words), _dev_ptr(d_word_offsets), _dev_ptr(d_offsets), int(count), int(total_words), _dev_ptr(d_out))

    # -- device-pointer API (async; data errors surface at sync()) -----------------------
    def _call_dev(self, fn, *args):
        err = L.BitnucErr()
        if fn(self._h, *args, C.byref(err)) != L.OK:
            _raise(err)

    def encode_dev(self, d_seq, length, d_out):
        self._call_dev(self._lib.bitnuc_encode_dev, _dev_ptr(d_seq), int(length), _dev_ptr(d_out))

    def decode_dev(self, d_ebuf, n_words, n_bases, d_out):
        self._call_dev(self._lib.bitnuc_decode_dev, _dev_ptr(d_ebuf), int(n_words), int(n_bases), _dev_ptr(d_out))

    def as_2bit_batch_dev(self, d_kmers, k, stride, count, d_out):
        self._call_dev(self._lib.bitnuc_as_2bit_batch_dev, _dev_ptr(d_kmers), int(k), int(stride), int(count), _dev_ptr(d_out))

    def kmer_hdist_scan_dev(self, d_ref, n, k, query, d_dist):
        self._call_dev(self._lib.bitnuc_kmer_hdist_scan_dev, _dev_ptr(d_ref), int(n), int(k), C.c_uint64(query), _dev_ptr(d_dist))

    def kmer_hdist_count_dev(self, d_ref, n, k, query, tau, d_count):
        """Number of windows with Hamming distance <= tau to the query (fused scan, no distance bytes written) -> *d_count (u64)."""
        self._call_dev(self._lib.bitnuc_kmer_hdist_count_dev, _dev_ptr(d_ref), int(n), int(k), C.c_uint64(query), int(tau), _dev_ptr(d_count))

    def kmer_hdist_scan_packed_dev(self, d_words, n_words, n, k, query, d_dist):
        """The scan on packed words in device memory (8-byte aligned) -> n - k + 1 distance bytes at d_dist (any byte offset)."""
        self._call_dev(self._lib.bitnuc_kmer_hdist_scan_packed_dev, _dev_ptr(d_words), int(n_words), int(n), int(k), C.c_uint64(query), _dev_ptr(d_dist))

    def kmer_hdist_count_packed_dev(self, d_words, n_words, n, k, query, tau, d_count):
        """The fused count on packed words in device memory -> *d_count (u64)."""
        self._call_dev(self._lib.bitnuc_kmer_hdist_count_packed_dev, _dev_ptr(d_words), int(n_words), int(n), int(k), C.c_uint64(query), int(tau), _dev_ptr(d_count))

    def kmer_hdist_hits_dev(self, d_ref, n, k, query, tau, d_pos, d_hit_dist, cap, d_n_hits):
        """The positions of the windows with distance <= tau -> d_pos[0 .. min(cap, total)) (u64, ascending), their distances at d_hit_dist (None: not
        written), total -> *d_n_hits (u64)."""
        self._call_dev(self._lib.bitnuc_kmer_hdist_hits_dev, _dev_ptr(d_ref), int(n), int(k), C.c_uint64(query), int(tau), _dev_ptr(d_pos),
                       _dev_ptr(d_hit_dist), int(cap), _dev_ptr(d_n_hits))

    def kmer_hdist_hits_packed_dev(self, d_words, n_words, n, k, query, tau, d_pos, d_hit_dist, cap, d_n_hits):
        """The hit list on packed words in device memory (8-byte aligned)."""
        self._call_dev(self._lib.bitnuc_kmer_hdist_hits_packed_dev, _dev_ptr(d_words), int(n_words), int(n), int(k), C.c_uint64(query), int(tau),
                       _dev_ptr(d_pos), _dev_ptr(d_hit_dist), int(cap), _dev_ptr(d_n_hits))

    def kmer_hdist_count_multi_dev(self, d_ref, n, k, d_queries, d_taus, n_queries, d_counts):
        """The fused count for n_queries queries at once: d_counts[q] (u64) = windows with distance <= d_taus[q] (u32) to d_queries[q] (u64)."""
        self._call_dev(self._lib.bitnuc_kmer_hdist_count_multi_dev, _dev_ptr(d_ref), int(n), int(k), _dev_ptr(d_queries), _dev_ptr(d_taus), int(n_queries),
                       _dev_ptr(d_counts))

    def kmer_hdist_count_multi_packed_dev(self, d_words, n_words, n, k, d_queries, d_taus, n_queries, d_counts):
        """The multi-query count on packed words in device memory (8-byte aligned)."""
        self._call_dev(self._lib.bitnuc_kmer_hdist_count_multi_packed_dev, _dev_ptr(d_words), int(n_words), int(n), int(k), _dev_ptr(d_queries),
                       _dev_ptr(d_taus), int(n_queries), _dev_ptr(d_counts))

    def kmer_hdist_best_async(self, d_ref, n, k, d_queries, n_queries, d_pos, d_dist):
        """The best match of n_queries queries at once: d_dist[q] (u8) = the smallest distance of a window to d_queries[q] (u64), d_pos[q] (u64) = the
        leftmost window that attains it.  Asynchronous on the context's stream, as the _dev calls."""
        self._call_dev(self._lib.bitnuc_kmer_hdist_best_async, _dev_ptr(d_ref), int(n), int(k), _dev_ptr(d_queries), int(n_queries), _dev_ptr(d_pos),
                       _dev_ptr(d_dist))

    def kmer_hdist_best_packed_async(self, d_words, n_words, n, k, d_queries, n_queries, d_pos, d_dist):
        """The best match per query on packed words in device memory (8-byte aligned)."""
        self._call_dev(self._lib.bitnuc_kmer_hdist_best_packed_async, _dev_ptr(d_words), int(n_words), int(n), int(k), _dev_ptr(d_queries), int(n_queries),
                       _dev_ptr(d_pos), _dev_ptr(d_dist))

    def reads_hdist_best_async(self, d_reads, read_len, count, k, d_queries, n_queries, d_best_query, d_best_pos, d_best_dist):
        """The best match per read of `count` back-to-back ASCII reads in device memory: d_best_query[r], d_best_pos[r] (u32), d_best_dist[r] (u8) =
        the smallest (distance, query, offset) over the windows inside read r.  Asynchronous on the context's stream, as the _dev calls."""
        self._call_dev(self._lib.bitnuc_reads_hdist_best_async, _dev_ptr(d_reads), int(read_len), int(count), int(k), _dev_ptr(d_queries), int(n_queries),
                       _dev_ptr(d_best_query), _dev_ptr(d_best_pos), _dev_ptr(d_best_dist))

    def reads_hdist_best_packed_async(self, d_words, read_len, count, k, d_queries, n_queries, d_best_query, d_best_pos, d_best_dist):
        """The best match per read on the packed words encode_fixed_dev writes (8-byte aligned, ceil(read_len / 32) words per read)."""
        self._call_dev(self._lib.bitnuc_reads_hdist_best_packed_async, _dev_ptr(d_words), int(read_len), int(count), int(k), _dev_ptr(d_queries),
                       int(n_queries), _dev_ptr(d_best_query), _dev_ptr(d_best_pos), _dev_ptr(d_best_dist))

    def reads_hdist_best2_async(self, d_reads, read_len, count, k, d_queries, n_queries, d_best_query, d_best_pos, d_best_dist, d_second_query, d_second_pos,
                                d_second_dist):
        """reads_hdist_best_async with the runner-up: d_second_query[r], d_second_pos[r] (u32), d_second_dist[r] (u8) = the smallest (distance, query,
        offset) over the queries other than d_best_query[r].  Asynchronous on the context's stream, as the _dev calls."""
        self._call_dev(self._lib.bitnuc_reads_hdist_best2_async, _dev_ptr(d_reads), int(read_len), int(count), int(k), _dev_ptr(d_queries), int(n_queries),
                       _dev_ptr(d_best_query), _dev_ptr(d_best_pos), _dev_ptr(d_best_dist), _dev_ptr(d_second_query), _dev_ptr(d_second_pos), _dev_ptr(d_second_dist))

    def reads_hdist_best2_packed_async(self, d_words, read_len, count, k, d_queries, n_queries, d_best_query, d_best_pos, d_best_dist, d_second_query, d_second_pos,
                                       d_second_dist):
        """The best match and the runner-up per read on the packed words encode_fixed_dev writes (8-byte aligned, ceil(read_len / 32) words per read)."""
        self._call_dev(self._lib.bitnuc_reads_hdist_best2_packed_async, _dev_ptr(d_words), int(read_len), int(count), int(k), _dev_ptr(d_queries), int(n_queries),
                       _dev_ptr(d_best_query), _dev_ptr(d_best_pos), _dev_ptr(d_best_dist), _dev_ptr(d_second_query), _dev_ptr(d_second_pos), _dev_ptr(d_second_dist))

    def reads_hdist_anchored_async(self, d_reads, read_len, count, k, d_queries, n_queries, d_best_query, d_best_pos, d_best_dist, d_second_query=None,
                                   d_second_pos=None, d_second_dist=None, pos_lo=0, pos_hi=None):
        """reads_hdist_best2_async over the offsets pos_lo <= i <= min(pos_hi, read_len - k) of every read only (pos_hi None: to the end of the read; a span
        of at most 64 bases); the three d_second_* all None: the best triple only.  Asynchronous on the context's stream, as the _dev calls."""
        self._call_dev(self._lib.bitnuc_reads_hdist_anchored_async, _dev_ptr(d_reads), int(read_len), int(count), int(k), int(pos_lo),
                       _SIZE_MAX if pos_hi is None else int(pos_hi), _dev_ptr(d_queries), int(n_queries), _dev_ptr(d_best_query), _dev_ptr(d_best_pos),
                       _dev_ptr(d_best_dist), *(_dev_ptr(a) for a in (d_second_query, d_second_pos, d_second_dist)))

    def reads_hdist_anchored_packed_async(self, d_words, read_len, count, k, d_queries, n_queries, d_best_query, d_best_pos, d_best_dist, d_second_query=None,
                                          d_second_pos=None, d_second_dist=None, pos_lo=0, pos_hi=None):
        """reads_hdist_anchored_async on the packed words encode_fixed_dev writes (8-byte aligned, ceil(read_len / 32) words per read)."""
        self._call_dev(self._lib.bitnuc_reads_hdist_anchored_packed_async, _dev_ptr(d_words), int(read_len), int(count), int(k), int(pos_lo),
                       _SIZE_MAX if pos_hi is None else int(pos_hi), _dev_ptr(d_queries), int(n_queries), _dev_ptr(d_best_query), _dev_ptr(d_best_pos),
                       _dev_ptr(d_best_dist), *(_dev_ptr(a) for a in (d_second_query, d_second_pos, d_second_dist)))

    def reads_hdist_anchored_batch_async(self, d_seq, d_offsets, count, total_bases, k, d_queries, n_queries, d_best_query, d_best_pos, d_best_dist,
                                         d_second_query=None, d_second_pos=None, d_second_dist=None, pos_lo=0, pos_hi=0, anchor="start"):
        """reads_hdist_anchored_async of a ragged batch in device memory: read r is d_seq[d_offsets[r] .. d_offsets[r + 1]) (u64, count + 1 entries from 0,
        total_bases = the last; trusted, read on the device).  anchor "start" / "end": the range pos_lo .. pos_hi counts offsets from the read's start, or
        bases behind the window from its end; pos_hi - pos_lo + k <= 64.  The three d_second_* all None: the best triple only."""
        self._call_dev(self._lib.bitnuc_reads_hdist_anchored_batch_async, _dev_ptr(d_seq), _dev_ptr(d_offsets), int(count), int(total_bases), int(k),
                       self._anchor(anchor), int(pos_lo), int(pos_hi), _dev_ptr(d_queries), int(n_queries), _dev_ptr(d_best_query), _dev_ptr(d_best_pos),
                       _dev_ptr(d_best_dist), *(_dev_ptr(a) for a in (d_second_query, d_second_pos, d_second_dist)))

    def reads_hdist_anchored_batch_packed_async(self, d_words, d_word_offsets, d_offsets, count, total_words, k, d_queries, n_queries, d_best_query, d_best_pos,
                                                d_best_dist, d_second_query=None, d_second_pos=None, d_second_dist=None, pos_lo=0, pos_hi=0, anchor="start"):
        """reads_hdist_anchored_batch_async on the packed words encode_batch_dev writes (8-byte aligned; both tables u64 in device memory, trusted)."""
        self._call_dev(self._lib.bitnuc_reads_hdist_anchored_batch_packed_async, _dev_ptr(d_words), _dev_ptr(d_word_offsets), _dev_ptr(d_offsets), int(count),
                       int(total_words), int(k), self._anchor(anchor), int(pos_lo), int(pos_hi), _dev_ptr(d_queries), int(n_queries), _dev_ptr(d_best_query),
                       _dev_ptr(d_best_pos), _dev_ptr(d_best_dist), *(_dev_ptr(a) for a in (d_second_query, d_second_pos, d_second_dist)))

    def reads_hdist_best_batch_async(self, d_seq, d_offsets, count, total_bases, k, d_queries, n_queries, d_best_query, d_best_pos, d_best_dist):
        """The best match per read of a ragged batch of ASCII reads in device memory: read r is d_seq[d_offsets[r] .. d_offsets[r + 1]) (u64, count + 1
        entries from 0, total_bases = the last).  The table is trusted and read on the device.  Asynchronous on the context's stream, as the _dev calls."""
        self._call_dev(self._lib.bitnuc_reads_hdist_best_batch_async, _dev_ptr(d_seq), _dev_ptr(d_offsets), int(count), int(total_bases), int(k),
                       _dev_ptr(d_queries), int(n_queries), _dev_ptr(d_best_query), _dev_ptr(d_best_pos), _dev_ptr(d_best_dist))

    def reads_hdist_best_batch_packed_async(self, d_words, d_word_offsets, d_offsets, count, total_words, k, d_queries, n_queries, d_best_query, d_best_pos,
                                            d_best_dist):
        """The best match per read on the packed words encode_batch_dev writes (8-byte aligned; both tables u64 in device memory, trusted)."""
        self._call_dev(self._lib.bitnuc_reads_hdist_best_batch_packed_async, _dev_ptr(d_words), _dev_ptr(d_word_offsets), _dev_ptr(d_offsets), int(count),
                       int(total_words), int(k), _dev_ptr(d_queries), int(n_queries), _dev_ptr(d_best_query), _dev_ptr(d_best_pos), _dev_ptr(d_best_dist))

    # the per-read matchers' pattern twins: the reads_hdist_*_async methods with d_patterns (n_queries bitnuc_pattern, 16 bytes each, 4-byte aligned,
    # device memory) where d_queries stood
    def reads_pattern_best_async(self, d_reads, read_len, count, k, d_patterns, n_queries, d_best_query, d_best_pos, d_best_dist):
        """reads_hdist_best_async under pattern queries."""
        self._call_dev(self._lib.bitnuc_reads_pattern_best_async, _dev_ptr(d_reads), int(read_len), int(count), int(k), _dev_ptr(d_patterns), int(n_queries),
                       _dev_ptr(d_best_query), _dev_ptr(d_best_pos), _dev_ptr(d_best_dist))

    def reads_pattern_best_packed_async(self, d_words, read_len, count, k, d_patterns, n_queries, d_best_query, d_best_pos, d_best_dist):
        """reads_hdist_best_packed_async under pattern queries."""
        self._call_dev(self._lib.bitnuc_reads_pattern_best_packed_async, _dev_ptr(d_words), int(read_len), int(count), int(k), _dev_ptr(d_patterns),
                       int(n_queries), _dev_ptr(d_best_query), _dev_ptr(d_best_pos), _dev_ptr(d_best_dist))

    def reads_pattern_best2_async(self, d_reads, read_len, count, k, d_patterns, n_queries, d_best_query, d_best_pos, d_best_dist, d_second_query, d_second_pos,
                                  d_second_dist):
        """reads_hdist_best2_async under pattern queries."""
        self._call_dev(self._lib.bitnuc_reads_pattern_best2_async, _dev_ptr(d_reads), int(read_len), int(count), int(k), _dev_ptr(d_patterns), int(n_queries),
                       _dev_ptr(d_best_query), _dev_ptr(d_best_pos), _dev_ptr(d_best_dist), _dev_ptr(d_second_query), _dev_ptr(d_second_pos), _dev_ptr(d_second_dist))

    def reads_pattern_best2_packed_async(self, d_words, read_len, count, k, d_patterns, n_queries, d_best_query, d_best_pos, d_best_dist, d_second_query,
                                         d_second_pos, d_second_dist):
        """reads_hdist_best2_packed_async under pattern queries."""
        self._call_dev(self._lib.bitnuc_reads_pattern_best2_packed_async, _dev_ptr(d_words), int(read_len), int(count), int(k), _dev_ptr(d_patterns), int(n_queries),
                       _dev_ptr(d_best_query), _dev_ptr(d_best_pos), _dev_ptr(d_best_dist), _dev_ptr(d_second_query), _dev_ptr(d_second_pos), _dev_ptr(d_second_dist))

    def reads_pattern_anchored_async(self, d_reads, read_len, count, k, d_patterns, n_queries, d_best_query, d_best_pos, d_best_dist, d_second_query=None,
                                     d_second_pos=None, d_second_dist=None, pos_lo=0, pos_hi=None):
        """reads_hdist_anchored_async under pattern queries."""
        self._call_dev(self._lib.bitnuc_reads_pattern_anchored_async, _dev_ptr(d_reads), int(read_len), int(count), int(k), int(pos_lo),
                       _SIZE_MAX if pos_hi is None else int(pos_hi), _dev_ptr(d_patterns), int(n_queries), _dev_ptr(d_best_query), _dev_ptr(d_best_pos),
                       _dev_ptr(d_best_dist), *(_dev_ptr(a) for a in (d_second_query, d_second_pos, d_second_dist)))

    def reads_pattern_anchored_packed_async(self, d_words, read_len, count, k, d_patterns, n_queries, d_best_query, d_best_pos, d_best_dist, d_second_query=None,
                                            d_second_pos=None, d_second_dist=None, pos_lo=0, pos_hi=None):
        """reads_hdist_anchored_packed_async under pattern queries."""
        self._call_dev(self._lib.bitnuc_reads_pattern_anchored_packed_async, _dev_ptr(d_words), int(read_len), int(count), int(k), int(pos_lo),
                       _SIZE_MAX if pos_hi is None else int(pos_hi), _dev_ptr(d_patterns), int(n_queries), _dev_ptr(d_best_query), _dev_ptr(d_best_pos),
                       _dev_ptr(d_best_dist), *(_dev_ptr(a) for a in (d_second_query, d_second_pos, d_second_dist)))

    def _reads_edist_async(self, fn, d_data, read_len, count, k, d_queries, n_queries, d_best, d_second, pos_lo, pos_hi):
        self._call_dev(fn, _dev_ptr(d_data), int(read_len), int(count), int(k), int(pos_lo), _SIZE_MAX if pos_hi is None else int(pos_hi), _dev_ptr(d_queries),
                       int(n_queries), *(_dev_ptr(a) for a in d_best), *(_dev_ptr(a) for a in d_second))

    def reads_edist_anchored_async(self, d_reads, read_len, count, k, d_queries, n_queries, d_best_query, d_best_end, d_best_dist, d_second_query=None,
                                   d_second_end=None, d_second_dist=None, pos_lo=0, pos_hi=None):
        """reads_edist_anchored on device tensors, asynchronous on the context's stream (d_second_*: all three or none); an invalid span byte is
        reported by the next sync()."""
        self._reads_edist_async(self._lib.bitnuc_reads_edist_anchored_async, d_reads, read_len, count, k, d_queries, n_queries,
                                (d_best_query, d_best_end, d_best_dist), (d_second_query, d_second_end, d_second_dist), pos_lo, pos_hi)

    def reads_edist_anchored_packed_async(self, d_words, read_len, count, k, d_queries, n_queries, d_best_query, d_best_end, d_best_dist, d_second_query=None,
                                          d_second_end=None, d_second_dist=None, pos_lo=0, pos_hi=None):
        """reads_edist_anchored_async of packed words (ceil(read_len / 32) per read)."""
        self._reads_edist_async(self._lib.bitnuc_reads_edist_anchored_packed_async, d_words, read_len, count, k, d_queries, n_queries,
                                (d_best_query, d_best_end, d_best_dist), (d_second_query, d_second_end, d_second_dist), pos_lo, pos_hi)

    def reads_pattern_edist_anchored_async(self, d_reads, read_len, count, k, d_patterns, n_queries, d_best_query, d_best_end, d_best_dist, d_second_query=None,
                                           d_second_end=None, d_second_dist=None, pos_lo=0, pos_hi=None):
        """reads_edist_anchored_async under pattern queries."""
        self._reads_edist_async(self._lib.bitnuc_reads_pattern_edist_anchored_async, d_reads, read_len, count, k, d_patterns, n_queries,
                                (d_best_query, d_best_end, d_best_dist), (d_second_query, d_second_end, d_second_dist), pos_lo, pos_hi)

    def reads_pattern_edist_anchored_packed_async(self, d_words, read_len, count, k, d_patterns, n_queries, d_best_query, d_best_end, d_best_dist,
                                                  d_second_query=None, d_second_end=None, d_second_dist=None, pos_lo=0, pos_hi=None):
        """reads_edist_anchored_packed_async under pattern queries."""
        self._reads_edist_async(self._lib.bitnuc_reads_pattern_edist_anchored_packed_async, d_words, read_len, count, k, d_patterns, n_queries,
                                (d_best_query, d_best_end, d_best_dist), (d_second_query, d_second_end, d_second_dist), pos_lo, pos_hi)

    def _reads_edist_batch_async(self, fn, head, k, d_queries, n_queries, d_best, d_second, pos_lo, pos_hi, anchor):
        self._call_dev(fn, *head, int(k), self._anchor(anchor), int(pos_lo), int(pos_hi), _dev_ptr(d_queries), int(n_queries), *(_dev_ptr(a) for a in d_best),
                       *(_dev_ptr(a) for a in d_second))

    def reads_edist_anchored_batch_async(self, d_seq, d_offsets, count, total_bases, k, d_queries, n_queries, d_best_query, d_best_end, d_best_dist,
                                         d_second_query=None, d_second_end=None, d_second_dist=None, pos_lo=0, pos_hi=0, anchor="start"):
        """reads_edist_anchored_batch on device tensors (the arguments of reads_hdist_anchored_batch_async, ends where positions stood), asynchronous on
        the context's stream; the table is trusted and read on the device; an invalid span byte is reported by the next sync()."""
        self._reads_edist_batch_async(self._lib.bitnuc_reads_edist_anchored_batch_async, (_dev_ptr(d_seq), _dev_ptr(d_offsets), int(count), int(total_bases)), k,
                                      d_queries, n_queries, (d_best_query, d_best_end, d_best_dist), (d_second_query, d_second_end, d_second_dist), pos_lo, pos_hi,
                                      anchor)

    def reads_edist_anchored_batch_packed_async(self, d_words, d_word_offsets, d_offsets, count, total_words, k, d_queries, n_queries, d_best_query, d_best_end,
                                                d_best_dist, d_second_query=None, d_second_end=None, d_second_dist=None, pos_lo=0, pos_hi=0, anchor="start"):
        """reads_edist_anchored_batch_async on the packed words encode_batch_dev writes (8-byte aligned; both tables u64 in device memory, trusted)."""
        self._reads_edist_batch_async(self._lib.bitnuc_reads_edist_anchored_batch_packed_async,
                                      (_dev_ptr(d_words), _dev_ptr(d_word_offsets), _dev_ptr(d_offsets), int(count), int(total_words)), k, d_queries, n_queries,
                                      (d_best_query, d_best_end, d_best_dist), (d_second_query, d_second_end, d_second_dist), pos_lo, pos_hi, anchor)

    def reads_pattern_edist_anchored_batch_async(self, d_seq, d_offsets, count, total_bases, k, d_patterns, n_queries, d_best_query, d_best_end, d_best_dist,
                                                 d_second_query=None, d_second_end=None, d_second_dist=None, pos_lo=0, pos_hi=0, anchor="start"):
        """reads_edist_anchored_batch_async under pattern queries."""
        self._reads_edist_batch_async(self._lib.bitnuc_reads_pattern_edist_anchored_batch_async, (_dev_ptr(d_seq), _dev_ptr(d_offsets), int(count), int(total_bases)),
                                      k, d_patterns, n_queries, (d_best_query, d_best_end, d_best_dist), (d_second_query, d_second_end, d_second_dist), pos_lo,
                                      pos_hi, anchor)

    def reads_pattern_edist_anchored_batch_packed_async(self, d_words, d_word_offsets, d_offsets, count, total_words, k, d_patterns, n_queries, d_best_query,
                                                        d_best_end, d_best_dist, d_second_query=None, d_second_end=None, d_second_dist=None, pos_lo=0, pos_hi=0,
                                                        anchor="start"):
        """reads_edist_anchored_batch_packed_async under pattern queries."""
        self._reads_edist_batch_async(self._lib.bitnuc_reads_pattern_edist_anchored_batch_packed_async,
                                      (_dev_ptr(d_words), _dev_ptr(d_word_offsets), _dev_ptr(d_offsets), int(count), int(total_words)), k, d_patterns, n_queries,
                                      (d_best_query, d_best_end, d_best_dist), (d_second_query, d_second_end, d_second_dist), pos_lo, pos_hi, anchor)

    def _reads_adapter_async(self, fn, head, k, d_queries, n_queries, min_overlap, rate, d_out):
        self._call_dev(fn, *head, int(k), _dev_ptr(d_queries), int(n_queries), int(min_overlap), int(rate[0]), int(rate[1]), *(_dev_ptr(a) for a in d_out))

    def reads_edist_adapter_async(self, d_reads, read_len, count, k, d_queries, n_queries, d_adapter, d_cut, d_end, d_overlap, d_dist, min_overlap=3,
                                  err_num=1, err_den=10):
        """reads_edist_adapter on device tensors, asynchronous on the context's stream (five outputs, all required); an invalid byte is reported by
        the next sync()."""
        self._reads_adapter_async(self._lib.bitnuc_reads_edist_adapter_async, (_dev_ptr(d_reads), int(read_len), int(count)), k, d_queries, n_queries,
                                  min_overlap, (err_num, err_den), (d_adapter, d_cut, d_end, d_overlap, d_dist))

    def reads_edist_adapter_packed_async(self, d_words, read_len, count, k, d_queries, n_queries, d_adapter, d_cut, d_end, d_overlap, d_dist, min_overlap=3,
                                         err_num=1, err_den=10):
        """reads_edist_adapter_async of packed words (ceil(read_len / 32) per read)."""
        self._reads_adapter_async(self._lib.bitnuc_reads_edist_adapter_packed_async, (_dev_ptr(d_words), int(read_len), int(count)), k, d_queries, n_queries,
                                  min_overlap, (err_num, err_den), (d_adapter, d_cut, d_end, d_overlap, d_dist))

    def reads_pattern_edist_adapter_async(self, d_reads, read_len, count, k, d_patterns, n_queries, d_adapter, d_cut, d_end, d_overlap, d_dist, min_overlap=3,
                                          err_num=1, err_den=10):
        """reads_edist_adapter_async under pattern queries."""
        self._reads_adapter_async(self._lib.bitnuc_reads_pattern_edist_adapter_async, (_dev_ptr(d_reads), int(read_len), int(count)), k, d_patterns, n_queries,
                                  min_overlap, (err_num, err_den), (d_adapter, d_cut, d_end, d_overlap, d_dist))

    def reads_pattern_edist_adapter_packed_async(self, d_words, read_len, count, k, d_patterns, n_queries, d_adapter, d_cut, d_end, d_overlap, d_dist,
                                                 min_overlap=3, err_num=1, err_den=10):
        """reads_edist_adapter_packed_async under pattern queries."""
        self._reads_adapter_async(self._lib.bitnuc_reads_pattern_edist_adapter_packed_async, (_dev_ptr(d_words), int(read_len), int(count)), k, d_patterns,
                                  n_queries, min_overlap, (err_num, err_den), (d_adapter, d_cut, d_end, d_overlap, d_dist))

    def reads_edist_adapter_batch_async(self, d_seq, d_offsets, count, total_bases, k, d_queries, n_queries, d_adapter, d_cut, d_end, d_overlap, d_dist,
                                        min_overlap=3, err_num=1, err_den=10):
        """reads_edist_adapter_batch on device tensors (the layout arguments of reads_edist_best_batch_async), asynchronous on the context's stream; the
        table is trusted and read on the device; an invalid byte is reported by the next sync()."""
        self._reads_adapter_async(self._lib.bitnuc_reads_edist_adapter_batch_async, (_dev_ptr(d_seq), _dev_ptr(d_offsets), int(count), int(total_bases)), k,
                                  d_queries, n_queries, min_overlap, (err_num, err_den), (d_adapter, d_cut, d_end, d_overlap, d_dist))

    def reads_edist_adapter_batch_packed_async(self, d_words, d_word_offsets, d_offsets, count, total_words, k, d_queries, n_queries, d_adapter, d_cut, d_end,
                                               d_overlap, d_dist, min_overlap=3, err_num=1, err_den=10):
        """reads_edist_adapter_batch_async on the packed words encode_batch_dev writes (8-byte aligned; both tables u64 in device memory, trusted)."""
        self._reads_adapter_async(self._lib.bitnuc_reads_edist_adapter_batch_packed_async,
                                  (_dev_ptr(d_words), _dev_ptr(d_word_offsets), _dev_ptr(d_offsets), int(count), int(total_words)), k, d_queries, n_queries,
                                  min_overlap, (err_num, err_den), (d_adapter, d_cut, d_end, d_overlap, d_dist))

    def reads_pattern_edist_adapter_batch_async(self, d_seq, d_offsets, count, total_bases, k, d_patterns, n_queries, d_adapter, d_cut, d_end, d_overlap,
                                                d_dist, min_overlap=3, err_num=1, err_den=10):
        """reads_edist_adapter_batch_async under pattern queries."""
        self._reads_adapter_async(self._lib.bitnuc_reads_pattern_edist_adapter_batch_async, (_dev_ptr(d_seq), _dev_ptr(d_offsets), int(count), int(total_bases)),
                                  k, d_patterns, n_queries, min_overlap, (err_num, err_den), (d_adapter, d_cut, d_end, d_overlap, d_dist))

    def reads_pattern_edist_adapter_batch_packed_async(self, d_words, d_word_offsets, d_offsets, count, total_words, k, d_patterns, n_queries, d_adapter, d_cut,
                                                       d_end, d_overlap, d_dist, min_overlap=3, err_num=1, err_den=10):
        """reads_edist_adapter_batch_packed_async under pattern queries."""
        self._reads_adapter_async(self._lib.bitnuc_reads_pattern_edist_adapter_batch_packed_async,
                                  (_dev_ptr(d_words), _dev_ptr(d_word_offsets), _dev_ptr(d_offsets), int(count), int(total_words)), k, d_patterns, n_queries,
                                  min_overlap, (err_num, err_den), (d_adapter, d_cut, d_end, d_overlap, d_dist))

    def _reads_edist_best_async(self, fn, head, k, d_queries, n_queries, d_best, d_second):
        self._call_dev(fn, *head, int(k), _dev_ptr(d_queries), int(n_queries), *(_dev_ptr(a) for a in d_best), *(_dev_ptr(a) for a in d_second))

    def reads_edist_best_async(self, d_reads, read_len, count, k, d_queries, n_queries, d_best_query, d_best_end, d_best_dist, d_second_query=None,
                               d_second_end=None, d_second_dist=None):
        """reads_edist_best on device tensors, asynchronous on the context's stream (d_second_*: all three or none); an invalid byte is reported by the
        next sync()."""
        self._reads_edist_best_async(self._lib.bitnuc_reads_edist_best_async, (_dev_ptr(d_reads), int(read_len), int(count)), k, d_queries, n_queries,
                                     (d_best_query, d_best_end, d_best_dist), (d_second_query, d_second_end, d_second_dist))

    def reads_edist_best_packed_async(self, d_words, read_len, count, k, d_queries, n_queries, d_best_query, d_best_end, d_best_dist, d_second_query=None,
                                      d_second_end=None, d_second_dist=None):
        """reads_edist_best_async of packed words (ceil(read_len / 32) per read)."""
        self._reads_edist_best_async(self._lib.bitnuc_reads_edist_best_packed_async, (_dev_ptr(d_words), int(read_len), int(count)), k, d_queries, n_queries,
                                     (d_best_query, d_best_end, d_best_dist), (d_second_query, d_second_end, d_second_dist))

    def reads_pattern_edist_best_async(self, d_reads, read_len, count, k, d_patterns, n_queries, d_best_query, d_best_end, d_best_dist, d_second_query=None,
                                       d_second_end=None, d_second_dist=None):
        """reads_edist_best_async under pattern queries."""
        self._reads_edist_best_async(self._lib.bitnuc_reads_pattern_edist_best_async, (_dev_ptr(d_reads), int(read_len), int(count)), k, d_patterns, n_queries,
                                     (d_best_query, d_best_end, d_best_dist), (d_second_query, d_second_end, d_second_dist))

    def reads_pattern_edist_best_packed_async(self, d_words, read_len, count, k, d_patterns, n_queries, d_best_query, d_best_end, d_best_dist,
                                              d_second_query=None, d_second_end=None, d_second_dist=None):
        """reads_edist_best_packed_async under pattern queries."""
        self._reads_edist_best_async(self._lib.bitnuc_reads_pattern_edist_best_packed_async, (_dev_ptr(d_words), int(read_len), int(count)), k, d_patterns,
                                     n_queries, (d_best_query, d_best_end, d_best_dist), (d_second_query, d_second_end, d_second_dist))

    def reads_edist_best_batch_async(self, d_seq, d_offsets, count, total_bases, k, d_queries, n_queries, d_best_query, d_best_end, d_best_dist,
                                     d_second_query=None, d_second_end=None, d_second_dist=None):
        """reads_edist_best_batch on device tensors (the arguments of reads_hdist_best_batch_async and six outputs), asynchronous on the context's stream;
        the table is trusted and read on the device; an invalid byte is reported by the next sync()."""
        self._reads_edist_best_async(self._lib.bitnuc_reads_edist_best_batch_async, (_dev_ptr(d_seq), _dev_ptr(d_offsets), int(count), int(total_bases)), k,
                                     d_queries, n_queries, (d_best_query, d_best_end, d_best_dist), (d_second_query, d_second_end, d_second_dist))

    def reads_edist_best_batch_packed_async(self, d_words, d_word_offsets, d_offsets, count, total_words, k, d_queries, n_queries, d_best_query, d_best_end,
                                            d_best_dist, d_second_query=None, d_second_end=None, d_second_dist=None):
        """reads_edist_best_batch_async on the packed words encode_batch_dev writes (8-byte aligned; both tables u64 in device memory, trusted)."""
        self._reads_edist_best_async(self._lib.bitnuc_reads_edist_best_batch_packed_async,
                                     (_dev_ptr(d_words), _dev_ptr(d_word_offsets), _dev_ptr(d_offsets), int(count), int(total_words)), k, d_queries, n_queries,
                                     (d_best_query, d_best_end, d_best_dist), (d_second_query, d_second_end, d_second_dist))

    def reads_pattern_edist_best_batch_async(self, d_seq, d_offsets, count, total_bases, k, d_patterns, n_queries, d_best_query, d_best_end, d_best_dist,
                                             d_second_query=None, d_second_end=None, d_second_dist=None):
        """reads_edist_best_batch_async under pattern queries."""
        self._reads_edist_best_async(self._lib.bitnuc_reads_pattern_edist_best_batch_async, (_dev_ptr(d_seq), _dev_ptr(d_offsets), int(count), int(total_bases)), k,
                                     d_patterns, n_queries, (d_best_query, d_best_end, d_best_dist), (d_second_query, d_second_end, d_second_dist))

    def reads_pattern_edist_best_batch_packed_async(self, d_words, d_word_offsets, d_offsets, count, total_words, k, d_patterns, n_queries, d_best_query,
                                                    d_best_end, d_best_dist, d_second_query=None, d_second_end=None, d_second_dist=None):
        """reads_edist_best_batch_packed_async under pattern queries."""
        self._reads_edist_best_async(self._lib.bitnuc_reads_pattern_edist_best_batch_packed_async,
                                     (_dev_ptr(d_words), _dev_ptr(d_word_offsets), _dev_ptr(d_offsets), int(count), int(total_words)), k, d_patterns, n_queries,
                                     (d_best_query, d_best_end, d_best_dist), (d_second_query, d_second_end, d_second_dist))

    def reads_pattern_anchored_batch_async(self, d_seq, d_offsets, count, total_bases, k, d_patterns, n_queries, d_best_query, d_best_pos, d_best_dist,
                                           d_second_query=None, d_second_pos=None, d_second_dist=None, pos_lo=0, pos_hi=0, anchor="start"):
        """reads_hdist_anchored_batch_async under pattern queries."""
        self._call_dev(self._lib.bitnuc_reads_pattern_anchored_batch_async, _dev_ptr(d_seq), _dev_ptr(d_offsets), int(count), int(total_bases), int(k),
                       self._anchor(anchor), int(pos_lo), int(pos_hi), _dev_ptr(d_patterns), int(n_queries), _dev_ptr(d_best_query), _dev_ptr(d_best_pos),
                       _dev_ptr(d_best_dist), *(_dev_ptr(a) for a in (d_second_query, d_second_pos, d_second_dist)))

    def reads_pattern_anchored_batch_packed_async(self, d_words, d_word_offsets, d_offsets, count, total_words, k, d_patterns, n_queries, d_best_query, d_best_pos,
                                                  d_best_dist, d_second_query=None, d_second_pos=None, d_second_dist=None, pos_lo=0, pos_hi=0, anchor="start"):
        """reads_hdist_anchored_batch_packed_async under pattern queries."""
        self._call_dev(self._lib.bitnuc_reads_pattern_anchored_batch_packed_async, _dev_ptr(d_words), _dev_ptr(d_word_offsets), _dev_ptr(d_offsets), int(count),
                       int(total_words), int(k), self._anchor(anchor), int(pos_lo), int(pos_hi), _dev_ptr(d_patterns), int(n_queries), _dev_ptr(d_best_query),
                       _dev_ptr(d_best_pos), _dev_ptr(d_best_dist), *(_dev_ptr(a) for a in (d_second_query, d_second_pos, d_second_dist)))

    def reads_pattern_best_batch_async(self, d_seq, d_offsets, count, total_bases, k, d_patterns, n_queries, d_best_query, d_best_pos, d_best_dist):
        """reads_hdist_best_batch_async under pattern queries."""
        self._call_dev(self._lib.bitnuc_reads_pattern_best_batch_async, _dev_ptr(d_seq), _dev_ptr(d_offsets), int(count), int(total_bases), int(k),
                       _dev_ptr(d_patterns), int(n_queries), _dev_ptr(d_best_query), _dev_ptr(d_best_pos), _dev_ptr(d_best_dist))

    def reads_pattern_best_batch_packed_async(self, d_words, d_word_offsets, d_offsets, count, total_words, k, d_patterns, n_queries, d_best_query, d_best_pos,
                                              d_best_dist):
        """reads_hdist_best_batch_packed_async under pattern queries."""
        self._call_dev(self._lib.bitnuc_reads_pattern_best_batch_packed_async, _dev_ptr(d_words), _dev_ptr(d_word_offsets), _dev_ptr(d_offsets), int(count),
                       int(total_words), int(k), _dev_ptr(d_patterns), int(n_queries), _dev_ptr(d_best_query), _dev_ptr(d_best_pos), _dev_ptr(d_best_dist))

    # the pattern twins: d_patterns holds n_queries bitnuc_pattern (16 bytes each, 4-byte aligned) in device memory; the hit lists take their one
    # pattern from the host (a (4,) np.uint32 array)
    def kmer_pattern_count_multi_async(self, d_ref, n, k, d_patterns, d_taus, n_queries, d_counts):
        """d_counts[q] (u64) = windows with pdist <= d_taus[q] (u32) under d_patterns[q].  Asynchronous on the context's stream, as the _dev calls."""
        self._call_dev(self._lib.bitnuc_kmer_pattern_count_multi_async, _dev_ptr(d_ref), int(n), int(k), _dev_ptr(d_patterns), _dev_ptr(d_taus), int(n_queries),
                       _dev_ptr(d_counts))

    def kmer_pattern_count_multi_packed_async(self, d_words, n_words, n, k, d_patterns, d_taus, n_queries, d_counts):
        """The multi-pattern count on packed words in device memory (8-byte aligned)."""
        self._call_dev(self._lib.bitnuc_kmer_pattern_count_multi_packed_async, _dev_ptr(d_words), int(n_words), int(n), int(k), _dev_ptr(d_patterns),
                       _dev_ptr(d_taus), int(n_queries), _dev_ptr(d_counts))

    def kmer_pattern_best_async(self, d_ref, n, k, d_patterns, n_queries, d_pos, d_dist):
        """d_dist[q] (u8) = the smallest pdist of a window under d_patterns[q], d_pos[q] (u64) = the leftmost window that attains it."""
        self._call_dev(self._lib.bitnuc_kmer_pattern_best_async, _dev_ptr(d_ref), int(n), int(k), _dev_ptr(d_patterns), int(n_queries), _dev_ptr(d_pos),
                       _dev_ptr(d_dist))

    def kmer_pattern_best_packed_async(self, d_words, n_words, n, k, d_patterns, n_queries, d_pos, d_dist):
        """The best match per pattern on packed words in device memory (8-byte aligned)."""
        self._call_dev(self._lib.bitnuc_kmer_pattern_best_packed_async, _dev_ptr(d_words), int(n_words), int(n), int(k), _dev_ptr(d_patterns), int(n_queries),
                       _dev_ptr(d_pos), _dev_ptr(d_dist))

    # the indel-tolerant search along a reference: d_end[q] (u64) one past the last aligned base, d_dist[q] (u8); d_counts[q] (u64) = ends j with
    # E_q(j) <= d_taus[q] (u32).  Asynchronous on the context's stream, as the _dev calls
    def kmer_edist_best_async(self, d_ref, n, k, d_queries, n_queries, d_end, d_dist):
        """The best match per query by edit distance: d_dist[q] = min over the ends j of E_q(j), d_end[q] = the smallest j that attains it."""
        self._call_dev(self._lib.bitnuc_kmer_edist_best_async, _dev_ptr(d_ref), int(n), int(k), _dev_ptr(d_queries), int(n_queries), _dev_ptr(d_end),
                       _dev_ptr(d_dist))

    def kmer_edist_best_packed_async(self, d_words, n_words, n, k, d_queries, n_queries, d_end, d_dist):
        """kmer_edist_best_async on packed words in device memory (8-byte aligned)."""
        self._call_dev(self._lib.bitnuc_kmer_edist_best_packed_async, _dev_ptr(d_words), int(n_words), int(n), int(k), _dev_ptr(d_queries), int(n_queries),
                       _dev_ptr(d_end), _dev_ptr(d_dist))

    def kmer_edist_count_multi_async(self, d_ref, n, k, d_queries, d_taus, n_queries, d_counts):
        """d_counts[q] = the ends j with E_q(j) <= d_taus[q]."""
        self._call_dev(self._lib.bitnuc_kmer_edist_count_multi_async, _dev_ptr(d_ref), int(n), int(k), _dev_ptr(d_queries), _dev_ptr(d_taus), int(n_queries),
                       _dev_ptr(d_counts))

    def kmer_edist_count_multi_packed_async(self, d_words, n_words, n, k, d_queries, d_taus, n_queries, d_counts):
        """kmer_edist_count_multi_async on packed words in device memory (8-byte aligned)."""
        self._call_dev(self._lib.bitnuc_kmer_edist_count_multi_packed_async, _dev_ptr(d_words), int(n_words), int(n), int(k), _dev_ptr(d_queries),
                       _dev_ptr(d_taus), int(n_queries), _dev_ptr(d_counts))

    def kmer_pattern_edist_best_async(self, d_ref, n, k, d_patterns, n_queries, d_end, d_dist):
        """kmer_edist_best_async under pattern queries."""
        self._call_dev(self._lib.bitnuc_kmer_pattern_edist_best_async, _dev_ptr(d_ref), int(n), int(k), _dev_ptr(d_patterns), int(n_queries), _dev_ptr(d_end),
                       _dev_ptr(d_dist))

    def kmer_pattern_edist_best_packed_async(self, d_words, n_words, n, k, d_patterns, n_queries, d_end, d_dist):
        """kmer_edist_best_packed_async under pattern queries."""
        self._call_dev(self._lib.bitnuc_kmer_pattern_edist_best_packed_async, _dev_ptr(d_words), int(n_words), int(n), int(k), _dev_ptr(d_patterns),
                       int(n_queries), _dev_ptr(d_end), _dev_ptr(d_dist))

    def kmer_pattern_edist_count_multi_async(self, d_ref, n, k, d_patterns, d_taus, n_queries, d_counts):
        """kmer_edist_count_multi_async under pattern queries."""
        self._call_dev(self._lib.bitnuc_kmer_pattern_edist_count_multi_async, _dev_ptr(d_ref), int(n), int(k), _dev_ptr(d_patterns), _dev_ptr(d_taus),
                       int(n_queries), _dev_ptr(d_counts))

    def kmer_pattern_edist_count_multi_packed_async(self, d_words, n_words, n, k, d_patterns, d_taus, n_queries, d_counts):
        """kmer_edist_count_multi_packed_async under pattern queries."""
        self._call_dev(self._lib.bitnuc_kmer_pattern_edist_count_multi_packed_async, _dev_ptr(d_words), int(n_words), int(n), int(k), _dev_ptr(d_patterns),
                       _dev_ptr(d_taus), int(n_queries), _dev_ptr(d_counts))

    def kmer_edist_hits_async(self, d_ref, n, k, query, tau, d_end, d_hit_dist, cap, d_n_hits):
        """The ends j with E(j) <= tau -> d_end[0 .. min(cap, total)) (u64, ascending), their distances at d_hit_dist (None: not written), total ->
        *d_n_hits (u64).  query: a host value.  Asynchronous on the context's stream, as the _dev calls."""
        self._call_dev(self._lib.bitnuc_kmer_edist_hits_async, _dev_ptr(d_ref), int(n), int(k), C.c_uint64(query), int(tau), _dev_ptr(d_end),
                       _dev_ptr(d_hit_dist), int(cap), _dev_ptr(d_n_hits))

    def kmer_edist_hits_packed_async(self, d_words, n_words, n, k, query, tau, d_end, d_hit_dist, cap, d_n_hits):
        """kmer_edist_hits_async on packed words in device memory (8-byte aligned)."""
        self._call_dev(self._lib.bitnuc_kmer_edist_hits_packed_async, _dev_ptr(d_words), int(n_words), int(n), int(k), C.c_uint64(query), int(tau),
                       _dev_ptr(d_end), _dev_ptr(d_hit_dist), int(cap), _dev_ptr(d_n_hits))

    def kmer_pattern_edist_hits_async(self, d_ref, n, k, pattern, tau, d_end, d_hit_dist, cap, d_n_hits):
        """kmer_edist_hits_async under a pattern query.  pattern: host memory ((4,) np.uint32) or None (the library refuses it)."""
        p = None if pattern is None else np.ascontiguousarray(np.asarray(pattern, dtype=np.uint32).reshape(4))
        self._call_dev(self._lib.bitnuc_kmer_pattern_edist_hits_async, _dev_ptr(d_ref), int(n), int(k), None if p is None else _ptr(p), int(tau),
                       _dev_ptr(d_end), _dev_ptr(d_hit_dist), int(cap), _dev_ptr(d_n_hits))

    def kmer_pattern_edist_hits_packed_async(self, d_words, n_words, n, k, pattern, tau, d_end, d_hit_dist, cap, d_n_hits):
        """kmer_pattern_edist_hits_async on packed words in device memory (8-byte aligned)."""
        p = None if pattern is None else np.ascontiguousarray(np.asarray(pattern, dtype=np.uint32).reshape(4))
        self._call_dev(self._lib.bitnuc_kmer_pattern_edist_hits_packed_async, _dev_ptr(d_words), int(n_words), int(n), int(k), None if p is None else _ptr(p),
                       int(tau), _dev_ptr(d_end), _dev_ptr(d_hit_dist), int(cap), _dev_ptr(d_n_hits))

    # the family's second stage on device tensors: d_query / d_end (u32; along a reference d_query_index u32 or None, d_end u64) -> d_start (u32 / u64),
    # d_dist (u8, or None).  Asynchronous on the context's stream; they chain behind the forward call without a sync (one table slot, stream order)
    def _reads_start_async(self, fn, head, k, d_queries, n_queries, d_query, d_end, d_start, d_dist, anchor, pos):
        self._call_dev(fn, *head, int(k), self._anchor(anchor), int(pos), _dev_ptr(d_queries), int(n_queries), _dev_ptr(d_query), _dev_ptr(d_end),
                       _dev_ptr(d_start), _dev_ptr(d_dist))

    def reads_edist_start_async(self, d_reads, read_len, count, k, d_queries, n_queries, d_query, d_end, d_start, d_dist=None, anchor="start", pos=0):
        """reads_edist_start on device tensors; an invalid byte in a walked range is reported by the next sync()."""
        self._reads_start_async(self._lib.bitnuc_reads_edist_start_async, (_dev_ptr(d_reads), int(read_len), int(count)), k, d_queries, n_queries, d_query, d_end,
                                d_start, d_dist, anchor, pos)

    def reads_edist_start_packed_async(self, d_words, read_len, count, k, d_queries, n_queries, d_query, d_end, d_start, d_dist=None, anchor="start", pos=0):
        """reads_edist_start_async of packed words (ceil(read_len / 32) per read)."""
        self._reads_start_async(self._lib.bitnuc_reads_edist_start_packed_async, (_dev_ptr(d_words), int(read_len), int(count)), k, d_queries, n_queries, d_query,
                                d_end, d_start, d_dist, anchor, pos)

    def reads_pattern_edist_start_async(self, d_reads, read_len, count, k, d_patterns, n_queries, d_query, d_end, d_start, d_dist=None, anchor="start", pos=0):
        """reads_edist_start_async under pattern queries."""
        self._reads_start_async(self._lib.bitnuc_reads_pattern_edist_start_async, (_dev_ptr(d_reads), int(read_len), int(count)), k, d_patterns, n_queries, d_query,
                                d_end, d_start, d_dist, anchor, pos)

    def reads_pattern_edist_start_packed_async(self, d_words, read_len, count, k, d_patterns, n_queries, d_query, d_end, d_start, d_dist=None, anchor="start", pos=0):
        """reads_edist_start_packed_async under pattern queries."""
        self._reads_start_async(self._lib.bitnuc_reads_pattern_edist_start_packed_async, (_dev_ptr(d_words), int(read_len), int(count)), k, d_patterns, n_queries,
                                d_query, d_end, d_start, d_dist, anchor, pos)

    def reads_edist_start_batch_async(self, d_seq, d_offsets, count, total_bases, k, d_queries, n_queries, d_query, d_end, d_start, d_dist=None, anchor="start",
                                      pos=0):
        """reads_edist_start_batch on device tensors; the table is trusted and read on the device."""
        self._reads_start_async(self._lib.bitnuc_reads_edist_start_batch_async, (_dev_ptr(d_seq), _dev_ptr(d_offsets), int(count), int(total_bases)), k, d_queries,
                                n_queries, d_query, d_end, d_start, d_dist, anchor, pos)

    def reads_edist_start_batch_packed_async(self, d_words, d_word_offsets, d_offsets, count, total_words, k, d_queries, n_queries, d_query, d_end, d_start,
                                             d_dist=None, anchor="start", pos=0):
        """reads_edist_start_batch_async on the packed words encode_batch_dev writes."""
        self._reads_start_async(self._lib.bitnuc_reads_edist_start_batch_packed_async,
                                (_dev_ptr(d_words), _dev_ptr(d_word_offsets), _dev_ptr(d_offsets), int(count), int(total_words)), k, d_queries, n_queries, d_query,
                                d_end, d_start, d_dist, anchor, pos)

    def reads_pattern_edist_start_batch_async(self, d_seq, d_offsets, count, total_bases, k, d_patterns, n_queries, d_query, d_end, d_start, d_dist=None,
                                              anchor="start", pos=0):
        """reads_edist_start_batch_async under pattern queries."""
        self._reads_start_async(self._lib.bitnuc_reads_pattern_edist_start_batch_async, (_dev_ptr(d_seq), _dev_ptr(d_offsets), int(count), int(total_bases)), k,
                                d_patterns, n_queries, d_query, d_end, d_start, d_dist, anchor, pos)

    def reads_pattern_edist_start_batch_packed_async(self, d_words, d_word_offsets, d_offsets, count, total_words, k, d_patterns, n_queries, d_query, d_end,
                                                     d_start, d_dist=None, anchor="start", pos=0):
        """reads_edist_start_batch_packed_async under pattern queries."""
        self._reads_start_async(self._lib.bitnuc_reads_pattern_edist_start_batch_packed_async,
                                (_dev_ptr(d_words), _dev_ptr(d_word_offsets), _dev_ptr(d_offsets), int(count), int(total_words)), k, d_patterns, n_queries, d_query,
                                d_end, d_start, d_dist, anchor, pos)

    def kmer_edist_start_async(self, d_ref, n, k, d_queries, n_queries, d_query_index, d_end, m, d_start, d_dist=None, d_m=None):
        """kmer_edist_start on device tensors: m items; d_m (a u64 device count, e.g. the hit list's d_n_hits) bounds them to min(m, *d_m) -- nothing at or
        beyond it is written."""
        self._call_dev(self._lib.bitnuc_ref_edist_start_async, _dev_ptr(d_ref), int(n), int(k), _dev_ptr(d_queries), int(n_queries), _dev_ptr(d_query_index),
                       _dev_ptr(d_end), int(m), _dev_ptr(d_m), _dev_ptr(d_start), _dev_ptr(d_dist))

    def kmer_edist_start_packed_async(self, d_words, n_words, n, k, d_queries, n_queries, d_query_index, d_end, m, d_start, d_dist=None, d_m=None):
        """kmer_edist_start_async on packed words in device memory (8-byte aligned)."""
        self._call_dev(self._lib.bitnuc_ref_edist_start_packed_async, _dev_ptr(d_words), int(n_words), int(n), int(k), _dev_ptr(d_queries), int(n_queries),
                       _dev_ptr(d_query_index), _dev_ptr(d_end), int(m), _dev_ptr(d_m), _dev_ptr(d_start), _dev_ptr(d_dist))

    def kmer_pattern_edist_start_async(self, d_ref, n, k, d_patterns, n_queries, d_query_index, d_end, m, d_start, d_dist=None, d_m=None):
        """kmer_edist_start_async under pattern queries."""
        self._call_dev(self._lib.bitnuc_ref_pattern_edist_start_async, _dev_ptr(d_ref), int(n), int(k), _dev_ptr(d_patterns), int(n_queries),
                       _dev_ptr(d_query_index), _dev_ptr(d_end), int(m), _dev_ptr(d_m), _dev_ptr(d_start), _dev_ptr(d_dist))

    def kmer_pattern_edist_start_packed_async(self, d_words, n_words, n, k, d_patterns, n_queries, d_query_index, d_end, m, d_start, d_dist=None, d_m=None):
        """kmer_edist_start_packed_async under pattern queries."""
        self._call_dev(self._lib.bitnuc_ref_pattern_edist_start_packed_async, _dev_ptr(d_words), int(n_words), int(n), int(k), _dev_ptr(d_patterns),
                       int(n_queries), _dev_ptr(d_query_index), _dev_ptr(d_end), int(m), _dev_ptr(d_m), _dev_ptr(d_start), _dev_ptr(d_dist))

    def kmer_hdist_hist_async(self, d_ref, n, k, d_queries, n_queries, n_bins, d_hist):
        """The mismatch histogram of n_queries queries at once: d_hist[q * n_bins + d] (u64) = windows at distance exactly d < n_bins from d_queries[q]
        (u64).  Asynchronous on the context's stream, as the _dev calls."""
        self._call_dev(self._lib.bitnuc_kmer_hdist_hist_async, _dev_ptr(d_ref), int(n), int(k), _dev_ptr(d_queries), int(n_queries), int(n_bins),
                       _dev_ptr(d_hist))

    def kmer_hdist_hist_packed_async(self, d_words, n_words, n, k, d_queries, n_queries, n_bins, d_hist):
        """The mismatch histogram per query on packed words in device memory (8-byte aligned)."""
        self._call_dev(self._lib.bitnuc_kmer_hdist_hist_packed_async, _dev_ptr(d_words), int(n_words), int(n), int(k), _dev_ptr(d_queries), int(n_queries),
                       int(n_bins), _dev_ptr(d_hist))

    def kmer_pattern_hist_async(self, d_ref, n, k, d_patterns, n_queries, n_bins, d_hist):
        """d_hist[q * n_bins + d] (u64) = windows with pdist exactly d < n_bins under d_patterns[q]."""
        self._call_dev(self._lib.bitnuc_kmer_pattern_hist_async, _dev_ptr(d_ref), int(n), int(k), _dev_ptr(d_patterns), int(n_queries), int(n_bins),
                       _dev_ptr(d_hist))

    def kmer_pattern_hist_packed_async(self, d_words, n_words, n, k, d_patterns, n_queries, n_bins, d_hist):
        """The mismatch histogram per pattern on packed words in device memory (8-byte aligned)."""
        self._call_dev(self._lib.bitnuc_kmer_pattern_hist_packed_async, _dev_ptr(d_words), int(n_words), int(n), int(k), _dev_ptr(d_patterns), int(n_queries),
                       int(n_bins), _dev_ptr(d_hist))

    def kmer_pattern_hits_async(self, d_ref, n, k, pattern, tau, d_pos, d_hit_dist, cap, d_n_hits):
        """The positions of the windows with pdist <= tau -> d_pos[0 .. min(cap, total)) (u64, ascending), their distances at d_hit_dist (None: not
        written), total -> *d_n_hits (u64).  pattern: host memory ((4,) np.uint32) or None (the library refuses it)."""
        p = None if pattern is None else np.ascontiguousarray(np.asarray(pattern, dtype=np.uint32).reshape(4))
        self._call_dev(self._lib.bitnuc_kmer_pattern_hits_async, _dev_ptr(d_ref), int(n), int(k), None if p is None else _ptr(p), int(tau), _dev_ptr(d_pos),
                       _dev_ptr(d_hit_dist), int(cap), _dev_ptr(d_n_hits))

    def kmer_pattern_hits_packed_async(self, d_words, n_words, n, k, pattern, tau, d_pos, d_hit_dist, cap, d_n_hits):
        """The pattern hit list on packed words in device memory (8-byte aligned)."""
        p = None if pattern is None else np.ascontiguousarray(np.asarray(pattern, dtype=np.uint32).reshape(4))
        self._call_dev(self._lib.bitnuc_kmer_pattern_hits_packed_async, _dev_ptr(d_words), int(n_words), int(n), int(k), None if p is None else _ptr(p), int(tau),
                       _dev_ptr(d_pos), _dev_ptr(d_hit_dist), int(cap), _dev_ptr(d_n_hits))

    def hdist_dev(self, d_a, na, d_b, nb, n_bases, d_result):
        self._call_dev(self._lib.bitnuc_hdist_dev, _dev_ptr(d_a), int(na), _dev_ptr(d_b), int(nb), int(n_bases), _dev_ptr(d_result))

    def nucgen_dev(self, d_out, length, seed, first=0, flags=0):
        self._call_dev(self._lib.bitnuc_nucgen_dev, _dev_ptr(d_out), int(length), C.c_uint64(seed), C.c_uint64(first), int(flags))

    def host_pipe_info(self):
        """Configuration of the pipelined host-pointer path (creates it if needed): bases per chunk and chunks in flight."""
        names = ["chunk_bases", "depth"]
        out = (C.c_double * len(names))()
        err = L.BitnucErr()
        if self._lib.bitnuc_host_pipe_info(self._h, out, len(names), C.byref(err)) != L.OK:
            _raise(err)
        return {k: int(v) for k, v in zip(names, out)}

    def stream_probe_dev(self, mode, d_src, d_dst, nbytes):
        self._call_dev(self._lib.bitnuc_stream_probe_dev, int(mode), _dev_ptr(d_src), _dev_ptr(d_dst), int(nbytes))


class BatchPlan:
    """Layout plan of a ragged batch (bitnuc_batch_plan): built once from the device offsets table, used by every
    encode / decode of that layout.  `build` may be called again for the next batch (memory is reused)."""

    def __init__(self, ctx, d_offsets=None, count=0):
        self._ctx, self._lib = ctx, ctx._lib
        self._h = C.c_void_p()
        err = L.BitnucErr()
        if self._lib.bitnuc_batch_plan_create(ctx._h, C.byref(self._h), C.byref(err)) != L.OK:
            self._h = C.c_void_p()
            _raise(err)
        self.total_words = 0
        if d_offsets is not None:
            self.build(d_offsets, count)

    def build(self, d_offsets, count):
        total = C.c_size_t(0)
        err = L.BitnucErr()
        if self._lib.bitnuc_batch_plan_build_dev(self._ctx._h, self._h, _dev_ptr(d_offsets), int(count), C.byref(total), C.byref(err)) != L.OK:
            _raise(err)
        self.total_words = total.value
        return total.value

    @property
    def word_offsets_ptr(self):
        """Device address of the plan's word-offsets table (count + 1 u64 entries)."""
        return self._lib.bitnuc_batch_plan_word_offsets_dev(self._h)

    def encode_dev(self, d_seq, d_out):
        err = L.BitnucErr()
        if self._lib.bitnuc_encode_batch_plan_dev(self._ctx._h, self._h, _dev_ptr(d_seq), _dev_ptr(d_out), C.byref(err)) != L.OK:
            _raise(err)

    def decode_dev(self, d_words, d_out):
        err = L.BitnucErr()
        if self._lib.bitnuc_decode_batch_plan_dev(self._ctx._h, self._h, _dev_ptr(d_words), _dev_ptr(d_out), C.byref(err)) != L.OK:
            _raise(err)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.bitnuc_batch_plan_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close


class Comm:
    """One rank of an RCCL communicator bound to a Context (config 4's concatenation).
    One process per GPU: rank 0 makes `Comm.unique_id()`, shares the 128 bytes, every rank
    calls `Comm(ctx, nranks, rank, uid)`."""

    def __init__(self, ctx, nranks, rank, uid):
        self._lib = L.load()
        self._ctx = ctx
        self._h = C.c_void_p()
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(uid))
        err = L.BitnucErr()
        if self._lib.bitnuc_comm_init_rank(ctx._h, int(nranks), int(rank), buf, C.byref(self._h), C.byref(err)) != L.OK:
            self._h = C.c_void_p()
            _raise(err)

    @staticmethod
    def unique_id():
        lib = L.load()
        buf = (C.c_uint8 * 128)()
        err = L.BitnucErr()
        if lib.bitnuc_comm_get_unique_id(buf, C.byref(err)) != L.OK:
            _raise(err)
        return bytes(buf)

    @property
    def nranks(self):
        return self._lib.bitnuc_comm_nranks(self._h)

    @property
    def rank(self):
        return self._lib.bitnuc_comm_rank(self._h)

    def allgather_words_dev(self, d_local, count, d_all):
        err = L.BitnucErr()
        if self._lib.bitnuc_allgather_words_dev(self._ctx._h, self._h, _dev_ptr(d_local), int(count), _dev_ptr(d_all), C.byref(err)) != L.OK:
            _raise(err)

    def allgatherv_words_dev(self, counts, d_all):
        """In-place all-gather of UNEQUAL word counts (a ragged batch sharded by whole sequences, dist.batch_shard_ranges): rank r's
        counts[r] words already sit at d_all + sum(counts[:r]); afterwards every rank holds all of them."""
        arr = (C.c_size_t * len(counts))(*[int(x) for x in counts])
        err = L.BitnucErr()
        if self._lib.bitnuc_allgatherv_words_dev(self._ctx._h, self._h, arr, _dev_ptr(d_all), C.byref(err)) != L.OK:
            _raise(err)

    def set_threaded(self, threaded=True):
        return self._lib.bitnuc_comm_set_threaded(self._h, int(bool(threaded)))

    def encode_sharded_allgather_dev(self, d_seq_shard, shard_len, d_all):
        err = L.BitnucErr()
        if self._lib.bitnuc_encode_sharded_allgather_dev(self._ctx._h, self._h, _dev_ptr(d_seq_shard), int(shard_len), _dev_ptr(d_all), C.byref(err)) != L.OK:
            _raise(err)

    def encode_sharded_allgather_overlapped_dev(self, d_seq_shard, shard_len, n_chunks, d_all):
        """Same result as encode_sharded_allgather_dev, the exchange hidden behind the encode: n_chunks pieces, each moved in
        place by a second stream as soon as it is encoded (include/bitnuc_hip.h)."""
        err = L.BitnucErr()
        if self._lib.bitnuc_encode_sharded_allgather_overlapped_dev(self._ctx._h, self._h, _dev_ptr(d_seq_shard), int(shard_len), int(n_chunks), _dev_ptr(d_all), C.byref(err)) != L.OK:
            _raise(err)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.bitnuc_comm_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close


class CommGroup:
    """All ranks of a communicator in ONE thread (bitnuc_comm_init_all[_devices]): n contexts + communicators, driven together by the
    _all entry points, which issue every rank's part of an exchange inside one RCCL group and synchronise every stream before they
    return.  The per-rank entry points refuse these communicators (they would wait for peers this thread has not issued yet)."""

    def __init__(self, n_gpus, devices=None, lib_path=None):
        self._lib = L.load(lib_path)
        self.n = int(n_gpus)
        self._ctxs = (C.c_void_p * self.n)()
        self._comms = (C.c_void_p * self.n)()
        devs = (C.c_int * self.n)(*devices) if devices is not None else None
        err = L.BitnucErr()
        if self._lib.bitnuc_comm_init_all_devices(self.n, devs, self._ctxs, self._comms, C.byref(err)) != L.OK:
            self.n = 0
            _raise(err)

    def encode_sharded_allgather(self, d_seq_shards, shard_len, d_alls, n_chunks=0):
        """d_seq_shards[r]: rank r's shard (shard_len bases, a multiple of 32, on rank r's device); d_alls[r]: rank r's output of
        n * shard_len / 32 words.  n_chunks = 0: one grouped ncclAllGather; >= 1: the chunked in-place exchange behind the encode.
        On InvalidBase the error carries the shard-relative index and, in .value, the rank."""
        seqs = (C.c_void_p * self.n)(*[_dev_ptr(t) for t in d_seq_shards])
        alls = (C.c_void_p * self.n)(*[_dev_ptr(t) for t in d_alls])
        err = L.BitnucErr()
        if n_chunks:
            st = self._lib.bitnuc_encode_sharded_allgather_overlapped_all(self.n, self._ctxs, self._comms, seqs, int(shard_len), int(n_chunks), alls, C.byref(err))
        else:
            st = self._lib.bitnuc_encode_sharded_allgather_all(self.n, self._ctxs, self._comms, seqs, int(shard_len), alls, C.byref(err))
        if st != L.OK:
            try:
                _raise(err)
            except NucleotideError as e:
                e.rank = int(err.value) if st == L.INVALID_BASE else None  # whose shard holds the byte
                raise

    def context(self, rank):
        """Rank `rank`'s context as a Context object that does NOT own the handle (the group destroys it): for the calls a rank makes
        on its own device between the group's exchanges -- building a BatchPlan, encoding its run of a ragged batch into its slot."""
        c = Context.__new__(Context)
        c._lib, c._h, c.device, c._borrowed = self._lib, C.c_void_p(self._ctxs[rank]), None, True
        return c

    def allgatherv_words(self, counts, d_alls):
        """bitnuc_allgatherv_words_all: every rank's counts[r] words (already at d_alls[r] + sum(counts[:r])) reach every rank's buffer."""
        arr = (C.c_size_t * self.n)(*[int(x) for x in counts])
        alls = (C.c_void_p * self.n)(*[_dev_ptr(t) for t in d_alls])
        err = L.BitnucErr()
        if self._lib.bitnuc_allgatherv_words_all(self.n, self._ctxs, self._comms, arr, alls, C.byref(err)) != L.OK:
            _raise(err)

    def close(self):
        for i in range(getattr(self, "n", 0)):
            if self._comms[i]:
                self._lib.bitnuc_comm_destroy(self._comms[i])
                self._comms[i] = None
            if self._ctxs[i]:
                self._lib.bitnuc_ctx_destroy(self._ctxs[i])
                self._ctxs[i] = None
        self.n = 0

    __del__ = close


def batch_shard_ranges(offsets, nranks, lib_path=None):
    """bitnuc_batch_shard_ranges (host arithmetic, no device): the partition of a ragged batch by WHOLE sequences, balanced by word
    count.  Returns (seq_first[nranks+1], word_first[nranks+1]) as numpy arrays; bitnuc_amd.dist.batch_shard_ranges is the same rule
    in numpy (tests hold the two against each other)."""
    lib = L.load(lib_path)
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    count = off.size - 1
    seq_first = np.zeros(nranks + 1, dtype=np.uint64)
    word_first = np.zeros(nranks + 1, dtype=np.uint64)
    err = L.BitnucErr()
    if lib.bitnuc_batch_shard_ranges(_ptr(off), count, int(nranks), _ptr(seq_first), _ptr(word_first), C.byref(err)) != L.OK:
        _raise(err)
    return seq_first, word_first


def peer_link_probe(src_device, dst_devices, nbytes=256 << 20, reps=3, lib_path=None):
    """xGMI link probe: hipMemcpyPeerAsync from src_device to each of dst_devices, one link at a time and all at once.
    Returns {"gb_s_each": [...], "gb_s_all": x}; raises NucleotideError('Unsupported') with fewer than two devices."""
    lib = L.load(lib_path)
    n = len(dst_devices)
    dst = (C.c_int * max(n, 1))(*dst_devices)
    each = (C.c_double * max(n, 1))()
    allv = C.c_double(0)
    err = L.BitnucErr()
    if lib.bitnuc_peer_link_probe(int(src_device), dst, n, int(nbytes), int(reps), each, C.byref(allv), C.byref(err)) != L.OK:
        _raise(err)
    return {"gb_s_each": [round(each[i], 1) for i in range(n)], "gb_s_all": round(allv.value, 1)}


# ---- module-level functions with the reference's names (default context, device 0) ----------
_default = None


def pattern_from_iupac(letters, lib_path=None):
    """A pattern query from IUPAC letters (ACGTU RYSWKM BDHV N, either case; at most 32) -> (4,) np.uint32: allow[c] bit i set <=> base code c
    (A 0, C 1, G 2, T 3) matches at position i.  Host code, no context."""
    b = np.frombuffer(letters.encode() if isinstance(letters, str) else bytes(letters), dtype=np.uint8)
    out = np.zeros(4, dtype=np.uint32)
    err = L.BitnucErr()
    if L.load(lib_path).bitnuc_pattern_from_iupac(_ptr(b) if b.size else None, b.size, _ptr(out), C.byref(err)) != L.OK:
        _raise(err)
    return out


def pattern_from_2bit(query, k, lib_path=None):
    """The pattern of singletons of a packed exact query of k bases -> (4,) np.uint32: it makes every pattern entry point compute what its exact twin
    computes for `query`.  Host code, no context."""
    out = np.zeros(4, dtype=np.uint32)
    err = L.BitnucErr()
    if L.load(lib_path).bitnuc_pattern_from_2bit(C.c_uint64(int(query)), int(k), _ptr(out), C.byref(err)) != L.OK:
        _raise(err)
    return out


def default_context():
    global _default
    if _default is None:
        _default = Context(0)
    return _default


_ctxfree = None


def context_free():
    """A handle with a NULL bitnuc_ctx: the single-word functions (and bulk host-pointer calls below the
    library's host cutoff) are host code and need no device, like the reference's free functions."""
    global _ctxfree
    if _ctxfree is None:
        c = Context.__new__(Context)
        c._lib, c._h, c.device = L.load(), C.c_void_p(0), None
        _ctxfree = c
    return _ctxfree


def as_2bit(seq):
    return context_free().as_2bit(seq)


def from_2bit(packed, expected_size, sequence):
    return context_free().from_2bit(packed, expected_size, sequence)


def from_2bit_alloc(packed, expected_size):
    return context_free().from_2bit_alloc(packed, expected_size)


def encode(sequence, ebuf):
    return default_context().encode(sequence, ebuf)


def encode_alloc(sequence):
    return default_context().encode_alloc(sequence)


def decode(ebuf, n_bases, dbuf):
    return default_context().decode(ebuf, n_bases, dbuf)


def hdist_scalar(u, v, length):
    return context_free().hdist_scalar(u, v, length)


def hdist(ebuf1, ebuf2, n_bases):
    return default_context().hdist(ebuf1, ebuf2, n_bases)


def as_2bit_batch(kmers, k, stride=None, count=None):
    return default_context().as_2bit_batch(kmers, k, stride, count)


def kmer_hdist_scan(ref, k, query):
    return default_context().kmer_hdist_scan(ref, k, query)


def kmer_hdist_scan_packed(words, n_bases, k, query):
    return default_context().kmer_hdist_scan_packed(words, n_bases, k, query)


def split_packed(ebuf, slen, idx, lbuf, rbuf, canonical=False):
    return default_context().split_packed(ebuf, slen, idx, lbuf, rbuf, canonical=canonical)
