//! bitnuc-hip: the public surface of `bitnuc` (src/lib.rs:214-220 of the reference)
//! re-implemented over libbitnuc_hip.so.  Swap `use bitnuc::{..}` for
//! `use bitnuc_hip::{..}`; names, argument meaning, Vec clear/append conventions and
//! error values are the reference's.
//!
//! NOT COMPILED IN THIS REPO's CI: the build image has no Rust toolchain.  Every function
//! below is a mechanical wrapper of a C-ABI entry point that is compiled and tested
//! (see tests/ and include/bitnuc.hpp, the same layer in C++).
pub mod ffi;

use std::cell::RefCell;
use std::fmt;

/// src/error.rs:3-18 of the reference.
#[derive(Debug, PartialEq, Eq)]
pub enum NucleotideError {
    InvalidBase(u8),
    SequenceTooLong(usize),
    InvalidLength(usize),
    IndexOutOfBounds { index: usize, length: usize },
    InvalidRange { start: usize, end: usize, length: usize },
    Unsupported,
}

impl fmt::Display for NucleotideError {
    fn fmt(&self, f: &mut fmt::Formatter<'_>) -> fmt::Result {
        match self {
            NucleotideError::InvalidBase(b) => write!(f, "Invalid nucleotide base: {}", b),
            NucleotideError::SequenceTooLong(len) => write!(f, "Sequence length {} exceeds maximum", len),
            NucleotideError::InvalidLength(len) => write!(f, "Invalid length: {}", len),
            NucleotideError::IndexOutOfBounds { index, length } => {
                write!(f, "Index {} out of bounds for sequence of length {}", index, length)
            }
            NucleotideError::InvalidRange { start, end, length } => {
                write!(f, "Invalid range {}..{} for sequence of length {}", start, end, length)
            }
            NucleotideError::Unsupported => write!(f, "Unsupported architecture"),
        }
    }
}
impl std::error::Error for NucleotideError {}

fn to_err(e: &ffi::bitnuc_err) -> NucleotideError {
    match e.status {
        ffi::BITNUC_INVALID_BASE => NucleotideError::InvalidBase(e.byte),
        ffi::BITNUC_SEQUENCE_TOO_LONG => NucleotideError::SequenceTooLong(e.value as usize),
        ffi::BITNUC_INVALID_LENGTH => NucleotideError::InvalidLength(e.value as usize),
        ffi::BITNUC_INDEX_OUT_OF_BOUNDS => NucleotideError::IndexOutOfBounds { index: e.index as usize, length: e.value as usize },
        // a HIP failure has no reference counterpart; there is no CPU fallback to fall to
        ffi::BITNUC_BACKEND_ERROR => panic!("bitnuc-hip: HIP backend error {}", e.backend_code),
        _ => NucleotideError::Unsupported,
    }
}

/// One device + stream + scratch.  `!Sync`: use one per thread.
pub struct Context {
    raw: *mut ffi::bitnuc_ctx,
}

impl Context {
    pub fn new(device: i32) -> Self {
        let mut raw = std::ptr::null_mut();
        let mut e = ffi::bitnuc_err::default();
        let st = unsafe { ffi::bitnuc_ctx_create(device, &mut raw, &mut e) };
        assert!(st == ffi::BITNUC_OK, "bitnuc-hip: no usable HIP device (hipError {})", e.backend_code);
        Context { raw }
    }
    pub fn raw(&self) -> *mut ffi::bitnuc_ctx {
        self.raw
    }
}
impl Drop for Context {
    fn drop(&mut self) {
        unsafe { ffi::bitnuc_ctx_destroy(self.raw) }
    }
}

thread_local! {
    static CTX: RefCell<Option<Context>> = RefCell::new(None);
}
fn with_ctx<R>(f: impl FnOnce(*mut ffi::bitnuc_ctx) -> R) -> R {
    CTX.with(|c| {
        let mut c = c.borrow_mut();
        let ctx = c.get_or_insert_with(|| Context::new(0));
        f(ctx.raw)
    })
}

/// `bitnuc::as_2bit` (src/utils/packing/mod.rs:80-110).
pub fn as_2bit(seq: &[u8]) -> Result<u64, NucleotideError> {
    let mut out = 0u64;
    let mut e = ffi::bitnuc_err::default();
    // context-free: single words are host code inside the library (include/bitnuc_hip.h, "Size dispatch"), like the reference's #[inline(always)] function
    let st = unsafe { ffi::bitnuc_as_2bit(std::ptr::null_mut(), seq.as_ptr(), seq.len(), &mut out, &mut e) };
    if st == ffi::BITNUC_OK { Ok(out) } else { Err(to_err(&e)) }
}

/// `bitnuc::from_2bit` (src/utils/unpacking/mod.rs:119-147): APPENDS `expected_size` bases.
pub fn from_2bit(packed: u64, expected_size: usize, sequence: &mut Vec<u8>) -> Result<(), NucleotideError> {
    let mut tmp = [0u8; 32];
    let mut e = ffi::bitnuc_err::default();
    let st = unsafe { ffi::bitnuc_from_2bit(std::ptr::null_mut(), packed, expected_size, tmp.as_mut_ptr(), &mut e) };
    if st != ffi::BITNUC_OK {
        return Err(to_err(&e));
    }
    sequence.extend_from_slice(&tmp[..expected_size]);
    Ok(())
}

/// `bitnuc::from_2bit_alloc` (src/utils/unpacking/mod.rs:178-182).
pub fn from_2bit_alloc(packed: u64, expected_size: usize) -> Result<Vec<u8>, NucleotideError> {
    let mut sequence = Vec::with_capacity(expected_size.min(32));
    from_2bit(packed, expected_size, &mut sequence)?;
    Ok(sequence)
}

/// `bitnuc::encode` (src/utils/mod.rs:22-25): CLEARS `ebuf`, then fills it.  On
/// `InvalidBase` the Vec keeps the words of the chunks before the failing one, like the
/// reference (packing/avx.rs:142-143).  Empty input panics, like the reference (:138).
pub fn encode(sequence: &[u8], ebuf: &mut Vec<u64>) -> Result<(), NucleotideError> {
    ebuf.clear();
    let n_chunks = sequence.len().div_ceil(32);
    let _ = n_chunks - 1; // same overflow panic as `for _ in 0..n_chunks - 1` in the reference
    ebuf.resize(n_chunks, 0);
    let mut n_words = 0usize;
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_encode(c, sequence.as_ptr(), sequence.len(), ebuf.as_mut_ptr(), &mut n_words, &mut e)
    });
    ebuf.truncate(n_words);
    if st == ffi::BITNUC_OK { Ok(()) } else { Err(to_err(&e)) }
}

/// `bitnuc::encode_alloc` (src/utils/mod.rs:38-42).
pub fn encode_alloc(sequence: &[u8]) -> Result<Vec<u64>, NucleotideError> {
    let mut ebuf = Vec::new();
    encode(sequence, &mut ebuf)?;
    Ok(ebuf)
}

/// `bitnuc::decode` (src/utils/mod.rs:60-62): APPENDS `n_bases` bases to `dbuf`.
pub fn decode(ebuf: &[u64], n_bases: usize, dbuf: &mut Vec<u8>) -> Result<(), NucleotideError> {
    let old = dbuf.len();
    dbuf.resize(old + n_bases, 0);
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_decode(c, ebuf.as_ptr(), ebuf.len(), n_bases, dbuf.as_mut_ptr().add(old), &mut e)
    });
    if st != ffi::BITNUC_OK {
        dbuf.truncate(old);
        return Err(to_err(&e));
    }
    Ok(())
}

/// `bitnuc::hdist_scalar` (src/utils/functions/hamming/scalar.rs:11-48).
pub fn hdist_scalar(u: u64, v: u64, len: usize) -> Result<u32, NucleotideError> {
    let mut out = 0u32;
    let mut e = ffi::bitnuc_err::default();
    let st = unsafe { ffi::bitnuc_hdist_scalar(std::ptr::null_mut(), u, v, len, &mut out, &mut e) };
    if st == ffi::BITNUC_OK { Ok(out) } else { Err(to_err(&e)) }
}

/// `bitnuc::hdist` (src/utils/functions/hamming/multi.rs:121-160).
pub fn hdist(ebuf1: &[u64], ebuf2: &[u64], n_bases: usize) -> Result<u32, NucleotideError> {
    let mut out = 0u32;
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_hdist(c, ebuf1.as_ptr(), ebuf1.len(), ebuf2.as_ptr(), ebuf2.len(), n_bases, &mut out, &mut e)
    });
    if st == ffi::BITNUC_OK { Ok(out) } else { Err(to_err(&e)) }
}

/// `bitnuc::split_packed` (src/utils/functions/split.rs:15-99), word for word
/// (`BITNUC_SPLIT_AS_WRITTEN`): validates, clears `lbuf`/`rbuf`, fills them.
pub fn split_packed(ebuf: &[u64], slen: usize, idx: usize, lbuf: &mut Vec<u64>, rbuf: &mut Vec<u64>) -> Result<(), NucleotideError> {
    split_packed_with(ebuf, slen, idx, lbuf, rbuf, ffi::BITNUC_SPLIT_AS_WRITTEN)
}

/// The funnel-shift split: `lbuf == encode(seq[..idx])`, `rbuf == encode(seq[idx..])`.
pub fn split_packed_canonical(ebuf: &[u64], slen: usize, idx: usize, lbuf: &mut Vec<u64>, rbuf: &mut Vec<u64>) -> Result<(), NucleotideError> {
    split_packed_with(ebuf, slen, idx, lbuf, rbuf, ffi::BITNUC_SPLIT_CANONICAL)
}

fn split_packed_with(ebuf: &[u64], slen: usize, idx: usize, lbuf: &mut Vec<u64>, rbuf: &mut Vec<u64>, flags: std::os::raw::c_int) -> Result<(), NucleotideError> {
    let (mut nl, mut nr) = (0usize, 0usize);
    let mut e = ffi::bitnuc_err::default();
    if unsafe { ffi::bitnuc_split_packed_sizes(ebuf.len(), slen, idx, flags, &mut nl, &mut nr, &mut e) } != ffi::BITNUC_OK {
        return Err(to_err(&e)); // before the buffers are cleared, like split.rs:23-32
    }
    lbuf.clear();
    rbuf.clear();
    lbuf.resize(nl, 0);
    rbuf.resize(nr, 0);
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_split_packed(c, ebuf.as_ptr(), ebuf.len(), slen, idx, flags, lbuf.as_mut_ptr(), &mut nl, rbuf.as_mut_ptr(), &mut nr, &mut e)
    });
    if st == ffi::BITNUC_OK { Ok(()) } else { Err(to_err(&e)) }
}

/// Batched form of the `for kmer in kmers { as_2bit(kmer)? }` idiom (README.md:52-56 of
/// the reference): `count` k-mers of length `k`, k-mer j at `kmers[j*stride..]`.
pub fn as_2bit_batch(kmers: &[u8], k: usize, stride: usize, count: usize) -> Result<Vec<u64>, NucleotideError> {
    assert!(count == 0 || (count - 1) * stride + k <= kmers.len());
    let mut out = vec![0u64; count];
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe { ffi::bitnuc_as_2bit_batch(c, kmers.as_ptr(), k, stride, count, out.as_mut_ptr(), &mut e) });
    if st == ffi::BITNUC_OK { Ok(out) } else { Err(to_err(&e)) }
}

/// `reference.windows(k).map(|w| hdist_scalar(as_2bit(w)?, query, k))` in one launch.
pub fn kmer_hdist_scan(reference: &[u8], k: usize, query: u64) -> Result<Vec<u8>, NucleotideError> {
    let nwin = if k > 0 && reference.len() >= k { reference.len() - k + 1 } else { 0 };
    let mut out = vec![0u8; nwin];
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_hdist_scan(c, reference.as_ptr(), reference.len(), k, query, out.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok(out) } else { Err(to_err(&e)) }
}

/// `kmer_hdist_scan` of the packed sequence `words` holding `n` bases (as `encode` writes them), without decoding it.
pub fn kmer_hdist_scan_packed(words: &[u64], n: usize, k: usize, query: u64) -> Result<Vec<u8>, NucleotideError> {
    let nwin = if k > 0 && n >= k { n - k + 1 } else { 0 };
    let mut out = vec![0u8; nwin];
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_hdist_scan_packed(c, words.as_ptr(), words.len(), n, k, query, out.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok(out) } else { Err(to_err(&e)) }
}

/// The number of windows of the packed sequence `words` (`n` bases) whose Hamming distance to `query` is at most `tau`.
pub fn kmer_hdist_count_packed(words: &[u64], n: usize, k: usize, query: u64, tau: u32) -> Result<u64, NucleotideError> {
    let mut count = 0u64;
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_hdist_count_packed(c, words.as_ptr(), words.len(), n, k, query, tau, &mut count, &mut e)
    });
    if st == ffi::BITNUC_OK { Ok(count) } else { Err(to_err(&e)) }
}

/// The positions (ascending) and distances of the windows of `reference` whose Hamming distance to `query` is at most `tau`: a first call
/// with cap 0 returns their number, a second fills the lists.
pub fn kmer_hdist_hits(reference: &[u8], k: usize, query: u64, tau: u32) -> Result<(Vec<u64>, Vec<u8>), NucleotideError> {
    let mut total = 0u64;
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_hdist_hits(c, reference.as_ptr(), reference.len(), k, query, tau, std::ptr::null_mut(), std::ptr::null_mut(), 0, &mut total, &mut e)
    });
    if st != ffi::BITNUC_OK { return Err(to_err(&e)); }
    let mut pos = vec![0u64; total as usize];
    let mut dist = vec![0u8; total as usize];
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_hdist_hits(c, reference.as_ptr(), reference.len(), k, query, tau, pos.as_mut_ptr(), dist.as_mut_ptr(), pos.len(), &mut total, &mut e)
    });
    if st == ffi::BITNUC_OK { Ok((pos, dist)) } else { Err(to_err(&e)) }
}

/// `kmer_hdist_hits` of the packed sequence `words` holding `n` bases, without decoding it.
pub fn kmer_hdist_hits_packed(words: &[u64], n: usize, k: usize, query: u64, tau: u32) -> Result<(Vec<u64>, Vec<u8>), NucleotideError> {
    let mut total = 0u64;
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_hdist_hits_packed(c, words.as_ptr(), words.len(), n, k, query, tau, std::ptr::null_mut(), std::ptr::null_mut(), 0, &mut total, &mut e)
    });
    if st != ffi::BITNUC_OK { return Err(to_err(&e)); }
    let mut pos = vec![0u64; total as usize];
    let mut dist = vec![0u8; total as usize];
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_hdist_hits_packed(c, words.as_ptr(), words.len(), n, k, query, tau, pos.as_mut_ptr(), dist.as_mut_ptr(), pos.len(), &mut total, &mut e)
    });
    if st == ffi::BITNUC_OK { Ok((pos, dist)) } else { Err(to_err(&e)) }
}

/// `counts[q]` = the number of windows of `reference` whose Hamming distance to `queries[q]` is at most `taus[q]`, every query in one pass
/// (`taus.len()` must equal `queries.len()`).
pub fn kmer_hdist_count_multi(reference: &[u8], k: usize, queries: &[u64], taus: &[u32]) -> Result<Vec<u64>, NucleotideError> {
    if taus.len() != queries.len() { return Err(NucleotideError::Unsupported); }
    let mut counts = vec![0u64; queries.len()];
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_hdist_count_multi(c, reference.as_ptr(), reference.len(), k, queries.as_ptr(), taus.as_ptr(), queries.len(), counts.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok(counts) } else { Err(to_err(&e)) }
}

/// `kmer_hdist_count_multi` of the packed sequence `words` holding `n` bases, without decoding it.
pub fn kmer_hdist_count_multi_packed(words: &[u64], n: usize, k: usize, queries: &[u64], taus: &[u32]) -> Result<Vec<u64>, NucleotideError> {
    if taus.len() != queries.len() { return Err(NucleotideError::Unsupported); }
    let mut counts = vec![0u64; queries.len()];
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_hdist_count_multi_packed(c, words.as_ptr(), words.len(), n, k, queries.as_ptr(), taus.as_ptr(), queries.len(), counts.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok(counts) } else { Err(to_err(&e)) }
}

/// The best match per query in one pass: `(pos, dist)` with `dist[q]` = the smallest Hamming distance of a window of `reference` to `queries[q]` and
/// `pos[q]` = the leftmost window that attains it (no windows: `u64::MAX` / `0xFF`).
pub fn kmer_hdist_best(reference: &[u8], k: usize, queries: &[u64]) -> Result<(Vec<u64>, Vec<u8>), NucleotideError> {
    let mut pos = vec![0u64; queries.len()];
    let mut dist = vec![0u8; queries.len()];
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_hdist_best(c, reference.as_ptr(), reference.len(), k, queries.as_ptr(), queries.len(), pos.as_mut_ptr(), dist.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok((pos, dist)) } else { Err(to_err(&e)) }
}

/// `kmer_hdist_best` of the packed sequence `words` holding `n` bases, without decoding it.
pub fn kmer_hdist_best_packed(words: &[u64], n: usize, k: usize, queries: &[u64]) -> Result<(Vec<u64>, Vec<u8>), NucleotideError> {
    let mut pos = vec![0u64; queries.len()];
    let mut dist = vec![0u8; queries.len()];
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_hdist_best_packed(c, words.as_ptr(), words.len(), n, k, queries.as_ptr(), queries.len(), pos.as_mut_ptr(), dist.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok((pos, dist)) } else { Err(to_err(&e)) }
}

/// The mismatch histogram per query in one pass: `hist[q * n_bins + d]` = the number of windows of `reference` at Hamming distance exactly `d` from
/// `queries[q]`, `d < n_bins <= 16`; a window at `n_bins` or more mismatches is counted nowhere.
pub fn kmer_hdist_hist(reference: &[u8], k: usize, queries: &[u64], n_bins: usize) -> Result<Vec<u64>, NucleotideError> {
    let mut hist = vec![0u64; queries.len() * n_bins.min(ffi::BITNUC_HIST_MAX_BINS)]; // (a refused n_bins writes nothing)
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_hdist_hist(c, reference.as_ptr(), reference.len(), k, queries.as_ptr(), queries.len(), n_bins, hist.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok(hist) } else { Err(to_err(&e)) }
}

/// `kmer_hdist_hist` of the packed sequence `words` holding `n` bases, without decoding it.
pub fn kmer_hdist_hist_packed(words: &[u64], n: usize, k: usize, queries: &[u64], n_bins: usize) -> Result<Vec<u64>, NucleotideError> {
    let mut hist = vec![0u64; queries.len() * n_bins.min(ffi::BITNUC_HIST_MAX_BINS)]; // (a refused n_bins writes nothing)
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_hdist_hist_packed(c, words.as_ptr(), words.len(), n, k, queries.as_ptr(), queries.len(), n_bins, hist.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok(hist) } else { Err(to_err(&e)) }
}

/// The best match per read of `count` back-to-back reads of `read_len` bases: `(query, pos, dist)` with the smallest (distance, query, offset)
/// over all queries and the windows that lie wholly inside each read; a read without a window gets `u32::MAX`, `u32::MAX`, `255`.
pub fn reads_hdist_best(reads: &[u8], read_len: usize, k: usize, queries: &[u64]) -> Result<(Vec<u32>, Vec<u32>, Vec<u8>), NucleotideError> {
    let count = if read_len == 0 { 0 } else { reads.len() / read_len };
    let (mut query, mut pos, mut dist) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_reads_hdist_best(c, reads.as_ptr(), read_len, count, k, queries.as_ptr(), queries.len(), query.as_mut_ptr(), pos.as_mut_ptr(), dist.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok((query, pos, dist)) } else { Err(to_err(&e)) }
}

/// `reads_hdist_best` of the packed words `encode_fixed` writes (`ceil(read_len / 32)` words per read), without decoding them.
pub fn reads_hdist_best_packed(words: &[u64], read_len: usize, count: usize, k: usize, queries: &[u64]) -> Result<(Vec<u32>, Vec<u32>, Vec<u8>), NucleotideError> {
    assert!(words.len() >= count * ((read_len + 31) / 32), "count reads of ceil(read_len / 32) words each");
    let (mut query, mut pos, mut dist) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_reads_hdist_best_packed(c, words.as_ptr(), read_len, count, k, queries.as_ptr(), queries.len(), query.as_mut_ptr(), pos.as_mut_ptr(), dist.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok((query, pos, dist)) } else { Err(to_err(&e)) }
}

/// `(query, pos, dist)` of the best match and of the runner-up per read.
pub type ReadsBest2 = ((Vec<u32>, Vec<u32>, Vec<u8>), (Vec<u32>, Vec<u32>, Vec<u8>));

/// The best match per read as `reads_hdist_best`, and the runner-up: the smallest (distance, query, offset) over the queries other than the
/// winner's (a second window of the winning query is never the runner-up; with one query it is `u32::MAX`, `u32::MAX`, `255`).
pub fn reads_hdist_best2(reads: &[u8], read_len: usize, k: usize, queries: &[u64]) -> Result<ReadsBest2, NucleotideError> {
    let count = if read_len == 0 { 0 } else { reads.len() / read_len };
    let (mut query, mut pos, mut dist) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let (mut query2, mut pos2, mut dist2) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_reads_hdist_best2(c, reads.as_ptr(), read_len, count, k, queries.as_ptr(), queries.len(), query.as_mut_ptr(), pos.as_mut_ptr(), dist.as_mut_ptr(),
                                      query2.as_mut_ptr(), pos2.as_mut_ptr(), dist2.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok(((query, pos, dist), (query2, pos2, dist2))) } else { Err(to_err(&e)) }
}

/// `reads_hdist_best2` of the packed words `encode_fixed` writes (`ceil(read_len / 32)` words per read), without decoding them.
pub fn reads_hdist_best2_packed(words: &[u64], read_len: usize, count: usize, k: usize, queries: &[u64]) -> Result<ReadsBest2, NucleotideError> {
    assert!(words.len() >= count * ((read_len + 31) / 32), "count reads of ceil(read_len / 32) words each");
    let (mut query, mut pos, mut dist) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let (mut query2, mut pos2, mut dist2) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_reads_hdist_best2_packed(c, words.as_ptr(), read_len, count, k, queries.as_ptr(), queries.len(), query.as_mut_ptr(), pos.as_mut_ptr(), dist.as_mut_ptr(),
                                             query2.as_mut_ptr(), pos2.as_mut_ptr(), dist2.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok(((query, pos, dist), (query2, pos2, dist2))) } else { Err(to_err(&e)) }
}

/// The best match and the runner-up per read as `reads_hdist_best2`, over the offsets `pos_lo <= i <= min(pos_hi, read_len - k)` only (`pos_hi = None`:
/// to the end of the read; a 3' anchor with slack `w` is `pos_lo = read_len - k - w`, `pos_hi = None`).  The span `hi - pos_lo + k` may not exceed 64
/// bases; only the span's bytes of each read are read and validated.  Positions are offsets in the read.
pub fn reads_hdist_anchored(reads: &[u8], read_len: usize, k: usize, pos_lo: usize, pos_hi: Option<usize>, queries: &[u64]) -> Result<ReadsBest2, NucleotideError> {
    let count = if read_len == 0 { 0 } else { reads.len() / read_len };
    let (mut query, mut pos, mut dist) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let (mut query2, mut pos2, mut dist2) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_reads_hdist_anchored(c, reads.as_ptr(), read_len, count, k, pos_lo, pos_hi.unwrap_or(usize::MAX), queries.as_ptr(), queries.len(), query.as_mut_ptr(),
                                         pos.as_mut_ptr(), dist.as_mut_ptr(), query2.as_mut_ptr(), pos2.as_mut_ptr(), dist2.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok(((query, pos, dist), (query2, pos2, dist2))) } else { Err(to_err(&e)) }
}

/// `reads_hdist_anchored` of the packed words `encode_fixed` writes (`ceil(read_len / 32)` words per read), without decoding them.
pub fn reads_hdist_anchored_packed(words: &[u64], read_len: usize, count: usize, k: usize, pos_lo: usize, pos_hi: Option<usize>, queries: &[u64]) -> Result<ReadsBest2, NucleotideError> {
    assert!(words.len() >= count * ((read_len + 31) / 32), "count reads of ceil(read_len / 32) words each");
    let (mut query, mut pos, mut dist) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let (mut query2, mut pos2, mut dist2) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_reads_hdist_anchored_packed(c, words.as_ptr(), read_len, count, k, pos_lo, pos_hi.unwrap_or(usize::MAX), queries.as_ptr(), queries.len(),
                                                query.as_mut_ptr(), pos.as_mut_ptr(), dist.as_mut_ptr(), query2.as_mut_ptr(), pos2.as_mut_ptr(), dist2.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok(((query, pos, dist), (query2, pos2, dist2))) } else { Err(to_err(&e)) }
}

/// Where the offset range of the ragged anchored calls is counted from: the read's start, or (in bases behind the window) its end.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum Anchor { Start, End }

impl Anchor {
    fn raw(self) -> std::os::raw::c_int { match self { Anchor::Start => ffi::BITNUC_ANCHOR_START, Anchor::End => ffi::BITNUC_ANCHOR_END } }
}

/// `reads_hdist_anchored` of a ragged batch (read `r` is `seq[offsets[r] .. offsets[r + 1])`): `Anchor::Start` admits the offsets
/// `pos_lo <= i <= min(pos_hi, len_r - k)`, `Anchor::End` those with `pos_lo <= len_r - k - i <= pos_hi` (`End, 0, 3`: the last `k` bases with three bases
/// of slack).  `pos_hi - pos_lo + k` may not exceed 64; a read without an admissible window gets the fill.  Positions are offsets from the read's start.
pub fn reads_hdist_anchored_batch(seq: &[u8], offsets: &[u64], k: usize, anchor: Anchor, pos_lo: usize, pos_hi: usize, queries: &[u64]) -> Result<ReadsBest2, NucleotideError> {
    let count = offsets.len().saturating_sub(1);
    assert!(count == 0 || seq.len() as u64 >= offsets[count], "seq holds offsets[count] bases");
    let (mut query, mut pos, mut dist) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let (mut query2, mut pos2, mut dist2) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_reads_hdist_anchored_batch(c, seq.as_ptr(), offsets.as_ptr(), count, k, anchor.raw(), pos_lo, pos_hi, queries.as_ptr(), queries.len(), query.as_mut_ptr(),
                                               pos.as_mut_ptr(), dist.as_mut_ptr(), query2.as_mut_ptr(), pos2.as_mut_ptr(), dist2.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok(((query, pos, dist), (query2, pos2, dist2))) } else { Err(to_err(&e)) }
}

/// `reads_hdist_anchored_batch` of the packed words `encode_batch` writes (read `r`'s words start at `words[word_offsets[r]]`), without decoding them.
pub fn reads_hdist_anchored_batch_packed(words: &[u64], word_offsets: &[u64], offsets: &[u64], k: usize, anchor: Anchor, pos_lo: usize, pos_hi: usize, queries: &[u64]) -> Result<ReadsBest2, NucleotideError> {
    let count = offsets.len().saturating_sub(1);
    assert!(word_offsets.len() == offsets.len(), "one word offset per base offset");
    assert!(count == 0 || words.len() as u64 >= word_offsets[count], "words holds word_offsets[count] words");
    let (mut query, mut pos, mut dist) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let (mut query2, mut pos2, mut dist2) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_reads_hdist_anchored_batch_packed(c, words.as_ptr(), word_offsets.as_ptr(), offsets.as_ptr(), count, k, anchor.raw(), pos_lo, pos_hi, queries.as_ptr(),
                                                      queries.len(), query.as_mut_ptr(), pos.as_mut_ptr(), dist.as_mut_ptr(), query2.as_mut_ptr(), pos2.as_mut_ptr(),
                                                      dist2.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok(((query, pos, dist), (query2, pos2, dist2))) } else { Err(to_err(&e)) }
}

/// The best match per read of a ragged batch: read `r` is `seq[offsets[r] .. offsets[r + 1])` (`offsets` has `count + 1` non-decreasing entries
/// from 0).  `(query, pos, dist)` as `reads_hdist_best`; an empty read or one shorter than `k` gets `u32::MAX`, `u32::MAX`, `255`.
pub fn reads_hdist_best_batch(seq: &[u8], offsets: &[u64], k: usize, queries: &[u64]) -> Result<(Vec<u32>, Vec<u32>, Vec<u8>), NucleotideError> {
    let count = offsets.len().saturating_sub(1);
    assert!(count == 0 || seq.len() as u64 >= offsets[count], "seq holds offsets[count] bases");
    let (mut query, mut pos, mut dist) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_reads_hdist_best_batch(c, seq.as_ptr(), offsets.as_ptr(), count, k, queries.as_ptr(), queries.len(), query.as_mut_ptr(), pos.as_mut_ptr(), dist.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok((query, pos, dist)) } else { Err(to_err(&e)) }
}

/// `reads_hdist_best_batch` of the packed words `encode_batch` writes (read `r`'s words start at `words[word_offsets[r]]`), without decoding them.
pub fn reads_hdist_best_batch_packed(words: &[u64], word_offsets: &[u64], offsets: &[u64], k: usize, queries: &[u64]) -> Result<(Vec<u32>, Vec<u32>, Vec<u8>), NucleotideError> {
    let count = offsets.len().saturating_sub(1);
    assert!(word_offsets.len() == offsets.len(), "one word offset per base offset");
    assert!(count == 0 || words.len() as u64 >= word_offsets[count], "words holds word_offsets[count] words");
    let (mut query, mut pos, mut dist) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_reads_hdist_best_batch_packed(c, words.as_ptr(), word_offsets.as_ptr(), offsets.as_ptr(), count, k, queries.as_ptr(), queries.len(), query.as_mut_ptr(), pos.as_mut_ptr(), dist.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok((query, pos, dist)) } else { Err(to_err(&e)) }
}

/// A pattern query: a set of bases per position (`allow[c]` bit `i` set <=> base code `c` matches at position `i`).
pub use ffi::bitnuc_pattern as Pattern;

/// The pattern of `letters` (IUPAC: `ACGTU RYSWKM BDHV N`, either case; at most 32).  Host code, no context.
pub fn pattern_from_iupac(letters: &[u8]) -> Result<Pattern, NucleotideError> {
    let mut p = Pattern::default();
    let mut e = ffi::bitnuc_err::default();
    let st = unsafe { ffi::bitnuc_pattern_from_iupac(letters.as_ptr(), letters.len(), &mut p, &mut e) };
    if st == ffi::BITNUC_OK { Ok(p) } else { Err(to_err(&e)) }
}

/// The pattern of singletons of the packed exact query `query` of `k` bases: under it the pattern functions return what their exact twins return.
pub fn pattern_from_2bit(query: u64, k: usize) -> Result<Pattern, NucleotideError> {
    let mut p = Pattern::default();
    let mut e = ffi::bitnuc_err::default();
    let st = unsafe { ffi::bitnuc_pattern_from_2bit(query, k, &mut p, &mut e) };
    if st == ffi::BITNUC_OK { Ok(p) } else { Err(to_err(&e)) }
}

/// `reads_hdist_best` under pattern queries: the distance of a window is `pdist`, the number of positions whose base is not in the pattern's set.
/// Ties go to the smallest pattern index, then the smallest offset; an `N` in a read is still an invalid base.
pub fn reads_pattern_best(reads: &[u8], read_len: usize, k: usize, patterns: &[Pattern]) -> Result<(Vec<u32>, Vec<u32>, Vec<u8>), NucleotideError> {
    let count = if read_len == 0 { 0 } else { reads.len() / read_len };
    let (mut query, mut pos, mut dist) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_reads_pattern_best(c, reads.as_ptr(), read_len, count, k, patterns.as_ptr(), patterns.len(), query.as_mut_ptr(), pos.as_mut_ptr(), dist.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok((query, pos, dist)) } else { Err(to_err(&e)) }
}

/// `reads_pattern_best` of the packed words `encode_fixed` writes (`ceil(read_len / 32)` words per read), without decoding them.
pub fn reads_pattern_best_packed(words: &[u64], read_len: usize, count: usize, k: usize, patterns: &[Pattern]) -> Result<(Vec<u32>, Vec<u32>, Vec<u8>), NucleotideError> {
    assert!(words.len() >= count * ((read_len + 31) / 32), "count reads of ceil(read_len / 32) words each");
    let (mut query, mut pos, mut dist) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_reads_pattern_best_packed(c, words.as_ptr(), read_len, count, k, patterns.as_ptr(), patterns.len(), query.as_mut_ptr(), pos.as_mut_ptr(), dist.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok((query, pos, dist)) } else { Err(to_err(&e)) }
}

/// `reads_hdist_best2` under pattern queries: two equal patterns are two queries (the second is the runner-up), another window of the winner never is.
pub fn reads_pattern_best2(reads: &[u8], read_len: usize, k: usize, patterns: &[Pattern]) -> Result<ReadsBest2, NucleotideError> {
    let count = if read_len == 0 { 0 } else { reads.len() / read_len };
    let (mut query, mut pos, mut dist) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let (mut query2, mut pos2, mut dist2) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_reads_pattern_best2(c, reads.as_ptr(), read_len, count, k, patterns.as_ptr(), patterns.len(), query.as_mut_ptr(), pos.as_mut_ptr(), dist.as_mut_ptr(),
                                        query2.as_mut_ptr(), pos2.as_mut_ptr(), dist2.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok(((query, pos, dist), (query2, pos2, dist2))) } else { Err(to_err(&e)) }
}

/// `reads_pattern_best2` of the packed words `encode_fixed` writes, without decoding them.
pub fn reads_pattern_best2_packed(words: &[u64], read_len: usize, count: usize, k: usize, patterns: &[Pattern]) -> Result<ReadsBest2, NucleotideError> {
    assert!(words.len() >= count * ((read_len + 31) / 32), "count reads of ceil(read_len / 32) words each");
    let (mut query, mut pos, mut dist) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let (mut query2, mut pos2, mut dist2) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_reads_pattern_best2_packed(c, words.as_ptr(), read_len, count, k, patterns.as_ptr(), patterns.len(), query.as_mut_ptr(), pos.as_mut_ptr(), dist.as_mut_ptr(),
                                               query2.as_mut_ptr(), pos2.as_mut_ptr(), dist2.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok(((query, pos, dist), (query2, pos2, dist2))) } else { Err(to_err(&e)) }
}

/// `reads_hdist_anchored` under pattern queries (the offsets `pos_lo <= i <= min(pos_hi, read_len - k)`; `pos_hi = None`: to the end of the read).
pub fn reads_pattern_anchored(reads: &[u8], read_len: usize, k: usize, pos_lo: usize, pos_hi: Option<usize>, patterns: &[Pattern]) -> Result<ReadsBest2, NucleotideError> {
    let count = if read_len == 0 { 0 } else { reads.len() / read_len };
    let (mut query, mut pos, mut dist) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let (mut query2, mut pos2, mut dist2) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_reads_pattern_anchored(c, reads.as_ptr(), read_len, count, k, pos_lo, pos_hi.unwrap_or(usize::MAX), patterns.as_ptr(), patterns.len(), query.as_mut_ptr(),
                                           pos.as_mut_ptr(), dist.as_mut_ptr(), query2.as_mut_ptr(), pos2.as_mut_ptr(), dist2.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok(((query, pos, dist), (query2, pos2, dist2))) } else { Err(to_err(&e)) }
}

/// `reads_pattern_anchored` of the packed words `encode_fixed` writes, without decoding them.
pub fn reads_pattern_anchored_packed(words: &[u64], read_len: usize, count: usize, k: usize, pos_lo: usize, pos_hi: Option<usize>, patterns: &[Pattern]) -> Result<ReadsBest2, NucleotideError> {
    assert!(words.len() >= count * ((read_len + 31) / 32), "count reads of ceil(read_len / 32) words each");
    let (mut query, mut pos, mut dist) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let (mut query2, mut pos2, mut dist2) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_reads_pattern_anchored_packed(c, words.as_ptr(), read_len, count, k, pos_lo, pos_hi.unwrap_or(usize::MAX), patterns.as_ptr(), patterns.len(),
                                                  query.as_mut_ptr(), pos.as_mut_ptr(), dist.as_mut_ptr(), query2.as_mut_ptr(), pos2.as_mut_ptr(), dist2.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok(((query, pos, dist), (query2, pos2, dist2))) } else { Err(to_err(&e)) }
}

/// The indel-tolerant anchored match: as `reads_hdist_anchored`, with the EDIT distance of each query to the best substring of the read's span
/// `[pos_lo, min(pos_hi, read_len - k) + k)` (at most 64 bases).  Per read `(query, end, dist)` of the best query and of the runner-up; `end` is an offset
/// in the read, one past the last aligned base (the alignment's start: `bitnuc_reads_edist_start*` of the C ABI, declared in `ffi`).  `dist` is never above `reads_hdist_anchored`'s.
pub fn reads_edist_anchored(reads: &[u8], read_len: usize, k: usize, pos_lo: usize, pos_hi: Option<usize>, queries: &[u64]) -> Result<ReadsBest2, NucleotideError> {
    let count = if read_len == 0 { 0 } else { reads.len() / read_len };
    let (mut query, mut end, mut dist) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let (mut query2, mut end2, mut dist2) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_reads_edist_anchored(c, reads.as_ptr(), read_len, count, k, pos_lo, pos_hi.unwrap_or(usize::MAX), queries.as_ptr(), queries.len(), query.as_mut_ptr(),
                                         end.as_mut_ptr(), dist.as_mut_ptr(), query2.as_mut_ptr(), end2.as_mut_ptr(), dist2.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok(((query, end, dist), (query2, end2, dist2))) } else { Err(to_err(&e)) }
}

/// `reads_edist_anchored` of the packed words `encode_fixed` writes (`ceil(read_len / 32)` words per read), without decoding them.
pub fn reads_edist_anchored_packed(words: &[u64], read_len: usize, count: usize, k: usize, pos_lo: usize, pos_hi: Option<usize>, queries: &[u64]) -> Result<ReadsBest2, NucleotideError> {
    assert!(words.len() >= count * ((read_len + 31) / 32), "count reads of ceil(read_len / 32) words each");
    let (mut query, mut end, mut dist) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let (mut query2, mut end2, mut dist2) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_reads_edist_anchored_packed(c, words.as_ptr(), read_len, count, k, pos_lo, pos_hi.unwrap_or(usize::MAX), queries.as_ptr(), queries.len(),
                                                query.as_mut_ptr(), end.as_mut_ptr(), dist.as_mut_ptr(), query2.as_mut_ptr(), end2.as_mut_ptr(), dist2.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok(((query, end, dist), (query2, end2, dist2))) } else { Err(to_err(&e)) }
}

/// `reads_edist_anchored` under pattern queries: a read base matches query position `i` when it is in the position's set.
pub fn reads_pattern_edist_anchored(reads: &[u8], read_len: usize, k: usize, pos_lo: usize, pos_hi: Option<usize>, patterns: &[Pattern]) -> Result<ReadsBest2, NucleotideError> {
    let count = if read_len == 0 { 0 } else { reads.len() / read_len };
    let (mut query, mut end, mut dist) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let (mut query2, mut end2, mut dist2) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_reads_pattern_edist_anchored(c, reads.as_ptr(), read_len, count, k, pos_lo, pos_hi.unwrap_or(usize::MAX), patterns.as_ptr(), patterns.len(),
                                                 query.as_mut_ptr(), end.as_mut_ptr(), dist.as_mut_ptr(), query2.as_mut_ptr(), end2.as_mut_ptr(), dist2.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok(((query, end, dist), (query2, end2, dist2))) } else { Err(to_err(&e)) }
}

/// `reads_pattern_edist_anchored` of the packed words `encode_fixed` writes, without decoding them.
pub fn reads_pattern_edist_anchored_packed(words: &[u64], read_len: usize, count: usize, k: usize, pos_lo: usize, pos_hi: Option<usize>, patterns: &[Pattern]) -> Result<ReadsBest2, NucleotideError> {
    assert!(words.len() >= count * ((read_len + 31) / 32), "count reads of ceil(read_len / 32) words each");
    let (mut query, mut end, mut dist) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let (mut query2, mut end2, mut dist2) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_reads_pattern_edist_anchored_packed(c, words.as_ptr(), read_len, count, k, pos_lo, pos_hi.unwrap_or(usize::MAX), patterns.as_ptr(), patterns.len(),
                                                        query.as_mut_ptr(), end.as_mut_ptr(), dist.as_mut_ptr(), query2.as_mut_ptr(), end2.as_mut_ptr(), dist2.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok(((query, end, dist), (query2, end2, dist2))) } else { Err(to_err(&e)) }
}

/// `reads_hdist_anchored_batch` under pattern queries.
pub fn reads_pattern_anchored_batch(seq: &[u8], offsets: &[u64], k: usize, anchor: Anchor, pos_lo: usize, pos_hi: usize, patterns: &[Pattern]) -> Result<ReadsBest2, NucleotideError> {
    let count = offsets.len().saturating_sub(1);
    assert!(count == 0 || seq.len() as u64 >= offsets[count], "seq holds offsets[count] bases");
    let (mut query, mut pos, mut dist) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let (mut query2, mut pos2, mut dist2) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_reads_pattern_anchored_batch(c, seq.as_ptr(), offsets.as_ptr(), count, k, anchor.raw(), pos_lo, pos_hi, patterns.as_ptr(), patterns.len(), query.as_mut_ptr(),
                                                 pos.as_mut_ptr(), dist.as_mut_ptr(), query2.as_mut_ptr(), pos2.as_mut_ptr(), dist2.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok(((query, pos, dist), (query2, pos2, dist2))) } else { Err(to_err(&e)) }
}

/// `reads_pattern_anchored_batch` of the packed words `encode_batch` writes, without decoding them.
pub fn reads_pattern_anchored_batch_packed(words: &[u64], word_offsets: &[u64], offsets: &[u64], k: usize, anchor: Anchor, pos_lo: usize, pos_hi: usize, patterns: &[Pattern]) -> Result<ReadsBest2, NucleotideError> {
    let count = offsets.len().saturating_sub(1);
    assert!(word_offsets.len() == offsets.len(), "one word offset per base offset");
    assert!(count == 0 || words.len() as u64 >= word_offsets[count], "words holds word_offsets[count] words");
    let (mut query, mut pos, mut dist) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let (mut query2, mut pos2, mut dist2) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_reads_pattern_anchored_batch_packed(c, words.as_ptr(), word_offsets.as_ptr(), offsets.as_ptr(), count, k, anchor.raw(), pos_lo, pos_hi, patterns.as_ptr(),
                                                        patterns.len(), query.as_mut_ptr(), pos.as_mut_ptr(), dist.as_mut_ptr(), query2.as_mut_ptr(), pos2.as_mut_ptr(),
                                                        dist2.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok(((query, pos, dist), (query2, pos2, dist2))) } else { Err(to_err(&e)) }
}

/// `reads_edist_anchored` of a ragged batch (read `r` is `seq[offsets[r]..offsets[r + 1]]`): the edit distance of each query to the best substring of each
/// read's own span, the bases `reads_hdist_anchored_batch` looks at for the same `(anchor, pos_lo, pos_hi)`; ends count from the read's start.
pub fn reads_edist_anchored_batch(seq: &[u8], offsets: &[u64], k: usize, anchor: Anchor, pos_lo: usize, pos_hi: usize, queries: &[u64]) -> Result<ReadsBest2, NucleotideError> {
    let count = offsets.len().saturating_sub(1);
    assert!(count == 0 || seq.len() as u64 >= offsets[count], "seq holds offsets[count] bases");
    let (mut query, mut end, mut dist) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let (mut query2, mut end2, mut dist2) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_reads_edist_anchored_batch(c, seq.as_ptr(), offsets.as_ptr(), count, k, anchor.raw(), pos_lo, pos_hi, queries.as_ptr(), queries.len(), query.as_mut_ptr(),
                                                 end.as_mut_ptr(), dist.as_mut_ptr(), query2.as_mut_ptr(), end2.as_mut_ptr(), dist2.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok(((query, end, dist), (query2, end2, dist2))) } else { Err(to_err(&e)) }
}

/// `reads_edist_anchored_batch` of the packed words `encode_batch` writes (read `r`'s words start at `words[word_offsets[r]]`), without decoding them.
pub fn reads_edist_anchored_batch_packed(words: &[u64], word_offsets: &[u64], offsets: &[u64], k: usize, anchor: Anchor, pos_lo: usize, pos_hi: usize, queries: &[u64]) -> Result<ReadsBest2, NucleotideError> {
    let count = offsets.len().saturating_sub(1);
    assert!(word_offsets.len() == offsets.len(), "one word offset per base offset");
    assert!(count == 0 || words.len() as u64 >= word_offsets[count], "words holds word_offsets[count] words");
    let (mut query, mut end, mut dist) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let (mut query2, mut end2, mut dist2) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_reads_edist_anchored_batch_packed(c, words.as_ptr(), word_offsets.as_ptr(), offsets.as_ptr(), count, k, anchor.raw(), pos_lo, pos_hi, queries.as_ptr(),
                                                        queries.len(), query.as_mut_ptr(), end.as_mut_ptr(), dist.as_mut_ptr(), query2.as_mut_ptr(), end2.as_mut_ptr(),
                                                        dist2.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok(((query, end, dist), (query2, end2, dist2))) } else { Err(to_err(&e)) }
}

/// `reads_edist_anchored_batch` under pattern queries.
pub fn reads_pattern_edist_anchored_batch(seq: &[u8], offsets: &[u64], k: usize, anchor: Anchor, pos_lo: usize, pos_hi: usize, patterns: &[Pattern]) -> Result<ReadsBest2, NucleotideError> {
    let count = offsets.len().saturating_sub(1);
    assert!(count == 0 || seq.len() as u64 >= offsets[count], "seq holds offsets[count] bases");
    let (mut query, mut end, mut dist) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let (mut query2, mut end2, mut dist2) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_reads_pattern_edist_anchored_batch(c, seq.as_ptr(), offsets.as_ptr(), count, k, anchor.raw(), pos_lo, pos_hi, patterns.as_ptr(), patterns.len(), query.as_mut_ptr(),
                                                 end.as_mut_ptr(), dist.as_mut_ptr(), query2.as_mut_ptr(), end2.as_mut_ptr(), dist2.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok(((query, end, dist), (query2, end2, dist2))) } else { Err(to_err(&e)) }
}

/// `reads_pattern_edist_anchored_batch` of the packed words `encode_batch` writes, without decoding them.
pub fn reads_pattern_edist_anchored_batch_packed(words: &[u64], word_offsets: &[u64], offsets: &[u64], k: usize, anchor: Anchor, pos_lo: usize, pos_hi: usize, patterns: &[Pattern]) -> Result<ReadsBest2, NucleotideError> {
    let count = offsets.len().saturating_sub(1);
    assert!(word_offsets.len() == offsets.len(), "one word offset per base offset");
    assert!(count == 0 || words.len() as u64 >= word_offsets[count], "words holds word_offsets[count] words");
    let (mut query, mut end, mut dist) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let (mut query2, mut end2, mut dist2) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_reads_pattern_edist_anchored_batch_packed(c, words.as_ptr(), word_offsets.as_ptr(), offsets.as_ptr(), count, k, anchor.raw(), pos_lo, pos_hi, patterns.as_ptr(),
                                                        patterns.len(), query.as_mut_ptr(), end.as_mut_ptr(), dist.as_mut_ptr(), query2.as_mut_ptr(), end2.as_mut_ptr(),
                                                        dist2.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok(((query, end, dist), (query2, end2, dist2))) } else { Err(to_err(&e)) }
}

/// `reads_hdist_best_batch` under pattern queries.
pub fn reads_pattern_best_batch(seq: &[u8], offsets: &[u64], k: usize, patterns: &[Pattern]) -> Result<(Vec<u32>, Vec<u32>, Vec<u8>), NucleotideError> {
    let count = offsets.len().saturating_sub(1);
    assert!(count == 0 || seq.len() as u64 >= offsets[count], "seq holds offsets[count] bases");
    let (mut query, mut pos, mut dist) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_reads_pattern_best_batch(c, seq.as_ptr(), offsets.as_ptr(), count, k, patterns.as_ptr(), patterns.len(), query.as_mut_ptr(), pos.as_mut_ptr(), dist.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok((query, pos, dist)) } else { Err(to_err(&e)) }
}

/// `reads_pattern_best_batch` of the packed words `encode_batch` writes, without decoding them.
pub fn reads_pattern_best_batch_packed(words: &[u64], word_offsets: &[u64], offsets: &[u64], k: usize, patterns: &[Pattern]) -> Result<(Vec<u32>, Vec<u32>, Vec<u8>), NucleotideError> {
    let count = offsets.len().saturating_sub(1);
    assert!(word_offsets.len() == offsets.len(), "one word offset per base offset");
    assert!(count == 0 || words.len() as u64 >= word_offsets[count], "words holds word_offsets[count] words");
    let (mut query, mut pos, mut dist) = (vec![0u32; count], vec![0u32; count], vec![0u8; count]);
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_reads_pattern_best_batch_packed(c, words.as_ptr(), word_offsets.as_ptr(), offsets.as_ptr(), count, k, patterns.as_ptr(), patterns.len(), query.as_mut_ptr(), pos.as_mut_ptr(), dist.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok((query, pos, dist)) } else { Err(to_err(&e)) }
}

/// `counts[q]` = the number of windows `j` of `reference` with `pdist(j) = #{ i < k : reference[j+i] not in S_i of patterns[q] } <= taus[q]`, every
/// pattern in one pass (`taus.len()` must equal `patterns.len()`).
pub fn kmer_pattern_count_multi(reference: &[u8], k: usize, patterns: &[Pattern], taus: &[u32]) -> Result<Vec<u64>, NucleotideError> {
    if taus.len() != patterns.len() { return Err(NucleotideError::Unsupported); }
    let mut counts = vec![0u64; patterns.len()];
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_pattern_count_multi(c, reference.as_ptr(), reference.len(), k, patterns.as_ptr(), taus.as_ptr(), patterns.len(), counts.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok(counts) } else { Err(to_err(&e)) }
}

/// `kmer_pattern_count_multi` of the packed sequence `words` holding `n` bases, without decoding it.
pub fn kmer_pattern_count_multi_packed(words: &[u64], n: usize, k: usize, patterns: &[Pattern], taus: &[u32]) -> Result<Vec<u64>, NucleotideError> {
    if taus.len() != patterns.len() { return Err(NucleotideError::Unsupported); }
    let mut counts = vec![0u64; patterns.len()];
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_pattern_count_multi_packed(c, words.as_ptr(), words.len(), n, k, patterns.as_ptr(), taus.as_ptr(), patterns.len(), counts.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok(counts) } else { Err(to_err(&e)) }
}

/// The best match per pattern in one pass: `(pos, dist)` with `dist[q]` = the smallest pdist of a window under `patterns[q]` and `pos[q]` = the leftmost
/// window that attains it (no windows: `u64::MAX` / `0xFF`).
pub fn kmer_pattern_best(reference: &[u8], k: usize, patterns: &[Pattern]) -> Result<(Vec<u64>, Vec<u8>), NucleotideError> {
    let mut pos = vec![0u64; patterns.len()];
    let mut dist = vec![0u8; patterns.len()];
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_pattern_best(c, reference.as_ptr(), reference.len(), k, patterns.as_ptr(), patterns.len(), pos.as_mut_ptr(), dist.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok((pos, dist)) } else { Err(to_err(&e)) }
}

/// `kmer_pattern_best` of the packed sequence `words` holding `n` bases, without decoding it.
pub fn kmer_pattern_best_packed(words: &[u64], n: usize, k: usize, patterns: &[Pattern]) -> Result<(Vec<u64>, Vec<u8>), NucleotideError> {
    let mut pos = vec![0u64; patterns.len()];
    let mut dist = vec![0u8; patterns.len()];
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_pattern_best_packed(c, words.as_ptr(), words.len(), n, k, patterns.as_ptr(), patterns.len(), pos.as_mut_ptr(), dist.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok((pos, dist)) } else { Err(to_err(&e)) }
}

// ---- the indel-tolerant search along a reference: E(j) = the edit distance of a query to the best substring of the reference that ends at base j
// (1 <= j <= n; the substring starts anywhere); `end` is one past the last aligned base, as `reads_edist_anchored`'s.

/// The best match per query by EDIT distance: `(end, dist)` with `dist[q]` = the smallest E(j) of `queries[q]` over the ends j of `reference` and
/// `end[q]` = the smallest j that attains it (`k == 0` or `n < k`: `u64::MAX` / `0xFF`).
pub fn kmer_edist_best(reference: &[u8], k: usize, queries: &[u64]) -> Result<(Vec<u64>, Vec<u8>), NucleotideError> {
    let mut end = vec![0u64; queries.len()];
    let mut dist = vec![0u8; queries.len()];
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_edist_best(c, reference.as_ptr(), reference.len(), k, queries.as_ptr(), queries.len(), end.as_mut_ptr(), dist.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok((end, dist)) } else { Err(to_err(&e)) }
}

/// `kmer_edist_best` of the packed sequence `words` holding `n` bases, without decoding it.
pub fn kmer_edist_best_packed(words: &[u64], n: usize, k: usize, queries: &[u64]) -> Result<(Vec<u64>, Vec<u8>), NucleotideError> {
    let mut end = vec![0u64; queries.len()];
    let mut dist = vec![0u8; queries.len()];
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_edist_best_packed(c, words.as_ptr(), words.len(), n, k, queries.as_ptr(), queries.len(), end.as_mut_ptr(), dist.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok((end, dist)) } else { Err(to_err(&e)) }
}

/// `counts[q]` = the number of ends j of `reference` with E(j) <= `taus[q]` for `queries[q]`: the end positions of approximate occurrences.
pub fn kmer_edist_count_multi(reference: &[u8], k: usize, queries: &[u64], taus: &[u32]) -> Result<Vec<u64>, NucleotideError> {
    if taus.len() != queries.len() { return Err(NucleotideError::Unsupported); }
    let mut counts = vec![0u64; queries.len()];
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_edist_count_multi(c, reference.as_ptr(), reference.len(), k, queries.as_ptr(), taus.as_ptr(), queries.len(), counts.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok(counts) } else { Err(to_err(&e)) }
}

/// `kmer_edist_count_multi` of the packed sequence `words` holding `n` bases, without decoding it.
pub fn kmer_edist_count_multi_packed(words: &[u64], n: usize, k: usize, queries: &[u64], taus: &[u32]) -> Result<Vec<u64>, NucleotideError> {
    if taus.len() != queries.len() { return Err(NucleotideError::Unsupported); }
    let mut counts = vec![0u64; queries.len()];
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_edist_count_multi_packed(c, words.as_ptr(), words.len(), n, k, queries.as_ptr(), taus.as_ptr(), queries.len(), counts.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok(counts) } else { Err(to_err(&e)) }
}

/// The best match per query by EDIT distance: `(end, dist)` with `dist[q]` = the smallest E(j) of `patterns[q]` over the ends j of `reference` and
/// `end[q]` = the smallest j that attains it (`k == 0` or `n < k`: `u64::MAX` / `0xFF`).
pub fn kmer_pattern_edist_best(reference: &[u8], k: usize, patterns: &[Pattern]) -> Result<(Vec<u64>, Vec<u8>), NucleotideError> {
    let mut end = vec![0u64; patterns.len()];
    let mut dist = vec![0u8; patterns.len()];
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_pattern_edist_best(c, reference.as_ptr(), reference.len(), k, patterns.as_ptr(), patterns.len(), end.as_mut_ptr(), dist.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok((end, dist)) } else { Err(to_err(&e)) }
}

/// `kmer_pattern_edist_best` of the packed sequence `words` holding `n` bases, without decoding it.
pub fn kmer_pattern_edist_best_packed(words: &[u64], n: usize, k: usize, patterns: &[Pattern]) -> Result<(Vec<u64>, Vec<u8>), NucleotideError> {
    let mut end = vec![0u64; patterns.len()];
    let mut dist = vec![0u8; patterns.len()];
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_pattern_edist_best_packed(c, words.as_ptr(), words.len(), n, k, patterns.as_ptr(), patterns.len(), end.as_mut_ptr(), dist.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok((end, dist)) } else { Err(to_err(&e)) }
}

/// `counts[q]` = the number of ends j of `reference` with E(j) <= `taus[q]` for `patterns[q]`: the end positions of approximate occurrences.
pub fn kmer_pattern_edist_count_multi(reference: &[u8], k: usize, patterns: &[Pattern], taus: &[u32]) -> Result<Vec<u64>, NucleotideError> {
    if taus.len() != patterns.len() { return Err(NucleotideError::Unsupported); }
    let mut counts = vec![0u64; patterns.len()];
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_pattern_edist_count_multi(c, reference.as_ptr(), reference.len(), k, patterns.as_ptr(), taus.as_ptr(), patterns.len(), counts.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok(counts) } else { Err(to_err(&e)) }
}

/// `kmer_pattern_edist_count_multi` of the packed sequence `words` holding `n` bases, without decoding it.
pub fn kmer_pattern_edist_count_multi_packed(words: &[u64], n: usize, k: usize, patterns: &[Pattern], taus: &[u32]) -> Result<Vec<u64>, NucleotideError> {
    if taus.len() != patterns.len() { return Err(NucleotideError::Unsupported); }
    let mut counts = vec![0u64; patterns.len()];
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_pattern_edist_count_multi_packed(c, words.as_ptr(), words.len(), n, k, patterns.as_ptr(), taus.as_ptr(), patterns.len(), counts.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok(counts) } else { Err(to_err(&e)) }
}

/// The ends j (ascending, one past the last aligned base) of `reference` with E(j) <= `tau` for `query`, and E at each: a first call with cap 0
/// returns their number, a second fills the lists.  Neighbouring ends of a good match are hits too; the list is not collapsed to local minima.
pub fn kmer_edist_hits(reference: &[u8], k: usize, query: u64, tau: u32) -> Result<(Vec<u64>, Vec<u8>), NucleotideError> {
    let mut total = 0u64;
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_edist_hits(c, reference.as_ptr(), reference.len(), k, query, tau, std::ptr::null_mut(), std::ptr::null_mut(), 0, &mut total, &mut e)
    });
    if st != ffi::BITNUC_OK { return Err(to_err(&e)); }
    let mut end = vec![0u64; total as usize];
    let mut dist = vec![0u8; total as usize];
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_edist_hits(c, reference.as_ptr(), reference.len(), k, query, tau, end.as_mut_ptr(), dist.as_mut_ptr(), end.len(), &mut total, &mut e)
    });
    if st == ffi::BITNUC_OK { Ok((end, dist)) } else { Err(to_err(&e)) }
}

/// `kmer_edist_hits` of the packed sequence `words` holding `n` bases, without decoding it.
pub fn kmer_edist_hits_packed(words: &[u64], n: usize, k: usize, query: u64, tau: u32) -> Result<(Vec<u64>, Vec<u8>), NucleotideError> {
    let mut total = 0u64;
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_edist_hits_packed(c, words.as_ptr(), words.len(), n, k, query, tau, std::ptr::null_mut(), std::ptr::null_mut(), 0, &mut total, &mut e)
    });
    if st != ffi::BITNUC_OK { return Err(to_err(&e)); }
    let mut end = vec![0u64; total as usize];
    let mut dist = vec![0u8; total as usize];
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_edist_hits_packed(c, words.as_ptr(), words.len(), n, k, query, tau, end.as_mut_ptr(), dist.as_mut_ptr(), end.len(), &mut total, &mut e)
    });
    if st == ffi::BITNUC_OK { Ok((end, dist)) } else { Err(to_err(&e)) }
}

/// `kmer_edist_hits` under a pattern query.
pub fn kmer_pattern_edist_hits(reference: &[u8], k: usize, pattern: &Pattern, tau: u32) -> Result<(Vec<u64>, Vec<u8>), NucleotideError> {
    let mut total = 0u64;
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_pattern_edist_hits(c, reference.as_ptr(), reference.len(), k, pattern, tau, std::ptr::null_mut(), std::ptr::null_mut(), 0, &mut total, &mut e)
    });
    if st != ffi::BITNUC_OK { return Err(to_err(&e)); }
    let mut end = vec![0u64; total as usize];
    let mut dist = vec![0u8; total as usize];
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_pattern_edist_hits(c, reference.as_ptr(), reference.len(), k, pattern, tau, end.as_mut_ptr(), dist.as_mut_ptr(), end.len(), &mut total, &mut e)
    });
    if st == ffi::BITNUC_OK { Ok((end, dist)) } else { Err(to_err(&e)) }
}

/// `kmer_pattern_edist_hits` of the packed sequence `words` holding `n` bases, without decoding it.
pub fn kmer_pattern_edist_hits_packed(words: &[u64], n: usize, k: usize, pattern: &Pattern, tau: u32) -> Result<(Vec<u64>, Vec<u8>), NucleotideError> {
    let mut total = 0u64;
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_pattern_edist_hits_packed(c, words.as_ptr(), words.len(), n, k, pattern, tau, std::ptr::null_mut(), std::ptr::null_mut(), 0, &mut total, &mut e)
    });
    if st != ffi::BITNUC_OK { return Err(to_err(&e)); }
    let mut end = vec![0u64; total as usize];
    let mut dist = vec![0u8; total as usize];
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_pattern_edist_hits_packed(c, words.as_ptr(), words.len(), n, k, pattern, tau, end.as_mut_ptr(), dist.as_mut_ptr(), end.len(), &mut total, &mut e)
    });
    if st == ffi::BITNUC_OK { Ok((end, dist)) } else { Err(to_err(&e)) }
}

/// The mismatch histogram per pattern in one pass: `hist[q * n_bins + d]` = the number of windows with pdist exactly `d` under `patterns[q]`,
/// `d < n_bins <= 16`.
pub fn kmer_pattern_hist(reference: &[u8], k: usize, patterns: &[Pattern], n_bins: usize) -> Result<Vec<u64>, NucleotideError> {
    let mut hist = vec![0u64; patterns.len() * n_bins.min(ffi::BITNUC_HIST_MAX_BINS)]; // (a refused n_bins writes nothing)
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_pattern_hist(c, reference.as_ptr(), reference.len(), k, patterns.as_ptr(), patterns.len(), n_bins, hist.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok(hist) } else { Err(to_err(&e)) }
}

/// `kmer_pattern_hist` of the packed sequence `words` holding `n` bases, without decoding it.
pub fn kmer_pattern_hist_packed(words: &[u64], n: usize, k: usize, patterns: &[Pattern], n_bins: usize) -> Result<Vec<u64>, NucleotideError> {
    let mut hist = vec![0u64; patterns.len() * n_bins.min(ffi::BITNUC_HIST_MAX_BINS)]; // (a refused n_bins writes nothing)
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_pattern_hist_packed(c, words.as_ptr(), words.len(), n, k, patterns.as_ptr(), patterns.len(), n_bins, hist.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok(hist) } else { Err(to_err(&e)) }
}

/// The positions (ascending) and distances of the windows of `reference` with pdist at most `tau` under `pattern`: a first call with cap 0 returns
/// their number, a second fills the lists.
pub fn kmer_pattern_hits(reference: &[u8], k: usize, pattern: &Pattern, tau: u32) -> Result<(Vec<u64>, Vec<u8>), NucleotideError> {
    let mut total = 0u64;
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_pattern_hits(c, reference.as_ptr(), reference.len(), k, pattern, tau, std::ptr::null_mut(), std::ptr::null_mut(), 0, &mut total, &mut e)
    });
    if st != ffi::BITNUC_OK { return Err(to_err(&e)); }
    let mut pos = vec![0u64; total as usize];
    let mut dist = vec![0u8; total as usize];
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_pattern_hits(c, reference.as_ptr(), reference.len(), k, pattern, tau, pos.as_mut_ptr(), dist.as_mut_ptr(), pos.len(), &mut total, &mut e)
    });
    if st == ffi::BITNUC_OK { Ok((pos, dist)) } else { Err(to_err(&e)) }
}

/// `kmer_pattern_hits` of the packed sequence `words` holding `n` bases, without decoding it.
pub fn kmer_pattern_hits_packed(words: &[u64], n: usize, k: usize, pattern: &Pattern, tau: u32) -> Result<(Vec<u64>, Vec<u8>), NucleotideError> {
    let mut total = 0u64;
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_pattern_hits_packed(c, words.as_ptr(), words.len(), n, k, pattern, tau, std::ptr::null_mut(), std::ptr::null_mut(), 0, &mut total, &mut e)
    });
    if st != ffi::BITNUC_OK { return Err(to_err(&e)); }
    let mut pos = vec![0u64; total as usize];
    let mut dist = vec![0u8; total as usize];
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_kmer_pattern_hits_packed(c, words.as_ptr(), words.len(), n, k, pattern, tau, pos.as_mut_ptr(), dist.as_mut_ptr(), pos.len(), &mut total, &mut e)
    });
    if st == ffi::BITNUC_OK { Ok((pos, dist)) } else { Err(to_err(&e)) }
}

/// `for s in seqs { encode(s, &mut ebuf)? }` in one launch: sequence i =
/// `seq[offsets[i]..offsets[i+1]]`; returns (concatenated words, word_offsets).
pub fn encode_batch(seq: &[u8], offsets: &[u64]) -> Result<(Vec<u64>, Vec<u64>), NucleotideError> {
    let count = offsets.len().saturating_sub(1);
    let cap = if count > 0 { ((offsets[count] - offsets[0]) / 32) as usize + count } else { 0 };
    let mut out = vec![0u64; cap];
    let mut word_offsets = vec![0u64; count + 1];
    let mut n_words = 0usize;
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_encode_batch(c, seq.as_ptr(), offsets.as_ptr(), count, out.as_mut_ptr(), cap,
                                 word_offsets.as_mut_ptr(), &mut n_words, &mut e)
    });
    if st != ffi::BITNUC_OK {
        return Err(to_err(&e));
    }
    out.truncate(n_words);
    Ok((out, word_offsets))
}

/// Inverse of `encode_batch`: sequence i's bases land at `out[offsets[i]..offsets[i+1]]`.
pub fn decode_batch(words: &[u64], word_offsets: &[u64], offsets: &[u64]) -> Result<Vec<u8>, NucleotideError> {
    let count = offsets.len().saturating_sub(1);
    let mut out = vec![0u8; if count > 0 { offsets[count] as usize } else { 0 }];
    let mut e = ffi::bitnuc_err::default();
    let st = with_ctx(|c| unsafe {
        ffi::bitnuc_decode_batch(c, words.as_ptr(), word_offsets.as_ptr(), offsets.as_ptr(), count, out.as_mut_ptr(), &mut e)
    });
    if st == ffi::BITNUC_OK { Ok(out) } else { Err(to_err(&e)) }
}

/// `bitnuc::PackedSequence` (src/sequence.rs:5-262) over GPU-encoded data.
#[derive(Debug, PartialEq, Eq, Clone, Hash)]
pub struct PackedSequence {
    data: Vec<u64>,
    length: usize,
}

impl PackedSequence {
    pub fn new(seq: &[u8]) -> Result<Self, NucleotideError> {
        let mut data = Vec::new();
        if !seq.is_empty() {
            encode(seq, &mut data)?;
        }
        Ok(Self { data, length: seq.len() })
    }
    pub fn len(&self) -> usize {
        self.length
    }
    pub fn is_empty(&self) -> bool {
        self.length == 0
    }
    pub fn get(&self, index: usize) -> Result<u8, NucleotideError> {
        if index >= self.length {
            return Err(NucleotideError::IndexOutOfBounds { index, length: self.length });
        }
        // the reference's shift + mask + match (sequence.rs:121-134): no call into the library
        Ok(b"ACGT"[((self.data[index / 32] >> ((index % 32) * 2)) & 3) as usize])
    }
    pub fn slice(&self, range: std::ops::Range<usize>) -> Result<Vec<u8>, NucleotideError> {
        if range.start > range.end || range.end > self.length {
            return Err(NucleotideError::InvalidRange { start: range.start, end: range.end, length: self.length });
        }
        if range.start == range.end {
            return Ok(Vec::new());
        }
        let (w0, w1) = (range.start / 32, range.end.div_ceil(32));
        let n = self.length.min(w1 * 32) - w0 * 32;
        let mut chunk = Vec::with_capacity(n);
        decode(&self.data[w0..w1], n, &mut chunk)?; // only the words the range touches
        Ok(chunk[range.start - w0 * 32..range.end - w0 * 32].to_vec())
    }
    pub fn to_vec(&self) -> Result<Vec<u8>, NucleotideError> {
        self.slice(0..self.length)
    }
}

/// src/utils/analysis.rs:3-39, evaluated on the packed words on the GPU.
pub trait GCContent {
    fn gc_content(&self) -> f64;
}
pub trait BaseCount {
    fn base_counts(&self) -> [usize; 4];
}
impl BaseCount for PackedSequence {
    fn base_counts(&self) -> [usize; 4] {
        let mut c = [0u64; 4];
        let mut e = ffi::bitnuc_err::default();
        let st = with_ctx(|ctx| unsafe {
            ffi::bitnuc_base_counts(ctx, self.data.as_ptr(), self.data.len(), self.length, c.as_mut_ptr(), &mut e)
        });
        assert!(st == ffi::BITNUC_OK);
        [c[0] as usize, c[1] as usize, c[2] as usize, c[3] as usize]
    }
}
impl GCContent for PackedSequence {
    fn gc_content(&self) -> f64 {
        if self.length == 0 {
            return 0.0;
        }
        let c = self.base_counts();
        ((c[1] + c[2]) as f64 / self.length as f64) * 100.0
    }
}

#[cfg(test)]
mod testing {
    // the reference's own unit tests (src/utils/packing/mod.rs:144-198 etc.) run unchanged
    // against this crate; tests/cpp/test_bitnuc_hpp.cpp holds the compiled C++ twin.
    use super::*;

    #[test]
    fn test_as_2bit_valid_sequence() {
        assert_eq!(as_2bit(b"ACGT").unwrap(), 0b11100100);
        assert!(matches!(as_2bit(b"ACGN"), Err(NucleotideError::InvalidBase(b'N'))));
        assert!(matches!(as_2bit(&vec![b'A'; 33]), Err(NucleotideError::SequenceTooLong(33))));
    }

    #[test]
    fn test_round_trip() {
        let seq = b"ACTGACTGACTGACTGACTGACTGACTGACTGACTGA";
        let mut ebuf = Vec::new();
        encode(seq, &mut ebuf).unwrap();
        let mut out = Vec::new();
        decode(&ebuf, seq.len(), &mut out).unwrap();
        assert_eq!(&out, seq);
    }
}
