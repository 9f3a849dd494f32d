// host_pipe.h -- the two drivers of the host-pointer bulk calls (codec.hip: encode / decode; kmer.hip: k-mer batches, scan;
// batch.hip: fixed-length reads).  Internal (needs HIP); the mover thread it drives is host_pool.h (no HIP, sanitized).
#pragma once
#include "runtime.h"
#include "host_pool.h"

#include <stdlib.h>

#include <atomic>

// ---- host-pointer jobs and their two drivers ---------------------------------------------------------------------------------
// A host-pointer bulk call describes its chunking ONCE, as a Job of `count` items; chunk [i0, i0 + m) copies in_bytes(m) bytes from
// in_src(i0) to a device buffer, launch() works on it on the context's stream, and out_bytes(m) bytes go back to out_dst(i0):
//   size_t count;  int in_kind, out_kind (kBufA / kBufB / kBufC);  bool drains, inout;
//   size_t pipe_per(size_t chunk);  size_t scratch_per();   // items per chunk of either driver (pipe_per 0: no item fits a pipe chunk)
//   const void *in_src(size_t i0); size_t in_bytes(size_t m);  void *out_dst(size_t i0); size_t out_bytes(size_t m);
//   int launch(size_t i0, size_t m, const uint8_t *d_in, uint8_t *d_out, bitnuc_err *err);   // takes its own error slot if it has one
// `drains`: the launches latch data errors (the driver drains the slot ring; otherwise it only waits for the stream).  `inout`: bytes
// of the output that the kernel does not write are the caller's and must come back unchanged, so each output chunk is copied in first.
// Two drivers run a Job: pipe_run (from kPipeMin of input) and scratch_run (smaller inputs, host_pipeline 0, shapes the pipe does
// not take).  Both report the first data error in sequence order.
//
// pipe_run.  On this platform the runtime pins a pageable buffer in place and a pageable hipMemcpyAsync runs at the pinned rate
// (56 GB/s either way, profiles/r03_pageable_copy_rates.txt) -- but it blocks its caller until the copy is done, so one thread gets
// one direction at a time.  So two threads move the data: the CALLING thread copies chunk c straight from the caller's memory to
// device buffer c % depth on s_in and launches on it, the MOVER thread (host_pool.h: TaskThread) waits for kernel c's event and
// copies its output straight into the caller's memory on s_out.  A device buffer pair is reused once the mover has finished the
// chunk that used it (a host-side ticket: by then the kernel has read its input and the copy has left its output), so no other
// guard is needed.  The library's own pinned buffers filled and emptied by pools of copy threads lost to this on four of four
// boxes (round 3's engine A/B, profiles/README.md).
constexpr int kPipeDepth = 3; // device buffer sets in flight: chunk c-2 goes back to the caller while chunk c-1 is worked on and chunk c comes in
constexpr size_t kPipeChunkDefault = (size_t)32 << 20; // bases per chunk; BITNUC_PIPE_CHUNK_MB overrides
constexpr size_t kPipeMin = (size_t)8 << 20;           // inputs below this stay on scratch (latency, not bandwidth, matters there)

// Three kinds of device buffer sets, kPipeDepth of each: A = chunk + 64 bytes (ASCII-sized), B = chunk / 4 + 64 bytes (word-sized),
// C = a second A-sized set that only the scan needs (input AND output are a byte per base); C is allocated on first use.
// scratch_run puts a kind's chunk in c->scratch[kind].
enum { kBufA = 0, kBufB = 1, kBufC = 2 };

struct HostPipe {
    hipStream_t s_in = nullptr, s_out = nullptr;
    hipEvent_t ev_in[kPipeDepth] = {}, ev_k[kPipeDepth] = {};
    uint8_t *dev[3][kPipeDepth] = {};
    bitnuc_host::TaskThread *mover = nullptr; // created on first use
    size_t chunk = kPipeChunkDefault; // bases per chunk (a multiple of 32)
    bool ok = false;
    size_t buf_bytes(int kind) const { return kind == kBufB ? chunk / 4 + 64 : chunk + 64; }
};

namespace bitnuc_rt {

inline void pipe_free(HostPipe *p) {
    if (!p) return;
    delete p->mover; // runs what is still queued, then joins
    for (int kind = 0; kind < 3; ++kind)
        for (int i = 0; i < kPipeDepth; ++i)
            if (p->dev[kind][i]) (void)hipFree(p->dev[kind][i]);
    for (int i = 0; i < kPipeDepth; ++i) {
        if (p->ev_in[i]) (void)hipEventDestroy(p->ev_in[i]);
        if (p->ev_k[i]) (void)hipEventDestroy(p->ev_k[i]);
    }
    if (p->s_in) (void)hipStreamDestroy(p->s_in);
    if (p->s_out) (void)hipStreamDestroy(p->s_out);
    delete p;
}

inline hipError_t pipe_alloc_kind(HostPipe *p, int kind) {
    hipError_t rc = hipSuccess;
    for (int i = 0; i < kPipeDepth && rc == hipSuccess; ++i)
        if (!p->dev[kind][i]) rc = hipMalloc(&p->dev[kind][i], p->buf_bytes(kind));
    return rc;
}

// kinds: bit mask of the buffer sets the caller needs (1 << kBufA | ...); A and B are allocated with the pipe, C on first use
inline int pipe_get(bitnuc_ctx *c, HostPipe **out, bitnuc_err *err, unsigned kinds = (1u << kBufA) | (1u << kBufB)) {
    if (c->pipe && c->pipe->ok) {
        if ((kinds & (1u << kBufC)) && !c->pipe->dev[kBufC][kPipeDepth - 1]) {
            const hipError_t rcC = pipe_alloc_kind(c->pipe, kBufC);
            if (rcC != hipSuccess) return fail_hip(err, rcC);
        }
        *out = c->pipe;
        return BITNUC_OK;
    }
    if (c->pipe) { pipe_free(c->pipe); c->pipe = nullptr; } // a pipe that an aborted call left in an unknown state: rebuild
    HostPipe *p = new HostPipe();
    hipError_t rc = hipStreamCreateWithFlags(&p->s_in, hipStreamNonBlocking);
    if (rc == hipSuccess) rc = hipStreamCreateWithFlags(&p->s_out, hipStreamNonBlocking);
    if (const char *e = getenv("BITNUC_PIPE_CHUNK_MB")) {
        const long v = atol(e);
        if (v >= 1 && v <= 1024) p->chunk = (size_t)v << 20;
    }
    for (int i = 0; i < kPipeDepth && rc == hipSuccess; ++i) {
        rc = hipEventCreateWithFlags(&p->ev_in[i], hipEventDisableTiming);
        if (rc == hipSuccess) rc = hipEventCreateWithFlags(&p->ev_k[i], hipEventDisableTiming);
    }
    if (rc == hipSuccess) rc = pipe_alloc_kind(p, kBufA);
    if (rc == hipSuccess) rc = pipe_alloc_kind(p, kBufB);
    if (rc == hipSuccess && (kinds & (1u << kBufC))) rc = pipe_alloc_kind(p, kBufC);
    if (rc != hipSuccess) { pipe_free(p); return fail_hip(err, rc); }
    p->ok = true;
    c->pipe = p;
    *out = p;
    return BITNUC_OK;
}

// A call that leaves the pipelined loop early (a HIP error mid-loop) must not leave copies, kernels or error slots behind:
// the next call assumes an idle pipe.  Unless dismissed, the guard waits for the three streams and empties the slot ring;
// the pipe is rebuilt by the next call.  Either way nothing is still being written into the caller's memory when it is done.
struct PipeAbort {
    bitnuc_ctx *c;
    HostPipe *p;
    bool dismissed = false;
    ~PipeAbort() {
        p->mover->drain();
        if (dismissed) return;
        (void)hipStreamSynchronize(p->s_in);
        (void)hipStreamSynchronize(p->s_out);
        bitnuc_err e;
        (void)drain(c, &e);
        (void)hipGetLastError();
        p->ok = false;
    }
};

// the end of a job's chunk (scratch_run) or of the whole job (pipe_run): the first data error in launch order = sequence order
template <class Job>
int job_wait(bitnuc_ctx *c, const Job &job, bitnuc_err *e) {
    if (job.drains) return drain(c, e);
    const hipError_t rc = hipStreamSynchronize(c->stream);
    return rc == hipSuccess ? BITNUC_OK : fail_hip(e, rc);
}

// One chunk at a time through context scratch: copy in, launch, copy out, wait, all on the context's stream.  The call stops at
// the first failing chunk (the outputs before it are the caller's).
template <class Job>
int scratch_run(bitnuc_ctx *c, const Job &job, bitnuc_err *err) {
    size_t per = job.scratch_per();
    if (per == 0) per = 1;
    if (per > job.count) per = job.count;
    if (int st = ensure_scratch(c, job.in_kind, job.in_bytes(per) + 16, err)) return st;
    if (int st = ensure_scratch(c, job.out_kind, job.out_bytes(per) + 16, err)) return st;
    uint8_t *d_in = c->scratch[job.in_kind], *d_out = c->scratch[job.out_kind];
    for (size_t i0 = 0; i0 < job.count; i0 += per) {
        const size_t m = job.count - i0 < per ? job.count - i0 : per;
        HIPCHK(hipMemcpyAsync(d_in, job.in_src(i0), job.in_bytes(m), hipMemcpyHostToDevice, c->stream));
        if (job.inout) HIPCHK(hipMemcpyAsync(d_out, job.out_dst(i0), job.out_bytes(m), hipMemcpyHostToDevice, c->stream));
        if (int st = job.launch(i0, m, d_in, d_out, err)) return st;
        HIPCHK(hipMemcpyAsync(job.out_dst(i0), d_out, job.out_bytes(m), hipMemcpyDeviceToHost, c->stream));
        bitnuc_err e;
        if (int st = job_wait(c, job, &e)) { if (err) *err = e; return st; }
    }
    return BITNUC_OK;
}

// The pipelined driver (see the top of this file).  Every chunk runs, one wait at the end: its slots are examined in launch order.
template <class Job>
int pipe_run(bitnuc_ctx *c, const Job &job, bitnuc_err *err) {
    constexpr int D = kPipeDepth;
    HostPipe *p;
    if (int st = pipe_get(c, &p, err, (1u << job.in_kind) | (1u << job.out_kind))) return st;
    const size_t per = job.pipe_per(p->chunk);
    if (per == 0 || job.inout) return scratch_run(c, job, err); // no whole item fits a chunk, or the output has to be copied in
    if (!p->mover) {
        p->mover = new bitnuc_host::TaskThread();
        const int dev = c->device;
        p->mover->post([dev] { (void)hipSetDevice(dev); });
    }
    bitnuc_host::TaskThread &w = *p->mover;
    std::atomic<int> mover_rc{0}; // (declared before the guard: the tasks it waits for write here)
    PipeAbort guard{c, p};
    const uint64_t base = w.tickets(); // all finished: the previous call drained
    for (size_t ci = 0, i0 = 0; i0 < job.count; ++ci, i0 += per) {
        const size_t m = job.count - i0 < per ? job.count - i0 : per;
        const int b = (int)(ci % D);
        if (ci >= (size_t)D) w.wait_done(base + ci - D + 1); // chunk ci-D is with the caller: device buffers b are free
        if (const int rc = mover_rc.load()) return fail_hip(err, (hipError_t)rc);
        const size_t nout = job.out_bytes(m);
        uint8_t *dev_in = p->dev[job.in_kind][b], *dev_out = p->dev[job.out_kind][b];
        HIPCHK(hipMemcpyAsync(dev_in, job.in_src(i0), job.in_bytes(m), hipMemcpyHostToDevice, p->s_in)); // pageable source: back when the copy is done
        HIPCHK(hipEventRecord(p->ev_in[b], p->s_in));
        HIPCHK(hipStreamWaitEvent(c->stream, p->ev_in[b], 0)); // (a caller that passes pinned memory gets a truly asynchronous copy)
        if (int st = job.launch(i0, m, dev_in, dev_out, err)) return st;
        HIPCHK(hipEventRecord(p->ev_k[b], c->stream));
        void *dst = job.out_dst(i0);
        hipStream_t s_out = p->s_out;
        hipEvent_t ev_k = p->ev_k[b];
        w.post([=, &mover_rc] {
            hipError_t e = hipStreamWaitEvent(s_out, ev_k, 0);
            if (e == hipSuccess) e = hipMemcpyAsync(dst, dev_out, nout, hipMemcpyDeviceToHost, s_out);
            if (e == hipSuccess) e = hipStreamSynchronize(s_out);
            if (e != hipSuccess) mover_rc.store((int)e);
        });
    }
    w.drain();
    if (const int rc = mover_rc.load()) return fail_hip(err, (hipError_t)rc);
    bitnuc_err e;
    const int st = job_wait(c, job, &e);
    if (st == BITNUC_BACKEND_ERROR) { if (err) *err = e; return st; }
    guard.dismissed = true; // every stream has been waited for (the copies out by the mover, the kernels by the wait)
    if (st != BITNUC_OK && err) *err = e;
    return st;
}

} // namespace bitnuc_rt
