// imm3_api.cpp -- the C ABI of include/imm3.h but for the run calls: contexts, segments, tables, query creation (validation that
// mirrors the reference's exceptions, predicate folding, batch layout), the getters and what they settle of the last run, and
// aggregation.  The run itself -- imm3_query_run / _run_select / _run_count and the launches they enqueue -- is imm3_run.cpp; which
// plan a projection takes is imm3_planner.cpp.
// Compiled with hipcc for gfx950.  There is NO CPU fallback: without a HIP device every entry point that
// touches data fails with IMM3_ERR_DEVICE.
#include "../../include/imm3.h"
#include "../../include/imm3_diag.h"
#include "imm3_internal.h"
#include "../host/codec.hpp"

#include <algorithm>
#include <cmath>
#include <map>
#include <mutex>
#include <unordered_map>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "imm3_handles.h"
#include "imm3_distinct_plan.h"
#include "imm3_api_internal.h" // (shared with the run, imm3_run.cpp, and the planner, imm3_planner.cpp)

using namespace imm3;

// ---------------------------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------------------------
static thread_local std::string g_err;

int imm3::fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

// ---------------------------------------------------------------------------------------------
// context-level caching allocator (imm3_sync.h: BlockPool, one per context, thread-safe)
// ---------------------------------------------------------------------------------------------
hipError_t imm3::pool_alloc(imm3_ctx *ctx, void **out, size_t bytes) { return (hipError_t)ctx->blocks.alloc(out, bytes); }
void imm3::pool_release(imm3_ctx *ctx, void *p) { ctx->blocks.release(p); }
static void pool_drain(imm3_ctx *ctx) { ctx->blocks.drain(); }

static const char *cond_name(int c) {
    switch (c) {
    case IMM3_MATCH: return "Match";
    case IMM3_STR_RANGE: return "StrRange";
    case IMM3_INT_IN: return "IntIn";
    case IMM3_INT_IN_SET: return "IntInSet";
    case IMM3_NOTMATCH: return "NotMatch";
    case IMM3_EQ: return "EQ";
    case IMM3_GT: return "GT";
    case IMM3_LT: return "LT";
    case IMM3_NOOP: return "NoOp";
    default: return "?";
    }
}

// ---------------------------------------------------------------------------------------------
// library / context
// ---------------------------------------------------------------------------------------------
extern "C" int imm3_abi_version(void) { return IMM3_ABI_VERSION; }
extern "C" const char *imm3_last_error(void) { return g_err.c_str(); }

extern "C" int imm3_device_count(int *count) {
    if (!count) return fail(IMM3_ERR_ARG, "count is null");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail(IMM3_ERR_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    }
    *count = n;
    return IMM3_OK;
}

extern "C" int imm3_ctx_create(int device, void *stream, imm3_ctx **out) {
    if (!out) return fail(IMM3_ERR_ARG, "out is null");
    *out = nullptr;
    int n = 0;
    HIPCHK(hipGetDeviceCount(&n));
    if (n <= 0) return fail(IMM3_ERR_DEVICE, "no HIP device: the immutable3 GPU path has no CPU fallback");
    if (device < 0 || device >= n) return fail(IMM3_ERR_ARG, "device index out of range");
    HIPCHK(hipSetDevice(device));
    std::unique_ptr<imm3_ctx> c(new imm3_ctx());
    c->device = device;
    if (stream) {
        c->stream = (hipStream_t)stream;
    } else {
        HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->own_stream = true;
    }
    *out = c.release();
    return IMM3_OK;
}

void imm3::ctx_retain(imm3_ctx *c) { ref_retain(c->refs); }
void imm3::ctx_release(imm3_ctx *c) {
    if (ref_release(c->refs)) delete c;
}

// a query's device buffers are about to move (or go): every graph that recorded one of its runs points at the old ones
void imm3::graphs_mark_stale(imm3_ctx *ctx, const imm3_query *q) {
    std::lock_guard<std::mutex> g(ctx->mu);
    for (imm3_graph *gr : ctx->graphs)
        if (std::find(gr->queries.begin(), gr->queries.end(), q) != gr->queries.end()) gr->stale = true;
}

// Destroying a context with live segments / tables / queries is allowed (see imm3_handles.h, "Lifetimes"): everything the
// context owns on the device goes now, the struct itself when the last dependant is destroyed.
extern "C" int imm3_ctx_destroy(imm3_ctx *ctx) {
    if (!ctx) return IMM3_OK;
    if (ctx->closed) return fail(IMM3_ERR_STATE, "context destroyed twice");
    (void)hipSetDevice(ctx->device);
    if (ctx->capture) { // an abandoned capture: end it and drop what it recorded.  The imm3_graph was never handed to the
        hipGraph_t g = nullptr; // caller, so nobody else can free it or the context reference it holds
        (void)hipStreamEndCapture(ctx->stream, &g);
        if (g) (void)hipGraphDestroy(g);
        (void)hipGetLastError();
        delete ctx->capture;
        ctx->capture = nullptr;
        if (ctx->gate.owned_by_me()) ctx->gate.end_exclusive();
        ctx_release(ctx); // the reference imm3_ctx_capture_begin took
    }
    // (the caller's contract: no other thread is inside a call on this context or its children while it is destroyed)
    (void)hipStreamSynchronize(ctx->stream);
    std::lock_guard<std::mutex> lk(ctx->mu);
    for (imm3_graph *g : ctx->graphs) { // the handles stay valid (imm3_graph_destroy frees them); what they recorded is gone
        if (g->exec) (void)hipGraphExecDestroy(g->exec);
        if (g->graph) (void)hipGraphDestroy(g->graph);
        g->exec = nullptr;
        g->graph = nullptr;
        g->stale = true;
    }
    ctx->graphs.clear();
    for (auto &r : ctx->pool) {
        (void)hipEventDestroy(r.start);
        (void)hipEventDestroy(r.stop);
    }
    ctx->pool.clear();
    ctx->used = 0;
    ctx->timing = false;
    if (ctx->aux) { (void)hipStreamSynchronize(ctx->aux); (void)hipStreamDestroy(ctx->aux); ctx->aux = nullptr; }
    if (ctx->copy) { (void)hipStreamSynchronize(ctx->copy); (void)hipStreamDestroy(ctx->copy); ctx->copy = nullptr; }
    (void)hipFree(ctx->d_stamps);
    ctx->d_stamps = nullptr;
    ctx->stamp_slots = 0;
    (void)hipFree(ctx->d_xpow8);
    ctx->d_xpow8 = nullptr;
    pool_drain(ctx);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
    ctx->stream = nullptr;
    ctx->closed = true;
    ctx_release(ctx);
    return IMM3_OK;
}

extern "C" int imm3_ctx_sync(imm3_ctx *ctx) {
    CTX_LIVE(ctx);
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (ctx->aux) HIPCHK(hipStreamSynchronize(ctx->aux));
    return IMM3_OK;
}

// ---------------------------------------------------------------------------------------------
// graphs: a recorded sequence of query runs, enqueued with one call (hipGraph)
// ---------------------------------------------------------------------------------------------
extern "C" int imm3_ctx_capture_begin(imm3_ctx *ctx) {
    if (!ctx) return fail(IMM3_ERR_ARG, "ctx is null");
    if (ctx->closed) return fail(IMM3_ERR_STATE, "the context of this handle has been destroyed");
    if (ctx->gate.owned_by_me()) return fail(IMM3_ERR_STATE, "a graph capture is open on this context: only imm3_query_run / imm3_query_run_select and imm3_ctx_capture_end are accepted");
    // exclusive from here to imm3_ctx_capture_end: calls of other threads on this context wait (whatever they enqueued
    // on the capturing stream would be recorded into the graph)
    if (!ctx->gate.begin_exclusive()) return fail(IMM3_ERR_STATE, "imm3_ctx_capture_begin from inside another call on this context");
    hipError_t e = hipSetDevice(ctx->device);
    imm3_graph *g = new imm3_graph();
    g->ctx = ctx;
    if (e == hipSuccess) e = hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeRelaxed);
    if (e != hipSuccess) {
        delete g;
        (void)hipGetLastError();
        ctx->gate.end_exclusive();
        return fail(IMM3_ERR_DEVICE, std::string("hipStreamBeginCapture: ") + hipGetErrorString(e));
    }
    ctx_retain(ctx);
    ctx->capture = g;
    return IMM3_OK;
}

extern "C" int imm3_ctx_capture_end(imm3_ctx *ctx, imm3_graph **out) {
    if (!out) return fail(IMM3_ERR_ARG, "null argument");
    if (!ctx) return fail(IMM3_ERR_ARG, "ctx is null");
    if (ctx->closed) return fail(IMM3_ERR_STATE, "the context of this handle has been destroyed");
    if (!ctx->gate.owned_by_me() || !ctx->capture) return fail(IMM3_ERR_STATE, "no capture is open on this context (begin and end belong to one thread)");
    imm3_graph *g = ctx->capture;
    ctx->capture = nullptr;
    // The recorded runs set the run record of their queries as if they had executed (the plan functions do; capture_note kept a copy
    // for the replays).  Nothing has executed: every query gets back the record it came with, whether the recording succeeded, was
    // refused half way or fails below -- a getter between here and the first launch answers for the last run that executed.
    for (size_t i = 0; i < g->queries.size() && i < g->live.size(); ++i) g->queries[i]->run = g->live[i];
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipStreamEndCapture(ctx->stream, &g->graph);
    if (e == hipSuccess) e = hipGraphInstantiate(&g->exec, g->graph, nullptr, nullptr, 0);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (g->graph) (void)hipGraphDestroy(g->graph);
        delete g;
        ctx->gate.end_exclusive();
        ctx_release(ctx);
        return fail(IMM3_ERR_DEVICE, std::string("graph capture failed: ") + hipGetErrorString(e));
    }
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        ctx->graphs.push_back(g);
    }
    ctx->gate.end_exclusive();
    *out = g;
    return IMM3_OK;
}

extern "C" int imm3_graph_launch(imm3_graph *g) {
    if (!g) return fail(IMM3_ERR_ARG, "graph is null");
    CTX_LIVE(g->ctx);
    {
        std::lock_guard<std::mutex> lk(g->ctx->mu);
        if (g->stale || !g->exec) return fail(IMM3_ERR_STATE, "a query recorded in this graph has been destroyed or has moved its buffers: record the graph again");
    }
    HIPCHK(hipSetDevice(g->ctx->device));
    HIPCHK(hipGraphLaunch(g->exec, g->ctx->stream));
    // A replay is the recorded runs again: every recorded query gets back the run record it had after its recorded run (a getter of a
    // single-pass run then reads THIS replay's status word -- round 3 left `sp_verified` set by an earlier getter, or
    // `ran_single_pass` cleared by an earlier fallback, and a busy or abandoned replay went unnoticed).
    // Two flags describe the groups, not the recorded run, when that run was a select only: the groups an executed imm3_query_run left stay
    // readable behind a replayed imm3_query_run_select (the record of a recording made before that run says "no aggregation"), and an
    // ordered view is valid only if it was when recorded AND is now (imm3_query_set_group_order may have changed the order since).
    for (size_t i = 0; i < g->queries.size() && i < g->states.size(); ++i) {
        imm3_query *q = g->queries[i];
        const QueryRunState before = q->run;
        q->run = g->states[i];
        q->run.sp_verified = false;
        q->run.ran_agg = q->run.ran_agg || before.ran_agg;
        q->run.group_order_valid = q->run.group_order_valid && before.group_order_valid;
    }
    return IMM3_OK;
}

extern "C" int imm3_graph_destroy(imm3_graph *g) {
    if (!g) return IMM3_OK;
    imm3_ctx *ctx = g->ctx;
    imm3::GateScope gate(&ctx->gate);
    if (!ctx->closed) {
        if (ctx->capture) return fail(IMM3_ERR_STATE, "a graph capture is open on this context");
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream); // a launch may still be running
        std::lock_guard<std::mutex> lk(ctx->mu);
        auto &gs = ctx->graphs;
        gs.erase(std::remove(gs.begin(), gs.end(), g), gs.end());
    }
    if (g->exec) (void)hipGraphExecDestroy(g->exec);
    if (g->graph) (void)hipGraphDestroy(g->graph);
    delete g;
    ctx_release(ctx);
    return IMM3_OK;
}

extern "C" int imm3_ctx_stream(imm3_ctx *ctx, void **stream_out) {
    if (!stream_out) return fail(IMM3_ERR_ARG, "null argument");
    CTX_LIVE(ctx);
    *stream_out = (void *)ctx->stream;
    return IMM3_OK;
}

extern "C" int imm3_ctx_set_tuning(imm3_ctx *ctx, int32_t filter_variant, int32_t grid_blocks) {
    CTX_LIVE(ctx);
    ctx->filter_variant = filter_variant;
    ctx->grid_blocks = grid_blocks;
    return IMM3_OK;
}

// Fault injection into the single-pass projection kernel (imm3_diag.h).  The fields travel in every launch's arguments; only the
// tools' build of the kernel (-DIMM3_ABLATE) reads them.
extern "C" int imm3_ctx_inject_fault(imm3_ctx *ctx, int32_t work_group, int32_t span, uint32_t max_polls) {
    CTX_LIVE(ctx);
#ifndef IMM3_ABLATE
    if (work_group >= 0 || max_polls) return fail(IMM3_ERR_STATE, "fault injection exists only in the tools' build of the library (make -C csrc ablate)");
#endif
    ctx->fault_wg = work_group;
    ctx->fault_span = span;
    ctx->fault_max_polls = max_polls;
    return IMM3_OK;
}

// The device's ticket word of the single-pass kernel (0 = free).  Tests put a foreign ticket there to make every launch find the
// device busy, deterministically; imm3_project.hip and run_single_pass say what the word is for.
extern "C" int imm3_ctx_debug_device_lock(imm3_ctx *ctx, uint64_t value, uint64_t *previous) {
    CTX_LIVE(ctx);
#ifndef IMM3_ABLATE
    // (the shipped library does not hand out a way to park every one-launch query of a device, in every context, on its fallback)
    (void)value;
    (void)previous;
    return fail(IMM3_ERR_STATE, "the device-lock hook exists only in the tools' build of the library (make -C csrc ablate)");
#else
    HIPCHK(hipSetDevice(ctx->device));
    unsigned long long *word = nullptr;
    const int rc = single_pass_lock_word(ctx->device, &word);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    unsigned long long old = 0, v = (unsigned long long)value;
    HIPCHK(hipMemcpy(&old, word, sizeof(old), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(word, &v, sizeof(v), hipMemcpyHostToDevice));
    if (previous) *previous = old;
    return IMM3_OK;
#endif
}

extern "C" int imm3_ctx_devclock_enable(imm3_ctx *ctx, int32_t max_launches) {
    CTX_LIVE(ctx);
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    std::lock_guard<std::mutex> lk(ctx->mu);
    (void)hipFree(ctx->d_stamps); // the stamp buffer only: the snappy CRC table and the buffer pool are not this call's to free
    ctx->d_stamps = nullptr;
    ctx->stamp_slots = 0;
    ctx->stamp_used = 0;
    ctx->stamp_grids.clear();
    if (max_launches > 0) {
        void *p = nullptr;
        HIPCHK(hipMalloc(&p, (size_t)max_launches * kMaxFilterGrid * 2 * sizeof(unsigned long long)));
        HIPCHK(hipMemset(p, 0, (size_t)max_launches * kMaxFilterGrid * 2 * sizeof(unsigned long long)));
        HIPCHK(hipStreamSynchronize(nullptr)); // (the memset runs on the null stream and may return early; the context's stream does not wait for that stream)
        ctx->d_stamps = (unsigned long long *)p;
        ctx->stamp_slots = max_launches;
    }
    return IMM3_OK;
}

extern "C" int imm3_ctx_devclock_collect(imm3_ctx *ctx, float *ms_out, int32_t cap, int32_t *n_out) {
    if (!n_out) return fail(IMM3_ERR_ARG, "null argument");
    CTX_LIVE(ctx);
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    std::lock_guard<std::mutex> lk(ctx->mu);
    const int32_t n = ctx->stamp_used;
    std::vector<unsigned long long> h((size_t)kMaxFilterGrid * 2);
    for (int32_t i = 0; i < n && i < cap; ++i) {
        const int32_t g = ctx->stamp_grids[(size_t)i];
        HIPCHK(hipMemcpy(h.data(), ctx->d_stamps + (size_t)i * kMaxFilterGrid * 2, (size_t)g * 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        unsigned long long lo = ~0ULL, hi = 0;
        for (int32_t b = 0; b < g; ++b) { lo = std::min(lo, h[(size_t)2 * b]); hi = std::max(hi, h[(size_t)2 * b + 1]); }
        if (ms_out) ms_out[i] = (float)((double)(hi - lo) / 100000.0); // 100 MHz ticks -> ms
    }
    *n_out = n;
    return IMM3_OK;
}

extern "C" int imm3_ctx_devclock_raw(imm3_ctx *ctx, int32_t launch, uint64_t *out, int32_t n) {
    if (!out || n < 0) return fail(IMM3_ERR_ARG, "null argument");
    CTX_LIVE(ctx);
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (launch < 0 || launch >= ctx->stamp_used) return fail(IMM3_ERR_ARG, "no such launch");
    if (n > kMaxFilterGrid * 2) n = kMaxFilterGrid * 2;
    HIPCHK(hipMemcpy(out, ctx->d_stamps + (size_t)launch * kMaxFilterGrid * 2, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return IMM3_OK;
}

extern "C" int imm3_ctx_measure_read_gbps(imm3_ctx *ctx, uint64_t bytes, int32_t iters, double *gbps) {
    if (!gbps) return fail(IMM3_ERR_ARG, "null argument");
    CTX_LIVE(ctx);
    if (iters < 1) iters = 1;
    HIPCHK(hipSetDevice(ctx->device));
    const int64_t n_tiles = (int64_t)(bytes / (kTileRows * 4));
    if (n_tiles < 1) return fail(IMM3_ERR_ARG, "bytes too small");
    const size_t sz = (size_t)n_tiles * kTileRows * 4;
    void *buf[3] = {nullptr, nullptr, nullptr};
    void *sink = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    for (auto &b : buf) {
        HIPCHK(hipMalloc(&b, sz));
        HIPCHK(hipMemsetAsync(b, 0x11, sz, ctx->stream));
    }
    HIPCHK(hipMalloc(&sink, 64));
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    std::vector<float> ms;
    for (int i = 0; i < iters + 3; ++i) {
        launch_read_stream((const int32_t *)buf[i % 3], n_tiles, (int32_t *)sink, ctx->stream, e0, e1);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventSynchronize(e1));
        float t = 0.f;
        HIPCHK(hipEventElapsedTime(&t, e0, e1));
        if (i >= 3) ms.push_back(t);
    }
    std::sort(ms.begin(), ms.end());
    *gbps = (double)sz / (ms[ms.size() / 2] * 1e-3) / 1e9;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    for (auto &b : buf) (void)hipFree(b);
    (void)hipFree(sink);
    return IMM3_OK;
}

extern "C" int imm3_ctx_timing_enable(imm3_ctx *ctx, int32_t max_records) {
    CTX_LIVE(ctx);
    HIPCHK(hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> lk(ctx->mu);
    while ((int32_t)ctx->pool.size() < max_records) {
        TimingRecord r{};
        HIPCHK(hipEventCreate(&r.start));
        HIPCHK(hipEventCreate(&r.stop));
        ctx->pool.push_back(r);
    }
    ctx->timing = max_records > 0;
    ctx->used = 0;
    return IMM3_OK;
}

extern "C" int imm3_ctx_timing_mask(imm3_ctx *ctx, uint32_t kernel_mask) {
    CTX_LIVE(ctx);
    ctx->timing_mask = kernel_mask;
    return IMM3_OK;
}

extern "C" int imm3_ctx_timing_reset(imm3_ctx *ctx) {
    CTX_LIVE(ctx);
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->used = 0;
    return IMM3_OK;
}

extern "C" int imm3_ctx_timing_collect(imm3_ctx *ctx, int32_t kernel_id, float *ms_out, int32_t cap, int32_t *n_out) {
    if (!n_out) return fail(IMM3_ERR_ARG, "null argument");
    CTX_LIVE(ctx);
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (ctx->aux) HIPCHK(hipStreamSynchronize(ctx->aux));
    std::lock_guard<std::mutex> lk(ctx->mu);
    int32_t n = 0;
    for (size_t i = 0; i < ctx->used; ++i) {
        if (ctx->pool[i].kernel_id != kernel_id) continue;
        if (n < cap && ms_out) {
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, ctx->pool[i].start, ctx->pool[i].stop));
            ms_out[n] = ms;
        }
        ++n;
    }
    *n_out = n;
    return IMM3_OK;
}

// ---------------------------------------------------------------------------------------------
// segment
// ---------------------------------------------------------------------------------------------
static constexpr uint64_t kPad = 16384; // readable slack past every column: a partial last tile is read as a whole (1024 rows x <= 16 B)

// Host ranges pinned in place for asynchronous staging are counted per context: two segments staged from the same buffer
// share one registration, and the range stays pinned until the last of them has finished with it (unpinning it under a
// copy still in flight is an error the runtime reports much later, on an unrelated call).
static bool pin_range(imm3_ctx *ctx, void *p, size_t bytes) {
    std::lock_guard<std::mutex> g(ctx->mu);
    auto it = ctx->pinned.find(p);
    if (it != ctx->pinned.end()) { ++it->second; return true; }
    hipError_t re = hipHostRegister(p, bytes, hipHostRegisterDefault);
    if (re != hipSuccess) { (void)hipGetLastError(); re = hipHostRegister(p, bytes, hipHostRegisterReadOnly); }
    if (re != hipSuccess) { (void)hipGetLastError(); return false; }
    ctx->pinned[p] = 1;
    return true;
}
static void unpin_range(imm3_ctx *ctx, void *p) {
    std::lock_guard<std::mutex> g(ctx->mu);
    auto it = ctx->pinned.find(p);
    if (it == ctx->pinned.end()) return;
    if (--it->second == 0) {
        if (hipHostUnregister(p) != hipSuccess) (void)hipGetLastError();
        ctx->pinned.erase(it);
    }
}

// last reference gone: free the columns (hipFree waits for the device by itself) and let go of the context
static void segment_free(imm3_segment *seg) {
    if (!seg) return;
    if (seg->ctx) (void)hipSetDevice(seg->ctx->device);
    for (auto &c : seg->cols) {
        if (c.owned && c.d_data) (void)hipFree(c.d_data);
        if (c.d_block_off) (void)hipFree(c.d_block_off);
        if (c.d_row_base) (void)hipFree(c.d_row_base);
        if (c.d_dense) (void)hipFree(c.d_dense);
        if (c.d_hi16) (void)hipFree(c.d_hi16);
    }
    for (auto &kv : seg->d_sample_ptrs) (void)hipFree(kv.second);
    (void)hipFree(seg->d_sample_rows);
    if (seg->ctx) for (void *p : seg->registered) unpin_range(seg->ctx, p);
    if (seg->ready) (void)hipEventDestroy(seg->ready);
    if (seg->ctx) ctx_release(seg->ctx);
    delete seg;
}
static void segment_retain(const imm3_segment *seg) { const_cast<imm3_segment *>(seg)->refs.fetch_add(1, std::memory_order_relaxed); }
static void segment_release(const imm3_segment *cseg) {
    imm3_segment *seg = const_cast<imm3_segment *>(cseg);
    if (seg->refs.fetch_sub(1, std::memory_order_acq_rel) == 1) segment_free(seg);
}

// PFOR_INT column: the rows of a block are not implied by its byte length; read the count word of every block
// (PFORCodec.scala:19-31 -> compressed(0) = input.length) and index the blocks for the kernels.
static int pfor_index(imm3_ctx *ctx, imm3_segment *seg, SegCol &sc) {
    if (sc.width != 4) return fail(IMM3_ERR_ARG, "width does not match codec");
    const size_t nb = sc.offsets.empty() ? 0 : sc.offsets.size() - 1;
    std::vector<uint32_t> off(nb + 1, 0u);
    for (size_t k = 0; k <= nb && !sc.offsets.empty(); ++k) {
        const int64_t o = sc.offsets[k];
        if (o < 0 || (uint64_t)o > sc.bytes || (o & 3) || (k > 0 && o < sc.offsets[k - 1]))
            return fail(IMM3_ERR_LAYOUT, "PFOR_INT block " + std::to_string(k) + ": offsets must ascend in whole 4-byte words within the segment data");
        off[k] = (uint32_t)o;
    }
    void *p = nullptr;
    HIPCHK(hipMalloc(&p, (nb + 1) * sizeof(uint32_t)));
    sc.d_block_off = (uint32_t *)p;
    HIPCHK(hipMalloc(&p, (nb + 1) * sizeof(uint32_t)));
    sc.d_row_base = (uint32_t *)p;
    seg->device_bytes += 2 * (nb + 1) * sizeof(uint32_t);
    HIPCHK(hipMemcpyAsync(sc.d_block_off, off.data(), (nb + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    sc.block_rows.assign(nb, 0);
    if (nb) {
        int32_t *d_counts = nullptr;
        HIPCHK(hipMalloc(&p, nb * sizeof(int32_t)));
        d_counts = (int32_t *)p;
        launch_pfor_counts(sc.d_data, sc.d_block_off, (int64_t)nb, d_counts, ctx->stream);
        const hipError_t e1 = hipGetLastError();
        const hipError_t e2 = hipMemcpyAsync(sc.block_rows.data(), d_counts, nb * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream);
        const hipError_t e3 = hipStreamSynchronize(ctx->stream);
        (void)hipFree(d_counts);
        HIPCHK(e1);
        HIPCHK(e2);
        HIPCHK(e3);
    }
    std::vector<uint32_t> base(nb + 1, 0u);
    int64_t rows = 0;
    sc.tile_aligned = true;
    for (size_t k = 0; k < nb; ++k) {
        const int64_t n = sc.block_rows[k];
        const int64_t words = ((int64_t)off[k + 1] - (int64_t)off[k]) / 4;
        // a block of n values needs at least the count word (+ n / 32 mini-blocks may all have width 0)
        if (n < 0 || words < 1) return fail(IMM3_ERR_LAYOUT, "PFOR_INT block " + std::to_string(k) + " is malformed (no count word)");
        if (k + 1 < nb && n != kTileRows) sc.tile_aligned = false;
        if (n > kTileRows) sc.tile_aligned = false;
        base[k] = (uint32_t)rows;
        rows += n;
        if (rows > 0xFFFFFFFFLL) return fail(IMM3_ERR_LAYOUT, "segment too large");
    }
    base[nb] = (uint32_t)rows;
    sc.rows = rows;
    HIPCHK(hipMemcpyAsync(sc.d_row_base, base.data(), (nb + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return IMM3_OK;
}

// Snappy-coded column: a block's rows = the uncompressed bytes its chunks declare / width (k_snappy_sizes walks the
// chunk headers); also sizes the LDS windows k_snappy_decode needs.
static constexpr int32_t kSnappyLdsBudget = 64 * 1024 - 1024; // staged block + one chunk (the CRC table takes 1 KiB)

static int snappy_index(imm3_ctx *ctx, imm3_segment *seg, SegCol &sc) {
    const size_t nb = sc.offsets.empty() ? 0 : sc.offsets.size() - 1;
    std::vector<uint32_t> off(nb + 1, 0u);
    uint32_t biggest_block = 0;
    for (size_t k = 0; k <= nb && !sc.offsets.empty(); ++k) {
        const int64_t o = sc.offsets[k];
        if (o < 0 || (uint64_t)o > sc.bytes || (k > 0 && o < sc.offsets[k - 1]))
            return fail(IMM3_ERR_LAYOUT, "snappy block " + std::to_string(k) + ": offsets must ascend within the segment data");
        off[k] = (uint32_t)o;
        if (k > 0) biggest_block = std::max(biggest_block, off[k] - off[k - 1]);
    }
    void *p = nullptr;
    HIPCHK(hipMalloc(&p, (nb + 1) * sizeof(uint32_t)));
    sc.d_block_off = (uint32_t *)p;
    HIPCHK(hipMalloc(&p, (nb + 1) * sizeof(uint32_t)));
    sc.d_row_base = (uint32_t *)p;
    seg->device_bytes += 2 * (nb + 1) * sizeof(uint32_t);
    HIPCHK(hipMemcpyAsync(sc.d_block_off, off.data(), (nb + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    std::vector<uint32_t> sizes(nb, 0u);
    uint32_t max_chunk = 0;
    if (nb) {
        HIPCHK(hipMalloc(&p, (nb + 1) * sizeof(uint32_t)));
        uint32_t *d_sizes = (uint32_t *)p; // [nb] = the largest chunk
        hipError_t e = hipMemsetAsync(d_sizes + nb, 0, sizeof(uint32_t), ctx->stream);
        if (e == hipSuccess) {
            launch_snappy_sizes(sc.d_data, sc.d_block_off, (int64_t)nb, d_sizes, d_sizes + nb, ctx->stream);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(sizes.data(), d_sizes, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(&max_chunk, d_sizes + nb, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        (void)hipFree(d_sizes);
        HIPCHK(e);
    }
    std::vector<uint32_t> base(nb + 1, 0u);
    sc.block_rows.assign(nb, 0);
    int64_t rows = 0;
    for (size_t k = 0; k < nb; ++k) {
        if (sizes[k] == 0xFFFFFFFFu) return fail(IMM3_ERR_LAYOUT, "snappy block " + std::to_string(k) + " is malformed (stream header, chunk header or length preamble)");
        if (sizes[k] % (uint32_t)sc.width) return fail(IMM3_ERR_LAYOUT, "snappy block " + std::to_string(k) + ": uncompressed length is not a multiple of the value width");
        sc.block_rows[k] = (int32_t)(sizes[k] / (uint32_t)sc.width);
        base[k] = (uint32_t)rows;
        rows += sc.block_rows[k];
        if (rows > 0xFFFFFFFFLL) return fail(IMM3_ERR_LAYOUT, "segment too large");
    }
    base[nb] = (uint32_t)rows;
    sc.rows = rows;
    sc.tile_aligned = false;
    sc.in_cap = (int32_t)((biggest_block + 3 + 8 + 15) & ~15u);
    sc.out_cap = (int32_t)((std::max<uint32_t>(max_chunk, 16) + 15) & ~15u);
    if (sc.in_cap + sc.out_cap > kSnappyLdsBudget)
        return fail(IMM3_ERR_LAYOUT, "snappy block of " + std::to_string(biggest_block) + " stored bytes does not fit the GPU decoder's LDS window (stored block + largest chunk <= 63 KiB)");
    HIPCHK(hipMemcpyAsync(sc.d_row_base, base.data(), (nb + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return IMM3_OK;
}

// x^(8 n) mod the CRC-32C polynomial (reflected) for n = 0 .. 32768: moves a slice's CRC past the bytes after it
static int ensure_xpow8(imm3_ctx *ctx) {
    std::lock_guard<std::mutex> g(ctx->mu);
    if (ctx->d_xpow8) return IMM3_OK;
    std::vector<uint32_t> t(32769);
    uint32_t c = 0x80000000u; // x^0
    for (size_t n = 0; n < t.size(); ++n) {
        t[n] = c;
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0x82F63B78u & (0u - (c & 1u))); // times x^8 = one zero byte
    }
    void *p = nullptr;
    HIPCHK(hipMalloc(&p, t.size() * sizeof(uint32_t)));
    const hipError_t e = hipMemcpy(p, t.data(), t.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(p); HIPCHK(e); }
    ctx->d_xpow8 = (uint32_t *)p;
    return IMM3_OK;
}

// The decoded (dense, fixed-width) form of a PFOR_INT / snappy column, made once per segment on first need.
static int ensure_dense(imm3_ctx *ctx, const imm3_segment *cseg, int32_t col) {
    imm3_segment *seg = const_cast<imm3_segment *>(cseg);
    SegCol &sc = seg->cols[(size_t)col];
    if (!is_compressed(sc.codec)) return IMM3_OK;
    if (is_snappy(sc.codec)) {
        const int xrc = ensure_xpow8(ctx);
        if (xrc) return xrc;
    }
    std::lock_guard<std::mutex> g(seg->decode_mu);
    if (sc.d_dense) return IMM3_OK;
    void *p = nullptr;
    const size_t bytes = (size_t)sc.rows * (size_t)sc.width + kPad;
    HIPCHK(hipMalloc(&p, bytes));
    uint32_t *d_status = nullptr;
    void *ps = nullptr;
    hipError_t e = hipMalloc(&ps, sizeof(uint32_t));
    if (e != hipSuccess) { (void)hipFree(p); HIPCHK(e); }
    d_status = (uint32_t *)ps;
    uint32_t status = 0;
    PforArgs a;
    std::memset(&a, 0, sizeof(a));
    a.data = sc.d_data;
    a.block_off = sc.d_block_off;
    a.row_base = sc.d_row_base;
    a.n_blocks = (int64_t)sc.block_rows.size();
    a.out = (int32_t *)p;
    a.status = d_status;
    e = hipMemsetAsync(d_status, 0, sizeof(uint32_t), ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync((uint8_t *)p + (size_t)sc.rows * (size_t)sc.width, 0, kPad, ctx->stream);
    if (e == hipSuccess && a.n_blocks > 0 && sc.codec == IMM3_PFOR_INT) {
        LaunchTimer t(ctx, 5);
        const int64_t want = (a.n_blocks + kWavesPerBlock - 1) / kWavesPerBlock;
        launch_pfor_decode(a, (int)std::min<int64_t>(want, 2048), ctx->stream, t.start, t.stop);
        e = hipGetLastError();
    } else if (e == hipSuccess && a.n_blocks > 0) {
        SnappyArgs sa;
        std::memset(&sa, 0, sizeof(sa));
        sa.data = sc.d_data;
        sa.block_off = sc.d_block_off;
        sa.row_base = sc.d_row_base;
        sa.xpow8 = ctx->d_xpow8;
        sa.n_blocks = a.n_blocks;
        sa.width = sc.width;
        sa.in_cap = sc.in_cap;
        sa.out_cap = sc.out_cap;
        sa.out = (uint8_t *)p;
        sa.status = d_status;
        LaunchTimer t(ctx, 5);
        // one wave per work-group; LDS per group decides how many are resident: ask for up to 16 per CU
        launch_snappy_decode(sa, (int)std::min<int64_t>(sa.n_blocks, 4096), ctx->stream, t.start, t.stop);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&status, d_status, sizeof(status), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    (void)hipFree(d_status);
    if (e != hipSuccess || status) {
        (void)hipFree(p);
        HIPCHK(e);
        return fail(IMM3_ERR_LAYOUT, sc.codec == IMM3_PFOR_INT ? "malformed PFOR_INT block (width above 32, data past the block end, or count mismatch)"
                                                              : "malformed snappy block (bad element, length mismatch or CRC-32C mismatch)");
    }
    sc.d_dense = (uint8_t *)p;
    seg->device_bytes += bytes;
    return IMM3_OK;
}

// The 16-bit high-half plane of a DENSE_INT column (SegCol::d_hi16), made once per segment the first time a query's plan wants it,
// as the decoded form above is: under the segment's mutex, on the context's stream (the caller has made that stream wait for an
// asynchronously created segment: segment_await), never in a run.  One kernel reads the column, writes the plane and reduces the
// halves' span; a column spanning fewer than kHi16MinSpan halves gives its plane back and is remembered as having none, and so is one
// whose plane could not be allocated -- neither is an error, the int32 scan stays.  While a graph capture is open nothing is built
// (the host has to wait for the span): the question stays open for the next query.
static int ensure_hi16(imm3_ctx *ctx, const imm3_segment *cseg, int32_t col) {
    imm3_segment *seg = const_cast<imm3_segment *>(cseg);
    SegCol &sc = seg->cols[(size_t)col];
    if (sc.codec != IMM3_DENSE_INT || sc.width != 4) return IMM3_OK;
    std::lock_guard<std::mutex> g(seg->decode_mu);
    if (sc.hi16_state != 0 || ctx->capture) return IMM3_OK;
    const int64_t rows = (int64_t)(sc.bytes / 4);
    const size_t bytes = (size_t)rows * 2 + kPad; // (the column's own slack: a tile's loads never leave the allocation)
    void *p = nullptr, *pm = nullptr;
    if (rows < 1 || hipMalloc(&p, bytes) != hipSuccess || hipMalloc(&pm, 2 * sizeof(int32_t)) != hipSuccess) {
        (void)hipGetLastError();
        if (p) (void)hipFree(p);
        sc.hi16_state = -1;
        return IMM3_OK;
    }
    int32_t min_max[2] = {32767, -32768};
    hipError_t e = hipMemcpyAsync(pm, min_max, sizeof(min_max), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync((uint8_t *)p + (size_t)rows * 2, 0, kPad, ctx->stream);
    if (e == hipSuccess) {
        LaunchTimer t(ctx, 5);
        launch_hi16_build((const int32_t *)sc.d_data, (int16_t *)p, rows, (int32_t *)pm, ctx->stream, t.start, t.stop);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(min_max, pm, sizeof(min_max), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    (void)hipFree(pm);
    if (e != hipSuccess) {
        (void)hipFree(p);
        HIPCHK(e);
    }
    sc.hi16_min = min_max[0];
    sc.hi16_max = min_max[1];
    if (!hi16_span_ok(min_max[0], min_max[1])) {
        (void)hipFree(p);
        sc.hi16_state = -1;
        return IMM3_OK;
    }
    sc.d_hi16 = (uint8_t *)p;
    sc.hi16_state = 1;
    seg->device_bytes += bytes;
    return IMM3_OK;
}

// the query stream must not touch a segment's columns before their copies have landed
static int segment_await(imm3_ctx *ctx, const imm3_segment *seg) {
    if (seg->ready_pending.load(std::memory_order_acquire)) HIPCHK(hipStreamWaitEvent(ctx->stream, seg->ready, 0));
    return IMM3_OK;
}

// Staging: the columns are copied on the context's COPY stream (pageable host memory goes over PCIe at the link rate on
// this platform -- 55-56 GB/s, the same as pinned or registered memory: tools/h2d_probe.py -- so there is nothing to gain
// from bounce buffers; what matters is that staging never occupies or synchronises the query stream).  async = false:
// returns when the host buffers have been consumed; async = true: returns at once, imm3_segment_wait() ends the
// caller's obligation to keep them mapped.
static int segment_build(imm3_ctx *ctx, const imm3_column *cols, int32_t ncols, bool wrap, imm3_segment **out, bool async = false) {
    if (!out) return fail(IMM3_ERR_ARG, "null argument");
    *out = nullptr;
    CTX_LIVE(ctx);
    if (ncols <= 0 || !cols) return fail(IMM3_ERR_ARG, "a segment needs at least one column");
    HIPCHK(hipSetDevice(ctx->device));
    std::unique_ptr<imm3_segment, void (*)(imm3_segment *)> seg(new imm3_segment(), segment_free);
    seg->ctx = ctx;
    ctx_retain(ctx);
    seg->cols.resize((size_t)ncols);
    if (!wrap) {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (!ctx->copy) HIPCHK(hipStreamCreateWithFlags(&ctx->copy, hipStreamNonBlocking));
    }
    bool any_compressed = false;
    for (int32_t i = 0; i < ncols; ++i) any_compressed |= is_compressed(cols[i].codec);
    for (int32_t i = 0; i < ncols; ++i) {
        const imm3_column &c = cols[i];
        SegCol &s = seg->cols[(size_t)i];
        if (c.width <= 0) return fail(IMM3_ERR_ARG, "column width must be positive");
        if (c.n_offsets < 0 || (c.n_offsets > 0 && !c.block_offsets)) return fail(IMM3_ERR_ARG, "bad block offset table");
        if (c.dat_bytes > 0 && !c.dat) return fail(IMM3_ERR_ARG, "column data pointer is null");
        s.codec = c.codec;
        s.vcodec = value_codec(c.codec);
        s.width = c.width;
        s.bytes = c.dat_bytes;
        s.offsets.assign(c.block_offsets, c.block_offsets + c.n_offsets);
        if (wrap) {
            if ((uintptr_t)c.dat & 15) return fail(IMM3_ERR_ARG, "wrapped device columns must be 16-byte aligned");
            s.d_data = (uint8_t *)c.dat;
            s.owned = false;
        } else {
            void *p = nullptr;
            HIPCHK(hipMalloc(&p, c.dat_bytes + kPad));
            s.d_data = (uint8_t *)p;
            s.owned = true;
            seg->device_bytes += c.dat_bytes + kPad;
            if (c.dat_bytes && async && !any_compressed) {
                // hipMemcpyAsync from pageable memory blocks the host for the whole copy; pinned IN PLACE (~4 ms per 400 MB,
                // against 7 ms for the copy itself) it returns at once.  A range that cannot be pinned is copied the blocking way.
                if (pin_range(ctx, (void *)c.dat, c.dat_bytes)) seg->registered.push_back((void *)c.dat);
            }
            if (c.dat_bytes) HIPCHK(hipMemcpyAsync(s.d_data, c.dat, c.dat_bytes, hipMemcpyHostToDevice, ctx->copy));
            HIPCHK(hipMemsetAsync(s.d_data + c.dat_bytes, 0, kPad, ctx->copy));
        }
    }
    if (!wrap) {
        HIPCHK(hipEventCreateWithFlags(&seg->ready, hipEventDisableTiming));
        HIPCHK(hipEventRecord(seg->ready, ctx->copy));
        seg->ready_pending.store(true, std::memory_order_release);
        if (!async || any_compressed) { // host buffers may be unmapped after we return: wait for the COPY stream only
            HIPCHK(hipStreamSynchronize(ctx->copy));
            seg->ready_pending.store(false, std::memory_order_release);
        }
    }
    for (auto &sc : seg->cols) {
        if (!is_compressed(sc.codec)) continue;
        const int rc = sc.codec == IMM3_PFOR_INT ? pfor_index(ctx, seg.get(), sc) : snappy_index(ctx, seg.get(), sc);
        if (rc) return rc;
    }
    *out = seg.release();
    return IMM3_OK;
}

extern "C" int imm3_segment_create(imm3_ctx *ctx, const imm3_column *cols, int32_t ncols, imm3_segment **out) {
    return segment_build(ctx, cols, ncols, false, out);
}
extern "C" int imm3_segment_wrap_device(imm3_ctx *ctx, const imm3_column *cols, int32_t ncols, imm3_segment **out) {
    return segment_build(ctx, cols, ncols, true, out);
}
extern "C" int imm3_segment_create_async(imm3_ctx *ctx, const imm3_column *cols, int32_t ncols, imm3_segment **out) {
    return segment_build(ctx, cols, ncols, false, out, true);
}
extern "C" int imm3_segment_wait(imm3_segment *seg) {
    if (!seg) return fail(IMM3_ERR_ARG, "segment is null");
    if (seg->ready_pending.load(std::memory_order_acquire)) {
        HIPCHK(hipSetDevice(seg->ctx->device));
        HIPCHK(hipEventSynchronize(seg->ready));
        seg->ready_pending.store(false, std::memory_order_release);
    }
    for (void *p : seg->registered) unpin_range(seg->ctx, p);
    seg->registered.clear();
    return IMM3_OK;
}

extern "C" int imm3_segment_destroy(imm3_segment *seg) {
    if (!seg) return IMM3_OK;
    if (seg->closed) return fail(IMM3_ERR_STATE, "segment destroyed twice");
    imm3_ctx *ctx = seg->ctx;
    ctx_retain(ctx); // (the gate lives in the context)
    struct Unref { imm3_ctx *c; ~Unref() { ctx_release(c); } } unref{ctx};
    imm3::GateScope gate(&ctx->gate);
    if (!ctx->closed && ctx->capture) return fail(IMM3_ERR_STATE, "a graph capture is open on this context");
    seg->closed = true;
    if (!seg->ctx->closed) { // (a destroyed context has already drained its streams)
        (void)hipSetDevice(seg->ctx->device);
        if (seg->ready_pending.load()) (void)hipEventSynchronize(seg->ready);
        (void)hipStreamSynchronize(seg->ctx->stream);
    }
    for (void *p : seg->registered) unpin_range(seg->ctx, p); // the caller may unmap its buffers after destroy
    seg->registered.clear();
    segment_release(seg); // tables / queries built on it keep the columns alive until they are destroyed
    return IMM3_OK;
}

// diagnostics (include/imm3_diag.h): the plane as the build kernel wrote it, and the span it reduced
extern "C" int imm3_segment_hi16_plane(const imm3_segment *seg, int32_t col, int16_t *out, int64_t cap_rows, int32_t *state, int32_t *min_max) {
    if (!seg || !state || !min_max || col < 0 || (size_t)col >= seg->cols.size()) return fail(IMM3_ERR_ARG, "bad argument");
    const SegCol &sc = seg->cols[(size_t)col];
    *state = sc.hi16_state;
    min_max[0] = sc.hi16_min;
    min_max[1] = sc.hi16_max;
    if (sc.hi16_state == 1 && out) {
        const int64_t rows = (int64_t)(sc.bytes / 4);
        HIPCHK(hipMemcpy(out, sc.d_hi16, (size_t)(rows < cap_rows ? rows : cap_rows) * sizeof(int16_t), hipMemcpyDeviceToHost));
    }
    return IMM3_OK;
}

extern "C" int imm3_segment_bytes(const imm3_segment *seg, uint64_t *device_bytes) {
    if (!seg || !device_bytes) return fail(IMM3_ERR_ARG, "null argument");
    *device_bytes = seg->device_bytes;
    return IMM3_OK;
}

// ---------------------------------------------------------------------------------------------
// query planning
// ---------------------------------------------------------------------------------------------
static void table_release(const imm3_table *t);

static void query_free(imm3_query *q) {
    if (!q) return;
    imm3_ctx *ctx = q->ctx;
    if (!ctx) { delete q; return; }
    (void)hipSetDevice(ctx->device);
    // no synchronisation: every buffer goes back to the context's pool and is only ever reused in stream order
    if (ctx->aux && q->total_on_aux) (void)hipStreamSynchronize(ctx->aux);
    pool_release(ctx, q->d_bitmap);
    pool_release(ctx, q->d_tile_offsets);
    pool_release(ctx, q->d_chunk_sums);
    pool_release(ctx, q->d_block_partials);
    pool_release(ctx, q->d_limit_state);
    pool_release(ctx, q->d_total);
    pool_release(ctx, q->d_word_row_base);
    pool_release(ctx, q->d_word_nvalid);
    pool_release(ctx, q->d_row_index);
    for (auto p : q->d_proj) pool_release(ctx, p);
    for (int b = 0; b < 2; ++b) { pool_release(ctx, q->d_order_keys[b]); pool_release(ctx, q->d_order_perm[b]); }
    pool_release(ctx, q->d_order_state); pool_release(ctx, q->d_order_counts); pool_release(ctx, q->d_order_diff); pool_release(ctx, q->d_order_tally);
    pool_release(ctx, q->d_order_row_index);
    for (auto p : q->d_order_proj) pool_release(ctx, p);
    group_order_release(q);
    for (auto &p : q->preds)
        if (!pred_list_shared(p)) pool_release(ctx, p.d_blob); // (a shared set's table is the set's)
    for (imm3_int_set *s : q->sets) int_set_release(s);
    for (auto &t : q->expr_terms)
        for (auto &p : t) pool_release(ctx, p.d_blob);
    pool_release(ctx, q->d_expr_preds);
    pool_release(ctx, q->d_expr_term_start);
    pool_release(ctx, q->d_stage_rec);
    pool_release(ctx, q->d_tile_start);
    pool_release(ctx, q->d_desc);
    pool_release(ctx, q->d_tile_desc);
    pool_release(ctx, q->d_akeys); pool_release(ctx, q->d_acounts); pool_release(ctx, q->d_okeys); pool_release(ctx, q->d_ocounts);
    pool_release(ctx, q->d_afirst); pool_release(ctx, q->d_ofirst); pool_release(ctx, q->d_ameta);
    pool_release(ctx, q->d_avals); pool_release(ctx, q->d_ovals);
    for (int j = 0; j < kMaxAggs; ++j) { pool_release(ctx, q->d_alive[j]); pool_release(ctx, q->d_chunks[j]); pool_release(ctx, q->d_dset[j]); }
    if (q->ev_filter_done) (void)hipEventDestroy(q->ev_filter_done);
    if (q->ev_total_done) (void)hipEventDestroy(q->ev_total_done);
    // the query kept its inputs alive (imm3_handles.h, "Lifetimes")
    if (q->table) table_release(q->table);
    else if (q->seg) segment_release(q->seg);
    ctx_release(ctx);
    delete q;
}

int imm3::ensure_row_capacity(imm3_query *q, uint64_t rows) {
    if (rows <= q->cap_rows && q->d_row_index) return IMM3_OK;
    if (rows < 1) rows = 1;
    imm3_ctx *ctx = q->ctx;
    if (q->d_row_index) graphs_mark_stale(ctx, q); // a recorded run would write through the old pointers (launch: IMM3_ERR_STATE)
    if (q->d_row_index && q->run.ran_project) q->run.rows_moved = true; // (the last run's rows went with the old arrays: settle_rows emits them again)
    pool_release(ctx, q->d_row_index); // stream-ordered: a gather still in flight finishes before any reuse
    q->d_row_index = nullptr;
    for (auto &p : q->d_proj) {
        pool_release(ctx, p);
        p = nullptr;
    }
    void *p = nullptr;
    HIPCHK(pool_alloc(ctx, &p, rows * sizeof(uint32_t)));
    q->d_row_index = (uint32_t *)p;
    q->d_proj.assign(q->proj.size(), nullptr);
    for (size_t j = 0; j < q->proj.size(); ++j) {
        const SegCol &sc = q->seg->cols[(size_t)q->used[(size_t)q->proj[j]]];
        HIPCHK(pool_alloc(ctx, &p, rows * (uint64_t)sc.width));
        q->d_proj[j] = (uint8_t *)p;
    }
    q->cap_rows = rows;
    return q->ordered ? ensure_order_buffers(q) : IMM3_OK;
}

// An ordered query's buffers (imm3_order.hip): two (key, permutation) buffers and the ordered arrays for as many rows as the row
// arrays hold, from the same pool; the fixed-size tables once.
int imm3::ensure_order_buffers(imm3_query *q) {
    if (!q->ordered || !q->d_row_index) return IMM3_OK;
    imm3_ctx *ctx = q->ctx;
    void *p = nullptr;
    if (!q->d_order_state) {
        HIPCHK(pool_alloc(ctx, &p, OW_WORDS * sizeof(uint32_t)));
        q->d_order_state = (uint32_t *)p;
        HIPCHK(hipMemsetAsync(p, 0, OW_WORDS * sizeof(uint32_t), ctx->stream));
        HIPCHK(pool_alloc(ctx, &p, (size_t)256 * kOrderWaves * sizeof(uint32_t)));
        q->d_order_counts = (uint32_t *)p;
        HIPCHK(pool_alloc(ctx, &p, (size_t)kOrderWaves * kOrderKeyWords * sizeof(uint32_t)));
        q->d_order_diff = (uint32_t *)p;
        HIPCHK(pool_alloc(ctx, &p, (size_t)kOrderWaves * 2 * sizeof(uint32_t)));
        q->d_order_tally = (uint32_t *)p;
    }
    if (q->order_cap_rows == q->cap_rows && q->d_order_row_index) return IMM3_OK;
    q->run.order_valid = false; // (the ordered arrays are allocated anew)
    const uint64_t rows = q->cap_rows;
    const uint64_t key_words = (uint64_t)(q->order_key_bytes + 3) / 4;
    for (int b = 0; b < 2; ++b) {
        pool_release(ctx, q->d_order_keys[b]);
        pool_release(ctx, q->d_order_perm[b]);
        q->d_order_keys[b] = q->d_order_perm[b] = nullptr;
    }
    pool_release(ctx, q->d_order_row_index);
    q->d_order_row_index = nullptr;
    for (auto &c : q->d_order_proj) {
        pool_release(ctx, c);
        c = nullptr;
    }
    for (int b = 0; b < 2; ++b) {
        HIPCHK(pool_alloc(ctx, &p, rows * key_words * sizeof(uint32_t)));
        q->d_order_keys[b] = (uint32_t *)p;
        HIPCHK(pool_alloc(ctx, &p, rows * sizeof(uint32_t)));
        q->d_order_perm[b] = (uint32_t *)p;
    }
    HIPCHK(pool_alloc(ctx, &p, rows * sizeof(uint32_t)));
    q->d_order_row_index = (uint32_t *)p;
    q->d_order_proj.assign(q->proj.size(), nullptr);
    for (size_t j = 0; j < q->proj.size(); ++j) {
        const SegCol &sc = q->seg->cols[(size_t)q->used[(size_t)q->proj[j]]];
        HIPCHK(pool_alloc(ctx, &p, rows * (uint64_t)sc.width));
        q->d_order_proj[j] = (uint8_t *)p;
    }
    q->order_cap_rows = rows;
    return IMM3_OK;
}

extern "C" int imm3_query_set_order(imm3_query *q, const imm3_order_key *keys, int32_t n_keys, int64_t limit) {
    if (!q) return fail(IMM3_ERR_ARG, "query is null");
    CTX_LIVE(q->ctx);
    std::vector<int32_t> widths;
    for (int32_t pj : q->proj) widths.push_back(q->seg->cols[(size_t)q->used[(size_t)pj]].width);
    int32_t key_bytes = 0;
    const int rc = imm3::order_check_args(q->is_agg, (int32_t)q->proj.size(), widths.data(), q->limit, q->run.ran_select || q->run.ran_project || q->run.ran_agg,
                                          keys, n_keys, limit, &key_bytes);
    if (rc) return rc;
    HIPCHK(hipSetDevice(q->ctx->device));
    q->order_keys.assign(keys, keys + n_keys);
    q->order_limit = limit > 0 ? limit : 0;
    if (q->ordered && key_bytes != q->order_key_bytes) q->order_cap_rows = 0; // (set again with wider keys: the key buffers are sized anew)
    q->order_key_bytes = key_bytes;
    q->ordered = true;
    q->run.order_valid = false;
    return ensure_order_buffers(q); // (rows reserved before this call: the order's buffers follow now)
}

// Batches of ONE segment as ScanOp yields them: the FIRST used column defines them (Scan.scala:55,72); BlockIterator
// takes each block by a relative get from a rewound buffer (Segment.scala:159-168), i.e. from a running cursor.
// Every other used column must hold the same rows in the same blocks, otherwise the reference either throws
// ArrayIndexOutOfBounds (shorter) or silently joins the wrong rows (longer): refused.
// rows of block k of a column: DENSE_* = bytes / width; PFOR_INT = the count the block declares
static inline int64_t block_rows_of(const SegCol &sc, int32_t k, int64_t len) {
    return is_compressed(sc.codec) ? (int64_t)sc.block_rows[(size_t)k] : len / sc.width;
}

static int compute_layout(const imm3_segment *seg, int32_t first_col, SegLayout &L) {
    const SegCol &first = seg->cols[(size_t)first_col];
    const int32_t nb = first.offsets.empty() ? 0 : (int32_t)first.offsets.size() - 1;
    L.size.resize((size_t)nb);
    L.word_off.resize((size_t)nb);
    uint64_t cursor = 0;
    for (int32_t k = 0; k < nb; ++k) {
        const int64_t len = (int64_t)first.offsets[(size_t)k + 1] - (int64_t)first.offsets[(size_t)k];
        if (len < 0) return fail(IMM3_ERR_LAYOUT, "block " + std::to_string(k) + ": negative length (NegativeArraySizeException in the reference)");
        if (!is_compressed(first.codec) && len % first.width) return fail(IMM3_ERR_LAYOUT, "block " + std::to_string(k) + ": byte length is not a multiple of the value width (malformed segment)");
        if (cursor + (uint64_t)len > first.bytes) return fail(IMM3_ERR_LAYOUT, "block " + std::to_string(k) + ": bytes [" + std::to_string(cursor) + ", " + std::to_string(cursor + (uint64_t)len) + ") run past the segment data of " + std::to_string(first.bytes) + " bytes (BufferUnderflowException in the reference)");
        const int64_t n = block_rows_of(first, k, len);
        L.size[(size_t)k] = (int32_t)n;
        L.word_off[(size_t)k] = L.words;
        if (k < nb - 1 && (n % 64)) L.ragged = true;
        L.words += (n + 63) / 64;
        L.rows += n;
        cursor += (uint64_t)len;
    }
    if (L.rows > 0xFFFFFFFFLL) return fail(IMM3_ERR_LAYOUT, "segment too large");
    return IMM3_OK;
}

// does used column `other` hold the same rows in the same blocks as the layout's first column?
static int check_same_blocks(const imm3_segment *seg, const SegLayout &L, int32_t other, size_t i) {
    const SegCol &sc = seg->cols[(size_t)other];
    const int32_t nb = (int32_t)L.size.size();
    const int32_t nbc = sc.offsets.empty() ? 0 : (int32_t)sc.offsets.size() - 1;
    if (nbc < nb) return fail(IMM3_ERR_LAYOUT, "used column " + std::to_string(i) + " has fewer blocks than the first used column (ArrayIndexOutOfBounds in the reference)");
    uint64_t cur = 0;
    for (int32_t k = 0; k < nb; ++k) {
        const int64_t len = (int64_t)sc.offsets[(size_t)k + 1] - (int64_t)sc.offsets[(size_t)k];
        if (len < 0 || (!is_compressed(sc.codec) && len % sc.width) || block_rows_of(sc, k, len) != L.size[(size_t)k])
            return fail(IMM3_ERR_LAYOUT, "used column " + std::to_string(i) + " block " + std::to_string(k) + " does not hold the same rows as the first used column");
        if (cur + (uint64_t)len > sc.bytes) return fail(IMM3_ERR_LAYOUT, "used column " + std::to_string(i) + " block " + std::to_string(k) + " runs past the segment data");
        cur += (uint64_t)len;
    }
    return IMM3_OK;
}

// The layout for these used columns, from the segment's cache (segments are immutable once created; any thread, any context).
static int segment_layout(const imm3_segment *cseg, const std::vector<int32_t> &used, std::shared_ptr<const SegLayout> &out) {
    imm3_segment *seg = const_cast<imm3_segment *>(cseg);
    std::lock_guard<std::mutex> g(seg->layout_mu);
    auto it = seg->layouts.find(used[0]);
    if (it == seg->layouts.end()) {
        auto L = std::make_shared<SegLayout>();
        const int rc = compute_layout(seg, used[0], *L);
        if (rc) return rc; // (a malformed column is reported every time it is asked for: nothing cached)
        it = seg->layouts.emplace(used[0], std::move(L)).first;
    }
    for (size_t i = 1; i < used.size(); ++i) {
        if (used[i] == used[0]) continue;
        const auto key = std::make_pair(used[0], used[i]);
        if (seg->same_blocks.count(key)) continue;
        const int rc = check_same_blocks(seg, *it->second, used[i], i);
        if (rc) return rc;
        seg->same_blocks[key] = true;
    }
    out = it->second;
    return IMM3_OK;
}

// Query creation, step 1: the arguments and the SelectOp conditions.
static int check_create_args(imm3_ctx *ctx, const imm3_segment *seg, const imm3_table *table, const int32_t *used_cols, int32_t n_used,
                             const imm3_select *sels, int32_t n_sels, const int32_t *proj, int32_t n_proj) {
    if (seg->closed || (table && table->closed)) return fail(IMM3_ERR_STATE, "the segment / table has been destroyed");
    if (seg->ctx->device != ctx->device) return fail(IMM3_ERR_ARG, "segment lives on another device");
    if (n_used <= 0 || !used_cols) return fail(IMM3_ERR_ARG, "a scan needs at least one used column");
    if (n_sels < 0 || (n_sels > 0 && !sels)) return fail(IMM3_ERR_ARG, "bad select list");
    if (n_proj < 0 || (n_proj > 0 && !proj)) return fail(IMM3_ERR_ARG, "bad project list");
    const int32_t nsegcols = (int32_t)seg->cols.size();
    for (int32_t i = 0; i < n_used; ++i)
        if (used_cols[i] < 0 || used_cols[i] >= nsegcols) return fail(IMM3_ERR_ARG, "used column index out of range");
    for (int32_t i = 0; i < n_sels; ++i)
        if (sels[i].column < 0 || sels[i].column >= n_used) return fail(IMM3_ERR_ARG, "select column is not among the used columns");
    for (int32_t i = 0; i < n_proj; ++i)
        if (proj[i] < 0 || proj[i] >= n_used) return fail(IMM3_ERR_ARG, "project column is not among the used columns");
    HIPCHK(hipSetDevice(ctx->device));
    if (table) {
        for (const imm3_segment *sg : table->segs) { const int wrc = segment_await(ctx, sg); if (wrc) return wrc; }
    } else {
        const int wrc = segment_await(ctx, seg);
        if (wrc) return wrc;
    }
    // SelectOp.iterator (Select.scala:17-23) rejects NotMatch / NoOp when the chain is built,
    // whether or not the segment has any block.
    for (int32_t i = 0; i < n_sels; ++i) {
        const int c = sels[i].cond;
        if (c != IMM3_MATCH && c != IMM3_GT && c != IMM3_LT && c != IMM3_EQ && c != IMM3_STR_RANGE && c != IMM3_INT_IN && c != IMM3_INT_IN_SET)
            return fail(IMM3_ERR_UNSUPPORTED_CONDITION, std::string("Unsupported condition: ") + cond_name(c));
        if (c == IMM3_MATCH && sels[i].n_match > 0 && (!sels[i].match_bytes || !sels[i].match_lens))
            return fail(IMM3_ERR_ARG, "Match without values");
        if (c == IMM3_STR_RANGE) { // (the bounds' lengths are held against a STRING column's width; any other column fails scan_layout's vector check)
            const SegCol &sc = seg->cols[(size_t)used_cols[sels[i].column]];
            const int rrc = str_range_check_leaf(sels[i].n_match, sels[i].match_bytes, sels[i].match_lens, sc.vcodec == IMM3_DENSE_STRING ? sc.width : 0);
            if (rrc) return rrc;
        }
        if (c == IMM3_INT_IN) { // (the count and the pointer; a STRING column fails scan_layout's vector check)
            const int lrc = int_list_check_leaf(sels[i].n_match, sels[i].match_bytes);
            if (lrc) return lrc;
        }
        if (c == IMM3_INT_IN_SET) { // (the handle; a STRING column fails scan_layout's vector check)
            const int src = int_set_check_leaf(ctx, sels[i].n_match, sels[i].match_bytes);
            if (src) return src;
        }
    }
    // a column with a set leaf takes no other list: whatever the sizes, so that the refusal does not depend on data
    for (int32_t i = 0; i < n_sels; ++i) {
        if (sels[i].cond != IMM3_INT_IN_SET) continue;
        for (int32_t k = 0; k < n_sels; ++k)
            if (k != i && used_cols[sels[k].column] == used_cols[sels[i].column] && (sels[k].cond == IMM3_INT_IN || sels[k].cond == IMM3_INT_IN_SET))
                return fail(IMM3_ERR_ARG, kIntSetOneListRefusal);
    }
    return IMM3_OK;
}

// Step 2: the batches (segment_layout), returned in `nb`; a table query concatenates the segments' batches, each segment's bitmap
// starting on a fresh tile of the virtual row space.  When there are batches, the codecs and vector types ScanOp and SelectOp
// dispatch on are checked.
static int scan_layout(imm3_query *q, const imm3_select *sels, int32_t n_sels, int32_t &nb) {
    if (!q->table) {
        const int lrc = segment_layout(q->seg, q->used, q->layout);
        if (lrc) return lrc;
        const SegLayout &L = *q->layout;
        nb = (int32_t)L.size.size();
        q->n_rows = L.rows;
        q->n_words = L.words;
        q->ragged = L.ragged;
        q->n_tiles = (q->n_words + kTileWords - 1) / kTileWords;
    } else {
        // every column of a table shares one block layout (imm3_table_create), so the batches do not depend on which
        // columns are used: they live in the table
        nb = (int32_t)q->table->batch_size.size();
        q->n_rows = q->table->n_rows;
        q->n_tiles = q->table->n_tiles;
        q->n_words = q->table->n_tiles * kTileWords; // virtual: every segment padded to whole tiles
    }
    q->n_chunks = (q->n_tiles + kChunkTiles - 1) / kChunkTiles;
    if (nb < 1) return IMM3_OK;
    // ScanOp.next dispatches on the codec of every used column (Scan.scala:37-50) ...
    for (int32_t sci : q->used) {
        const SegCol &sc = q->seg->cols[(size_t)sci];
        // PFOR_INT: the reference dispatches it too (Scan.scala:37-39) but its decode throws on every block
        // (PFORCodec.scala:43-50); here the blocks its encoder writes are decoded (imm3_codec.hip).
        // Snappy-coded columns (IMM3_SNAPPY_*) are this library's extension: the reference only has the encoder.
        if (sc.vcodec != IMM3_DENSE_INT && sc.vcodec != IMM3_DENSE_TINYINT && sc.vcodec != IMM3_DENSE_STRING)
            return fail(IMM3_ERR_NO_CODEC, "No implementation for codec " + std::to_string(sc.codec));
        if ((sc.vcodec == IMM3_DENSE_INT && sc.width != 4) || (sc.vcodec == IMM3_DENSE_TINYINT && sc.width != 1))
            return fail(IMM3_ERR_ARG, "width does not match codec");
    }
    // ... and each SelectIterator dispatches on the vector type (Select.scala:41,80,118,156).
    for (int32_t i = 0; i < n_sels; ++i) {
        const SegCol &sc = q->seg->cols[(size_t)q->used[(size_t)sels[i].column]];
        const bool is_str = sc.vcodec == IMM3_DENSE_STRING;
        if ((sels[i].cond == IMM3_MATCH || sels[i].cond == IMM3_STR_RANGE) != is_str) return fail(IMM3_ERR_UNSUPPORTED_VECTOR, "Unsupported column vector");
    }
    return IMM3_OK;
}

// Step 3 (a segment with batches): fold the SelectOp leaves per column into q->preds.  Every leaf only clears bits
// (Select.scala:37,68,106,144) and runOps ignores AND/OR (Engine.scala:240), so the chain is a conjunction and order is irrelevant.
static int fold_selects(imm3_query *q, const imm3_select *sels, int32_t n_sels) {
    for (int32_t i = 0; i < n_sels; ++i) {
        const int32_t sci = q->used[(size_t)sels[i].column];
        const SegCol &sc = q->seg->cols[(size_t)sci];
        FoldedPred leaf; // (one leaf alone, then the conjunction with what the column has so far: imm3_expr_norm.cpp)
        const int rc = leaf_pred(sci, sc.vcodec, sc.width, sels[i], leaf);
        if (rc) return rc;
        FoldedPred *fp = pred_on(q->preds, sci);
        if (!fp) q->preds.push_back(leaf);
        else merge_pred(*fp, leaf);
    }
    for (const auto &p : q->preds)
        if (p.has_range ? pred_empty(p) : (p.kind == KIND_STR ? p.match.empty() : p.lo > p.hi)) q->always_false = true;
    // a range every row passes leaves its column: a query left without predicates is the NoSelect form
    q->preds.erase(std::remove_if(q->preds.begin(), q->preds.end(), [](const FoldedPred &p) { return p.has_range && pred_unconstrained(p); }), q->preds.end());
    return IMM3_OK;
}

// Step 3 of a select tree with an OR or a NOT in it (a segment with batches): its normal form (imm3_expr_norm.cpp) into q->expr_terms;
// q->preds stays empty.  No term left: the tree selects nothing.  The one term without a predicate: it selects EVERY row, and the
// query is from here on the NoSelect form -- no tree, no predicate, the scan every query without select leaves runs (the tree
// kernels have no instance without a column).
static int fold_tree(imm3_query *q, const imm3_select *sels, int32_t n_sels, const int32_t *prog, int32_t n_prog) {
    std::vector<ExprCol> leaf_cols;
    for (int32_t i = 0; i < n_sels; ++i) {
        const int32_t sci = q->used[(size_t)sels[i].column];
        const SegCol &sc = q->seg->cols[(size_t)sci];
        leaf_cols.push_back(ExprCol{sci, sc.vcodec, sc.width});
    }
    const int rc = expr_normalize(leaf_cols, sels, n_sels, prog, n_prog, q->expr_terms);
    if (rc) return rc;
    if (q->expr_terms.size() == 1 && q->expr_terms[0].empty()) {
        q->expr_terms.clear();
        q->expr_universal = true;
        return IMM3_OK;
    }
    q->is_expr = true;
    if (q->expr_terms.empty()) q->always_false = true;
    return IMM3_OK;
}

// A table has no word-at-a-time kernel: the predicates that would need it are refused when the query is created.
const char *const imm3::kTableGenericRefusal =
    "table queries take int32 / int8 predicates, Match on 2-byte string columns with at most 8 IN-list values, and Match on string "
    "columns whose width is a multiple of 4 (4 .. 256 bytes, any IN-list); still refused: string columns of any other width and "
    "2-byte string columns with more than 8 values; use per-segment queries";

// ... and a range (IMM3_STR_RANGE) goes through its string pass or not at all
const char *const imm3::kTableRangeRefusal =
    "table queries take a string range (IMM3_STR_RANGE) on string columns whose width is a multiple of 4 (4 .. 256 bytes) only: a table "
    "has no word-at-a-time kernel for the other widths; use per-segment queries";
static const char *const kTreeRangeRefusal =
    "a select program with an IMM3_EXPR_OR or an IMM3_EXPR_NOT does not take IMM3_STR_RANGE leaves (its normal form would need "
    "complemented ranges and ranges with exclusions); a program of IMM3_EXPR_AND alone does";

static int upload_match_blobs(imm3_query *q, std::vector<FoldedPred> &preds);

// Step 5 of a select tree: which kernel form can take the terms, and the generic form's predicates on the device.  (Compressed
// predicate columns have been decoded by now: place_compressed finds no folded predicate to fuse into k_filter_pfor.)
static int expr_setup(imm3_query *q) {
    if (q->always_false) return IMM3_OK;
    // a table has no row-per-lane kernel: the tree fits the tile form or the query is refused, each bound by name.  Every refusal
    // starts with IMM3_TABLE_TREE_REFUSED: that prefix is what sends a caller to per-segment queries (imm3.h).
    const auto refuse = [](const std::string &bound) {
        return fail(IMM3_ERR_ARG, std::string(IMM3_TABLE_TREE_REFUSED) + bound + "; use per-segment queries");
    };
    const auto n = [](size_t v) { return std::to_string(v); };
    if (q->table) {
        std::vector<int32_t> seen;
        for (const auto &t : q->expr_terms)
            for (const auto &p : t) {
                if (p.kind == KIND_STR && p.width != 2)
                    return refuse("string predicates on 2-byte columns only (column width " + n((size_t)p.width) + ")");
                if (p.kind == KIND_STR && p.match.size() > (size_t)kMaxTileMatch)
                    return refuse(std::string(p.negated ? "IN-lists and exclusion lists" : "IN-lists") + " of at most " + n((size_t)kMaxTileMatch) + " values (got " + n(p.match.size()) + ")");
                if (tile_kind(p) == TK_NONE)
                    return refuse("predicates on int32, int8 and 2-byte string columns only (column " + n((size_t)p.seg_col) + " is none of them)");
                if (std::find(seen.begin(), seen.end(), p.seg_col) == seen.end()) seen.push_back(p.seg_col);
            }
        if (q->expr_terms.size() > (size_t)kMaxExprTerms)
            return refuse("at most " + n((size_t)kMaxExprTerms) + " terms (this one normalises to " + n(q->expr_terms.size()) + ")");
        if (seen.size() > (size_t)kMaxTileCols)
            return refuse("at most " + n((size_t)kMaxTileCols) + " predicate columns (got " + n(seen.size()) + ")");
    } else {
        for (auto &t : q->expr_terms) {
            const int rc = upload_match_blobs(q, t);
            if (rc) return rc;
        }
    }
    // tile form: <= kMaxExprTerms terms, every predicate of a tile kind, <= 3 distinct columns that make an instantiated combination
    bool ok = !q->ragged && q->expr_terms.size() <= (size_t)kMaxExprTerms;
    std::vector<std::pair<int32_t, int32_t>> cols; // (tile kind, segment column), in first-seen order
    for (const auto &t : q->expr_terms)
        for (const auto &p : t) {
            const int tk = tile_kind(p);
            ok = ok && tk != TK_NONE;
            bool seen = false;
            for (auto &c : cols) seen = seen || c.second == p.seg_col;
            if (!seen) cols.emplace_back(tk, p.seg_col);
        }
    ok = ok && cols.size() <= (size_t)kMaxTileCols;
    if (ok) {
        std::stable_sort(cols.begin(), cols.end(), [](const std::pair<int32_t, int32_t> &x, const std::pair<int32_t, int32_t> &y) { return x.first < y.first; });
        int n_s2 = 0;
        for (size_t k = 0; k < cols.size(); ++k) {
            q->expr_kinds[k] = cols[k].first;
            q->expr_seg_col[k] = cols[k].second;
            n_s2 += cols[k].first == TK_S2;
        }
        ok = n_s2 <= 1 && filter_tile_group(q->expr_kinds) > 0; // (k_filter_expr is instantiated for k_filter_tile's combinations)
    }
    q->expr_tile_ok = ok;
    if (q->table) { // (no generic form: nothing to upload)
        if (!ok)
            return refuse("at most one 2-byte string column among its predicate columns, in a uniform block layout "
                          "(no kernel for this column-kind combination)");
        return IMM3_OK;
    }
    // generic form (also what TV_GENERIC_ONLY runs): the predicates term after term
    q->h_expr_term_start.assign(1, 0);
    for (const auto &t : q->expr_terms) {
        for (const auto &p : t) {
            ColPred cp;
            fill_colpred(q, p, cp);
            q->h_expr_preds.push_back(cp);
        }
        q->h_expr_term_start.push_back((int32_t)q->h_expr_preds.size());
    }
    void *d = nullptr;
    HIPCHK(pool_alloc(q->ctx, &d, q->h_expr_preds.size() * sizeof(ColPred)));
    q->d_expr_preds = (ColPred *)d;
    HIPCHK(pool_alloc(q->ctx, &d, q->h_expr_term_start.size() * sizeof(int32_t)));
    q->d_expr_term_start = (int32_t *)d;
    HIPCHK(hipMemcpyAsync(q->d_expr_preds, q->h_expr_preds.data(), q->h_expr_preds.size() * sizeof(ColPred), hipMemcpyHostToDevice, q->ctx->stream));
    HIPCHK(hipMemcpyAsync(q->d_expr_term_start, q->h_expr_term_start.data(), q->h_expr_term_start.size() * sizeof(int32_t), hipMemcpyHostToDevice, q->ctx->stream));
    return IMM3_OK;
}

// Step 4: where compressed columns are read.  A PFOR_INT predicate-only column of a tile-aligned segment is evaluated on its
// compressed blocks (k_filter_pfor); anything else reads the decoded column, made once per segment.  `row_cols` are the used
// columns an aggregation reads row by row (its group and aggregate columns; matched by segment column: a predicate on the same
// column is not fused either).  Without batches only those are decoded.
static int place_compressed(imm3_query *q, bool have_batches, const std::vector<int32_t> &row_cols) {
    const int fv = q->ctx->filter_variant;
    for (int32_t i = 0; i < (int32_t)q->used.size(); ++i) {
        const int32_t sci = q->used[(size_t)i];
        const SegCol &sc = q->seg->cols[(size_t)sci];
        bool agg_reads = false;
        for (int32_t r : row_cols) agg_reads |= r >= 0 && r < (int32_t)q->used.size() && q->used[(size_t)r] == sci;
        if (!is_compressed(sc.codec) || !(have_batches || agg_reads)) continue;
        bool projected = false;
        for (int32_t pj : q->proj) projected |= (pj == i);
        FoldedPred *fp = pred_on(q->preds, sci);
        const bool fused = sc.codec == IMM3_PFOR_INT && fp && !fp->has_list && !q->table && !q->ragged && sc.tile_aligned && !projected && !agg_reads &&
                           fv != TV_GENERIC_ONLY && fv != TV_PFOR_DECODED;
        if (fused) fp->pfor = true;
        else if (!q->table) { // a table decodes its PFOR_INT columns when it is created
            const int drc = ensure_dense(q->ctx, q->seg, sci);
            if (drc) return drc;
        }
    }
    return IMM3_OK;
}

// Step 4b: the high-half planes this query's tile passes can scan (hi16_eligible with the run-time facts open).  A column that has
// no plane yet gets one here.  A projection with a limit is left alone altogether: its runs scan in chunks over the column itself, and
// it neither makes a plane nor takes one.  What creation found goes into the folded predicate; a run reads nothing else.
static int place_hi16(imm3_query *q, bool have_batches) {
    const int fv = q->ctx->filter_variant;
    if (!have_batches || q->table || q->is_expr || q->ragged || q->always_false || fv == TV_I32_SCAN || fv == TV_GENERIC_ONLY) return IMM3_OK;
    if (q->limit > 0 && !q->proj.empty()) return IMM3_OK;
    const SelectChain chain = plan_select_chain(q);
    for (const auto &take : chain.tile_passes)
        for (const FoldedPred *cfp : take) {
            if (tile_kind(*cfp) != TK_I32) continue;
            Hi16Inputs in = hi16_inputs(q, *cfp, take);
            in.has_plane = true; // (it may get one)
            if (!hi16_eligible(in)) continue;
            const int rc = ensure_hi16(q->ctx, q->seg, cfp->seg_col);
            if (rc) return rc;
            std::lock_guard<std::mutex> g(const_cast<imm3_segment *>(q->seg)->decode_mu);
            pred_on(q->preds, cfp->seg_col)->d_hi16 = q->seg->cols[(size_t)cfp->seg_col].d_hi16;
        }
    return IMM3_OK;
}

// Step 5: IN-lists too long for the kernel arguments go to the device -- and so does the probe table of an int32 column's folded
// IMM3_INT_IN list of more than kMaxMatch values (built here, once: imm3_int_list_plan.cpp; the list pass's LDS / GLOBAL forms and the
// word-at-a-time kernels probe it); a shorter list travels as its values and an int8 column's list as its 256-bit set, both in the
// kernel arguments.
static int upload_match_blobs(imm3_query *q, std::vector<FoldedPred> &preds) {
    for (auto &p : preds) {
        if (p.kind != KIND_STR && pred_list_shared(p)) { // IMM3_INT_IN_SET: everything is on the device already, in the set
            const imm3_int_set *set = p.set;
            if (p.kind == KIND_I8) std::memcpy(p.list_set, set->set256, sizeof(p.list_set));
            else {
                p.list_mask = set->mask;
                p.list_shift = set->shift;
                p.list_max_probe = set->max_probe;
                p.list_empty = set->empty;
                p.d_blob = (uint8_t *)set->d_table; // (not owned: query_free)
            }
            continue;
        }
        if (p.kind != KIND_STR && p.has_list && !p.list.empty()) {
            if (p.kind == KIND_I8) {
                int_list_set256(p.list, p.list_set);
                continue;
            }
            if (int_list_form(p.width, pred_list_count(p)) == INT_LIST_ARGS) continue; // (the values travel in the kernel arguments on every route: no table, no allocation, no wait)
            IntListTable t;
            int_list_build_table(p.list, t);
            p.list_mask = t.mask;
            p.list_shift = t.shift;
            p.list_max_probe = t.max_probe;
            p.list_empty = t.empty;
            void *d = nullptr;
            HIPCHK(pool_alloc(q->ctx, &d, t.slots.size() * sizeof(int32_t)));
            p.d_blob = (uint8_t *)d;
            HIPCHK(hipMemcpyAsync(d, t.slots.data(), t.slots.size() * sizeof(int32_t), hipMemcpyHostToDevice, q->ctx->stream));
            HIPCHK(hipStreamSynchronize(q->ctx->stream)); // (the host image goes away with this scope)
            continue;
        }
        if (p.kind != KIND_STR || (!p.has_range && (p.match.empty() || (p.width <= 8 && p.match.size() <= (size_t)kMaxMatch)))) continue;
        std::string blob;
        for (auto &v : p.match) blob += v;
        if (p.has_range) { // (always on the device: the bounds byte for byte, then dword-swapped for the string pass's tails)
            std::vector<uint8_t> packed;
            str_range_pack(p.range_lo, p.range_hi, packed, p.range_lo4, p.range_hi4);
            blob.assign(packed.begin(), packed.end());
        }
        void *d = nullptr;
        HIPCHK(pool_alloc(q->ctx, &d, blob.size()));
        p.d_blob = (uint8_t *)d;
        HIPCHK(hipMemcpyAsync(d, blob.data(), blob.size(), hipMemcpyHostToDevice, q->ctx->stream));
        HIPCHK(hipStreamSynchronize(q->ctx->stream));
    }
    return IMM3_OK;
}

// Step 6: the device buffers every query has, and their initial contents.
static int alloc_buffers(imm3_query *q) {
    imm3_ctx *ctx = q->ctx;
    void *p = nullptr;
    const size_t words_alloc = (size_t)std::max<int64_t>(q->n_tiles * kTileWords, 1);
    HIPCHK(pool_alloc(ctx, &p, words_alloc * sizeof(uint64_t)));
    q->d_bitmap = (uint64_t *)p;
    HIPCHK(pool_alloc(ctx, &p, (size_t)std::max<int64_t>(q->n_tiles, 1) * sizeof(uint32_t)));
    q->d_tile_offsets = (uint32_t *)p;
    HIPCHK(pool_alloc(ctx, &p, (size_t)std::max<int64_t>(q->n_chunks, 1) * sizeof(uint32_t)));
    q->d_chunk_sums = (uint32_t *)p;
    HIPCHK(pool_alloc(ctx, &p, kMaxFilterGrid * sizeof(uint32_t)));
    q->d_block_partials = (uint32_t *)p;
    if (q->limit > 0 && q->limit <= kLimitGatherMaxRows && !q->table) { // (k_limit_gather's per-work-group counts: pooled memory, so cleared -- a run's tag is never zero)
        HIPCHK(pool_alloc(ctx, &p, 256 * sizeof(unsigned long long)));
        q->d_limit_state = (unsigned long long *)p;
        HIPCHK(hipMemsetAsync(q->d_limit_state, 0, 256 * sizeof(unsigned long long), ctx->stream));
    }
    HIPCHK(pool_alloc(ctx, &p, kFinishWords * sizeof(unsigned long long))); // {total, n_emit, status, limit, tally, log, log index, log capacity}, then the sub-tallies (imm3_device.h)
    q->d_total = (unsigned long long *)p;
    q->d_n_emit = q->d_total + 1;
    // Creation enqueues and returns: nothing below waits for the device (round 3 ended every creation with a stream
    // synchronisation, behind a 12.5 MB memset of the bitmap -- a query cost four times what running it did).  What the copies
    // read lives in the query handle.  The finish block = zeros + the limit, ONE copy; of the bitmap only the words behind
    // n_words in its last tile need to be zero (the offsets scan and the aggregation read whole tiles): every run writes all the
    // others before anything reads them.
    q->h_init.assign((size_t)kFinishWords, 0ULL);
    q->h_init[3] = (unsigned long long)q->limit;
    HIPCHK(hipMemcpyAsync(q->d_total, q->h_init.data(), (size_t)kFinishWords * sizeof(unsigned long long), hipMemcpyHostToDevice, ctx->stream));
    const size_t from = (size_t)std::min<int64_t>(std::max<int64_t>(q->n_words, 0), (int64_t)words_alloc); // (words [n_words, words_alloc): at most one tile's worth)
    if (from < words_alloc) HIPCHK(hipMemsetAsync(q->d_bitmap + from, 0, (words_alloc - from) * sizeof(uint64_t), ctx->stream));
    if (q->ragged) { // the first row and the valid rows of every bitmap word
        std::vector<uint32_t> &base = q->h_word_row_base;
        std::vector<uint8_t> &nvalid = q->h_word_nvalid;
        base.assign((size_t)q->n_tiles * kTileWords, 0u);
        nvalid.assign((size_t)q->n_tiles * kTileWords, 0);
        int64_t row = 0;
        size_t w = 0;
        for (const int64_t n : q->layout->size) {
            for (int64_t r = 0; r < n; r += 64) {
                base[w] = (uint32_t)(row + r);
                nvalid[w] = (uint8_t)std::min<int64_t>(64, n - r);
                ++w;
            }
            row += n;
        }
        HIPCHK(pool_alloc(ctx, &p, base.size() * sizeof(uint32_t) + 4));
        q->d_word_row_base = (uint32_t *)p;
        HIPCHK(pool_alloc(ctx, &p, nvalid.size() + 4));
        q->d_word_nvalid = (uint8_t *)p;
        if (!base.empty()) {
            HIPCHK(hipMemcpyAsync(q->d_word_row_base, base.data(), base.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(hipMemcpyAsync(q->d_word_nvalid, nvalid.data(), nvalid.size(), hipMemcpyHostToDevice, ctx->stream));
        }
    }
    if (!q->proj.empty() && q->limit > 0) return ensure_row_capacity(q, (uint64_t)std::min<int64_t>(q->limit, std::max<int64_t>(q->n_rows, 1)));
    return IMM3_OK;
}

// `row_cols`: the used columns an aggregation reads row by row (place_compressed); empty for a projection.
static int query_create_impl(imm3_ctx *ctx, const imm3_segment *seg, const imm3_table *table,
                                 const int32_t *used_cols, int32_t n_used,
                                 const imm3_select *sels, int32_t n_sels,
                                 const int32_t *proj, int32_t n_proj, int64_t limit,
                                 int32_t table_block_size, const std::vector<int32_t> &row_cols, imm3_query **out,
                                 const int32_t *prog = nullptr, int32_t n_prog = 0, bool tree = false) {
    if (!seg || !out) return fail(IMM3_ERR_ARG, "null argument");
    *out = nullptr;
    CTX_LIVE(ctx); // (the context's gate is held until creation returns)
    int rc = check_create_args(ctx, seg, table, used_cols, n_used, sels, n_sels, proj, n_proj);
    if (rc) return rc;
    // A select tree (imm3_query_create_expr): the leaves have passed the checks of a flat list; now the program.  Without an OR and
    // without a NOT it IS a flat list -- the leaves in program order go through the steps below exactly as imm3_query_create's do.
    // A table's tree (imm3_query_create_table_expr) has ALL its leaves through imm3_query_create_table's checks first, the ones that
    // need the batches (scan_layout) included, and its program checked behind them.
    std::vector<imm3_select> flat;
    bool has_or = false, has_not = false;
    auto check_program = [&]() -> int {
        const int prc = expr_check_program(prog, n_prog, n_sels, &has_or, &has_not);
        if (prc) return prc;
        if (has_or || has_not)
            for (int32_t i = 0; i < n_sels; ++i)
                if (sels[i].cond == IMM3_STR_RANGE) return fail(IMM3_ERR_ARG, kTreeRangeRefusal);
        if (has_or || has_not)
            for (int32_t i = 0; i < n_sels; ++i)
                if (sels[i].cond == IMM3_INT_IN) return fail(IMM3_ERR_ARG, kTreeIntInRefusal);
        if (has_or || has_not)
            for (int32_t i = 0; i < n_sels; ++i)
                if (sels[i].cond == IMM3_INT_IN_SET) return fail(IMM3_ERR_ARG, kTreeIntSetRefusal);
        if (!has_or && !has_not) {
            for (int32_t i = 0; i < n_prog; ++i)
                if (prog[i] >= 0) flat.push_back(sels[prog[i]]);
            sels = flat.data();
            n_sels = (int32_t)flat.size();
        }
        return IMM3_OK;
    };
    if (tree && !table) { rc = check_program(); if (rc) return rc; }

    std::unique_ptr<imm3_query, void (*)(imm3_query *)> q(new imm3_query(), query_free);
    q->ctx = ctx;
    ctx_retain(ctx);
    q->seg = seg;
    q->table = table;
    if (table) const_cast<imm3_table *>(table)->refs.fetch_add(1, std::memory_order_relaxed); // (the table holds its segments)
    else segment_retain(seg);
    q->table_block_size = table_block_size;
    q->used.assign(used_cols, used_cols + n_used);
    q->proj.assign(proj, proj + n_proj);
    q->limit = limit;
    for (int32_t i = 0; i < n_sels; ++i) // the sets of the leaves stay alive as long as the query does (its predicates point into them)
        if (sels[i].cond == IMM3_INT_IN_SET) q->sets.push_back(int_set_retain((imm3_int_set *)const_cast<uint8_t *>(sels[i].match_bytes)));

    int32_t nb = 0;
    rc = scan_layout(q.get(), sels, n_sels, nb); if (rc) return rc;
    if (tree && table) { rc = check_program(); if (rc) return rc; }
    if (nb >= 1 && (has_or || has_not)) { rc = fold_tree(q.get(), sels, n_sels, prog, n_prog); if (rc) return rc; }
    else if (nb >= 1) { rc = fold_selects(q.get(), sels, n_sels); if (rc) return rc; }
    rc = place_compressed(q.get(), nb >= 1, row_cols); if (rc) return rc;
    rc = place_hi16(q.get(), nb >= 1); if (rc) return rc;
    if (table) // (a flat select list; a tree's terms are checked by expr_setup)
        for (const FoldedPred &p : q->preds)
            if (pred_route(p) == 2 && (p.has_range ? !q->always_false : !p.match.empty())) return fail(IMM3_ERR_ARG, p.has_range ? kTableRangeRefusal : kTableGenericRefusal);
    rc = upload_match_blobs(q.get(), q->preds); if (rc) return rc;
    if (q->is_expr) { rc = expr_setup(q.get()); if (rc) return rc; }
    rc = alloc_buffers(q.get()); if (rc) return rc;
    rc = plan_projection(q.get()); if (rc) return rc;
    *out = q.release();
    return IMM3_OK;
}

extern "C" int imm3_query_create(imm3_ctx *ctx, const imm3_segment *seg,
                                 const int32_t *used_cols, int32_t n_used,
                                 const imm3_select *sels, int32_t n_sels,
                                 const int32_t *proj, int32_t n_proj, int64_t limit,
                                 int32_t table_block_size, imm3_query **out) {
    return query_create_impl(ctx, seg, nullptr, used_cols, n_used, sels, n_sels, proj, n_proj, limit, table_block_size, {}, out);
}

extern "C" int imm3_query_create_expr(imm3_ctx *ctx, const imm3_segment *seg,
                                      const int32_t *used_cols, int32_t n_used,
                                      const imm3_select *leaves, int32_t n_leaves, const int32_t *prog, int32_t n_prog,
                                      const int32_t *proj, int32_t n_proj, int64_t limit,
                                      int32_t table_block_size, imm3_query **out) {
    return query_create_impl(ctx, seg, nullptr, used_cols, n_used, leaves, n_leaves, proj, n_proj, limit, table_block_size, {}, out, prog, n_prog, true);
}

extern "C" int imm3_query_create_table_expr(imm3_ctx *ctx, const imm3_table *table,
                                            const int32_t *used_cols, int32_t n_used,
                                            const imm3_select *leaves, int32_t n_leaves, const int32_t *prog, int32_t n_prog,
                                            const int32_t *proj, int32_t n_proj, int64_t limit,
                                            int32_t table_block_size, imm3_query **out) {
    if (!table || table->segs.empty()) return fail(IMM3_ERR_ARG, "table is null or empty");
    return query_create_impl(ctx, table->segs[0], table, used_cols, n_used, leaves, n_leaves, proj, n_proj, limit, table_block_size, {}, out, prog, n_prog, true);
}

extern "C" int imm3_query_create_table(imm3_ctx *ctx, const imm3_table *table,
                                       const int32_t *used_cols, int32_t n_used,
                                       const imm3_select *sels, int32_t n_sels,
                                       const int32_t *proj, int32_t n_proj, int64_t limit,
                                       int32_t table_block_size, imm3_query **out) {
    if (!table || table->segs.empty()) return fail(IMM3_ERR_ARG, "table is null or empty");
    return query_create_impl(ctx, table->segs[0], table, used_cols, n_used, sels, n_sels, proj, n_proj, limit, table_block_size, {}, out);
}

// ---------------------------------------------------------------------------------------------
// table: the tile table over all segments
// ---------------------------------------------------------------------------------------------
static void table_free(imm3_table *t) {
    if (!t) return;
    if (t->ctx) (void)hipSetDevice(t->ctx->device);
    (void)hipFree(t->d_tile_rows);
    for (auto p : t->d_tile_ptrs) (void)hipFree(p);
    (void)hipFree(t->d_sample_rows);
    for (auto p : t->d_sample_ptrs) (void)hipFree(p);
    for (auto sg : t->segs) segment_release(sg);
    if (t->ctx) ctx_release(t->ctx);
    delete t;
}
static void table_release(const imm3_table *ct) {
    imm3_table *t = const_cast<imm3_table *>(ct);
    if (t->refs.fetch_sub(1, std::memory_order_acq_rel) == 1) table_free(t);
}

extern "C" int imm3_table_create(imm3_ctx *ctx, const imm3_segment *const *segs, int32_t n_segs, imm3_table **out) {
    if (!out) return fail(IMM3_ERR_ARG, "null argument");
    *out = nullptr;
    CTX_LIVE(ctx);
    if (n_segs <= 0 || !segs) return fail(IMM3_ERR_ARG, "a table needs at least one segment");
    HIPCHK(hipSetDevice(ctx->device));
    std::unique_ptr<imm3_table, void (*)(imm3_table *)> t(new imm3_table(), table_free);
    t->ctx = ctx;
    ctx_retain(ctx);
    const size_t ncols = segs[0]->cols.size();
    std::vector<int32_t> all_cols(ncols);
    for (size_t c = 0; c < ncols; ++c) all_cols[c] = (int32_t)c;
    t->tile_start.push_back(0);
    for (int32_t si = 0; si < n_segs; ++si) {
        const imm3_segment *sg = segs[si];
        if (!sg || sg->ctx->device != ctx->device) return fail(IMM3_ERR_ARG, "segment is null or lives on another device");
        if (sg->closed) return fail(IMM3_ERR_STATE, "segment " + std::to_string(si) + " has been destroyed");
        if (sg->cols.size() != ncols) return fail(IMM3_ERR_ARG, "segments of one table must have the same columns");
        for (size_t c = 0; c < ncols; ++c)
            if (sg->cols[c].codec != segs[0]->cols[c].codec || sg->cols[c].width != segs[0]->cols[c].width)
                return fail(IMM3_ERR_ARG, "segments of one table must have the same column types");
        std::shared_ptr<const SegLayout> Lp;
        const int rc = segment_layout(sg, all_cols, Lp);
        if (rc) return rc;
        const SegLayout &L = *Lp;
        if (L.ragged) return fail(IMM3_ERR_LAYOUT, "segment " + std::to_string(si) + ": a non-final block is not a multiple of 64 rows (ragged layout); use per-segment queries");
        for (size_t c = 0; c < ncols; ++c) { // the tile table addresses flat columns: decode PFOR_INT ones now
            const int drc = ensure_dense(ctx, sg, (int32_t)c);
            if (drc) return drc;
        }
        t->segs.push_back(sg);
        segment_retain(sg); // the tile table points into the segment's columns
        t->seg_rows.push_back(L.rows);
        t->seg_first_batch.push_back((int32_t)t->batch_size.size());
        t->seg_first_word.push_back(t->tile_start.back() * kTileWords);
        for (size_t k = 0; k < L.size.size(); ++k) {
            t->batch_size.push_back(L.size[k]);
            t->batch_k.push_back((int32_t)k);
            t->batch_word_off.push_back(t->tile_start.back() * kTileWords + L.word_off[k]);
        }
        t->tile_start.push_back(t->tile_start.back() + (L.rows + kTileRows - 1) / kTileRows);
        t->n_rows += L.rows;
    }
    t->n_tiles = t->tile_start.back();
    t->seg_first_batch.push_back((int32_t)t->batch_size.size());
    t->seg_first_word.push_back(t->n_tiles * kTileWords);
    if (t->n_tiles * (int64_t)kTileRows > 0xFFFFFFFFLL) return fail(IMM3_ERR_LAYOUT, "table too large for 32-bit virtual row ids on one device");
    std::vector<uint32_t> rows((size_t)std::max<int64_t>(t->n_tiles, 1), 0);
    std::vector<std::vector<const void *>> ptrs(ncols, std::vector<const void *>((size_t)std::max<int64_t>(t->n_tiles, 1), nullptr));
    for (size_t si = 0; si < t->segs.size(); ++si) {
        const int64_t nt = t->tile_start[si + 1] - t->tile_start[si];
        for (int64_t k = 0; k < nt; ++k) {
            const size_t tile = (size_t)(t->tile_start[si] + k);
            rows[tile] = (uint32_t)std::min<int64_t>(kTileRows, t->seg_rows[si] - k * kTileRows);
            for (size_t c = 0; c < ncols; ++c) ptrs[c][tile] = col_flat(t->segs[si]->cols[c]) + (size_t)k * kTileRows * (size_t)t->segs[si]->cols[c].width;
        }
    }
    void *p = nullptr;
    HIPCHK(hipMalloc(&p, rows.size() * sizeof(uint32_t)));
    t->d_tile_rows = (uint32_t *)p;
    HIPCHK(hipMemcpyAsync(t->d_tile_rows, rows.data(), rows.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    t->d_tile_ptrs.assign(ncols, nullptr);
    for (size_t c = 0; c < ncols; ++c) {
        HIPCHK(hipMalloc(&p, ptrs[c].size() * sizeof(void *)));
        t->d_tile_ptrs[c] = (void **)p;
        HIPCHK(hipMemcpyAsync(t->d_tile_ptrs[c], ptrs[c].data(), ptrs[c].size() * sizeof(void *), hipMemcpyHostToDevice, ctx->stream));
    }
    // the sample a query's plan is made on (single_pass_sample): eight chunks of 64 tiles spread evenly over the table
    std::vector<uint32_t> srows;
    std::vector<std::vector<const void *>> sptrs;
    if (t->n_tiles >= 4096) {
        srows.resize((size_t)kSampleTiles);
        sptrs.assign(ncols, std::vector<const void *>((size_t)kSampleTiles, nullptr));
        for (int i = 0; i < kSampleChunks; ++i) {
            int64_t tile0 = (int64_t)((2 * i + 1) * t->n_tiles / (2 * kSampleChunks)) - kSampleChunkTiles / 2;
            tile0 = std::max<int64_t>(0, std::min<int64_t>(tile0, t->n_tiles - kSampleChunkTiles));
            for (int64_t k = 0; k < kSampleChunkTiles; ++k) {
                srows[(size_t)(i * kSampleChunkTiles + k)] = rows[(size_t)(tile0 + k)];
                for (size_t c = 0; c < ncols; ++c) sptrs[c][(size_t)(i * kSampleChunkTiles + k)] = ptrs[c][(size_t)(tile0 + k)];
            }
        }
        HIPCHK(hipMalloc(&p, srows.size() * sizeof(uint32_t)));
        t->d_sample_rows = (uint32_t *)p;
        HIPCHK(hipMemcpyAsync(t->d_sample_rows, srows.data(), srows.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        t->d_sample_ptrs.assign(ncols, nullptr);
        for (size_t c = 0; c < ncols; ++c) {
            HIPCHK(hipMalloc(&p, sptrs[c].size() * sizeof(void *)));
            t->d_sample_ptrs[c] = (void **)p;
            HIPCHK(hipMemcpyAsync(t->d_sample_ptrs[c], sptrs[c].data(), sptrs[c].size() * sizeof(void *), hipMemcpyHostToDevice, ctx->stream));
        }
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    *out = t.release();
    return IMM3_OK;
}

extern "C" int imm3_table_destroy(imm3_table *t) {
    if (!t) return IMM3_OK;
    if (t->closed) return fail(IMM3_ERR_STATE, "table destroyed twice");
    imm3_ctx *ctx = t->ctx;
    ctx_retain(ctx);
    struct Unref { imm3_ctx *c; ~Unref() { ctx_release(c); } } unref{ctx};
    imm3::GateScope gate(&ctx->gate);
    if (!ctx->closed && ctx->capture) return fail(IMM3_ERR_STATE, "a graph capture is open on this context");
    t->closed = true;
    if (!t->ctx->closed) {
        (void)hipSetDevice(t->ctx->device);
        (void)hipStreamSynchronize(t->ctx->stream);
    }
    table_release(t); // queries built on it keep the tile table (and its segments) alive until they are destroyed
    return IMM3_OK;
}

extern "C" int imm3_query_segment_starts(const imm3_query *q, int32_t *n_segments, int32_t *first_batch, int64_t *first_word) {
    if (!q) return fail(IMM3_ERR_ARG, "query is null");
    if (!q->table) { // one segment
        if (n_segments) *n_segments = 1;
        if (first_batch) { first_batch[0] = 0; first_batch[1] = (int32_t)q->layout->size.size(); }
        if (first_word) { first_word[0] = 0; first_word[1] = q->n_words; }
        return IMM3_OK;
    }
    const size_t n = q->table->segs.size();
    if (n_segments) *n_segments = (int32_t)n;
    if (first_batch) std::memcpy(first_batch, q->table->seg_first_batch.data(), (n + 1) * sizeof(int32_t));
    if (first_word) std::memcpy(first_word, q->table->seg_first_word.data(), (n + 1) * sizeof(int64_t));
    return IMM3_OK;
}

extern "C" int imm3_query_locate_rows(const imm3_query *q, const uint32_t *row_index, uint64_t n, uint32_t *segment_out, uint32_t *row_out) {
    if (!q || (n && !row_index)) return fail(IMM3_ERR_ARG, "null argument");
    for (uint64_t i = 0; i < n; ++i) {
        if (!q->table) {
            if (segment_out) segment_out[i] = 0;
            if (row_out) row_out[i] = row_index[i];
            continue;
        }
        const int64_t tile = row_index[i] >> 10;
        const auto &ts = q->table->tile_start;
        const size_t si = (size_t)(std::upper_bound(ts.begin(), ts.end(), tile) - ts.begin()) - 1;
        if (segment_out) segment_out[i] = (uint32_t)si;
        if (row_out) row_out[i] = (uint32_t)((tile - ts[si]) * kTileRows + (row_index[i] & (kTileRows - 1)));
    }
    return IMM3_OK;
}

extern "C" int imm3_query_destroy(imm3_query *q) {
    if (!q) return IMM3_OK;
    imm3_ctx *ctx = q->ctx;
    if (!ctx) { query_free(q); return IMM3_OK; }
    ctx_retain(ctx); // the gate lives in the context: keep it past query_free
    int rc = IMM3_OK;
    {
        imm3::GateScope gate(&ctx->gate);
        if (!ctx->closed && ctx->capture) rc = fail(IMM3_ERR_STATE, "a graph capture is open on this context");
        else {
            if (!ctx->closed) graphs_mark_stale(ctx, q); // a graph that recorded this query's runs points into its buffers
            query_free(q);
        }
    }
    ctx_release(ctx);
    return rc;
}

extern "C" int imm3_query_reserve_rows(imm3_query *q, uint64_t rows) {
    if (!q) return fail(IMM3_ERR_ARG, "query is null");
    CTX_LIVE(q->ctx);
    HIPCHK(hipSetDevice(q->ctx->device));
    const int rc = ensure_row_capacity(q, rows);
    if (rc) return rc;
    q->reserved = true;
    if (rows < (uint64_t)q->n_rows) { // (a reservation skips the first run's look at the count: it is the estimate)
        const int src = single_pass_stream_columns(q, rows);
        if (src) return src;
    }
    if (rows < (uint64_t)q->n_rows) single_pass_adapt(q, rows, -1); // (the reservation bounds the survivors)
    return IMM3_OK;
}

// ---------------------------------------------------------------------------------------------
// results
// ---------------------------------------------------------------------------------------------
extern "C" int imm3_query_layout(const imm3_query *q, int32_t *n_batches, int64_t *total_words, int64_t *n_rows) {
    if (!q) return fail(IMM3_ERR_ARG, "query is null");
    if (n_batches) *n_batches = (int32_t)(q->table ? q->table->batch_size.size() : q->layout->size.size());
    if (total_words) *total_words = q->n_words;
    if (n_rows) *n_rows = q->n_rows;
    return IMM3_OK;
}

extern "C" int imm3_query_batches(const imm3_query *q, int32_t *batch_size, int32_t *batch_oid, int64_t *batch_word_off) {
    if (!q) return fail(IMM3_ERR_ARG, "query is null");
    if (q->table) {
        const imm3_table *t = q->table;
        const size_t nb = t->batch_size.size();
        if (batch_size && nb) std::memcpy(batch_size, t->batch_size.data(), nb * sizeof(int32_t));
        if (batch_oid)
            for (size_t k = 0; k < nb; ++k) batch_oid[k] = (int32_t)((uint32_t)t->batch_k[k] * (uint32_t)q->table_block_size); // vecCounter * table.blockSize
        if (batch_word_off && nb) std::memcpy(batch_word_off, t->batch_word_off.data(), nb * sizeof(int64_t));
        return IMM3_OK;
    }
    const SegLayout &L = *q->layout;
    const size_t nb = L.size.size();
    if (batch_size && nb) std::memcpy(batch_size, L.size.data(), nb * sizeof(int32_t));
    if (batch_oid)
        for (size_t k = 0; k < nb; ++k) batch_oid[k] = (int32_t)((uint32_t)k * (uint32_t)q->table_block_size); // vecCounter * table.blockSize (Scan.scala:60)
    if (batch_word_off && nb) std::memcpy(batch_word_off, L.word_off.data(), nb * sizeof(int64_t));
    return IMM3_OK;
}

extern "C" int imm3_query_log_counts(imm3_query *q, uint64_t *device_log, uint64_t capacity) {
    if (!q) return fail(IMM3_ERR_ARG, "query is null");
    CTX_LIVE(q->ctx);
    HIPCHK(hipSetDevice(q->ctx->device));
    const unsigned long long v[3] = {(unsigned long long)(uintptr_t)device_log, 0ULL, device_log ? (unsigned long long)capacity : 0ULL};
    HIPCHK(hipMemcpyAsync(q->d_total + 5, v, sizeof(v), hipMemcpyHostToDevice, q->ctx->stream));
    HIPCHK(hipStreamSynchronize(q->ctx->stream)); // `v` is a stack array; also orders the switch after earlier runs
    q->count_log_on = device_log != nullptr;
    return IMM3_OK;
}

// the offsets scan over the bitmap of the last run (for a gather from the bitmap): tile offsets and chunk sums
static int scan_offsets(imm3_query *q) {
    if (q->run.offsets_valid || q->n_tiles <= 0) return IMM3_OK;
    ScanArgs sa;
    std::memset(&sa, 0, sizeof(sa));
    sa.bitmap = q->d_bitmap;
    sa.tile_offsets = q->d_tile_offsets;
    sa.chunk_sums = q->d_chunk_sums;
    sa.n_tiles = q->n_tiles;
    sa.scanned_tiles = q->run.select_partial ? q->d_total + kFinishLimitTiles : nullptr;
    launch_scan(sa, q->ctx->stream, nullptr, nullptr); // (finish = null: the count is already published)
    HIPCHK(hipGetLastError());
    q->run.offsets_valid = true;
    return IMM3_OK;
}

// Did the query's last single-pass launch give up on its rows?  `head` = the first kFinishDense + 1 words of the finish block as
// fetched AFTER that launch: its flags are tagged with its epoch, and the launch bumped the run counter exactly once.
static unsigned long long single_pass_flags(const unsigned long long *head) {
    const unsigned long long status = head[kFinishStatus], epoch_run = head[kFinishEpoch] - 1ULL;
    if (((status >> kStatusEpochShift) & kStatusEpochMask) != (epoch_run & kStatusEpochMask)) return 0ULL; // (an earlier run's flags)
    return status & (kStatusAbandoned | kStatusBusy);
}

// The last run was a records run that stored no bitmap (run_select: bitmap_lazy): a getter wants it -- the select chain runs once
// more, plainly.  The rows that run emitted stay what they are (the same rows); a later re-gather takes them from the bitmap.
static int settle_lazy_bitmap(imm3_query *q) {
    if (q->run.bitmap_valid || !q->run.bitmap_lazy) return IMM3_OK;
    if (q->ctx->capture) return fail(IMM3_ERR_STATE, "a graph capture is open on this context");
    return run_select(q, SEL_WHOLE | SEL_PLAIN); // (offsets_valid stands: the offsets scan counted the same survivors from the records)
}

// A projection with a limit stops its scan when the limit is reached (run_select, chunks): the bitmap and the count then cover the
// tiles scanned so far.  The reference never sees the batches behind the limit either (Project.scala:73-80); a caller that asks for
// the segment's count or bitmap all the same gets them exact: the whole select runs now, once (the rows were emitted from the scanned
// prefix and stay what they are -- they are the first `limit` survivors either way).
static int settle_whole_select(imm3_query *q) {
    if (!q->run.select_partial) return IMM3_OK;
    if (q->ctx->capture) return fail(IMM3_ERR_STATE, "a graph capture is open on this context");
    const int rc = run_select(q, SEL_WHOLE);
    if (rc) return rc;
    q->run.offsets_valid = false;
    return IMM3_OK;
}

// Every getter's first step after a single-pass run: read the run's status word (with the count and the dense-range tally, one
// copy).  The count and the bitmap of a run are exact whatever the flags say (imm3_project.hip: a work-group that gives up on the
// rows goes on in count + bitmap mode); only the ROWS of a flagged run are incomplete, and they are gathered here from the bitmap
// (offsets scan + k_gather into the same arrays).  Abandoned (a prefix never came although the device was this launch's: not
// every work-group resident?): the query keeps the bitmap path from now on.  Busy (another launch of the kernel owned the device --
// also when that made other work-groups of this launch time out, flags = busy | abandoned): this run only.
static int settle_single_pass(imm3_query *q) {
    if (!q->run.ran_single_pass || q->run.sp_verified) return IMM3_OK;
    imm3_ctx *ctx = q->ctx;
    static_assert(kFinishStatus == 2 && kFinishEpoch < kFinishDense, "count, status word, run counter and dense tally are fetched together");
    unsigned long long head[kFinishDense + 1] = {0}; // {count, rows emitted, status, ..., run counter, dense ranges}
    HIPCHK(hipMemcpyAsync(head, q->d_total, sizeof(head), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    q->run.sp_verified = true;
    const unsigned long long flags = single_pass_flags(head);
    if (!flags) {
        if (!q->plan_have_density && head[0] > 0 && q->n_rows > 0) { // no sample: what this run saw -- ranges that outgrew their ring mean dense stretches
            const double sigma = (double)head[0] / (double)q->n_rows, n_ranges = (double)q->sp_spans * kProjectStreamers, dense = (double)head[kFinishDense];
            q->plan_density.sigma = sigma;
            q->plan_density.sloc = dense > 0.02 * n_ranges ? std::min(1.0, sigma * n_ranges / dense) : sigma;
            q->plan_density.full = q->plan_density.sloc >= 0.95 && q->plan_density.sloc > 1.5 * sigma ? 1.0 : 0.0;
            q->plan_have_density = true;
        }
        single_pass_adapt(q, head[0], (int64_t)head[kFinishDense]); // (later runs: P from the selectivity this run saw)
        if (!q->sp_narrow_checked) { // (once: the data do not change)
            q->sp_narrow_checked = true;
            single_pass_drop_if_narrow(q, head[0]);
        }
        return IMM3_OK;
    }
    if (flags & kStatusBusy) ++q->sp_busy_runs;
    else {
        ++q->sp_abandoned_runs;
        graphs_mark_stale(ctx, q); // (a recorded run would take the abandoned path again)
        q->single_pass = false;
    }
    q->run.ran_single_pass = false; // (the rows the getters see come from the bitmap path)
    q->run.stage_written = false;
    int rc = scan_offsets(q);
    if (rc) return rc;
    return q->n_tiles > 0 ? launch_project(q) : IMM3_OK;
}

static int settle_agg_select(imm3_query *q);
// The one settle path of the getters: each names what it needs of the last run, settle() runs those steps, always in this order.
// A step is a no-op unless the run record (q->run) says the run left that work undone.
enum SettleStep : unsigned {
    SETTLE_AGG_SELECT = 1u << 0,   // the select an aggregation fused into its launch (settle_agg_select)
    SETTLE_LAZY_BITMAP = 1u << 1,  // the bitmap a records run did not store (settle_lazy_bitmap)
    SETTLE_SINGLE_PASS = 1u << 2,  // a single-pass run's status word: its rows gathered again if it gave up on them (settle_single_pass)
    SETTLE_WHOLE_SELECT = 1u << 3, // the tiles a limit scan never reached (settle_whole_select)
    SETTLE_JOIN = 1u << 4,         // the count reduced on the aux stream, joined into the context's stream (join_total)
};
enum SettleNeed : unsigned {
    NEED_HOST_COUNT = SETTLE_AGG_SELECT | SETTLE_SINGLE_PASS | SETTLE_WHOLE_SELECT | SETTLE_JOIN,
    NEED_DEVICE_COUNT = SETTLE_AGG_SELECT | SETTLE_WHOLE_SELECT | SETTLE_JOIN, // (enqueued only: no host wait)
    NEED_BITMAP = SETTLE_AGG_SELECT | SETTLE_LAZY_BITMAP | SETTLE_SINGLE_PASS | SETTLE_WHOLE_SELECT,
    NEED_ROWS = SETTLE_SINGLE_PASS, // (settle_rows then looks at k_limit_gather's give-up tag itself)
};
static int settle(imm3_query *q, SettleNeed need) {
    int rc = IMM3_OK;
    if (need & SETTLE_AGG_SELECT) rc = settle_agg_select(q);
    if (!rc && (need & SETTLE_LAZY_BITMAP)) rc = settle_lazy_bitmap(q);
    if (!rc && (need & SETTLE_SINGLE_PASS)) rc = settle_single_pass(q);
    if (!rc && (need & SETTLE_WHOLE_SELECT)) rc = settle_whole_select(q);
    if (!rc && (need & SETTLE_JOIN)) rc = join_total(q, q->ctx->stream);
    return rc;
}

// The hand-off to device-side consumers of the count word (imm3_query_join_count, imm3_comm_allreduce_count): it is the segment's
// count -- after a limit scan that stopped early the whole select runs first, enqueued, no host wait.
int imm3::join_query_count(imm3_query *q) { return settle(q, NEED_DEVICE_COUNT); }

// The query's select bitmap as imm3_query_bitmap would hand it out, left on the device (imm3_int_set_create's sources): what the last
// run left undone is settled; a query whose last run stored no bitmap (count-only), or that has never run, runs its select chain.
int imm3::query_bitmap_current(imm3_query *q) {
    int rc = q->run.ran_select ? settle(q, NEED_BITMAP) : IMM3_OK;
    if (rc) return rc;
    if (!q->run.ran_select || !q->run.bitmap_valid) {
        rc = run_select(q, SEL_WHOLE | SEL_PLAIN);
        if (rc) return rc;
        q->run.offsets_valid = false;
    }
    return q->run.bitmap_valid ? IMM3_OK : fail(IMM3_ERR_STATE, "internal: the select run stored no bitmap");
}
int imm3::segment_dense_column(imm3_ctx *ctx, const imm3_segment *seg, int32_t col) { return ensure_dense(ctx, seg, col); }

extern "C" int imm3_query_count(imm3_query *q, uint64_t *selected_rows) {
    if (!q || !selected_rows) return fail(IMM3_ERR_ARG, "null argument");
    CTX_LIVE(q->ctx);
    if (!q->run.ran_select) return fail(IMM3_ERR_STATE, "imm3_query_run has not been called");
    HIPCHK(hipSetDevice(q->ctx->device));
    const int rc = settle(q, NEED_HOST_COUNT);
    if (rc) return rc;
    unsigned long long total = 0, status = 0;
    HIPCHK(hipMemcpyAsync(&total, q->d_total, sizeof(total), hipMemcpyDeviceToHost, q->ctx->stream));
    if (q->run.has_pfor_pass) HIPCHK(hipMemcpyAsync(&status, q->d_total + 2, sizeof(status), hipMemcpyDeviceToHost, q->ctx->stream));
    HIPCHK(hipStreamSynchronize(q->ctx->stream));
    if (status) return fail(IMM3_ERR_LAYOUT, "malformed PFOR_INT block (width above 32, data past the block end, or count mismatch)");
    *selected_rows = total;
    return IMM3_OK;
}

extern "C" int imm3_query_bitmap(imm3_query *q, uint64_t *words_out, int64_t n_words) {
    if (!q) return fail(IMM3_ERR_ARG, "query is null");
    CTX_LIVE(q->ctx);
    if (!q->run.ran_select) return fail(IMM3_ERR_STATE, "imm3_query_run has not been called");
    if (n_words < 0 || n_words > q->n_words) return fail(IMM3_ERR_ARG, "n_words exceeds the bitmap");
    if (n_words && !words_out) return fail(IMM3_ERR_ARG, "words_out is null");
    HIPCHK(hipSetDevice(q->ctx->device));
    const int rc = settle(q, NEED_BITMAP);
    if (rc) return rc;
    if (!q->run.bitmap_valid) return fail(IMM3_ERR_STATE, "the last run was count-only (imm3_query_run_count): it stored no bitmap");
    if (n_words) HIPCHK(hipMemcpyAsync(words_out, q->d_bitmap, (size_t)n_words * sizeof(uint64_t), hipMemcpyDeviceToHost, q->ctx->stream));
    HIPCHK(hipStreamSynchronize(q->ctx->stream));
    return IMM3_OK;
}

static int settle_rows(imm3_query *q, uint64_t *rows) {
    CTX_LIVE(q->ctx);
    if (!q->run.ran_project) return fail(IMM3_ERR_STATE, "no projection has been run (n_proj == 0 or imm3_query_run not called)");
    HIPCHK(hipSetDevice(q->ctx->device));
    const int src = settle(q, NEED_ROWS);
    if (src) return src;
    unsigned long long emit = 0;
    if (q->n_tiles > 0 && q->run.limit_gather_ran) {
        // k_limit_gather's look-back is bounded: a launch whose wait ran out tagged finish[kFinishLimitGaveUp] with its run and
        // wrote only some of the rows -- gather them the two-launch way (one copy brings the row count, the epoch and the tag)
        unsigned long long head[kFinishLimitGaveUp + 1];
        HIPCHK(hipMemcpyAsync(head, q->d_total, sizeof(head), hipMemcpyDeviceToHost, q->ctx->stream));
        HIPCHK(hipStreamSynchronize(q->ctx->stream));
        emit = head[1];
        if (head[kFinishLimitGaveUp] == (((head[kFinishEpoch] & 0x7FFFFFULL) << 1) | 1ULL)) {
            ++q->limit_gather_gave_up;
            q->run.limit_gather_ran = false;
            int rc = scan_offsets(q);
            if (rc) return rc;
            rc = launch_project(q);
            if (rc) return rc;
            HIPCHK(hipStreamSynchronize(q->ctx->stream));
        }
    } else if (q->n_tiles > 0) {
        HIPCHK(hipMemcpyAsync(&emit, q->d_n_emit, sizeof(emit), hipMemcpyDeviceToHost, q->ctx->stream));
        HIPCHK(hipStreamSynchronize(q->ctx->stream));
    }
    if (emit > q->cap_rows || q->run.rows_moved) {
        // the reservation was too small: grow and gather again (offsets are still valid; a single-pass run made none:
        // they come from the bitmap now) -- or a reservation behind the run moved the arrays: the rows are gathered into the new ones
        int rc = emit > q->cap_rows ? ensure_row_capacity(q, q->reserved ? emit : std::min<unsigned long long>((unsigned long long)std::max<int64_t>(q->n_rows, 1), emit + emit / 8 + 1024)) : IMM3_OK;
        if (rc) return rc;
        if (!q->run.stage_written) rc = settle_lazy_bitmap(q); // (records that the reservation's plan change released: the bitmap they stood for)
        if (rc) return rc;
        q->run.rows_moved = false;
        q->run.limit_gather_ran = false;
        rc = scan_offsets(q); // (a single-pass run made no offsets: they come from the bitmap now)
        if (rc) return rc;
        rc = launch_project(q); // (from the records when the run staged them, from the bitmap otherwise)
        if (rc) return rc;
        HIPCHK(hipStreamSynchronize(q->ctx->stream));
    }
    if (q->ordered) {
        // the one place that emits rows again is also the one that orders them again: whatever happened above (a single-pass run that
        // gave up on its rows, arrays that were outgrown) went through launch_project, which cleared order_valid
        if (q->n_tiles <= 0) emit = 0;
        else {
            if (!q->run.order_valid) {
                const int rc = run_order(q);
                if (rc) return rc;
            }
            uint32_t st[OW_WORDS];
            HIPCHK(hipMemcpyAsync(st, q->d_order_state, sizeof(st), hipMemcpyDeviceToHost, q->ctx->stream));
            HIPCHK(hipStreamSynchronize(q->ctx->stream));
            emit = st[OW_N_OUT];
            if (q->order_counted != q->order_launches) { // (each enqueued order is counted once, by the path the device took)
                q->order_counted = q->order_launches;
                if (st[OW_SELECT]) ++q->order_select_runs;
                else ++q->order_full_runs;
            }
        }
    }
    *rows = emit;
    return IMM3_OK;
}

extern "C" int imm3_query_row_count(imm3_query *q, uint64_t *rows) {
    if (!q || !rows) return fail(IMM3_ERR_ARG, "null argument");
    return settle_rows(q, rows);
}

extern "C" int imm3_query_fetch_rows(imm3_query *q, uint32_t *row_index_out, void *const *col_out, uint64_t max_rows) {
    if (!q) return fail(IMM3_ERR_ARG, "query is null");
    CTX_LIVE(q->ctx);
    uint64_t rows = 0;
    const int rc = settle_rows(q, &rows);
    if (rc) return rc;
    const uint64_t n = std::min(rows, max_rows);
    hipStream_t s = q->ctx->stream;
    if (n) {
        // (an ordered query: the ordered arrays -- the unordered projection stays where it was)
        if (row_index_out) HIPCHK(hipMemcpyAsync(row_index_out, q->ordered ? q->d_order_row_index : q->d_row_index, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        for (size_t j = 0; j < q->proj.size(); ++j) {
            if (!col_out || !col_out[j]) continue;
            const SegCol &sc = q->seg->cols[(size_t)q->used[(size_t)q->proj[j]]];
            HIPCHK(hipMemcpyAsync(col_out[j], q->ordered ? q->d_order_proj[j] : q->d_proj[j], n * (uint64_t)sc.width, hipMemcpyDeviceToHost, s));
        }
    }
    HIPCHK(hipStreamSynchronize(s));
    return IMM3_OK;
}

extern "C" int imm3_query_device_ptr(imm3_query *q, int32_t which, void **ptr) {
    if (!q || !ptr) return fail(IMM3_ERR_ARG, "null argument");
    switch (which) {
    case 0: *ptr = q->d_bitmap; return IMM3_OK;
    case 1: *ptr = q->d_total; return IMM3_OK;
    case 2: *ptr = q->d_row_index; return IMM3_OK;
    case 3: *ptr = q->d_n_emit; return IMM3_OK;
    case 4: *ptr = q->d_total + kFinishStatus; return IMM3_OK; // the status word (imm3.h: which device-side consumers must look at it)
    default:
        // an ORDERED query's arrays sit at a base of their own, far from 16+j (a SELECT list has no bound: 16+j runs on)
        if (q->ordered && which == IMM3_PTR_ORDER_ROW_INDEX) { *ptr = q->d_order_row_index; return IMM3_OK; }
        if (q->ordered && which == IMM3_PTR_ORDER_ROW_COUNT) { *ptr = q->d_order_state ? q->d_order_state + OW_N_OUT : nullptr; return IMM3_OK; }
        if (q->ordered && which >= IMM3_PTR_ORDER_COLUMN && (size_t)(which - IMM3_PTR_ORDER_COLUMN) < q->proj.size()) {
            const size_t j = (size_t)(which - IMM3_PTR_ORDER_COLUMN);
            *ptr = j < q->d_order_proj.size() ? q->d_order_proj[j] : nullptr;
            return IMM3_OK;
        }
        if (which >= 16 && (size_t)(which - 16) < q->d_proj.size()) {
            *ptr = q->d_proj[(size_t)(which - 16)];
            return IMM3_OK;
        }
        return fail(IMM3_ERR_ARG, "unknown device pointer id");
    }
}

extern "C" int imm3_query_plan(const imm3_query *q, int64_t *out, int32_t n) {
    if (!q || !out) return fail(IMM3_ERR_ARG, "null argument");
    const int64_t v[15] = {q->single_pass ? 1 : 0, q->sp_P, q->sp_grid, q->sp_spans, q->d_stage_rec ? 1 : 0,
                           (q->single_pass || q->d_stage_rec) ? rec_layout(q->stage_kinds, -1).dwords : 0, q->run.ran_single_pass ? 1 : 0, (int64_t)q->run_syncs,
                           (int64_t)q->sp_abandoned_runs, (int64_t)q->sp_busy_runs, (int64_t)q->limit_gather_gave_up,
                           (int64_t)q->order_select_runs, (int64_t)q->order_full_runs, (int64_t)q->order_launches,
                           q->hi16_ran ? 1 : 0};
    for (int32_t i = 0; i < n && i < 15; ++i) out[i] = v[i];
    return IMM3_OK;
}

// The word a plane scan's refining tiles set (finish[kFinishHi16Refined]), read and cleared: it speaks of the runs since the last
// call.  Waits for the context's stream; refused inside an open capture.
extern "C" int imm3_query_hi16_refined(imm3_query *q, int32_t *refined) {
    if (!q || !refined) return fail(IMM3_ERR_ARG, "null argument");
    if (q->ctx->capture) return fail(IMM3_ERR_STATE, "a graph capture is open");
    *refined = 0;
    if (!q->d_total) return IMM3_OK;
    unsigned long long w = 0;
    HIPCHK(hipMemcpyAsync(&w, q->d_total + kFinishHi16Refined, sizeof(w), hipMemcpyDeviceToHost, q->ctx->stream));
    HIPCHK(hipStreamSynchronize(q->ctx->stream));
    if (w) HIPCHK(hipMemsetAsync(q->d_total + kFinishHi16Refined, 0, sizeof(w), q->ctx->stream));
    *refined = w ? 1 : 0;
    return IMM3_OK;
}

// ---------------------------------------------------------------------------------------------
// group-by aggregation (ProjectAggOp)
// ---------------------------------------------------------------------------------------------
static int query_create_agg_impl(imm3_ctx *ctx, const imm3_segment *seg, const imm3_table *table,
                                 const int32_t *used_cols, int32_t n_used,
                                 const imm3_select *sels, int32_t n_sels,
                                 const int32_t *group_cols, int32_t n_group,
                                 const imm3_aggregate *aggs, int32_t n_aggs,
                                 int32_t table_block_size, imm3_query **out, bool wide_keys,
                                 const int32_t *prog = nullptr, int32_t n_prog = 0, bool tree = false) {
    if (!out) return fail(IMM3_ERR_ARG, "out is null");
    *out = nullptr;
    if (n_group < 0 || n_group > kMaxGroupCols || (n_group > 0 && !group_cols)) return fail(IMM3_ERR_ARG, "0..4 group columns are supported on the GPU path");
    if (n_aggs < 1 || n_aggs > kMaxAggs || !aggs) return fail(IMM3_ERR_ARG, "1..4 aggregates are supported on the GPU path");
    imm3_query *q = nullptr;
    std::vector<int32_t> row_cols(group_cols, group_cols + n_group); // read row by row: PFOR_INT ones through their decoded form
    for (int32_t j = 0; j < n_aggs; ++j) row_cols.push_back(aggs[j].column);
    int rc = query_create_impl(ctx, seg, table, used_cols, n_used, sels, n_sels, nullptr, 0, 0, table_block_size, row_cols, &q, prog, n_prog, tree);
    if (rc) return rc;
    std::unique_ptr<imm3_query, void (*)(imm3_query *)> guard(q, query_free);
    int key_bytes = 0;
    for (int32_t g = 0; g < n_group; ++g) {
        if (group_cols[g] < 0 || group_cols[g] >= n_used) return fail(IMM3_ERR_ARG, "group column is not among the used columns");
        key_bytes += seg->cols[(size_t)q->used[(size_t)group_cols[g]]].width;
    }
    if (!wide_keys && key_bytes > 8) return fail(IMM3_ERR_ARG, "group key wider than 8 bytes is not supported on the GPU path");
    if (key_bytes > kGroupKeyMaxWidth)
        return fail(IMM3_ERR_ARG, "group key wider than " + std::to_string(kGroupKeyMaxWidth) + " bytes is not supported on the GPU path");
    const bool has_batches = table ? !table->batch_size.empty() : !q->layout->size.empty();
    bool has_distinct = false;
    for (int32_t j = 0; j < n_aggs; ++j) {
        if (aggs[j].column < 0 || aggs[j].column >= n_used) return fail(IMM3_ERR_ARG, "aggregate column is not among the used columns");
        const SegCol &sc = seg->cols[(size_t)q->used[(size_t)aggs[j].column]];
        const bool is_str = sc.vcodec == IMM3_DENSE_STRING;
        if (aggs[j].kind != IMM3_AGG_COUNT && aggs[j].kind != IMM3_AGG_MIN && aggs[j].kind != IMM3_AGG_MAX && aggs[j].kind != IMM3_AGG_SUM &&
            aggs[j].kind != IMM3_AGG_COUNT_DISTINCT)
            return fail(IMM3_ERR_ARG, "Unknown Aggregate type");
        if (aggs[j].kind == IMM3_AGG_COUNT_DISTINCT) {
            // an entry of the pair set holds the value's raw bytes in 32 bits.  OUT OF SCOPE: values wider than 4 bytes
            const bool ok = is_str ? (sc.width >= 1 && sc.width <= kDistinctMaxWidth) : (sc.width == 1 || sc.width == 4);
            if (!ok)
                return fail(IMM3_ERR_ARG, "COUNT_DISTINCT takes int32, int8 and string columns of at most " + std::to_string(kDistinctMaxWidth) +
                                              " bytes on the GPU path (this column is " + std::to_string(sc.width) + " bytes wide)");
            has_distinct = true;
        }
        // ProjectAggregate.scala:176-220: a String vector only takes CountAggr / MaxStringAggr (AvgDoubleAggr's sum is numeric only)
        if (has_batches && is_str && (aggs[j].kind == IMM3_AGG_MIN || aggs[j].kind == IMM3_AGG_SUM)) return fail(IMM3_ERR_UNSUPPORTED_VECTOR, "bad aggregator for this data type");
        if (is_str && aggs[j].kind == IMM3_AGG_MAX && sc.width > kStrMaxWidth)
            return fail(IMM3_ERR_ARG, "MAX over strings wider than " + std::to_string(kStrMaxWidth) + " bytes is not supported on the GPU path");
    }
    q->is_agg = true;
    q->agg_wide_key = key_bytes > 8;
    q->group_cols.assign(group_cols, group_cols + n_group);
    q->aggs.assign(aggs, aggs + n_aggs);
    {   // SelectOp fused into the aggregation launch (k_group_agg_lanes' FUSED instances; whether the lanes form takes the query is
        // the launcher's call at run time)
        bool ok = !table && !q->ragged && !q->always_false && has_batches && q->n_rows > 0 && q->preds.size() <= (size_t)kMaxAggPreds &&
                  !q->is_expr && // (a select tree's launch writes the bitmap, the aggregation reads it)
                  !has_distinct; // (k_distinct_mark walks the bitmap; the fast forms decline the kind anyway: group_agg_fast_ok)
        for (const auto &fp : q->preds)
            ok = ok && !fp.pfor && !fp.has_list && (fp.kind == KIND_I8 || fp.kind == KIND_I32) && col_flat(seg->cols[(size_t)fp.seg_col]) != nullptr;
        q->agg_fusable = ok;
    }
    // table capacity: twice the number of possible groups, bounded by the rows and by 2^27 slots (a wide key's domain saturates)
    double domain = 1.0;
    for (int b = 0; b < key_bytes; ++b) domain *= 256.0;
    const double bound = std::min<double>(domain, (double)std::max<int64_t>(q->n_rows, 1));
    uint64_t slots = 1024;
    while ((double)slots < 2.0 * bound && slots < (1ULL << 27)) slots <<= 1;
    q->agg_mask = (uint32_t)(slots - 1);
    HIPCHK(hipSetDevice(ctx->device));
    void *p = nullptr;
    const size_t n = (size_t)slots + 1;
    HIPCHK(pool_alloc(ctx, &p, n * sizeof(unsigned long long))); q->d_akeys = (unsigned long long *)p;
    HIPCHK(pool_alloc(ctx, &p, n * sizeof(uint32_t))); q->d_afirst = (uint32_t *)p;
    HIPCHK(pool_alloc(ctx, &p, n * sizeof(unsigned long long))); q->d_acounts = (unsigned long long *)p;
    HIPCHK(pool_alloc(ctx, &p, n * kMaxAggs * sizeof(long long))); q->d_avals = (long long *)p;
    HIPCHK(pool_alloc(ctx, &p, 2 * sizeof(uint32_t))); q->d_ameta = (uint32_t *)p;
    for (int32_t j = 0; j < n_aggs; ++j) { // a string MAX wider than 8 bytes: the refine passes' bitmap and chunk table (no per-row buffer)
        const SegCol &sc = seg->cols[(size_t)q->used[(size_t)aggs[j].column]];
        if (sc.vcodec != IMM3_DENSE_STRING || aggs[j].kind != IMM3_AGG_MAX || sc.width <= 8) continue;
        HIPCHK(pool_alloc(ctx, &p, (size_t)std::max<int64_t>(q->n_words, 1) * sizeof(uint64_t))); q->d_alive[j] = (uint64_t *)p;
        HIPCHK(pool_alloc(ctx, &p, (size_t)((sc.width + 7) / 8 - 1) * n * sizeof(unsigned long long))); q->d_chunks[j] = (unsigned long long *)p;
    }
    for (int32_t j = 0; j < n_aggs; ++j) { // COUNT_DISTINCT: the pair set, sized here once (imm3_distinct_plan.h)
        if (aggs[j].kind != IMM3_AGG_COUNT_DISTINCT) continue;
        const SegCol &sc = seg->cols[(size_t)q->used[(size_t)aggs[j].column]];
        const int64_t entries = distinct_capacity(q->n_rows, key_bytes, sc.width);
        if (entries < 0)
            return fail(IMM3_ERR_ARG, "COUNT_DISTINCT: the pair set of this query would need more than 2^28 entries (2 GiB; more than 2^27 rows)");
        HIPCHK(pool_alloc(ctx, &p, (size_t)entries * sizeof(unsigned long long))); q->d_dset[j] = (unsigned long long *)p;
        q->dset_entries[j] = (uint64_t)entries;
    }
    *out = guard.release();
    return IMM3_OK;
}

extern "C" int imm3_query_create_agg(imm3_ctx *ctx, const imm3_segment *seg,
                                     const int32_t *used_cols, int32_t n_used,
                                     const imm3_select *sels, int32_t n_sels,
                                     const int32_t *group_cols, int32_t n_group,
                                     const imm3_aggregate *aggs, int32_t n_aggs,
                                     int32_t table_block_size, imm3_query **out) {
    return query_create_agg_impl(ctx, seg, nullptr, used_cols, n_used, sels, n_sels, group_cols, n_group, aggs, n_aggs, table_block_size, out, false);
}

extern "C" int imm3_query_create_agg_wide(imm3_ctx *ctx, const imm3_segment *seg,
                                          const int32_t *used_cols, int32_t n_used,
                                          const imm3_select *sels, int32_t n_sels,
                                          const int32_t *group_cols, int32_t n_group,
                                          const imm3_aggregate *aggs, int32_t n_aggs,
                                          int32_t table_block_size, imm3_query **out) {
    return query_create_agg_impl(ctx, seg, nullptr, used_cols, n_used, sels, n_sels, group_cols, n_group, aggs, n_aggs, table_block_size, out, true);
}

extern "C" int imm3_query_create_agg_expr(imm3_ctx *ctx, const imm3_segment *seg,
                                          const int32_t *used_cols, int32_t n_used,
                                          const imm3_select *leaves, int32_t n_leaves, const int32_t *prog, int32_t n_prog,
                                          const int32_t *group_cols, int32_t n_group,
                                          const imm3_aggregate *aggs, int32_t n_aggs,
                                          int32_t table_block_size, imm3_query **out) {
    return query_create_agg_impl(ctx, seg, nullptr, used_cols, n_used, leaves, n_leaves, group_cols, n_group, aggs, n_aggs, table_block_size, out, true, prog, n_prog, true);
}

extern "C" int imm3_query_create_table_agg(imm3_ctx *ctx, const imm3_table *table,
                                           const int32_t *used_cols, int32_t n_used,
                                           const imm3_select *sels, int32_t n_sels,
                                           const int32_t *group_cols, int32_t n_group,
                                           const imm3_aggregate *aggs, int32_t n_aggs,
                                           int32_t table_block_size, imm3_query **out) {
    if (!table || table->segs.empty()) return fail(IMM3_ERR_ARG, "table is null or empty");
    return query_create_agg_impl(ctx, table->segs[0], table, used_cols, n_used, sels, n_sels, group_cols, n_group, aggs, n_aggs, table_block_size, out, false);
}

extern "C" int imm3_query_create_table_agg_wide(imm3_ctx *ctx, const imm3_table *table,
                                                const int32_t *used_cols, int32_t n_used,
                                                const imm3_select *sels, int32_t n_sels,
                                                const int32_t *group_cols, int32_t n_group,
                                                const imm3_aggregate *aggs, int32_t n_aggs,
                                                int32_t table_block_size, imm3_query **out) {
    if (!table || table->segs.empty()) return fail(IMM3_ERR_ARG, "table is null or empty");
    return query_create_agg_impl(ctx, table->segs[0], table, used_cols, n_used, sels, n_sels, group_cols, n_group, aggs, n_aggs, table_block_size, out, true);
}

extern "C" int imm3_query_create_table_agg_expr(imm3_ctx *ctx, const imm3_table *table,
                                                const int32_t *used_cols, int32_t n_used,
                                                const imm3_select *leaves, int32_t n_leaves, const int32_t *prog, int32_t n_prog,
                                                const int32_t *group_cols, int32_t n_group,
                                                const imm3_aggregate *aggs, int32_t n_aggs,
                                                int32_t table_block_size, imm3_query **out) {
    if (!table || table->segs.empty()) return fail(IMM3_ERR_ARG, "table is null or empty");
    return query_create_agg_impl(ctx, table->segs[0], table, used_cols, n_used, leaves, n_leaves, group_cols, n_group, aggs, n_aggs, table_block_size, out, true, prog, n_prog, true);
}

static void fill_agg_args(const imm3_query *q, AggArgs &a) {
    std::memset(&a, 0, sizeof(a));
    a.bitmap = q->d_bitmap;
    a.n_words = q->n_words;
    a.n_tiles = q->n_tiles;
    a.n_rows = q->n_rows;
    a.word_row_base = q->d_word_row_base;
    int shift = 0;
    for (size_t g = 0; g < q->group_cols.size(); ++g) {
        const SegCol &sc = q->seg->cols[(size_t)q->used[(size_t)q->group_cols[g]]];
        a.groups[g].data = col_flat(sc);
        a.groups[g].tile_ptrs = q->table ? (const void *const *)q->table->d_tile_ptrs[(size_t)q->used[(size_t)q->group_cols[g]]] : nullptr;
        a.groups[g].width = sc.width;
        a.groups[g].shift = shift;
        shift += sc.width;
    }
    a.n_group = (int32_t)q->group_cols.size();
    for (size_t j = 0; j < q->aggs.size(); ++j) {
        const SegCol &sc = q->seg->cols[(size_t)q->used[(size_t)q->aggs[j].column]];
        a.aggs[j].data = col_flat(sc);
        a.aggs[j].tile_ptrs = q->table ? (const void *const *)q->table->d_tile_ptrs[(size_t)q->used[(size_t)q->aggs[j].column]] : nullptr;
        a.aggs[j].width = sc.width;
        a.aggs[j].kind = q->aggs[j].kind;
        a.aggs[j].is_str = sc.vcodec == IMM3_DENSE_STRING;
        a.aggs[j].chunks = q->d_chunks[j];
        a.aggs[j].alive = q->d_alive[j];
        a.aggs[j].dset = q->d_dset[j];
        a.aggs[j].dset_mask = q->d_dset[j] ? (uint32_t)(q->dset_entries[j] - 1) : 0u;
    }
    a.n_agg = (int32_t)q->aggs.size();
    if (q->agg_fusable && q->ctx->filter_variant != TV_AGG_SELECT_LAUNCH) { // (filter launch + aggregation launch, as before round 5)
        int first_value = -1; // the aggregate whose rows the lanes form keeps in registers: the first one that is not a count
        for (size_t j = 0; j < q->aggs.size() && first_value < 0; ++j)
            if (q->aggs[j].kind != IMM3_AGG_COUNT) first_value = (int)j;
        for (const auto &fp : q->preds) {
            AggPred &f = a.fused[a.n_fused++];
            const SegCol &sc = q->seg->cols[(size_t)fp.seg_col];
            f.data = col_flat(sc);
            f.width = sc.width;
            f.lo = (int32_t)fp.lo;
            f.hi = (int32_t)fp.hi;
            f.share = first_value >= 0 && q->used[(size_t)q->aggs[(size_t)first_value].column] == fp.seg_col ? 1 : 0;
        }
        a.fused_all = q->preds.empty() ? 1 : 0;
    }
    a.keys = q->d_akeys;
    a.first = q->d_afirst;
    a.counts = q->d_acounts;
    a.vals = q->d_avals;
    a.mask = q->agg_mask;
    a.n_groups = q->d_ameta;
    a.overflow = q->d_ameta + 1;
    a.out_cap = q->out_cap;
    a.out_keys = q->d_okeys;
    a.out_first = q->d_ofirst;
    a.out_counts = q->d_ocounts;
    a.out_vals = q->d_ovals;
    a.wide_key = q->agg_wide_key ? 1 : 0;
    a.hash_mask = q->ctx->filter_variant == TV_AGG_WEAK_HASH ? 0x7u : 0xFFFFFFFFu;
}

static void agg_launch_args(const imm3_query *q, AggArgs &a) {
    fill_agg_args(q, a);
    // (tools/aggexp.py: TV_AGG_FORM + form starts the chain at that form)
    const int fv = q->ctx->filter_variant;
    a.first_form = agg_form_variant(fv) >= 0 ? agg_form_variant(fv) : q->agg_first_form; // (agg_first_form: past the forms this query's keys overflowed)
    a.ablate = agg_ablation(fv);
}
// will this run's aggregation launch evaluate the select chain itself?  (then no select launch precedes it)
bool imm3::agg_run_fuses(const imm3_query *q) {
    if (!q->is_agg || !q->agg_fusable || q->count_log_on) return false; // (a count log wants every run's count on the device: the select launch produces it)
    AggArgs a;
    agg_launch_args(q, a);
    return group_agg_fuses_select(a);
}
// A getter wants the bitmap or the selected-row count of an aggregation whose last run fused the select: the select chain runs now.
static int settle_agg_select(imm3_query *q) {
    if (!q->run.agg_select_skipped) return IMM3_OK;
    if (q->ctx->capture) return fail(IMM3_ERR_STATE, "a graph capture is open on this context");
    const int rc = run_select(q, SEL_DEFAULT);
    if (rc) return rc;
    q->run.agg_select_skipped = false;
    return IMM3_OK;
}

// The aggregation launch (timed as kernel 4).  A string MAX wider than 8 bytes adds a zeroing launch before it and its refine passes
// after it (kernel 6, one record per pass): a fixed sequence for the query, so a recorded run replays it whole.
static int launch_agg(imm3_query *q, const AggArgs &a, hipStream_t s, bool timed) {
    imm3_ctx *ctx = q->ctx;
    bool wide = false;
    for (int j = 0; j < a.n_agg; ++j) wide |= a.aggs[j].alive != nullptr;
    if (wide) launch_strmax_init(a, s);
    for (int j = 0; j < a.n_agg; ++j) { // COUNT_DISTINCT: every run starts from the empty set (kernel 11: one record per clear)
        if (!a.aggs[j].dset) continue;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (timed) {
            LaunchTimer t(ctx, 11);
            e0 = t.start;
            e1 = t.stop;
        }
        if (e0) HIPCHK(hipEventRecord(e0, s));
        HIPCHK(hipMemsetAsync(a.aggs[j].dset, 0xFF, ((size_t)a.aggs[j].dset_mask + 1) * sizeof(unsigned long long), s));
        if (e1) HIPCHK(hipEventRecord(e1, s));
    }
    if (timed) {
        LaunchTimer t(ctx, 4);
        q->agg_form_ran = launch_group_agg(a, s, t.start, t.stop);
    } else q->agg_form_ran = launch_group_agg(a, s, nullptr, nullptr);
    for (int j = 0; j < a.n_agg; ++j) {
        if (!a.aggs[j].alive) continue;
        for (int k = 1; k < (a.aggs[j].width + 7) / 8; ++k) {
            if (timed) {
                LaunchTimer t(ctx, 6);
                launch_strmax_refine(a, j, k, s, t.start, t.stop);
            } else launch_strmax_refine(a, j, k, s, nullptr, nullptr);
        }
    }
    for (int j = 0; j < a.n_agg; ++j) { // COUNT_DISTINCT: the mark pass (kernel 10), behind the table's last writer
        if (!a.aggs[j].dset) continue;
        if (timed) {
            LaunchTimer t(ctx, 10);
            launch_distinct_mark(a, j, s, t.start, t.stop);
        } else launch_distinct_mark(a, j, s, nullptr, nullptr);
    }
    HIPCHK(hipGetLastError());
    return IMM3_OK;
}

int imm3::run_agg(imm3_query *q) {
    imm3_ctx *ctx = q->ctx;
    AggArgs a;
    agg_launch_args(q, a);
    if (!q->run.agg_select_skipped) { a.n_fused = 0; a.fused_all = 0; } // (the select ran: the bitmap is what this launch reads)
    const int rc = launch_agg(q, a, ctx->stream, true);
    if (rc) return rc;
    q->run.ran_agg = true;
    q->run.group_order_valid = false; // (new groups: an ordered view is made again when a getter asks)
    return IMM3_OK;
}

// collect the occupied slots; grows the dense output and collects again if it was too small
static int settle_groups(imm3_query *q, uint32_t *n_groups) {
    CTX_LIVE(q->ctx);
    if (!q->is_agg || !q->run.ran_agg) return fail(IMM3_ERR_STATE, "no aggregation has been run");
    imm3_ctx *ctx = q->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    for (int attempt = 0; attempt < 5; ++attempt) {
        AggArgs a;
        fill_agg_args(q, a);
        HIPCHK(hipMemsetAsync(q->d_ameta, 0, sizeof(uint32_t), s)); // n_groups only; keep the overflow flag
        launch_group_collect(a, s);
        HIPCHK(hipGetLastError());
        uint32_t meta[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(meta, q->d_ameta, sizeof(meta), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (meta[1] == 2 || meta[1] == 3) { // a fast form's per-work-group table filled up: aggregate again with the next form
            AggArgs g;                       // (3: k_group_agg_lanes -> k_group_agg_direct; 2: -> the general kernel)
            fill_agg_args(q, g);
            // lanes (63 keys) -> lanes (127 keys) -> direct -> general
            q->agg_first_form = meta[1] == 3 ? (q->agg_first_form == AGG_FORM_LANES ? AGG_FORM_LANES_WIDE : AGG_FORM_DIRECT) : AGG_FORM_GENERAL;
            g.first_form = q->agg_first_form;
            {   // (the forms behind the 63-key lanes form read the bitmap: a run that fused the select has none yet -- and a count-only
                // run since then has stored none either: the chain runs for this launch, and imm3_query_bitmap goes on refusing)
                int arc = settle_agg_select(q);
                if (!arc && !q->run.bitmap_valid) {
                    if (q->ctx->capture) return fail(IMM3_ERR_STATE, "a graph capture is open on this context");
                    arc = run_select(q, SEL_DEFAULT);
                    q->run.bitmap_valid = false;
                }
                if (arc) return arc;
                g.n_fused = 0;
                g.fused_all = 0;
            }
            const int lrc = launch_agg(q, g, s, false);
            if (lrc) return lrc;
            continue;
        }
        if (meta[1]) return fail(IMM3_ERR_LAYOUT, "more distinct groups than the aggregation table holds (2^27)");
        if (meta[0] <= q->out_cap) { *n_groups = meta[0]; return IMM3_OK; }
        if (q->d_okeys) graphs_mark_stale(ctx, q);
        pool_release(ctx, q->d_okeys); pool_release(ctx, q->d_ofirst); pool_release(ctx, q->d_ocounts); pool_release(ctx, q->d_ovals);
        q->d_okeys = nullptr; q->d_ofirst = nullptr; q->d_ocounts = nullptr; q->d_ovals = nullptr;
        void *p = nullptr;
        const size_t n = meta[0];
        HIPCHK(pool_alloc(ctx, &p, n * sizeof(unsigned long long))); q->d_okeys = (unsigned long long *)p;
        HIPCHK(pool_alloc(ctx, &p, n * sizeof(uint32_t))); q->d_ofirst = (uint32_t *)p;
        HIPCHK(pool_alloc(ctx, &p, n * sizeof(unsigned long long))); q->d_ocounts = (unsigned long long *)p;
        HIPCHK(pool_alloc(ctx, &p, n * kMaxAggs * sizeof(long long))); q->d_ovals = (long long *)p;
        q->out_cap = meta[0];
    }
    return fail(IMM3_ERR_DEVICE, "group collection did not converge");
}

int imm3::query_groups(imm3_query *q, uint32_t *n_groups) { return settle_groups(q, n_groups); }
void imm3::query_agg_args(const imm3_query *q, AggArgs &a) { fill_agg_args(q, a); }

// bytes of the packed group key: the group columns' widths
static int32_t agg_key_bytes(const imm3_query *q) {
    int32_t kb = 0;
    for (int32_t g : q->group_cols) kb += q->seg->cols[(size_t)q->used[(size_t)g]].width;
    return kb;
}

extern "C" int imm3_query_agg_shape(const imm3_query *q, int32_t *n_group_cols, int32_t *n_aggs, int32_t *key_bytes) {
    if (!q) return fail(IMM3_ERR_ARG, "query is null");
    if (!q->is_agg) return fail(IMM3_ERR_ARG, "not an aggregation query");
    if (n_group_cols) *n_group_cols = (int32_t)q->group_cols.size();
    if (n_aggs) *n_aggs = (int32_t)q->aggs.size();
    if (key_bytes) *key_bytes = agg_key_bytes(q);
    return IMM3_OK;
}

extern "C" int imm3_query_group_count(imm3_query *q, uint32_t *n_groups) {
    if (!q || !n_groups) return fail(IMM3_ERR_ARG, "null argument");
    if (q->group_ordered || q->group_filtered) { // (imm3_query_set_group_order: min(groups, limit))
        CTX_LIVE(q->ctx);
        return group_order_settle(q, n_groups);
    }
    return settle_groups(q, n_groups);
}

// A wide-key query's packed key bytes of its n dense groups (k_group_collect's order), key_bytes each, gathered at their first rows
static int gather_group_keys(imm3_query *q, uint32_t n, std::vector<uint8_t> &out) {
    imm3_ctx *ctx = q->ctx;
    const int32_t kb = agg_key_bytes(q);
    out.assign((size_t)n * (size_t)kb, 0);
    if (!n || !kb) return IMM3_OK;
    std::unique_ptr<void, std::function<void(void *)>> d(nullptr, [ctx](void *p) { pool_release(ctx, p); });
    void *p = nullptr;
    HIPCHK(pool_alloc(ctx, &p, out.size()));
    d.reset(p);
    AggArgs a;
    fill_agg_args(q, a);
    launch_group_keys(a, n, kb, (uint8_t *)p, ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out.data(), p, out.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return IMM3_OK;
}

extern "C" int imm3_query_fetch_groups(imm3_query *q, uint64_t *keys, uint32_t *first_row, uint64_t *counts, int64_t *vals, uint32_t max_groups) {
    if (!q) return fail(IMM3_ERR_ARG, "query is null");
    CTX_LIVE(q->ctx);
    if (q->group_ordered || q->group_filtered) return group_order_fetch_groups(q, keys, first_row, counts, vals, max_groups); // (ordered on the device: only the groups asked for are copied)
    uint32_t n = 0;
    const int rc = settle_groups(q, &n);
    if (rc) return rc;
    std::vector<uint8_t> wk; // a wide key: its bytes (the table holds tags), keys[g] = the first 8 of them little-endian
    if (q->agg_wide_key && keys) {
        const int grc = gather_group_keys(q, n, wk);
        if (grc) return grc;
    }
    std::vector<unsigned long long> hk(n), hc(n);
    std::vector<uint32_t> hf(n);
    std::vector<long long> hv((size_t)n * kMaxAggs);
    hipStream_t s = q->ctx->stream;
    if (n) {
        HIPCHK(hipMemcpyAsync(hk.data(), q->d_okeys, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(hf.data(), q->d_ofirst, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(hc.data(), q->d_ocounts, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(hv.data(), q->d_ovals, (size_t)n * kMaxAggs * sizeof(long long), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    std::vector<uint32_t> order(n);
    for (uint32_t i = 0; i < n; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return hf[x] < hf[y]; }); // first-seen order
    const size_t na = q->aggs.size();
    for (uint32_t o = 0; o < n && o < max_groups; ++o) {
        const uint32_t i = order[o];
        if (keys && q->agg_wide_key) {
            const size_t kb = (size_t)agg_key_bytes(q);
            uint64_t k = 0;
            for (size_t b = 0; b < 8 && b < kb; ++b) k |= (uint64_t)wk[(size_t)i * kb + b] << (8 * b);
            keys[o] = k;
        } else if (keys) keys[o] = hk[i];
        if (first_row) first_row[o] = hf[i];
        if (counts) counts[o] = hc[i];
        if (vals)
            for (size_t j = 0; j < na; ++j)
                vals[(size_t)o * na + j] = q->aggs[j].kind == IMM3_AGG_COUNT ? (int64_t)hc[i] : (int64_t)hv[(size_t)i * kMaxAggs + j];
    }
    return IMM3_OK;
}

extern "C" int imm3_query_fetch_group_strings(imm3_query *q, int32_t agg, uint8_t *out, uint32_t max_groups) {
    if (!q) return fail(IMM3_ERR_ARG, "query is null");
    if (!q->is_agg) return fail(IMM3_ERR_ARG, "not an aggregation query");
    if (agg < 0 || agg >= (int32_t)q->aggs.size()) return fail(IMM3_ERR_ARG, "aggregate index out of range");
    const SegCol &sc = q->seg->cols[(size_t)q->used[(size_t)q->aggs[(size_t)agg].column]];
    if (q->aggs[(size_t)agg].kind != IMM3_AGG_MAX || sc.vcodec != IMM3_DENSE_STRING) return fail(IMM3_ERR_ARG, "the aggregate is not a MAX over a STRING column");
    if (!out && max_groups > 0) return fail(IMM3_ERR_ARG, "out is null");
    CTX_LIVE(q->ctx);
    if (q->group_ordered || q->group_filtered) return group_order_fetch_strings(q, agg, out, max_groups);
    uint32_t n = 0;
    const int rc = settle_groups(q, &n);
    if (rc) return rc;
    imm3_ctx *ctx = q->ctx;
    hipStream_t s = ctx->stream;
    const size_t w = (size_t)sc.width;
    const bool wide = q->d_chunks[agg] != nullptr;
    std::vector<uint32_t> hf(n);
    std::vector<long long> hv(wide ? 0 : (size_t)n * kMaxAggs);
    std::vector<uint8_t> hb(wide ? (size_t)n * w : 0);
    std::unique_ptr<void, std::function<void(void *)>> d(nullptr, [ctx](void *p) { pool_release(ctx, p); });
    if (n) {
        HIPCHK(hipMemcpyAsync(hf.data(), q->d_ofirst, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        if (wide) { // the exact values, assembled from the chunks on the device in the dense groups' order
            void *p = nullptr;
            HIPCHK(pool_alloc(ctx, &p, hb.size()));
            d.reset(p);
            AggArgs a;
            fill_agg_args(q, a);
            launch_strmax_collect(a, agg, n, (uint8_t *)p, s);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(hb.data(), p, hb.size(), hipMemcpyDeviceToHost, s));
        } else HIPCHK(hipMemcpyAsync(hv.data(), q->d_ovals, hv.size() * sizeof(long long), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    std::vector<uint32_t> order(n);
    for (uint32_t i = 0; i < n; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return hf[x] < hf[y]; }); // imm3_query_fetch_groups' order
    for (uint32_t o = 0; o < n && o < max_groups; ++o) {
        const uint32_t i = order[o];
        uint8_t *dst = out + (size_t)o * w;
        if (wide) std::memcpy(dst, hb.data() + (size_t)i * w, w);
        else { // (<= 8 bytes: the value packed big-endian)
            const unsigned long long v = (unsigned long long)hv[(size_t)i * kMaxAggs + (size_t)agg];
            for (size_t b = 0; b < w; ++b) dst[b] = (uint8_t)(v >> (8 * (w - 1 - b)));
        }
    }
    return IMM3_OK;
}

extern "C" int imm3_query_fetch_group_keys(imm3_query *q, uint8_t *out, uint32_t max_groups) {
    if (!q) return fail(IMM3_ERR_ARG, "query is null");
    if (!q->is_agg) return fail(IMM3_ERR_ARG, "not an aggregation query");
    if (!out && max_groups > 0) return fail(IMM3_ERR_ARG, "out is null");
    CTX_LIVE(q->ctx);
    if (q->group_ordered || q->group_filtered) return group_order_fetch_keys(q, out, max_groups);
    uint32_t n = 0;
    const int rc = settle_groups(q, &n);
    if (rc) return rc;
    hipStream_t s = q->ctx->stream;
    const size_t kb = (size_t)agg_key_bytes(q);
    std::vector<uint32_t> hf(n);
    std::vector<unsigned long long> hk(q->agg_wide_key ? 0 : n);
    std::vector<uint8_t> wk;
    if (n) {
        HIPCHK(hipMemcpyAsync(hf.data(), q->d_ofirst, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        if (!q->agg_wide_key) HIPCHK(hipMemcpyAsync(hk.data(), q->d_okeys, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    if (q->agg_wide_key) {
        const int grc = gather_group_keys(q, n, wk);
        if (grc) return grc;
    }
    std::vector<uint32_t> order(n);
    for (uint32_t i = 0; i < n; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return hf[x] < hf[y]; }); // imm3_query_fetch_groups' order
    for (uint32_t o = 0; o < n && o < max_groups; ++o) {
        const uint32_t i = order[o];
        uint8_t *dst = out + (size_t)o * kb;
        if (q->agg_wide_key) std::memcpy(dst, wk.data() + (size_t)i * kb, kb);
        else // (<= 8 bytes: the u64 key, little-endian)
            for (size_t b = 0; b < kb; ++b) dst[b] = (uint8_t)(hk[i] >> (8 * b));
    }
    return IMM3_OK;
}

extern "C" int imm3_query_agg_form(const imm3_query *q, int32_t *form) {
    if (!q || !form) return fail(IMM3_ERR_ARG, "null argument");
    if (!q->is_agg) return fail(IMM3_ERR_ARG, "not an aggregation query");
    *form = q->agg_form_ran;
    return IMM3_OK;
}

// ---------------------------------------------------------------------------------------------
// write side of the PFOR_INT codec (host only; host/codec.hpp)
// ---------------------------------------------------------------------------------------------
extern "C" int imm3_query_expr_form(const imm3_query *q, int32_t *form) {
    if (!q || !form) return fail(IMM3_ERR_ARG, "null argument");
    *form = q->expr_form_ran;
    return IMM3_OK;
}

extern "C" uint64_t imm3_pfor_encode_bound(int32_t n_values) {
    return n_values < 0 ? 0 : (uint64_t)immutabledb::codec::pforEncodeBound(n_values);
}

extern "C" int imm3_pfor_encode_block(const int32_t *values, int32_t n_values, void *out, uint64_t cap, uint64_t *bytes_out) {
    if (n_values < 0 || (n_values > 0 && !values) || !out || !bytes_out) return fail(IMM3_ERR_ARG, "bad argument");
    const std::vector<uint8_t> blk = immutabledb::codec::pforEncodeBlock(values, n_values);
    if (blk.size() > cap) return fail(IMM3_ERR_ARG, "output buffer too small (see imm3_pfor_encode_bound)");
    std::memcpy(out, blk.data(), blk.size());
    *bytes_out = blk.size();
    return IMM3_OK;
}

extern "C" int imm3_pfor_encode_column(const int32_t *values, uint64_t n_values, int32_t block_rows, void *out, uint64_t cap,
                                       int32_t *offsets_out, uint64_t *bytes_out) {
    if ((n_values > 0 && !values) || block_rows <= 0 || !out || !offsets_out || !bytes_out) return fail(IMM3_ERR_ARG, "bad argument");
    uint64_t pos = 0;
    size_t k = 0;
    offsets_out[0] = 0;
    for (uint64_t r = 0; r < n_values; r += (uint64_t)block_rows) {
        const int32_t n = (int32_t)std::min<uint64_t>((uint64_t)block_rows, n_values - r);
        const std::vector<uint8_t> blk = immutabledb::codec::pforEncodeBlock(values + r, n);
        if (pos + blk.size() > cap) return fail(IMM3_ERR_ARG, "output buffer too small");
        if (pos + blk.size() > 0x7FFFFFFFULL) return fail(IMM3_ERR_LAYOUT, "segment data above 2 GiB (blockOffset is an Int, Segment.scala:33)");
        std::memcpy((uint8_t *)out + pos, blk.data(), blk.size());
        pos += blk.size();
        offsets_out[++k] = (int32_t)pos;
    }
    *bytes_out = pos;
    return IMM3_OK;
}

// ---------------------------------------------------------------------------------------------
// write side of the snappy block format (host only; host/codec.hpp)
// ---------------------------------------------------------------------------------------------
extern "C" uint64_t imm3_snappy_encode_bound(uint64_t n_bytes) { return (uint64_t)immutabledb::codec::snappyEncodeBound((size_t)n_bytes); }

extern "C" int imm3_snappy_encode_block(const void *bytes, uint64_t n_bytes, void *out, uint64_t cap, uint64_t *bytes_out) {
    if ((n_bytes > 0 && !bytes) || !out || !bytes_out) return fail(IMM3_ERR_ARG, "bad argument");
    const std::vector<uint8_t> blk = immutabledb::codec::snappyEncodeBlock((const uint8_t *)bytes, (size_t)n_bytes);
    if (blk.size() > cap) return fail(IMM3_ERR_ARG, "output buffer too small (see imm3_snappy_encode_bound)");
    std::memcpy(out, blk.data(), blk.size());
    *bytes_out = blk.size();
    return IMM3_OK;
}
