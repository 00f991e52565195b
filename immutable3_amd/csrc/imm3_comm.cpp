// imm3_comm.cpp -- the one collective of the path, behind the C ABI: the selected-row counts of the per-segment
// pipelines (one PipelineThread per segment, engine/src/main/scala/immutabledb/engine/Engine.scala:176-180, whose
// results meet on the consumer thread, :190-196) summed over the GPUs with ONE 8-byte ncclAllReduce(sum, ncclUint64)
// over RCCL / xGMI.  Nothing else is exchanged on the scan path: segments are sharded s mod G and
// bitmaps, row lists and oids stay on the GPU that produced them.  This file holds the communicator, its streams and fences,
// the count all-reduce and the tools' stand-in kernel; the cross-rank merges of group tables and ordered rows are in
// imm3_merge_groups.cpp, imm3_merge_wide.cpp and imm3_merge_ordered.cpp, over the protocol of imm3_merge_protocol.cpp.
//
// RCCL is bound at run time (dlopen of librccl.so.1): a host that never creates a communicator -- one GPU -- does not
// need the library, and a host that already carries it (PyTorch-ROCm ships its own copy under the same soname) gets
// that copy instead of a second one.
#include "imm3_comm_internal.h"

#include <dlfcn.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>

using namespace imm3;

namespace imm3 {
Rccl g_rccl;
}

namespace {

std::once_flag g_rccl_once;

void rccl_bind() {
    // IMM3_RCCL_LIB: another library that exports the nine nccl* entry points bound below, tried first.  The test suite's
    // loopback transport (tests/native/loopback_rccl.cpp: two ranks of ONE process on ONE device, which RCCL itself refuses)
    // comes in this way, so that the world > 1 paths of this file run where no second GPU exists.
    const char *override_path = getenv("IMM3_RCCL_LIB");
    const char *names[] = {override_path && *override_path ? override_path : "librccl.so.1", "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char *n : names) {
        g_rccl.so = dlopen(n, RTLD_NOW | RTLD_LOCAL);
        if (g_rccl.so) break;
        if (override_path && *override_path && n == names[0]) { // (an override that does not load is an error, not a silent fall-back)
            const char *e = dlerror();
            g_rccl.error = std::string("cannot load IMM3_RCCL_LIB=") + override_path + ": " + (e ? e : "?");
            return;
        }
    }
    if (!g_rccl.so) {
        const char *e = dlerror();
        g_rccl.error = std::string("cannot load librccl.so.1: ") + (e ? e : "?");
        return;
    }
    auto sym = [&](const char *name) -> void * {
        void *p = dlsym(g_rccl.so, name);
        if (!p && g_rccl.error.empty()) g_rccl.error = std::string("librccl has no symbol ") + name;
        return p;
    };
    g_rccl.GetUniqueId = (decltype(g_rccl.GetUniqueId))sym("ncclGetUniqueId");
    g_rccl.CommInitRank = (decltype(g_rccl.CommInitRank))sym("ncclCommInitRank");
    g_rccl.CommInitAll = (decltype(g_rccl.CommInitAll))sym("ncclCommInitAll");
    g_rccl.CommDestroy = (decltype(g_rccl.CommDestroy))sym("ncclCommDestroy");
    g_rccl.AllReduce = (decltype(g_rccl.AllReduce))sym("ncclAllReduce");
    g_rccl.AllGather = (decltype(g_rccl.AllGather))sym("ncclAllGather");
    g_rccl.GroupStart = (decltype(g_rccl.GroupStart))sym("ncclGroupStart");
    g_rccl.GroupEnd = (decltype(g_rccl.GroupEnd))sym("ncclGroupEnd");
    g_rccl.GetErrorString = (decltype(g_rccl.GetErrorString))sym("ncclGetErrorString");
}

} // namespace

int imm3::rccl_ready() {
    std::call_once(g_rccl_once, rccl_bind);
    if (!g_rccl.error.empty()) return fail(IMM3_ERR_DEVICE, g_rccl.error);
    return IMM3_OK;
}

// A communicator whose collectives put KERNELS on the device -- more than one rank (a one-rank all-reduce launches none), or the
// tools' stand-in -- makes the one-launch plans of its context leave a CU per XCD free (imm3_planner.cpp: single_pass_run_grid).
static void comm_reserve(imm3_comm *c, bool on) {
    if (on == c->reserves) return;
    c->reserves = on;
    if (on) c->ctx->comms_attached.fetch_add(1, std::memory_order_relaxed);
    else c->ctx->comms_attached.fetch_sub(1, std::memory_order_relaxed);
}

#ifdef IMM3_ABLATE
// A stand-in for the kernel RCCL launches for the count all-reduce when there are other ranks: same footprint -- 512 threads,
// 37 664 bytes of LDS, 256 vector registers per lane, as ncclDevKernel_Generic_* is built for gfx950 in ROCm 7.2 (read from
// librccl.so's code object) -- so it takes a CU the way that kernel does: it cannot share one with a work-group of the one-launch
// projection (LDS and registers), which is what decides whether the next pass waits for the collective or the collective for
// the pass.  Spins on the device clock.  One GPU is enough to measure that (tools/overlap_probe.py).
__global__ __launch_bounds__(512) void k_comm_standin(uint32_t ticks, unsigned long long *sink) {
    __shared__ unsigned char s_fill[37664];
    asm volatile("; footprint" ::: "v255");   // (256 vector registers per lane, like the kernel it stands for)
    if (threadIdx.x < 64) s_fill[threadIdx.x] = (unsigned char)threadIdx.x;
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < (unsigned long long)ticks) __builtin_amdgcn_s_sleep(8);
    if (s_fill[threadIdx.x & 63] == 255 && sink) *sink = t0;
}
#endif

// the collective on `buf` may start once the context's stream has reached this point
static int fence_in(imm3_comm *c) {
    HIPCHK(hipEventRecord(c->ev_ready, c->ctx->stream));
    HIPCHK(hipStreamWaitEvent(c->stream, c->ev_ready, 0));
    return IMM3_OK;
}
static int fence_out(imm3_comm *c) {
    HIPCHK(hipEventRecord(c->ev_done, c->stream));
    c->in_flight = true;
    return IMM3_OK;
}

static int comm_finish(imm3_ctx *ctx, ncclComm_t nc, int32_t world, int32_t rank, imm3_comm **out) {
    std::unique_ptr<imm3_comm> c(new imm3_comm());
    c->nccl = nc;
    c->world = world;
    c->rank = rank;
    void *p = nullptr;
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipMalloc(&p, 64);
    if (e == hipSuccess) e = hipMemset(p, 0, 64);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_ready, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_done, hipEventDisableTiming);
    if (e != hipSuccess) {
        (void)g_rccl.CommDestroy(nc);
        (void)hipFree(p);
        if (c->stream) (void)hipStreamDestroy(c->stream);
        if (c->ev_ready) (void)hipEventDestroy(c->ev_ready);
        if (c->ev_done) (void)hipEventDestroy(c->ev_done);
        return fail(IMM3_ERR_DEVICE, std::string("communicator scratch: ") + hipGetErrorString(e));
    }
    c->d_slot = (unsigned long long *)p;
    c->ctx = ctx;
    ctx_retain(ctx);
    comm_reserve(c.get(), world > 1);
    *out = c.release();
    return IMM3_OK;
}

extern "C" int imm3_comm_debug_standin(imm3_comm *c, int32_t work_groups, uint32_t spin_us) {
    if (!c) return fail(IMM3_ERR_ARG, "comm is null");
#ifndef IMM3_ABLATE
    if (work_groups > 0) return fail(IMM3_ERR_STATE, "the collective's stand-in kernel exists only in the tools' build of the library (make -C csrc ablate)");
#endif
    if (work_groups < 0 || work_groups > 64) return fail(IMM3_ERR_ARG, "0..64 work-groups");
    c->standin_wgs = work_groups;
    c->standin_ticks = spin_us * 100u;
    comm_reserve(c, c->world > 1 || work_groups > 0);
    return IMM3_OK;
}

extern "C" int imm3_comm_unique_id(uint8_t *id_out) {
    if (!id_out) return fail(IMM3_ERR_ARG, "id_out is null");
    const int rc = rccl_ready();
    if (rc) return rc;
    static_assert(sizeof(ncclUniqueId) == IMM3_COMM_ID_BYTES, "IMM3_COMM_ID_BYTES must be RCCL's unique-id size");
    ncclUniqueId id;
    NCCLCHK(g_rccl.GetUniqueId(&id));
    std::memcpy(id_out, &id, sizeof(id));
    return IMM3_OK;
}

extern "C" int imm3_comm_create(imm3_ctx *ctx, int32_t world, int32_t rank, const uint8_t *id, imm3_comm **out) {
    if (!out) return fail(IMM3_ERR_ARG, "out is null");
    *out = nullptr;
    if (!ctx) return fail(IMM3_ERR_ARG, "ctx is null");
    if (ctx->closed) return fail(IMM3_ERR_STATE, "the context has been destroyed");
    if (world < 1 || rank < 0 || rank >= world || !id) return fail(IMM3_ERR_ARG, "bad world / rank / id");
    const int rc = rccl_ready();
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    ncclUniqueId uid;
    std::memcpy(&uid, id, sizeof(uid));
    ncclComm_t nc = nullptr;
    NCCLCHK(g_rccl.CommInitRank(&nc, world, uid, rank));
    return comm_finish(ctx, nc, world, rank, out);
}

extern "C" int imm3_comm_create_all(imm3_ctx *const *ctxs, int32_t n, imm3_comm **out) {
    if (!out) return fail(IMM3_ERR_ARG, "out is null");
    for (int32_t i = 0; i < n; ++i) out[i] = nullptr;
    if (n < 1 || !ctxs) return fail(IMM3_ERR_ARG, "a communicator needs at least one context");
    std::vector<int> devs((size_t)n);
    for (int32_t i = 0; i < n; ++i) {
        if (!ctxs[i]) return fail(IMM3_ERR_ARG, "ctx is null");
        if (ctxs[i]->closed) return fail(IMM3_ERR_STATE, "a context has been destroyed");
        devs[(size_t)i] = ctxs[i]->device;
        for (int32_t j = 0; j < i; ++j)
            if (devs[(size_t)j] == devs[(size_t)i]) return fail(IMM3_ERR_ARG, "one context per device: two contexts share device " + std::to_string(devs[(size_t)i]));
    }
    const int rc = rccl_ready();
    if (rc) return rc;
    std::vector<ncclComm_t> ncs((size_t)n, nullptr);
    NCCLCHK(g_rccl.CommInitAll(ncs.data(), n, devs.data()));
    for (int32_t i = 0; i < n; ++i) {
        const int frc = comm_finish(ctxs[i], ncs[(size_t)i], n, i, &out[i]);
        if (frc) { // all or nothing: the communicators made so far go too (the caller only sees nulls)
            const std::string why = imm3_last_error();
            for (int32_t j = i + 1; j < n; ++j) (void)g_rccl.CommDestroy(ncs[(size_t)j]);
            for (int32_t j = 0; j < i; ++j) {
                (void)imm3_comm_destroy(out[j]);
                out[j] = nullptr;
            }
            return fail(frc, why);
        }
    }
    return IMM3_OK;
}

extern "C" int imm3_comm_destroy(imm3_comm *c) {
    if (!c) return IMM3_OK;
    (void)hipSetDevice(c->ctx->device);
    {
        imm3::GateScope gate(&c->ctx->gate);
        if (!c->ctx->closed) (void)hipStreamSynchronize(c->ctx->stream);
    }
    (void)hipStreamSynchronize(c->stream);
    if (c->nccl) (void)g_rccl.CommDestroy(c->nccl);
    (void)hipStreamDestroy(c->stream);
    (void)hipEventDestroy(c->ev_ready);
    (void)hipEventDestroy(c->ev_done);
    (void)hipFree(c->d_slot);
    comm_reserve(c, false);
    ctx_release(c->ctx);
    delete c;
    return IMM3_OK;
}

extern "C" int imm3_comm_info(const imm3_comm *c, int32_t *world, int32_t *rank) {
    if (!c) return fail(IMM3_ERR_ARG, "comm is null");
    if (world) *world = c->world;
    if (rank) *rank = c->rank;
    return IMM3_OK;
}

extern "C" int imm3_comm_allreduce_u64(imm3_comm *c, uint64_t *device_buf, uint64_t n) {
    if (!c || !device_buf || n == 0) return fail(IMM3_ERR_ARG, "bad argument");
    imm3::GateScope gate(&c->ctx->gate);
    if (c->ctx->closed) return fail(IMM3_ERR_STATE, "the context of this communicator has been destroyed");
    HIPCHK(hipSetDevice(c->ctx->device));
    int rc = fence_in(c);
    if (rc) return rc;
    NCCLCHK(g_rccl.AllReduce(device_buf, device_buf, (size_t)n, ncclUint64, ncclSum, c->nccl, c->stream));
    return fence_out(c);
}

extern "C" int imm3_comm_sync(imm3_comm *c) {
    if (!c) return fail(IMM3_ERR_ARG, "comm is null");
    HIPCHK(hipSetDevice(c->ctx->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->in_flight = false;
    return IMM3_OK;
}

extern "C" int imm3_comm_join(imm3_comm *c) {
    if (!c) return fail(IMM3_ERR_ARG, "comm is null");
    imm3::GateScope gate(&c->ctx->gate);
    if (c->ctx->closed) return fail(IMM3_ERR_STATE, "the context of this communicator has been destroyed");
    HIPCHK(hipSetDevice(c->ctx->device));
    if (c->in_flight) HIPCHK(hipStreamWaitEvent(c->ctx->stream, c->ev_done, 0));
    return IMM3_OK;
}

// this rank's part: the counts of its queries summed into `dst` on the context's stream, behind the scans that
// produce them (same stream; a count reduced on the aux stream is joined first)
static int local_sum(imm3_comm *c, imm3_query *const *queries, int32_t n_queries, unsigned long long *dst) {
    imm3_ctx *ctx = c->ctx;
    hipStream_t s = ctx->stream;
    // the communicator's own word may still be travelling from the previous call: wait for that collective (stream side)
    if (dst == c->d_slot && c->in_flight) HIPCHK(hipStreamWaitEvent(s, c->ev_done, 0));
    if (n_queries == 0) {
        HIPCHK(hipMemsetAsync(dst, 0, sizeof(unsigned long long), s));
        return IMM3_OK;
    }
    for (int32_t base = 0; base < n_queries; base += kMaxSumCounts) {
        SumCountsArgs a;
        std::memset(&a, 0, sizeof(a));
        a.n = std::min<int32_t>(kMaxSumCounts, n_queries - base);
        for (int32_t i = 0; i < a.n; ++i) {
            imm3_query *q = queries[base + i];
            if (!q) return fail(IMM3_ERR_ARG, "query is null");
            if (q->ctx != ctx) return fail(IMM3_ERR_ARG, "the query runs on another context than the communicator");
            if (!q->run.ran_select) return fail(IMM3_ERR_STATE, "imm3_query_run has not been called");
            const int jrc = join_query_count(q);
            if (jrc) return jrc;
            a.src[i] = q->d_total;
        }
        a.accumulate = base > 0;
        a.dst = dst;
        launch_sum_counts(a, s);
        HIPCHK(hipGetLastError());
    }
    return IMM3_OK;
}

extern "C" int imm3_comm_allreduce_count(imm3_comm *c, imm3_query *const *queries, int32_t n_queries, uint64_t *device_out,
                                         uint64_t *host_out) {
    if (!c || n_queries < 0 || (n_queries > 0 && !queries)) return fail(IMM3_ERR_ARG, "bad argument");
    imm3::GateScope gate(&c->ctx->gate);
    if (c->ctx->closed) return fail(IMM3_ERR_STATE, "the context of this communicator has been destroyed");
    HIPCHK(hipSetDevice(c->ctx->device));
    unsigned long long *dst = device_out ? (unsigned long long *)device_out : c->d_slot;
    int rc = local_sum(c, queries, n_queries, dst);
    if (rc) return rc;
    rc = fence_in(c);
    if (rc) return rc;
#ifdef IMM3_ABLATE
    if (c->standin_wgs > 0) { // (tools: what a real multi-rank all-reduce puts on the device at this point)
        hipLaunchKernelGGL(k_comm_standin, dim3((unsigned)c->standin_wgs), dim3(512), 0, c->stream, c->standin_ticks, (unsigned long long *)nullptr);
        HIPCHK(hipGetLastError());
    }
#endif
    NCCLCHK(g_rccl.AllReduce(dst, dst, 1, ncclUint64, ncclSum, c->nccl, c->stream));
    rc = fence_out(c);
    if (rc) return rc;
    if (host_out) {
        unsigned long long v = 0;
        HIPCHK(hipMemcpyAsync(&v, dst, sizeof(v), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        c->in_flight = false;
        *host_out = v;
    }
    return IMM3_OK;
}

// Single-process shape (one JVM, every GPU): the per-device collectives are issued by ONE thread, so they go into a
// ncclGroupStart / ncclGroupEnd section (RCCL would otherwise wait in the first call for the ranks behind it).
extern "C" int imm3_comm_allreduce_count_all(imm3_comm *const *comms, int32_t n_comms, imm3_query *const *const *queries,
                                             const int32_t *n_queries, uint64_t *host_out) {
    if (!comms || n_comms < 1 || !n_queries || !queries) return fail(IMM3_ERR_ARG, "bad argument");
    for (int32_t i = 0; i < n_comms; ++i)
        if (!comms[i] || n_queries[i] < 0 || (n_queries[i] > 0 && !queries[i])) return fail(IMM3_ERR_ARG, "bad argument");
    std::vector<std::unique_ptr<imm3::GateScope>> gates; // one context per device, each with its own capture gate
    for (int32_t i = 0; i < n_comms; ++i) gates.emplace_back(new imm3::GateScope(&comms[i]->ctx->gate));
    for (int32_t i = 0; i < n_comms; ++i) {
        if (comms[i]->ctx->closed) return fail(IMM3_ERR_STATE, "the context of a communicator has been destroyed");
        HIPCHK(hipSetDevice(comms[i]->ctx->device));
        int rc = local_sum(comms[i], queries[i], n_queries[i], comms[i]->d_slot);
        if (!rc) rc = fence_in(comms[i]);
        if (rc) return rc;
    }
    NCCLCHK(g_rccl.GroupStart());
    for (int32_t i = 0; i < n_comms; ++i) {
        imm3_comm *c = comms[i];
        const ncclResult_t r = g_rccl.AllReduce(c->d_slot, c->d_slot, 1, ncclUint64, ncclSum, c->nccl, c->stream);
        if (r != ncclSuccess) {
            (void)g_rccl.GroupEnd();
            return fail(IMM3_ERR_DEVICE, std::string("ncclAllReduce: ") + g_rccl.GetErrorString(r));
        }
    }
    NCCLCHK(g_rccl.GroupEnd());
    for (int32_t i = 0; i < n_comms; ++i) {
        HIPCHK(hipSetDevice(comms[i]->ctx->device));
        const int rc = fence_out(comms[i]);
        if (rc) return rc;
    }
    if (host_out) {
        imm3_comm *c = comms[0];
        unsigned long long v = 0;
        HIPCHK(hipSetDevice(c->ctx->device));
        HIPCHK(hipMemcpyAsync(&v, c->d_slot, sizeof(v), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        c->in_flight = false;
        *host_out = v;
    }
    return IMM3_OK;
}
