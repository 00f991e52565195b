// imm3_comm.cpp -- the one collective of the path, behind the C ABI: the selected-row counts of the per-segment
// pipelines (one PipelineThread per segment, engine/src/main/scala/immutabledb/engine/Engine.scala:176-180, whose
// results meet on the consumer thread, :190-196) summed over the GPUs with ONE 8-byte ncclAllReduce(sum, ncclUint64)
// over RCCL / xGMI.  Nothing else is exchanged: segments are sharded s mod G and bitmaps, row
// lists and oids stay on the GPU that produced them.
//
// RCCL is bound at run time (dlopen of librccl.so.1): a host that never creates a communicator -- one GPU -- does not
// need the library, and a host that already carries it (PyTorch-ROCm ships its own copy under the same soname) gets
// that copy instead of a second one.
#include "imm3_handles.h"
#include "imm3_merge_order.h"

#include <dlfcn.h>
#include <rccl/rccl.h> // types and enums only; every call goes through the table below

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>

using namespace imm3;

namespace {

struct Rccl {
    void *so = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    std::string error; // why the library could not be bound
};

Rccl g_rccl;
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

int rccl_ready() {
    std::call_once(g_rccl_once, rccl_bind);
    if (!g_rccl.error.empty()) return fail(IMM3_ERR_DEVICE, g_rccl.error);
    return IMM3_OK;
}

#define NCCLCHK(expr)                                                                                              \
    do {                                                                                                           \
        ncclResult_t _r = (expr);                                                                                  \
        if (_r != ncclSuccess) return fail(IMM3_ERR_DEVICE, std::string(#expr) + ": " + g_rccl.GetErrorString(_r)); \
    } while (0)

} // namespace

// Streams.  The collective runs on the communicator's OWN stream, fenced by events: it starts after everything already
// enqueued on the context's stream (the scans that produce the counts, the kernel that sums them) and the context's
// stream never waits for it -- the next pass's scans start right behind the sum while the 8 bytes cross xGMI (a
// latency-bound message: tens of microseconds that would otherwise sit between two 60-200 us scans).  imm3_comm_sync
// (host) / imm3_comm_join (stream side) are the ways back.
struct imm3_comm {
    imm3_ctx *ctx = nullptr;      // the GPU this rank drives
    ncclComm_t nccl = nullptr;
    int32_t world = 1, rank = 0;
    hipStream_t stream = nullptr; // where the collectives run
    hipEvent_t ev_ready = nullptr, ev_done = nullptr;
    bool in_flight = false;       // a collective has been enqueued since the last join / sync
    unsigned long long *d_slot = nullptr; // send/receive word of imm3_comm_allreduce_count when the caller passes no buffer
    // tools' build (imm3_comm_debug_standin): a kernel with the footprint of RCCL's, in front of every count all-reduce
    int32_t standin_wgs = 0;
    uint32_t standin_ticks = 0;   // how long each of its work-groups spins, in ticks of the 100 MHz device clock
    bool reserves = false;        // counted in ctx->comms_attached: its collectives launch kernels (more than one rank, or the stand-in)
};

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

// ---------------------------------------------------------------------------------------------
// Cross-segment / cross-GPU merge of group tables: ProjectAggregateQueueOp
// (engine/src/main/scala/immutabledb/engine/operator/ProjectAggregateQueue.scala:9-55) merges the per-segment maps by key --
// counts add, max / min combine, the first arrival keeps its place (here: ascending segment index, then first row).  Every
// rank brings the group tables of its own segments' aggregation queries; every rank gets the merged table.
//   keys of <= 2 bytes : the groups are scattered into a direct-indexed device table (k_merge_scatter) and the ranks' tables
//                        meet in element-wise all-reduces: sum on the counts, min on `segment << 32 | first row`, max / min
//                        on each aggregate -- no host work but the final compaction of the occupied slots;
//   wider keys         : the ranks' (locally merged) group lists are exchanged with ncclAllGather -- fixed-size slots,
//                        sized by an all-reduce(max) of the list lengths -- and merged by key.
// ---------------------------------------------------------------------------------------------
namespace {

struct MergedGroup {
    unsigned long long key, first, count;
    long long vals[kMaxAggs];
};

int same_spec(imm3_query *const *queries, int32_t n, const char **why) {
    for (int32_t i = 0; i < n; ++i) {
        imm3_query *q = queries[i];
        if (!q) { *why = "query is null"; return IMM3_ERR_ARG; }
        if (!q->is_agg) { *why = "not an aggregation query"; return IMM3_ERR_ARG; }
        if (!q->run.ran_agg) { *why = "imm3_query_run has not been called"; return IMM3_ERR_STATE; }
        imm3_query *q0 = queries[0];
        if (q->aggs.size() != q0->aggs.size() || q->group_cols.size() != q0->group_cols.size()) { *why = "the queries aggregate differently"; return IMM3_ERR_ARG; }
        for (size_t j = 0; j < q->aggs.size(); ++j)
            if (q->aggs[j].kind != q0->aggs[j].kind) { *why = "the queries aggregate differently"; return IMM3_ERR_ARG; }
    }
    return IMM3_OK;
}

void combine(MergedGroup &into, const MergedGroup &g, const int32_t *kinds, const int32_t *is_str, int n_agg) {
    into.count += g.count;
    into.first = std::min(into.first, g.first);
    for (int j = 0; j < n_agg; ++j) {
        if (kinds[j] == AGG_MAX) {
            if (is_str[j]) into.vals[j] = (long long)std::max((unsigned long long)into.vals[j], (unsigned long long)g.vals[j]);
            else into.vals[j] = std::max(into.vals[j], g.vals[j]);
        } else if (kinds[j] == AGG_MIN) into.vals[j] = std::min(into.vals[j], g.vals[j]);
        else if (kinds[j] == AGG_SUM) into.vals[j] += g.vals[j];
    }
}

} // namespace

extern "C" int imm3_comm_merge_groups(imm3_comm *c, imm3_query *const *queries, const int32_t *segment_index, int32_t n_queries,
                                      uint64_t *keys, uint64_t *first, uint64_t *counts, int64_t *vals, uint32_t max_groups, uint32_t *n_groups) {
    if (!c || !n_groups || n_queries < 0 || (n_queries > 0 && (!queries || !segment_index))) return fail(IMM3_ERR_ARG, "bad argument");
    imm3_ctx *ctx = c->ctx;
    imm3::GateScope gate(&ctx->gate);
    if (ctx->closed) return fail(IMM3_ERR_STATE, "the context of this communicator has been destroyed");
    if (ctx->capture) return fail(IMM3_ERR_STATE, "a graph capture is open on this context");
    HIPCHK(hipSetDevice(ctx->device));
    // Every rank must take the same road AND the same exit: a rank that returned early while the others went on to the next
    // collective would leave them waiting in hipStreamSynchronize for good.  So everything that can fail on this rank alone --
    // argument checks, the queries' group lists (device work), the table's allocation -- happens BEFORE the first collective,
    // and what it found travels with the shape exchange: {key width, aggregates, their complements (max of the complement = min),
    // error flag}, one all-reduce(max) -- every rank sees whether all ranks agree and whether any of them has failed.
    int local_rc = IMM3_OK;
    std::string local_why;
    auto local_fail = [&](int code, const std::string &msg) {
        if (local_rc == IMM3_OK) { local_rc = code; local_why = msg; }
    };
    {
        const char *why = "";
        const int src = same_spec(queries, n_queries, &why);
        if (src) local_fail(src, why);
        else if (n_queries == 0) local_fail(IMM3_ERR_ARG, "a rank joins the merge with at least one aggregation query (the aggregates' kinds come from it)");
    }
    int key_bytes = 0, n_agg = 0;
    int32_t kinds[kMaxAggs] = {0, 0, 0, 0}, is_str[kMaxAggs] = {0, 0, 0, 0};
    std::vector<uint32_t> n_local((size_t)std::max(n_queries, 0), 0u); // groups of each query (its dense list is complete in q->d_o*)
    if (local_rc == IMM3_OK) {
        imm3_query *q0 = queries[0];
        for (int32_t g : q0->group_cols) key_bytes += q0->seg->cols[(size_t)q0->used[(size_t)g]].width;
        n_agg = (int)q0->aggs.size();
        for (int j = 0; j < n_agg; ++j) {
            kinds[j] = q0->aggs[j].kind;
            is_str[j] = q0->seg->cols[(size_t)q0->used[(size_t)q0->aggs[j].column]].vcodec == IMM3_DENSE_STRING;
        }
        for (int32_t i = 0; i < n_queries && local_rc == IMM3_OK; ++i) // (... and u64 keys: never a wide key's prefix)
            if (queries[i]->agg_wide_key) local_fail(IMM3_ERR_ARG, "a group key wider than 8 bytes cannot be merged (imm3_query_fetch_group_keys gives each query's keys)");
        for (int32_t i = 0; i < n_queries && local_rc == IMM3_OK; ++i) // (the tables below hold 8 bytes per value: never a wide value's prefix)
            for (int32_t j = 0; j < (int32_t)queries[i]->aggs.size(); ++j)
                if (queries[i]->d_chunks[j]) {
                    local_fail(IMM3_ERR_ARG, "a MAX over a STRING column wider than 8 bytes cannot be merged (imm3_query_fetch_group_strings gives each query's values)");
                    break;
                }
        for (int32_t i = 0; i < n_queries && local_rc == IMM3_OK; ++i) {
            if (queries[i]->ctx != ctx) { local_fail(IMM3_ERR_ARG, "the query runs on another context than the communicator"); break; }
            const int grc = query_groups(queries[i], &n_local[(size_t)i]);
            if (grc) local_fail(grc, imm3_last_error());
        }
    }
    // (wide keys: this rank's entries must leave room for a table of twice their number + 1 slots in the kernels' 32-bit slot
    // fields -- 2^30 entries: checked HERE, before the first collective, like everything else that can fail on one rank alone)
    constexpr unsigned long long kMaxMergeEntries = 1ULL << 30;
    unsigned long long total_local = 0;
    for (int32_t i = 0; i < n_queries; ++i) total_local += n_local[(size_t)i];
    if (local_rc == IMM3_OK && key_bytes > 2 && total_local > kMaxMergeEntries) local_fail(IMM3_ERR_ARG, "too many groups to merge");
    hipStream_t s = ctx->stream;
    // the direct table of narrow keys (allocated before the exchange: a failure here is this rank's to report)
    void *table = nullptr;
    std::unique_ptr<void, void (*)(void *)> table_guard(nullptr, [](void *q) { (void)hipFree(q); });
    const uint32_t K = key_bytes == 0 ? 1u : (key_bytes == 1 ? 256u : 65536u);
    const size_t table_words = (size_t)K * (2 + kMaxAggs);
    if (local_rc == IMM3_OK && key_bytes <= 2) {
        const hipError_t e = hipMalloc(&table, table_words * sizeof(unsigned long long));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            local_fail(IMM3_ERR_DEVICE, std::string("hipMalloc of the merge table: ") + hipGetErrorString(e));
        } else table_guard.reset(table);
    }
    if (c->world > 1) {
        const int rrc = rccl_ready();
        if (rrc) return rrc; // (no RCCL in this process: no rank of this process can be inside the collective either)
        // The communicator's word and the communicator itself may still be in use by an imm3_comm_allreduce_count on the
        // communicator's own stream: the merge's collectives run on the context's stream, behind that one.
        if (c->in_flight) HIPCHK(hipStreamWaitEvent(s, c->ev_done, 0));
        unsigned long long shape[5] = {(unsigned long long)key_bytes, (unsigned long long)n_agg, ~(unsigned long long)key_bytes, ~(unsigned long long)n_agg,
                                       local_rc == IMM3_OK ? 0ULL : 1ULL};
        if (local_rc != IMM3_OK) { shape[0] = shape[1] = 0ULL; shape[2] = shape[3] = 0ULL; } // (a failed rank does not vote on the shape)
        HIPCHK(hipMemcpyAsync(c->d_slot, shape, sizeof(shape), hipMemcpyHostToDevice, s));
        NCCLCHK(g_rccl.AllReduce(c->d_slot, c->d_slot, 5, ncclUint64, ncclMax, c->nccl, s));
        HIPCHK(hipMemcpyAsync(shape, c->d_slot, sizeof(shape), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (local_rc != IMM3_OK) return fail(local_rc, local_why);
        if (shape[4]) return fail(IMM3_ERR_STATE, "another rank failed before the merge (its call says why); no rank has merged anything");
        if (shape[0] != ~shape[2] || shape[1] != ~shape[3] || shape[0] != (unsigned long long)key_bytes || shape[1] != (unsigned long long)n_agg)
            return fail(IMM3_ERR_ARG, "the ranks' aggregation queries differ in key width or number of aggregates"); // (max != min: every rank sees it and leaves here)
    } else if (local_rc != IMM3_OK) return fail(local_rc, local_why);
    std::vector<MergedGroup> merged;
    if (key_bytes <= 2) {
        // ---- direct table + element-wise all-reduces ----
        void *p = table;
        const size_t words = table_words;
        MergeArgs a;
        std::memset(&a, 0, sizeof(a));
        a.slots = K;
        a.t_counts = (unsigned long long *)p;
        a.t_first = a.t_counts + K;
        a.t_vals = (long long *)(a.t_first + K);
        a.n_agg = n_agg;
        for (int j = 0; j < kMaxAggs; ++j) { a.kinds[j] = kinds[j]; a.is_str[j] = is_str[j]; }
        launch_merge_init(a, s);
        HIPCHK(hipGetLastError());
        for (int32_t i = 0; i < n_queries; ++i) {
            imm3_query *q = queries[i];
            const uint32_t ng = n_local[(size_t)i];
            a.keys = q->d_okeys;
            a.first = q->d_ofirst;
            a.counts = q->d_ocounts;
            a.vals = q->d_ovals;
            a.n_groups = ng;
            a.seg_hi = (unsigned long long)(uint32_t)segment_index[i] << 32;
            if (ng) launch_merge_scatter(a, s);
            HIPCHK(hipGetLastError());
        }
        if (c->world > 1) {
            NCCLCHK(g_rccl.AllReduce(a.t_counts, a.t_counts, K, ncclUint64, ncclSum, c->nccl, s));
            NCCLCHK(g_rccl.AllReduce(a.t_first, a.t_first, K, ncclUint64, ncclMin, c->nccl, s));
            for (int j = 0; j < n_agg; ++j) {
                long long *t = a.t_vals + (size_t)j * K;
                if (kinds[j] == AGG_MAX) NCCLCHK(g_rccl.AllReduce(t, t, K, is_str[j] ? ncclUint64 : ncclInt64, ncclMax, c->nccl, s));
                else if (kinds[j] == AGG_MIN) NCCLCHK(g_rccl.AllReduce(t, t, K, ncclInt64, ncclMin, c->nccl, s));
                else if (kinds[j] == AGG_SUM) NCCLCHK(g_rccl.AllReduce(t, t, K, ncclInt64, ncclSum, c->nccl, s));
            }
        }
        std::vector<unsigned long long> h(words);
        HIPCHK(hipMemcpyAsync(h.data(), p, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (uint32_t k = 0; k < K; ++k) {
            if (!h[k]) continue;
            MergedGroup g;
            g.key = k;
            g.count = h[k];
            g.first = h[(size_t)K + k];
            for (int j = 0; j < kMaxAggs; ++j) g.vals[j] = (long long)h[(size_t)K * (2 + j) + k];
            merged.push_back(g);
        }
    } else {
        // ---- wide keys: merged by key ON THE DEVICE (round 4; rounds 2-3 merged std::maps on the host, fine for thousands of
        // groups, not for 10^5 and more): this rank's queries' lists go into a hash table (compare-and-swap on the key, atomic
        // add / min / max on the columns), its occupied slots come out as a packed list, the ranks' lists are exchanged with
        // ncclAllGather -- fixed-size slots, sized by an all-reduce(max) of the list lengths -- and merged the same way.  The
        // host only sorts the result by first arrival.
        auto pow2_at_least = [](unsigned long long v) { unsigned long long p = 1024; while (p < v) p <<= 1; return p; };
        // one table: {keys, counts, first, vals[kMaxAggs]} x slots, then the packed list and its counter
        auto table_bytes = [](unsigned long long slots, unsigned long long list_cap) {
            return (size_t)((slots * (3 + kMaxAggs) + list_cap * kMergeListWords + 8) * sizeof(unsigned long long));
        };
        auto bind = [&](MergeArgs &a, void *p, unsigned long long cap, unsigned long long list_cap) {
            std::memset(&a, 0, sizeof(a));
            a.mask = (uint32_t)(cap - 1);
            a.slots = (uint32_t)(cap + 1); // (+ the slot of the one key that equals the empty marker)
            unsigned long long *w = (unsigned long long *)p;
            a.t_keys = w;
            a.t_counts = a.t_keys + a.slots;
            a.t_first = a.t_counts + a.slots;
            a.t_vals = (long long *)(a.t_first + a.slots);
            a.out_list = (unsigned long long *)(a.t_vals + (size_t)kMaxAggs * a.slots);
            a.out_n = a.out_list + list_cap * kMergeListWords;
            a.out_cap = (uint32_t)list_cap;
            a.n_agg = n_agg;
            for (int j = 0; j < kMaxAggs; ++j) { a.kinds[j] = kinds[j]; a.is_str[j] = is_str[j]; }
        };
        if (c->world == 1 && total_local > kMaxMergeEntries) return fail(IMM3_ERR_ARG, "too many groups to merge"); // (world > 1: refused before the shape exchange)
        const unsigned long long cap1 = pow2_at_least(2 * std::max<unsigned long long>(total_local, 1)), list1 = std::max<unsigned long long>(total_local, 1);
        void *p1 = nullptr;
        {   // (a failure here is this rank's alone: with more than one rank it would leave the others in the collective below, so the
            // allocation is small-step: the table of the LOCAL merge was sized from counts every rank already has)
            const hipError_t e = hipMalloc(&p1, table_bytes(cap1 + 1, list1));
            if (e != hipSuccess) { (void)hipGetLastError(); p1 = nullptr; }
        }
        std::unique_ptr<void, void (*)(void *)> g1(p1, [](void *q) { (void)hipFree(q); });
        unsigned long long mine = 0;
        MergeArgs a1;
        std::memset(&a1, 0, sizeof(a1));
        std::string p1_why = "hipMalloc of the merge table failed";
        if (p1) {
            // Device work of THIS rank between two collectives: whatever fails here must not return -- the other ranks are on
            // their way to the list-length all-reduce below and would wait there for good.  A failure clears p1 instead: the
            // rank then says ~0 in that all-reduce and every rank leaves together.
            auto local_step = [&](hipError_t e, const char *what) {
                if (e == hipSuccess || !p1) return;
                (void)hipGetLastError();
                p1_why = std::string(what) + ": " + hipGetErrorString(e);
                p1 = nullptr;
            };
            bind(a1, p1, cap1, list1);
            launch_merge_init(a1, s);
            local_step(hipGetLastError(), "merge table init");
            for (int32_t i = 0; i < n_queries && p1; ++i) {
                imm3_query *q = queries[i];
                const uint32_t ng = n_local[(size_t)i];
                a1.keys = q->d_okeys;
                a1.first = q->d_ofirst;
                a1.counts = q->d_ocounts;
                a1.vals = q->d_ovals;
                a1.n_groups = ng;
                a1.seg_hi = (unsigned long long)(uint32_t)segment_index[i] << 32;
                if (ng) launch_merge_scatter(a1, s);
                local_step(hipGetLastError(), "merge scatter");
            }
            if (p1) {
                launch_merge_collect_list(a1, s);
                local_step(hipGetLastError(), "merge collect");
            }
            if (p1) local_step(hipMemcpyAsync(&mine, a1.out_n, sizeof(mine), hipMemcpyDeviceToHost, s), "merge list length");
            if (p1) local_step(hipStreamSynchronize(s), "merge list length");
        }
        auto take_list = [&](const unsigned long long *d_list, unsigned long long n) -> int {
            std::vector<unsigned long long> h((size_t)n * kMergeListWords);
            if (n) HIPCHK(hipMemcpyAsync(h.data(), d_list, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            merged.reserve((size_t)n);
            for (size_t i = 0; i < (size_t)n; ++i) {
                const unsigned long long *w = h.data() + i * kMergeListWords;
                MergedGroup m;
                m.key = w[0];
                m.first = w[1];
                m.count = w[2];
                for (int j = 0; j < kMaxAggs; ++j) m.vals[j] = (long long)w[3 + j];
                merged.push_back(m);
            }
            return IMM3_OK;
        };
        if (c->world == 1) {
            if (!p1) return fail(IMM3_ERR_DEVICE, p1_why);
            const int trc = take_list(a1.out_list, mine);
            if (trc) return trc;
        } else {
            // list lengths -> the common slot count (a rank whose table could not be allocated says so with ~0: every rank leaves)
            unsigned long long word = p1 ? mine : ~0ULL, most = 0;
            HIPCHK(hipMemcpyAsync(c->d_slot, &word, sizeof(word), hipMemcpyHostToDevice, s));
            NCCLCHK(g_rccl.AllReduce(c->d_slot, c->d_slot, 1, ncclUint64, ncclMax, c->nccl, s));
            HIPCHK(hipMemcpyAsync(&most, c->d_slot, sizeof(most), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            if (most == ~0ULL) return fail(IMM3_ERR_DEVICE, p1 ? std::string("a rank could not build its merge table; no rank has merged anything") : p1_why + "; no rank has merged anything");
            const size_t per_rank = (size_t)most * kMergeListWords;
            if (per_rank) {
                const unsigned long long entries = most * (unsigned long long)c->world;
                if (entries > kMaxMergeEntries) return fail(IMM3_ERR_ARG, "too many groups to merge"); // (the same figure on every rank: every rank leaves here)
                const unsigned long long cap2 = pow2_at_least(2 * entries);
                void *p = nullptr;
                // (sizes are the same on every rank: an allocation failure here is reported through one more flag exchange)
                hipError_t e = hipMalloc(&p, (per_rank + per_rank * (size_t)c->world) * sizeof(unsigned long long) + table_bytes(cap2 + 1, entries));
                if (e != hipSuccess) { (void)hipGetLastError(); p = nullptr; }
                std::unique_ptr<void, void (*)(void *)> guard(p, [](void *q) { (void)hipFree(q); });
                unsigned long long ok = p ? 0ULL : 1ULL, any = 0;
                HIPCHK(hipMemcpyAsync(c->d_slot, &ok, sizeof(ok), hipMemcpyHostToDevice, s));
                NCCLCHK(g_rccl.AllReduce(c->d_slot, c->d_slot, 1, ncclUint64, ncclMax, c->nccl, s));
                HIPCHK(hipMemcpyAsync(&any, c->d_slot, sizeof(any), hipMemcpyDeviceToHost, s));
                HIPCHK(hipStreamSynchronize(s));
                if (any) return fail(IMM3_ERR_DEVICE, "a rank could not allocate the exchange buffers of the merge; no rank has merged anything");
                unsigned long long *d_send = (unsigned long long *)p, *d_recv = d_send + per_rank;
                HIPCHK(hipMemsetAsync(d_send, 0, per_rank * sizeof(unsigned long long), s)); // (padding entries: count 0)
                if (mine) HIPCHK(hipMemcpyAsync(d_send, a1.out_list, (size_t)mine * kMergeListWords * sizeof(unsigned long long), hipMemcpyDeviceToDevice, s));
                NCCLCHK(g_rccl.AllGather(d_send, d_recv, per_rank, ncclUint64, c->nccl, s));
                MergeArgs a2;
                bind(a2, d_recv + per_rank * (size_t)c->world, cap2, entries);
                launch_merge_init(a2, s);
                HIPCHK(hipGetLastError());
                a2.list = d_recv;
                a2.n_groups = (uint32_t)entries;
                launch_merge_insert_list(a2, s);
                HIPCHK(hipGetLastError());
                launch_merge_collect_list(a2, s);
                HIPCHK(hipGetLastError());
                unsigned long long n2 = 0;
                HIPCHK(hipMemcpyAsync(&n2, a2.out_n, sizeof(n2), hipMemcpyDeviceToHost, s));
                HIPCHK(hipStreamSynchronize(s));
                const int trc = take_list(a2.out_list, n2);
                if (trc) return trc;
            }
        }
    }
    std::sort(merged.begin(), merged.end(), [](const MergedGroup &x, const MergedGroup &y) { return x.first < y.first; }); // first arrival first
    *n_groups = (uint32_t)merged.size();
    for (size_t o = 0; o < merged.size() && o < max_groups; ++o) {
        if (keys) keys[o] = merged[o].key;
        if (first) first[o] = merged[o].first;
        if (counts) counts[o] = merged[o].count;
        if (vals)
            for (int j = 0; j < n_agg; ++j) vals[o * (size_t)n_agg + (size_t)j] = kinds[j] == AGG_COUNT ? (int64_t)merged[o].count : (int64_t)merged[o].vals[j];
    }
    return IMM3_OK;
}

// Single-process flavour (one JVM, every GPU: comms from imm3_comm_create_all): the group tables of all devices are in this
// process, so they are merged here -- per device the same scatter / list as above (no collective), then one merge by key on
// the host; the tables are a few KB.  comms[i] brings queries[i][0 .. n_queries[i]) with segment_index[i][...].
extern "C" int imm3_comm_merge_groups_all(imm3_comm *const *comms, int32_t n_comms, imm3_query *const *const *queries,
                                          const int32_t *const *segment_index, const int32_t *n_queries,
                                          uint64_t *keys, uint64_t *first, uint64_t *counts, int64_t *vals, uint32_t max_groups, uint32_t *n_groups) {
    if (!comms || n_comms < 1 || !queries || !segment_index || !n_queries || !n_groups) return fail(IMM3_ERR_ARG, "bad argument");
    int n_agg = -1;
    int32_t kinds[kMaxAggs] = {0, 0, 0, 0}, is_str[kMaxAggs] = {0, 0, 0, 0};
    std::map<unsigned long long, MergedGroup> all;
    for (int32_t i = 0; i < n_comms; ++i) {
        if (!comms[i] || n_queries[i] < 0 || (n_queries[i] > 0 && (!queries[i] || !segment_index[i]))) return fail(IMM3_ERR_ARG, "bad argument");
        if (n_queries[i] == 0) continue;
        imm3_comm one = *comms[i]; // the same communicator seen as a world of one: its device's queries merged without a collective
        one.world = 1;
        uint32_t n = 0;
        int rc = imm3_comm_merge_groups(&one, queries[i], segment_index[i], n_queries[i], nullptr, nullptr, nullptr, nullptr, 0, &n);
        if (rc) return rc;
        imm3_query *q0 = queries[i][0];
        const int na = (int)q0->aggs.size();
        if (n_agg < 0) {
            n_agg = na;
            for (int j = 0; j < na; ++j) {
                kinds[j] = q0->aggs[j].kind;
                is_str[j] = q0->seg->cols[(size_t)q0->used[(size_t)q0->aggs[j].column]].vcodec == IMM3_DENSE_STRING;
            }
        } else if (na != n_agg) return fail(IMM3_ERR_ARG, "the devices' aggregation queries differ");
        std::vector<uint64_t> k(n), f(n), c(n);
        std::vector<int64_t> v((size_t)n * (size_t)std::max(na, 1));
        rc = imm3_comm_merge_groups(&one, queries[i], segment_index[i], n_queries[i], k.data(), f.data(), c.data(), v.data(), n, &n);
        if (rc) return rc;
        for (uint32_t g = 0; g < n; ++g) {
            MergedGroup m;
            m.key = k[g];
            m.first = f[g];
            m.count = c[g];
            for (int j = 0; j < kMaxAggs; ++j) m.vals[j] = j < na ? v[(size_t)g * na + j] : 0;
            auto it = all.find(m.key);
            if (it == all.end()) all.emplace(m.key, m);
            else combine(it->second, m, kinds, is_str, n_agg);
        }
    }
    std::vector<MergedGroup> merged;
    for (auto &kv : all) merged.push_back(kv.second);
    std::sort(merged.begin(), merged.end(), [](const MergedGroup &x, const MergedGroup &y) { return x.first < y.first; });
    *n_groups = (uint32_t)merged.size();
    for (size_t o = 0; o < merged.size() && o < max_groups; ++o) {
        if (keys) keys[o] = merged[o].key;
        if (first) first[o] = merged[o].first;
        if (counts) counts[o] = merged[o].count;
        if (vals)
            for (int j = 0; j < n_agg; ++j) vals[o * (size_t)n_agg + (size_t)j] = kinds[j] == AGG_COUNT ? (int64_t)merged[o].count : (int64_t)merged[o].vals[j];
    }
    return IMM3_OK;
}

// ---------------------------------------------------------------------------------------------
// The same merge by BYTE key: group keys of 0 .. IMM3_GROUP_KEY_MAX_WIDTH bytes and string maxima of any width
// (imm3_comm_merge_groups_wide).  Every (query, group) becomes one immutable record (MergeWideArgs, imm3_internal.h); the records go
// through a device hash table whose slots hold the index of the record that claimed them, the occupied slots come out as records
// again, and with more than one rank those lists are exchanged with ncclAllGather -- fixed-size slots, sized by an all-reduce(max)
// of the list lengths -- and go through the same table once more.  The protocol around the collectives is that of
// imm3_comm_merge_groups: everything that can fail on one rank alone happens before the first collective and travels with the
// shape vote, so every rank takes the same exit.
// ---------------------------------------------------------------------------------------------
namespace {

struct WideSpec {
    int key_bytes = 0, n_agg = 0;
    int32_t kinds[kMaxAggs] = {0, 0, 0, 0}, is_str[kMaxAggs] = {0, 0, 0, 0};
    int32_t str_width[kMaxAggs] = {0, 0, 0, 0}; // of every MAX over a STRING column, narrow ones included; 0: another aggregate
    bool operator==(const WideSpec &o) const {
        if (key_bytes != o.key_bytes || n_agg != o.n_agg) return false;
        for (int j = 0; j < kMaxAggs; ++j)
            if (kinds[j] != o.kinds[j] || is_str[j] != o.is_str[j] || str_width[j] != o.str_width[j]) return false;
        return true;
    }
    // what the ranks vote on: {key width, aggregates, their kinds, which are strings}, {the string widths}
    unsigned long long vote(int word) const {
        unsigned long long v = 0;
        if (word == 0) {
            v = (unsigned long long)key_bytes | (unsigned long long)n_agg << 16;
            for (int j = 0; j < kMaxAggs; ++j) v |= (unsigned long long)(kinds[j] & 3) << (24 + 2 * j) | (unsigned long long)(is_str[j] & 1) << (32 + j);
        } else
            for (int j = 0; j < kMaxAggs; ++j) v |= (unsigned long long)str_width[j] << (16 * j);
        return v;
    }
};

WideSpec wide_spec_of(const imm3_query *q) {
    WideSpec sp;
    for (int32_t g : q->group_cols) sp.key_bytes += q->seg->cols[(size_t)q->used[(size_t)g]].width;
    sp.n_agg = (int)q->aggs.size();
    for (int j = 0; j < sp.n_agg; ++j) {
        const SegCol &sc = q->seg->cols[(size_t)q->used[(size_t)q->aggs[(size_t)j].column]];
        sp.kinds[j] = q->aggs[(size_t)j].kind;
        sp.is_str[j] = sc.vcodec == IMM3_DENSE_STRING;
        if (sp.kinds[j] == AGG_MAX && sp.is_str[j]) sp.str_width[j] = sc.width;
    }
    return sp;
}

// the record geometry of a spec (the table and list pointers stay null)
MergeWideArgs wide_geometry(const WideSpec &sp) {
    MergeWideArgs a;
    std::memset(&a, 0, sizeof(a));
    a.key_bytes = sp.key_bytes;
    a.key_words = (sp.key_bytes + 7) / 8;
    a.n_agg = sp.n_agg;
    int off = kMergeWideHead + a.key_words, planes = 0;
    for (int j = 0; j < kMaxAggs; ++j) {
        a.kinds[j] = sp.kinds[j];
        a.is_str[j] = sp.is_str[j];
        a.best_plane[j] = -1;
        if (sp.str_width[j] > 8) {
            a.str_off[j] = off;
            a.str_words[j] = (sp.str_width[j] + 7) / 8;
            a.str_width[j] = sp.str_width[j];
            a.best_plane[j] = planes++;
            off += a.str_words[j];
        }
    }
    a.rec_words = off;
    return a;
}
int wide_planes(const MergeWideArgs &a) {
    int n = 0;
    for (int j = 0; j < kMaxAggs; ++j) n += a.best_plane[j] >= 0;
    return n;
}

// one allocation: {counts, first, vals[kMaxAggs]} x slots, the collected list and its counter, then the 32-bit planes {claim, best ...}
size_t wide_table_bytes(const MergeWideArgs &geo, unsigned long long slots, unsigned long long list_cap) {
    return (size_t)((slots * (2 + kMaxAggs) + list_cap * (unsigned long long)geo.rec_words + 8) * sizeof(unsigned long long) +
                    slots * (unsigned long long)(1 + wide_planes(geo)) * sizeof(uint32_t));
}
void wide_bind(MergeWideArgs &a, void *p, unsigned long long slots, unsigned long long list_cap) {
    a.slots = (uint32_t)slots;
    a.mask = (uint32_t)(slots - 1);
    unsigned long long *w = (unsigned long long *)p;
    a.t_counts = w;
    a.t_first = a.t_counts + slots;
    a.t_vals = (long long *)(a.t_first + slots);
    a.out_recs = (unsigned long long *)(a.t_vals + (size_t)kMaxAggs * slots);
    a.out_n = a.out_recs + list_cap * (unsigned long long)a.rec_words;
    a.out_cap = (uint32_t)list_cap;
    a.t_claim = (uint32_t *)(a.out_n + 8);
    a.t_best = a.t_claim + slots;
}

void combine_wide(unsigned long long *into, const unsigned long long *g, const MergeWideArgs &geo) {
    into[0] = std::min(into[0], g[0]);
    into[1] += g[1];
    for (int j = 0; j < geo.n_agg; ++j) {
        unsigned long long &t = into[2 + j];
        const unsigned long long v = g[2 + j];
        if (geo.kinds[j] == AGG_MAX) t = geo.is_str[j] ? std::max(t, v) : (unsigned long long)std::max((long long)t, (long long)v);
        else if (geo.kinds[j] == AGG_MIN) t = (unsigned long long)std::min((long long)t, (long long)v);
        else if (geo.kinds[j] == AGG_SUM) t += v;
        if (geo.str_off[j] && std::memcmp(g + geo.str_off[j], into + geo.str_off[j], (size_t)geo.str_width[j]) > 0)
            std::memcpy(into + geo.str_off[j], g + geo.str_off[j], (size_t)geo.str_words[j] * sizeof(unsigned long long));
    }
}

// records (any order) -> the caller's arrays, ascending first arrival
void unpack_wide(const std::vector<unsigned long long> &recs, const WideSpec &sp, const MergeWideArgs &geo, uint8_t *key_bytes_out, uint64_t *first,
                 uint64_t *counts, int64_t *vals, uint8_t *const *str_out, uint32_t max_groups, uint32_t *n_groups) {
    const size_t R = (size_t)geo.rec_words, n = recs.size() / R;
    std::vector<const unsigned long long *> order(n);
    for (size_t i = 0; i < n; ++i) order[i] = recs.data() + i * R;
    std::sort(order.begin(), order.end(), [](const unsigned long long *x, const unsigned long long *y) { return x[0] < y[0]; }); // first arrival first
    *n_groups = (uint32_t)n;
    for (size_t o = 0; o < n && o < max_groups; ++o) {
        const unsigned long long *w = order[o];
        if (key_bytes_out && sp.key_bytes) std::memcpy(key_bytes_out + o * (size_t)sp.key_bytes, w + kMergeWideHead, (size_t)sp.key_bytes);
        if (first) first[o] = w[0];
        if (counts) counts[o] = w[1];
        for (int j = 0; j < sp.n_agg; ++j) {
            if (vals) vals[o * (size_t)sp.n_agg + (size_t)j] = sp.kinds[j] == AGG_COUNT ? (int64_t)w[1] : (int64_t)w[2 + j];
            if (!str_out || !str_out[j]) continue;
            const size_t wd = (size_t)sp.str_width[j];
            uint8_t *dst = str_out[j] + o * wd;
            if (geo.str_off[j]) std::memcpy(dst, w + geo.str_off[j], wd);
            else // (<= 8 bytes: the value packed big-endian)
                for (size_t b = 0; b < wd; ++b) dst[b] = (uint8_t)(w[2 + j] >> (8 * (wd - 1 - b)));
        }
    }
}

// The merged records of this communicator's ranks (every rank gets all of them), in no particular order.
int merge_wide_records(imm3_comm *c, imm3_query *const *queries, const int32_t *segment_index, int32_t n_queries, uint8_t *const *str_out,
                       WideSpec &sp, std::vector<unsigned long long> &out) {
    imm3_ctx *ctx = c->ctx;
    imm3::GateScope gate(&ctx->gate);
    if (ctx->closed) return fail(IMM3_ERR_STATE, "the context of this communicator has been destroyed");
    if (ctx->capture) return fail(IMM3_ERR_STATE, "a graph capture is open on this context");
    HIPCHK(hipSetDevice(ctx->device));
    // ---- everything this rank can get wrong on its own, before the first collective ----
    int local_rc = IMM3_OK;
    std::string local_why;
    auto local_fail = [&](int code, const std::string &msg) {
        if (local_rc == IMM3_OK) { local_rc = code; local_why = msg; }
    };
    {
        const char *why = "";
        const int src = same_spec(queries, n_queries, &why);
        if (src) local_fail(src, why);
        else if (n_queries == 0) local_fail(IMM3_ERR_ARG, "a rank joins the merge with at least one aggregation query (the aggregates' kinds come from it)");
    }
    std::vector<uint32_t> n_local((size_t)std::max(n_queries, 0), 0u);
    if (local_rc == IMM3_OK) {
        sp = wide_spec_of(queries[0]);
        for (int32_t i = 1; i < n_queries && local_rc == IMM3_OK; ++i) {
            const WideSpec si = wide_spec_of(queries[i]);
            if (si.key_bytes != sp.key_bytes) local_fail(IMM3_ERR_ARG, "the queries' group keys differ in width");
            else if (!(si == sp)) local_fail(IMM3_ERR_ARG, "the queries aggregate differently (kinds, or the widths of their string MAX columns)");
        }
        for (int j = 0; j < kMaxAggs && local_rc == IMM3_OK && str_out; ++j)
            if (j < sp.n_agg && str_out[j] && !sp.str_width[j]) local_fail(IMM3_ERR_ARG, "str_out[" + std::to_string(j) + "] is set, but that aggregate is not a MAX over a STRING column");
        for (int32_t i = 0; i < n_queries && local_rc == IMM3_OK; ++i) {
            if (queries[i]->ctx != ctx) { local_fail(IMM3_ERR_ARG, "the query runs on another context than the communicator"); break; }
            const int grc = query_groups(queries[i], &n_local[(size_t)i]);
            if (grc) local_fail(grc, imm3_last_error());
        }
    }
    constexpr unsigned long long kMaxMergeEntries = 1ULL << 30; // (the table's slot fields and record indices are 32 bits; 0xFFFFFFFF is the empty marker)
    unsigned long long total_local = 0;
    uint32_t most_local = 0;
    for (int32_t i = 0; i < n_queries; ++i) { total_local += n_local[(size_t)i]; most_local = std::max(most_local, n_local[(size_t)i]); }
    if (local_rc == IMM3_OK && total_local > kMaxMergeEntries) local_fail(IMM3_ERR_ARG, "too many groups to merge");
    hipStream_t s = ctx->stream;
    if (c->world > 1) {
        const int rrc = rccl_ready();
        if (rrc) return rrc; // (no RCCL in this process: no rank of this process can be inside the collective either)
        if (c->in_flight) HIPCHK(hipStreamWaitEvent(s, c->ev_done, 0));
        unsigned long long shape[5] = {sp.vote(0), sp.vote(1), ~sp.vote(0), ~sp.vote(1), local_rc == IMM3_OK ? 0ULL : 1ULL};
        if (local_rc != IMM3_OK) shape[0] = shape[1] = shape[2] = shape[3] = 0ULL; // (a failed rank does not vote on the shape)
        HIPCHK(hipMemcpyAsync(c->d_slot, shape, sizeof(shape), hipMemcpyHostToDevice, s));
        NCCLCHK(g_rccl.AllReduce(c->d_slot, c->d_slot, 5, ncclUint64, ncclMax, c->nccl, s));
        HIPCHK(hipMemcpyAsync(shape, c->d_slot, sizeof(shape), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (local_rc != IMM3_OK) return fail(local_rc, local_why);
        if (shape[4]) return fail(IMM3_ERR_STATE, "another rank failed before the merge (its call says why); no rank has merged anything");
        if (shape[0] != ~shape[2] || shape[1] != ~shape[3]) // (max != min: every rank sees it and leaves here)
            return fail(IMM3_ERR_ARG, "the ranks' aggregation queries differ in key width, aggregates or string MAX widths");
    } else if (local_rc != IMM3_OK) return fail(local_rc, local_why);
    const MergeWideArgs geo = wide_geometry(sp);
    const size_t R = (size_t)geo.rec_words;
    auto pow2_at_least = [](unsigned long long v) { unsigned long long p = 1024; while (p < v) p <<= 1; return p; };
    auto round8 = [](size_t v) { return (v + 7) & ~(size_t)7; };
    // ---- this rank's records and their merge: {records, key bytes of one query, string bytes of one query per wide MAX, table} ----
    const unsigned long long n1 = std::max<unsigned long long>(total_local, 1), slots1 = pow2_at_least(2 * n1);
    const size_t rec_bytes = (size_t)n1 * R * sizeof(unsigned long long);
    const size_t keyb_bytes = sp.key_bytes > 8 ? round8((size_t)most_local * (size_t)sp.key_bytes) : 0;
    size_t strb_bytes[kMaxAggs], tmp_bytes = keyb_bytes;
    for (int j = 0; j < kMaxAggs; ++j) { strb_bytes[j] = geo.str_off[j] ? round8((size_t)most_local * (size_t)geo.str_width[j]) : 0; tmp_bytes += strb_bytes[j]; }
    void *p1 = nullptr;
    {
        const hipError_t e = hipMalloc(&p1, rec_bytes + tmp_bytes + wide_table_bytes(geo, slots1, n1));
        if (e != hipSuccess) { (void)hipGetLastError(); p1 = nullptr; }
    }
    std::unique_ptr<void, void (*)(void *)> g1(p1, [](void *q) { (void)hipFree(q); });
    std::string p1_why = "hipMalloc of the merge table failed";
    unsigned long long mine = 0;
    MergeWideArgs a1 = geo;
    if (p1) {
        // device work of THIS rank between two collectives: a failure clears p1 instead of returning (the rank then says ~0 in the
        // list-length all-reduce and every rank leaves together)
        auto local_step = [&](hipError_t e, const char *what) {
            if (e == hipSuccess || !p1) return;
            (void)hipGetLastError();
            p1_why = std::string(what) + ": " + hipGetErrorString(e);
            p1 = nullptr;
        };
        unsigned long long *d_recs = (unsigned long long *)p1;
        uint8_t *d_tmp = (uint8_t *)p1 + rec_bytes;
        uint8_t *d_keyb = d_tmp, *d_strb[kMaxAggs];
        d_tmp += keyb_bytes;
        for (int j = 0; j < kMaxAggs; ++j) { d_strb[j] = d_tmp; d_tmp += strb_bytes[j]; }
        wide_bind(a1, d_tmp, slots1, n1);
        launch_mergew_init(a1, s);
        local_step(hipGetLastError(), "merge table init");
        size_t at = 0;
        for (int32_t i = 0; i < n_queries && p1; ++i) {
            imm3_query *q = queries[i];
            const uint32_t ng = n_local[(size_t)i];
            if (!ng) continue;
            AggArgs qa;
            query_agg_args(q, qa);
            a1.q_keys = q->d_okeys;
            a1.q_key_bytes = nullptr;
            if (sp.key_bytes > 8) { // (the table holds tags: the bytes are read at each group's first row)
                launch_group_keys(qa, ng, sp.key_bytes, d_keyb, s);
                a1.q_key_bytes = d_keyb;
            }
            for (int j = 0; j < kMaxAggs; ++j) {
                a1.q_str[j] = nullptr;
                if (!geo.str_off[j]) continue;
                launch_strmax_collect(qa, j, ng, d_strb[j], s);
                a1.q_str[j] = d_strb[j];
            }
            a1.q_first = q->d_ofirst;
            a1.q_counts = q->d_ocounts;
            a1.q_vals = q->d_ovals;
            a1.n_groups = ng;
            a1.seg_hi = (unsigned long long)(uint32_t)segment_index[i] << 32;
            a1.rec_out = d_recs + at * R;
            launch_mergew_pack(a1, s); // (the next query's gathers overwrite d_keyb / d_strb behind this launch: same stream)
            local_step(hipGetLastError(), "merge pack");
            at += ng;
        }
        if (p1) {
            a1.recs = d_recs;
            a1.n_recs = (uint32_t)total_local;
            if (total_local) launch_mergew_insert(a1, s);
            launch_mergew_collect(a1, s);
            local_step(hipGetLastError(), "merge insert / collect");
        }
        if (p1) local_step(hipMemcpyAsync(&mine, a1.out_n, sizeof(mine), hipMemcpyDeviceToHost, s), "merge list length");
        if (p1) local_step(hipStreamSynchronize(s), "merge list length");
    }
    auto take_list = [&](const unsigned long long *d_list, unsigned long long n) -> int {
        out.assign((size_t)n * R, 0ULL);
        if (n) HIPCHK(hipMemcpyAsync(out.data(), d_list, out.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return IMM3_OK;
    };
    if (c->world == 1) {
        if (!p1) return fail(IMM3_ERR_DEVICE, p1_why);
        return take_list(a1.out_recs, mine);
    }
    // list lengths -> the common slot count (a rank whose table could not be built says so with ~0: every rank leaves)
    unsigned long long word = p1 ? mine : ~0ULL, most = 0;
    HIPCHK(hipMemcpyAsync(c->d_slot, &word, sizeof(word), hipMemcpyHostToDevice, s));
    NCCLCHK(g_rccl.AllReduce(c->d_slot, c->d_slot, 1, ncclUint64, ncclMax, c->nccl, s));
    HIPCHK(hipMemcpyAsync(&most, c->d_slot, sizeof(most), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (most == ~0ULL) return fail(IMM3_ERR_DEVICE, p1 ? std::string("a rank could not build its merge table; no rank has merged anything") : p1_why + "; no rank has merged anything");
    out.clear();
    const size_t per_rank = (size_t)most * R;
    if (!per_rank) return IMM3_OK;
    const unsigned long long entries = most * (unsigned long long)c->world;
    if (entries > kMaxMergeEntries) return fail(IMM3_ERR_ARG, "too many groups to merge"); // (the same figure on every rank: every rank leaves here)
    const unsigned long long slots2 = pow2_at_least(2 * entries);
    void *p = nullptr;
    // (sizes are the same on every rank: an allocation failure here is reported through one more flag exchange)
    hipError_t e = hipMalloc(&p, (per_rank + per_rank * (size_t)c->world) * sizeof(unsigned long long) + wide_table_bytes(geo, slots2, entries));
    if (e != hipSuccess) { (void)hipGetLastError(); p = nullptr; }
    std::unique_ptr<void, void (*)(void *)> guard(p, [](void *q) { (void)hipFree(q); });
    unsigned long long ok = p ? 0ULL : 1ULL, any = 0;
    HIPCHK(hipMemcpyAsync(c->d_slot, &ok, sizeof(ok), hipMemcpyHostToDevice, s));
    NCCLCHK(g_rccl.AllReduce(c->d_slot, c->d_slot, 1, ncclUint64, ncclMax, c->nccl, s));
    HIPCHK(hipMemcpyAsync(&any, c->d_slot, sizeof(any), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (any) return fail(IMM3_ERR_DEVICE, "a rank could not allocate the exchange buffers of the merge; no rank has merged anything");
    unsigned long long *d_send = (unsigned long long *)p, *d_recv = d_send + per_rank;
    HIPCHK(hipMemsetAsync(d_send, 0, per_rank * sizeof(unsigned long long), s)); // (padding records: count 0)
    if (mine) HIPCHK(hipMemcpyAsync(d_send, a1.out_recs, (size_t)mine * R * sizeof(unsigned long long), hipMemcpyDeviceToDevice, s));
    NCCLCHK(g_rccl.AllGather(d_send, d_recv, per_rank, ncclUint64, c->nccl, s));
    MergeWideArgs a2 = geo;
    wide_bind(a2, d_recv + per_rank * (size_t)c->world, slots2, entries);
    launch_mergew_init(a2, s);
    HIPCHK(hipGetLastError());
    a2.recs = d_recv;
    a2.n_recs = (uint32_t)entries;
    launch_mergew_insert(a2, s);
    HIPCHK(hipGetLastError());
    launch_mergew_collect(a2, s);
    HIPCHK(hipGetLastError());
    unsigned long long n2 = 0;
    HIPCHK(hipMemcpyAsync(&n2, a2.out_n, sizeof(n2), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return take_list(a2.out_recs, n2);
}

} // namespace

extern "C" int imm3_comm_merge_groups_wide(imm3_comm *c, imm3_query *const *queries, const int32_t *segment_index, int32_t n_queries,
                                           uint8_t *key_bytes_out, uint64_t *first, uint64_t *counts, int64_t *vals,
                                           uint8_t *const *str_out, uint32_t max_groups, uint32_t *n_groups) {
    if (!c || !n_groups || n_queries < 0 || (n_queries > 0 && (!queries || !segment_index))) return fail(IMM3_ERR_ARG, "bad argument");
    WideSpec sp;
    std::vector<unsigned long long> recs;
    const int rc = merge_wide_records(c, queries, segment_index, n_queries, str_out, sp, recs);
    if (rc) return rc;
    unpack_wide(recs, sp, wide_geometry(sp), key_bytes_out, first, counts, vals, str_out, max_groups, n_groups);
    return IMM3_OK;
}

// Single-process flavour (comms from imm3_comm_create_all): per device the world-of-one merge above, then one merge by byte key on
// the host.
extern "C" int imm3_comm_merge_groups_wide_all(imm3_comm *const *comms, int32_t n_comms, imm3_query *const *const *queries,
                                               const int32_t *const *segment_index, const int32_t *n_queries,
                                               uint8_t *key_bytes_out, uint64_t *first, uint64_t *counts, int64_t *vals,
                                               uint8_t *const *str_out, uint32_t max_groups, uint32_t *n_groups) {
    if (!comms || n_comms < 1 || !queries || !segment_index || !n_queries || !n_groups) return fail(IMM3_ERR_ARG, "bad argument");
    bool have = false;
    WideSpec sp;
    MergeWideArgs geo = wide_geometry(sp);
    std::map<std::string, std::vector<unsigned long long>> all;
    for (int32_t i = 0; i < n_comms; ++i) {
        if (!comms[i] || n_queries[i] < 0 || (n_queries[i] > 0 && (!queries[i] || !segment_index[i]))) return fail(IMM3_ERR_ARG, "bad argument");
        if (n_queries[i] == 0) continue;
        imm3_comm one = *comms[i]; // the same communicator seen as a world of one: its device's queries merged without a collective
        one.world = 1;
        WideSpec si;
        std::vector<unsigned long long> recs;
        const int rc = merge_wide_records(&one, queries[i], segment_index[i], n_queries[i], str_out, si, recs);
        if (rc) return rc;
        if (!have) { sp = si; geo = wide_geometry(sp); have = true; }
        else if (!(si == sp)) return fail(IMM3_ERR_ARG, "the devices' aggregation queries differ in key width, aggregates or string MAX widths");
        const size_t R = (size_t)geo.rec_words;
        for (size_t g = 0; g < recs.size() / R; ++g) {
            const unsigned long long *w = recs.data() + g * R;
            std::string key((const char *)(w + kMergeWideHead), (size_t)sp.key_bytes);
            auto it = all.find(key);
            if (it == all.end()) all.emplace(std::move(key), std::vector<unsigned long long>(w, w + R));
            else combine_wide(it->second.data(), w, geo);
        }
    }
    std::vector<unsigned long long> merged;
    for (auto &kv : all) merged.insert(merged.end(), kv.second.begin(), kv.second.end());
    unpack_wide(merged, sp, geo, key_bytes_out, first, counts, vals, str_out, max_groups, n_groups);
    return IMM3_OK;
}

// ---------------------------------------------------------------------------------------------
// Merging ORDERED results (imm3_comm_merge_ordered; DESIGN.md section 21, "Merging ordered results").  Every (query, ordered row)
// becomes one record whose first six words are its sort key (imm3_merge_order.h); this rank's lists -- one per query, already in
// order -- are merged by k_merge_order_rank and cut to the limit, and with more than one rank those lists are exchanged with
// ncclAllGather -- fixed-size slots, sized by an all-reduce(max) of the list lengths -- and merged by the same kernel.  The
// protocol around the collectives is that of merge_wide_records: everything that can fail on one rank alone happens before the
// first collective and travels with the shape vote, so every rank takes the same exit.
// ---------------------------------------------------------------------------------------------
namespace {

MergeOrderSpec order_spec_of(const imm3_query *q) {
    MergeOrderSpec sp;
    for (int32_t p : q->proj) {
        const SegCol &sc = q->seg->cols[(size_t)q->used[(size_t)p]];
        sp.widths.push_back(sc.width);
        sp.kinds.push_back(sc.vcodec == IMM3_DENSE_INT ? KIND_I32 : (sc.vcodec == IMM3_DENSE_TINYINT ? KIND_I8 : KIND_STR));
    }
    for (const imm3_order_key &k : q->order_keys) {
        sp.key_proj.push_back(k.proj);
        sp.key_desc.push_back(k.descending ? 1 : 0);
    }
    return sp;
}

// The merged records of this communicator's ranks, in order, cut to `limit` (every rank gets all of them); *total: their number.
int merge_ordered_records(imm3_comm *c, imm3_query *const *queries, const int32_t *segment_index, int32_t n_queries, int64_t limit,
                          MergeOrderSpec &sp, std::vector<uint32_t> &out, uint64_t *total) {
    imm3_ctx *ctx = c->ctx;
    imm3::GateScope gate(&ctx->gate);
    if (ctx->closed) return fail(IMM3_ERR_STATE, "the context of this communicator has been destroyed");
    if (ctx->capture) return fail(IMM3_ERR_STATE, "a graph capture is open on this context");
    HIPCHK(hipSetDevice(ctx->device));
    out.clear();
    *total = 0;
    // ---- everything this rank can get wrong on its own, before the first collective ----
    int local_rc = IMM3_OK;
    std::string local_why;
    auto local_fail = [&](int code, const std::string &msg) {
        if (local_rc == IMM3_OK) { local_rc = code; local_why = msg; }
    };
    if (n_queries == 0) local_fail(IMM3_ERR_ARG, "a rank joins the merge with at least one ordered query (the SELECT list and the keys come from it)");
    for (int32_t i = 0; i < n_queries && local_rc == IMM3_OK; ++i) {
        const imm3_query *q = queries[i];
        if (!q) local_fail(IMM3_ERR_ARG, "query is null");
        else if (q->is_agg || q->proj.empty() || !q->ordered) local_fail(IMM3_ERR_ARG, "not an ordered projection (imm3_query_set_order on a projecting query)");
        else if (q->ctx != ctx) local_fail(IMM3_ERR_ARG, "the query runs on another context than the communicator");
    }
    for (int32_t i = 0; i < n_queries && local_rc == IMM3_OK; ++i)
        if (!queries[i]->run.ran_project) local_fail(IMM3_ERR_STATE, "imm3_query_run has not been called");
    std::vector<int32_t> n_entries((size_t)std::max(n_queries, 0), 1);
    std::vector<size_t> entry_at((size_t)std::max(n_queries, 0), 0);
    std::vector<uint64_t> n_local((size_t)std::max(n_queries, 0), 0);
    std::vector<char> split((size_t)std::max(n_queries, 0), 0); // a table query whose global indices are not ascending
    unsigned long long total_local = 0;
    if (local_rc == IMM3_OK) {
        sp = order_spec_of(queries[0]);
        for (int32_t i = 1; i < n_queries && local_rc == IMM3_OK; ++i)
            if (!(order_spec_of(queries[i]) == sp)) local_fail(IMM3_ERR_ARG, "the queries differ in their SELECT lists (columns, widths, kinds) or in their order keys");
    }
    if (local_rc == IMM3_OK) {
        std::vector<int64_t> own((size_t)n_queries);
        size_t at = 0;
        for (int32_t i = 0; i < n_queries; ++i) {
            own[(size_t)i] = queries[i]->order_limit;
            n_entries[(size_t)i] = queries[i]->table ? (int32_t)queries[i]->table->segs.size() : 1;
            entry_at[(size_t)i] = at;
            at += (size_t)n_entries[(size_t)i];
        }
        std::string why;
        if (!merge_order_check(limit, own.data(), n_entries.data(), n_queries, segment_index, &why)) local_fail(IMM3_ERR_ARG, why);
        for (int32_t i = 0; i < n_queries && local_rc == IMM3_OK; ++i)
            for (int32_t e = 1; e < n_entries[(size_t)i]; ++e)
                if (segment_index[entry_at[(size_t)i] + (size_t)e] < segment_index[entry_at[(size_t)i] + (size_t)e - 1]) split[(size_t)i] = 1;
    }
    for (int32_t i = 0; i < n_queries && local_rc == IMM3_OK; ++i) { // (waits for the run; orders again when the arrays were outgrown)
        const int rrc = imm3_query_row_count(queries[i], &n_local[(size_t)i]);
        if (rrc) local_fail(rrc, imm3_last_error());
        total_local += n_local[(size_t)i];
    }
    if (local_rc == IMM3_OK && total_local > kMergeOrderMaxRows) local_fail(IMM3_ERR_ARG, "too many rows to merge (more than 2^30 enter the merge)");
    hipStream_t s = ctx->stream;
    if (c->world > 1) {
        const int rrc = rccl_ready();
        if (rrc) return rrc; // (no RCCL in this process: no rank of this process can be inside the collective either)
        if (c->in_flight) HIPCHK(hipStreamWaitEvent(s, c->ev_done, 0));
        unsigned long long shape[5] = {sp.vote(0, limit), sp.vote(1, limit), ~sp.vote(0, limit), ~sp.vote(1, limit), local_rc == IMM3_OK ? 0ULL : 1ULL};
        if (local_rc != IMM3_OK) shape[0] = shape[1] = shape[2] = shape[3] = 0ULL; // (a failed rank does not vote on the shape)
        HIPCHK(hipMemcpyAsync(c->d_slot, shape, sizeof(shape), hipMemcpyHostToDevice, s));
        NCCLCHK(g_rccl.AllReduce(c->d_slot, c->d_slot, 5, ncclUint64, ncclMax, c->nccl, s));
        HIPCHK(hipMemcpyAsync(shape, c->d_slot, sizeof(shape), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (local_rc != IMM3_OK) return fail(local_rc, local_why);
        if (shape[4]) return fail(IMM3_ERR_STATE, "another rank failed before the merge (its call says why); no rank has merged anything");
        if (shape[0] != ~shape[2] || shape[1] != ~shape[3]) // (max != min: every rank sees it and leaves here)
            return fail(IMM3_ERR_ARG, "the ranks' ordered queries differ in SELECT list, order keys or the merge's limit");
    } else if (local_rc != IMM3_OK) return fail(local_rc, local_why);
    const MergeOrderGeometry geo = merge_order_geometry(sp.widths);
    const size_t R = (size_t)geo.rec_words;
    const uint64_t ulimit = limit > 0 ? (uint64_t)limit : 0;
    auto cut_of = [&](unsigned long long n) { return ulimit && ulimit < n ? (unsigned long long)ulimit : n; };
    // ---- this rank's lists and their merge.  One allocation: {input records, a split query's records in its own order, merged
    // records, total word, list table, per table query: tile starts + global indices, a split query's per-segment counts} ----
    int32_t n_lists = 0;
    unsigned long long list_cap = 0, split_rows = 0, split_segs = 0, meta_u32 = 0;
    for (int32_t i = 0; i < n_queries; ++i) {
        n_lists += split[(size_t)i] ? n_entries[(size_t)i] : 1;
        list_cap = std::max<unsigned long long>(list_cap, n_local[(size_t)i]);
        if (split[(size_t)i]) { split_rows = std::max<unsigned long long>(split_rows, n_local[(size_t)i]); split_segs = std::max<unsigned long long>(split_segs, (unsigned long long)n_entries[(size_t)i]); }
        if (queries[i]->table) meta_u32 += 2ULL * (unsigned long long)n_entries[(size_t)i] + 2ULL;
    }
    auto even = [](unsigned long long v) { return (v + 1ULL) & ~1ULL; };
    const unsigned long long mine = cut_of(total_local);
    const unsigned long long in_words = total_local * R, tmp_words = split_rows * R, out_words = mine * R;
    const unsigned long long w_in = 0, w_tmp = w_in + in_words, w_out = w_tmp + tmp_words, w_total = w_out + out_words, w_lists = w_total + 2,
                             w_meta = w_lists + 4ULL * (unsigned long long)n_lists, w_counts = w_meta + even(meta_u32), w_end = w_counts + even(split_segs);
    const unsigned long long rank_waves = (unsigned long long)n_lists * ((list_cap + 63ULL) / 64ULL);
    void *p1 = nullptr;
    std::string p1_why = "hipMalloc of the ordered merge's buffers failed";
    if (rank_waves / 4ULL >= 0x7FFFFFFFULL) p1_why = "too many lists of too many rows to merge in one launch";
    else {
        const hipError_t e = hipMalloc(&p1, (size_t)w_end * sizeof(uint32_t));
        if (e != hipSuccess) { (void)hipGetLastError(); p1 = nullptr; }
    }
    std::unique_ptr<void, void (*)(void *)> g1(p1, [](void *q) { (void)hipFree(q); });
    uint32_t *const d1 = (uint32_t *)p1;
    std::vector<uint32_t> h_meta;              // host images: live until the stream has been synchronised below
    std::vector<unsigned long long> h_lists;
    if (p1) {
        // device work of THIS rank between two collectives: a failure clears p1 instead of returning (the rank then says ~0 in the
        // list-length all-reduce and every rank leaves together)
        auto local_step = [&](hipError_t e, const char *what) {
            if (e == hipSuccess || !p1) return;
            (void)hipGetLastError();
            p1_why = std::string(what) + ": " + hipGetErrorString(e);
            p1 = nullptr;
        };
        local_step(hipMemsetAsync(d1, 0, (size_t)w_end * sizeof(uint32_t), s), "merge buffer clear"); // (pad words: records are bit-exact images)
        // the list table and the tables' lookups
        h_lists.assign(2 * (size_t)n_lists, 0ULL);
        h_meta.assign((size_t)even(meta_u32), 0u);
        std::vector<size_t> meta_at((size_t)n_queries, 0), list_at((size_t)n_queries, 0);
        {
            size_t m = 0, l = 0;
            unsigned long long rec_at = 0;
            for (int32_t i = 0; i < n_queries; ++i) {
                const imm3_query *q = queries[i];
                list_at[(size_t)i] = l;
                if (!split[(size_t)i]) { // (a split query's entries are written by its move launch)
                    h_lists[2 * l] = w_in + rec_at * R;
                    h_lists[2 * l + 1] = n_local[(size_t)i];
                }
                l += split[(size_t)i] ? (size_t)n_entries[(size_t)i] : 1;
                rec_at += n_local[(size_t)i];
                if (!q->table) continue;
                meta_at[(size_t)i] = m;
                const int32_t ns = n_entries[(size_t)i];
                for (int32_t t = 0; t <= ns; ++t) h_meta[m + (size_t)t] = (uint32_t)q->table->tile_start[(size_t)t];
                for (int32_t t = 0; t < ns; ++t) h_meta[m + (size_t)ns + 1 + (size_t)t] = (uint32_t)segment_index[entry_at[(size_t)i] + (size_t)t];
                m += 2 * (size_t)ns + 2;
            }
        }
        local_step(hipMemcpyAsync(d1 + w_lists, h_lists.data(), h_lists.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, s), "merge list table");
        if (!h_meta.empty()) local_step(hipMemcpyAsync(d1 + w_meta, h_meta.data(), h_meta.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s), "merge table lookups");
        unsigned long long rec_at = 0;
        for (int32_t i = 0; i < n_queries && p1; ++i) {
            imm3_query *q = queries[i];
            const uint64_t n = n_local[(size_t)i];
            if (!n) continue;
            MergeOrderPackArgs pa;
            std::memset(&pa, 0, sizeof(pa));
            pa.n_keys = (int32_t)q->order_keys.size();
            pa.key_bytes = q->order_key_bytes;
            for (int k = 0; k < pa.n_keys; ++k) {
                const int32_t pj = q->order_keys[(size_t)k].proj;
                pa.keys[k].src = q->d_order_proj[(size_t)pj];
                pa.keys[k].width = sp.widths[(size_t)pj];
                pa.keys[k].kind = sp.kinds[(size_t)pj];
                pa.keys[k].descending = q->order_keys[(size_t)k].descending ? 1 : 0;
            }
            pa.row_index = q->d_order_row_index;
            pa.n_rows = (uint32_t)n;
            pa.rec_words = (int32_t)R;
            pa.recs = d1 + (split[(size_t)i] ? w_tmp : w_in + rec_at * R);
            if (q->table) {
                pa.n_tsegs = n_entries[(size_t)i];
                pa.tile_start = d1 + w_meta + meta_at[(size_t)i];
                pa.global_index = pa.tile_start + pa.n_tsegs + 1;
            } else pa.segment = (uint32_t)segment_index[entry_at[(size_t)i]];
            const size_t np = q->proj.size();
            for (size_t done = 0; done < np && p1;) { // more SELECT-list columns than one launch carries: in groups (the key with the first)
                const size_t take = std::min<size_t>(kMaxProj, np - done);
                pa.with_key = done == 0;
                pa.n_cols = (int32_t)take;
                for (size_t j = 0; j < take; ++j) {
                    pa.cols[j].src = q->d_order_proj[done + j];
                    pa.cols[j].width = sp.widths[done + j];
                    pa.cols[j].rec_off = geo.col_off[done + j];
                }
                done += take;
                launch_merge_order_pack(pa, s);
                local_step(hipGetLastError(), "merge pack");
            }
            if (split[(size_t)i] && p1) {
                MergeOrderSplitArgs sa;
                std::memset(&sa, 0, sizeof(sa));
                sa.src = d1 + w_tmp;
                sa.dst = d1;
                sa.dst_word = w_in + rec_at * R;
                sa.n_rows = (uint32_t)n;
                sa.n_tsegs = n_entries[(size_t)i];
                sa.rec_words = (int32_t)R;
                sa.global_index = pa.global_index;
                sa.counts = d1 + w_counts;
                sa.lists = (unsigned long long *)(d1 + w_lists) + 2 * list_at[(size_t)i];
                launch_merge_order_split(sa, s); // (the next split query reuses the records behind this launch: same stream)
                local_step(hipGetLastError(), "merge split");
            }
            rec_at += n;
        }
        if (p1 && total_local) {
            MergeOrderArgs ma;
            std::memset(&ma, 0, sizeof(ma));
            ma.recs = d1;
            ma.buf_words = w_tmp; // (the input records only)
            ma.lists = (const unsigned long long *)(d1 + w_lists);
            ma.n_lists = n_lists;
            ma.rec_words = (int32_t)R;
            ma.list_cap = (uint32_t)list_cap;
            ma.cut = (uint32_t)mine;
            ma.out = d1 + w_out;
            ma.out_total = (unsigned long long *)(d1 + w_total);
            launch_merge_order_rank(ma, s);
            local_step(hipGetLastError(), "merge rank");
        }
        if (p1) local_step(hipStreamSynchronize(s), "merge of this rank's lists");
    }
    if (c->world == 1) {
        if (!p1) return fail(IMM3_ERR_DEVICE, p1_why);
        out.assign((size_t)out_words, 0u);
        if (out_words) HIPCHK(hipMemcpyAsync(out.data(), d1 + w_out, (size_t)out_words * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        *total = mine;
        return IMM3_OK;
    }
    // list lengths -> the common slot size (a rank whose lists could not be merged says so with ~0: every rank leaves)
    unsigned long long word = p1 ? mine : ~0ULL, most = 0;
    HIPCHK(hipMemcpyAsync(c->d_slot, &word, sizeof(word), hipMemcpyHostToDevice, s));
    NCCLCHK(g_rccl.AllReduce(c->d_slot, c->d_slot, 1, ncclUint64, ncclMax, c->nccl, s));
    HIPCHK(hipMemcpyAsync(&most, c->d_slot, sizeof(most), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (most == ~0ULL) return fail(IMM3_ERR_DEVICE, p1 ? std::string("a rank could not merge its own lists; no rank has merged anything") : p1_why + "; no rank has merged anything");
    if (!most) return IMM3_OK; // (every rank's list is empty)
    const unsigned long long entries = most * (unsigned long long)c->world;
    if (entries > kMergeOrderMaxRows) return fail(IMM3_ERR_ARG, "too many rows to merge (more than 2^30 enter the merge)"); // (the same figure on every rank: every rank leaves here)
    const unsigned long long slot_words = 2ULL + most * R, cut2 = cut_of(entries);
    // {send slot, the ranks' slots, total word, merged records}; sizes are the same on every rank: an allocation failure is reported
    // through one more flag exchange
    const unsigned long long x_recv = slot_words, x_total = x_recv + slot_words * (unsigned long long)c->world, x_out = x_total + 2, x_end = x_out + cut2 * R;
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, (size_t)x_end * sizeof(uint32_t));
    if (e != hipSuccess) { (void)hipGetLastError(); p = nullptr; }
    std::unique_ptr<void, void (*)(void *)> guard(p, [](void *q) { (void)hipFree(q); });
    unsigned long long ok = p ? 0ULL : 1ULL, any = 0;
    HIPCHK(hipMemcpyAsync(c->d_slot, &ok, sizeof(ok), hipMemcpyHostToDevice, s));
    NCCLCHK(g_rccl.AllReduce(c->d_slot, c->d_slot, 1, ncclUint64, ncclMax, c->nccl, s));
    HIPCHK(hipMemcpyAsync(&any, c->d_slot, sizeof(any), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (any) return fail(IMM3_ERR_DEVICE, "a rank could not allocate the exchange buffers of the merge; no rank has merged anything");
    uint32_t *const dx = (uint32_t *)p;
    HIPCHK(hipMemsetAsync(dx, 0, (size_t)slot_words * sizeof(uint32_t), s)); // (the slot's tail behind this rank's records)
    HIPCHK(hipMemcpyAsync(dx, &mine, sizeof(mine), hipMemcpyHostToDevice, s)); // the slot's length word
    if (mine) HIPCHK(hipMemcpyAsync(dx + 2, d1 + w_out, (size_t)out_words * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    NCCLCHK(g_rccl.AllGather(dx, dx + x_recv, (size_t)(slot_words / 2), ncclUint64, c->nccl, s));
    MergeOrderArgs ma;
    std::memset(&ma, 0, sizeof(ma));
    ma.recs = dx + x_recv;
    ma.buf_words = slot_words * (unsigned long long)c->world;
    ma.slot_words = slot_words;
    ma.n_lists = c->world;
    ma.rec_words = (int32_t)R;
    ma.list_cap = (uint32_t)most;
    ma.cut = (uint32_t)cut2;
    ma.out = dx + x_out;
    ma.out_total = (unsigned long long *)(dx + x_total);
    launch_merge_order_rank(ma, s);
    HIPCHK(hipGetLastError());
    std::vector<uint32_t> h((size_t)(2 + cut2 * R)); // one copy: the total word and the records behind it
    HIPCHK(hipMemcpyAsync(h.data(), dx + x_total, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    unsigned long long all = 0;
    std::memcpy(&all, h.data(), sizeof(all));
    *total = std::min(all, cut2);
    out.assign(h.begin() + 2, h.begin() + 2 + (size_t)(*total * R));
    return IMM3_OK;
}

} // namespace

extern "C" int imm3_comm_merge_ordered(imm3_comm *c, imm3_query *const *queries, const int32_t *segment_index, int32_t n_queries,
                                       int64_t limit, uint32_t *segment_out, uint32_t *row_out, void *const *col_out,
                                       uint64_t max_rows, uint64_t *n_rows) {
    if (!c || !n_rows || n_queries < 0 || (n_queries > 0 && (!queries || !segment_index))) return fail(IMM3_ERR_ARG, "bad argument");
    MergeOrderSpec sp;
    std::vector<uint32_t> recs;
    uint64_t total = 0;
    const int rc = merge_ordered_records(c, queries, segment_index, n_queries, limit, sp, recs, &total);
    if (rc) return rc;
    *n_rows = total;
    merge_order_unpack(recs.data(), total, merge_order_geometry(sp.widths), sp.widths, segment_out, row_out, col_out, max_rows);
    return IMM3_OK;
}

// Single-process flavour (comms from imm3_comm_create_all): per device the world-of-one merge above, cut to the limit, then one
// k-way merge of the devices' lists on the host.
extern "C" int imm3_comm_merge_ordered_all(imm3_comm *const *comms, int32_t n_comms, imm3_query *const *const *queries,
                                           const int32_t *const *segment_index, const int32_t *n_queries,
                                           int64_t limit, uint32_t *segment_out, uint32_t *row_out, void *const *col_out,
                                           uint64_t max_rows, uint64_t *n_rows) {
    if (!comms || n_comms < 1 || !queries || !segment_index || !n_queries || !n_rows) return fail(IMM3_ERR_ARG, "bad argument");
    bool have = false;
    MergeOrderSpec sp;
    std::vector<std::vector<uint32_t>> lists;
    std::vector<uint64_t> lens;
    for (int32_t i = 0; i < n_comms; ++i) {
        if (!comms[i] || n_queries[i] < 0 || (n_queries[i] > 0 && (!queries[i] || !segment_index[i]))) return fail(IMM3_ERR_ARG, "bad argument");
        if (n_queries[i] == 0) continue;
        imm3_comm one = *comms[i]; // the same communicator seen as a world of one: its device's queries merged without a collective
        one.world = 1;
        MergeOrderSpec si;
        std::vector<uint32_t> recs;
        uint64_t n = 0;
        const int rc = merge_ordered_records(&one, queries[i], segment_index[i], n_queries[i], limit, si, recs, &n);
        if (rc) return rc;
        if (!have) { sp = si; have = true; }
        else if (!(si == sp)) return fail(IMM3_ERR_ARG, "the devices' ordered queries differ in SELECT list or order keys");
        lists.push_back(std::move(recs));
        lens.push_back(n);
    }
    const MergeOrderGeometry geo = merge_order_geometry(sp.widths);
    std::vector<const uint32_t *> ptrs;
    for (auto &l : lists) ptrs.push_back(l.data());
    std::vector<uint32_t> merged;
    merge_order_host(ptrs.data(), lens.data(), (int32_t)lists.size(), geo.rec_words, limit > 0 ? (uint64_t)limit : 0, merged);
    *n_rows = merged.size() / (size_t)geo.rec_words;
    merge_order_unpack(merged.data(), *n_rows, geo, sp.widths, segment_out, row_out, col_out, max_rows);
    return IMM3_OK;
}
