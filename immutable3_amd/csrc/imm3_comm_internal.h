// imm3_comm_internal.h -- what the communicator's translation units share: the handle (imm3_comm.cpp), the RCCL table bound at
// run time (imm3_comm.cpp), and the collective protocol of the cross-rank merges (imm3_merge_protocol.cpp), which
// imm3_merge_groups.cpp, imm3_merge_wide.cpp and imm3_merge_ordered.cpp are built from.  Private to csrc/.
#pragma once

#include "imm3_handles.h"
#include "imm3_merge_vote.h"

#include <rccl/rccl.h> // types and enums only; every call goes through the table below

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
    int32_t view_path = 0;        // diagnostics (imm3_comm_merge_view_path): the GroupOrderPath of the last imm3_comm_merge_groups_view
};

namespace imm3 {

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
extern Rccl g_rccl;
int rccl_ready(); // binds the library on first use; IMM3_OK, or fail() with why it could not be bound

#define NCCLCHK(expr)                                                                                                    \
    do {                                                                                                                 \
        ncclResult_t _r = (expr);                                                                                        \
        if (_r != ncclSuccess) return fail(IMM3_ERR_DEVICE, std::string(#expr) + ": " + imm3::g_rccl.GetErrorString(_r)); \
    } while (0)

// ---------------------------------------------------------------------------------------------
// The collective protocol of the merges.  Every rank must take the same road AND the same exit: a rank that returned early
// while the others went on to the next collective would leave them waiting in hipStreamSynchronize for good.  So
//   * everything that can fail on this rank alone BEFORE the first collective -- argument checks, the queries' group lists,
//     allocations -- goes into a LocalVerdict and travels with the shape vote (merge_vote);
//   * device work of this rank whose failure the vote no longer carries goes through a LocalStep: a failure is kept, not
//     returned, the rank says ~0 in the list-length exchange (merge_list_length) and every rank leaves together;
//   * what is sized the same on every rank (the exchange buffers) is allocated with one more flag exchange (merge_exchange_alloc);
//   * the lists meet in fixed-size slots (merge_gather).
// All of it runs on the CONTEXT's stream `s`, behind the rank's own kernels.  Where a HIP or RCCL call of the protocol itself
// fails, these functions still return at once (HIPCHK / NCCLCHK): the device is gone then, and the other ranks with it.
// ---------------------------------------------------------------------------------------------
struct LocalVerdict { // the first thing that went wrong on this rank alone
    int rc = IMM3_OK;
    std::string why;
    bool ok() const { return rc == IMM3_OK; }
    void fail(int code, const std::string &msg) {
        if (rc == IMM3_OK) { rc = code; why = msg; }
    }
};

struct LocalStep { // device work of this rank that must not return: the first failure is kept
    bool ok = true;
    std::string why;
    void refuse(const std::string &msg) {
        if (ok) { ok = false; why = msg; }
    }
    void operator()(hipError_t e, const char *what) {
        if (e == hipSuccess || !ok) return;
        (void)hipGetLastError();
        refuse(std::string(what) + ": " + hipGetErrorString(e));
    }
};

struct DeviceBlock { // one hipMalloc, freed with the scope
    void *p = nullptr;
    DeviceBlock() = default;
    DeviceBlock(const DeviceBlock &) = delete;
    DeviceBlock &operator=(const DeviceBlock &) = delete;
    ~DeviceBlock() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { // (a failure leaves no sticky error behind)
        const hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) { (void)hipGetLastError(); p = nullptr; }
        return e;
    }
};

inline unsigned long long pow2_at_least(unsigned long long v) { // slots of a hash table, 1024 at least
    unsigned long long p = 1024;
    while (p < v) p <<= 1;
    return p;
}

// what a rank that meets no other rank returns after its local phase
int merge_local_result(const LocalVerdict &verdict, const LocalStep &step);

// The shape vote (imm3_merge_vote.h): IMM3_OK when every rank is well and brought the same (v0, v1); else this rank's own
// error, "another rank failed", or `differ_message` -- on every rank in the same call.  A world of one: the own error only.
int merge_vote(imm3_comm *c, hipStream_t s, unsigned long long v0, unsigned long long v1, const LocalVerdict &verdict, const char *differ_message);

// one word, all-reduce(max), back on the host (synchronises `s`)
int merge_max_word(imm3_comm *c, hipStream_t s, unsigned long long mine, unsigned long long *most);

// The ranks' list lengths -> the longest.  A rank whose step failed says ~0: it returns its step's reason, the others
// `other_rank_message`, all of them here.
int merge_list_length(imm3_comm *c, hipStream_t s, const LocalStep &step, unsigned long long mine, const char *other_rank_message, unsigned long long *most);

// The exchange buffers: `bytes` is the same figure on every rank, so a rank that cannot allocate says so in one more flag
// exchange and every rank leaves here.
int merge_exchange_alloc(imm3_comm *c, hipStream_t s, size_t bytes, DeviceBlock &block);

// This rank's zeroed slot of `slot_u64` 64-bit words filled -- `length_word` first, where the slot carries one (host memory that
// lives until `s` is next synchronised), then `list_bytes` of `d_list` -- and every rank's slot gathered into d_recv, rank by rank.
int merge_gather(imm3_comm *c, hipStream_t s, void *d_send, void *d_recv, size_t slot_u64, const unsigned long long *length_word, const void *d_list,
                 size_t list_bytes);

// The first check of both group merges (imm3_merge_groups.cpp): every query is an aggregation that has run, all of them aggregate
// alike, and there is at least one.
void merge_check_agg_queries(imm3_query *const *queries, int32_t n, LocalVerdict &verdict);

// ---- views of merged groups (imm3_merge_view_api.cpp; the plan: imm3_merge_view_plan.h).  imm3_merge_wide.cpp runs its merge as always
// and keeps the final record list on the device; these pieces check the view, make the ranks agree on it and compute it there. ----
struct MergeViewCall {
    MergeViewPlan plan;            // the user keys, the program and the limit once merge_view_check has passed; the tie once merge_view_agree has
    uint32_t largest_segment = 0;  // of this rank's segment_index
};
// The view's own checks on this rank (the rules of imm3_query_set_group_order and imm3_query_set_group_filter over queries[0]'s
// shape), into the verdict: they travel with the shape vote.  Called once the queries themselves have passed.
void merge_view_check(imm3_query *const *queries, const int32_t *segment_index, int32_t n_queries, const imm3_group_view *view, MergeViewCall &v, LocalVerdict &verdict);
// Behind the shape vote: every rank brought the same view (one more merge_vote, on the hash of its canonical bytes), the largest
// segment index of any rank (one merge_max_word), then the tie or its refusal -- the same answer on every rank, before any gather.
int merge_view_agree(imm3_comm *c, hipStream_t s, MergeViewCall &v);
// The view of the `n` records at d_list (device, geometry `geo`), computed on the device: the first min(view, max_groups) records in
// the view's order in `out`, *n_view = min(kept, limit), *n_kept.  Local to this rank: nothing collective.
int merge_view_device(imm3_comm *c, MergeViewCall &v, const MergeWideArgs &geo, const unsigned long long *d_list, unsigned long long n, uint32_t max_groups,
                      std::vector<unsigned long long> &out, uint64_t *n_view, uint64_t *n_kept);
// ... and of `n` records on the host (merge_view_host): the single-process flavour
void merge_view_of_host_records(MergeViewCall &v, const MergeWideArgs &geo, const std::vector<unsigned long long> &recs, std::vector<unsigned long long> &out,
                                uint64_t *n_view, uint64_t *n_kept);

} // namespace imm3
