// imm3_merge_protocol.cpp -- the collective protocol of the cross-rank merges (imm3_comm_internal.h says what it is for), once:
// imm3_merge_groups.cpp, imm3_merge_wide.cpp and imm3_merge_ordered.cpp are a local phase each plus an exchange built from these
// pieces.  Every collective here is on the communicator's d_slot (the votes and flags) or on the caller's buffers (the gather), on
// the context's stream.
#include "imm3_comm_internal.h"

namespace imm3 {

int merge_local_result(const LocalVerdict &verdict, const LocalStep &step) {
    if (!verdict.ok()) return fail(verdict.rc, verdict.why);
    if (!step.ok) return fail(IMM3_ERR_DEVICE, step.why);
    return IMM3_OK;
}

int merge_vote(imm3_comm *c, hipStream_t s, unsigned long long v0, unsigned long long v1, const LocalVerdict &verdict, const char *differ_message) {
    if (c->world == 1) return verdict.ok() ? IMM3_OK : fail(verdict.rc, verdict.why);
    const int rrc = rccl_ready();
    if (rrc) return rrc; // (no RCCL in this process: no rank of this process can be inside the collective either)
    // The communicator's word and the communicator itself may still be in use by an imm3_comm_allreduce_count on the
    // communicator's own stream: the merge's collectives run on the context's stream, behind that one.
    if (c->in_flight) HIPCHK(hipStreamWaitEvent(s, c->ev_done, 0));
    unsigned long long shape[kMergeVoteWords];
    merge_vote_pack(v0, v1, !verdict.ok(), shape); // (a failed rank does not vote on the shape)
    HIPCHK(hipMemcpyAsync(c->d_slot, shape, sizeof(shape), hipMemcpyHostToDevice, s));
    NCCLCHK(g_rccl.AllReduce(c->d_slot, c->d_slot, kMergeVoteWords, ncclUint64, ncclMax, c->nccl, s));
    HIPCHK(hipMemcpyAsync(shape, c->d_slot, sizeof(shape), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    switch (merge_vote_read(shape, !verdict.ok())) {
    case MERGE_VOTE_OWN_ERROR: return fail(verdict.rc, verdict.why);
    case MERGE_VOTE_OTHER_FAILED: return fail(IMM3_ERR_STATE, "another rank failed before the merge (its call says why); no rank has merged anything");
    case MERGE_VOTE_DIFFER: return fail(IMM3_ERR_ARG, differ_message); // (max != min: every rank sees it and leaves here)
    case MERGE_VOTE_AGREE: break;
    }
    return IMM3_OK;
}

int merge_max_word(imm3_comm *c, hipStream_t s, unsigned long long mine, unsigned long long *most) {
    HIPCHK(hipMemcpyAsync(c->d_slot, &mine, sizeof(mine), hipMemcpyHostToDevice, s));
    NCCLCHK(g_rccl.AllReduce(c->d_slot, c->d_slot, 1, ncclUint64, ncclMax, c->nccl, s));
    HIPCHK(hipMemcpyAsync(most, c->d_slot, sizeof(*most), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return IMM3_OK;
}

int merge_list_length(imm3_comm *c, hipStream_t s, const LocalStep &step, unsigned long long mine, const char *other_rank_message, unsigned long long *most) {
    const int rc = merge_max_word(c, s, step.ok ? mine : ~0ULL, most);
    if (rc) return rc;
    if (*most == ~0ULL) return fail(IMM3_ERR_DEVICE, step.ok ? std::string(other_rank_message) : step.why + "; no rank has merged anything");
    return IMM3_OK;
}

int merge_exchange_alloc(imm3_comm *c, hipStream_t s, size_t bytes, DeviceBlock &block) {
    unsigned long long any = 0;
    const int rc = merge_max_word(c, s, block.alloc(bytes) == hipSuccess ? 0ULL : 1ULL, &any);
    if (rc) return rc;
    if (any) return fail(IMM3_ERR_DEVICE, "a rank could not allocate the exchange buffers of the merge; no rank has merged anything");
    return IMM3_OK;
}

int merge_gather(imm3_comm *c, hipStream_t s, void *d_send, void *d_recv, size_t slot_u64, const unsigned long long *length_word, const void *d_list,
                 size_t list_bytes) {
    HIPCHK(hipMemsetAsync(d_send, 0, slot_u64 * sizeof(unsigned long long), s)); // (padding behind this rank's list: entries of count 0)
    uint8_t *at = (uint8_t *)d_send;
    if (length_word) {
        HIPCHK(hipMemcpyAsync(at, length_word, sizeof(*length_word), hipMemcpyHostToDevice, s));
        at += sizeof(*length_word);
    }
    if (list_bytes) HIPCHK(hipMemcpyAsync(at, d_list, list_bytes, hipMemcpyDeviceToDevice, s));
    NCCLCHK(g_rccl.AllGather(d_send, d_recv, slot_u64, ncclUint64, c->nccl, s));
    return IMM3_OK;
}

} // namespace imm3
