// imm3_merge_vote.h -- the arithmetic of the merges' shape vote, host only (no HIP include, so it builds and runs alone:
// tests/native/merge_vote_asan.cpp).  The collective around it is merge_vote (imm3_merge_protocol.cpp).
//
// Every rank brings two words that must be the same on all ranks (what they mean is the caller's: key width and aggregates, a
// hash of the SELECT list ...) and whether it has failed on its own.  The five words {v0, v1, ~v0, ~v1, failed} go through ONE
// all-reduce(max): the max of a complement is the complement of the min, so max == min -- all ranks agree -- shows as
// w[0] == ~w[2] and w[1] == ~w[3], and w[4] says whether any rank has failed.  A failed rank sends zeros in the first four words:
// they are the identity of max, so its (meaningless) shape neither makes the others disagree nor hides that they do.
#ifndef IMM3_MERGE_VOTE_H
#define IMM3_MERGE_VOTE_H

namespace imm3 {

constexpr int kMergeVoteWords = 5;

enum MergeVoteResult {
    MERGE_VOTE_AGREE = 0,
    MERGE_VOTE_OWN_ERROR,    // this rank failed before the vote: it reports its own error whatever the others sent
    MERGE_VOTE_OTHER_FAILED, // another rank did: reported before any disagreement (a failed rank has not voted)
    MERGE_VOTE_DIFFER,       // nobody failed and the ranks' words differ
};

// the words this rank sends
inline void merge_vote_pack(unsigned long long v0, unsigned long long v1, bool failed, unsigned long long w[kMergeVoteWords]) {
    w[0] = failed ? 0ULL : v0;
    w[1] = failed ? 0ULL : v1;
    w[2] = failed ? 0ULL : ~v0;
    w[3] = failed ? 0ULL : ~v1;
    w[4] = failed ? 1ULL : 0ULL;
}

// what this rank reads from the reduced words; the order of the tests is the order of the verdicts on every rank
inline MergeVoteResult merge_vote_read(const unsigned long long w[kMergeVoteWords], bool failed) {
    if (failed) return MERGE_VOTE_OWN_ERROR;
    if (w[4]) return MERGE_VOTE_OTHER_FAILED;
    if (w[0] != ~w[2] || w[1] != ~w[3]) return MERGE_VOTE_DIFFER;
    return MERGE_VOTE_AGREE;
}

} // namespace imm3
#endif
