// The arithmetic of the merges' shape vote (immutable3_amd/csrc/imm3_merge_vote.h) on its own, for a build under
// -fsanitize=address,undefined: tests/test_merge_vote_host.py compiles this file and runs it.  No device and no other part of the
// library.  The all-reduce(max) the ranks' words go through is simulated element-wise over 2 and 3 ranks; every rank then reads the
// reduced words and must come to the verdict the protocol promises.  Prints one line per check; exits non-zero when one fails.
#include "../../immutable3_amd/csrc/imm3_merge_vote.h"

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

using namespace imm3;

static int bad = 0;
static void check(const std::string &what, bool ok) {
    std::printf("%-72s %s\n", what.c_str(), ok ? "ok" : "FAILED");
    if (!ok) ++bad;
}

struct Rank {
    unsigned long long v0, v1;
    bool failed;
    MergeVoteResult want;
};

// every rank packs, the words meet in max, every rank reads
static void vote_case(const std::string &what, const std::vector<Rank> &ranks) {
    std::vector<std::vector<unsigned long long>> sent;
    for (const Rank &r : ranks) { // (each rank's words in a heap buffer of exactly five: a write past them is a sanitizer finding)
        sent.emplace_back((size_t)kMergeVoteWords);
        merge_vote_pack(r.v0, r.v1, r.failed, sent.back().data());
    }
    std::vector<unsigned long long> reduced((size_t)kMergeVoteWords, 0ULL);
    for (const auto &w : sent)
        for (int i = 0; i < kMergeVoteWords; ++i) reduced[(size_t)i] = std::max(reduced[(size_t)i], w[(size_t)i]);
    bool ok = true;
    for (const Rank &r : ranks) ok = ok && merge_vote_read(reduced.data(), r.failed) == r.want;
    check(what + ", " + std::to_string(ranks.size()) + " ranks", ok);
}

int main() {
    const unsigned long long ONES = ~0ULL, A = 0x0000000411000511ULL, B = 0x0010001000000010ULL;
    const MergeVoteResult AGREE = MERGE_VOTE_AGREE, OWN = MERGE_VOTE_OWN_ERROR, OTHER = MERGE_VOTE_OTHER_FAILED, DIFFER = MERGE_VOTE_DIFFER;
    {   // what a rank sends
        unsigned long long w[kMergeVoteWords];
        merge_vote_pack(A, B, false, w);
        check("a rank sends its words, their complements and no flag", w[0] == A && w[1] == B && w[2] == ~A && w[3] == ~B && w[4] == 0);
        merge_vote_pack(A, B, true, w);
        check("a failed rank sends zeros and the flag", w[0] == 0 && w[1] == 0 && w[2] == 0 && w[3] == 0 && w[4] == 1);
    }
    for (int world = 2; world <= 3; ++world) {
        const size_t n = (size_t)world;
        vote_case("all agree", std::vector<Rank>(n, Rank{A, B, false, AGREE}));
        {
            std::vector<Rank> r(n, Rank{A, B, false, DIFFER});
            r[n - 1].v0 = A + 1;
            vote_case("word 0 differs on one rank, word 1 agrees", r);
            r[n - 1].v0 = A - 1; // (below the others: only the complement's max shows it)
            vote_case("word 0 is smaller on one rank", r);
        }
        {
            std::vector<Rank> r(n, Rank{A, B, false, DIFFER});
            r[0].v1 = B ^ (1ULL << 63);
            vote_case("word 1 differs on one rank, word 0 agrees", r);
        }
        vote_case("the words 0 and ~0 on every rank agree", std::vector<Rank>(n, Rank{0ULL, ONES, false, AGREE}));
        {
            std::vector<Rank> r(n, Rank{0ULL, ONES, false, DIFFER});
            r[n - 1].v0 = ONES;
            vote_case("0 against ~0 in word 0", r);
            r[n - 1].v0 = 0ULL;
            r[n - 1].v1 = 0ULL;
            vote_case("~0 against 0 in word 1", r);
        }
        {
            std::vector<Rank> r(n, Rank{A, B, false, OTHER});
            r[0] = Rank{B, A, true, OWN}; // (its own words would disagree: it does not vote)
            vote_case("one failed rank reads its own error, the others that a rank failed", r);
            r[n - 1].v0 = A + 1;          // the well ranks (or the well rank and the failed one's words) disagree as well
            r[n - 1].v1 = 0ULL;
            vote_case("... and that is reported before any disagreement", r);
        }
        vote_case("all ranks failed: each reads its own error", std::vector<Rank>(n, Rank{A, B, true, OWN}));
    }
    {   // a zero vote of well ranks is not mistaken for the zeros of a failed one
        std::vector<Rank> r(3, Rank{0ULL, 0ULL, false, OTHER});
        r[1] = Rank{0ULL, 0ULL, true, OWN};
        vote_case("well ranks voting (0, 0) beside a failed rank", r);
        vote_case("well ranks voting (0, 0)", std::vector<Rank>(3, Rank{0ULL, 0ULL, false, AGREE}));
    }
    return bad ? 1 : 0;
}
