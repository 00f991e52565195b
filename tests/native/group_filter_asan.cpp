// The program of imm3_query_set_group_filter on its own (immutable3_amd/csrc/imm3_group_filter_plan.{h,cpp}), for a build under
// -fsanitize=address,undefined: tests/test_group_filter_host.py compiles this file together with the checks (and imm3_expr_norm.cpp,
// whose expr_check_program they call) and runs it.  No device and no query handle: the checks take plain values, and the evaluator
// here is the one the kernels run (group_filter_eval, plain inline under g++).  10 000 random trees -- up to 8 leaves, up to 32 program
// entries, with NOTs -- over random (count, vals) are held against a recursive evaluation of the tree; then the overflow edge of the
// average and a few refused calls.  Prints one line per part; exits non-zero on the first disagreement.
#include "../../immutable3_amd/csrc/imm3_group_filter_plan.h"

#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

static std::string g_error;
namespace imm3 {
int fail(int code, const std::string &msg) {
    g_error = msg;
    return code;
}
} // namespace imm3
using namespace imm3;

typedef imm3_group_filter_leaf L;
static const int32_t kAggKind[4] = {IMM3_AGG_COUNT, IMM3_AGG_MIN, IMM3_AGG_MAX, IMM3_AGG_SUM};
static const int32_t kColKind[4] = {0, 0, 1, 0};
static GroupOrderShape shape() {
    GroupOrderShape s;
    std::memset(&s, 0, sizeof(s));
    s.is_agg = 1;
    s.n_aggs = 4;
    s.agg_kind = kAggKind;
    s.agg_col_kind = kColKind;
    return s;
}

struct Node {
    int32_t op; // >= 0: a leaf; IMM3_EXPR_AND / _OR / _NOT
    int l, r;
};
struct Tree {
    std::vector<Node> nodes;
    std::vector<int32_t> prog;
};
static int gen(Tree &t, std::mt19937_64 &rng, int n_leaves, int depth) {
    const int pick = depth >= 5 ? 0 : (int)(rng() % 10);
    Node n{0, -1, -1};
    if (pick < 3) n.op = (int32_t)(rng() % (uint64_t)n_leaves);
    else if (pick < 5) { n.op = IMM3_EXPR_NOT; n.l = gen(t, rng, n_leaves, depth + 1); }
    else { n.op = pick < 8 ? IMM3_EXPR_AND : IMM3_EXPR_OR; n.l = gen(t, rng, n_leaves, depth + 1); n.r = gen(t, rng, n_leaves, depth + 1); }
    t.prog.push_back(n.op); // (postfix: the operands are already there)
    t.nodes.push_back(n);
    return (int)t.nodes.size() - 1;
}
// exact, in __int128: what the leaf means
static bool leaf_truth(const L &l, unsigned long long count, const int64_t *vals) {
    __int128 lhs, rhs = l.value;
    if (l.agg == IMM3_GROUP_FILTER_COUNT || kAggKind[l.agg] == IMM3_AGG_COUNT) lhs = (__int128)count;
    else {
        lhs = vals[l.agg];
        if (l.average) rhs = (__int128)l.value * (__int128)count;
    }
    return l.cond == IMM3_GT ? lhs > rhs : (l.cond == IMM3_LT ? lhs < rhs : lhs == rhs);
}
static bool truth(const Tree &t, int at, const std::vector<L> &leaves, unsigned long long count, const int64_t *vals) {
    const Node &n = t.nodes[(size_t)at];
    if (n.op >= 0) return leaf_truth(leaves[(size_t)n.op], count, vals);
    if (n.op == IMM3_EXPR_NOT) return !truth(t, n.l, leaves, count, vals);
    const bool a = truth(t, n.l, leaves, count, vals), b = truth(t, n.r, leaves, count, vals);
    return n.op == IMM3_EXPR_AND ? (a && b) : (a || b);
}

int main() {
    std::mt19937_64 rng(20261020);
    const int conds[3] = {IMM3_GT, IMM3_LT, IMM3_EQ};
    int done = 0, with_not = 0, longest = 0;
    while (done < 10000) {
        const int n_leaves = 1 + (int)(rng() % IMM3_GROUP_FILTER_MAX_LEAVES);
        std::vector<L> leaves((size_t)n_leaves); // (heap, exactly n_leaves: a read past them is the sanitizer's)
        for (auto &l : leaves) {
            const int a = (int)(rng() % 5) - 1; // -1 = IMM3_GROUP_FILTER_COUNT, 0 .. 3
            l.agg = a;
            l.average = a == 3 && (rng() & 1) ? 1 : 0;
            l.cond = conds[rng() % 3];
            l.value = (int64_t)(rng() % 41) - 20;
        }
        Tree t;
        const int root = gen(t, rng, n_leaves, 0);
        if ((int)t.prog.size() > IMM3_GROUP_FILTER_MAX_PROG) continue;
        std::vector<int32_t> prog(t.prog); // (heap, exactly n_prog)
        GroupFilterProg fp;
        std::memset(&fp, 0x5A, sizeof(fp));
        const int rc = group_filter_plan(shape(), leaves.data(), n_leaves, prog.data(), (int32_t)prog.size(), &fp);
        if (rc != IMM3_OK) { std::printf("program %d refused: %s\n", done, g_error.c_str()); return 1; }
        for (int g = 0; g < 8; ++g) {
            const unsigned long long count = 1 + rng() % 30;
            int64_t vals[4];
            for (auto &v : vals) v = (int64_t)(rng() % 801) - 400;
            const bool got = group_filter_eval(fp, count, vals), want = truth(t, root, leaves, count, vals);
            if (got != want) { std::printf("program %d group %d: got %d want %d\n", done, g, (int)got, (int)want); return 1; }
        }
        for (int32_t op : prog) if (op == IMM3_EXPR_NOT) { ++with_not; break; }
        if ((int)prog.size() > longest) longest = (int)prog.size();
        ++done;
    }
    std::printf("%d programs ok (%d with a NOT, longest %d)\n", done, with_not, longest);
    if (with_not < 1000 || longest != IMM3_GROUP_FILTER_MAX_PROG) return 1;

    // the average: negative sums (no division, no rounding) and the product at the int64 edge
    struct Edge { int64_t sum; unsigned long long count; int cond; int64_t value; bool want; };
    const int64_t lo = -(int64_t)2147483648LL, hi = 2147483647LL;
    const unsigned long long cmax = 4294967295ULL;
    const Edge edges[] = {
        {-7, 2, IMM3_GT, -4, true}, {-7, 2, IMM3_LT, -3, true}, {-7, 2, IMM3_EQ, -3, false}, {-7, 2, IMM3_EQ, -4, false}, {-8, 2, IMM3_EQ, -4, true},
        {7, 2, IMM3_GT, 3, true}, {7, 2, IMM3_LT, 4, true}, {7, 2, IMM3_EQ, 3, false},
        {lo * (int64_t)cmax, cmax, IMM3_EQ, lo, true}, {lo * (int64_t)cmax + 1, cmax, IMM3_GT, lo, true}, {lo * (int64_t)cmax - 1, cmax, IMM3_LT, lo, true},
        {hi * (int64_t)cmax, cmax, IMM3_EQ, hi, true}, {hi * (int64_t)cmax - 1, cmax, IMM3_LT, hi, true}, {INT64_MAX, cmax, IMM3_GT, hi, true},
        {INT64_MIN, cmax, IMM3_LT, lo, true}, {INT64_MIN, 1, IMM3_LT, lo, true}, {INT64_MAX, 1, IMM3_GT, hi, true},
    };
    int n_edges = 0;
    for (const Edge &e : edges) {
        std::vector<L> leaf(1);
        leaf[0] = L{3, 1, e.cond, e.value};
        std::vector<int32_t> prog(1, 0);
        GroupFilterProg fp;
        if (group_filter_plan(shape(), leaf.data(), 1, prog.data(), 1, &fp) != IMM3_OK) { std::printf("edge %d refused: %s\n", n_edges, g_error.c_str()); return 1; }
        const int64_t vals[4] = {0, 0, 0, e.sum};
        const bool got = group_filter_eval(fp, e.count, vals);
        if (got != e.want || got != leaf_truth(leaf[0], e.count, vals)) { std::printf("edge %d: got %d want %d\n", n_edges, (int)got, (int)e.want); return 1; }
        ++n_edges;
    }
    std::printf("%d average edges ok\n", n_edges);

    // refused calls leave a zeroed program behind and name their cause
    struct Bad { L leaf; int32_t n_leaves; std::vector<int32_t> prog; const char *frag; };
    const Bad bads[] = {
        {L{3, 1, IMM3_GT, hi + 1}, 1, {0}, "[-2^31, 2^31 - 1]"}, {L{3, 1, IMM3_GT, lo - 1}, 1, {0}, "[-2^31, 2^31 - 1]"},
        {L{1, 1, IMM3_GT, 0}, 1, {0}, "average is for a SUM aggregate only"}, {L{4, 0, IMM3_GT, 0}, 1, {0}, "names aggregate 4 of 4"},
        {L{0, 0, IMM3_MATCH, 0}, 1, {0}, "unknown cond"}, {L{0, 0, IMM3_GT, 0}, 1, {0, IMM3_EXPR_AND}, "stack underflow"},
        {L{0, 0, IMM3_GT, 0}, 1, {0, 0}, "more than one result"}, {L{0, 0, IMM3_GT, 0}, 1, {0, -3}, "unknown operator"},
        {L{0, 0, IMM3_GT, 0}, 1, {1}, "leaf index out of range"}, {L{0, 0, IMM3_GT, 0}, 9, {0}, "n_leaves must be 0 .. 8"},
        {L{0, 0, IMM3_GT, 0}, 1, {}, "empty, but leaves were given"},
    };
    int n_bad = 0;
    for (const Bad &b : bads) {
        std::vector<L> leaves((size_t)b.n_leaves, b.leaf);
        std::vector<int32_t> prog(b.prog);
        GroupFilterProg fp;
        std::memset(&fp, 0x5A, sizeof(fp));
        g_error.clear();
        const int rc = group_filter_plan(shape(), leaves.data(), b.n_leaves, prog.empty() ? nullptr : prog.data(), (int32_t)prog.size(), &fp);
        if (rc != IMM3_ERR_ARG || g_error.find(b.frag) == std::string::npos || fp.n_prog != 0) { std::printf("refusal %d: rc %d, %s\n", n_bad, rc, g_error.c_str()); return 1; }
        ++n_bad;
    }
    GroupFilterProg none;
    std::memset(&none, 0x5A, sizeof(none));
    if (group_filter_plan(shape(), nullptr, 0, nullptr, 0, &none) != IMM3_OK || none.n_prog != 0 || !group_filter_eval(none, 1ULL, (const int64_t *)nullptr)) return 1;
    std::printf("%d refusals ok, removal ok\n", n_bad);
    return 0;
}
