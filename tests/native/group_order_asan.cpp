// The argument checks and the key layout of imm3_query_set_group_order (immutable3_amd/csrc/imm3_group_order_plan.cpp) on their own, for a
// build under -fsanitize=address,undefined: tests/test_group_order_host.py compiles this file together with the checks and runs it.  The
// query handle is a stub -- the plain values the checks take: the group columns' kinds and widths, the aggregates' kinds and their
// columns' kinds and widths -- so no device and no other part of the library is needed; the one function the checks take from the rest
// (imm3::fail) is defined here.  Prints one line per case; exits non-zero when a status or a layout is not the expected one.
#include "../../immutable3_amd/csrc/imm3_group_order_plan.h"

#include <cstdio>
#include <cstring>
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

struct StubQuery { // what the checks read of a query handle; every array is a heap allocation of exactly its length
    bool is_agg = true;
    std::vector<int32_t> group_kind, group_width, agg_kind, agg_col_kind, agg_col_width;
    GroupOrderShape shape() const {
        GroupOrderShape s;
        s.is_agg = is_agg ? 1 : 0;
        s.n_group = (int32_t)group_kind.size();
        s.n_aggs = (int32_t)agg_kind.size();
        s.group_kind = group_kind.data();
        s.group_width = group_width.data();
        s.agg_kind = agg_kind.data();
        s.agg_col_kind = agg_col_kind.data();
        s.agg_col_width = agg_col_width.data();
        return s;
    }
};

static int bad = 0;
typedef imm3_group_order_key K;
// want_bytes: the user's key bytes of an accepted call (-1: do not check)
static GroupOrderLayout expect(const char *what, const StubQuery &q, const std::vector<K> &keys, int32_t n_keys, int want, int want_bytes = -1, const char *frag = "") {
    std::vector<K> exact(keys.begin(), keys.begin() + (n_keys > 0 && (size_t)n_keys <= keys.size() ? n_keys : 0));
    GroupOrderLayout l;
    std::memset(&l, 0x5A, sizeof(l));
    g_error.clear();
    const int rc = group_order_plan(q.shape(), exact.empty() ? nullptr : exact.data(), n_keys, &l);
    bool ok = rc == want && (rc == IMM3_OK || (!g_error.empty() && g_error.find(frag) != std::string::npos));
    if (rc == IMM3_OK && n_keys > 0)
        ok = ok && l.n_keys == n_keys && (want_bytes < 0 || l.user_bytes == want_bytes) && l.key_bytes == l.user_bytes + 4 && l.key_words == (l.key_bytes + 3) / 4 &&
             l.key_bytes >= 5 && l.key_bytes <= 16;
    if (rc == IMM3_OK && n_keys == 0) ok = ok && l.n_keys == 0 && l.key_bytes == 0;
    std::printf("%-52s %d %d %s%s\n", what, rc, rc == IMM3_OK ? l.user_bytes : -1, g_error.c_str(), ok ? " ok" : " WRONG");
    if (!ok) ++bad;
    return l;
}

int main() {
    const int I32 = 0, I8 = 1, STR = 2;
    StubQuery q; // group by (id int32, age int8, state string(2), name string(12)); count(id), min(id), max(age), sum(id)
    q.group_kind = {I32, I8, STR, STR};
    q.group_width = {4, 1, 2, 12};
    q.agg_kind = {IMM3_AGG_COUNT, IMM3_AGG_MIN, IMM3_AGG_MAX, IMM3_AGG_SUM};
    q.agg_col_kind = {I32, I32, I8, I32};
    q.agg_col_width = {4, 4, 1, 4};
    const int G = IMM3_GROUP_ORDER_GROUP_COL, A = IMM3_GROUP_ORDER_AGG;

    // every kind / width combination, one key each: source, width and offset
    struct { const char *what; K key; int src, width, at; } one[] = {
        {"group column int32", {G, 0, 0}, GO_KEY_I32, 4, 0},       {"group column int8", {G, 1, 1}, GO_KEY_I8, 1, 4},
        {"group column string(2)", {G, 2, 0}, GO_KEY_STR, 2, 5},   {"group column string(12)", {G, 3, 1}, GO_KEY_STR, 12, 7},
        {"count", {A, 0, 1}, GO_COUNT, 5, 0},                      {"min on int32", {A, 1, 0}, GO_VAL_I32, 4, 1},
        {"max on int8", {A, 2, 1}, GO_VAL_I8, 1, 2},               {"sum", {A, 3, 0}, GO_SUM, 8, 3},
    };
    for (const auto &c : one) {
        const GroupOrderLayout l = expect(c.what, q, {c.key}, 1, IMM3_OK, c.width);
        if (l.k[0].src != c.src || l.k[0].width != c.width || l.k[0].at != c.at || l.k[0].descending != (c.key.descending ? 1 : 0)) {
            std::printf("  layout of %s WRONG: src %d width %d at %d\n", c.what, l.k[0].src, l.k[0].width, l.k[0].at);
            ++bad;
        }
    }
    for (int w = 1; w <= 16; ++w) { // MAX over a string of every width up to 16, and a string group column of that width
        StubQuery s;
        s.group_kind = {STR};
        s.group_width = {w};
        s.agg_kind = {IMM3_AGG_MAX};
        s.agg_col_kind = {STR};
        s.agg_col_width = {w};
        const std::string name = "string max / group column of " + std::to_string(w) + " bytes";
        const int want = w <= IMM3_GROUP_ORDER_KEY_MAX_WIDTH ? IMM3_OK : IMM3_ERR_ARG;
        const GroupOrderLayout l = expect(name.c_str(), s, {K{A, 0, 0}}, 1, want, w, "bytes wide, more than 12");
        if (want == IMM3_OK && (l.k[0].src != (w <= 8 ? GO_VAL_STR : GO_WIDE_STR) || l.k[0].width != w)) ++bad;
        expect(name.c_str(), s, {K{G, 0, 1}}, 1, want, w, "bytes wide, more than 12");
    }
    expect("four keys, 12 bytes", q, {K{G, 0, 0}, K{A, 0, 1}, K{G, 2, 0}, K{A, 2, 1}}, 4, IMM3_OK, 12);
    expect("sum + min, 12 bytes", q, {K{A, 3, 1}, K{A, 1, 0}}, 2, IMM3_OK, 12);
    expect("sum + count, 13 bytes", q, {K{A, 3, 1}, K{A, 0, 0}}, 2, IMM3_ERR_ARG, -1, "13 bytes wide together, more than 12");
    expect("string(12) + int8 group columns", q, {K{G, 3, 0}, K{G, 1, 0}}, 2, IMM3_ERR_ARG, -1, "13 bytes wide together");
    expect("no key: the order is removed", q, {}, 0, IMM3_OK);
    expect("negative n_keys", q, {}, -1, IMM3_ERR_ARG, -1, "n_keys must be 0 .. 4");
    expect("five keys", q, {K{G, 0, 0}, K{G, 1, 0}, K{G, 2, 0}, K{A, 0, 0}, K{A, 1, 0}}, 5, IMM3_ERR_ARG, -1, "n_keys must be 0 .. 4");
    expect("null keys", q, {}, 2, IMM3_ERR_ARG, -1, "keys is null");
    expect("unknown kind", q, {K{2, 0, 0}}, 1, IMM3_ERR_ARG, -1, "unknown kind 2");
    expect("negative kind", q, {K{-1, 0, 0}}, 1, IMM3_ERR_ARG, -1, "unknown kind -1");
    expect("group column == n_group", q, {K{G, 4, 0}}, 1, IMM3_ERR_ARG, -1, "names group column 4 of 4");
    expect("group column < 0", q, {K{G, -1, 0}}, 1, IMM3_ERR_ARG, -1, "names group column -1 of 4");
    expect("group column INT32_MAX", q, {K{G, INT32_MAX, 0}}, 1, IMM3_ERR_ARG, -1, "names group column");
    expect("aggregate == n_aggs", q, {K{A, 4, 0}}, 1, IMM3_ERR_ARG, -1, "names aggregate 4 of 4");
    expect("aggregate INT32_MIN", q, {K{A, INT32_MIN, 1}}, 1, IMM3_ERR_ARG, -1, "names aggregate");
    expect("the same group column twice", q, {K{G, 1, 0}, K{A, 0, 0}, K{G, 1, 1}}, 3, IMM3_ERR_ARG, -1, "group column 1 is an order key twice");
    expect("the same aggregate twice", q, {K{A, 2, 0}, K{A, 2, 0}}, 2, IMM3_ERR_ARG, -1, "aggregate 2 is an order key twice");
    expect("group column 0 and aggregate 0", q, {K{G, 0, 0}, K{A, 0, 0}}, 2, IMM3_OK, 9);
    StubQuery proj;
    proj.is_agg = false;
    expect("not an aggregation", proj, {K{G, 0, 0}}, 1, IMM3_ERR_ARG, -1, "not an aggregation query");
    expect("not an aggregation, no key", proj, {}, 0, IMM3_ERR_ARG, -1, "not an aggregation query");
    StubQuery none; // an aggregation without group columns: count(*) alone
    none.agg_kind = {IMM3_AGG_COUNT};
    none.agg_col_kind = {I32};
    none.agg_col_width = {4};
    expect("no group column: an aggregate key", none, {K{A, 0, 1}}, 1, IMM3_OK, 5);
    expect("no group column: a group key", none, {K{G, 0, 0}}, 1, IMM3_ERR_ARG, -1, "names group column 0 of 0");
    return bad ? 1 : 0;
}
