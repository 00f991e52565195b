// The argument checks of imm3_query_set_order (immutable3_amd/csrc/imm3_order_args.cpp) on their own, for a build under
// -fsanitize=address,undefined: tests/test_order_host.py compiles this file together with the checks and runs it.  The query handle
// is a stub -- the plain values the checks take: SELECT-list widths, the creation-time limit, "has run", "is an aggregation" -- so no
// device and no other part of the library is needed; the one function the checks take from the rest (imm3::fail) is defined here.
// Prints one line per case, "<status> <key bytes>"; exits non-zero when a status is not the expected one.
#include "../../include/imm3.h"

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
int order_check_args(bool is_agg, int32_t n_proj, const int32_t *proj_widths, int64_t create_limit, bool has_run,
                     const imm3_order_key *keys, int32_t n_keys, int64_t limit, int32_t *key_bytes_out);
} // namespace imm3

struct StubQuery { // what the checks read of a query handle
    bool is_agg = false, has_run = false;
    int64_t create_limit = 0;
    std::vector<int32_t> widths; // exactly n_proj entries on the heap: a read past them is a sanitizer finding
};

static int bad = 0;
static void expect(const char *what, const StubQuery &q, const std::vector<imm3_order_key> &keys, int32_t n_keys, int64_t limit, int want) {
    // the keys are copied into an allocation of exactly n_keys entries (none at all when n_keys <= 0)
    std::vector<imm3_order_key> exact(keys.begin(), keys.begin() + (n_keys > 0 && (size_t)n_keys <= keys.size() ? n_keys : 0));
    int32_t bytes = -1;
    g_error.clear();
    const int rc = imm3::order_check_args(q.is_agg, (int32_t)q.widths.size(), q.widths.data(), q.create_limit, q.has_run,
                                          exact.empty() ? nullptr : exact.data(), n_keys, limit, &bytes);
    std::printf("%-44s %d %d %s\n", what, rc, bytes, g_error.c_str());
    if (rc != want || (rc != IMM3_OK && g_error.empty())) ++bad;
}

int main() {
    StubQuery q;
    q.widths = {4, 1, 2, 8, 4}; // id, age, state, an 8-byte string, another int
    const imm3_order_key k0{0, 0}, k1{1, 1}, k2{2, 0}, k3{3, 1}, k4{4, 0};
    expect("one key", q, {k0}, 1, 0, IMM3_OK);
    expect("four keys, 15 bytes", q, {k0, k1, k2, k3}, 4, 10, IMM3_OK);
    expect("four keys, 16 bytes", q, {k0, k4, k3}, 3, 0, IMM3_OK);
    expect("18 bytes", q, {k0, k2, k3, k4}, 4, 0, IMM3_ERR_ARG);
    expect("no key", q, {}, 0, 0, IMM3_ERR_ARG);
    expect("negative n_keys", q, {}, -3, 0, IMM3_ERR_ARG);
    expect("five keys", q, {k0, k1, k2, k3, k4}, 5, 0, IMM3_ERR_ARG);
    expect("null keys", q, {}, 2, 0, IMM3_ERR_ARG);
    expect("proj == n_proj", q, {imm3_order_key{5, 0}}, 1, 0, IMM3_ERR_ARG);
    expect("proj < 0", q, {imm3_order_key{-1, 0}}, 1, 0, IMM3_ERR_ARG);
    expect("proj = INT32_MAX", q, {imm3_order_key{INT32_MAX, 0}}, 1, 0, IMM3_ERR_ARG);
    expect("proj = INT32_MIN", q, {imm3_order_key{INT32_MIN, 1}}, 1, 0, IMM3_ERR_ARG);
    expect("repeated", q, {k1, k0, k1}, 3, 0, IMM3_ERR_ARG);
    expect("limit = INT64_MAX", q, {k0}, 1, INT64_MAX, IMM3_OK);
    expect("limit < 0", q, {k0}, 1, INT64_MIN, IMM3_OK);
    StubQuery lim = q;
    lim.create_limit = 10;
    expect("creation limit and order limit", lim, {k0}, 1, 5, IMM3_ERR_ARG);
    expect("creation limit, no order limit", lim, {k0}, 1, 0, IMM3_ERR_ARG);
    StubQuery ran = q;
    ran.has_run = true;
    expect("already run", ran, {k0}, 1, 0, IMM3_ERR_STATE);
    StubQuery agg = q;
    agg.is_agg = true;
    expect("aggregation", agg, {k0}, 1, 0, IMM3_ERR_ARG);
    StubQuery none;
    expect("no SELECT list", none, {k0}, 1, 0, IMM3_ERR_ARG);
    StubQuery wide;
    wide.widths = {32, 4};
    expect("one key column wider than 16 bytes", wide, {k0}, 1, 0, IMM3_ERR_ARG);
    return bad ? 1 : 0;
}
