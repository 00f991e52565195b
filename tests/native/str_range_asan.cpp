// The host logic of IMM3_STR_RANGE (immutable3_amd/csrc/imm3_str_range.cpp) on its own, for a build under -fsanitize=address,undefined:
// tests/test_str_range_host.py compiles this file together with that unit and runs it.  Every buffer handed in is an allocation of
// exactly the bytes it should hold, so a read or write past a bound, a column or a blob is a sanitizer finding.  The one function the
// unit takes from the rest of the library (imm3::fail) is defined here.  Prints one line per check; exits non-zero when one fails.
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
int str_range_check_leaf(int32_t n_match, const uint8_t *bytes, const int32_t *lens, int32_t width);
void str_range_pad(const uint8_t *lo, int32_t lo_len, const uint8_t *hi, int32_t hi_len, int32_t width, std::string &lo_out, std::string &hi_out);
bool str_range_empty(const std::string &lo, const std::string &hi);
bool str_range_full(const std::string &lo, const std::string &hi);
bool str_range_holds(const std::string &lo, const std::string &hi, const std::string &v);
void str_range_intersect(std::string &lo, std::string &hi, const std::string &lo2, const std::string &hi2);
void str_range_filter_match(const std::string &lo, const std::string &hi, std::vector<std::string> &match);
bool str_range_successor(std::string &v);
bool str_range_predecessor(std::string &v);
int str_range_route(int32_t width);
void str_range_pack(const std::string &lo, const std::string &hi, std::vector<uint8_t> &blob, uint32_t lo4[4], uint32_t hi4[4]);
} // namespace imm3
using namespace imm3;

static int bad = 0;
static void expect(const char *what, bool ok) {
    std::printf("%-64s %s\n", what, ok ? "ok" : "FAILED");
    if (!ok) ++bad;
}
static std::string S(std::initializer_list<int> b) {
    std::string s;
    for (int x : b) s += (char)x;
    return s;
}
// the padded bounds of (lo, hi) on a column of `width` bytes, the bounds handed over in allocations of exactly their lengths
static void padded(const std::string &lo, const std::string &hi, int width, std::string &plo, std::string &phi) {
    std::vector<uint8_t> a(lo.begin(), lo.end()), b(hi.begin(), hi.end());
    str_range_pad(a.empty() ? nullptr : a.data(), (int32_t)a.size(), b.empty() ? nullptr : b.data(), (int32_t)b.size(), width, plo, phi);
}

int main() {
    std::string lo, hi;
    // ---- padding ----
    padded("Jo", "Jo", 6, lo, hi);
    expect("pad: lo with 00, hi with FF", lo == S({'J', 'o', 0, 0, 0, 0}) && hi == S({'J', 'o', 0xFF, 0xFF, 0xFF, 0xFF}));
    padded("", "", 4, lo, hi);
    expect("pad: bounds of length 0", lo == std::string(4, '\0') && hi == std::string(4, (char)0xFF) && str_range_full(lo, hi) && !str_range_empty(lo, hi));
    padded("abcd", "abcd", 4, lo, hi);
    expect("pad: bounds of length width", lo == "abcd" && hi == "abcd" && !str_range_full(lo, hi) && !str_range_empty(lo, hi));
    padded(std::string(256, 'x'), "", 256, lo, hi);
    expect("pad: width 256", lo.size() == 256 && hi.size() == 256 && lo == std::string(256, 'x') && hi == std::string(256, (char)0xFF));
    // ---- empty and full ----
    padded("M", "", 3, lo, hi);
    expect("from M on: neither empty nor full", !str_range_empty(lo, hi) && !str_range_full(lo, hi));
    expect("from M on holds M00 and FFFFFF, not L..", str_range_holds(lo, hi, S({'M', 0, 0})) && str_range_holds(lo, hi, S({0xFF, 0xFF, 0xFF})) && !str_range_holds(lo, hi, S({'L', 0xFF, 0xFF})));
    padded("b", "a", 3, lo, hi);
    expect("lo' > hi' is empty", str_range_empty(lo, hi));
    padded(S({0x80}), S({0x7F}), 2, lo, hi);
    expect("80 > 7F: unsigned order", str_range_empty(lo, hi));
    padded(S({0x7F}), S({0x80}), 2, lo, hi);
    expect("7F .. 80 holds 7F00, 80FF, not 8100", !str_range_empty(lo, hi) && str_range_holds(lo, hi, S({0x7F, 0})) && str_range_holds(lo, hi, S({0x80, 0xFF})) && !str_range_holds(lo, hi, S({0x81, 0})));
    padded("a", "a", 2, lo, hi);
    expect("a value of another length is never held", !str_range_holds(lo, hi, "a") && !str_range_holds(lo, hi, "abc"));
    // ---- intersection ----
    std::string l2, h2;
    padded("b", "x", 4, lo, hi);
    padded("f", "", 4, l2, h2);
    str_range_intersect(lo, hi, l2, h2);
    expect("intersect: max of the los, min of the his", lo == S({'f', 0, 0, 0}) && hi == S({'x', 0xFF, 0xFF, 0xFF}));
    padded("a", "c", 4, lo, hi);
    padded("d", "e", 4, l2, h2);
    str_range_intersect(lo, hi, l2, h2);
    expect("intersect: ranges that do not meet are empty", str_range_empty(lo, hi));
    padded("", "", 4, lo, hi);
    padded("", "", 4, l2, h2);
    str_range_intersect(lo, hi, l2, h2);
    expect("intersect: full and full is full", str_range_full(lo, hi));
    // ---- range and Match ----
    padded("b", "d", 2, lo, hi);
    std::vector<std::string> list = {"zz", "b", S({'b', 0}), S({'d', 0xFF}), "cc", S({'a', 0xFF}), S({'e', 0}), "c"};
    str_range_filter_match(lo, hi, list);
    expect("Range and Match: the values inside, in the list's order", list == std::vector<std::string>({S({'b', 0}), S({'d', 0xFF}), "cc"}));
    list.clear();
    str_range_filter_match(lo, hi, list);
    expect("Range and an empty IN-list", list.empty());
    // ---- successor and predecessor ----
    std::string v = S({'m', 0x00, 0xFF, 0xFF, 0xFF, 0xFF});
    expect("successor carries across a dword boundary", str_range_successor(v) && v == S({'m', 0x01, 0, 0, 0, 0}));
    expect("predecessor borrows across it", str_range_predecessor(v) && v == S({'m', 0x00, 0xFF, 0xFF, 0xFF, 0xFF}));
    v = std::string(8, (char)0xFF);
    expect("no successor behind FF .. FF", !str_range_successor(v) && v == std::string(8, (char)0xFF));
    expect("predecessor of FF .. FF", str_range_predecessor(v) && v == std::string(7, (char)0xFF) + S({0xFE}));
    v = std::string(8, '\0');
    expect("no predecessor before 00 .. 00", !str_range_predecessor(v) && v == std::string(8, '\0'));
    expect("successor of 00 .. 00", str_range_successor(v) && v == std::string(7, '\0') + S({1}));
    v = std::string(255, (char)0xFF);
    v.insert(v.begin(), 'a');
    expect("successor, width 256: the carry runs through 255 bytes", str_range_successor(v) && v == "b" + std::string(255, '\0'));
    expect("predecessor, width 256", str_range_predecessor(v) && v == "a" + std::string(255, (char)0xFF));
    v.clear();
    expect("a column without bytes has neither", !str_range_successor(v) && !str_range_predecessor(v));
    // ---- the leaf's checks ----
    {
        std::vector<uint8_t> bytes = {'a', 'b', 'c'};
        std::vector<int32_t> lens = {1, 2};
        expect("leaf: two bounds", str_range_check_leaf(2, bytes.data(), lens.data(), 4) == IMM3_OK);
        expect("leaf: n_match 1", str_range_check_leaf(1, bytes.data(), lens.data(), 4) == IMM3_ERR_ARG && g_error.find("n_match") != std::string::npos);
        expect("leaf: n_match 3", str_range_check_leaf(3, bytes.data(), lens.data(), 4) == IMM3_ERR_ARG);
        expect("leaf: null lengths", str_range_check_leaf(2, bytes.data(), nullptr, 4) == IMM3_ERR_ARG && g_error.find("match_lens") != std::string::npos);
        expect("leaf: null bytes", str_range_check_leaf(2, nullptr, lens.data(), 4) == IMM3_ERR_ARG && g_error.find("match_bytes") != std::string::npos);
        expect("leaf: a bound longer than the column", str_range_check_leaf(2, bytes.data(), lens.data(), 1) == IMM3_ERR_ARG && g_error.find("longer") != std::string::npos);
        std::vector<int32_t> neg = {-1, 2}, zero = {0, 0};
        expect("leaf: negative length", str_range_check_leaf(2, bytes.data(), neg.data(), 4) == IMM3_ERR_ARG);
        expect("leaf: two empty bounds need no bytes", str_range_check_leaf(2, nullptr, zero.data(), 4) == IMM3_OK);
    }
    // ---- route and packing ----
    bool route_ok = str_range_route(0) == -1 && str_range_route(257) == -1 && str_range_route(-4) == -1;
    for (int w = 1; w <= 256; ++w) route_ok = route_ok && str_range_route(w) == (w % 4 == 0 ? 1 : 2);
    expect("route: the string pass for 4, 8, .. 256, the generic kernel else", route_ok);
    {
        std::vector<uint8_t> blob;
        uint32_t lo4[4], hi4[4];
        padded("ABCDEFGH", "ABCDEFGH", 8, lo, hi);
        str_range_pack(lo, hi, blob, lo4, hi4);
        expect("pack, width 8: bytes, then swapped dwords", blob.size() == 32 && std::memcmp(blob.data(), "ABCDEFGHABCDEFGH", 16) == 0 && lo4[0] == 0x41424344u &&
                                                                lo4[1] == 0x45464748u && hi4[1] == 0x45464748u && lo4[2] == 0 && hi4[3] == 0);
        uint32_t d0;
        std::memcpy(&d0, blob.data() + 16, 4);
        expect("pack, width 8: the tails start behind 2 x width bytes", d0 == 0x41424344u);
        padded("abc", "", 3, lo, hi);
        str_range_pack(lo, hi, blob, lo4, hi4);
        expect("pack, width 3: bytes only", blob.size() == 6 && blob[0] == 'a' && blob[3] == 0xFF && lo4[0] == 0);
        padded(std::string(256, 'q'), "", 256, lo, hi);
        str_range_pack(lo, hi, blob, lo4, hi4);
        expect("pack, width 256", blob.size() == 1024 && lo4[3] == 0x71717171u && hi4[0] == 0xFFFFFFFFu && blob[1023] == 0xFF && blob[512] == 'q');
    }
    return bad ? 1 : 0;
}
