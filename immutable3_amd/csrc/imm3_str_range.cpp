// imm3_str_range.cpp -- IMM3_STR_RANGE (include/imm3.h) on the host: the leaf's checks, the padded bounds, what leaves on one column
// fold to, the successor / predecessor the strict front-end forms are made of, and the bounds in the form the kernels read.  Pure
// code over plain values: no handle, no device.  imm3_expr_norm.cpp, imm3_api.cpp and imm3_planner.cpp call it;
// tests/native/str_range_asan.cpp builds it alone under the sanitizers.
// The order is the one of ORDER BY and the string MAX aggregate: unsigned, byte-wise, from the first byte -- std::string::compare
// over equal lengths (char_traits<char>::lt compares as unsigned char).
#include "../../include/imm3.h"

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace imm3 {
int fail(int code, const std::string &msg); // sets the calling thread's imm3_last_error() text

namespace {
bool bytes_less(const std::string &a, const std::string &b) { // equal lengths
    return std::memcmp(a.data(), b.data(), std::min(a.size(), b.size())) < 0;
}
} // namespace

// The leaf's own checks, in the order imm3.h lists them.  width <= 0: the column's width is not known (yet) and no length is held
// against it.
int str_range_check_leaf(int32_t n_match, const uint8_t *bytes, const int32_t *lens, int32_t width) {
    if (n_match != 2) return fail(IMM3_ERR_ARG, "StrRange takes exactly two bounds, lo and hi (n_match is " + std::to_string(n_match) + ", not 2)");
    if (!lens) return fail(IMM3_ERR_ARG, "StrRange without bounds: match_lens is null");
    for (int i = 0; i < 2; ++i) {
        if (lens[i] < 0) return fail(IMM3_ERR_ARG, std::string("StrRange: negative length of ") + (i ? "hi" : "lo"));
        if (width > 0 && lens[i] > width)
            return fail(IMM3_ERR_ARG, std::string("StrRange: ") + (i ? "hi" : "lo") + " is " + std::to_string(lens[i]) + " bytes, longer than the column's " + std::to_string(width));
    }
    if (!bytes && (lens[0] > 0 || lens[1] > 0)) return fail(IMM3_ERR_ARG, "StrRange without bounds: match_bytes is null");
    return IMM3_OK;
}

// lo' = lo padded to `width` with 0x00, hi' = hi padded with 0xFF (lengths 0 .. width: str_range_check_leaf)
void str_range_pad(const uint8_t *lo, int32_t lo_len, const uint8_t *hi, int32_t hi_len, int32_t width, std::string &lo_out, std::string &hi_out) {
    lo_out.assign((size_t)std::max(width, 0), '\0');
    hi_out.assign((size_t)std::max(width, 0), (char)0xFF);
    if (lo_len > 0) std::memcpy(&lo_out[0], lo, (size_t)std::min(lo_len, width));
    if (hi_len > 0) std::memcpy(&hi_out[0], hi, (size_t)std::min(hi_len, width));
}

bool str_range_empty(const std::string &lo, const std::string &hi) { return bytes_less(hi, lo); } // lo' > hi': no row passes
bool str_range_full(const std::string &lo, const std::string &hi) {                                // every row passes
    for (unsigned char c : lo) if (c != 0x00) return false;
    for (unsigned char c : hi) if (c != 0xFF) return false;
    return true;
}
bool str_range_holds(const std::string &lo, const std::string &hi, const std::string &v) { // v: exactly the column's width
    return v.size() == lo.size() && !bytes_less(v, lo) && !bytes_less(hi, v);
}

// two ranges on one column: the larger lo, the smaller hi
void str_range_intersect(std::string &lo, std::string &hi, const std::string &lo2, const std::string &hi2) {
    if (bytes_less(lo, lo2)) lo = lo2;
    if (bytes_less(hi2, hi)) hi = hi2;
}

// a range and a Match on one column: the IN-list's values that lie inside the range, in the list's order
void str_range_filter_match(const std::string &lo, const std::string &hi, std::vector<std::string> &match) {
    std::vector<std::string> left;
    for (auto &v : match)
        if (str_range_holds(lo, hi, v)) left.push_back(v);
    match.swap(left);
}

// The next / the previous value of the column's width in byte order: big-endian arithmetic over all its bytes, carries and borrows
// running from the last byte to the first.  false: there is none (all 0xFF / all 0x00, or a column without bytes); v is unchanged.
bool str_range_successor(std::string &v) {
    size_t i = v.size();
    while (i > 0 && (unsigned char)v[i - 1] == 0xFF) --i;
    if (i == 0) return false;
    v[i - 1] = (char)((unsigned char)v[i - 1] + 1);
    std::fill(v.begin() + (std::ptrdiff_t)i, v.end(), '\0');
    return true;
}
bool str_range_predecessor(std::string &v) {
    size_t i = v.size();
    while (i > 0 && (unsigned char)v[i - 1] == 0x00) --i;
    if (i == 0) return false;
    v[i - 1] = (char)((unsigned char)v[i - 1] - 1);
    std::fill(v.begin() + (std::ptrdiff_t)i, v.end(), (char)0xFF);
    return true;
}

// Which kernel a range goes to on a uniform layout: 1 the string pass (a whole number of dwords, 4 .. IMM3_STRING_MAX_WIDTH bytes),
// 2 the word-at-a-time kernel, -1 no such column.
int str_range_route(int32_t width) {
    if (width < 1 || width > IMM3_STRING_MAX_WIDTH) return -1;
    return width % 4 == 0 ? 1 : 2;
}

// The bounds as the kernels read them.  `blob` (device memory behind FoldedPred::d_blob): lo' then hi' as they are, `width` bytes each
// (the word-at-a-time kernel compares byte by byte); for a width of D whole dwords then D + D dwords more, lo' and hi' with every
// dword's bytes swapped -- the dword's first byte most significant, so that unsigned dword order is byte order (the string pass
// reads the tails behind the first 16 bytes from there).  lo4 / hi4: the first min(D, 4) swapped dwords, the string pass's kernel
// arguments (the rest zero).
void str_range_pack(const std::string &lo, const std::string &hi, std::vector<uint8_t> &blob, uint32_t lo4[4], uint32_t hi4[4]) {
    const size_t W = lo.size();
    blob.assign(lo.begin(), lo.end());
    blob.insert(blob.end(), hi.begin(), hi.end());
    for (int d = 0; d < 4; ++d) lo4[d] = hi4[d] = 0;
    if (W == 0 || W % 4 != 0) return;
    const size_t D = W / 4;
    for (int side = 0; side < 2; ++side) {
        const std::string &b = side ? hi : lo;
        for (size_t d = 0; d < D; ++d) {
            const uint32_t x = ((uint32_t)(uint8_t)b[4 * d] << 24) | ((uint32_t)(uint8_t)b[4 * d + 1] << 16) | ((uint32_t)(uint8_t)b[4 * d + 2] << 8) | (uint32_t)(uint8_t)b[4 * d + 3];
            uint8_t raw[4];
            std::memcpy(raw, &x, 4);
            blob.insert(blob.end(), raw, raw + 4);
            if (d < 4) (side ? hi4 : lo4)[d] = x;
        }
    }
}

} // namespace imm3

extern "C" int imm3_plan_string_range_route(int32_t width) { return imm3::str_range_route(width); }
