// The select-tree normaliser (immutable3_amd/csrc/imm3_expr_norm.cpp) on its own, for a build under -fsanitize=address,undefined:
// tests/test_expr_not_host.py compiles this file together with the normaliser, runs it and compares what it prints with what
// the library gives through python.  Every line of the input (stdin) is one program over the fixed leaves below; the output is one
// line per program: its normal form as JSON, or "error <code> <message>".  No device, no other part of the library: the one
// function the normaliser takes from the rest (imm3::fail) is defined here.
#include "../../include/imm3.h"
#include "../../include/imm3_diag.h"

#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

static std::string g_error;
namespace imm3 {
int fail(int code, const std::string &msg) {
    g_error = msg;
    return code;
}
} // namespace imm3

int main() {
    // columns: int32, int8, 2-byte string, 4-byte string (the tests' CODECS / WIDTHS)
    const int32_t codec[4] = {IMM3_DENSE_INT, IMM3_DENSE_TINYINT, IMM3_DENSE_STRING, IMM3_DENSE_STRING};
    const int32_t width[4] = {4, 1, 2, 4};
    // leaves: what test_expr_not_host.py's ASAN_LEAVES lists, in that order
    static const char m_ca[] = "CA", m_ca_ny[] = "CANY", m_ny_tx[] = "NYTX", m_wrong[] = "XYZQ", m_code[] = "ab12";
    static const int32_t l2[1] = {2}, l22[2] = {2, 2}, l31[2] = {3, 1}, l4[1] = {4};
    const double nan = std::strtod("nan", nullptr);
    std::vector<imm3_select> leaves;
    const auto num = [&](int32_t col, int32_t cond, double v) {
        imm3_select s;
        std::memset(&s, 0, sizeof(s));
        s.column = col;
        s.cond = cond;
        s.value = v;
        leaves.push_back(s);
    };
    const auto match = [&](int32_t col, const char *bytes, const int32_t *lens, int32_t n) {
        imm3_select s;
        std::memset(&s, 0, sizeof(s));
        s.column = col;
        s.cond = IMM3_MATCH;
        s.match_bytes = (const uint8_t *)bytes;
        s.match_lens = lens;
        s.n_match = n;
        leaves.push_back(s);
    };
    num(0, IMM3_GT, 1e12);            // 0
    num(0, IMM3_LT, -1e12);           // 1
    num(0, IMM3_GT, nan);             // 2
    num(0, IMM3_EQ, -2147483648.0);   // 3
    num(0, IMM3_EQ, 2147483647.0);    // 4
    num(0, IMM3_EQ, 7.0);             // 5
    num(1, IMM3_EQ, -128.0);          // 6
    num(1, IMM3_EQ, 127.0);           // 7
    num(1, IMM3_GT, 18.0);            // 8
    num(1, IMM3_LT, 30.0);            // 9
    match(2, m_ca, l2, 1);            // 10
    match(2, m_ca_ny, l22, 2);        // 11
    match(2, m_ny_tx, l22, 2);        // 12
    match(2, m_wrong, l31, 2);        // 13: "XYZ", "Q" -- wrong lengths only
    match(3, m_code, l4, 1);          // 14
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::vector<int32_t> prog;
        for (int32_t v; in >> v;) prog.push_back(v);
        int64_t need = 0;
        int rc = imm3_expr_normalize(codec, width, 4, leaves.data(), (int32_t)leaves.size(), prog.data(), (int32_t)prog.size(), nullptr, 0, &need);
        std::vector<char> buf((size_t)(need > 0 ? need : 1));
        if (!rc) rc = imm3_expr_normalize(codec, width, 4, leaves.data(), (int32_t)leaves.size(), prog.data(), (int32_t)prog.size(), buf.data(), need, nullptr);
        if (rc) std::printf("error %d %s\n", rc, g_error.c_str());
        else std::printf("%s\n", buf.data());
    }
    return 0;
}
