// imm3_expr_norm.cpp -- select trees on the host: one leaf as a folded predicate, the postfix program's checks, and the normal form
// the kernels of imm3_expr.hip evaluate -- a disjunction of TERMS, each a conjunction with at most one folded predicate per column
// (one closed interval, or one intersected IN-list: what fold_selects makes of a flat select list; under an IMM3_EXPR_NOT also a
// NEGATED IN-list, the exclusions of a complemented Match).  No device is touched here.
#include "../../include/imm3.h"
#include "../../include/imm3_diag.h"
#include "imm3_handles.h"
#include "imm3_api_internal.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace imm3 {

// The range logic is a unit of its own (imm3_str_range.cpp) and a WEAK reference from this file: the normaliser is also built
// without it (tests/native/expr_not_asan.cpp links this file alone), where a range leaf is refused instead of folded.
__attribute__((weak)) int str_range_check_leaf(int32_t n_match, const uint8_t *bytes, const int32_t *lens, int32_t width);
__attribute__((weak)) void str_range_pad(const uint8_t *lo, int32_t lo_len, const uint8_t *hi, int32_t hi_len, int32_t width, std::string &lo_out, std::string &hi_out);
__attribute__((weak)) bool str_range_empty(const std::string &lo, const std::string &hi);
__attribute__((weak)) bool str_range_full(const std::string &lo, const std::string &hi);
__attribute__((weak)) void str_range_intersect(std::string &lo, std::string &hi, const std::string &lo2, const std::string &hi2);
__attribute__((weak)) void str_range_filter_match(const std::string &lo, const std::string &hi, std::vector<std::string> &match);
// ... and so is the list logic of IMM3_INT_IN (imm3_int_list_plan.cpp)
__attribute__((weak)) int int_list_parse(int32_t n_match, const uint8_t *bytes, int32_t width, std::vector<int32_t> &out);
__attribute__((weak)) void int_list_clip(std::vector<int32_t> &list, int64_t lo, int64_t hi);
__attribute__((weak)) void int_list_intersect(std::vector<int32_t> &list, const std::vector<int32_t> &other);
// ... and the set leaf's interval (IMM3_INT_IN_SET: imm3_int_set_plan.cpp)
__attribute__((weak)) void int_set_fold_interval(int64_t &lo, int64_t &hi, int64_t n, int32_t min, int32_t max);

const char *const kTreeIntInRefusal =
    "a select program with an IMM3_EXPR_OR or an IMM3_EXPR_NOT does not take IMM3_INT_IN leaves (its normal form would need "
    "negated lists and intervals with exclusions); a program of IMM3_EXPR_AND alone does";
const char *const kTreeIntSetRefusal =
    "a select program with an IMM3_EXPR_OR or an IMM3_EXPR_NOT does not take IMM3_INT_IN_SET leaves (NOT IN (sub-query) and a set under "
    "OR are out of scope: its normal form would need negated sets and intervals with exclusions); a program of IMM3_EXPR_AND alone does";
const char *const kIntSetOneListRefusal =
    "a column with an IMM3_INT_IN_SET leaf takes no other IMM3_INT_IN or IMM3_INT_IN_SET leaf (the intersection of device-resident sets "
    "is not built); intersect in the sub-query instead";

namespace {
// a numeric predicate with a list, settled: the list's values inside the interval, the interval tightened to the list's minimum and
// maximum; no value left: the empty interval (lo > hi), which is what every caller reads as "selects nothing"
void settle_list(FoldedPred &p) {
    if (!p.has_list) return;
    if (pred_list_shared(p)) { // the values stay on the device: the interval is already cut to the set's span, and the probe tests it first
        if (p.lo > p.hi) { p.lo = 1; p.hi = 0; }
        return;
    }
    int_list_clip(p.list, p.lo, p.hi);
    if (p.list.empty()) { p.lo = 1; p.hi = 0; }
    else { p.lo = p.list.front(); p.hi = p.list.back(); }
}
} // namespace

// One SelectOp leaf on a column of DENSE_* codec `vcodec`: GT / LT / EQ narrow the column type's full interval (threshold narrowed
// per leaf: d.toInt / d.toByte, Select.scala:65,73), Match keeps the values of exactly `width` bytes, each once.
int leaf_pred(int32_t seg_col, int32_t vcodec, int32_t width, const imm3_select &leaf, FoldedPred &out) {
    out = unfolded_pred(seg_col, vcodec, width);
    if (out.kind == KIND_STR && leaf.cond == IMM3_STR_RANGE) { // lo' <= row <= hi' (imm3_str_range.cpp)
        if (!str_range_check_leaf || !str_range_pad) return fail(IMM3_ERR_ARG, "IMM3_STR_RANGE: this build holds no range logic");
        const int rc = str_range_check_leaf(leaf.n_match, leaf.match_bytes, leaf.match_lens, width);
        if (rc) return rc;
        out.has_range = true;
        str_range_pad(leaf.match_bytes, leaf.match_lens[0], leaf.match_bytes + leaf.match_lens[0], leaf.match_lens[1], width, out.range_lo, out.range_hi);
    } else if (out.kind == KIND_STR) {
        int64_t off = 0;
        for (int32_t m = 0; m < leaf.n_match; ++m) {
            const int32_t len = leaf.match_lens[m];
            if (len < 0) return fail(IMM3_ERR_ARG, "negative match length");
            // String.equals can only hold for a value of exactly `width` bytes (DataType.scala:69-70)
            if (len == width) {
                std::string v((const char *)leaf.match_bytes + off, (size_t)len);
                if (std::find(out.match.begin(), out.match.end(), v) == out.match.end()) out.match.push_back(v);
            }
            off += len;
        }
    } else if (leaf.cond == IMM3_INT_IN) { // a member of the list (imm3_int_list_plan.cpp)
        if (!int_list_parse || !int_list_clip || !int_list_intersect) return fail(IMM3_ERR_ARG, "IMM3_INT_IN: this build holds no list logic");
        const int rc = int_list_parse(leaf.n_match, leaf.match_bytes, width, out.list);
        if (rc) return rc;
        out.has_list = true;
        settle_list(out);
    } else if (leaf.cond == IMM3_INT_IN_SET) { // a member of a shared set (the handle has passed int_set_check_leaf)
        if (!int_list_clip || !int_set_fold_interval) return fail(IMM3_ERR_ARG, "IMM3_INT_IN_SET: this build holds no set logic");
        const imm3_int_set *set = (const imm3_int_set *)leaf.match_bytes;
        out.has_list = true;
        out.set = set;
        if (!pred_list_shared(out)) out.list = set->small; // an ordinary short list from here on (int8: settle_list drops what no row holds)
        else {
            int_set_fold_interval(out.lo, out.hi, set->n, set->min, set->max);
            bool any8 = false;
            for (int i = 0; i < 8; ++i) any8 = any8 || set->set256[i] != 0;
            if (out.kind == KIND_I8 && !any8) { out.lo = 1; out.hi = 0; } // none of its values is an int8
        }
        settle_list(out);
    } else {
        const int64_t t = out.kind == KIND_I32 ? (int64_t)jvm_d2i(leaf.value) : (int64_t)jvm_d2b(leaf.value);
        if (leaf.cond == IMM3_GT) out.lo = std::max(out.lo, t + 1);      // strict >, Select.scala:68,76
        else if (leaf.cond == IMM3_LT) out.hi = std::min(out.hi, t - 1); // strict <, Select.scala:106,114
        else { out.lo = std::max(out.lo, t); out.hi = std::min(out.hi, t); } // ==, Select.scala:144,152
    }
    return IMM3_OK;
}

// the conjunction of two predicates on the same column: intervals intersect, IN-lists intersect (the first one's order stays);
// IN and NOT-IN: the IN-list minus the exclusions (still an IN-list, maybe empty); NOT-IN and NOT-IN: the union of the exclusions,
// first seen first
void merge_pred(FoldedPred &into, const FoldedPred &other) {
    if (into.kind == KIND_STR && (into.has_range || other.has_range)) {
        // two ranges: their intersection; a range and an IN-list: the list's values inside the range -- an ordinary Match from here on
        // (a program with an OR or a NOT takes no range: neither side is negated)
        if (into.has_range && other.has_range) str_range_intersect(into.range_lo, into.range_hi, other.range_lo, other.range_hi);
        else {
            const FoldedPred &r = into.has_range ? into : other;
            std::vector<std::string> list = into.has_range ? other.match : into.match;
            str_range_filter_match(r.range_lo, r.range_hi, list);
            into.match = list;
            into.has_range = false;
            into.range_lo.clear();
            into.range_hi.clear();
        }
    } else if (into.kind == KIND_STR) {
        const auto has = [](const std::vector<std::string> &l, const std::string &v) { return std::find(l.begin(), l.end(), v) != l.end(); };
        if (into.negated && other.negated) {
            for (auto &v : other.match)
                if (!has(into.match, v)) into.match.push_back(v);
            return;
        }
        const std::vector<std::string> &in = into.negated ? other.match : into.match, &cut = into.negated ? into.match : other.match;
        const bool keep_common = !into.negated && !other.negated; // IN and IN: what both hold; else: what the exclusions leave
        std::vector<std::string> left;
        for (auto &v : in)
            if (has(cut, v) == keep_common) left.push_back(v);
        into.match = left;
        into.negated = false;
    } else { // an interval, and optionally a list: two lists intersect, the list keeps its values inside the interval
        into.lo = std::max(into.lo, other.lo);
        into.hi = std::min(into.hi, other.hi);
        if (into.has_list && other.has_list) int_list_intersect(into.list, other.list);
        else if (other.has_list) { into.has_list = true; into.list = other.list; into.set = other.set; }
        settle_list(into);
    }
}

bool pred_empty(const FoldedPred &p) { // (a NOT-IN is never empty)
    if (p.kind == KIND_STR && p.has_range) return str_range_empty(p.range_lo, p.range_hi);
    return p.kind == KIND_STR ? (!p.negated && p.match.empty()) : p.lo > p.hi;
}

// every value passes: the column type's full interval, or a NOT-IN without exclusions (only a complement makes one)
bool pred_unconstrained(const FoldedPred &p) {
    if (p.kind == KIND_STR && p.has_range) return str_range_full(p.range_lo, p.range_hi);
    if (p.kind == KIND_STR) return p.negated && p.match.empty();
    if (p.has_list) return false; // (a list is a constraint even when it holds every value of the type)
    const FoldedPred full = unfolded_pred(p.seg_col, p.kind == KIND_I32 ? IMM3_DENSE_INT : IMM3_DENSE_TINYINT, p.width);
    return p.lo <= full.lo && p.hi >= full.hi;
}

int expr_check_program(const int32_t *prog, int32_t n_prog, int32_t n_leaves, bool *has_or, bool *has_not) {
    if (has_or) *has_or = false;
    if (has_not) *has_not = false;
    if (n_prog < 0 || (n_prog > 0 && !prog)) return fail(IMM3_ERR_ARG, "bad select program");
    if (n_prog == 0) return n_leaves == 0 ? IMM3_OK : fail(IMM3_ERR_ARG, "select program: empty, but leaves were given");
    int64_t depth = 0;
    for (int32_t i = 0; i < n_prog; ++i) {
        const int32_t op = prog[i];
        if (op >= 0) {
            if (op >= n_leaves) return fail(IMM3_ERR_ARG, "select program: leaf index out of range");
            ++depth;
        } else if (op == IMM3_EXPR_AND || op == IMM3_EXPR_OR) {
            if (depth < 2) return fail(IMM3_ERR_ARG, "select program: stack underflow");
            --depth;
            if (op == IMM3_EXPR_OR && has_or) *has_or = true;
        } else if (op == IMM3_EXPR_NOT) {
            if (depth < 1) return fail(IMM3_ERR_ARG, "select program: stack underflow");
            if (has_not) *has_not = true;
        } else return fail(IMM3_ERR_ARG, "select program: unknown operator");
    }
    if (depth != 1) return fail(IMM3_ERR_ARG, "select program: more than one result");
    return IMM3_OK;
}

namespace {
bool same_pred(const FoldedPred &a, const FoldedPred &b) {
    if (a.seg_col != b.seg_col) return false;
    if (a.kind != KIND_STR) return a.lo == b.lo && a.hi == b.hi && a.has_list == b.has_list && a.list == b.list;
    if (a.negated != b.negated || a.match.size() != b.match.size()) return false;
    for (auto &v : a.match)
        if (std::find(b.match.begin(), b.match.end(), v) == b.match.end()) return false;
    return true;
}
bool same_term(const ExprTerm &a, const ExprTerm &b) {
    if (a.size() != b.size()) return false;
    for (const auto &p : a) {
        bool found = false;
        for (const auto &r : b) found = found || same_pred(p, r);
        if (!found) return false;
    }
    return true;
}
// The disjunction of two predicates on one column as ONE predicate, where a complement makes that possible: intervals that overlap
// or touch, and a string list with a NOT-IN (IN or NOT-IN: the exclusions the IN-list does not give back; NOT-IN or NOT-IN: the
// exclusions both hold).  Two IN-lists stay two terms, as in a tree without NOT.
bool union_pred(const FoldedPred &a, const FoldedPred &b, FoldedPred &out) {
    out = a;
    if (a.kind != KIND_STR) {
        if (a.lo > b.hi + 1 || b.lo > a.hi + 1) return false;
        out.lo = std::min(a.lo, b.lo);
        out.hi = std::max(a.hi, b.hi);
        return true;
    }
    if (!a.negated && !b.negated) return false;
    const FoldedPred &neg = a.negated ? a : b, &other = a.negated ? b : a;
    out = neg;
    out.match.clear();
    for (auto &v : neg.match) {
        const bool in_other = std::find(other.match.begin(), other.match.end(), v) != other.match.end();
        if (in_other == other.negated) out.match.push_back(v); // still excluded: by both NOT-INs / not given back by the IN-list
    }
    return true;
}
// `complemented` (the tree holds a negation that did not cancel): the result sheds predicates every value passes -- a term without
// any is UNIVERSAL and absorbs all others -- and a term that differs from one already there in ONE column, where the two predicates
// are one (union_pred), replaces it: `x or not x` comes out as the universal term, not as two halves.  A tree without NOT never
// holds such a predicate and keeps its terms exactly as they were before NOT existed.
void add_term(std::vector<ExprTerm> &dnf, ExprTerm t, bool complemented) {
    for (const auto &p : t)
        if (pred_empty(p)) return; // selects nothing
    if (complemented) {
        if (dnf.size() == 1 && dnf[0].empty()) return; // (universal already)
        t.erase(std::remove_if(t.begin(), t.end(), pred_unconstrained), t.end());
        if (t.empty()) {
            dnf.assign(1, t);
            return;
        }
        for (size_t h = 0; h < dnf.size(); ++h) {
            const ExprTerm &have = dnf[h];
            if (have.size() != t.size()) continue;
            const FoldedPred *mine = nullptr, *theirs = nullptr;
            int differ = 0;
            for (const auto &p : t) {
                const FoldedPred *r = nullptr;
                for (const auto &c : have)
                    if (c.seg_col == p.seg_col) r = &c;
                if (!r) { differ = 2; break; }
                if (!same_pred(p, *r)) { ++differ; mine = &p; theirs = r; }
            }
            FoldedPred u;
            if (differ != 1 || !union_pred(*theirs, *mine, u)) continue;
            ExprTerm merged;
            for (const auto &c : have) merged.push_back(c.seg_col == u.seg_col ? u : c);
            dnf.erase(dnf.begin() + (std::ptrdiff_t)h);
            add_term(dnf, merged, true); // (it may now meet a third term the same way)
            return;
        }
    }
    for (const auto &have : dnf)
        if (same_term(have, t)) return;
    dnf.push_back(t);
}
constexpr size_t kMaxWorkTerms = 4096; // terms of an intermediate result (the final bound is the kernels': kMaxExprGenericTerms)

// The complement of one leaf as terms, in int64 so nothing overflows at the type's ends: NOT GT t = [MIN, t], NOT LT t = [t, MAX],
// NOT EQ t = [MIN, t - 1] or [t + 1, MAX] (an empty piece dropped), NOT Match = the NEGATED IN-list of the values of the column's
// width (the others never matched: they are no exclusions either).
void complement_leaf(const FoldedPred &full, const FoldedPred &leaf, int32_t cond, std::vector<ExprTerm> &dnf) {
    FoldedPred c = full;
    if (leaf.kind == KIND_STR) {
        c.match = leaf.match;
        c.negated = true;
        add_term(dnf, ExprTerm{c}, true);
        return;
    }
    if (cond == IMM3_GT) c.hi = leaf.lo - 1;        // leaf: [t + 1, MAX]
    else if (cond == IMM3_LT) c.lo = leaf.hi + 1;   // leaf: [MIN, t - 1]
    else {                                          // leaf: [t, t]
        FoldedPred below = full;
        below.hi = leaf.lo - 1;
        add_term(dnf, ExprTerm{below}, true);
        c.lo = leaf.lo + 1;
    }
    add_term(dnf, ExprTerm{c}, true);
}
} // namespace

// The tree as a disjunction of terms.  IMM3_EXPR_NOT is pushed down to the leaves first (De Morgan over AND / OR, a double NOT
// cancels): one walk over the program from its end tells every leaf whether it stands complemented and every AND / OR whether it
// trades places with the other.  Then AND distributes over OR (every pair of terms, merged per column), terms that select nothing
// and duplicates are dropped; no term left = the tree selects nothing, the one term without a predicate = it selects every row.
// A term keeps its columns in the order the program first names them: a tree without OR and NOT gives the one term whose predicates
// are fold_selects' of the same leaves in program order.
int expr_normalize(const std::vector<ExprCol> &leaf_cols, const imm3_select *leaves, int32_t n_leaves, const int32_t *prog, int32_t n_prog,
                   std::vector<ExprTerm> &terms) {
    terms.clear();
    const int crc = expr_check_program(prog, n_prog, n_leaves, nullptr, nullptr);
    if (crc) return crc;
    std::vector<uint8_t> flipped((size_t)n_prog, 0); // leaf: complemented; AND / OR: the other one
    bool complemented = false;
    {
        std::vector<uint8_t> pending(1, 0); // the parity each subtree still to come (walking backwards) stands under
        for (int32_t i = n_prog - 1; i >= 0; --i) {
            const uint8_t par = pending.back();
            pending.pop_back();
            const int32_t op = prog[i];
            if (op == IMM3_EXPR_NOT) pending.push_back(par ^ 1);
            else {
                flipped[(size_t)i] = par;
                complemented = complemented || par;
                if (op < 0) pending.insert(pending.end(), 2, par);
            }
        }
    }
    std::vector<std::vector<ExprTerm>> stack;
    for (int32_t i = 0; i < n_prog; ++i) {
        int32_t op = prog[i];
        if (op == IMM3_EXPR_NOT) continue; // (it has reached its leaves)
        if (op >= 0) {
            const ExprCol &c = leaf_cols[(size_t)op];
            FoldedPred fp;
            const int lrc = leaf_pred(c.seg_col, c.vcodec, c.width, leaves[op], fp);
            if (lrc) return lrc;
            std::vector<ExprTerm> dnf;
            if (flipped[(size_t)i]) complement_leaf(unfolded_pred(c.seg_col, c.vcodec, c.width), fp, leaves[op].cond, dnf);
            else add_term(dnf, ExprTerm{fp}, complemented);
            stack.push_back(std::move(dnf));
            continue;
        }
        if (flipped[(size_t)i]) op = op == IMM3_EXPR_OR ? IMM3_EXPR_AND : IMM3_EXPR_OR;
        std::vector<ExprTerm> b = std::move(stack.back());
        stack.pop_back();
        std::vector<ExprTerm> a = std::move(stack.back());
        stack.pop_back();
        std::vector<ExprTerm> r;
        if (op == IMM3_EXPR_OR) {
            r = std::move(a);
            for (const auto &t : b) add_term(r, t, complemented);
        } else {
            for (const auto &x : a)
                for (const auto &y : b) {
                    ExprTerm t = x;
                    for (const auto &p : y) {
                        FoldedPred *mine = pred_on(t, p.seg_col);
                        if (mine) merge_pred(*mine, p);
                        else t.push_back(p);
                    }
                    add_term(r, t, complemented);
                    if (r.size() > kMaxWorkTerms) return fail(IMM3_ERR_ARG, "select tree: too many terms");
                }
        }
        if (r.size() > kMaxWorkTerms) return fail(IMM3_ERR_ARG, "select tree: too many terms");
        stack.push_back(std::move(r));
    }
    if (!stack.empty()) terms = std::move(stack.back());
    if (terms.size() > (size_t)kMaxExprGenericTerms)
        return fail(IMM3_ERR_ARG, "select tree: its normal form has " + std::to_string(terms.size()) + " terms, more than " + std::to_string(kMaxExprGenericTerms));
    return IMM3_OK;
}

} // namespace imm3

using namespace imm3;

// diagnostics: the normaliser without a device (tests hold the terms' truth table against the tree's)
extern "C" int imm3_expr_normalize(const int32_t *col_codec, const int32_t *col_width, int32_t n_cols, const imm3_select *leaves, int32_t n_leaves,
                                   const int32_t *prog, int32_t n_prog, char *json_out, int64_t cap, int64_t *needed) {
    if (n_cols < 0 || (n_cols > 0 && (!col_codec || !col_width)) || n_leaves < 0 || (n_leaves > 0 && !leaves) || cap < 0 || (cap > 0 && !json_out))
        return fail(IMM3_ERR_ARG, "bad argument");
    std::vector<ExprCol> leaf_cols;
    for (int32_t i = 0; i < n_leaves; ++i) {
        const int32_t c = leaves[i].column, cond = leaves[i].cond;
        if (c < 0 || c >= n_cols) return fail(IMM3_ERR_ARG, "select column is not among the columns");
        if (cond != IMM3_MATCH && cond != IMM3_GT && cond != IMM3_LT && cond != IMM3_EQ && cond != IMM3_INT_IN) return fail(IMM3_ERR_UNSUPPORTED_CONDITION, "Unsupported condition");
        const int32_t vc = value_codec(col_codec[c]);
        if (vc != IMM3_DENSE_INT && vc != IMM3_DENSE_TINYINT && vc != IMM3_DENSE_STRING) return fail(IMM3_ERR_NO_CODEC, "No implementation for codec " + std::to_string(col_codec[c]));
        if ((cond == IMM3_MATCH) != (vc == IMM3_DENSE_STRING)) return fail(IMM3_ERR_UNSUPPORTED_VECTOR, "Unsupported column vector");
        if (cond == IMM3_MATCH && leaves[i].n_match > 0 && (!leaves[i].match_bytes || !leaves[i].match_lens)) return fail(IMM3_ERR_ARG, "Match without values");
        leaf_cols.push_back(ExprCol{c, vc, col_width[c]});
    }
    {   // (as query creation: a program with an OR or a NOT takes no list)
        bool has_or = false, has_not = false;
        const int prc = expr_check_program(prog, n_prog, n_leaves, &has_or, &has_not);
        if (prc) return prc;
        for (int32_t i = 0; (has_or || has_not) && i < n_leaves; ++i)
            if (leaves[i].cond == IMM3_INT_IN) return fail(IMM3_ERR_ARG, kTreeIntInRefusal);
    }
    std::vector<ExprTerm> terms;
    const int rc = expr_normalize(leaf_cols, leaves, n_leaves, prog, n_prog, terms);
    if (rc) return rc;
    std::string js = "[";
    for (size_t t = 0; t < terms.size(); ++t) {
        js += t ? ",[" : "[";
        for (size_t k = 0; k < terms[t].size(); ++k) {
            const FoldedPred &p = terms[t][k];
            js += k ? ",{" : "{";
            js += "\"col\":" + std::to_string(p.seg_col);
            if (p.kind == KIND_STR) {
                js += p.negated ? ",\"not_match\":[" : ",\"match\":[";
                for (size_t m = 0; m < p.match.size(); ++m) {
                    js += m ? ",\"" : "\"";
                    char hex[3];
                    for (unsigned char ch : p.match[m]) {
                        std::snprintf(hex, sizeof(hex), "%02x", ch);
                        js += hex;
                    }
                    js += "\"";
                }
                js += "]";
            } else {
                js += ",\"lo\":" + std::to_string(p.lo) + ",\"hi\":" + std::to_string(p.hi);
                if (p.has_list) {
                    js += ",\"list\":[";
                    for (size_t m = 0; m < p.list.size(); ++m) js += (m ? "," : "") + std::to_string(p.list[m]);
                    js += "]";
                }
            }
            js += "}";
        }
        js += "]";
    }
    js += "]";
    if (needed) *needed = (int64_t)js.size() + 1;
    if ((int64_t)js.size() + 1 > cap) return cap == 0 ? IMM3_OK : fail(IMM3_ERR_ARG, "json_out is too small");
    std::memcpy(json_out, js.c_str(), js.size() + 1);
    return IMM3_OK;
}
