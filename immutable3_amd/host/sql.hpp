// sql.hpp -- SQLParser: the SQL subset of engine/src/main/scala/immutabledb/sql/SQLParser.scala:8-129,
// restated as a backtracking recursive-descent parser with the semantics of scala-parser-combinators'
// JavaTokenParsers: whitespace is skipped before every literal / regex, literals match as PREFIXES (no word
// boundary), alternatives are tried in order with backtracking, parseAll must consume the whole input.
//
//   query            := queryProjectAgg | queryProjectAggNoGroup | queryProject            (:13)
//   queryProject     := "select" repsep(ident, ",") "from" ident where limit               (:27-31, :45-47, :115-116)
//   queryProjectAgg  := "select" rep1sep(agg, ",") "from" ident where ["group" "by" rep1sep(ident, ",")]   (:15-25)
//   where            := opt("where" filter)                                                  (:49-54)
//   filter           := "(" repsep(filter,"and") ")" | "(" repsep(filter,"or") ")"
//                     | ident "=" value | ident "=" "'" value "'" | ident ">" value | ident "<" value   (:56-96)
//   limit            := opt("limit" digits)                                                  (:37)
// EXTENSION, only when the parser is asked for it (parseAll(sql, true); imm3_sql --order-by) -- the "sort" core/Query.scala:27 announces:
//   queryProject     := "select" repsep(ident, ",") "from" ident where orderBy limit
//   orderBy          := opt("order" "by" rep1sep(ident opt("asc" | "desc"), ","))
//   queryProjectAgg  := "select" rep1sep(agg, ",") "from" ident where ["group" "by" rep1sep(ident, ",")] orderBy limit
// an aggregation's order key being an ident (a group-by column or an alias) or an aggregate call as written in the SELECT list
// (`count(id)`), which resolves to its alias (id_count); a name that is neither is refused.
// With the flag off the grammar is the reference's, and such a statement fails to parse as it always has.
// EXTENSION, only when asked for (parseAll(sql, orderBy, true); imm3_sql --string-ranges) -- byte-order ranges on string columns
// (SelectCondition::prefix / strGT / strLT), tried behind the reference's alternatives:
//   filter           := ... | ident ">" "'" value "'" | ident "<" "'" value "'" | ident "like" "'" value "%" "'"
// With the flag off those statements fail to parse with the message they have always given.
// EXTENSION, only when asked for (parseAll(sql, orderBy, stringRanges, true); imm3_sql --having) -- HAVING over the groups of an
// aggregation, before their order and limit:
//   queryProjectAgg  := "select" rep1sep(agg, ",") "from" ident where ["group" "by" rep1sep(ident, ",")] having orderBy limit
//   having           := opt("having" hfilter)
//   hfilter          := "(" repsep(hfilter,"and") ")" | "(" repsep(hfilter,"or") ")" | hkey ">" value | hkey "<" value | hkey "=" value
//   hkey             := ident | the aggregate call as written in the SELECT list (count(id) names id_count)
// orderBy / limit follow only under their own flag.  The tree becomes ProjectADT::having; a name that is no alias, a group-by column
// and a threshold that is no integer are refused (checkGroupFilterNames).  With the flag off the grammar and every parse-failure
// message are what they were.
// EXTENSION, only when asked for (parseAll(sql, orderBy, stringRanges, having, true); imm3_sql --count-distinct) -- the number of
// distinct values per group (Aggregate::CountDistinct), tried in front of the reference's aggregates:
//   agg              := "count" "(" "distinct" ident ")" | ...
// wherever an aggregate call may stand (the SELECT list, an order key, a having key: `count(distinct age)` names age_distinct).
// Literals match as prefixes, as everywhere here, so under the flag `count(distinctx)` is count(distinct x); a column called `distinct`
// itself still counts as before (no ident follows).  With the flag off the grammar is exactly what it was: `count(distinct x)` fails
// with "`)' expected".
// EXTENSION, only when asked for (parseAll(sql, orderBy, stringRanges, having, countDistinct, true); imm3_sql --int-lists) -- IN-lists
// on int32 / int8 columns (SelectCondition::IntIn), tried behind the reference's alternatives (and behind the string ranges):
//   filter           := ... | ident "in" "(" rep1sep(int, ",") ")"        int = -?[0-9]+
// A literal outside int32 throws (kIntListRangeError + the literal) at parse time.  With the flag off the grammar and every
// parse-failure message are what they were.
// EXTENSION, only when asked for (parseAll(sql, ..., intLists, true); imm3_sql --subqueries) -- IN (sub-query) on int32 / int8 columns
// (SelectCondition::IntInQuery), tried behind everything above:
//   filter           := ... | ident "in" "(" "select" ident from where ")"
// The inner statement is one column, a table and an optional where tree (which may hold further sub-queries): no aggregate, no group
// by, order by or limit can be spelled there.  With the flag off the grammar and every parse-failure message are what they were.
//   ident =[\w#]+   value = [\w0-9#]+  (no sign, no decimal point)                          (:119-121)
#pragma once

#include <cctype>
#include <cstdlib>
#include <cstring>

#include "schema.hpp"

namespace immutabledb {

class SQLParser {
  public:
    static constexpr const char *kIntListRangeError = "integer literal out of range for an IN-list (int32): ";
    static Query parseAll(const std::string &input, bool orderBy = false, bool stringRanges = false, bool having = false, bool countDistinct = false,
                          bool intLists = false, bool subqueries = false) {
        SQLParser p(input);
        p.intLists_ = intLists;
        p.subqueries_ = subqueries;
        p.countDistinct_ = countDistinct;
        p.orderBy_ = orderBy;
        p.stringRanges_ = stringRanges;
        p.having_ = having;
        Query q;
        size_t end = 0;
        if (p.query(0, q, end)) {
            end = p.skipWs(end);
            if (end == input.size()) return q;
            throw Exception("[1." + std::to_string(end + 1) + "] failure: end of input expected\n\n" + input);
        }
        throw Exception("[1." + std::to_string(p.furthest_ + 1) + "] failure: " + p.expected_ + " expected\n\n" + input);
    }

  private:
    explicit SQLParser(const std::string &s) : s_(s) {}
    const std::string &s_;
    size_t furthest_ = 0;
    bool orderBy_ = false, stringRanges_ = false, having_ = false, countDistinct_ = false, intLists_ = false, subqueries_ = false;
    std::string expected_ = "`select'";

    size_t skipWs(size_t i) const {
        while (i < s_.size() && std::isspace((unsigned char)s_[i])) ++i;
        return i;
    }
    void note(size_t at, const std::string &what) {
        if (at >= furthest_) { furthest_ = at; expected_ = what; }
    }
    bool lit(size_t i, const char *word, size_t &out) {
        i = skipWs(i);
        const size_t n = std::strlen(word);
        if (s_.compare(i, n, word) == 0) { out = i + n; return true; }
        note(i, std::string("`") + word + "'");
        return false;
    }
    static bool wordChar(char c) { return std::isalnum((unsigned char)c) || c == '_' || c == '#'; }
    bool ident(size_t i, std::string &val, size_t &out) { // [\w#]+ (value has the same character class)
        i = skipWs(i);
        size_t j = i;
        while (j < s_.size() && wordChar(s_[j])) ++j;
        if (j == i) { note(i, "string matching regex `[\\w\\#]+'"); return false; }
        val = s_.substr(i, j - i);
        out = j;
        return true;
    }
    static double toDouble(const std::string &v) { // String.toDouble on [\w#]+ : NumberFormatException unless numeric
        char *end = nullptr;
        const double d = std::strtod(v.c_str(), &end);
        bool ok = !v.empty() && end == v.c_str() + v.size();
        // Java's parser accepts a trailing d/D/f/F and hex floats; strtod accepts "inf"/"nan"/hex too. Keep digits-only plus those.
        if (!ok && !v.empty() && (v.back() == 'd' || v.back() == 'D' || v.back() == 'f' || v.back() == 'F')) {
            const std::string w = v.substr(0, v.size() - 1);
            const double d2 = std::strtod(w.c_str(), &end);
            if (!w.empty() && end == w.c_str() + w.size()) return d2;
        }
        if (!ok) throw Exception("NumberFormatException: For input string: \"" + v + "\"");
        return d;
    }

    // ---- filters ----
    bool filterList(size_t i, const char *sep, bool isAnd, std::shared_ptr<SelectADT> &out, size_t &end) {
        size_t p;
        if (!lit(i, "(", p)) return false;
        std::vector<std::shared_ptr<SelectADT>> xs;
        std::shared_ptr<SelectADT> f;
        size_t q;
        if (filter(p, f, q)) { // repsep: zero or more
            xs.push_back(f);
            p = q;
            for (;;) {
                size_t r;
                if (!lit(p, sep, r)) break;
                if (!filter(r, f, q)) break; // repsep backtracks over the dangling separator
                xs.push_back(f);
                p = q;
            }
        }
        if (!lit(p, ")", q)) return false;
        if (xs.empty()) throw Exception("UnsupportedOperationException: tail of empty list"); // xs.tail on Nil (:64)
        std::shared_ptr<SelectADT> acc = xs[0];
        for (size_t k = 1; k < xs.size(); ++k) acc = isAnd ? SelectADT::mkAnd(acc, xs[k]) : SelectADT::mkOr(acc, xs[k]);
        out = acc;
        end = q;
        return true;
    }
    bool filter(size_t i, std::shared_ptr<SelectADT> &out, size_t &end) {
        if (filterList(i, "and", true, out, end)) return true;  // filterAnd
        if (filterList(i, "or", false, out, end)) return true;  // filterOr
        std::string f, v;
        size_t p, q, r, t;
        if (ident(i, f, p) && lit(p, "=", q) && ident(q, v, r)) { // filterEQ
            out = SelectADT::mkSelect(f, SelectCondition::eq(toDouble(v)));
            end = r;
            return true;
        }
        if (ident(i, f, p) && lit(p, "=", q) && lit(q, "'", r) && ident(r, v, t)) { // filterEQString
            size_t u;
            if (lit(t, "'", u)) {
                out = SelectADT::mkSelect(f, SelectCondition::match({v}));
                end = u;
                return true;
            }
        }
        if (ident(i, f, p) && lit(p, ">", q) && ident(q, v, r)) { // filterGT
            out = SelectADT::mkSelect(f, SelectCondition::gt(toDouble(v)));
            end = r;
            return true;
        }
        if (ident(i, f, p) && lit(p, "<", q) && ident(q, v, r)) { // filterLT
            out = SelectADT::mkSelect(f, SelectCondition::lt(toDouble(v)));
            end = r;
            return true;
        }
        if (stringRanges_) { // filterGTString | filterLTString | filterLike
            static const struct { const char *op; int kind; const char *tail; } forms[] = {{">", 0, ""}, {"<", 1, ""}, {"like", 2, "%"}};
            for (const auto &fm : forms) {
                size_t u = 0;
                if (!(ident(i, f, p) && lit(p, fm.op, q) && lit(q, "'", r) && ident(r, v, t))) continue;
                if (*fm.tail && !lit(t, fm.tail, t)) continue;
                if (!lit(t, "'", u)) continue;
                out = SelectADT::mkSelect(f, fm.kind == 0 ? SelectCondition::strGT(v) : fm.kind == 1 ? SelectCondition::strLT(v) : SelectCondition::prefix(v));
                end = u;
                return true;
            }
        }
        if (intLists_) { // filterIn: ident "in" "(" rep1sep(int, ",") ")"
            std::vector<int32_t> ints;
            int32_t x = 0;
            if (ident(i, f, p) && lit(p, "in", q) && lit(q, "(", r) && intLiteral(r, x, t)) {
                ints.push_back(x);
                for (;;) {
                    size_t c, u;
                    if (!lit(t, ",", c) || !intLiteral(c, x, u)) break; // rep1sep backtracks over a dangling separator
                    ints.push_back(x);
                    t = u;
                }
                size_t u;
                if (lit(t, ")", u)) {
                    out = SelectADT::mkSelect(f, SelectCondition::intIn(ints));
                    end = u;
                    return true;
                }
            }
        }
        if (subqueries_) { // filterInQuery: ident "in" "(" "select" ident from where ")"
            std::string g, tbl;
            size_t s, a, b, e, u;
            if (ident(i, f, p) && lit(p, "in", q) && lit(q, "(", r) && lit(r, "select", s) && ident(s, g, a) && fromTable(a, tbl, b)) {
                Query inner;
                inner.table = tbl;
                where(b, inner.select, e);
                if (lit(e, ")", u)) {
                    inner.project.kind = ProjectADT::Project;
                    inner.project.cols = {g};
                    out = SelectADT::mkSelect(f, SelectCondition::intInQuery(inner));
                    end = u;
                    return true;
                }
            }
        }
        return false;
    }
    bool intLiteral(size_t i, int32_t &val, size_t &out) { // -?[0-9]+ ; a literal outside int32 is an error, not a parse failure
        i = skipWs(i);
        size_t j = i;
        if (j < s_.size() && s_[j] == '-') ++j;
        const size_t digits = j;
        while (j < s_.size() && s_[j] >= '0' && s_[j] <= '9') ++j;
        if (j == digits) { note(i, "string matching regex `-?[0-9]+'"); return false; }
        const std::string text = s_.substr(i, j - i);
        size_t k = digits - i; // leading zeros do not count towards the length
        while (k + 1 < text.size() && text[k] == '0') ++k;
        if (text.size() - k > 10) throw Exception(kIntListRangeError + text);
        const long long v = std::strtoll(text.c_str(), nullptr, 10);
        if (v < -2147483648LL || v > 2147483647LL) throw Exception(kIntListRangeError + text);
        val = (int32_t)v;
        out = j;
        return true;
    }
    bool where(size_t i, std::shared_ptr<SelectADT> &out, size_t &end) { // opt("where" ~> filter)
        size_t p, q;
        std::shared_ptr<SelectADT> f;
        if (lit(i, "where", p) && filter(p, f, q)) { out = f; end = q; return true; }
        out = SelectADT::noSelect();
        end = i;
        return true;
    }
    bool fromTable(size_t i, std::string &t, size_t &end) {
        size_t p;
        return lit(i, "from", p) && ident(p, t, end);
    }
    bool identList(size_t i, bool atLeastOne, std::vector<std::string> &out, size_t &end) {
        std::string f;
        size_t p;
        out.clear();
        if (!ident(i, f, p)) { end = i; return !atLeastOne; }
        out.push_back(f);
        for (;;) {
            size_t q, r;
            if (!lit(p, ",", q) || !ident(q, f, r)) break;
            out.push_back(f);
            p = r;
        }
        end = p;
        return true;
    }
    // opt("order" ~ "by" ~> rep1sep(ident ~ opt("asc" | "desc"), ",")): the position behind the clause, or i when there is none
    // an order key: ident, or -- in an aggregation (aggs) -- an aggregate call as written in the SELECT list, which names its alias
    bool orderKey(size_t i, bool aggs, std::string &name, size_t &end) {
        Aggregate a;
        if (aggs && agg(i, a, end)) { name = defaultAlias(a); return true; }
        return ident(i, name, end);
    }
    // hfilter: a parenthesised and-list / or-list of hfilters, or hkey (an ident or an aggregate call) > | < | = value
    bool hfilter(size_t i, std::shared_ptr<SelectADT> &out, size_t &end) {
        static const struct { const char *sep; bool isAnd; } lists[] = {{"and", true}, {"or", false}};
        for (const auto &l : lists) {
            size_t p, q;
            if (!lit(i, "(", p)) continue;
            std::vector<std::shared_ptr<SelectADT>> xs;
            std::shared_ptr<SelectADT> f;
            while (hfilter(p, f, q)) {
                xs.push_back(f);
                p = q;
                size_t r;
                if (!lit(p, l.sep, r)) break;
                std::shared_ptr<SelectADT> g;
                size_t u;
                if (!hfilter(r, g, u)) break; // (repsep backtracks over a dangling separator)
                p = r;
            }
            if (xs.empty() || !lit(p, ")", q)) continue;
            std::shared_ptr<SelectADT> acc = xs[0];
            for (size_t k = 1; k < xs.size(); ++k) acc = l.isAnd ? SelectADT::mkAnd(acc, xs[k]) : SelectADT::mkOr(acc, xs[k]);
            out = acc;
            end = q;
            return true;
        }
        std::string name, v;
        size_t k, q, r;
        if (!orderKey(i, true, name, k)) return false;
        static const char *ops[] = {">", "<", "="};
        for (int o = 0; o < 3; ++o)
            if (lit(k, ops[o], q) && ident(q, v, r)) {
                const double d = toDouble(v);
                out = SelectADT::mkSelect(name, o == 0 ? SelectCondition::gt(d) : (o == 1 ? SelectCondition::lt(d) : SelectCondition::eq(d)));
                end = r;
                return true;
            }
        return false;
    }
    // opt("having" hfilter): the position behind the clause, or i when there is none
    size_t havingClause(size_t i, std::shared_ptr<SelectADT> &out) {
        size_t p, q;
        std::shared_ptr<SelectADT> f;
        if (lit(i, "having", p) && hfilter(p, f, q)) { out = f; return q; }
        return i;
    }
    // opt("limit" digits): the position behind it, or d when there is none
    size_t limitClause(size_t d, int &limit) {
        size_t e;
        if (lit(d, "limit", e)) {
            size_t k = skipWs(e), j = k;
            while (j < s_.size() && std::isdigit((unsigned char)s_[j])) ++j;
            if (j > k) {
                limit = std::atoi(s_.substr(k, j - k).c_str());
                return j;
            }
        }
        return d;
    }
    size_t orderByClause(size_t i, std::vector<std::pair<std::string, bool>> &out, bool aggs = false) {
        size_t p, q;
        if (!lit(i, "order", p) || !lit(p, "by", q)) return i;
        std::vector<std::pair<std::string, bool>> keys;
        for (;;) {
            std::string f;
            size_t r, t;
            if (!orderKey(q, aggs, f, r)) break;
            bool desc = false;
            if (lit(r, "desc", t)) { desc = true; r = t; }
            else if (lit(r, "asc", t)) r = t;
            keys.push_back({f, desc});
            q = r;
            if (!lit(q, ",", t)) break;
            std::string g;
            size_t u;
            if (!orderKey(t, aggs, g, u)) break; // (rep1sep backtracks over a dangling separator)
            q = t;
        }
        if (keys.empty()) return i;
        out = keys;
        return q;
    }
    bool agg(size_t i, Aggregate &a, size_t &end) { // aggSumP | aggMinP | aggMaxP | aggCountP (:103-117)
        static const struct { const char *kw; Aggregate::Kind k; } kinds[] = {
            {"sum", Aggregate::Sum}, {"min", Aggregate::Min}, {"max", Aggregate::Max}, {"count", Aggregate::Count}};
        if (countDistinct_) { // (the opt-in: "count" "(" "distinct" ident ")")
            size_t p, q, d, r, t;
            std::string name;
            if (lit(i, "count", p) && lit(p, "(", q) && lit(q, "distinct", d) && ident(d, name, r) && lit(r, ")", t)) {
                a.kind = Aggregate::CountDistinct;
                a.col = name;
                a.alias.clear();
                end = t;
                return true;
            }
        }
        for (const auto &k : kinds) {
            size_t p, q, r, t;
            std::string name;
            if (lit(i, k.kw, p) && lit(p, "(", q) && ident(q, name, r) && lit(r, ")", t)) {
                a.kind = k.k;
                a.col = name;
                a.alias.clear();
                end = t;
                return true;
            }
        }
        return false;
    }
    bool selectProjectAgg(size_t i, ProjectADT &p, size_t &end) {
        size_t q;
        if (!lit(i, "select", q)) return false;
        Aggregate a;
        size_t r;
        if (!agg(q, a, r)) return false;
        p = ProjectADT();
        p.kind = ProjectADT::ProjectAgg;
        p.aggs.push_back(a);
        for (;;) {
            size_t c, t;
            if (!lit(r, ",", c) || !agg(c, a, t)) break;
            p.aggs.push_back(a);
            r = t;
        }
        end = r;
        return true;
    }
    bool query(size_t i, Query &out, size_t &end) {
        {   // queryProjectAgg: selectProjectAgg ~ fromTable ~ where ~ groupBy
            ProjectADT p;
            size_t a, b, c, d, e, f;
            std::string t;
            std::shared_ptr<SelectADT> w;
            if (selectProjectAgg(i, p, a) && fromTable(a, t, b) && where(b, w, c)) {
                std::vector<std::string> g;
                // parseAll: this alternative only wins if it consumes everything; otherwise Scala's `|`
                // has already committed to it (first success), and parseAll then fails on the leftovers.
                if (lit(c, "group", d) && lit(d, "by", e) && identList(e, true, g, f)) {
                    p.groupBy = g;
                    end = f;
                } else end = c; // queryProjectAggNoGroup
                if (having_) { // (the opt-in, like orderBy_ below)
                    end = havingClause(end, p.having);
                    checkGroupFilterNames(p);
                }
                if (orderBy_) { // (the opt-in: with it off the statement ends here, as in the reference)
                    end = orderByClause(end, p.orderBy, true);
                    end = limitClause(end, p.limit);
                    checkGroupOrderNames(p);
                }
                out = Query{t, w, p};
                return true;
            }
        }
        {   // queryProject: selectProject ~ fromTable ~ where ~ limit
            size_t a, b, c, d;
            std::vector<std::string> cols;
            std::string t;
            std::shared_ptr<SelectADT> w;
            if (lit(i, "select", a) && identList(a, false, cols, b) && fromTable(b, t, c) && where(c, w, d)) {
                ProjectADT p;
                p.kind = ProjectADT::Project;
                p.cols = cols;
                if (orderBy_) d = orderByClause(d, p.orderBy);
                d = limitClause(d, p.limit);
                out = Query{t, w, p};
                end = d;
                return true;
            }
        }
        return false;
    }
};

} // namespace immutabledb
