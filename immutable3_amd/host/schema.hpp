// schema.hpp -- Column / Table / TableIO / Row, mirroring core/src/main/scala/immutabledb/{Column,Table,Record}.scala
// and the Query ADT of core/src/main/scala/immutabledb/Query.scala (same names, same fields).
#pragma once

#include <dirent.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdint>
#include <fstream>
#include <map>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "json.hpp"

namespace immutabledb {

// `throw new Exception(msg)` of the reference
struct Exception : std::runtime_error {
    explicit Exception(const std::string &m) : std::runtime_error(m) {}
};

// ---- CodecType (codec/Codec.scala:21-24) / ColumnType (Column.scala:13-16) ----
// SNAPPY_* are this library's extension (include/imm3.h): blocks as SnappyCodec.encode writes them
// (codec/SnappyCodec.scala:15-43); the reference has no CodecType for them and cannot read them.
enum class CodecType : int { PFOR_INT = 0, DENSE_INT = 1, DENSE_TINYINT = 2, DENSE_STRING = 3, SNAPPY_INT = 16, SNAPPY_TINYINT = 17, SNAPPY_STRING = 18 };
inline bool isSnappy(CodecType c) { return (int)c >= 16; }
enum class ColumnType : int { INT = 0, TINYINT = 1, STRING = 2 };

inline const char *toString(CodecType c) {
    static const char *n[] = {"PFOR_INT", "DENSE_INT", "DENSE_TINYINT", "DENSE_STRING"};
    static const char *x[] = {"SNAPPY_INT", "SNAPPY_TINYINT", "SNAPPY_STRING"};
    return isSnappy(c) ? x[(int)c - 16] : n[(int)c];
}
inline const char *toString(ColumnType c) {
    static const char *n[] = {"INT", "TINYINT", "STRING"};
    return n[(int)c];
}
inline CodecType codecWithName(const std::string &s) {
    for (int i = 0; i < 4; ++i)
        if (s == toString((CodecType)i)) return (CodecType)i;
    for (int i = 16; i < 19; ++i)
        if (s == toString((CodecType)i)) return (CodecType)i;
    throw Exception("No value found for '" + s + "'"); // Enumeration.withName
}
inline ColumnType columnTypeWithName(const std::string &s) {
    for (int i = 0; i < 3; ++i)
        if (s == toString((ColumnType)i)) return (ColumnType)i;
    throw Exception("No value found for '" + s + "'");
}

// ---- Column (Column.scala:18-63) ----
struct Column {
    std::string name;
    ColumnType columnType = ColumnType::INT;
    CodecType codec = CodecType::DENSE_INT;
    std::vector<std::pair<std::string, std::string>> dtypeAttrs; // Map[String, String]

    static Column make(const std::string &name, CodecType codec, std::vector<std::pair<std::string, std::string>> attrs = {}) {
        Column c;
        c.name = name;
        c.codec = codec;
        c.dtypeAttrs = std::move(attrs);
        switch (codec) {
        case CodecType::DENSE_INT:
        case CodecType::SNAPPY_INT:
        case CodecType::PFOR_INT: c.columnType = ColumnType::INT; break;
        case CodecType::SNAPPY_TINYINT:
        case CodecType::DENSE_TINYINT: c.columnType = ColumnType::TINYINT; break;
        case CodecType::SNAPPY_STRING:
        case CodecType::DENSE_STRING: c.columnType = ColumnType::STRING; break;
        }
        return c;
    }
    std::string attr(const std::string &k) const {
        for (const auto &kv : dtypeAttrs)
            if (kv.first == k) return kv.second;
        throw Exception("key not found: " + k);
    }
    // dtype.size of Column.getCodec(column) (Column.scala:57-63; DataType.scala:34,54,64)
    int width() const {
        switch (codec) {
        case CodecType::DENSE_INT:
        case CodecType::SNAPPY_INT:
        case CodecType::PFOR_INT: return 4;
        case CodecType::SNAPPY_TINYINT:
        case CodecType::DENSE_TINYINT: return 1;
        case CodecType::SNAPPY_STRING:
        case CodecType::DENSE_STRING: return std::stoi(attr("size"));
        }
        throw Exception("");
    }
    bool operator==(const Column &o) const { return name == o.name && columnType == o.columnType && codec == o.codec && dtypeAttrs == o.dtypeAttrs; }

    json::Value toJsonValue() const { // Column.scala:21-29
        json::Value v = json::Value::object();
        v.put("name", json::Value::string(name));
        v.put("columnType", json::Value::string(toString(columnType)));
        v.put("codec", json::Value::string(toString(codec)));
        json::Value a = json::Value::object();
        for (const auto &kv : dtypeAttrs) a.put(kv.first, json::Value::string(kv.second));
        v.put("dtypeAttrs", a);
        return v;
    }
    static Column fromJsonValue(const json::Value &j) { // Column.scala:31-38
        Column c;
        c.name = j.at("name").str;
        c.columnType = columnTypeWithName(j.at("columnType").str);
        c.codec = codecWithName(j.at("codec").str);
        for (const auto &kv : j.at("dtypeAttrs").obj) c.dtypeAttrs.emplace_back(kv.first, kv.second.str);
        return c;
    }
};

// ---- Table / TableIO (Table.scala:9-66) ----
struct Table {
    std::string name;
    std::vector<Column> columns;
    int blockSize = 1024;

    const Column &getColumn(const std::string &colName) const {
        for (const auto &c : columns)
            if (c.name == colName) return c;
        throw Exception("Column " + colName + " does not exist in table " + name);
    }
    int columnIndex(const std::string &colName) const {
        for (size_t i = 0; i < columns.size(); ++i)
            if (columns[i].name == colName) return (int)i;
        throw Exception("Column " + colName + " does not exist in table " + name);
    }
};

inline std::string readFile(const std::string &path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw Exception(path + " (No such file or directory)");
    std::ostringstream ss;
    ss << f.rdbuf();
    return ss.str();
}

inline void mkdirs(const std::string &path) {
    std::string cur;
    for (size_t i = 0; i <= path.size(); ++i) {
        if (i == path.size() || path[i] == '/') {
            if (!cur.empty()) ::mkdir(cur.c_str(), 0777);
        }
        if (i < path.size()) cur += path[i];
    }
}

inline std::vector<std::string> listDir(const std::string &path, bool dirsOnly) {
    std::vector<std::string> out;
    DIR *d = ::opendir(path.c_str());
    if (!d) return out;
    while (struct dirent *e = ::readdir(d)) {
        const std::string n = e->d_name;
        if (n == "." || n == "..") continue;
        struct stat st {};
        if (::stat((path + "/" + n).c_str(), &st) != 0) continue;
        if (dirsOnly ? S_ISDIR(st.st_mode) : S_ISREG(st.st_mode)) out.push_back(n);
    }
    ::closedir(d);
    return out;
}

struct TableIO {
    static constexpr const char *fileName = "_table.meta";

    static json::Value toJsonValue(const Table &t) { // Table.scala:29-35
        json::Value v = json::Value::object();
        v.put("name", json::Value::string(t.name));
        json::Value cols = json::Value::array();
        for (const auto &c : t.columns) cols.arr.push_back(c.toJsonValue());
        v.put("columns", cols);
        v.put("blockSize", json::Value::number(t.blockSize));
        return v;
    }
    static Table fromJsonValue(const json::Value &j) { // Table.scala:37-43
        Table t;
        t.name = j.at("name").str;
        for (const auto &c : j.at("columns").arr) t.columns.push_back(Column::fromJsonValue(c));
        t.blockSize = (int)j.at("blockSize").num;
        return t;
    }
    static Table load(const std::string &dataDir, const std::string &tableName) {
        return fromJsonValue(json::parse(readFile(dataDir + "/" + tableName + "/" + fileName)));
    }
    static void store(const std::string &dataDir, const Table &t) {
        const std::string path = dataDir + "/" + t.name;
        mkdirs(path);
        std::ofstream f(path + "/" + fileName, std::ios::binary | std::ios::trunc);
        f << json::dump(toJsonValue(t));
    }
    static void clear(const std::string &dataDir, const Table &t) { // Table.scala:61-66: delete the table's files
        const std::string path = dataDir + "/" + t.name;
        for (const auto &f : listDir(path, false)) ::unlink((path + "/" + f).c_str());
    }
};

// ---- Row (Record.scala:7-14): boxed Int / Byte / String values ----
struct Value {
    enum Kind { Int, Byte, String } kind = Int;
    int32_t i = 0;
    std::string s;
    static Value ofInt(int32_t v) { Value x; x.kind = Int; x.i = v; return x; }
    static Value ofByte(int8_t v) { Value x; x.kind = Byte; x.i = v; return x; }
    static Value ofString(std::string v) { Value x; x.kind = String; x.s = std::move(v); return x; }
    std::string toString() const { return kind == String ? s : std::to_string(i); }
    bool operator==(const Value &o) const { return kind == o.kind && i == o.i && s == o.s; }
};

struct Row {
    std::vector<Value> xs;
    static Row fromSeq(std::vector<Value> v) { Row r; r.xs = std::move(v); return r; }
    int8_t getByte(size_t idx) const { return (int8_t)xs.at(idx).i; }
    int32_t getInt(size_t idx) const { return xs.at(idx).i; }
    const std::string &getString(size_t idx) const { return xs.at(idx).s; }
    std::string toString() const { // xs.mkString("Row(", ",", ")")
        std::string out = "Row(";
        for (size_t k = 0; k < xs.size(); ++k) {
            if (k) out += ",";
            out += xs[k].toString();
        }
        return out + ")";
    }
};

// ---- Query ADT (Query.scala:3-46) ----
struct Query;
inline std::string showInnerQuery(const Query &q); // (defined behind Query: an IntInQuery condition prints its inner statement)
struct SelectCondition {
    // Match .. NoOp: same order as IMM3_MATCH .. IMM3_NOOP.  EXTENSION, behind them: byte-order ranges on a string column (include/imm3.h:
    // IMM3_STR_RANGE; the order of ORDER BY and the string MAX aggregate -- unsigned, byte-wise, from the first byte).  StrRange(lo, hi)
    // is closed, lo padded to the column's width with 0x00 and hi with 0xFF; Prefix(p) = StrRange(p, p); StrGT(v) / StrLT(v) are strict,
    // relative to v padded with 0x00.
    // EXTENSION, behind those: IntIn(values), an IN-list on an int32 / int8 column (include/imm3.h: IMM3_INT_IN) -- exact integer
    // membership, duplicates once, an empty list selects nothing; not under an Or or a NotMatch-as-NOT tree (the library refuses it).
    // EXTENSION, behind that: IntInQuery(query), IN (sub-query) -- the rows whose value is one the inner query's column takes among the
    // rows it selects (include/imm3.h: IMM3_INT_IN_SET).  The inner query is a plain projection of exactly one int32 / int8 column
    // with a where tree: an aggregation, an order by or a limit inside is refused (intInQuery).  Engine::execute resolves it to
    // IntInSet(set) -- the device-resident set built from the inner selection (imm3_int_set_create) -- which is what the operators see.
    enum Kind { Match, NotMatch, EQ, GT, LT, NoOp, StrRange, Prefix, StrGT, StrLT, IntIn, IntInQuery, IntInSet } kind = NoOp;
    double value = 0;                 // EQ / GT / LT
    std::vector<std::string> values;  // Match / NotMatch; StrRange: {lo, hi}; Prefix / StrGT / StrLT: {the value}
    std::vector<int32_t> ints;        // IntIn
    std::shared_ptr<Query> inner;     // IntInQuery
    std::shared_ptr<void> set;        // IntInSet: the imm3_int_set handle (destroyed with the last condition that holds it)
    static inline SelectCondition intInQuery(const Query &q); // (defined behind Query)
    static SelectCondition intInSet(std::shared_ptr<void> handle) { SelectCondition c; c.kind = IntInSet; c.set = std::move(handle); return c; }
    static SelectCondition intIn(std::vector<int32_t> v) { SelectCondition c; c.kind = IntIn; c.ints = std::move(v); return c; }
    static SelectCondition strRange(std::string lo, std::string hi) { SelectCondition c; c.kind = StrRange; c.values = {std::move(lo), std::move(hi)}; return c; }
    static SelectCondition prefix(std::string p) { SelectCondition c; c.kind = Prefix; c.values = {std::move(p)}; return c; }
    static SelectCondition strGT(std::string v) { SelectCondition c; c.kind = StrGT; c.values = {std::move(v)}; return c; }
    static SelectCondition strLT(std::string v) { SelectCondition c; c.kind = StrLT; c.values = {std::move(v)}; return c; }
    bool isStrRange() const { return kind >= StrRange && kind <= StrLT; }
    // what the C ABI's leaf carries: the condition code (a range form: 6, IMM3_STR_RANGE) and the values -- of a range form the leaf's
    // {lo, hi} on a string column of `width` bytes.  StrGT(v) is from the successor of v padded with 0x00 on, StrLT(v) up to its
    // predecessor (big-endian arithmetic over the column's width); where there is none the leaf is one no row passes (lo 01, hi 00:
    // 01 00 00 .. > 00 FF FF ..).  A bound longer than the column throws (the library refuses it too).
    // An IntIn leaf (7, IMM3_INT_IN) carries each value as its 4 little-endian bytes: concatenated they are the leaf's match_bytes.
    // An IntInSet leaf (8, IMM3_INT_IN_SET) carries no values: its match_bytes is the handle itself, n_match 1 (operators.hpp: setLeaf).
    int32_t abiCond() const { return kind == IntInSet ? 8 : (kind == IntIn ? 7 : (isStrRange() ? 6 : (int32_t)kind)); }
    std::vector<std::string> abiValues(int width) const {
        if (kind == IntIn) {
            std::vector<std::string> out;
            for (int32_t v : ints) {
                const uint32_t u = (uint32_t)v;
                out.push_back(std::string{(char)(u & 255), (char)((u >> 8) & 255), (char)((u >> 16) & 255), (char)(u >> 24)});
            }
            return out;
        }
        if (!isStrRange()) return values;
        for (const auto &b : values)
            if ((int)b.size() > width) throw Exception("string bound '" + b + "' is longer than the column's " + std::to_string(width) + " bytes");
        if (kind == StrRange) return values;
        if (kind == Prefix) return {values[0], values[0]};
        std::string v = values[0];
        v.resize((size_t)std::max(width, 0), '\0');
        size_t i = v.size();
        if (kind == StrGT) {
            while (i > 0 && (unsigned char)v[i - 1] == 0xFF) --i;
            if (i == 0) return {std::string("\x01"), std::string(1, '\0')};
            v[i - 1] = (char)((unsigned char)v[i - 1] + 1);
            for (size_t k = i; k < v.size(); ++k) v[k] = '\0';
            return {v, std::string()};
        }
        while (i > 0 && (unsigned char)v[i - 1] == 0x00) --i;
        if (i == 0) return {std::string("\x01"), std::string(1, '\0')};
        v[i - 1] = (char)((unsigned char)v[i - 1] - 1);
        for (size_t k = i; k < v.size(); ++k) v[k] = (char)0xFF;
        return {std::string(), v};
    }
    static SelectCondition match(std::vector<std::string> v) { SelectCondition c; c.kind = Match; c.values = std::move(v); return c; }
    static SelectCondition notMatch(std::vector<std::string> v) { SelectCondition c; c.kind = NotMatch; c.values = std::move(v); return c; }
    static SelectCondition eq(double d) { SelectCondition c; c.kind = EQ; c.value = d; return c; }
    static SelectCondition gt(double d) { SelectCondition c; c.kind = GT; c.value = d; return c; }
    static SelectCondition lt(double d) { SelectCondition c; c.kind = LT; c.value = d; return c; }
    std::string toString() const {
        auto list = [&]() { std::string s = "List("; for (size_t i = 0; i < values.size(); ++i) { if (i) s += ", "; s += values[i]; } return s + ")"; };
        std::ostringstream d;
        d << value;
        switch (kind) {
        case Match: return "Match(" + list() + ")";
        case NotMatch: return "NotMatch(" + list() + ")";
        case EQ: return "EQ(" + d.str() + ")";
        case GT: return "GT(" + d.str() + ")";
        case LT: return "LT(" + d.str() + ")";
        case StrRange: return "StrRange(" + values[0] + "," + values[1] + ")";
        case Prefix: return "Prefix(" + values[0] + ")";
        case StrGT: return "StrGT(" + values[0] + ")";
        case StrLT: return "StrLT(" + values[0] + ")";
        case IntIn: { std::string s = "IntIn(List("; for (size_t i = 0; i < ints.size(); ++i) s += (i ? ", " : "") + std::to_string(ints[i]); return s + "))"; }
        case IntInQuery: return "IntInQuery(" + showInnerQuery(*inner) + ")";
        case IntInSet: return "IntInSet";
        default: return "NoOp";
        }
    }
};

struct SelectADT {
    enum Kind { And, Or, Select, NoSelect } kind = NoSelect;
    std::shared_ptr<SelectADT> op1, op2; // And / Or
    std::string col;                     // Select
    SelectCondition cond;
    static std::shared_ptr<SelectADT> mkAnd(std::shared_ptr<SelectADT> a, std::shared_ptr<SelectADT> b) { auto s = std::make_shared<SelectADT>(); s->kind = And; s->op1 = a; s->op2 = b; return s; }
    static std::shared_ptr<SelectADT> mkOr(std::shared_ptr<SelectADT> a, std::shared_ptr<SelectADT> b) { auto s = std::make_shared<SelectADT>(); s->kind = Or; s->op1 = a; s->op2 = b; return s; }
    static std::shared_ptr<SelectADT> mkSelect(const std::string &c, SelectCondition cond) { auto s = std::make_shared<SelectADT>(); s->kind = Select; s->col = c; s->cond = std::move(cond); return s; }
    static std::shared_ptr<SelectADT> noSelect() { return std::make_shared<SelectADT>(); }
};

struct Aggregate { // Query.scala:17-26
    enum Kind { Sum, Avg, Min, Max, Count, CountDistinct } kind = Count; // CountDistinct: not in the reference -- count(distinct col), SQLParser's opt-in
    std::string col;
    std::string alias; // empty = None
};

// the alias Engine.resolveProjectOp gives an aggregate without one (Engine.scala:130-156): <col>_max / _min / _count; a CountDistinct: <col>_distinct
inline std::string defaultAlias(const Aggregate &a) {
    static const char *suffix[] = {"sum", "avg", "min", "max", "count", "distinct"};
    return a.alias.empty() ? a.col + "_" + suffix[a.kind] : a.alias;
}

struct ProjectADT {
    enum Kind { Project, ProjectAgg, NoProject } kind = NoProject;
    std::vector<std::string> cols; // Project
    int limit = 0;                 // ProjectAgg: > 0 keeps the first `limit` groups of the order (without an order: of the first-seen order)
    // (name, descending), most significant first -- the "sort" Query.scala:27 announces; empty: none.  Project: a SELECT-list column;
    // ProjectAgg: a group-by column or an aggregate's alias (imm3_query_set_group_order)
    std::vector<std::pair<std::string, bool>> orderBy;
    std::vector<Aggregate> aggs;   // ProjectAgg
    std::vector<std::string> groupBy;
    // ProjectAgg: HAVING -- And / Or over Select(alias, GT | LT | EQ); null: none.  The groups kept, BEFORE the order and the limit
    // (imm3_query_set_group_filter)
    std::shared_ptr<SelectADT> having;
};

// A HAVING tree checked against an aggregation's aliases and group-by columns and flattened: the leaves (alias, condition code --
// SelectCondition::EQ / GT / LT, the C ABI's IMM3_EQ / IMM3_GT / IMM3_LT --, integer threshold) and the postfix program over their
// indices with -1 = and, -2 = or (IMM3_EXPR_AND / IMM3_EXPR_OR).  Refused: a name that is no alias, a group-by column (rows are
// filtered by the where clause), a condition other than GT / LT / EQ, a threshold that is no integer (aggregates are compared exactly).
struct GroupFilterLeaf {
    std::string alias;
    int cond;
    long long value;
    bool average = false; // an average's alias: sum <cond> value * count (no aggregator of this host layer is one)
};
inline void groupFilterLeaves(const std::vector<std::string> &aliases, const std::vector<std::string> &groupBy, const SelectADT *having,
                              std::vector<GroupFilterLeaf> &leaves, std::vector<int32_t> &prog) {
    if (!having) return;
    if (having->kind == SelectADT::And || having->kind == SelectADT::Or) {
        groupFilterLeaves(aliases, groupBy, having->op1.get(), leaves, prog);
        groupFilterLeaves(aliases, groupBy, having->op2.get(), leaves, prog);
        prog.push_back(having->kind == SelectADT::And ? -1 : -2);
        return;
    }
    if (having->kind != SelectADT::Select) throw Exception("having: neither And, Or nor Select");
    const std::string &name = having->col;
    for (const auto &g : groupBy)
        if (g == name) throw Exception("having `" + name + "': a group-by column is filtered by the select (where), not by having");
    bool found = false;
    for (const auto &a : aliases) found = found || a == name;
    if (!found) throw Exception("having `" + name + "' is not an aggregate's alias");
    const SelectCondition &c = having->cond;
    if (c.kind != SelectCondition::GT && c.kind != SelectCondition::LT && c.kind != SelectCondition::EQ)
        throw Exception("having `" + name + "': the condition must be GT, LT or EQ");
    if (!(c.value >= -9.2e18 && c.value <= 9.2e18) || (double)(long long)c.value != c.value)
        throw Exception("having `" + name + "': the threshold is not an integer (aggregates are compared exactly)");
    prog.push_back((int32_t)leaves.size());
    leaves.push_back(GroupFilterLeaf{name, (int)c.kind, (long long)c.value});
}
inline void checkGroupFilterNames(const ProjectADT &p) {
    std::vector<std::string> aliases;
    for (const auto &a : p.aggs) aliases.push_back(defaultAlias(a));
    std::vector<GroupFilterLeaf> leaves;
    std::vector<int32_t> prog;
    groupFilterLeaves(aliases, p.groupBy, p.having.get(), leaves, prog);
}

// ORDER BY entries of an aggregation checked against its group-by columns and its aggregates' aliases: a name that is neither is refused,
// and so is an average (ordering by a quotient is out of scope: include/imm3.h).  A name that is both means the group column.
inline void checkGroupOrderNames(const ProjectADT &p) {
    for (const auto &k : p.orderBy) {
        bool found = false;
        for (const auto &g : p.groupBy) found = found || g == k.first;
        if (found) continue;
        for (const auto &a : p.aggs)
            if (defaultAlias(a) == k.first) {
                if (a.kind == Aggregate::Avg) throw Exception("order by `" + k.first + "': ordering by an average is not supported");
                found = true;
            }
        if (!found) throw Exception("order by `" + k.first + "' is neither a group-by column nor an aggregate's alias");
    }
}

// ORDER BY keys as places in the SELECT list: (index into cols, descending).  A key that is not a SELECT-list column is refused.
inline std::vector<std::pair<int, bool>> orderKeys(const std::vector<std::string> &cols, const std::vector<std::pair<std::string, bool>> &orderBy) {
    std::vector<std::pair<int, bool>> out;
    for (const auto &k : orderBy) {
        int idx = -1;
        for (size_t j = 0; j < cols.size() && idx < 0; ++j)
            if (cols[j] == k.first) idx = (int)j;
        if (idx < 0) throw Exception("order by column `" + k.first + "' is not in the SELECT list");
        out.push_back({idx, k.second});
    }
    return out;
}
// rows ordered by such keys: Int / Byte values as signed integers, strings byte-wise unsigned; stable (equal keys keep their order)
inline bool rowBefore(const Row &a, const Row &b, const std::vector<std::pair<int, bool>> &keys) {
    for (const auto &k : keys) {
        const Value &x = a.xs.at((size_t)k.first), &y = b.xs.at((size_t)k.first);
        int c = 0;
        if (x.kind == Value::String) c = x.s.compare(y.s);
        else c = x.i < y.i ? -1 : (x.i > y.i ? 1 : 0);
        if (c != 0) return k.second ? c > 0 : c < 0;
    }
    return false;
}

struct Query {
    std::string table;
    std::shared_ptr<SelectADT> select;
    ProjectADT project;
};

inline std::string showSelectADT(const SelectADT &s) {
    switch (s.kind) {
    case SelectADT::And: return "And(" + showSelectADT(*s.op1) + "," + showSelectADT(*s.op2) + ")";
    case SelectADT::Or: return "Or(" + showSelectADT(*s.op1) + "," + showSelectADT(*s.op2) + ")";
    case SelectADT::Select: return "Select(" + s.col + "," + s.cond.toString() + ")";
    default: return "NoSelect";
    }
}
// an IntInQuery's inner statement: always a projection of one column without a limit
inline std::string showInnerQuery(const Query &q) {
    return "Query(" + q.table + "," + showSelectADT(*q.select) + ",Project(List(" + (q.project.cols.empty() ? std::string() : q.project.cols[0]) + "),0))";
}
inline SelectCondition SelectCondition::intInQuery(const Query &q) {
    if (q.project.kind != ProjectADT::Project) throw Exception("IntInQuery: the inner query is an aggregation; it must be a plain projection of one column");
    if (q.project.cols.size() != 1) throw Exception("IntInQuery: the inner query must project exactly one column, not " + std::to_string(q.project.cols.size()));
    if (!q.project.orderBy.empty()) throw Exception("IntInQuery: the inner query has an order by; the set is its whole selection, unordered");
    if (q.project.limit != 0) throw Exception("IntInQuery: the inner query has a limit; the set is its whole selection");
    SelectCondition c;
    c.kind = IntInQuery;
    c.inner = std::make_shared<Query>(q);
    return c;
}

} // namespace immutabledb
