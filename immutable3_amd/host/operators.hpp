// operators.hpp -- GPU-backed Operator / ScanOp / SelectOp / ProjectOp / Engine: the C++ host-side mirror of the
// reference's operator package above the C ABI (include/imm3.h).  Same names, argument meaning and error texts:
//
//   engine/src/main/scala/immutabledb/engine/operator/Operator.scala:14-28   Operator / ColumnVectorOperator / ProjectionOperator
//   engine/src/main/scala/immutabledb/engine/operator/Scan.scala:10-73       ScanOp, mkScanOp
//   engine/src/main/scala/immutabledb/engine/operator/Select.scala:5-165     SelectOp, mkSelectOp
//   engine/src/main/scala/immutabledb/engine/operator/Project.scala:8-81     ProjectOp, mkProjectOp
//   engine/src/main/scala/immutabledb/engine/Engine.scala:85-128,158-262     getColumns / resolveSelectOps / execute
//   core/src/main/scala/immutabledb/DataVector.scala:15-48                   ColumnVectorBatch family
//
// Operators are plan builders: the first iterator() call fuses ScanOp -> SelectOp* (-> ProjectOp) of one segment
// into one imm3_query.  Everything that touches data goes through the C ABI; there is no CPU evaluation path.
#pragma once

#include <algorithm>
#include <cstring>
#include <functional>
#include <memory>

#include "../../include/imm3.h"
#include "../../include/imm3_diag.h" // (imm3_query_expr_form, for Engine::lastPath)
#include "storage.hpp"
#include "scala_sets.hpp"

namespace immutabledb {

inline void imm3Check(int rc) {
    if (rc != IMM3_OK) throw Exception(imm3_last_error());
}
// an _table_expr entry point refused a select tree because it does not fit the one table launch (imm3.h: the message prefix is the
// contract) -- the one creation error that per-segment queries answer; any other IMM3_ERR_ARG is a real argument error
inline bool tableTreeRefused(int rc) {
    return rc == IMM3_ERR_ARG && std::strncmp(imm3_last_error(), IMM3_TABLE_TREE_REFUSED, sizeof(IMM3_TABLE_TREE_REFUSED) - 1) == 0;
}

// ---- vectors (DataVector.scala) ----
struct BitSet { // scala.collection.mutable.BitSet over the GPU's words: bit i <-> word i>>6, bit i&63
    std::vector<uint64_t> words;
    bool contains(int i) const { return (size_t)(i >> 6) < words.size() && ((words[(size_t)(i >> 6)] >> (i & 63)) & 1ULL); }
    int size() const { int c = 0; for (uint64_t w : words) c += __builtin_popcountll(w); return c; }
    bool isEmpty() const { for (uint64_t w : words) if (w) return false; return true; }
    std::vector<int> toList() const {
        std::vector<int> out;
        for (size_t k = 0; k < words.size(); ++k)
            for (uint64_t w = words[k]; w; w &= w - 1) out.push_back((int)(k * 64 + (size_t)__builtin_ctzll(w)));
        return out;
    }
};

struct ColumnVector { // Int / TinyInt / String column vector: a typed VIEW of the block (DENSE decode is a reinterpretation)
    ColumnType type = ColumnType::INT;
    const uint8_t *data = nullptr;
    int width = 4;
    int n = 0;
    std::shared_ptr<std::vector<uint8_t>> owner; // PFOR_INT: the column decoded by the GPU (data points into it)
    Value value(int pos) const {
        switch (type) {
        case ColumnType::INT: { int32_t v; std::memcpy(&v, data + (size_t)pos * 4, 4); return Value::ofInt(v); }
        case ColumnType::TINYINT: return Value::ofByte((int8_t)data[pos]);
        default: return Value::ofString(std::string((const char *)data + (size_t)pos * (size_t)width, (size_t)width)); // new String(bytes)
        }
    }
};

struct ColumnVectorBatch { // FilledColumnVectorBatch (DataVector.scala:24-31)
    int oid = 0;
    int size = 0;
    std::vector<ColumnVector> columnVectors;
    std::vector<Column> columns;
    BitSet selected;
    bool selectedInUse = true;
};

// ---- pull iterators (scala Iterator) ----
template <typename A>
struct Iterator {
    virtual ~Iterator() = default;
    virtual bool hasNext() = 0;
    virtual A next() = 0;
};

template <typename A>
struct Operator { // Operator.scala:14-16
    virtual ~Operator() = default;
    virtual std::unique_ptr<Iterator<A>> iterator() = 0;
};
using ColumnVectorOperator = Operator<ColumnVectorBatch>; // Operator.scala:18-20
using ProjectionOperator = Operator<Row>;                 // Operator.scala:26-28

template <typename A>
struct VectorIterator : Iterator<A> {
    std::vector<A> items;
    size_t pos = 0;
    bool hasNext() override { return pos < items.size(); }
    A next() override { return std::move(items[pos++]); }
};

// ---- device-resident SegmentManager ----
class GpuSegmentManager {
  public:
    explicit GpuSegmentManager(const SegmentManager &sm, int device = 0) : sm(sm) { imm3Check(imm3_ctx_create(device, nullptr, &ctx_)); }
    ~GpuSegmentManager() {
        for (auto &kv : tables_) imm3_table_destroy(kv.second);
        for (auto &kv : segs_) imm3_segment_destroy(kv.second);
        imm3_ctx_destroy(ctx_);
    }
    // every segment of the table as ONE scan unit (imm3_table), or nullptr when the table cannot take the
    // single-launch path (ragged segments): callers then fall back to one pipeline per segment
    imm3_table *deviceTable(const std::string &tableName) {
        auto it = tables_.find(tableName);
        if (it != tables_.end()) return it->second;
        std::vector<const imm3_segment *> segs;
        const int n = sm.getTableSegmentCount(tableName);
        for (int s = 0; s < n; ++s) segs.push_back(deviceSegment(tableName, s));
        imm3_table *t = nullptr;
        if (!segs.empty()) {
            const int rc = imm3_table_create(ctx_, segs.data(), (int32_t)segs.size(), &t);
            if (rc != IMM3_OK && rc != IMM3_ERR_LAYOUT) throw Exception(imm3_last_error());
            if (rc != IMM3_OK) t = nullptr;
        }
        tables_[tableName] = t;
        return t;
    }
    GpuSegmentManager(const GpuSegmentManager &) = delete;
    GpuSegmentManager &operator=(const GpuSegmentManager &) = delete;

    imm3_ctx *ctx() const { return ctx_; }
    // all columns of one segment id, staged into HBM once (SegmentManager keeps its mmaps the same way)
    imm3_segment *deviceSegment(const std::string &tableName, int segIdx) {
        const auto key = std::make_pair(tableName, segIdx);
        auto it = segs_.find(key);
        if (it != segs_.end()) return it->second;
        const Table &t = sm.getTable(tableName);
        std::vector<imm3_column> cols(t.columns.size());
        for (size_t i = 0; i < t.columns.size(); ++i) {
            const std::string k = tableName + "." + t.columns[i].name;
            const MappedFile &f = sm.segments.at(k).at((size_t)segIdx);
            const SegmentMeta &m = sm.segmentsMeta.at(k).at((size_t)segIdx);
            cols[i].codec = (int32_t)t.columns[i].codec;
            cols[i].width = t.columns[i].width();
            cols[i].dat = f.data;
            cols[i].dat_bytes = f.size;
            cols[i].block_offsets = m.blockOffsets.data();
            cols[i].n_offsets = (int32_t)m.blockOffsets.size();
        }
        imm3_segment *seg = nullptr;
        imm3Check(imm3_segment_create(ctx_, cols.data(), (int32_t)cols.size(), &seg));
        segs_[key] = seg;
        return seg;
    }
    const SegmentManager &sm;

  private:
    imm3_ctx *ctx_ = nullptr;
    std::map<std::pair<std::string, int>, imm3_segment *> segs_;
    std::map<std::string, imm3_table *> tables_;
};

struct Leaf { std::string col; SelectCondition cond; };
// an IntInSet leaf carries the set's handle where the other leaves carry their values' bytes (include/imm3.h: IMM3_INT_IN_SET)
inline void setLeaf(imm3_select &s, const SelectCondition &c) {
    if (c.kind != SelectCondition::IntInSet) return;
    s.match_bytes = (const uint8_t *)c.set.get();
    s.match_lens = nullptr;
    s.n_match = 1;
}

// RAII imm3_query
struct QueryHandle {
    imm3_query *q = nullptr;
    ~QueryHandle() { if (q) imm3_query_destroy(q); }
};

// ---- ScanOp (Scan.scala:17) ----
class ScanOp : public ColumnVectorOperator {
  public:
    ScanOp(GpuSegmentManager &sm, int segIdx, const std::string &tableName, std::vector<Column> cols)
        : sm_(sm), segIdx_(segIdx), tableName_(tableName), cols_(std::move(cols)) {}
    static std::function<std::shared_ptr<ScanOp>(const std::vector<Column> &, int)> mkScanOp(GpuSegmentManager &sm, const std::string &tableName) {
        return [&sm, tableName](const std::vector<Column> &cols, int segIdx) { return std::make_shared<ScanOp>(sm, segIdx, tableName, cols); };
    }
    const Table &table() const { return sm_.sm.getTable(tableName_); }
    GpuSegmentManager &manager() const { return sm_; }

    // builds the fused query: leaves in application order, optional projection.  `prog`: the leaves are those of a select TREE and
    // this is its postfix program (include/imm3.h: imm3_query_create_expr), AND / OR honoured; null: the leaves are a conjunction
    void makeQuery(const std::vector<Leaf> &leaves, const std::vector<std::string> &projNames, int limit, QueryHandle &h, const std::vector<int32_t> *prog = nullptr) const {
        const Table &t = table();
        std::vector<int32_t> used;
        for (const auto &c : cols_) used.push_back(t.columnIndex(c.name));
        auto usedIndex = [&](const std::string &name) -> int32_t {
            for (size_t i = 0; i < cols_.size(); ++i)
                if (cols_[i].name == name) return (int32_t)i; // `.filter(_.name == col).head`, Select.scala:60
            throw Exception("NoSuchElementException: next on empty iterator");
        };
        std::vector<imm3_select> sels(leaves.size());
        std::vector<std::string> blobs(leaves.size());
        std::vector<std::vector<int32_t>> lens(leaves.size());
        for (size_t i = 0; i < leaves.size(); ++i) {
            sels[i] = imm3_select{};
            sels[i].column = usedIndex(leaves[i].col);
            sels[i].cond = leaves[i].cond.abiCond();
            sels[i].value = leaves[i].cond.value;
            for (const auto &v : leaves[i].cond.abiValues(cols_[(size_t)sels[i].column].width())) { blobs[i] += v; lens[i].push_back((int32_t)v.size()); }
            sels[i].match_bytes = (const uint8_t *)blobs[i].data();
            sels[i].match_lens = lens[i].data();
            sels[i].n_match = (int32_t)lens[i].size();
            setLeaf(sels[i], leaves[i].cond);
        }
        std::vector<int32_t> proj;
        for (const auto &n : projNames) {
            bool found = false;
            for (size_t i = 0; i < cols_.size() && !found; ++i)
                if (cols_[i].name == n) { proj.push_back((int32_t)i); found = true; }
            if (!found) throw Exception("NoSuchElementException: key not found: " + n); // vecCols(col), Project.scala:56
        }
        if (prog)
            imm3Check(imm3_query_create_expr(sm_.ctx(), sm_.deviceSegment(tableName_, segIdx_), used.data(), (int32_t)used.size(), sels.data(), (int32_t)sels.size(),
                                             prog->data(), (int32_t)prog->size(), proj.data(), (int32_t)proj.size(), limit, t.blockSize, &h.q));
        else
        imm3Check(imm3_query_create(sm_.ctx(), sm_.deviceSegment(tableName_, segIdx_), used.data(), (int32_t)used.size(),
                                    sels.data(), (int32_t)sels.size(), proj.data(), (int32_t)proj.size(), limit, t.blockSize, &h.q));
    }

    void makeAggQuery(const std::vector<Leaf> &leaves, const std::vector<int32_t> &group, const std::vector<imm3_aggregate> &aggs, QueryHandle &h,
                      const std::vector<int32_t> *prog = nullptr) const {
        const Table &t = table();
        std::vector<int32_t> used;
        for (const auto &c : cols_) used.push_back(t.columnIndex(c.name));
        std::vector<imm3_select> sels(leaves.size());
        std::vector<std::string> blobs(leaves.size());
        std::vector<std::vector<int32_t>> lens(leaves.size());
        for (size_t i = 0; i < leaves.size(); ++i) {
            sels[i] = imm3_select{};
            sels[i].column = -1;
            for (size_t k = 0; k < cols_.size(); ++k) if (cols_[k].name == leaves[i].col) { sels[i].column = (int32_t)k; break; }
            if (sels[i].column < 0) throw Exception("NoSuchElementException: next on empty iterator");
            sels[i].cond = leaves[i].cond.abiCond();
            sels[i].value = leaves[i].cond.value;
            for (const auto &v : leaves[i].cond.abiValues(cols_[(size_t)sels[i].column].width())) { blobs[i] += v; lens[i].push_back((int32_t)v.size()); }
            sels[i].match_bytes = (const uint8_t *)blobs[i].data();
            sels[i].match_lens = lens[i].data();
            sels[i].n_match = (int32_t)lens[i].size();
            setLeaf(sels[i], leaves[i].cond);
        }
        int keyBytes = 0; // a group key wider than 8 bytes: the _wide entry point
        for (int32_t g : group) keyBytes += cols_[(size_t)g].width();
        if (prog) { // (one entry point for narrow and wide keys)
            imm3Check(imm3_query_create_agg_expr(sm_.ctx(), sm_.deviceSegment(tableName_, segIdx_), used.data(), (int32_t)used.size(), sels.data(), (int32_t)sels.size(),
                                                 prog->data(), (int32_t)prog->size(), group.data(), (int32_t)group.size(), aggs.data(), (int32_t)aggs.size(), t.blockSize, &h.q));
            return;
        }
        imm3Check((keyBytes > 8 ? imm3_query_create_agg_wide : imm3_query_create_agg)(
            sm_.ctx(), sm_.deviceSegment(tableName_, segIdx_), used.data(), (int32_t)used.size(), sels.data(), (int32_t)sels.size(),
            group.data(), (int32_t)group.size(), aggs.data(), (int32_t)aggs.size(), t.blockSize, &h.q));
    }

    std::unique_ptr<Iterator<ColumnVectorBatch>> batches(const std::vector<Leaf> &leaves, const std::vector<int32_t> *prog = nullptr) const {
        QueryHandle h;
        makeQuery(leaves, {}, 0, h, prog);
        imm3Check(imm3_query_run_select(h.q));
        int32_t nb = 0;
        int64_t nwords = 0, nrows = 0;
        imm3Check(imm3_query_layout(h.q, &nb, &nwords, &nrows));
        std::vector<int32_t> size((size_t)nb), oid((size_t)nb);
        std::vector<int64_t> woff((size_t)nb);
        imm3Check(imm3_query_batches(h.q, size.data(), oid.data(), woff.data()));
        std::vector<uint64_t> words((size_t)nwords);
        imm3Check(imm3_query_bitmap(h.q, words.data(), nwords));
        auto it = std::make_unique<VectorIterator<ColumnVectorBatch>>();
        // PFOR_INT / snappy columns: the vectors of the batches are the GPU's decode of the segment (one projection, no predicate)
        std::vector<std::shared_ptr<std::vector<uint8_t>>> decoded(cols_.size());
        for (size_t ci = 0; ci < cols_.size(); ++ci) {
            if ((cols_[ci].codec != CodecType::PFOR_INT && !isSnappy(cols_[ci].codec)) || nrows == 0) continue;
            QueryHandle d;
            const Table &t = table();
            const int32_t used = t.columnIndex(cols_[ci].name), proj = 0;
            imm3Check(imm3_query_create(sm_.ctx(), sm_.deviceSegment(tableName_, segIdx_), &used, 1, nullptr, 0, &proj, 1, 0, t.blockSize, &d.q));
            imm3Check(imm3_query_run(d.q));
            uint64_t n = 0;
            imm3Check(imm3_query_row_count(d.q, &n));
            decoded[ci] = std::make_shared<std::vector<uint8_t>>((size_t)n * (size_t)cols_[ci].width());
            void *outp = decoded[ci]->data();
            imm3Check(imm3_query_fetch_rows(d.q, nullptr, &outp, n));
        }
        int64_t row = 0;
        for (int32_t k = 0; k < nb; ++k) {
            ColumnVectorBatch b;
            b.oid = oid[(size_t)k];
            b.size = size[(size_t)k];
            b.columns = cols_;
            const int64_t nw = (b.size + 63) / 64;
            b.selected.words.assign(words.begin() + woff[(size_t)k], words.begin() + woff[(size_t)k] + nw);
            b.selectedInUse = leaves.empty() ? true : !b.selected.isEmpty(); // Select.scala:44-47
            for (size_t ci = 0; ci < cols_.size(); ++ci) {
                const Column &c = cols_[ci];
                const MappedFile &f = sm_.sm.segments.at(tableName_ + "." + c.name).at((size_t)segIdx_);
                ColumnVector v;
                v.type = c.columnType;
                v.width = c.width();
                v.owner = decoded[ci];
                v.data = (decoded[ci] ? decoded[ci]->data() : f.data) + (size_t)row * (size_t)v.width;
                v.n = b.size;
                b.columnVectors.push_back(v);
            }
            row += b.size;
            it->items.push_back(std::move(b));
        }
        return it;
    }
    std::unique_ptr<Iterator<ColumnVectorBatch>> iterator() override { return batches({}); }
    const std::vector<Column> &cols() const { return cols_; }

  private:
    GpuSegmentManager &sm_;
    int segIdx_;
    std::string tableName_;
    std::vector<Column> cols_;
};

// ---- SelectOp (Select.scala:14) ----
class SelectOp : public ColumnVectorOperator {
  public:
    SelectOp(const std::string &col, SelectCondition cond, std::shared_ptr<ColumnVectorOperator> op) : col_(col), cond_(std::move(cond)), op_(std::move(op)) {}
    static std::function<std::shared_ptr<ColumnVectorOperator>(std::shared_ptr<ColumnVectorOperator>)> mkSelectOp(const std::string &col, const SelectCondition &cond) {
        return [col, cond](std::shared_ptr<ColumnVectorOperator> op) { return std::make_shared<SelectOp>(col, cond, op); };
    }
    // (ScanOp, leaves in application order: innermost SelectOp first)
    std::shared_ptr<ScanOp> chain(std::vector<Leaf> &leaves) const {
        std::shared_ptr<ScanOp> scan;
        if (auto inner = std::dynamic_pointer_cast<SelectOp>(op_)) scan = inner->chain(leaves);
        else if (auto s = std::dynamic_pointer_cast<ScanOp>(op_)) scan = s;
        else throw Exception("SelectOp chain must end in a ScanOp for the fused GPU path");
        leaves.push_back(Leaf{col_, cond_});
        return scan;
    }
    static void checkConditions(const std::vector<Leaf> &leaves) {
        for (const auto &l : leaves)
            if (l.cond.kind == SelectCondition::NotMatch || l.cond.kind == SelectCondition::NoOp)
                throw Exception("Unsupported condition: " + l.cond.toString()); // Select.scala:22
        for (const auto &l : leaves)
            if (l.cond.kind == SelectCondition::IntInQuery) throw Exception("IntInQuery: a sub-query runs through Engine::execute / executeAgg, which resolve it to a set");
    }
    std::unique_ptr<Iterator<ColumnVectorBatch>> iterator() override {
        std::vector<Leaf> leaves;
        auto scan = chain(leaves);
        checkConditions(leaves);
        return scan->batches(leaves);
    }

  private:
    std::string col_;
    SelectCondition cond_;
    std::shared_ptr<ColumnVectorOperator> op_;
};

// ---- SelectTreeOp: a whole SelectADT over a ScanOp with its AND / OR tags HONOURED -- what the reference announces and does not do
// (Engine.scala:236,266: "TODO: use AND/OR operators").  Fuses with ScanOp / ProjectOp / ProjectAggOp like a SelectOp chain does.
// honourNotMatch: a NotMatch(values) leaf -- which the reference's SelectOp throws on (Select.scala:22) -- is emitted as Match(values)
// followed by IMM3_EXPR_NOT, the complement of its Match; off, the leaf stays what checkConditions rejects. ----
class SelectTreeOp : public ColumnVectorOperator {
  public:
    SelectTreeOp(std::shared_ptr<SelectADT> select, std::shared_ptr<ColumnVectorOperator> op, bool honourNotMatch = false)
        : select_(std::move(select)), op_(std::move(op)), honourNotMatch_(honourNotMatch) {}
    // the tree as leaves + postfix program, post-order (a NoSelect side adds nothing: the other side stands alone)
    static void program(const SelectADT &s, std::vector<Leaf> &leaves, std::vector<int32_t> &prog, bool honourNotMatch = false) {
        if (s.kind == SelectADT::And || s.kind == SelectADT::Or) {
            const size_t before = prog.size();
            program(*s.op1, leaves, prog, honourNotMatch);
            const size_t mid = prog.size();
            program(*s.op2, leaves, prog, honourNotMatch);
            if (mid > before && prog.size() > mid) prog.push_back(s.kind == SelectADT::And ? IMM3_EXPR_AND : IMM3_EXPR_OR);
        } else if (s.kind == SelectADT::Select) {
            prog.push_back((int32_t)leaves.size());
            if (honourNotMatch && s.cond.kind == SelectCondition::NotMatch) {
                leaves.push_back(Leaf{s.col, SelectCondition::match(s.cond.values)});
                prog.push_back(IMM3_EXPR_NOT);
            } else leaves.push_back(Leaf{s.col, s.cond});
        }
    }
    static bool hasOr(const SelectADT &s) {
        return s.kind == SelectADT::Or || (s.kind == SelectADT::And && (hasOr(*s.op1) || hasOr(*s.op2)));
    }
    static bool hasNotMatch(const SelectADT &s) {
        if (s.kind == SelectADT::And || s.kind == SelectADT::Or) return hasNotMatch(*s.op1) || hasNotMatch(*s.op2);
        return s.kind == SelectADT::Select && s.cond.kind == SelectCondition::NotMatch;
    }
    std::shared_ptr<ScanOp> chain(std::vector<Leaf> &leaves, std::vector<int32_t> &prog) const {
        auto scan = std::dynamic_pointer_cast<ScanOp>(op_);
        if (!scan) throw Exception("SelectTreeOp must sit on a ScanOp for the fused GPU path");
        program(*select_, leaves, prog, honourNotMatch_);
        return scan;
    }
    std::unique_ptr<Iterator<ColumnVectorBatch>> iterator() override {
        std::vector<Leaf> leaves;
        std::vector<int32_t> prog;
        auto scan = chain(leaves, prog);
        SelectOp::checkConditions(leaves);
        return scan->batches(leaves, &prog);
    }

  private:
    std::shared_ptr<SelectADT> select_;
    std::shared_ptr<ColumnVectorOperator> op_;
    bool honourNotMatch_ = false;
};

// ---- ProjectOp (Project.scala:17) ----
class ProjectOp : public ProjectionOperator {
  public:
    // orderBy: (column of `cols`, descending), most significant first -- the rows come back in that order, `limit` applied behind it
    // (imm3_query_set_order: sorted on the device); empty: the reference's ProjectOp
    ProjectOp(std::vector<std::string> cols, std::shared_ptr<ColumnVectorOperator> op, int limit = 0, std::vector<std::pair<std::string, bool>> orderBy = {})
        : cols_(std::move(cols)), op_(std::move(op)), limit_(limit), orderKeys_(orderKeys(cols_, orderBy)) {}
    static std::function<std::shared_ptr<ProjectOp>(std::shared_ptr<ColumnVectorOperator>)> mkProjectOp(const std::vector<std::string> &cols, int limit = 0,
                                                                                                          const std::vector<std::pair<std::string, bool>> &orderBy = {}) {
        return [cols, limit, orderBy](std::shared_ptr<ColumnVectorOperator> op) { return std::make_shared<ProjectOp>(cols, op, limit, orderBy); };
    }
    // the one call an ordered query adds between its creation and its first run
    static void setOrder(imm3_query *q, const std::vector<std::pair<int, bool>> &keys, int limit) {
        std::vector<imm3_order_key> ks;
        for (const auto &k : keys) ks.push_back(imm3_order_key{(int32_t)k.first, k.second ? 1 : 0});
        imm3Check(imm3_query_set_order(q, ks.data(), (int32_t)ks.size(), limit));
    }
    std::unique_ptr<Iterator<Row>> iterator() override {
        std::vector<Leaf> leaves;
        std::vector<int32_t> prog;
        const std::vector<int32_t> *progp = nullptr;
        std::shared_ptr<ScanOp> scan;
        if (auto sel = std::dynamic_pointer_cast<SelectOp>(op_)) scan = sel->chain(leaves);
        else if (auto tree = std::dynamic_pointer_cast<SelectTreeOp>(op_)) { scan = tree->chain(leaves, prog); progp = &prog; }
        else scan = std::dynamic_pointer_cast<ScanOp>(op_);
        if (!scan) return hostIterator();
        SelectOp::checkConditions(leaves);
        QueryHandle h;
        scan->makeQuery(leaves, cols_, orderKeys_.empty() ? limit_ : 0, h, progp); // (an order's limit is applied behind the order: no creation-time limit)
        if (!orderKeys_.empty()) setOrder(h.q, orderKeys_, limit_);
        imm3Check(imm3_query_run(h.q));
        uint64_t n = 0;
        imm3Check(imm3_query_row_count(h.q, &n));
        std::vector<Column> pcols;
        for (const auto &name : cols_)
            for (const auto &c : scan->cols())
                if (c.name == name) { pcols.push_back(c); break; }
        std::vector<std::vector<uint8_t>> bufs(pcols.size());
        std::vector<void *> ptrs(pcols.size());
        for (size_t j = 0; j < pcols.size(); ++j) {
            bufs[j].resize((size_t)std::max<uint64_t>(n, 1) * (size_t)pcols[j].width());
            ptrs[j] = bufs[j].data();
        }
        imm3Check(imm3_query_fetch_rows(h.q, nullptr, ptrs.data(), n));
        auto it = std::make_unique<VectorIterator<Row>>();
        it->items.reserve((size_t)n);
        for (uint64_t i = 0; i < n; ++i) {
            std::vector<Value> xs;
            for (size_t j = 0; j < pcols.size(); ++j) {
                ColumnVector v;
                v.type = pcols[j].columnType;
                v.width = pcols[j].width();
                v.data = bufs[j].data();
                xs.push_back(v.value((int)i));
            }
            it->items.push_back(Row::fromSeq(std::move(xs)));
        }
        return it;
    }

  private:
    // ProjectIterator over batches from a non-fusable upstream (Project.scala:37-80); empty batches are skipped
    // (the reference faults on them).
    std::unique_ptr<Iterator<Row>> hostIterator() {
        auto it = std::make_unique<VectorIterator<Row>>();
        auto in = op_->iterator();
        int total = 0;
        const int limit = orderKeys_.empty() ? limit_ : 0; // (ordered: every row, sorted below)
        while (in->hasNext() && !(limit > 0 && total >= limit)) {
            ColumnVectorBatch vec = in->next();
            std::vector<int> vecCols;
            for (const auto &name : cols_) {
                int idx = -1;
                for (size_t i = 0; i < vec.columns.size(); ++i)
                    if (vec.columns[i].name == name) { idx = (int)i; break; }
                if (idx < 0) throw Exception("NoSuchElementException: key not found: " + name);
                vecCols.push_back(idx);
            }
            for (int pos : vec.selected.toList()) {
                if (limit > 0 && total >= limit) break;
                std::vector<Value> xs;
                for (int ci : vecCols) xs.push_back(vec.columnVectors[(size_t)ci].value(pos));
                it->items.push_back(Row::fromSeq(std::move(xs)));
                ++total;
            }
        }
        if (!orderKeys_.empty()) {
            std::stable_sort(it->items.begin(), it->items.end(), [this](const Row &a, const Row &b) { return rowBefore(a, b, orderKeys_); });
            if (limit_ > 0 && it->items.size() > (size_t)limit_) it->items.resize((size_t)limit_);
        }
        return it;
    }
    std::vector<std::string> cols_;
    std::shared_ptr<ColumnVectorOperator> op_;
    int limit_;
    std::vector<std::pair<int, bool>> orderKeys_;
};


// ---- aggregation (engine/.../operator/ProjectAggregate.scala:11-227, ProjectAggregateQueue.scala:9-55) ----
inline std::string javaDoubleToString(double v) { // Double.toString for the integral values the aggregators hold
    const long long iv = (long long)v;
    if (iv > -10000000LL && iv < 10000000LL) return std::to_string(iv) + ".0";
    std::string digits = std::to_string(iv < 0 ? -iv : iv);
    std::string frac = digits.substr(1);
    while (!frac.empty() && frac.back() == '0') frac.pop_back();
    if (frac.empty()) frac = "0";
    return std::string(iv < 0 ? "-" : "") + digits[0] + "." + frac + "E" + std::to_string(digits.size() - 1);
}

// CountDistinctAggr (not in the reference): count(distinct col), the number of distinct values per group (IMM3_AGG_COUNT_DISTINCT); its
// figure is `counter`.  The figure is exact because ONE query counts it over a set on the device; two figures do not add, so combine()
// throws -- OUT OF SCOPE: a getter for the sets themselves, and with it the engines' per-segment fallback.
constexpr const char *kCountDistinctOneQuery = "count(distinct) runs as one table query only";
struct Aggregator { // CountAggr / MaxDoubleAggr / MinDoubleAggr / MaxStringAggr / CountDistinctAggr, folded into one tagged value
    enum Kind { CountAggr, MaxDoubleAggr, MinDoubleAggr, MaxStringAggr, CountDistinctAggr } kind = CountAggr;
    std::string col, alias;
    long long counter = 0;
    double dvalue = 0;
    std::string svalue;
    static Aggregator make(Kind k, const std::string &col, const std::string &alias) {
        Aggregator a;
        a.kind = k;
        a.col = col;
        a.alias = alias;
        a.dvalue = k == MaxDoubleAggr ? -1.7976931348623157e308 : 1.7976931348623157e308; // Double.MinValue / MaxValue
        return a;
    }
    int abiKind() const { return kind == CountAggr ? IMM3_AGG_COUNT : (kind == CountDistinctAggr ? IMM3_AGG_COUNT_DISTINCT : (kind == MinDoubleAggr ? IMM3_AGG_MIN : IMM3_AGG_MAX)); }
    bool isCounter() const { return kind == CountAggr || kind == CountDistinctAggr; } // an exact integer in `counter`
    void combine(const Aggregator &o) { // ProjectAggregateQueue.scala:27-34
        switch (kind) {
        case CountAggr: counter += o.counter; break;
        case MaxDoubleAggr: if (o.dvalue > dvalue) dvalue = o.dvalue; break;
        case MinDoubleAggr: if (o.dvalue < dvalue) dvalue = o.dvalue; break;
        case MaxStringAggr: if (svalue.empty() || o.svalue > svalue) svalue = o.svalue; break;
        case CountDistinctAggr: throw Exception(std::string(kCountDistinctOneQuery) + ": `" + alias + "' of two queries cannot be combined (counts of distinct values do not add)");
        }
    }
    std::string repr() const {
        switch (kind) {
        case CountAggr: case CountDistinctAggr: return std::to_string(counter);
        case MaxStringAggr: return svalue;
        default: return javaDoubleToString(dvalue);
        }
    }
};

using AggMap = std::vector<Aggregator>;                       // alias order = SELECT-list order (see Engine::executeAgg)
using AggMapTuple = std::pair<std::string, AggMap>;           // (groupKey, aggregators)
using RawKey = std::vector<std::string>;                      // the raw bytes of a group key's parts, in batch-column order

// ORDER BY over groups: entries (name, descending) over an aggregation's group-by columns and aliases, resolved.  A name that is
// neither is refused; so is anything but the four aggregators above (ordering by an average is out of scope).
struct GroupOrderEntry {
    bool isAgg;
    std::string name;
    bool desc;
};
inline std::vector<GroupOrderEntry> groupOrderSpec(const std::vector<Aggregator> &aggs, const std::vector<std::string> &groupBy,
                                                   const std::vector<std::pair<std::string, bool>> &orderBy) {
    std::vector<GroupOrderEntry> out;
    for (const auto &k : orderBy) {
        bool isGroup = false, isAlias = false;
        for (const auto &g : groupBy) isGroup = isGroup || g == k.first;
        for (const auto &a : aggs) isAlias = isAlias || a.alias == k.first;
        if (!isGroup && !isAlias) throw Exception("order by `" + k.first + "' is neither a group-by column nor an aggregate's alias");
        out.push_back(GroupOrderEntry{!isGroup, k.first, k.second});
    }
    return out;
}

// The host's ORDER BY over MERGED groups (the per-segment fallback; the Python mirror: operators.order_groups): `groups` in merged
// first-arrival order, raw[i] the raw key parts of groups[i] in the order of groupCols.  The normal form is the device's
// (include/imm3.h): signed integers biased to unsigned, big-endian; counts as integers; strings byte-wise; a descending key
// complemented; ties -- all keys equal -- in arrival order.  Cut to `limit` > 0.
inline void orderGroups(std::vector<AggMapTuple> &groups, const std::vector<RawKey> &raw, const std::vector<Column> &groupCols,
                        const std::vector<GroupOrderEntry> &spec, int limit) {
    auto be64 = [](unsigned long long v) { std::string b(8, '\0'); for (int x = 0; x < 8; ++x) b[(size_t)x] = (char)(v >> (8 * (7 - x))); return b; };
    if (!spec.empty()) {
        std::vector<std::string> normal(groups.size());
        for (size_t i = 0; i < groups.size(); ++i) {
            for (const auto &e : spec) {
                std::string b;
                if (!e.isAgg) {
                    size_t k = 0;
                    while (k < groupCols.size() && groupCols[k].name != e.name) ++k;
                    const std::string &r = raw.at(i).at(k);
                    if (groupCols[k].columnType == ColumnType::STRING) b = r;
                    else { // int32 / int8, little-endian: sign-extend, then bias
                        long long v = 0;
                        for (size_t x = 0; x < r.size(); ++x) v |= (long long)(unsigned char)r[x] << (8 * x);
                        const int bits = 8 * (int)r.size();
                        if (bits < 64 && (v >> (bits - 1)) & 1) v -= 1LL << bits;
                        b = be64((unsigned long long)v ^ (1ULL << 63));
                    }
                } else {
                    const Aggregator *a = nullptr;
                    for (const auto &x : groups[i].second) if (x.alias == e.name) a = &x;
                    if (!a) throw Exception("NoSuchElementException: key not found: " + e.name);
                    if (a->isCounter()) b = be64((unsigned long long)a->counter);
                    else if (a->kind == Aggregator::MaxStringAggr) b = a->svalue;
                    else b = be64((unsigned long long)(long long)a->dvalue ^ (1ULL << 63));
                }
                if (e.desc) for (auto &ch : b) ch = (char)~(unsigned char)ch;
                normal[i] += b;
            }
        }
        std::vector<size_t> idx(groups.size());
        for (size_t i = 0; i < idx.size(); ++i) idx[i] = i;
        std::stable_sort(idx.begin(), idx.end(), [&normal](size_t x, size_t y) { return normal[x] < normal[y]; });
        std::vector<AggMapTuple> sorted;
        sorted.reserve(groups.size());
        for (size_t i : idx) sorted.push_back(std::move(groups[i]));
        groups.swap(sorted);
    }
    if (limit > 0 && groups.size() > (size_t)limit) groups.resize((size_t)limit);
}

// HAVING over an aggregation's aggregators: groupFilterLeaves' checks, and a MaxStringAggr's alias is refused (string maxima are not
// compared).
inline void groupFilterSpec(const std::vector<Aggregator> &aggs, const std::vector<std::string> &groupBy, const SelectADT *having,
                            std::vector<GroupFilterLeaf> &leaves, std::vector<int32_t> &prog) {
    std::vector<std::string> aliases;
    for (const auto &a : aggs) aliases.push_back(a.alias);
    groupFilterLeaves(aliases, groupBy, having, leaves, prog);
    for (const auto &l : leaves)
        for (const auto &a : aggs)
            if (a.alias == l.alias && a.kind == Aggregator::MaxStringAggr) throw Exception("having `" + l.alias + "': a string MAX is not compared by having");
}
// one leaf on exact integers: lhs <cond> value, or -- an average -- sum <cond> value * count (the device's rule: include/imm3.h,
// imm3_query_set_group_filter; |value| <= 2^31 and count < 2^32 keep the product inside int64)
inline bool groupFilterCompare(long long lhs, long long count, const GroupFilterLeaf &l) {
    const long long rhs = l.average ? l.value * count : l.value;
    return l.cond == IMM3_GT ? lhs > rhs : (l.cond == IMM3_LT ? lhs < rhs : lhs == rhs);
}
// a postfix program over leaf answers (leaf index, IMM3_EXPR_AND / _OR / _NOT)
template <class LeafFn>
inline bool groupFilterEval(const std::vector<int32_t> &prog, LeafFn leaf) {
    std::vector<char> st;
    for (int32_t op : prog) {
        if (op >= 0) st.push_back(leaf(op) ? 1 : 0);
        else if (op == IMM3_EXPR_NOT) st.back() = !st.back();
        else {
            const char y = st.back();
            st.pop_back();
            st.back() = op == IMM3_EXPR_AND ? (st.back() && y) : (st.back() || y);
        }
    }
    return st.empty() || st.back();
}
// The host's HAVING over MERGED groups (the per-segment fallback; the Python mirror: operators.filter_groups): the groups the program
// keeps, in their order; `raw` (parallel to `groups`) is cut with them.
inline void filterGroups(std::vector<AggMapTuple> &groups, std::vector<RawKey> &raw, const std::vector<GroupFilterLeaf> &leaves, const std::vector<int32_t> &prog) {
    if (prog.empty()) return;
    size_t w = 0;
    for (size_t i = 0; i < groups.size(); ++i) {
        const AggMap &m = groups[i].second;
        const bool keep = groupFilterEval(prog, [&](int32_t at) {
            const GroupFilterLeaf &l = leaves.at((size_t)at);
            for (const auto &a : m)
                if (a.alias == l.alias) return groupFilterCompare(a.isCounter() ? a.counter : (long long)a.dvalue, 1, l);
            throw Exception("NoSuchElementException: key not found: " + l.alias);
        });
        if (!keep) continue;
        if (w != i) {
            groups[w] = std::move(groups[i]);
            if (i < raw.size()) raw[w] = std::move(raw[i]);
        }
        ++w;
    }
    groups.resize(w);
    if (raw.size() > w) raw.resize(w);
}

// ProjectAggOp(aggs, op, groupBy): one segment, fused on the GPU (scan+select kernel, LDS hash aggregation kernel)
class ProjectAggOp : public Operator<AggMapTuple> {
  public:
    // orderBy -- (name, descending) over the group-by columns and the aliases -- and limit are applied by the device when ONE query
    // answers (runOn: a table query); per-segment results are ordered after their merge (orderGroups)
    ProjectAggOp(std::vector<Aggregator> aggs, std::shared_ptr<ColumnVectorOperator> op, std::vector<std::string> groupBy,
                 std::vector<std::pair<std::string, bool>> orderBy = {}, int limit = 0, std::shared_ptr<SelectADT> having = nullptr)
        : aggs_(std::move(aggs)), op_(std::move(op)), groupBy_(std::move(groupBy)), limit_(limit) {
        spec_ = groupOrderSpec(aggs_, groupBy_, orderBy);
        groupFilterSpec(aggs_, groupBy_, having.get(), filterLeaves_, filterProg_); // having: applied by the device when ONE query answers (runOn), else filterGroups
    }
    const std::vector<GroupOrderEntry> &orderSpec() const { return spec_; }
    const std::vector<RawKey> &rawKeys() const { return rawKeys_; } // of the groups the last iterator() / runOn produced, in their order
    std::unique_ptr<Iterator<AggMapTuple>> iterator() override {
        std::vector<Leaf> leaves;
        std::vector<int32_t> prog;
        const std::vector<int32_t> *progp = nullptr;
        std::shared_ptr<ScanOp> scan;
        if (auto sel = std::dynamic_pointer_cast<SelectOp>(op_)) scan = sel->chain(leaves);
        else if (auto tree = std::dynamic_pointer_cast<SelectTreeOp>(op_)) { scan = tree->chain(leaves, prog); progp = &prog; }
        else scan = std::dynamic_pointer_cast<ScanOp>(op_);
        if (!scan) throw Exception("ProjectAggOp must sit on a ScanOp / SelectOp chain for the fused GPU path");
        SelectOp::checkConditions(leaves);
        const std::vector<Column> &cols = scan->cols();
        auto usedIndex = [&](const std::string &n) -> int32_t {
            for (size_t i = 0; i < cols.size(); ++i) if (cols[i].name == n) return (int32_t)i;
            throw Exception("NoSuchElementException: key not found: " + n);
        };
        // groupCols filters the BATCH columns by membership in groupBy (ProjectAggregate.scala:135-140)
        std::vector<int32_t> group;
        for (size_t i = 0; i < cols.size(); ++i)
            for (const auto &g : groupBy_) if (cols[i].name == g) { group.push_back((int32_t)i); break; }
        // aggsMap is keyed by alias: a later duplicate replaces an earlier one
        std::vector<Aggregator> aggs;
        for (const auto &a : aggs_) {
            bool replaced = false;
            for (auto &b : aggs) if (b.alias == a.alias) { b = a; replaced = true; }
            if (!replaced) aggs.push_back(a);
        }
        std::vector<imm3_aggregate> abi(aggs.size());
        for (size_t j = 0; j < aggs.size(); ++j) { abi[j].kind = aggs[j].abiKind(); abi[j].column = usedIndex(aggs[j].col); }
        QueryHandle h;
        scan->makeAggQuery(leaves, group, abi, h, progp);
        auto it = std::make_unique<VectorIterator<AggMapTuple>>();
        it->items = decode(h, cols, group, aggs, abi, rawKeys_);
        return it;
    }

    // the same aggregation as ONE table-level query (imm3_table): groups merged across segments on the GPU.  `prog`: `sels` are the
    // leaves of a select TREE and this is its postfix program (imm3_query_create_table_agg_expr); false: the table refused the tree
    // (IMM3_ERR_ARG: it does not fit the one launch) and the caller runs per-segment queries.
    bool runOn(imm3_table *table, const std::vector<Column> &cols, const std::vector<int32_t> &usedIdx, const std::vector<imm3_select> &sels,
               const std::vector<int32_t> *prog, std::vector<AggMapTuple> &out) {
        std::vector<int32_t> group;
        for (size_t i = 0; i < cols.size(); ++i)
            for (const auto &g : groupBy_) if (cols[i].name == g) { group.push_back((int32_t)i); break; }
        std::vector<Aggregator> aggs;
        for (const auto &a : aggs_) {
            bool replaced = false;
            for (auto &b : aggs) if (b.alias == a.alias) { b = a; replaced = true; }
            if (!replaced) aggs.push_back(a);
        }
        std::vector<imm3_aggregate> abi(aggs.size());
        for (size_t j = 0; j < aggs.size(); ++j) {
            abi[j].kind = aggs[j].abiKind();
            abi[j].column = -1;
            for (size_t i = 0; i < cols.size(); ++i) if (cols[i].name == aggs[j].col) abi[j].column = (int32_t)i;
            if (abi[j].column < 0) throw Exception("NoSuchElementException: key not found: " + aggs[j].col);
        }
        auto scanOp = std::dynamic_pointer_cast<ScanOp>(op_);
        QueryHandle h;
        int keyBytes = 0; // a group key wider than 8 bytes: the _wide entry point
        for (int32_t g : group) keyBytes += cols[(size_t)g].width();
        if (prog) { // (one entry point for narrow and wide keys)
            const int rc = imm3_query_create_table_agg_expr(scanOp->manager().ctx(), table, usedIdx.data(), (int32_t)usedIdx.size(), sels.data(), (int32_t)sels.size(),
                                                            prog->data(), (int32_t)prog->size(), group.data(), (int32_t)group.size(), abi.data(), (int32_t)abi.size(),
                                                            scanOp->table().blockSize, &h.q);
            if (tableTreeRefused(rc)) return false;
            imm3Check(rc);
        } else
        imm3Check((keyBytes > 8 ? imm3_query_create_table_agg_wide : imm3_query_create_table_agg)(
            scanOp->manager().ctx(), table, usedIdx.data(), (int32_t)usedIdx.size(), sels.data(), (int32_t)sels.size(),
            group.data(), (int32_t)group.size(), abi.data(), (int32_t)abi.size(), scanOp->table().blockSize, &h.q));
        if (!filterProg_.empty()) { // filter, then order, then limit: all on the device
            std::vector<imm3_group_filter_leaf> fl;
            for (const auto &l : filterLeaves_) {
                imm3_group_filter_leaf x{-2, l.average ? 1 : 0, l.cond, l.value};
                for (size_t j = 0; j < aggs.size(); ++j) if (aggs[j].alias == l.alias) x.agg = (int32_t)j;
                fl.push_back(x);
            }
            imm3Check(imm3_query_set_group_filter(h.q, fl.data(), (int32_t)fl.size(), filterProg_.data(), (int32_t)filterProg_.size()));
        }
        if (!spec_.empty()) { // this query's groups are the whole answer: the device orders them and cuts them to the limit
            std::vector<imm3_group_order_key> keys;
            for (const auto &e : spec_) {
                imm3_group_order_key k{e.isAgg ? IMM3_GROUP_ORDER_AGG : IMM3_GROUP_ORDER_GROUP_COL, -1, e.desc ? 1 : 0};
                if (e.isAgg) { for (size_t j = 0; j < aggs.size(); ++j) if (aggs[j].alias == e.name) k.index = (int32_t)j; }
                else for (size_t g = 0; g < group.size(); ++g) if (cols[(size_t)group[g]].name == e.name) k.index = (int32_t)g;
                keys.push_back(k);
            }
            imm3Check(imm3_query_set_group_order(h.q, keys.data(), (int32_t)keys.size(), limit_));
        }
        out = decode(h, cols, group, aggs, abi, rawKeys_);
        if (spec_.empty() && limit_ > 0 && out.size() > (size_t)limit_) out.resize((size_t)limit_);
        return true;
    }

  private:
    static std::vector<AggMapTuple> decode(QueryHandle &h, const std::vector<Column> &cols, const std::vector<int32_t> &group,
                                           const std::vector<Aggregator> &aggs, const std::vector<imm3_aggregate> &abi, std::vector<RawKey> &rawKeys) {
        rawKeys.clear();
        imm3Check(imm3_query_run(h.q));
        uint32_t n = 0;
        imm3Check(imm3_query_group_count(h.q, &n));
        std::vector<uint64_t> keys(n), counts(n);
        std::vector<uint32_t> first(n);
        std::vector<int64_t> vals((size_t)n * aggs.size());
        imm3Check(imm3_query_fetch_groups(h.q, keys.data(), first.data(), counts.data(), vals.data(), n));
        // a MaxStringAggr over a column wider than 8 bytes: vals hold its first 8 bytes, the exact values come per aggregate
        std::vector<std::vector<uint8_t>> wide(aggs.size());
        for (size_t j = 0; j < aggs.size(); ++j) {
            const int w = cols[(size_t)abi[j].column].width();
            if (aggs[j].kind != Aggregator::MaxStringAggr || w <= 8) continue;
            wide[j].resize((size_t)n * (size_t)w);
            imm3Check(imm3_query_fetch_group_strings(h.q, (int32_t)j, wide[j].data(), n));
        }
        // the packed group keys: from the u64 keys, or (a key wider than 8 bytes) from the device
        size_t keyBytes = 0;
        for (int32_t gc : group) keyBytes += (size_t)cols[(size_t)gc].width();
        std::vector<uint8_t> packed((size_t)n * keyBytes);
        if (keyBytes > 8) imm3Check(imm3_query_fetch_group_keys(h.q, packed.data(), n));
        else
            for (uint32_t g = 0; g < n; ++g)
                for (size_t b = 0; b < keyBytes; ++b) packed[(size_t)g * keyBytes + b] = (uint8_t)(keys[g] >> (8 * b));
        std::vector<AggMapTuple> items;
        for (uint32_t g = 0; g < n; ++g) {
            std::string key;
            int off = 0;
            rawKeys.emplace_back();
            for (size_t k = 0; k < group.size(); ++k) {
                const Column &c = cols[(size_t)group[k]];
                const int w = c.width();
                ColumnVector v;
                v.type = c.columnType;
                v.width = w;
                v.data = packed.data() + (size_t)g * keyBytes + (size_t)off;
                if (k) key += "_";
                key += v.value(0).toString(); // mkString("_"), ProjectAggregate.scala:144
                rawKeys.back().emplace_back((const char *)v.data, (size_t)w);
                off += w;
            }
            AggMap m = aggs;
            for (size_t j = 0; j < aggs.size(); ++j) {
                const int64_t x = vals[(size_t)g * aggs.size() + j];
                switch (m[j].kind) {
                case Aggregator::CountAggr: m[j].counter = (long long)counts[g]; break;
                case Aggregator::CountDistinctAggr: m[j].counter = (long long)x; break; // the pair set's figure, an int64 in the value column
                case Aggregator::MaxStringAggr: {
                    const int w = cols[(size_t)abi[j].column].width();
                    std::string sv((size_t)w, '\0');
                    if (!wide[j].empty()) sv.assign((const char *)wide[j].data() + (size_t)g * (size_t)w, (size_t)w);
                    else
                        for (int b = 0; b < w; ++b) sv[(size_t)b] = (char)((uint64_t)x >> (8 * (w - 1 - b)));
                    m[j].svalue = sv;
                    break;
                }
                default: m[j].dvalue = (double)x;
                }
            }
            items.emplace_back(key, std::move(m));
        }
        return items;
    }

    std::vector<Aggregator> aggs_;
    std::shared_ptr<ColumnVectorOperator> op_;
    std::vector<std::string> groupBy_;
    std::vector<GroupOrderEntry> spec_;
    std::vector<GroupFilterLeaf> filterLeaves_;
    std::vector<int32_t> filterProg_;
    int limit_ = 0;
    std::vector<RawKey> rawKeys_;
};

// ---- Engine (Engine.scala:81-197) ----
class Engine {
  public:
    // honourAndOr: a query whose select tree holds an Or runs it as a disjunction (one table launch when the table takes the tree, else
    // one SelectTreeOp per segment) instead of the reference's conjunction.  Off (the default) nothing changes; a tree without Or is the same either way.
    // honourNotMatch: a query whose select tree holds a NotMatch leaf runs as a tree, whether or not it has an Or: the leaf is the
    // complement of its Match (IMM3_EXPR_NOT), and the And / Or tags of THAT query are then honoured too.  Off (the default) nothing
    // changes: the leaf throws "Unsupported condition", as in the reference.
    explicit Engine(GpuSegmentManager &sm, bool honourAndOr = false, bool honourNotMatch = false) : sm_(sm), honourAndOr_(honourAndOr), honourNotMatch_(honourNotMatch) {}
    bool notTree(const Query &q) const { return honourNotMatch_ && SelectTreeOp::hasNotMatch(*q.select); }
    bool asTree(const Query &q) const { return (honourAndOr_ && SelectTreeOp::hasOr(*q.select)) || notTree(q); }
    // the operators between ScanOp and the projection: the reference's SelectOp chain, or one SelectTreeOp
    std::shared_ptr<ColumnVectorOperator> selectOps(const Query &q, const std::vector<Leaf> &leaves, std::shared_ptr<ColumnVectorOperator> op) const {
        if (asTree(q)) return std::make_shared<SelectTreeOp>(q.select, op, notTree(q));
        for (const auto &l : leaves) op = SelectOp::mkSelectOp(l.col, l.cond)(op);
        return op;
    }

    // Engine.getColumns (:85-106): (rec(query.select).toList ++ projectColumns).toSet.toList.  Scala's Set1..Set4 keep
    // insertion order, so for <= 4 distinct columns this is first-seen order (SURVEY A.1 rule 3); from the fifth distinct
    // column on, the set is an immutable.HashSet and the order is its hash trie's (scala_sets.hpp).
    static std::vector<Column> getColumns(const Query &q, const Table &table) {
        std::function<scalasets::ColumnSet(const SelectADT &)> rec = [&](const SelectADT &s) {
            scalasets::ColumnSet out;
            if (s.kind == SelectADT::And || s.kind == SelectADT::Or) { // rec(a) ++ rec(b): b's elements, in b's order, added to a
                out = rec(*s.op1);
                for (const auto &c : rec(*s.op2).toList()) out.add(c);
            } else if (s.kind == SelectADT::Select) out.add(table.getColumn(s.col));
            return out;
        };
        scalasets::ColumnSet all;
        for (const auto &c : rec(*q.select).toList()) all.add(c);
        if (q.project.kind == ProjectADT::Project) for (const auto &c : q.project.cols) all.add(table.getColumn(c));
        else if (q.project.kind == ProjectADT::ProjectAgg) {
            for (const auto &a : q.project.aggs) all.add(table.getColumn(a.col));
            for (const auto &g : q.project.groupBy) all.add(table.getColumn(g));
        }
        return all.toList();
    }
    // resolveSelectOps + runOps (:108-128, :237-245): left-to-right fold, AND/OR tag ignored
    static std::vector<Leaf> resolveSelectOps(const Query &q) {
        std::vector<Leaf> out;
        std::function<void(const SelectADT &)> rec = [&](const SelectADT &s) {
            if (s.kind == SelectADT::And || s.kind == SelectADT::Or) { rec(*s.op1); rec(*s.op2); }
            else if (s.kind == SelectADT::Select) out.push_back(Leaf{s.col, s.cond});
        };
        rec(*q.select);
        return out;
    }
    // ---- single-launch table path (imm3_table) ----
    struct TablePlan {
        imm3_table *table = nullptr;
        std::vector<Column> used;
        std::vector<int32_t> usedIdx;
        std::vector<imm3_select> sels;
        std::vector<std::string> blobs;
        std::vector<std::vector<int32_t>> lens;
        bool tree = false;         // `sels` are the leaves of a select tree with an Or (honourAndOr) or a NotMatch (honourNotMatch) and `prog` its postfix program:
        std::vector<int32_t> prog; // the _table_expr entry points, which may still refuse it (IMM3_ERR_ARG: per-segment queries)
    };
    // fills `p` and returns true when the whole table can run as one fused launch
    bool tablePlan(const Query &q, TablePlan &p) {
        const Table &table = sm_.sm.getTable(q.table);
        p.table = sm_.deviceTable(q.table);
        if (!p.table) return false;
        p.used = getColumns(q, table);
        for (const auto &c : p.used) p.usedIdx.push_back(table.columnIndex(c.name));
        p.tree = asTree(q);
        std::vector<Leaf> leaves;
        if (p.tree) SelectTreeOp::program(*q.select, leaves, p.prog, notTree(q));
        else leaves = resolveSelectOps(q);
        SelectOp::checkConditions(leaves);
        p.sels.resize(leaves.size());
        p.blobs.resize(leaves.size());
        p.lens.resize(leaves.size());
        for (size_t i = 0; i < leaves.size(); ++i) {
            int32_t ci = -1;
            for (size_t k = 0; k < p.used.size(); ++k) if (p.used[k].name == leaves[i].col) { ci = (int32_t)k; break; }
            if (ci < 0) throw Exception("NoSuchElementException: next on empty iterator");
            const Column &c = p.used[(size_t)ci];
            if (leaves[i].cond.kind == SelectCondition::Match) {
                // the tile kernels take 2-byte strings with <= 8 IN-list values; a flat select list also takes any non-empty IN-list
                // on a string column whose width is a multiple of 4 (k_filter_str_rows); a tree keeps the tile kinds
                const bool isStr = c.columnType == ColumnType::STRING;
                const size_t nv = leaves[i].cond.values.size();
                const bool tile = isStr && c.width() == 2 && nv > 0 && nv <= 8;
                const bool rows = isStr && !p.tree && c.width() % 4 == 0 && c.width() >= 4 && c.width() <= 256 && nv > 0;
                if (!tile && !rows) return false;
            }
            // a table takes a range on a string column whose width is a multiple of 4, in a flat select list only
            if (leaves[i].cond.isStrRange() && !(c.columnType == ColumnType::STRING && !p.tree && c.width() % 4 == 0 && c.width() >= 4 && c.width() <= 256)) return false;
            p.sels[i] = imm3_select{};
            p.sels[i].column = ci;
            p.sels[i].cond = leaves[i].cond.abiCond();
            p.sels[i].value = leaves[i].cond.value;
            for (const auto &v : leaves[i].cond.abiValues(c.width())) { p.blobs[i] += v; p.lens[i].push_back((int32_t)v.size()); }
            p.sels[i].match_bytes = (const uint8_t *)p.blobs[i].data();
            p.sels[i].match_lens = p.lens[i].data();
            p.sels[i].n_match = (int32_t)p.lens[i].size();
            setLeaf(p.sels[i], leaves[i].cond);
        }
        return true;
    }

    // one fused pipeline per segment; rows in ascending segment order (the reference's order across segments is
    // unspecified: queue interleaving, Engine.scala:255); `limit` is global, as the consumer-side ProjectOp's is.
    // Engine.resolveProjectOp (:130-156): default aliases col_max / col_min / col_count; Min over a STRING column
    // becomes MaxStringAggr (the reference's own mapping, :145); Sum / Avg parse but are rejected (:152).
    static std::vector<Aggregator> resolveProjectOp(const ProjectADT &p, const Table &table) {
        std::vector<Aggregator> out;
        for (const auto &a : p.aggs) {
            const bool isStr = table.getColumn(a.col).columnType == ColumnType::STRING;
            switch (a.kind) {
            case Aggregate::Max: out.push_back(Aggregator::make(isStr ? Aggregator::MaxStringAggr : Aggregator::MaxDoubleAggr, a.col, a.alias.empty() ? a.col + "_max" : a.alias)); break;
            case Aggregate::Min: out.push_back(Aggregator::make(isStr ? Aggregator::MaxStringAggr : Aggregator::MinDoubleAggr, a.col, a.alias.empty() ? a.col + "_min" : a.alias)); break;
            case Aggregate::Count: out.push_back(Aggregator::make(Aggregator::CountAggr, a.col, a.alias.empty() ? a.col + "_count" : a.alias)); break;
            case Aggregate::CountDistinct: out.push_back(Aggregator::make(Aggregator::CountDistinctAggr, a.col, a.alias.empty() ? a.col + "_distinct" : a.alias)); break;
            default: throw Exception("Unknown Aggregate type");
            }
        }
        return out;
    }
    // ProjectAgg: per-segment ProjectAggOp + ProjectAggregateQueueOp's combine by key (first arrival first; segments
    // ascending).  Rows list the aggregators' repr in SELECT-list order (the reference iterates a mutable.HashMap
    // keyed by alias, whose order is not reproduced).
    // ---- IN (sub-query): every IntInQuery leaf becomes IntInSet(the device-resident set of its inner selection) ----
    static bool hasSubquery(const SelectADT &s) {
        if (s.kind == SelectADT::And || s.kind == SelectADT::Or) return hasSubquery(*s.op1) || hasSubquery(*s.op2);
        return s.kind == SelectADT::Select && s.cond.kind == SelectCondition::IntInQuery;
    }
    static bool hasResolvedSet(const SelectADT &s) {
        if (s.kind == SelectADT::And || s.kind == SelectADT::Or) return hasResolvedSet(*s.op1) || hasResolvedSet(*s.op2);
        return s.kind == SelectADT::Select && s.cond.kind == SelectCondition::IntInSet;
    }
    // The statement with its sub-queries resolved: the inner query's selects run as one table query where tablePlan takes them, else as
    // per-segment queries; either way all of them are the sources of one imm3_int_set, and the outer statement then takes whichever
    // plan it would take with an IntIn.  (This manager has one context: there is no host route here.)
    Query resolveSubqueries(const Query &q) {
        subPaths_.clear();
        Query out = q;
        out.select = resolveSelect(*q.select);
        return out;
    }
    std::shared_ptr<SelectADT> resolveSelect(const SelectADT &s) {
        if (s.kind == SelectADT::And) return SelectADT::mkAnd(resolveSelect(*s.op1), resolveSelect(*s.op2));
        if (s.kind == SelectADT::Or) return SelectADT::mkOr(resolveSelect(*s.op1), resolveSelect(*s.op2));
        if (s.kind == SelectADT::Select && s.cond.kind == SelectCondition::IntInQuery) return SelectADT::mkSelect(s.col, resolveInner(*s.cond.inner));
        return std::make_shared<SelectADT>(s);
    }
    SelectCondition resolveInner(const Query &inner0) {
        const size_t at = subPaths_.size();
        subPaths_.push_back("");
        Query inner = inner0;
        inner.select = resolveSelect(*inner0.select); // (sub-queries of the sub-query first)
        const Table &table = sm_.sm.getTable(inner.table);
        const Column &col = table.getColumn(inner.project.cols.at(0));
        if (col.columnType == ColumnType::STRING) throw Exception("IntInQuery: the inner column `" + col.name + "' is neither int32 nor int8 (Unsupported column vector)");
        std::vector<std::unique_ptr<QueryHandle>> opened;
        std::vector<imm3_query *> sources;
        std::vector<int32_t> columns;
        auto placeOf = [&](const std::vector<Column> &used) -> int32_t {
            for (size_t k = 0; k < used.size(); ++k) if (used[k].name == col.name) return (int32_t)k;
            throw Exception("NoSuchElementException: key not found: " + col.name);
        };
        TablePlan p;
        if (tablePlan(inner, p)) {
            opened.push_back(std::make_unique<QueryHandle>());
            int rc;
            if (p.tree) rc = imm3_query_create_table_expr(sm_.ctx(), p.table, p.usedIdx.data(), (int32_t)p.usedIdx.size(), p.sels.data(), (int32_t)p.sels.size(),
                                                          p.prog.data(), (int32_t)p.prog.size(), nullptr, 0, 0, table.blockSize, &opened.back()->q);
            else rc = imm3_query_create_table(sm_.ctx(), p.table, p.usedIdx.data(), (int32_t)p.usedIdx.size(), p.sels.data(), (int32_t)p.sels.size(),
                                              nullptr, 0, 0, table.blockSize, &opened.back()->q);
            if (p.tree && tableTreeRefused(rc)) opened.clear();
            else {
                imm3Check(rc);
                sources.push_back(opened.back()->q);
                columns.push_back(placeOf(p.used));
                subPaths_[at] = "set/table";
            }
        }
        if (sources.empty()) {
            subPaths_[at] = "set/segments";
            const std::vector<Column> used = getColumns(inner, table);
            std::vector<Leaf> leaves;
            std::vector<int32_t> prog;
            const bool tree = asTree(inner);
            if (tree) SelectTreeOp::program(*inner.select, leaves, prog, notTree(inner));
            else leaves = resolveSelectOps(inner);
            SelectOp::checkConditions(leaves);
            const int nseg = sm_.sm.getTableSegmentCount(table.name);
            for (int seg = 0; seg < nseg; ++seg) {
                ScanOp scan(sm_, seg, inner.table, used);
                opened.push_back(std::make_unique<QueryHandle>());
                scan.makeQuery(leaves, {}, 0, *opened.back(), tree ? &prog : nullptr);
                sources.push_back(opened.back()->q);
                columns.push_back(placeOf(used));
            }
        }
        if (sources.empty()) return SelectCondition::intIn({}); // no segment at all: the empty list
        imm3_int_set *set = nullptr;
        imm3Check(imm3_int_set_create(sm_.ctx(), sources.data(), columns.data(), (int32_t)sources.size(), &set)); // (runs every source's select chain; sources are not retained)
        return SelectCondition::intInSet(std::shared_ptr<void>(set, [](void *h) { imm3_int_set_destroy((imm3_int_set *)h); }));
    }

    std::vector<AggMapTuple> executeAgg(const Query &q) {
        if (hasSubquery(*q.select)) return executeAgg(resolveSubqueries(q));
        if (!hasResolvedSet(*q.select)) subPaths_.clear(); // (a resolved statement keeps what its resolution recorded)
        const Table &table = sm_.sm.getTable(q.table);
        const std::vector<Column> used = getColumns(q, table);
        const std::vector<Leaf> leaves = resolveSelectOps(q);
        const std::vector<Aggregator> aggs = resolveProjectOp(q.project, table);
        path_ = "per-segment queries";
        {   // one table-level aggregation query: groups come back already merged in (segment, row) first-seen order
            TablePlan p;
            if (tablePlan(q, p)) {
                auto scan = std::make_shared<ScanOp>(sm_, 0, q.table, p.used);
                ProjectAggOp op(aggs, scan, q.project.groupBy, q.project.orderBy, q.project.limit, q.project.having);
                std::vector<AggMapTuple> merged;
                if (op.runOn(p.table, p.used, p.usedIdx, p.sels, p.tree ? &p.prog : nullptr, merged)) {
                    path_ = p.tree ? "one table query: select tree" : "one table query";
                    return merged;
                }
                path_ = std::string("per-segment queries: ") + imm3_last_error();
            }
        }
        auto mkScan = ScanOp::mkScanOp(sm_, q.table);
        std::vector<AggMapTuple> result;
        std::vector<RawKey> raw; // parallel to `result`: the first arrival's key parts
        const std::vector<GroupOrderEntry> spec = groupOrderSpec(aggs, q.project.groupBy, q.project.orderBy);
        std::vector<GroupFilterLeaf> filterLeaves;
        std::vector<int32_t> filterProg;
        groupFilterSpec(aggs, q.project.groupBy, q.project.having.get(), filterLeaves, filterProg);
        const int nseg = sm_.sm.getTableSegmentCount(table.name);
        // count(distinct): no table query answered -- a single segment still does (its query's figure is the table's), several queries'
        // groups cannot be combined
        for (const auto &a : aggs)
            if (a.kind == Aggregator::CountDistinctAggr && nseg > 1)
                throw Exception(std::string(kCountDistinctOneQuery) + ": the table's " + std::to_string(nseg) + " segments would run as per-segment queries (" + path_ + ")");
        for (int seg = 0; seg < nseg; ++seg) {
            std::shared_ptr<ColumnVectorOperator> op = mkScan(used, seg);
            op = selectOps(q, leaves, op);
            ProjectAggOp agg(aggs, op, q.project.groupBy);
            auto it = agg.iterator();
            for (size_t at = 0; it->hasNext(); ++at) {
                AggMapTuple t = it->next();
                bool merged = false;
                for (auto &r : result)
                    if (r.first == t.first) {
                        for (size_t j = 0; j < r.second.size() && j < t.second.size(); ++j) r.second[j].combine(t.second[j]);
                        merged = true;
                        break;
                    }
                if (!merged) {
                    result.push_back(std::move(t));
                    raw.push_back(agg.rawKeys().at(at));
                }
            }
        }
        filterGroups(result, raw, filterLeaves, filterProg); // HAVING over the merged groups, before their order
        // the merged groups ordered on the host, ties in merged first-arrival order, then the limit
        std::vector<Column> groupCols;
        for (const auto &c : used)
            for (const auto &g : q.project.groupBy) if (c.name == g) { groupCols.push_back(c); break; }
        orderGroups(result, raw, groupCols, spec, q.project.limit);
        return result;
    }
    std::vector<Row> execute(const Query &q) {
        if (q.project.kind == ProjectADT::ProjectAgg) {
            std::vector<Row> rows;
            for (const auto &t : executeAgg(q)) {
                std::vector<Value> xs;
                for (const auto &a : t.second) xs.push_back(Value::ofString(a.repr()));
                rows.push_back(Row::fromSeq(std::move(xs)));
            }
            return rows;
        }
        if (hasSubquery(*q.select)) return execute(resolveSubqueries(q));
        if (!hasResolvedSet(*q.select)) subPaths_.clear();
        if (q.project.kind != ProjectADT::Project) throw Exception("NoProject");
        const std::vector<std::pair<int, bool>> okeys = orderKeys(q.project.cols, q.project.orderBy); // (throws for a key outside the SELECT list)
        const bool ordered = !okeys.empty();
        const int createLimit = ordered ? 0 : q.project.limit; // an order's limit is applied behind the order (imm3_query_set_order)
        path_ = "per-segment queries";
        {   // the whole table in ONE fused launch when it qualifies
            TablePlan p;
            bool planned = tablePlan(q, p);
            QueryHandle h;
            std::vector<int32_t> proj;
            std::vector<Column> pcols;
            if (planned) {
                for (const auto &name : q.project.cols) {
                    bool found = false;
                    for (size_t k = 0; k < p.used.size() && !found; ++k)
                        if (p.used[k].name == name) { proj.push_back((int32_t)k); pcols.push_back(p.used[k]); found = true; }
                    if (!found) throw Exception("NoSuchElementException: key not found: " + name);
                }
                if (p.tree) {
                    const int rc = imm3_query_create_table_expr(sm_.ctx(), p.table, p.usedIdx.data(), (int32_t)p.usedIdx.size(), p.sels.data(), (int32_t)p.sels.size(),
                                                                p.prog.data(), (int32_t)p.prog.size(), proj.data(), (int32_t)proj.size(), createLimit,
                                                                sm_.sm.getTable(q.table).blockSize, &h.q);
                    if (tableTreeRefused(rc)) { planned = false; path_ = std::string("per-segment queries: ") + imm3_last_error(); }
                    else imm3Check(rc);
                } else
                imm3Check(imm3_query_create_table(sm_.ctx(), p.table, p.usedIdx.data(), (int32_t)p.usedIdx.size(), p.sels.data(), (int32_t)p.sels.size(),
                                                  proj.data(), (int32_t)proj.size(), createLimit, sm_.sm.getTable(q.table).blockSize, &h.q));
            }
            if (planned) {
                if (ordered) ProjectOp::setOrder(h.q, okeys, q.project.limit); // ONE ordered table query: sorted on the device
                imm3Check(imm3_query_run(h.q));
                path_ = "one table query";
                if (p.tree) { // the tree's one launch over all segments: say which kernel the library ran (imm3_diag.h)
                    int32_t form = -1;
                    imm3Check(imm3_query_expr_form(h.q, &form));
                    path_ += ": select tree, " + std::string(form == 0 ? "tile form" : form == 1 ? "generic form" : "no launch (selects nothing)");
                }
                uint64_t n = 0;
                imm3Check(imm3_query_row_count(h.q, &n));
                std::vector<std::vector<uint8_t>> bufs(pcols.size());
                std::vector<void *> ptrs(pcols.size());
                for (size_t j = 0; j < pcols.size(); ++j) {
                    bufs[j].resize((size_t)std::max<uint64_t>(n, 1) * (size_t)pcols[j].width());
                    ptrs[j] = bufs[j].data();
                }
                imm3Check(imm3_query_fetch_rows(h.q, nullptr, ptrs.data(), n));
                std::vector<Row> rows;
                rows.reserve((size_t)n);
                for (uint64_t i = 0; i < n; ++i) {
                    std::vector<Value> xs;
                    for (size_t j = 0; j < pcols.size(); ++j) {
                        ColumnVector v;
                        v.type = pcols[j].columnType;
                        v.width = pcols[j].width();
                        v.data = bufs[j].data();
                        xs.push_back(v.value((int)i));
                    }
                    rows.push_back(Row::fromSeq(std::move(xs)));
                }
                return rows;
            }
        }
        const Table &table = sm_.sm.getTable(q.table);
        const std::vector<Column> used = getColumns(q, table);
        const std::vector<Leaf> leaves = resolveSelectOps(q);
        auto mkScan = ScanOp::mkScanOp(sm_, q.table);
        auto mkProj = ProjectOp::mkProjectOp(q.project.cols, q.project.limit, q.project.orderBy);
        std::vector<Row> rows;
        const int nseg = sm_.sm.getTableSegmentCount(table.name);
        if (ordered) {
            // per-segment ordered queries, each with the limit (no segment can contribute more), then a stable merge: the segments'
            // results are appended in segment order, each in (keys, row) order, so a stable sort by the keys is by (keys, segment, row)
            for (int seg = 0; seg < nseg; ++seg) {
                std::shared_ptr<ColumnVectorOperator> op = mkScan(used, seg);
                op = selectOps(q, leaves, op);
                auto it = mkProj(op)->iterator();
                while (it->hasNext()) rows.push_back(it->next());
            }
            std::stable_sort(rows.begin(), rows.end(), [&okeys](const Row &a, const Row &b) { return rowBefore(a, b, okeys); });
            if (q.project.limit > 0 && rows.size() > (size_t)q.project.limit) rows.resize((size_t)q.project.limit);
            return rows;
        }
        for (int seg = 0; seg < nseg; ++seg) {
            if (q.project.limit > 0 && (int)rows.size() >= q.project.limit) break;
            std::shared_ptr<ColumnVectorOperator> op = mkScan(used, seg);
            op = selectOps(q, leaves, op);
            auto it = mkProj(op)->iterator();
            while (it->hasNext() && !(q.project.limit > 0 && (int)rows.size() >= q.project.limit)) rows.push_back(it->next());
        }
        return rows;
    }

    // which way the last execute / executeAgg went: "one table query[: select tree, <kernel form>]", or "per-segment queries[: <the
    // library's refusal of the tree>]" (imm3_sql --explain prints it)
    // ... and, for a statement with sub-queries, how each ran, outermost first: "set/table" (one table query was the set's source) or
    // "set/segments" (per-segment queries were)
    std::string lastPath() const {
        std::string out = path_;
        for (size_t i = 0; i < subPaths_.size(); ++i) out += (i ? "," : "; sub-queries: ") + subPaths_[i];
        return out;
    }

  private:
    GpuSegmentManager &sm_;
    bool honourAndOr_ = false, honourNotMatch_ = false;
    std::string path_;
    std::vector<std::string> subPaths_;
};

} // namespace immutabledb
