// imm3_sql -- the reference's SqlCli (engine/src/main/scala/immutabledb/SqlCli.scala:22-76) on the GPU path.
//   imm3_sql -q "select id, age from test_100 where (age > 18 and age < 30) limit 10" -d <dataDir> [--device n]
// Prints one `Row(...)` per line, like `println(it.next)` (SqlCli.scala:72).
//   --parse-only   print the parsed Query ADT and the planner's column order / leaves; no GPU needed.
//   --honour-and-or  run an `or` of the where clause as a disjunction (default off: the reference executes every Or as an And,
//                  Engine.scala:236-245).  With --parse-only it also prints the tree's postfix program.
//   --order-by     accept `order by f [asc|desc] {, f [asc|desc]}` between the where clause and `limit` (default off: the reference's
//                  grammar, in which such a statement does not parse); the rows come back sorted on the GPU, `limit` applied behind the order.
//                  An aggregation takes the clause behind its `group by`: `select count(id), max(age) from t group by state order by
//                  id_count desc limit 10` -- a key is a group-by column, an alias (<col>_count / _max / _min) or the aggregate call itself.
//   --having       accept `having <hfilter>` behind an aggregation's `group by` (default off: such a statement does not parse): and / or
//                  lists over `alias|aggregate call  > | < | =  integer`; the groups are filtered on the GPU BEFORE the order and the
//                  limit of --order-by.
//   --count-distinct  accept `count(distinct f)` wherever an aggregate call may stand (default off: such a statement does not parse): the
//                  number of distinct values of f per group, exact, counted on the GPU (f: int32, int8 or a string of at most 4 bytes).
//                  The statement runs as ONE table query (or its single segment's); a table that would need per-segment queries is
//                  refused: "count(distinct) runs as one table query only".
//   --string-ranges  accept `f like 'value%'`, `f > 'value'` and `f < 'value'` on string columns (default off: the reference's grammar, in
//                  which such a statement does not parse): byte-order prefix / range predicates, run on the GPU.  With --parse-only and a
//                  data directory, the leaves of such conditions are also printed as the bytes the library gets ("leafbytes:").
//   --subqueries   accept `f in (select g from t where ...)` on int32 / int8 columns (default off: such a statement does not parse): the
//                  semi-join.  The inner selection's distinct values become a set built and kept on the GPU (imm3_int_set_create), the
//                  outer statement probes it; --explain also says how the sub-queries ran.
//   --explain      after the rows, one line on stderr: whether the query ran as one table query or per segment ("path: ...").
#include <chrono>
#include <cstdio>
#include <cstring>
#include <iostream>

#include "../operators.hpp"
#include "../sql.hpp"

using namespace immutabledb;

static std::string showSelect(const SelectADT &s) { return showSelectADT(s); }

static std::string showQuery(const Query &q) {
    std::string p;
    auto list = [](const std::vector<std::string> &v) { std::string s = "List("; for (size_t i = 0; i < v.size(); ++i) { if (i) s += ", "; s += v[i]; } return s + ")"; };
    if (q.project.kind == ProjectADT::Project) {
        p = "Project(" + list(q.project.cols) + "," + std::to_string(q.project.limit);
        if (!q.project.orderBy.empty()) { // (only under --order-by: the reference's Project has two fields)
            p += ",List(";
            for (size_t i = 0; i < q.project.orderBy.size(); ++i) p += std::string(i ? ", " : "") + "(" + q.project.orderBy[i].first + "," + (q.project.orderBy[i].second ? "desc" : "asc") + ")";
            p += ")";
        }
        p += ")";
    }
    else {
        static const char *names[] = {"Sum", "Avg", "Min", "Max", "Count", "CountDistinct"};
        p = "ProjectAgg(List(";
        for (size_t i = 0; i < q.project.aggs.size(); ++i) { if (i) p += ", "; p += std::string(names[q.project.aggs[i].kind]) + "(" + q.project.aggs[i].col + ",None)"; }
        p += ")," + list(q.project.groupBy);
        if (!q.project.orderBy.empty() || q.project.limit > 0 || q.project.having) { // (only under --order-by / --having: the reference's ProjectAgg has two fields)
            p += ",List(";
            for (size_t i = 0; i < q.project.orderBy.size(); ++i) p += std::string(i ? ", " : "") + "(" + q.project.orderBy[i].first + "," + (q.project.orderBy[i].second ? "desc" : "asc") + ")";
            p += ")," + std::to_string(q.project.limit);
            if (q.project.having) p += ",Some(" + showSelect(*q.project.having) + ")";
        }
        p += ")";
    }
    return "Query(" + q.table + "," + showSelect(*q.select) + "," + p + ")";
}

int main(int argc, char **argv) {
    std::string query, dataDir;
    int device = 0, repeat = 0;
    bool parseOnly = false, honourAndOr = false, explain = false, orderBy = false, stringRanges = false, having = false, countDistinct = false, intLists = false, subqueries = false;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if ((a == "-q" || a == "--query") && i + 1 < argc) query = argv[++i];
        else if ((a == "-d" || a == "--data-dir") && i + 1 < argc) dataDir = argv[++i];
        else if (a == "--device" && i + 1 < argc) device = std::atoi(argv[++i]);
        else if (a == "--cpu-count" && i + 1 < argc) ++i; // accepted for SqlCli compatibility; segments run on the GPU
        else if (a == "--parse-only") parseOnly = true;
        else if (a == "--honour-and-or") honourAndOr = true;
        else if (a == "--order-by") orderBy = true;
        else if (a == "--string-ranges") stringRanges = true;
        else if (a == "--having") having = true;
        else if (a == "--count-distinct") countDistinct = true;
        else if (a == "--int-lists") intLists = true;
        else if (a == "--subqueries") subqueries = true;
        else if (a == "--explain") explain = true;
        else if (a == "--repeat" && i + 1 < argc) repeat = std::atoi(argv[++i]); // re-run the query N times on the resident table, time to stderr
        else { std::fprintf(stderr, "Error parsing arguments: %s\n", a.c_str()); return 2; }
    }
    if (query.empty() || (dataDir.empty() && !parseOnly)) {
        std::fprintf(stderr, "Usage: imm3_sql -q <sql> -d <dataDir> [--device n] [--parse-only] [--honour-and-or] [--order-by] [--having] [--count-distinct] [--string-ranges] [--int-lists] [--subqueries] [--explain]\n");
        return 2;
    }
    try {
        const Query q = SQLParser::parseAll(query, orderBy, stringRanges, having, countDistinct, intLists, subqueries);
        if (parseOnly) {
            std::cout << showQuery(q) << "\n";
            if (!dataDir.empty()) {
                SegmentManager sm(dataDir);
                const Table &t = sm.getTable(q.table);
                std::cout << "usedColumns:";
                for (const auto &c : Engine::getColumns(q, t)) std::cout << " " << c.name;
                std::cout << "\nleaves:";
                for (const auto &l : Engine::resolveSelectOps(q)) std::cout << " " << l.col << ":" << l.cond.toString();
                std::cout << "\n";
                if (stringRanges) { // the range leaves as the C ABI gets them: column:lo:hi, the bounds in hex
                    auto hex = [](const std::string &b) { static const char *d = "0123456789abcdef"; std::string h; for (unsigned char ch : b) { h += d[ch >> 4]; h += d[ch & 15]; } return h; };
                    std::cout << "leafbytes:";
                    for (const auto &l : Engine::resolveSelectOps(q))
                        if (l.cond.isStrRange()) {
                            const auto b = l.cond.abiValues(t.getColumn(l.col).width());
                            std::cout << " " << l.col << ":" << hex(b[0]) << ":" << hex(b[1]);
                        }
                    std::cout << "\n";
                }
            }
            if (honourAndOr && SelectTreeOp::hasOr(*q.select)) { // leaf index | AND | OR, post-order (include/imm3.h: select trees)
                std::vector<Leaf> leaves;
                std::vector<int32_t> prog;
                SelectTreeOp::program(*q.select, leaves, prog);
                std::cout << "program:";
                for (int32_t op : prog) std::cout << " " << (op == IMM3_EXPR_AND ? std::string("AND") : op == IMM3_EXPR_OR ? std::string("OR") : std::to_string(op));
                std::cout << "\n";
            }
            return 0;
        }
        SegmentManager sm(dataDir);
        GpuSegmentManager gsm(sm, device);
        Engine engine(gsm, honourAndOr);
        for (const Row &r : engine.execute(q)) std::cout << r.toString() << "\n";
        if (explain) std::fprintf(stderr, "path: %s\n", engine.lastPath().c_str());
        for (int k = 0; k < repeat; ++k) { // segments are resident now: this is the steady-state query time
            const auto t0 = std::chrono::steady_clock::now();
            const size_t n = engine.execute(q).size();
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            std::fprintf(stderr, "repeat %d: %.3f ms (%zu rows)\n", k, ms, n);
        }
    } catch (const std::exception &e) {
        std::cout << e.what() << "\n"; // res.fold(err => println(err), ...)
        return 1;
    }
    return 0;
}
