// host/operators.hpp's Engine with honourNotMatch, for tests/test_gpu_expr_not.py: the queries a SQL front end cannot write (the
// grammar has no `not`), built as ADTs.
//   engine_not <dataDir> <query 0|1|2> <honourNotMatch 0|1>
// query 0: state NotMatch(CA); 1: age > 30 And state NotMatch(CA); 2: age > 90 Or state NotMatch(CA) -- over table "tn".
// Prints the projection's rows (id, age) as `Row(..)` lines, then the groups of count(id), max(age) by state as `group Row(..)`
// lines.  Exit status 3 and the message on stderr when the engine throws.
#include <cstdio>
#include <cstdlib>
#include <iostream>

#include "../../immutable3_amd/host/operators.hpp"

using namespace immutabledb;

static std::shared_ptr<SelectADT> leaf(const std::string &col, SelectCondition cond) {
    auto s = std::make_shared<SelectADT>();
    s->kind = SelectADT::Select;
    s->col = col;
    s->cond = std::move(cond);
    return s;
}

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    const int which = std::atoi(argv[2]);
    const bool honour = std::atoi(argv[3]) != 0;
    try {
        SegmentManager sm(argv[1]);
        GpuSegmentManager gsm(sm, 0);
        Engine engine(gsm, false, honour);
        auto notCa = leaf("state", SelectCondition::notMatch({"CA"}));
        Query q;
        q.table = "tn";
        q.select = which == 0 ? notCa : which == 1 ? SelectADT::mkAnd(leaf("age", SelectCondition::gt(30)), notCa) : SelectADT::mkOr(leaf("age", SelectCondition::gt(90)), notCa);
        q.project.kind = ProjectADT::Project;
        q.project.cols = {"id", "age"};
        for (const Row &r : engine.execute(q)) std::cout << r.toString() << "\n";
        Query g = q;
        g.project = ProjectADT{};
        g.project.kind = ProjectADT::ProjectAgg;
        Aggregate count, max;
        count.kind = Aggregate::Count;
        count.col = "id";
        max.kind = Aggregate::Max;
        max.col = "age";
        g.project.aggs = {count, max};
        g.project.groupBy = {"state"};
        for (const Row &r : engine.execute(g)) std::cout << "group " << r.toString() << "\n";
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
