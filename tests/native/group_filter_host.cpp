// filterGroups and groupFilterCompare of immutable3_amd/host/operators.hpp on vectors from stdin, for tests/test_group_filter_host.py (the
// Python operators.filter_groups is held to the same vectors).  No device is touched.  Input, whitespace-separated:
//   L n   then n leaves:  alias cond value        (cond: the C ABI's IMM3_EQ / IMM3_GT / IMM3_LT)
//   P n   then n program entries                  (leaf index, IMM3_EXPR_AND / _OR / _NOT)
//   G n   then n groups:  id_count v_max w_min    (a CountAggr, a MaxDoubleAggr, a MinDoubleAggr)
//   C n   then n compares: lhs count cond value average
// Output: "kept" and the indices of the groups the program keeps, then "cmp" and one 0 / 1 per compare.
#include <iostream>

#include "../../immutable3_amd/host/operators.hpp"

using namespace immutabledb;

int main() {
    std::string tag;
    size_t n = 0;
    std::vector<GroupFilterLeaf> leaves;
    std::vector<int32_t> prog;
    std::vector<AggMapTuple> groups;
    std::vector<RawKey> raw;
    std::vector<int> cmp;
    while (std::cin >> tag >> n) {
        for (size_t i = 0; i < n; ++i) {
            if (tag == "L") {
                GroupFilterLeaf l;
                std::cin >> l.alias >> l.cond >> l.value;
                leaves.push_back(l);
            } else if (tag == "P") {
                int32_t op;
                std::cin >> op;
                prog.push_back(op);
            } else if (tag == "G") {
                long long c, mx, mn;
                std::cin >> c >> mx >> mn;
                AggMap m = {Aggregator::make(Aggregator::CountAggr, "id", "id_count"), Aggregator::make(Aggregator::MaxDoubleAggr, "v", "v_max"),
                            Aggregator::make(Aggregator::MinDoubleAggr, "w", "w_min")};
                m[0].counter = c;
                m[1].dvalue = (double)mx;
                m[2].dvalue = (double)mn;
                groups.emplace_back(std::to_string(i), m);
                raw.push_back(RawKey{std::to_string(i)});
            } else if (tag == "C") {
                GroupFilterLeaf l;
                long long lhs, count;
                int average;
                std::cin >> lhs >> count >> l.cond >> l.value >> average;
                l.average = average != 0;
                cmp.push_back(groupFilterCompare(lhs, count, l) ? 1 : 0);
            } else return 2;
        }
    }
    filterGroups(groups, raw, leaves, prog);
    if (raw.size() != groups.size()) return 3;
    std::cout << "kept";
    for (size_t i = 0; i < groups.size(); ++i) {
        if (raw[i].at(0) != groups[i].first) return 3;
        std::cout << " " << groups[i].first;
    }
    std::cout << "\ncmp";
    for (int c : cmp) std::cout << " " << c;
    std::cout << "\n";
    return 0;
}
