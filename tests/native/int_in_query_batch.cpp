// host/operators.hpp's Engine over a file of SQL statements with IN (sub-query), for tests/test_gpu_int_in_query.py: one SegmentManager /
// GpuSegmentManager / Engine for the whole file.
//   int_in_query_batch <dataDir> <file>
// One statement per line, parsed with the int-lists and the sub-queries extensions on (and no other).  Per statement:
// `== <line no> path: <engine.lastPath()>`, then its `Row(..)` lines.  A statement the parser or the engine throws on prints
// `== <line no> error: <what>` and ends the run there (exit status 4): it may be a device error, and nothing more is started on a device
// that has just failed.  Exit status 2: bad arguments or an unreadable file; 3: the managers could not be made; 4: see above.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>

#include "../../immutable3_amd/host/operators.hpp"
#include "../../immutable3_amd/host/sql.hpp"

using namespace immutabledb;

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    std::ifstream in(argv[2]);
    if (!in) return 2;
    try {
        SegmentManager sm(argv[1]);
        GpuSegmentManager gsm(sm, 0);
        Engine engine(gsm, false);
        std::string line;
        for (int n = 1; std::getline(in, line); ++n) {
            try {
                const Query q = SQLParser::parseAll(line, false, false, false, false, true, true);
                const std::vector<Row> rows = engine.execute(q);
                std::cout << "== " << n << " path: " << engine.lastPath() << "\n";
                for (const Row &r : rows) std::cout << r.toString() << "\n";
            } catch (const std::exception &e) {
                std::cout << "== " << n << " error: " << e.what() << "\n";
                return 4;
            }
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
