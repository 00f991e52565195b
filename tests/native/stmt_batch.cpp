// host/operators.hpp's Engine over a file of SQL statements, for tests/test_gpu_stmt_fuzz.py: one SegmentManager / GpuSegmentManager /
// Engine for the whole file, so that the C++ engine sees a few hundred statements in a handful of processes.
//   stmt_batch <dataDir> <honourAndOr 0|1> <file>
// One statement per line, parsed with every extension of the grammar on.  Per statement: `== <line no> path: <engine.lastPath()>`, then
// its `Row(..)` lines; a statement the parser or the engine throws on prints `== <line no> error: <what>`.  A line that begins with `!`
// is a statement the caller expects to be refused: after its error the next one runs.  An error nobody expected ends the run there
// (exit status 4): it may be a device error, and nothing more is started on a device that has just failed.
// Exit status 2: bad arguments or an unreadable file; 3: the managers could not be made; 4: see above.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>

#include "../../immutable3_amd/host/operators.hpp"
#include "../../immutable3_amd/host/sql.hpp"

using namespace immutabledb;

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    std::ifstream in(argv[3]);
    if (!in) return 2;
    try {
        SegmentManager sm(argv[1]);
        GpuSegmentManager gsm(sm, 0);
        Engine engine(gsm, std::atoi(argv[2]) != 0);
        std::string line;
        for (int n = 1; std::getline(in, line); ++n) {
            const bool refusal = !line.empty() && line[0] == '!';
            if (refusal) line.erase(0, 1);
            try {
                const Query q = SQLParser::parseAll(line, true, true, true);
                const std::vector<Row> rows = engine.execute(q);
                std::cout << "== " << n << " path: " << engine.lastPath() << "\n";
                for (const Row &r : rows) std::cout << r.toString() << "\n";
            } catch (const std::exception &e) {
                std::cout << "== " << n << " error: " << e.what() << "\n";
                if (!refusal) return 4;
            }
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
