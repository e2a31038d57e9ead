// tools/micro/squeeze_host.cpp -- context for tools/place_tree_bench.py, not product code: the all-gap columns taken out of every group of backbone
// rows ON THE HOST, the way the reference does it (src/sequencedb.cpp:171-210, restated: per group one pass that marks the columns in which
// some row holds anything but '-', parallel over the columns, then one pass that moves every row's kept bytes to its front, parallel over
// the rows; one group after the other), with OpenMP in place of TBB.  Prints one line: the seconds of the loop over all groups.
//   squeeze_host <backbone.aln> <groups.txt: one line per group, the row numbers of its members>      (OMP_NUM_THREADS sets the threads)
#include <chrono>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include <omp.h>

int main(int argc, char **argv)
{
    if (argc < 3) return 1;
    std::vector<std::string> rows;
    {
        std::ifstream in(argv[1]);
        for (std::string line; std::getline(in, line);) {
            if (!line.empty() && line[0] == '>') rows.emplace_back();
            else if (!rows.empty()) rows.back() += line;
        }
    }
    std::vector<std::vector<int>> groups;
    {
        std::ifstream in(argv[2]);
        for (std::string line; std::getline(in, line);) {
            std::istringstream s(line);
            groups.emplace_back();
            for (int id; s >> id;) groups.back().push_back(id);
            if (groups.back().empty()) groups.pop_back();
        }
    }
    long long before = 0, after = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (const auto &g : groups) {
        const long long L = (long long)rows[g[0]].size();
        std::vector<unsigned char> drop((size_t)L, 1);
#pragma omp parallel for schedule(static)
        for (long long j = 0; j < L; ++j)
            for (int id : g)
                if (rows[id][(size_t)j] != '-') { drop[(size_t)j] = 0; break; }
#pragma omp parallel for schedule(static)
        for (long long k = 0; k < (long long)g.size(); ++k) {
            std::string &r = rows[g[(size_t)k]];
            size_t at = 0;
            for (long long j = 0; j < L; ++j)
                if (!drop[(size_t)j]) r[at++] = r[(size_t)j];
            r.resize(at);
        }
        before += L;
        after += (long long)rows[g[0]].size();
    }
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("groups %zu threads %d columns %lld -> %lld seconds %.6f\n", groups.size(), omp_get_max_threads(), before, after, s);
    return 0;
}
