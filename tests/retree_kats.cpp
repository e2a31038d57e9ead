// tests/retree_kats.cpp -- the host half of the rebuilt guide tree (twilight_amd/csrc/host/guide_upgma.hpp: pure, no device) on given pair counts.
// Reads cases from stdin until it ends -- "N", N names, N*N match counts, N*N both counts -- and prints for each the distances of the upper
// triangle, row by row, as C hexadecimal floats (exact) on one line, then the Newick text; tests/test_retree_tree_cpu.py compares them with
// tests/retree_oracle.py.  Built with -ffp-contract=off.
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>
#include "../twilight_amd/csrc/host/guide_upgma.hpp"

int main()
{
    int n;
    while (std::cin >> n) {
        std::vector<std::string> names((size_t)n);
        for (auto &s : names) std::cin >> s;
        std::vector<uint32_t> match((size_t)n * n), both((size_t)n * n);
        for (auto &v : match) std::cin >> v;
        for (auto &v : both) std::cin >> v;
        msa::guide::Triangle d = msa::guide::distancesFromCounts(n, match.data(), both.data());
        for (int a = 0; a < n; ++a)
            for (int b = a + 1; b < n; ++b) printf("%a ", d.at(a, b));
        printf("\n");
        const std::vector<msa::guide::Merge> merges = msa::guide::upgma(d);
        fputs(msa::guide::newick(names, merges).c_str(), stdout);
    }
    return 0;
}
