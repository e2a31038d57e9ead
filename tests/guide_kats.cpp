// tests/guide_kats.cpp -- the host clustering and text of the guide tree (twilight_amd/csrc/host/guide_upgma.hpp: pure, no device) on given
// distance matrices.  Reads cases from stdin until it ends -- "N", N names, N*N distances as C hexadecimal floats (exact) -- and prints the
// Newick text of each; tests/test_guide_tree_cpu.py compares them with tests/guide_oracle.py.  Built with -ffp-contract=off.
#include <cstdio>
#include <cstdlib>
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
        msa::guide::Triangle d(n);
        for (int a = 0; a < n; ++a)
            for (int b = 0; b < n; ++b) {
                std::string tok;
                std::cin >> tok;
                if (a < b) d.at(a, b) = strtod(tok.c_str(), nullptr);
            }
        const std::vector<msa::guide::Merge> merges = msa::guide::upgma(d);
        fputs(msa::guide::newick(names, merges).c_str(), stdout);
    }
    return 0;
}
