// tests/guide_stage_kats.cpp -- the host steps of the two-stage guide tree (twilight_amd/csrc/host/guide_stage.hpp: pure, no device) on given
// assignments and distance matrices.  Reads cases from stdin until it ends -- "N S", N names, N seed indices (the assignment), N*N distances
// as C hexadecimal floats (exact) -- and prints two lines per case: the S seed ids, and the Newick text of the seeds' tree with every leaf
// replaced by its cluster's tree.  The clusters' and the seeds' matrices are cut out of the N x N one, as guide.cpp gets them from the device
// group by group.  tests/test_guide_stage_tree_cpu.py compares the lines with tests/guide_stage_oracle.py.  Built with -ffp-contract=off.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>
#include "../twilight_amd/csrc/host/guide_stage.hpp"

using namespace msa::guide;

static Triangle cut(const std::vector<double> &d, int n, const std::vector<int32_t> &rows)
{
    Triangle t((int)rows.size());
    for (size_t a = 0; a < rows.size(); ++a)
        for (size_t b = a + 1; b < rows.size(); ++b) t.at((int)a, (int)b) = d[(size_t)rows[a] * n + rows[b]];
    return t;
}

int main()
{
    int n, s;
    while (std::cin >> n >> s) {
        std::vector<std::string> names((size_t)n);
        for (auto &x : names) std::cin >> x;
        std::vector<int32_t> seedOf((size_t)n);
        for (auto &x : seedOf) std::cin >> x;
        std::vector<double> d((size_t)n * n);
        for (auto &x : d) { std::string tok; std::cin >> tok; x = strtod(tok.c_str(), nullptr); }
        const std::vector<int32_t> seeds = seedIds(n, s);
        for (int t = 0; t < s; ++t) printf("%d%c", seeds[(size_t)t], t + 1 < s ? ' ' : '\n');
        const std::vector<std::vector<int32_t>> k = clustersOf(s, seedOf);
        std::vector<Subtree> sub((size_t)s);
        for (int t = 0; t < s; ++t) {
            std::vector<std::string> member;
            for (int32_t i : k[(size_t)t]) member.push_back(names[(size_t)i]);
            Triangle dt = cut(d, n, k[(size_t)t]);
            sub[(size_t)t] = subtreeOf(member, upgma(dt));
        }
        Triangle ds = cut(d, n, seeds);
        fputs(graftedNewick(sub, upgma(ds)).c_str(), stdout);
    }
    return 0;
}
