// twilight_amd/csrc/host/guide_stage.hpp -- the host steps of the two-stage guide tree (`--tree-seeds S`) that need no
// device, as pure functions: the seeds, the clusters of an assignment, and the text of the seed tree with every leaf replaced by its
// cluster's tree.  tests/guide_stage_kats.cpp includes this file directly.  Clustering and the text of one tree: guide_upgma.hpp, unchanged.
#pragma once
#include "guide_upgma.hpp"

namespace msa {
namespace guide {

// seed t = floor(t * N / S) in 64-bit integers, t < S; distinct and ascending for 2 <= S <= N
inline std::vector<int32_t> seedIds(int64_t n, int64_t s)
{
    std::vector<int32_t> ids((size_t)s);
    for (int64_t t = 0; t < s; ++t) ids[(size_t)t] = (int32_t)(t * n / s);
    return ids;
}

// K_t = the sequences i with seedOf[i] == t, in input order
inline std::vector<std::vector<int32_t>> clustersOf(int32_t nSeeds, const std::vector<int32_t> &seedOf)
{
    std::vector<std::vector<int32_t>> k((size_t)nSeeds);
    for (size_t i = 0; i < seedOf.size(); ++i) k[(size_t)seedOf[i]].push_back((int32_t)i);
    return k;
}

// One cluster's tree, ready to be grafted: its section 4f text without the ';' and the newline, and the height of its root (0 for one member)
struct Subtree { std::string text; double height = 0; };

inline Subtree subtreeOf(const std::vector<std::string> &names, const std::vector<Merge> &merges)
{
    Subtree s;
    s.text = newick(names, merges);
    s.text.resize(s.text.size() - 2);
    s.height = merges.empty() ? 0.0 : merges.back().height;
    return s;
}

// The seed tree (the merges of the S seeds) with leaf t replaced by sub[t]: the text rule of guide_upgma.hpp's newick on the combined tree, a
// grafted root standing at its own height.
inline std::string graftedNewick(const std::vector<Subtree> &sub, const std::vector<Merge> &merges)
{
    const int n = (int)sub.size();
    if (n == 1) return sub[0].text + ";\n";
    std::string out;
    auto height = [&](int v) { return v < n ? sub[(size_t)v].height : merges[(size_t)(v - n)].height; };
    struct Frame { int v, parent, state; };      // state 0: open, 1: between the children, 2: close
    std::vector<Frame> stack{{n + (int)merges.size() - 1, -1, 0}};
    char num[64];
    while (!stack.empty()) {
        Frame &f = stack.back();
        if (f.v < n) out += sub[(size_t)f.v].text;
        else if (f.state == 0) { out += '('; f.state = 1; stack.push_back(Frame{merges[(size_t)(f.v - n)].left, f.v, 0}); continue; }
        else if (f.state == 1) { out += ','; f.state = 2; stack.push_back(Frame{merges[(size_t)(f.v - n)].right, f.v, 0}); continue; }
        else out += ')';
        if (f.parent >= 0) {
            double len = height(f.parent) - height(f.v);
            if (len < 0) len = 0.0;
            snprintf(num, sizeof num, ":%.6f", len);
            out += num;
        }
        stack.pop_back();
    }
    out += ";\n";
    return out;
}

}  // namespace guide
}  // namespace msa
