// tests/partition_kats.cpp -- the partition of a guide tree (twilight_amd/csrc/host/partition.cpp) in a form a test can hold to known answers.
//   partition_kats <tree.nwk> <m> [<m> ...]
// prints one line per m:
//   PARTITION m=<m> parts=<number of subtrees> leaves=<leaf>:<subtree>,... roots=<subtree>:<root node>:<leaves>,... tree=<root>(<child>(...),<child>)
// leaves in the order of the Newick string, roots in ascending subtree index, the tree of subtrees in child order ("-" when there is none).
// Linked with phylo.cpp and partition.cpp alone (tests/test_partition_cpu.py).
#include "../twilight_amd/csrc/host/twl_host.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>
#include <vector>

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    for (int a = 2; a < argc; ++a) {
        phylogeny::Tree T{std::string(argv[1])};
        phylogeny::PartitionInfo P((size_t)atol(argv[a]), 0, 0);
        P.partitionTree(T.root);
        printf("PARTITION m=%s parts=%zu leaves=", argv[a], P.partitionsRoot.size());
        bool first = true;
        std::function<void(phylogeny::Node *)> leaves = [&](phylogeny::Node *n) {
            if (n->children.empty()) { printf("%s%s:%d", first ? "" : ",", n->identifier.c_str(), n->grpID); first = false; }
            for (phylogeny::Node *c : n->children) leaves(c);
        };
        leaves(T.root);
        std::vector<std::pair<int, std::string>> roots;
        for (auto &kv : P.partitionsRoot) roots.push_back({kv.second.first->grpID, kv.first + ":" + std::to_string(kv.second.second)});
        std::sort(roots.begin(), roots.end());
        printf(" roots=");
        for (size_t k = 0; k < roots.size(); ++k) printf("%s%d:%s", k ? "," : "", roots[k].first, roots[k].second.c_str());
        if (roots.empty()) printf("-");
        phylogeny::Tree *S = phylogeny::constructTreeFromPartitions(T.root, &P);
        printf(" tree=");
        std::function<void(phylogeny::Node *)> show = [&](phylogeny::Node *n) {
            printf("%s", n->identifier.c_str());
            if (n->children.empty()) return;
            printf("(");
            for (size_t c = 0; c < n->children.size(); ++c) { if (c) printf(","); show(n->children[c]); }
            printf(")");
        };
        if (S->root) show(S->root); else printf("-");
        printf("\n");
        delete S;
    }
    return 0;
}
