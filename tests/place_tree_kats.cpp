// tests/place_tree_kats.cpp -- known answers of Tree::reroot(true), the reroot of placement along a tree (reference src/tree.cpp:588-696 with
// placement = true: the two searches start at the first placed leaf and only placed nodes count as farthest), derived by hand on trees whose
// longest path between placed leaves is unique and has an odd number of nodes, so the answer depends neither on the start leaf nor on the
// direction the path is walked in.  Also: reroot() without the argument still gives the answer tests/host_kats.cpp derives.
// Prints "OK <name>" / "FAIL <name>".
#include "../twilight_amd/csrc/host/twl_host.hpp"

#include <cstdio>
#include <fstream>
#include <functional>
#include <string>

using msa::Node;
using msa::Tree;

static int g_fail = 0;
#define CHECK(name, cond) do { if (cond) printf("OK %s\n", name); else { printf("FAIL %s\n", name); ++g_fail; } } while (0)

static std::string show(Node *n)
{
    std::string s;
    if (n->is_leaf()) s = n->identifier;
    else { s = "("; for (size_t c = 0; c < n->children.size(); ++c) { if (c) s += ","; s += show(n->children[c]); if (n->children[c]->parent != n) s += "!"; } s += ")"; }
    char b[32]; snprintf(b, sizeof b, ":%g", (double)n->branchLength);
    return s + b;
}

// the tree of `newick`, copied without a reroot as the mode does, the leaves of `placed` marked; then reroot(mode): 0 = reroot(), 1 = reroot(false), 2 = reroot(true)
static std::string rerooted(const std::string &tmp, const char *newick, std::initializer_list<const char *> placed, int mode, bool *sane)
{
    const std::string f = tmp + "/place_tree_kat.nwk";
    { std::ofstream o(f); o << newick << "\n"; }
    Tree T(f);
    const std::string rootName = T.root->identifier;
    phylogeny::assignSinglePartition(T.root);
    Tree *sub = new Tree(T.root, false);
    for (const char *p : placed) sub->allNodes.at(p)->placed = true;
    if (mode == 0) sub->reroot(); else sub->reroot(mode == 2);
    const std::string got = show(sub->root);
    *sane = sub->root->identifier == rootName && sub->root->parent == nullptr && sub->allNodes.at(rootName) == sub->root && sub->root->level == 1;
    for (auto &kv : sub->allNodes) *sane = *sane && kv.second->identifier == kv.first;
    for (const char *p : placed) *sane = *sane && sub->allNodes.at(p)->placed && sub->allNodes.at(p)->is_leaf();
    delete sub;
    return got;
}

int main(int argc, char **argv)
{
    const std::string tmp = argc > 1 ? argv[1] : ".";
    bool sane = false;
    // T1: p1 hangs 4 edges below the root, p2 2 edges: the path p1, V, X, Y, root, W, p2 has 7 nodes, its middle is Y = (((p1,bv),bx),by).  The edge
    // Y - root turns over: the old root keeps W as its only child and is spliced out, W carries 10 + 7; Y's children [X, by, W] get a joint of
    // length 0 for the first two.  The unplaced chain under W is deeper than everything placed: it must not matter.
    const char *T1 = "((((p1:1,bv:2):3,bx:4):5,by:6):7,(p2:8,(c1:1,(c2:1,(c3:1,(c4:1,c5:1):1):1):1):9):10);";
    std::string got = rerooted(tmp, T1, {"p1", "p2"}, 2, &sane);
    if (got != "((((p1:1,bv:2):3,bx:4):5,by:6):0,(p2:8,(c1:1,(c2:1,(c3:1,(c4:1,c5:1):1):1):1):9):17):0") printf("  gave %s\n", got.c_str());
    CHECK("placement_reroot_goes_to_the_middle_of_the_placed_path", sane && got == "((((p1:1,bv:2):3,bx:4):5,by:6):0,(p2:8,(c1:1,(c2:1,(c3:1,(c4:1,c5:1):1):1):1):9):17):0");
    // ... while reroot(false) looks at all leaves: the longest path c4 | c5 ... p1 | bv has 11 nodes whichever ends it takes, its middle is W = (p2, chain)
    const char *T1plain = "((p2:8,(c1:1,(c2:1,(c3:1,(c4:1,c5:1):1):1):1):9):0,(((p1:1,bv:2):3,bx:4):5,by:6):17):0";
    got = rerooted(tmp, T1, {"p1", "p2"}, 1, &sane);
    if (got != T1plain) printf("  gave %s\n", got.c_str());
    CHECK("the_plain_reroot_of_the_same_tree_chooses_another_root", sane && got == T1plain);
    got = rerooted(tmp, T1, {"p1", "p2"}, 0, &sane);
    CHECK("reroot_without_the_argument_is_the_plain_reroot", sane && got == T1plain);
    // T2: three placed leaves; the longest placed path p1, root, Rr, S, C, C2, p3 (7 nodes) is unique (p1 - p2 and p2 - p3 have 5 edges), its middle is
    // S = ((p2,b),(c,(p3,e2))).  Two edges turn over: Rr hangs under S with 5 and takes the old root as its last child with 7; the old root keeps p1 alone
    // and is spliced out, p1 carries 1 + 7.
    const char *T2 = "(p1:1,(((p2:1,b:1):2,(c:1,(p3:1,e2:1):3):4):5,(d:1,(e:1,(f:1,(g:1,h:1):1):1):1):6):7);";
    got = rerooted(tmp, T2, {"p1", "p2", "p3"}, 2, &sane);
    if (got != "(((p2:1,b:1):2,(c:1,(p3:1,e2:1):3):4):0,((d:1,(e:1,(f:1,(g:1,h:1):1):1):1):6,p1:8):5):0") printf("  gave %s\n", got.c_str());
    CHECK("placement_reroot_with_three_placed_leaves", sane && got == "(((p2:1,b:1):2,(c:1,(p3:1,e2:1):3):4):0,((d:1,(e:1,(f:1,(g:1,h:1):1):1):1):6,p1:8):5):0");
    // one placed leaf: the path is that leaf alone; the tree keeps its root (the reference moves the root into the leaf: a deliberate difference)
    got = rerooted(tmp, T1, {"p2"}, 2, &sane);
    if (got != "((((p1:1,bv:2):3,bx:4):5,by:6):7,(p2:8,(c1:1,(c2:1,(c3:1,(c4:1,c5:1):1):1):1):9):10):0") printf("  gave %s\n", got.c_str());
    CHECK("one_placed_leaf_keeps_the_root", sane && got == "((((p1:1,bv:2):3,bx:4):5,by:6):7,(p2:8,(c1:1,(c2:1,(c3:1,(c4:1,c5:1):1):1):1):9):10):0");
    // today's answers on the existing case (tests/host_kats.cpp), through reroot(), reroot(false) and the constructor that reroots
    const char *T3 = "((((A:1,B:2):3,C:4):5,D:6):7,(E:8,F:9):10);";
    const char *T3want = "((((A:1,B:2):3,C:4):5,D:6):0,(E:8,F:9):17):0";
    CHECK("reroot_default_on_the_existing_case", rerooted(tmp, T3, {}, 0, &sane) == T3want && sane);
    CHECK("reroot_false_on_the_existing_case", rerooted(tmp, T3, {}, 1, &sane) == T3want && sane);
    // ... and with every leaf placed the placement reroot is the plain one
    CHECK("all_leaves_placed_is_the_plain_reroot", rerooted(tmp, T3, {"A", "B", "C", "D", "E", "F"}, 2, &sane) == T3want && sane);
    printf("%s\n", g_fail ? "SOME FAILED" : "ALL PASSED");
    return g_fail ? 1 : 0;
}
