// tests/place_tree_dump.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
//
// oracle/schedule_dump for placement along a tree (-t -a -i --place-on-tree): runs the host half of the mode up to the level schedule
// (tree -> both reads -> reroot between placed nodes -> marks -> groups -> placement tree -> scheduling) and prints ONE JSON document:
//   "tree_root", "tree"   the whole tree after the reroot: every node with its children in order, "new": 1 for a leaf read from -i
//   "sequences"           as schedule_dump prints them (id, name, weight, low_quality, subtree_idx, seq = the row as read, gaps included)
//   "groups"              per placed inner node that brings members: their ids in order, "num" and "weight" (fp32, %.9g)
//   "root", "nodes", "levels"   the placement tree after the scheduling and the level batches, in the format of schedule_dump
// tests/place_tree_oracle.py builds it with plain g++ from the host sources (place_tree.cpp with TWL_PLACE_TREE_HOST_ONLY: its first half)
// and holds groups and levels to a Python restatement.
//   place_tree_dump <CLI flags as for twilight-mi355x, with --place-on-tree> > dump.json
// With TWL_DUMP_NO_ROWS set in the environment every "seq" is printed empty (tools/place_tree_bench.py takes the groups of a large input from it).
#include "../twilight_amd/csrc/host/twl_host.hpp"

#include <cstdio>
#include <cstdlib>
#include <stack>

static void jstr(const std::string &s)
{
    putchar('"');
    for (char c : s) { if (c == '"' || c == '\\') putchar('\\'); putchar(c); }
    putchar('"');
}

static void dumpNodes(msa::Node *root, bool marks)
{
    putchar('{');
    bool first = true;
    std::stack<msa::Node *> st;
    st.push(root);
    while (!st.empty()) {
        msa::Node *n = st.top(); st.pop();
        printf("%s", first ? "" : ",");
        first = false;
        jstr(n->identifier);
        printf(":{\"leaf\":%d,", n->is_leaf() ? 1 : 0);
        if (marks) printf("\"new\":%d,", n->is_leaf() && n->placed ? 1 : 0);
        else printf("\"grp\":%d,", n->grpID);
        printf("\"children\":[");
        for (size_t c = 0; c < n->children.size(); ++c) { if (c) putchar(','); jstr(n->children[c]->identifier); st.push(n->children[c]); }
        printf("]}");
    }
    putchar('}');
}

int main(int argc, char **argv)
{
    msa::Option option;
    if (!msa::parseCommandLine(argc, argv, option, true) || option.alnMode != msa::PLACE_W_TREE) return 1;
    msa::SequenceDB db;
    db.updateSeqTh = option.updateSeqTh;
    msa::Tree *T = msa::openTree(option);
    phylogeny::assignSinglePartition(T->root);
    msa::Tree *subT = new msa::Tree(T->root, false);
    msa::PlacementGroups groups;
    msa::Tree *pT = msa::readPlacementInputs(option, db, subT, groups);
    // (a leaf of the whole tree that is new: its mark; an inner node's mark is what the oracle derives)
    printf("{\"type\":\"%c\",\"backbone_rows\":%d,\"backbone_len\":%d,\"tree_root\":", option.type, groups.backboneRows, groups.backboneLen);
    jstr(subT->root->identifier);
    printf(",\"tree\":");
    dumpNodes(subT->root, true);
    printf(",\"sequences\":[");
    for (size_t i = 0; i < db.sequences.size(); ++i) {
        auto *s = db.sequences[i];
        printf("%s{\"id\":%d,\"name\":", i ? "," : "", s->id);
        jstr(s->name);
        printf(",\"weight\":%.9g,\"low_quality\":%d,\"subtree_idx\":%d,\"seq\":", s->weight, s->lowQuality ? 1 : 0, s->subtreeIdx);
        jstr(getenv("TWL_DUMP_NO_ROWS") ? std::string() : std::string(s->alnStorage[s->storage], (size_t)s->len));
        printf("}");
    }
    printf("],\"groups\":{");
    for (size_t k = 0; k < groups.nodes.size(); ++k) {
        const msa::Node *n = groups.nodes[k];
        printf("%s", k ? "," : "");
        jstr(n->identifier);
        printf(":{\"ids\":[");
        for (size_t m = 0; m < n->seqsIncluded.size(); ++m) printf("%s%d", m ? "," : "", n->seqsIncluded[m]);
        printf("],\"num\":%d,\"weight\":%.9g}", n->alnNum, n->alnWeight);
    }
    std::vector<msa::NodePairVec> levels;
    msa::progressive::scheduling(pT->root, levels, 0);
    printf("},\"root\":");
    jstr(pT->root->identifier);
    printf(",\"nodes\":");
    dumpNodes(pT->root, false);
    printf(",\"levels\":[");
    for (size_t l = 0; l < levels.size(); ++l) {
        printf("%s[", l ? "," : "");
        for (size_t i = 0; i < levels[l].size(); ++i) { if (i) putchar(','); putchar('['); jstr(levels[l][i].first->identifier); putchar(','); jstr(levels[l][i].second->identifier); putchar(']'); }
        printf("]");
    }
    printf("]}\n");
    delete pT;
    delete subT;
    delete T;
    return 0;
}
