// tests/subtree_dump.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
//
// oracle/schedule_dump for the subtree mode (-m N): runs the host mirror up to the level schedule once per subtree of the partition
// (tree -> partition -> per subtree: its own tree, rerooted -> its sequences -> scheduling) and prints, one JSON document per line and
// subtree in ascending subtree index, what oracle/msa_replay.py needs to replay that subtree on its own: the format of schedule_dump plus
// "subtree" (its index, -1 for a tree that is not split) and "root_in_tree" (the name of its root in the whole tree).
// tests/subtree_oracle.py builds it with plain g++ from the host sources and holds its partition to a Python restatement.
//   subtree_dump <CLI flags as for twilight-mi355x, with -m N> > dumps.jsonl
#include "../twilight_amd/csrc/host/twl_host.hpp"

#include <algorithm>
#include <cstdio>
#include <iostream>
#include <stack>

static void jstr(const std::string &s)
{
    putchar('"');
    for (char c : s) { if (c == '"' || c == '\\') putchar('\\'); putchar(c); }
    putchar('"');
}

static void dumpSubtree(msa::Option &option, msa::Node *rootInTree, int subtree)
{
    msa::SequenceDB db;
    db.updateSeqTh = option.updateSeqTh;
    msa::Tree *subT = new msa::Tree(rootInTree, option.reroot);
    msa::io::readSequences(option.seqFile, &db, &option, subT);
    std::vector<msa::NodePairVec> levels;
    msa::progressive::scheduling(subT->root, levels, 0);
    printf("{\"subtree\":%d,\"root_in_tree\":", subtree);
    jstr(rootInTree->identifier);
    printf(",\"type\":\"%c\",\"root\":", option.type);
    jstr(subT->root->identifier);
    printf(",\"sequences\":[");
    for (size_t i = 0; i < db.sequences.size(); ++i) {
        auto *s = db.sequences[i];
        printf("%s{\"id\":%d,\"name\":", i ? "," : "", s->id);
        jstr(s->name);
        printf(",\"weight\":%.9g,\"low_quality\":%d,\"subtree_idx\":%d,\"seq\":", s->weight, s->lowQuality ? 1 : 0, s->subtreeIdx);
        jstr(std::string(s->alnStorage[s->storage], (size_t)s->len));
        printf("}");
    }
    printf("],\"nodes\":{");
    bool first = true;
    std::stack<msa::Node *> st;
    st.push(subT->root);
    while (!st.empty()) {
        msa::Node *n = st.top(); st.pop();
        printf("%s", first ? "" : ",");
        first = false;
        jstr(n->identifier);
        printf(":{\"leaf\":%d,\"grp\":%d,\"children\":[", n->is_leaf() ? 1 : 0, n->grpID);
        for (size_t c = 0; c < n->children.size(); ++c) { if (c) putchar(','); jstr(n->children[c]->identifier); st.push(n->children[c]); }
        printf("]}");
    }
    printf("},\"levels\":[");
    for (size_t l = 0; l < levels.size(); ++l) {
        printf("%s[", l ? "," : "");
        for (size_t i = 0; i < levels[l].size(); ++i) { if (i) putchar(','); putchar('['); jstr(levels[l][i].first->identifier); putchar(','); jstr(levels[l][i].second->identifier); putchar(']'); }
        printf("]");
    }
    printf("]}\n");
    delete subT;
}

int main(int argc, char **argv)
{
    msa::Option option;
    if (!msa::parseCommandLine(argc, argv, option, false, false, true)) return 1;
    msa::Tree *T = new msa::Tree(option.treeFile);
    phylogeny::PartitionInfo P((size_t)option.maxSubtree, 0, 0);
    P.partitionTree(T->root);
    if (P.partitionsRoot.size() <= 1) {
        phylogeny::assignSinglePartition(T->root);
        dumpSubtree(option, T->root, -1);
    } else {
        std::vector<std::pair<int, msa::Node *>> order;
        for (auto &kv : P.partitionsRoot) order.push_back({kv.second.first->grpID, kv.second.first});
        std::sort(order.begin(), order.end());
        for (auto &o : order) dumpSubtree(option, o.second, o.first);
    }
    delete T;
    return 0;
}
