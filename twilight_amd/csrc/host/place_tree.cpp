// twilight_amd/csrc/host/place_tree.cpp -- PLACE_W_TREE: new sequences placed into an existing alignment where a guide tree says they belong
// (reference src/twilight-main.cpp:237-291 without -m, `twilight -t tree.nwk -a backbone.aln -i new.fa -o out.aln`; here behind --place-on-tree).
//
// The tree holds the backbone's rows and the new sequences as leaves.  The new leaves and all their ancestors are "placed"; every placed
// node takes as members the backbone leaves below its unplaced children: one group of rows per placed node, aligned among themselves as
// the backbone has them.  The placed nodes alone form the placement tree, on which the ordinary progressive alignment runs: a node that
// brings members is one more side of a pair.  So the groups are re-aligned AGAINST EACH OTHER by the DP -- the backbone's columns survive
// within a group, not between groups.  That is the reference's behaviour.
//
// Host (this file, first half; tests/place_tree_dump.cpp prints it): both reads, Tree::reroot(true), the marks, the groups, the placement tree
// (SequenceDB::getPlacementTree, sequencedb.cpp:148-246).  Device: the columns that are all '-' inside a group leave it (:171-210, a host
// loop there) in ONE call for all groups, twl_store_squeeze_groups (include/twl_backbone.h), on the run's own store right behind the
// upload; then the levels of the device-resident kernel, unchanged.
//
// Deliberate differences from the reference, which crashes or reads past a row in these cases: a backbone whose rows differ in length, and
// a tree leaf found in neither file, end the run with a message.
#include "twl_host.hpp"

#include <algorithm>
#include <functional>
#include <iostream>
#include <string>
#include <vector>

namespace msa {

Tree *readPlacementInputs(Option &option, SequenceDB &database, Tree *subT, PlacementGroups &groups)
{
    // ---- the two reads, backbone first: weights are the tree's as it stands, before the reroot (twilight-main.cpp:256-258) ----
    io::readSequences(option.backboneAlnFile, &database, &option, subT);
    const int B = (int)database.sequences.size();
    for (int i = 1; i < B; ++i)
        if (database.sequences[i]->len != database.sequences[0]->len) {
            std::cerr << "ERROR: length of \"" << database.sequences[i]->name << "\" (" << database.sequences[i]->len << ") does not match in " << option.backboneAlnFile << " ("
                      << database.sequences[0]->len << "): the rows of a backbone alignment must all have one length.\n";
            exit(1);
        }
    if (option.debug)                                       // --check compares a row without its gaps (sequencedb.cpp:19-25: '-' only)
        for (int i = 0; i < B; ++i) { std::string &u = database.sequences[i]->unalignedSeq; u.erase(std::remove(u.begin(), u.end(), '-'), u.end()); }
    io::readSequences(option.seqFile, &database, &option, subT);
    for (auto &kv : subT->allNodes)
        if (kv.second->is_leaf() && !database.name_map.count(kv.first)) {
            std::cerr << "ERROR: the tree's leaf \"" << kv.first << "\" is neither a row of " << option.backboneAlnFile << " nor a sequence of " << option.seqFile
                      << ": placement along a tree needs every leaf in one of the two files.\n";
            exit(1);
        }
    groups.backboneRows = B;
    groups.backboneLen = database.sequences[0]->len;
    if (option.reroot) subT->reroot(true);

    // ---- the marks: every ancestor of a placed leaf (sequencedb.cpp:150-159) ----
    for (auto &kv : subT->allNodes)
        if (kv.second->is_leaf() && kv.second->placed)
            for (Node *cur = kv.second; cur->parent != nullptr && !cur->parent->placed; cur = cur->parent) cur->parent->placed = true;
    // ---- the groups: a placed node's backbone leaves below its unplaced children, depth first, children in order (:161-170) ----
    std::function<void(Node *, Node *)> addBackbone = [&](Node *owner, Node *node) {
        if (node->is_leaf() && !node->placed) owner->seqsIncluded.push_back(database.name_map[node->identifier]->id);
        for (Node *c : node->children)
            if (!c->placed) addBackbone(owner, c);
    };
    for (auto &kv : subT->allNodes)
        if (kv.second->placed) addBackbone(kv.second, kv.second);
    // a group enters the alignment at the backbone's width until its all-gap columns are out (runPlacementOnTree); num and weight in member order, fp32 (:204-207)
    for (auto &kv : subT->allNodes) {
        Node *n = kv.second;
        if (!n->placed || n->is_leaf() || n->seqsIncluded.empty()) continue;
        n->alnLen = groups.backboneLen;
        n->alnNum = (int)n->seqsIncluded.size();
        n->alnWeight = 0.0f;
        for (int sIdx : n->seqsIncluded) n->alnWeight += database.sequences[sIdx]->weight;
    }
    // ---- the placement tree: the placed nodes, children in the tree's order (:212-239) ----
    Tree *pT = new Tree();
    for (auto &kv : subT->allNodes) {
        const Node *n = kv.second;
        if (!n->placed) continue;
        Node *cp = new Node(n->identifier, n->branchLength);
        cp->level = n->level; cp->weight = n->weight; cp->numLeaves = n->numLeaves; cp->grpID = n->grpID; cp->placed = true;
        cp->seqsIncluded = n->seqsIncluded; cp->alnLen = n->alnLen; cp->alnNum = n->alnNum; cp->alnWeight = n->alnWeight;
        pT->allNodes[cp->identifier] = cp;
    }
    for (auto &kv : pT->allNodes) {
        const Node *n = subT->allNodes[kv.first];
        for (Node *c : n->children)
            if (c->placed) kv.second->children.push_back(pT->allNodes[c->identifier]);
        if (n->parent) kv.second->parent = pT->allNodes[n->parent->identifier];
        else { kv.second->parent = nullptr; pT->root = kv.second; }
    }
    size_t depth = 0, leaves = 0;
    for (auto &kv : pT->allNodes) { depth = std::max(depth, kv.second->level); if (kv.second->is_leaf()) ++leaves; }
    pT->m_numLeaves = leaves;
    pT->m_maxDepth = depth;
    for (auto &kv : pT->allNodes)
        if (!kv.second->is_leaf() && !kv.second->seqsIncluded.empty()) groups.nodes.push_back(kv.second);
    std::sort(groups.nodes.begin(), groups.nodes.end(), [](const Node *a, const Node *b) { return a->identifier < b->identifier; });
    return pT;
}

}  // namespace msa

#ifndef TWL_PLACE_TREE_HOST_ONLY      // (tests/place_tree_dump.cpp takes the half above alone, without the library)

#include "align_gpu.hpp"

#include "../../../include/twl_backbone.h"

#include <chrono>
#include <cstdio>

namespace msa {

int runPlacementOnTree(Option &option)
{
    using progressive::gpu::die;
    using progressive::gpu::nowMs;
    const double t0 = nowMs();
    SequenceDB database;
    database.updateSeqTh = option.updateSeqTh;
    database.trimRequested = option.trimRule >= 0;
    Params param(option, option.type);
    Tree *T = openTree(option);                                              // twilight-main.cpp:238
    phylogeny::assignSinglePartition(T->root);                               // :239-240 without -m
    Tree *subT = new Tree(T->root, false);                                   // :255: not rerooted yet
    PlacementGroups groups;
    Tree *placementT = readPlacementInputs(option, database, subT, groups);  // :256-259
    const double t1 = nowMs();

    // ---- the squeeze, on the run's own store as soon as it exists: all groups in one call, no second upload of the backbone ----
    struct Squeeze { int32_t groups = 0, rows = 0; int64_t colsBefore = 0, colsAfter = 0, bytesRead = 0, bytesWritten = 0; double kernelMs = 0, callMs = 0; } sq;
    progressive::gpu::ctxOf(&database).onStoreCreated = [&](twl_store *st) {
        std::vector<int32_t> off{0}, ids, kept(groups.nodes.size());
        for (const Node *n : groups.nodes) { ids.insert(ids.end(), n->seqsIncluded.begin(), n->seqsIncluded.end()); off.push_back((int32_t)ids.size()); }
        const double ts = nowMs();
        int rc = twl_store_squeeze_groups(st, (int32_t)groups.nodes.size(), off.data(), ids.data(), kept.data());
        if (rc != TWL_OK) die("twl_store_squeeze_groups", rc);
        sq = Squeeze{};
        sq.callMs = nowMs() - ts;
        if ((rc = twl_store_squeeze_timing(st, &sq.kernelMs)) != TWL_OK) die("twl_store_squeeze_timing", rc);
        for (size_t k = 0; k < groups.nodes.size(); ++k) {
            Node *n = groups.nodes[k];
            for (int sIdx : n->seqsIncluded) database.sequences[sIdx]->len = kept[k];
            sq.colsBefore += groups.backboneLen; sq.colsAfter += kept[k];
            sq.bytesRead += 2 * (int64_t)n->seqsIncluded.size() * groups.backboneLen;      // (the flags pass and the compaction both read every row)
            sq.bytesWritten += (int64_t)n->seqsIncluded.size() * kept[k];
            n->alnLen = kept[k];
        }
        sq.groups = (int32_t)groups.nodes.size(); sq.rows = (int32_t)ids.size();
    };

    const alnFunction kernel = progressive::gpu::alignmentKernel_Resident;   // both passes, as in the default mode
    progressive::msaOnSubtree(placementT, &database, &option, param, kernel, kernel);      // :261
    // Tree::extractResult (tree.cpp:698-704): the result goes back to the whole tree's root
    subT->root->seqsIncluded = placementT->root->seqsIncluded;
    if (!placementT->root->msaFreq.empty()) subT->root->msaFreq = placementT->root->msaFreq;
    subT->root->alnLen = placementT->root->alnLen;
    subT->root->alnNum = placementT->root->alnNum;
    subT->root->alnWeight = placementT->root->alnWeight;
    const double t2 = nowMs();
    if (option.debug && !database.debug()) std::cerr << "WARNING: --check found an illegal alignment row.\n";
    int alnLen = subT->root->getAlnLen(database.currentTask);
    const int mergedLen = alnLen;
    if (database.trimRequested) alnLen = database.trimmedLen >= 0 ? database.trimmedLen : trimDatabaseRows(&database, &option, alnLen);      // (trim.cpp: in the last download, or on an uploaded copy)
    io::writeFinalMSA(&database, &option, alnLen);                          // :280: database order -- backbone rows in file order, then the new sequences
    const double t3 = nowMs();
    const size_t levels = progressive::gpu::levelRecords(&database).size();
    std::cerr << "Placed " << (database.sequences.size() - (size_t)groups.backboneRows) << " sequences along the tree into " << groups.backboneRows
              << " backbone rows in " << sq.groups << " groups: final alignment length " << mergedLen << " (backbone " << groups.backboneLen << ")\n";
    if (option.printDetail)
        fprintf(stderr, "Placement-on-tree phases: groups %d, rows %d, columns %lld -> %lld, squeeze kernels %.3f ms (call %.3f ms, row bytes read %lld, written %lld), levels %zu; "
                        "read %.3f ms, align %.3f ms, write %.3f ms\n", sq.groups, sq.rows, (long long)sq.colsBefore, (long long)sq.colsAfter, sq.kernelMs, sq.callMs,
                (long long)sq.bytesRead, (long long)sq.bytesWritten, levels, t1 - t0, t2 - t1, t3 - t2);
    delete placementT;
    delete subT;
    delete T;
    return alnLen;
}

}  // namespace msa

#endif
