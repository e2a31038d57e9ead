// twilight_amd/csrc/host/subtrees.cpp -- DEFAULT_ALN with -m / --max-subtree N: the guide tree aligned in subtrees, their profiles merged
// (reference src/twilight-main.cpp:129-192, `twilight -t tree.nwk -i seqs.fa -o out.aln -m N`).
//
// Phase A, per subtree in ascending index (:139-176): a fresh SequenceDB, the subtree's own tree (rerooted unless --rooted), its sequences
// (length median and low-quality flags are therefore per subtree), msaOnSubtree with the device-resident level kernel for both passes.
// What is kept of a subtree: the rows that are written (everything not lowQuality) with their names, root->alnLen, alnNum =
// root->seqsIncluded.size(), root->alnWeight (updateSubrootInfo, tree.cpp:519-526) and its profile (storeSubtreeProfile,
// sequencedb.cpp:122-138): root->msaFreq when the pass left one, otherwise the rows of root->seqsIncluded added up in that order in fp32,
// each weighted by its sequence weight (twl_store_weighted_columns, include/twl_subtree.h).  root->seqsIncluded is what
// progressive::updateAlignment leaves: the members the root had and then every sequence of the subtree's database once more (all of
// them carry the subtree index -1: io.cpp:84 with tree.cpp:252), so the reference adds every row twice, at two places of the order, and
// counts it twice in alnNum.  The device call takes every id once, so the list goes up as rows of a store of its own, one row per ENTRY
// of the list, and the profile comes back to the host; sequences that --filter excluded have no row of the alignment's length and are left
// out of the sum (the reference reads past their end).
//
// Phase B (:177-192, merge.cpp generalised): the kept rows of all subtrees in one store, one group per subtree, its profile the cached
// profile of the group's id; scheduling mode 1 over the tree of the subtrees' roots; every level goes to the device as one level of
// n pairs (progressive::gpu::mergeProfileLevel, shared with the merge of a directory); no row is touched until twl_merge_finish rewrites
// every row once through its subtree's map.  One read-back, then the output: subtrees in ascending index, rows in input order.
// Deliberate differences from the reference: no temporary directory (-d, -k, -c are not part of this mode; the reference concatenates its
// per-subtree files in shell-glob order, subtree-10 before subtree-2), and a subtree with fewer than two leaves is refused.
#include "align_gpu.hpp"

#include "../../../include/twl_merge.h"
#include "../../../include/twl_subtree.h"

#include <algorithm>
#include <cstdio>
#include <iostream>
#include <numeric>
#include <string>
#include <vector>

namespace msa {

using progressive::gpu::die;
using progressive::gpu::nowMs;

namespace {

struct Subtree {
    int index = 0;                           // its index in the partition (grpID)
    Node *rootInTree = nullptr;
    std::vector<std::string> names, rows;    // the rows that are written, in input order, alnLen columns each
    int32_t alnLen = 0, alnNum = 0;
    float alnWeight = 0;
    std::vector<float> profile;              // float[alnLen][P]
};

struct SubtreeTotals { double phaseA = 0, profiles = 0, phaseB = 0, finish = 0, read = 0, write = 0; uint64_t cellsA = 0, pairsA = 0, profileBytes = 0; progressive::gpu::MergeLevelTotals level; };

// storeSubtreeProfile's sum on the device: one row per entry of root->seqsIncluded, in that order
void weightedProfile(int device, const Option &option, SequenceDB &db, const Node *root, int subtree, Subtree &sub, SubtreeTotals &tot)
{
    std::vector<const char *> rowPtr;
    std::vector<int32_t> rowLen, ids;
    std::vector<float> weights;
    for (int sIdx : root->seqsIncluded) {
        const auto *s = db.sequences[(size_t)sIdx];
        if (s->lowQuality && !option.noFilter) continue;      // excluded: it has no row of this alignment
        rowPtr.push_back(s->alnStorage[s->storage]);
        rowLen.push_back(sub.alnLen);
        weights.push_back(s->weight);
    }
    ids.resize(rowPtr.size());
    std::iota(ids.begin(), ids.end(), 0);
    const double t0 = nowMs();
    twl_store *ts = nullptr;
    int rc = twl_store_create(device, option.type, (int32_t)rowPtr.size(), rowPtr.data(), rowLen.data(), &ts);
    if (rc != TWL_OK) die("twl_store_create", rc);
    const double t1 = nowMs();
    if ((rc = twl_store_weighted_columns(ts, (int32_t)ids.size(), ids.data(), weights.data(), 0)) != TWL_OK) die("twl_store_weighted_columns", rc);
    const double t2 = nowMs();
    int32_t len = 0;
    sub.profile.resize((size_t)sub.alnLen * (option.type == 'n' ? 6 : 22));
    if ((rc = twl_store_read_cache(ts, 0, sub.profile.data(), &len)) != TWL_OK) die("twl_store_read_cache", rc);
    twl_store_destroy(ts);
    tot.profiles += nowMs() - t0;
    tot.profileBytes += (uint64_t)ids.size() * (uint64_t)sub.alnLen;
    if (option.printDetail)
        fprintf(stderr, "Subtree %d profile: weighted columns over %zu rows x %d columns (%.3f ms, %llu row bytes read; upload %.3f ms)\n", subtree, ids.size(), sub.alnLen,
                t2 - t1, (unsigned long long)ids.size() * (unsigned long long)sub.alnLen, t1 - t0);
}

}  // namespace

int runSubtrees(Option &option)
{
    using progressive::gpu::ensureInit;
    using progressive::gpu::selectedDevices;
    SubtreeTotals tot;
    Params param(option, option.type);
    Tree *T = openTree(option);                                                        // twilight-main.cpp:122
    phylogeny::PartitionInfo P((size_t)option.maxSubtree, 0, 0);                       // :129-130
    P.partitionTree(T->root);
    if (P.partitionsRoot.size() == 1) { delete T; return -1; }                         // not split: the default run
    if (P.partitionsRoot.empty()) {
        std::cerr << "ERROR: -m " << option.maxSubtree << ": the tree cannot be cut into subtrees of at most " << option.maxSubtree
                  << " leaves: the best place to cut it is its root.\n";
        exit(1);
    }
    Tree *subRootT = phylogeny::constructTreeFromPartitions(T->root, &P);              // :131
    std::cerr << "Decomposed the tree into " << P.partitionsRoot.size() << " subtrees.\n";
    std::vector<Subtree> subs;
    for (auto &kv : P.partitionsRoot) { Subtree s; s.index = kv.second.first->grpID; s.rootInTree = kv.second.first; subs.push_back(std::move(s)); }
    std::sort(subs.begin(), subs.end(), [](const Subtree &a, const Subtree &b) { return a.index < b.index; });
    for (const Subtree &s : subs)
        if (P.partitionsRoot[s.rootInTree->identifier].second < 2) {
            std::cerr << "ERROR: -m " << option.maxSubtree << " leaves subtree " << s.index << " with " << P.partitionsRoot[s.rootInTree->identifier].second
                      << " leaf/leaves; a subtree needs two to be aligned.  Choose a larger -m.\n";
            exit(1);
        }
    const int32_t G = (int32_t)subs.size();
    const int P_ = option.type == 'n' ? 6 : 22;

    // ---- phase A: every subtree on its own ----
    ensureInit(&option);
    const int device = selectedDevices().empty() ? 0 : selectedDevices()[0];
    alnFunction kernel = progressive::gpu::alignmentKernel_Resident;
    double t = nowMs();
    for (int32_t g = 0; g < G; ++g) {
        Subtree &sub = subs[(size_t)g];
        std::cerr << "Start processing subalignment No. " << sub.index << ". (" << g + 1 << '/' << G << ")\n";
        SequenceDB db;                                                                  // (the reference's cleanSubtreeDB)
        db.updateSeqTh = option.updateSeqTh;
        Tree *subT = new Tree(sub.rootInTree, option.reroot);                          // :145
        io::readSequences(option.seqFile, &db, &option, subT);                         // :146
        bool anyKept = false;
        for (const auto *s : db.sequences) anyKept = anyKept || !(s->lowQuality && !option.noFilter);
        if (!anyKept) { std::cerr << "ERROR: every sequence of subtree " << sub.index << " was excluded (--filter); nothing of it can be aligned.\n"; exit(1); }
        progressive::msaOnSubtree(subT, &db, &option, param, kernel, kernel);          // :148
        if (option.debug && !db.debug()) std::cerr << "WARNING: --check found an illegal alignment row.\n";
        const progressive::gpu::LevelTotals lt = progressive::gpu::runTotals(&db);
        tot.cellsA += lt.band_cells;
        tot.pairsA += lt.pairs;
        Node *root = subT->root;
        Node *subroot = subRootT->allNodes[sub.rootInTree->identifier];
        phylogeny::updateSubrootInfo(subroot, subT, g);                                // :156 (the group of the merge plays the subtree index)
        sub.alnLen = subroot->alnLen;
        sub.alnNum = subroot->alnNum;
        sub.alnWeight = subroot->alnWeight;
        if (sub.alnLen < 1 || root->seqsIncluded.empty()) { std::cerr << "ERROR: subtree " << sub.index << " has no aligned sequence.\n"; exit(1); }
        if (!subroot->msaFreq.empty()) {                                               // storeSubtreeProfile's early return
            if ((int32_t)subroot->msaFreq.size() != sub.alnLen) { std::cerr << "ERROR: the cached profile of subtree " << sub.index << " does not have its alignment's length.\n"; exit(1); }
            sub.profile.resize((size_t)sub.alnLen * P_);
            for (int32_t j = 0; j < sub.alnLen; ++j) std::copy(subroot->msaFreq[j].begin(), subroot->msaFreq[j].begin() + P_, &sub.profile[(size_t)j * P_]);
            phylogeny::Profile().swap(subroot->msaFreq);
            if (option.printDetail) std::cerr << "Subtree " << sub.index << " profile: cached msaFreq (" << sub.alnLen << " columns)\n";
        } else
            weightedProfile(device, option, db, root, sub.index, sub, tot);
        for (const auto *s : db.sequences)                                             // io.cpp:512-525: what writeAlignment would write
            if (!s->lowQuality) { sub.names.push_back(s->name); sub.rows.emplace_back(s->alnStorage[s->storage], (size_t)sub.alnLen); }
        if (sub.rows.empty()) { std::cerr << "ERROR: subtree " << sub.index << " has no sequence to write.\n"; exit(1); }
        delete subT;
    }
    tot.phaseA = nowMs() - t - tot.profiles;
    std::cerr << "Finished all subalignments.\n";

    // ---- phase B: one store, group g = subtree g (ascending index), its profile the cached profile g ----
    t = nowMs();
    std::vector<const char *> rowPtr;
    std::vector<int32_t> rowLen, groupOff{0};
    for (const Subtree &s : subs) {
        for (const std::string &r : s.rows) { rowPtr.push_back(r.data()); rowLen.push_back(s.alnLen); }
        groupOff.push_back((int32_t)rowPtr.size());
    }
    const int32_t nRows = (int32_t)rowPtr.size();
    std::vector<int32_t> rowIds((size_t)nRows);
    std::iota(rowIds.begin(), rowIds.end(), 0);
    twl_store *st = nullptr;
    int rc = twl_store_create(device, option.type, nRows, rowPtr.data(), rowLen.data(), &st);
    if (rc != TWL_OK) die("twl_store_create", rc);
    for (Subtree &s : subs) for (std::string &r : s.rows) std::string().swap(r);
    for (int32_t g = 0; g < G; ++g) {
        if ((rc = twl_store_write_cache(st, g, subs[(size_t)g].profile.data(), subs[(size_t)g].alnLen)) != TWL_OK) die("twl_store_write_cache", rc);
        std::vector<float>().swap(subs[(size_t)g].profile);
    }
    twl_merge *mg = nullptr;
    if ((rc = twl_merge_create(st, G, groupOff.data(), rowIds.data(), &mg)) != TWL_OK) die("twl_merge_create", rc);

    std::vector<NodePairVec> levels;
    progressive::scheduling(subRootT->root, levels, 1);                                // :183 (currentTask 2)
    const twl_params tp = progressive::gpu::baseParams(param);
    std::vector<std::vector<int32_t>> under((size_t)G);                                // the subtrees merged into a node so far
    for (int32_t g = 0; g < G; ++g) under[(size_t)g] = {g};
    auto groupOf = [](const Node *n) { return (int32_t)n->seqsIncluded[0]; };
    for (size_t l = 0; l < levels.size(); ++l) {
        std::vector<progressive::gpu::ProfilePair> pairs;
        for (const NodePair &np : levels[l]) {
            const Node *a = np.first, *b = np.second;
            pairs.push_back({groupOf(a), groupOf(b), a->alnLen, b->alnLen, a->alnNum, b->alnNum, a->alnWeight, b->alnWeight, under[(size_t)groupOf(a)], under[(size_t)groupOf(b)],
                             "subtrees " + std::to_string(subs[(size_t)groupOf(a)].index) + " and " + std::to_string(subs[(size_t)groupOf(b)].index)});
        }
        const std::vector<int32_t> pathLen = progressive::gpu::mergeProfileLevel(st, mg, device, tp, param, option, pairs, tot.level);
        for (size_t i = 0; i < levels[l].size(); ++i) {                                 // alignment-helper.cpp:474-477
            Node *a = levels[l][i].first, *b = levels[l][i].second;
            a->alnNum += b->alnNum;
            a->alnLen = pathLen[i];
            a->alnWeight += b->alnWeight;
            auto &ua = under[(size_t)groupOf(a)];
            const auto &ub = under[(size_t)groupOf(b)];
            ua.insert(ua.end(), ub.begin(), ub.end());
        }
        if (option.printDetail)
            std::cerr << "Subtree merge level " << l + 1 << ": " << levels[l].size() << (levels[l].size() > 1 ? " pairs" : " pair") << " in one twl_merge_apply\n";
    }
    tot.phaseB = nowMs() - t;

    // ---- every row through its subtree's map, once; one read-back; output ----
    int32_t W = 0;
    t = nowMs();
    if ((rc = twl_merge_finish(mg, &W)) != TWL_OK) die("twl_merge_finish", rc);
    tot.finish = nowMs() - t;
    t = nowMs();
    std::vector<int32_t> outLen((size_t)nRows);
    std::vector<char> rows;
    if (option.trimRule >= 0) {            // the rows lose their gappy columns on the device first (trim.cpp): W is the kept length from here on
        std::vector<const std::string *> nameOf;
        for (const Subtree &s : subs) for (const std::string &nm : s.names) nameOf.push_back(&nm);
        W = trimAndReadRows(option, st, nRows, rowIds.data(), [&](int32_t k) { return writtenNameOf(option, *nameOf[(size_t)k]); }, rows);
    } else {
        rows.resize((size_t)nRows * (size_t)W + 1);
        if ((rc = twl_store_read_rows_of(st, nRows, rowIds.data(), rows.data(), outLen.data())) != TWL_OK) die("twl_store_read_rows_of", rc);
    }
    tot.read = nowMs() - t;
    twl_merge_destroy(mg);
    twl_store_destroy(st);
    t = nowMs();
    std::vector<const std::string *> names;
    std::vector<const char *> rowAt;
    for (const Subtree &s : subs)
        for (const std::string &n : s.names) { rowAt.push_back(rows.data() + names.size() * (size_t)W); names.push_back(&n); }
    std::cerr << "Final Alignment Length: " << W << '\n';
    io::writeRecords(option.outFile, names, rowAt, W, &option);
    tot.write = nowMs() - t;
    std::cerr << "Aligned " << G << " subtrees (" << nRows << " rows) and merged them: subtrees " << tot.pairsA << " pairs, " << tot.cellsA << " band cells; merge "
              << tot.level.run.cells << " band cells, " << tot.level.run.retries << " retried DP run(s)\n";
    if (option.printDetail)
        fprintf(stderr, "Subtree phases (ms): subtrees %.3f, profiles %.3f (%llu row bytes), merge %.3f (prepare+DP %.3f, restore %.3f, apply %.3f, commit %.3f), finish %.3f, "
                        "read-back %.3f, write %.3f; restored on the host %d\n", tot.phaseA, tot.profiles, (unsigned long long)tot.profileBytes, tot.phaseB, tot.level.dp, tot.level.restore,
                tot.level.apply, tot.level.commit, tot.finish, tot.read, tot.write, tot.level.restoredOnHost);
    delete subRootT;
    delete T;
    return W;
}

}  // namespace msa
