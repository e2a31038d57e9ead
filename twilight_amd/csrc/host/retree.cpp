// twilight_amd/csrc/host/retree.cpp -- `--iterations K`: the default alignment run K times, runs 2 .. K on a guide tree computed from the
// alignment of the run before.
//
//   run k                  runDefaultAlignment on the tree of the moment (the user's or the k-mer tree for k = 1); only run K writes the MSA
//   its rows, at the end   twl_retree_pair_counts -> match and both of all pairs over the columns the mask keeps, on the device (include/twl_retree.h)
//   distances, UPGMA, text -> guide_upgma.hpp, on the host, in double: the tree of run k + 1, parsed from its text by the parser of -t
// With --retree-seeds S the tree is rebuilt in two stages instead (rebuildStagedTree; twl_retree_set_*, guide_stage.hpp), for
// alignments of up to 2^20 rows: the device keeps the rows' bit-planes, and no matrix is larger than one cluster's.
// Every run reads the FASTA again, as the passes of -m do; nothing stays in HBM between runs.  What is refused because of the input is refused
// before a device is opened.
#include "align_gpu.hpp"
#include "guide_stage.hpp"

#include "../../../include/twl_retree.h"
#include "../../../include/twl_retree_set.h"
#include "../twl_retree_plan.inc.hip"

#include <algorithm>
#include <fstream>
#include <iostream>
#include <unordered_set>

namespace msa {

using progressive::gpu::die;
using progressive::gpu::nowMs;

namespace {

// the finished rows of run k in input order: names are the sequences in input order (the slots of the definition)
std::vector<const char *> finishedRows(SequenceDB *db, const std::vector<std::string> &names, int iteration)
{
    const size_t N = names.size();
    std::vector<const char *> rows(N, nullptr);
    for (size_t i = 0; i < N; ++i) {
        const auto it = db->name_map.find(names[i]);
        if (it == db->name_map.end() || it->second->lowQuality) {
            std::cerr << "ERROR: the alignment of iteration " << iteration << " has no row for the sequence " << names[i]
                      << " (is it a leaf of the tree?); the tree of the next iteration needs every sequence.\n";
            exit(1);
        }
        rows[i] = it->second->alnStorage[it->second->storage];
    }
    if (db->finalAlnLen < 1) { std::cerr << "ERROR: the alignment of iteration " << iteration << " has no columns.\n"; exit(1); }
    return rows;
}

// the tree of run k + 1 from the finished rows of run k
std::string rebuildTree(const Option &option, SequenceDB *db, const std::vector<std::string> &names, int iteration, int device)
{
    const size_t N = names.size();
    const int32_t W = db->finalAlnLen;
    const std::vector<const char *> rows = finishedRows(db, names, iteration);
    const int32_t maxGaps = retree_max_gaps(option.maskGappy, (int32_t)N);
    std::vector<uint32_t> match(N * N), both(N * N);
    int32_t kept = 0;
    int rc = twl_retree_pair_counts(device, option.type, (int32_t)N, W, rows.data(), maxGaps, match.data(), both.data(), &kept);
    if (rc != TWL_OK) die("twl_retree_pair_counts", rc);
    double uploadMs = 0, gapsMs = 0, packMs = 0, pairsMs = 0, downloadMs = 0;
    if ((rc = twl_retree_timing(device, &uploadMs, &gapsMs, &packMs, &pairsMs, &downloadMs)) != TWL_OK) die("twl_retree_timing", rc);
    const double t0 = nowMs();
    guide::Triangle d = guide::distancesFromCounts((int)N, match.data(), both.data());
    std::vector<uint32_t>().swap(match);
    std::vector<uint32_t>().swap(both);
    const std::vector<guide::Merge> merges = guide::upgma(d);
    const double t1 = nowMs();
    std::string text = guide::newick(names, merges);
    const double t2 = nowMs();
    if (option.printDetail)
        std::cerr << "Guide tree rebuilt from the alignment of iteration " << iteration << ": kept " << kept << " of " << W << " columns, " << N << " sequences (ms): upload "
                  << uploadMs << ", gaps " << gapsMs << ", pack " << packMs << ", pairs " << pairsMs << ", download " << downloadMs << ", UPGMA " << t1 - t0 << ", text " << t2 - t1 << '\n';
    return text;
}

// --retree-seeds S: the same mask and letters, but every row goes to the closest of S seed rows, each cluster and the
// seeds get a tree of section 4h, and the clusters' trees replace the leaves of the seeds' tree.
std::string rebuildStagedTree(const Option &option, SequenceDB *db, const std::vector<std::string> &names, int iteration, int device)
{
    const size_t N = names.size();
    const int32_t W = db->finalAlnLen, S = option.retreeSeeds;
    const std::vector<const char *> rows = finishedRows(db, names, iteration);
    twl_retree_set *set = nullptr;
    int32_t kept = 0;
    int rc = twl_retree_set_create(device, option.type, (int32_t)N, W, rows.data(), retree_max_gaps(option.maskGappy, (int32_t)N), &set, &kept);
    if (rc != TWL_OK) die("twl_retree_set_create", rc);
    const std::vector<int32_t> seeds = guide::seedIds((int64_t)N, S);
    std::vector<int32_t> seedOf(N);
    if ((rc = twl_retree_set_assign(set, S, seeds.data(), seedOf.data(), nullptr, nullptr)) != TWL_OK) die("twl_retree_set_assign", rc);
    const double t0 = nowMs();
    const std::vector<std::vector<int32_t>> clusters = guide::clustersOf(S, seedOf);
    std::vector<size_t> sizes;
    for (const auto &k : clusters) sizes.push_back(k.size());
    std::sort(sizes.begin(), sizes.end());
    if (sizes.back() > (size_t)TWL_RETREE_MAX_SEQS) {
        std::cerr << "ERROR: with --retree-seeds " << S << " one cluster of the alignment of iteration " << iteration << " holds " << sizes.back()
                  << " sequences; a cluster's tree is built for at most " << TWL_RETREE_MAX_SEQS << ": raise --retree-seeds.\n";
        exit(1);
    }
    double hostMs = nowMs() - t0;
    // the clusters' trees, in calls whose matrices stay under 2^28 entries each; a cluster of one member needs no matrix
    std::vector<guide::Subtree> sub((size_t)S);
    std::vector<uint32_t> match, both;
    for (int32_t first = 0; first < S;) {
        std::vector<int32_t> which, off{0}, ids;
        uint64_t words = 0;
        int32_t t = first;
        for (; t < S; ++t) {
            const std::vector<int32_t> &k = clusters[(size_t)t];
            if (k.size() < 2) continue;
            const uint64_t w = (uint64_t)k.size() * k.size();
            if (words + w > (1ull << 28) && !which.empty()) break;
            words += w;
            which.push_back(t);
            ids.insert(ids.end(), k.begin(), k.end());
            off.push_back((int32_t)ids.size());
        }
        first = t;
        if (which.empty()) continue;
        match.resize((size_t)words);
        both.resize((size_t)words);
        if ((rc = twl_retree_set_pair_groups(set, (int32_t)which.size(), off.data(), ids.data(), match.data(), both.data())) != TWL_OK) die("twl_retree_set_pair_groups", rc);
        const double t1 = nowMs();
        std::vector<size_t> block(which.size(), 0);
        for (size_t g = 1; g < which.size(); ++g) block[g] = block[g - 1] + (size_t)(off[g] - off[g - 1]) * (size_t)(off[g] - off[g - 1]);
#pragma omp parallel for schedule(dynamic, 1) if (which.size() > 1)      // (a lone cluster keeps the threads for its own loops)
        for (size_t g = 0; g < which.size(); ++g) {
            const std::vector<int32_t> &k = clusters[(size_t)which[g]];
            std::vector<std::string> member;
            for (int32_t i : k) member.push_back(names[(size_t)i]);
            guide::Triangle d = guide::distancesFromCounts((int)k.size(), match.data() + block[g], both.data() + block[g]);
            sub[(size_t)which[g]] = guide::subtreeOf(member, guide::upgma(d));
        }
        hostMs += nowMs() - t1;
    }
    for (int32_t t = 0; t < S; ++t)
        if (clusters[(size_t)t].size() == 1) sub[(size_t)t].text = names[(size_t)clusters[(size_t)t][0]];
    // the seeds' tree: one group
    const int32_t seedOff[2] = {0, S};
    match.resize((size_t)S * (size_t)S);
    both.resize((size_t)S * (size_t)S);
    if ((rc = twl_retree_set_pair_groups(set, 1, seedOff, seeds.data(), match.data(), both.data())) != TWL_OK) die("twl_retree_set_pair_groups", rc);
    double uploadMs = 0, gapsMs = 0, packMs = 0, assignMs = 0, groupsMs = 0, downloadMs = 0;
    if ((rc = twl_retree_set_timing(set, &uploadMs, &gapsMs, &packMs, &assignMs, &groupsMs, &downloadMs)) != TWL_OK) die("twl_retree_set_timing", rc);
    twl_retree_set_destroy(set);
    const double t2 = nowMs();
    guide::Triangle d = guide::distancesFromCounts(S, match.data(), both.data());
    std::vector<uint32_t>().swap(match);
    std::vector<uint32_t>().swap(both);
    const std::vector<guide::Merge> merges = guide::upgma(d);
    const double t3 = nowMs();
    std::string text = guide::graftedNewick(sub, merges);
    const double t4 = nowMs();
    if (option.printDetail)
        std::cerr << "Guide tree rebuilt in two stages from the alignment of iteration " << iteration << ": kept " << kept << " of " << W << " columns, " << N << " sequences, " << S
                  << " seeds (ms): upload " << uploadMs << ", gaps " << gapsMs << ", pack " << packMs << ", assign " << assignMs << ", groups " << groupsMs << ", download " << downloadMs
                  << ", UPGMA " << hostMs + (t3 - t2) << ", text " << t4 - t3 << "; clusters: smallest " << sizes.front() << ", median " << sizes[sizes.size() / 2] << ", largest "
                  << sizes.back() << '\n';
    return text;
}

}  // namespace

int runIterations(Option &option)
{
    // one pass over the records: the slots of the definition, and what the input itself rules out
    std::vector<std::string> names;
    {
        std::unordered_set<std::string> seen;
        io::readRecords(option.seqFile, [&](std::string &name, std::string &) {
            if (!seen.insert(name).second) return;      // (readSequences keeps the first record of a name)
            refuseName(name);
            names.push_back(name);
        });
    }
    const size_t N = names.size();
    if (N < 2) { std::cerr << "ERROR: --iterations rebuilds a guide tree, which needs at least 2 sequences; " << option.seqFile << " holds " << N << ".\n"; exit(1); }
    if (option.retreeSeeds == 0 && N > (size_t)TWL_RETREE_MAX_SEQS) {
        std::cerr << "ERROR: " << option.seqFile << " holds " << N << " sequences; --iterations rebuilds the guide tree from an alignment of at most " << TWL_RETREE_MAX_SEQS
                  << " (with or without --tree-seeds).\n"
                  << "       (or rebuild it in two stages: --retree-seeds S, with S near twice the square root of the number of sequences)\n";
        exit(1);
    }
    if (option.retreeSeeds > 0 && N > (size_t)TWL_RETREE_SET_MAX_SEQS) {
        std::cerr << "ERROR: " << option.seqFile << " holds " << N << " sequences; --iterations with --retree-seeds rebuilds the guide tree from an alignment of at most "
                  << TWL_RETREE_SET_MAX_SEQS << ".\n";
        exit(1);
    }
    if (option.retreeSeeds > 0 && (size_t)option.retreeSeeds > N) {
        std::cerr << "ERROR: --retree-seeds " << option.retreeSeeds << " is more than the " << N << " sequences of " << option.seqFile << ".\n";
        exit(1);
    }
    const std::string treeFile = option.writeTreeFile;
    if (option.buildTree) {
        option.writeTreeFile.clear();      // (the tree that is written is the last one, below)
        option.treeText = buildGuideTree(option);
    } else if (!option.adjustDirection)      // (--adjust-direction has brought the device up already)
        progressive::gpu::beginInit(&option);
    alnFunction kernel = progressive::gpu::alignmentKernel_Resident;
    int alnLen = 0;
    for (int k = 1; k <= option.iterations; ++k) {
        const bool last = k == option.iterations;
        std::cerr << "===== Iteration " << k << " of " << option.iterations << " =====\n";
        option.scoreRun = k;
        if (last && !treeFile.empty()) {
            std::ofstream out(treeFile, std::ios::binary);
            out << option.treeText;
            if (!out.flush()) { std::cerr << "ERROR: cannot write the tree to " << treeFile << ".\n"; exit(1); }
        }
        std::string next;
        alnLen = runDefaultAlignment(option, kernel, kernel, last, [&](SequenceDB *db) {
            if (last) return;
            if (option.scoreWritten) option.scoreWritten(names, finishedRows(db, names, k), db->finalAlnLen);      // --score: a line per run (the last run's comes from its writer)
            progressive::gpu::ensureInit(&option);
            const int device = progressive::gpu::selectedDevices().empty() ? 0 : progressive::gpu::selectedDevices()[0];
            next = option.retreeSeeds > 0 ? rebuildStagedTree(option, db, names, k, device) : rebuildTree(option, db, names, k, device);
        });
        if (!last) option.treeText = std::move(next);
    }
    return alnLen;
}

}  // namespace msa
