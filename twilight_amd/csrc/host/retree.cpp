// twilight_amd/csrc/host/retree.cpp -- `--iterations K`: the default alignment run K times, runs 2 .. K on a guide tree computed from the
// alignment of the run before.
//
//   run k                  runDefaultAlignment on the tree of the moment (the user's or the k-mer tree for k = 1); only run K writes the MSA
//   its rows, at the end   twl_retree_pair_counts -> match and both of all pairs over the columns the mask keeps, on the device (include/twl_retree.h)
//   distances, UPGMA, text -> guide_upgma.hpp, on the host, in double: the tree of run k + 1, parsed from its text by the parser of -t
// Every run reads the FASTA again, as the passes of -m do; nothing stays in HBM between runs.  What is refused because of the input is refused
// before a device is opened.
#include "align_gpu.hpp"
#include "guide_upgma.hpp"

#include "../../../include/twl_retree.h"
#include "../twl_retree_plan.inc.hip"

#include <fstream>
#include <iostream>
#include <unordered_set>

namespace msa {

using progressive::gpu::die;
using progressive::gpu::nowMs;

namespace {

// the tree of run k + 1 from the finished rows of run k; names: the sequences in input order (the slots of the definition)
std::string rebuildTree(const Option &option, SequenceDB *db, const std::vector<std::string> &names, int iteration, int device)
{
    const size_t N = names.size();
    const int32_t W = db->finalAlnLen;
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
    if (W < 1) { std::cerr << "ERROR: the alignment of iteration " << iteration << " has no columns.\n"; exit(1); }
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
    if (N > (size_t)TWL_RETREE_MAX_SEQS) {
        std::cerr << "ERROR: " << option.seqFile << " holds " << N << " sequences; --iterations rebuilds the guide tree from an alignment of at most " << TWL_RETREE_MAX_SEQS
                  << " (with or without --tree-seeds).\n";
        exit(1);
    }
    const std::string treeFile = option.writeTreeFile;
    if (option.buildTree) {
        option.writeTreeFile.clear();      // (the tree that is written is the last one, below)
        option.treeText = buildGuideTree(option);
    } else
        progressive::gpu::beginInit(&option);
    alnFunction kernel = progressive::gpu::alignmentKernel_Resident;
    int alnLen = 0;
    for (int k = 1; k <= option.iterations; ++k) {
        const bool last = k == option.iterations;
        std::cerr << "===== Iteration " << k << " of " << option.iterations << " =====\n";
        if (last && !treeFile.empty()) {
            std::ofstream out(treeFile, std::ios::binary);
            out << option.treeText;
            if (!out.flush()) { std::cerr << "ERROR: cannot write the tree to " << treeFile << ".\n"; exit(1); }
        }
        std::string next;
        alnLen = runDefaultAlignment(option, kernel, kernel, last, [&](SequenceDB *db) {
            if (last) return;
            progressive::gpu::ensureInit(&option);
            const int device = progressive::gpu::selectedDevices().empty() ? 0 : progressive::gpu::selectedDevices()[0];
            next = rebuildTree(option, db, names, k, device);
        });
        if (!last) option.treeText = std::move(next);
    }
    return alnLen;
}

}  // namespace msa
