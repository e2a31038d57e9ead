// twilight_amd/csrc/host/guide.cpp -- the guide tree of a run that brings none (`twilight-mi355x -i seqs.fa -o out.aln` without -t).
//
//   records of -i (first record of a name, as readSequences keeps them)
//   twl_guide_shared      -> the shared k-mer counts of all pairs, on the device (include/twl_guide.h)
//   distances, UPGMA, text -> guide_upgma.hpp, on the host, in double
// With --tree-seeds S the tree is built in two stages instead (buildStagedTree; twl_guide_set_*, guide_stage.hpp), for inputs of any size up to 2^20.
// The text is then what -t would have read: the caller parses it with the parser of -t, so `-t` on the written tree repeats the run.
// What is refused here is refused before a device is opened.
#include "align_gpu.hpp"
#include "guide_stage.hpp"

#include "../../../include/twl_guide.h"

#include <algorithm>
#include <cstring>
#include <fstream>
#include <iostream>
#include <unordered_set>

namespace msa {

using progressive::gpu::die;
using progressive::gpu::nowMs;

void refuseName(const std::string &name)
{
    if (name.empty()) { std::cerr << "ERROR: a sequence without a name cannot be a leaf of the guide tree; name every record, or bring a tree with -t.\n"; exit(1); }
    for (char c : name)
        if (isspace((unsigned char)c) || strchr("(),:;'", c)) {
            std::cerr << "ERROR: the sequence name \"" << name << "\" contains whitespace or one of ( ) , : ; ' and cannot be written into a Newick tree; rename it, or bring a tree with -t.\n";
            exit(1);
        }
    if (name.compare(0, 4, "node") == 0) {
        std::cerr << "ERROR: the sequence name \"" << name << "\" begins with \"node\", which the tree keeps for its internal nodes; rename it.\n";
        exit(1);
    }
}

static void writeTree(const Option &option, const std::string &text)
{
    if (option.writeTreeFile.empty()) return;
    std::ofstream out(option.writeTreeFile, std::ios::binary);
    out << text;
    if (!out.flush()) { std::cerr << "ERROR: cannot write the tree to " << option.writeTreeFile << ".\n"; exit(1); }
}

// --tree-seeds S: every sequence goes to the closest of S seeds, each cluster and the seeds get a tree of section 4f,
// and the clusters' trees replace the leaves of the seeds' tree.  The device holds the count panels (twl_guide_set); no matrix is larger
// than one cluster's.
static std::string buildStagedTree(Option &option, const std::vector<std::string> &names, std::vector<std::string> &seqs, const std::vector<const char *> &ptr,
                                   const std::vector<int32_t> &len, int device)
{
    const size_t N = names.size();
    const int32_t S = option.treeSeeds;
    twl_guide_set *set = nullptr;
    int rc = twl_guide_set_create(device, option.type, (int32_t)N, ptr.data(), len.data(), &set);
    if (rc != TWL_OK) die("twl_guide_set_create", rc);
    std::vector<std::string>().swap(seqs);
    const std::vector<int32_t> seeds = guide::seedIds((int64_t)N, S);
    std::vector<int32_t> seedOf(N);
    if ((rc = twl_guide_set_assign(set, S, seeds.data(), seedOf.data(), nullptr)) != TWL_OK) die("twl_guide_set_assign", rc);
    const double t0 = nowMs();
    const std::vector<std::vector<int32_t>> clusters = guide::clustersOf(S, seedOf);
    std::vector<size_t> sizes;
    for (const auto &k : clusters) sizes.push_back(k.size());
    std::sort(sizes.begin(), sizes.end());
    if (sizes.back() > (size_t)TWL_GUIDE_MAX_SEQS) {
        std::cerr << "ERROR: with --tree-seeds " << S << " one cluster holds " << sizes.back() << " sequences; a cluster's tree is built for at most " << TWL_GUIDE_MAX_SEQS
                  << ": raise --tree-seeds.\n";
        exit(1);
    }
    double hostMs = nowMs() - t0;
    // the clusters' trees, in calls whose matrices stay under 2^28 entries together; a cluster of one member needs no matrix
    std::vector<guide::Subtree> sub((size_t)S);
    std::vector<uint32_t> shared;
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
        shared.resize((size_t)words);
        if ((rc = twl_guide_set_shared_groups(set, (int32_t)which.size(), off.data(), ids.data(), shared.data())) != TWL_OK) die("twl_guide_set_shared_groups", rc);
        const double t1 = nowMs();
        std::vector<size_t> block(which.size(), 0);
        for (size_t g = 1; g < which.size(); ++g) block[g] = block[g - 1] + (size_t)(off[g] - off[g - 1]) * (size_t)(off[g] - off[g - 1]);
#pragma omp parallel for schedule(dynamic, 1) if (which.size() > 1)      // (a lone cluster keeps the threads for its own loops)
        for (size_t g = 0; g < which.size(); ++g) {
            const std::vector<int32_t> &k = clusters[(size_t)which[g]];
            std::vector<std::string> member;
            for (int32_t i : k) member.push_back(names[(size_t)i]);
            guide::Triangle d = guide::distances((int)k.size(), shared.data() + block[g]);
            sub[(size_t)which[g]] = guide::subtreeOf(member, guide::upgma(d));
        }
        hostMs += nowMs() - t1;
    }
    for (int32_t t = 0; t < S; ++t)
        if (clusters[(size_t)t].size() == 1) sub[(size_t)t].text = names[(size_t)clusters[(size_t)t][0]];
    // the seeds' tree: one group
    const int32_t seedOff[2] = {0, S};
    shared.resize((size_t)S * (size_t)S);
    if ((rc = twl_guide_set_shared_groups(set, 1, seedOff, seeds.data(), shared.data())) != TWL_OK) die("twl_guide_set_shared_groups", rc);
    double countMs = 0, assignMs = 0, groupsMs = 0, downloadMs = 0;
    if ((rc = twl_guide_set_timing(set, &countMs, &assignMs, &groupsMs, &downloadMs)) != TWL_OK) die("twl_guide_set_timing", rc);
    twl_guide_set_destroy(set);
    const double t2 = nowMs();
    guide::Triangle d = guide::distances(S, shared.data());
    std::vector<uint32_t>().swap(shared);
    const std::vector<guide::Merge> merges = guide::upgma(d);
    const double t3 = nowMs();
    std::string text = guide::graftedNewick(sub, merges);
    const double t4 = nowMs();
    writeTree(option, text);
    if (option.printDetail)
        std::cerr << "Guide tree of " << N << " sequences in two stages, " << S << " seeds (ms): upload + count " << countMs << ", assign " << assignMs << ", groups " << groupsMs
                  << ", download " << downloadMs << ", UPGMA " << hostMs + (t3 - t2) << ", text " << t4 - t3 << "; clusters: smallest " << sizes.front() << ", median "
                  << sizes[sizes.size() / 2] << ", largest " << sizes.back() << '\n';
    return text;
}

std::string buildGuideTree(Option &option)
{
    std::vector<std::string> names, seqs;
    std::unordered_set<std::string> seen;
    io::readRecords(option.seqFile, [&](std::string &name, std::string &seq) {
        if (!seen.insert(name).second) return;      // (readSequences keeps the first record of a name and warns)
        refuseName(name);
        names.push_back(name);
        seqs.push_back(std::move(seq));
    }, &option);      // (oriented where --adjust-direction turned a record: the tree is built from what is aligned)
    const size_t N = names.size();
    if (N < 2) { std::cerr << "ERROR: a guide tree needs at least 2 sequences; " << option.seqFile << " holds " << N << ".\n"; exit(1); }
    if (option.treeSeeds > 0 && (size_t)option.treeSeeds > N) {
        std::cerr << "ERROR: --tree-seeds " << option.treeSeeds << " is more than the " << N << " sequences of " << option.seqFile << ".\n";
        exit(1);
    }
    if (option.treeSeeds > 0 && N > (size_t)TWL_GUIDE_SET_MAX_SEQS) {
        std::cerr << "ERROR: " << option.seqFile << " holds " << N << " sequences; a two-stage guide tree is built for at most " << TWL_GUIDE_SET_MAX_SEQS << ": bring a tree with -t.\n";
        exit(1);
    }
    if (option.treeSeeds == 0 && N > (size_t)TWL_GUIDE_MAX_SEQS) {
        std::cerr << "ERROR: " << option.seqFile << " holds " << N << " sequences; a guide tree is built for at most " << TWL_GUIDE_MAX_SEQS << ": bring a tree with -t.\n"
                  << "       (or build it in two stages: --tree-seeds S, with S near twice the square root of the number of sequences)\n";
        exit(1);
    }
    std::vector<const char *> ptr(N);
    std::vector<int32_t> len(N);
    for (size_t i = 0; i < N; ++i) {
        if (seqs[i].size() > (size_t)INT32_MAX) { std::cerr << "ERROR: the sequence " << names[i] << " is too long.\n"; exit(1); }
        ptr[i] = seqs[i].data(); len[i] = (int32_t)seqs[i].size();
    }
    progressive::gpu::ensureInit(&option);
    const int device = progressive::gpu::selectedDevices().empty() ? 0 : progressive::gpu::selectedDevices()[0];
    if (option.treeSeeds > 0) return buildStagedTree(option, names, seqs, ptr, len, device);
    std::vector<uint32_t> shared(N * N);
    int rc = twl_guide_shared(device, option.type, (int32_t)N, ptr.data(), len.data(), shared.data());
    if (rc != TWL_OK) die("twl_guide_shared", rc);
    double countMs = 0, pairsMs = 0, downloadMs = 0;
    if ((rc = twl_guide_timing(device, &countMs, &pairsMs, &downloadMs)) != TWL_OK) die("twl_guide_timing", rc);
    std::vector<std::string>().swap(seqs);
    const double t0 = nowMs();
    guide::Triangle d = guide::distances((int)N, shared.data());
    std::vector<uint32_t>().swap(shared);
    const std::vector<guide::Merge> merges = guide::upgma(d);
    const double t1 = nowMs();
    std::string text = guide::newick(names, merges);
    const double t2 = nowMs();
    writeTree(option, text);
    if (option.printDetail)
        std::cerr << "Guide tree of " << N << " sequences (ms): upload + count " << countMs << ", all pairs " << pairsMs << ", download " << downloadMs
                  << ", UPGMA " << t1 - t0 << ", text " << t2 - t1 << '\n';
    return text;
}

}  // namespace msa
