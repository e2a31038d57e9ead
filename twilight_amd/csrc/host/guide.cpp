// twilight_amd/csrc/host/guide.cpp -- the guide tree of a run that brings none (`twilight-mi355x -i seqs.fa -o out.aln` without -t).
//
//   records of -i (first record of a name, as readSequences keeps them)
//   twl_guide_shared      -> the shared k-mer counts of all pairs, on the device (include/twl_guide.h)
//   distances, UPGMA, text -> guide_upgma.hpp, on the host, in double
// The text is then what -t would have read: the caller parses it with the parser of -t, so `-t` on the written tree repeats the run.
// What is refused here is refused before a device is opened.
#include "align_gpu.hpp"
#include "guide_upgma.hpp"

#include "../../../include/twl_guide.h"

#include <cstring>
#include <fstream>
#include <iostream>
#include <unordered_set>

namespace msa {

using progressive::gpu::die;
using progressive::gpu::nowMs;

static void refuseName(const std::string &name)
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

std::string buildGuideTree(Option &option)
{
    std::vector<std::string> names, seqs;
    std::unordered_set<std::string> seen;
    io::readRecords(option.seqFile, [&](std::string &name, std::string &seq) {
        if (!seen.insert(name).second) return;      // (readSequences keeps the first record of a name and warns)
        refuseName(name);
        names.push_back(name);
        seqs.push_back(std::move(seq));
    });
    const size_t N = names.size();
    if (N < 2) { std::cerr << "ERROR: a guide tree needs at least 2 sequences; " << option.seqFile << " holds " << N << ".\n"; exit(1); }
    if (N > (size_t)TWL_GUIDE_MAX_SEQS) {
        std::cerr << "ERROR: " << option.seqFile << " holds " << N << " sequences; a guide tree is built for at most " << TWL_GUIDE_MAX_SEQS << ": bring a tree with -t.\n";
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
    if (!option.writeTreeFile.empty()) {
        std::ofstream out(option.writeTreeFile, std::ios::binary);
        out << text;
        if (!out.flush()) { std::cerr << "ERROR: cannot write the tree to " << option.writeTreeFile << ".\n"; exit(1); }
    }
    if (option.printDetail)
        std::cerr << "Guide tree of " << N << " sequences (ms): upload + count " << countMs << ", all pairs " << pairsMs << ", download " << downloadMs
                  << ", UPGMA " << t1 - t0 << ", text " << t2 - t1 << '\n';
    return text;
}

}  // namespace msa
