// twilight_amd/csrc/host/strand.cpp -- `--adjust-direction`: the records of -i that lie reverse-complemented are found and turned before
// anything else reads them.
//
//   records of -i (first record of a name; with -t the leaves of the tree only)      -> one twl_guide_set: 6-mer counts on the device
//   S seeds at the stride of guide::seedIds                                         -> F = S(seed, seed) (twl_guide_set_shared_groups), R = O(seed, seed) (twl_guide_set_opposite)
//   strand::seedFlips                                                               -> the seeds' directions, a spanning tree on the host (strand_orient.hpp)
//   twl_guide_set_strand_assign                                                     -> every record's closest (seed, strand): its direction
// With -a the set is the degapped backbone rows followed by the new sequences, the seeds are backbone rows, all forward, and only new
// sequences are turned.  The result is Option::reversedNames: io::readSequences / io::readRecords turn those records as they read them, the
// writers name them _R_<name>.  What is refused here is refused before a device is opened.
#include "align_gpu.hpp"
#include "guide_stage.hpp"
#include "strand_orient.hpp"

#include "../../../include/twl_strand.h"

#include <fstream>
#include <iostream>
#include <unordered_set>

namespace msa {

using progressive::gpu::die;
using progressive::gpu::nowMs;

void adjustDirections(Option &option)
{
    const bool place = !option.backboneAlnFile.empty();
    std::vector<std::string> names, seqs;
    // ---- with -a: the backbone's rows without their gaps come first ----
    std::unordered_set<std::string> bbNames;
    if (place) {
        std::vector<std::string> rows;
        io::readAlignedRows(option.backboneAlnFile, "a backbone alignment", names, rows);
        for (std::string &r : rows) {
            std::string s;
            for (char c : r)
                if (c != '-' && c != '.') s += c;
            seqs.push_back(std::move(s));
        }
        if (names.empty()) { std::cerr << "ERROR: no rows were read from the backbone alignment " << option.backboneAlnFile << ".\n"; exit(1); }
        bbNames.insert(names.begin(), names.end());
    }
    const size_t B = names.size();
    // ---- the records of -i that the run keeps ----
    {
        Tree *T = option.treeFile.empty() ? nullptr : new Tree(option.treeFile);
        std::unordered_set<std::string> seen;
        io::readRecords(option.seqFile, [&](std::string &name, std::string &seq) {
            if (T && T->allNodes.find(name) == T->allNodes.end()) return;      // (readSequences skips a record that is no leaf)
            if (!seen.insert(name).second) return;                             // (... and keeps the first record of a name)
            names.push_back(name);
            seqs.push_back(std::move(seq));
        });
        delete T;
    }
    const size_t N = names.size() - B, total = names.size();
    if (N < 1) { std::cerr << "ERROR: --adjust-direction found no sequence to orient in " << option.seqFile << ".\n"; exit(1); }
    if (total > (size_t)TWL_GUIDE_SET_MAX_SEQS) {
        std::cerr << "ERROR: --adjust-direction decides the directions of at most " << TWL_GUIDE_SET_MAX_SEQS << " sequences; " << option.seqFile << (place ? " and the backbone hold " : " holds ")
                  << total << ".\n";
        exit(1);
    }
    const size_t cap = place ? B : N;
    if (option.directionSeeds > 0 && (size_t)option.directionSeeds > cap) {
        std::cerr << "ERROR: --direction-seeds " << option.directionSeeds << " is more than the " << cap << (place ? " rows of the backbone " + option.backboneAlnFile : " sequences of " + option.seqFile) << ".\n";
        exit(1);
    }
    const int32_t S = option.directionSeeds > 0 ? option.directionSeeds : strand::defaultSeeds((int64_t)total, (int64_t)cap);
    std::vector<const char *> ptr(total);
    std::vector<int32_t> len(total);
    for (size_t i = 0; i < total; ++i) {
        if (seqs[i].size() > (size_t)INT32_MAX) { std::cerr << "ERROR: the sequence " << names[i] << " is too long.\n"; exit(1); }
        ptr[i] = seqs[i].data(); len[i] = (int32_t)seqs[i].size();
    }
    // ---- the device: counts, the seeds' two matrices, every record's direction ----
    progressive::gpu::ensureInit(&option);
    const int device = progressive::gpu::selectedDevices().empty() ? 0 : progressive::gpu::selectedDevices()[0];
    twl_guide_set *set = nullptr;
    int rc = twl_guide_set_create(device, 'n', (int32_t)total, ptr.data(), len.data(), &set);
    if (rc != TWL_OK) die("twl_guide_set_create", rc);
    std::vector<std::string>().swap(seqs);
    const std::vector<int32_t> seeds = guide::seedIds((int64_t)cap, S);
    std::vector<uint8_t> flip((size_t)S, 0);
    double primMs = 0;
    if (!place) {
        std::vector<uint32_t> F((size_t)S * (size_t)S), R((size_t)S * (size_t)S);
        const int32_t off[2] = {0, S};
        if ((rc = twl_guide_set_shared_groups(set, 1, off, seeds.data(), F.data())) != TWL_OK) die("twl_guide_set_shared_groups", rc);
        if ((rc = twl_guide_set_opposite(set, S, seeds.data(), R.data())) != TWL_OK) die("twl_guide_set_opposite", rc);
        const double t0 = nowMs();
        flip = strand::seedFlips(S, F.data(), R.data());
        primMs = nowMs() - t0;
    }
    std::vector<int32_t> seedOf(total);
    std::vector<uint8_t> dir(total);
    if ((rc = twl_guide_set_strand_assign(set, S, seeds.data(), flip.data(), seedOf.data(), dir.data(), nullptr)) != TWL_OK) die("twl_guide_set_strand_assign", rc);
    double countMs = 0, a = 0, g = 0, dl = 0, permuteMs = 0, assignMs = 0, oppositeMs = 0, downloadMs = 0;
    if ((rc = twl_guide_set_timing(set, &countMs, &a, &g, &dl)) != TWL_OK) die("twl_guide_set_timing", rc);
    if ((rc = twl_guide_set_strand_timing(set, &permuteMs, &assignMs, &oppositeMs, &downloadMs)) != TWL_OK) die("twl_guide_set_strand_timing", rc);
    twl_guide_set_destroy(set);
    // ---- the result ----
    size_t turned = 0;
    for (size_t i = B; i < total; ++i) {
        if (!dir[i]) continue;
        if (bbNames.count(names[i])) {
            std::cerr << "ERROR: the new sequence \"" << names[i] << "\" lies reversed and carries the name of a backbone row: the output could not tell them apart; rename it.\n";
            exit(1);
        }
        option.reversedNames.insert(names[i]);
        ++turned;
    }
    if (!option.writeDirectionsFile.empty()) {
        std::ofstream out(option.writeDirectionsFile, std::ios::binary);
        for (size_t i = B; i < total; ++i) out << names[i] << '\t' << (dir[i] ? '-' : '+') << '\n';
        if (!out.flush()) { std::cerr << "ERROR: cannot write the directions to " << option.writeDirectionsFile << ".\n"; exit(1); }
    }
    std::cerr << "Directions: " << turned << " of " << N << " sequences lie reversed and are reverse-complemented (" << S << " seeds" << (place ? ", rows of the backbone" : "") << ")\n";
    if (option.printDetail)
        std::cerr << "Directions of " << N << " sequences (ms): upload + count " << countMs << ", seeds' shared counts " << g << ", permute " << permuteMs << ", opposite " << oppositeMs
                  << ", assign " << assignMs << ", download " << dl + downloadMs << ", spanning tree " << primMs << '\n';
}

}  // namespace msa
