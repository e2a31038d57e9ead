// twilight_amd/csrc/host/driver.cpp -- DEFAULT_ALN flow of /root/reference/src/twilight-main.cpp:115-176 for the
// single-partition case (no -m), plus the handful of CLI flags the hot path needs (names as in twilight-main.cpp:13-84).
#include "twl_host.hpp"

#include <unistd.h>
#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <thread>

#include <omp.h>

namespace msa {

// CPUs this process may really use: the cgroup quota (cpu.max) can be far below what the OS reports
static int effectiveCpus()
{
    int n = (int)std::thread::hardware_concurrency();
    if (n < 1) n = 1;
    std::ifstream f("/sys/fs/cgroup/cpu.max");
    std::string quota;
    long period = 0;
    if (f >> quota >> period && quota != "max" && period > 0) {
        long q = atol(quota.c_str());
        if (q > 0) n = std::min<long>(n, std::max<long>(1, (q + period - 1) / period));
    }
    return n;
}

static bool flag(const char *a, const char *s, const char *l) { return (s && !strcmp(a, s)) || (l && !strcmp(a, l)); }

bool parseCommandLine(int argc, char **argv, Option &o, bool allowPlacement, bool allowMerge, bool allowSubtrees, bool allowGuide, bool allowTrim)
{
    const bool allowCompare = o.allowCompare;
    bool typeGiven = false, subtreesGiven = false, maskGiven = false, trimGappyGiven = false, trimToGiven = false, iterationsGiven = false;
    o.cpuNum = 0;
    for (int i = 1; i < argc; ++i) {
        const char *a = argv[i];
        auto val = [&]() -> const char * { if (i + 1 >= argc) { std::cerr << "ERROR: missing value for " << a << '\n'; exit(1); } return argv[++i]; };
        if (flag(a, "-t", "--tree")) o.treeFile = val();
        else if (flag(a, "-i", "--sequences")) o.seqFile = val();
        else if (flag(a, "-o", "--output")) o.outFile = val();
        else if (flag(a, "-r", "--remove-gappy")) o.gappyVertical = (float)atof(val());
        else if (flag(a, "-C", "--cpu")) o.cpuNum = atoi(val());
        else if (flag(a, "-G", "--gpu")) o.gpuNum = atoi(val());
        else if (flag(a, nullptr, "--gpu-index")) { o.gpuIdx.clear(); for (char *tok = strtok(const_cast<char *>(val()), ","); tok; tok = strtok(nullptr, ",")) o.gpuIdx.push_back(atoi(tok)); }
        else if (flag(a, nullptr, "--cpu-only")) o.cpuOnly = true;
        else if (flag(a, nullptr, "--type")) { o.type = val()[0]; typeGiven = true; }
        else if (flag(a, "-w", "--wildcard")) o.wildcard = true;
        else if (flag(a, nullptr, "--rooted")) o.reroot = false;
        else if (flag(a, nullptr, "--match")) o.match = (float)atof(val());
        else if (flag(a, nullptr, "--mismatch")) o.mismatch = (float)atof(val());
        else if (flag(a, nullptr, "--transition")) o.transition = (float)atof(val());
        else if (flag(a, nullptr, "--gap-open")) o.gapOpen = (float)atof(val());
        else if (flag(a, nullptr, "--gap-extend")) o.gapExtend = (float)atof(val());
        else if (flag(a, nullptr, "--gap-ends")) { o.gapEnds = (float)atof(val()); o.hasGapEnds = true; }
        else if (flag(a, nullptr, "--xdrop")) o.xdrop = (float)atof(val());
        else if (flag(a, "-b", "--blosum")) o.blosum = atoi(val());
        else if (flag(a, "-x", "--matrix")) o.matrixFile = val();
        else if (flag(a, nullptr, "--length-deviation")) o.lenDev = (float)atof(val());
        else if (flag(a, nullptr, "--max-ambig")) o.maxAmbig = (float)atof(val());
        else if (flag(a, nullptr, "--max-len")) o.maxLen = atoi(val());
        else if (flag(a, nullptr, "--min-len")) o.minLen = atoi(val());
        else if (flag(a, nullptr, "--filter")) o.noFilter = false;
        else if (flag(a, nullptr, "--check")) o.debug = true;
        else if (flag(a, "-v", "--verbose")) o.printDetail = true;
        else if (flag(a, "--host-staged", "--host-staged")) o.hostStaged = true;
        // development / test switches (documented in include/twl_msa.h): the reference's two thresholds, replicas of the store on one device
        else if (flag(a, nullptr, "--test-cal-profile-th")) { const int v = atoi(val()); if (v > 0) o.calProfileTh = v; }
        else if (flag(a, nullptr, "--test-update-seq-th")) { const int v = atoi(val()); if (v > 0) o.updateSeqTh = v; }
        else if (flag(a, nullptr, "--test-virtual-devices")) o.testVirtualDevices = std::max(0, atoi(val()));
        else if (flag(a, nullptr, "--test-no-ownership")) o.testNoOwnership = true;
        else if (flag(a, nullptr, "--test-fork-host-staged")) o.testForkHostStaged = true;
        else if (allowPlacement && flag(a, "-a", "--alignment")) o.backboneAlnFile = val();
        else if (allowPlacement && flag(a, nullptr, "--place-on-tree")) o.placeOnTree = true;
        else if (allowPlacement && flag(a, nullptr, "--test-place-chunk")) o.testPlaceChunk = std::max(0, atoi(val()));
        else if (allowPlacement && flag(a, nullptr, "--keep-length")) o.keepLength = true;
        else if (allowPlacement && flag(a, nullptr, "--write-insertions")) o.writeInsertionsFile = val();
        else if (allowMerge && flag(a, "-f", "--files")) o.msaDir = val();
        else if (allowSubtrees && flag(a, "-m", "--max-subtree")) {
            const char *v = val();
            char *end = nullptr;
            const long n = strtol(v, &end, 10);
            if (end == v || *end != '\0' || n < 1) { std::cerr << "ERROR: -m / --max-subtree needs a number of leaves >= 1 (got " << v << ").\n"; exit(1); }
            o.maxSubtree = (int)std::min<long>(n, INT32_MAX);
            subtreesGiven = true;
        }
        else if (allowGuide && flag(a, nullptr, "--write-tree")) o.writeTreeFile = val();
        else if (allowGuide && flag(a, nullptr, "--tree-seeds")) {
            const char *v = val();
            char *end = nullptr;
            const long n = strtol(v, &end, 10);
            if (end == v || *end != '\0' || n < 2 || n > 16384) { std::cerr << "ERROR: --tree-seeds needs a number of seeds from 2 to 16384 (got " << v << ").\n"; exit(1); }
            o.treeSeeds = (int)n;
        }
        else if (allowGuide && flag(a, nullptr, "--iterations")) {
            const char *v = val();
            char *end = nullptr;
            const long n = strtol(v, &end, 10);
            if (end == v || *end != '\0' || n < 1 || n > 5) { std::cerr << "ERROR: --iterations needs a number of runs from 1 to 5 (got " << v << ").\n"; exit(1); }
            o.iterations = (int)n;
            iterationsGiven = true;
        }
        else if (allowGuide && flag(a, nullptr, "--mask-gappy")) {
            const char *v = val();
            char *end = nullptr;
            const double t = strtod(v, &end);
            if (end == v || *end != '\0' || !(t > 0.0 && t <= 1.0)) { std::cerr << "ERROR: --mask-gappy needs a value in (0, 1] (got " << v << ").\n"; exit(1); }
            o.maskGappy = t;
            maskGiven = true;
        }
        else if (allowGuide && flag(a, nullptr, "--retree-seeds")) {
            const char *v = val();
            char *end = nullptr;
            const long n = strtol(v, &end, 10);
            if (end == v || *end != '\0' || n < 2 || n > 16384) { std::cerr << "ERROR: --retree-seeds needs a number of seeds from 2 to 16384 (got " << v << ").\n"; exit(1); }
            o.retreeSeeds = (int)n;
        }
        else if (allowGuide && flag(a, nullptr, "--adjust-direction")) o.adjustDirection = true;
        else if (allowGuide && flag(a, nullptr, "--write-directions")) o.writeDirectionsFile = val();
        else if (allowGuide && flag(a, nullptr, "--direction-seeds")) {
            const char *v = val();
            char *end = nullptr;
            const long n = strtol(v, &end, 10);
            if (end == v || *end != '\0' || n < 1 || n > 16384) { std::cerr << "ERROR: --direction-seeds needs a number of seeds from 1 to 16384 (got " << v << ").\n"; exit(1); }
            o.directionSeeds = (int)n;
        }
        else if (allowTrim && flag(a, nullptr, "--trim-gappy")) {
            const char *v = val();
            char *end = nullptr;
            const double t = strtod(v, &end);
            if (end == v || *end != '\0' || !(t >= 0.0 && t <= 1.0)) { std::cerr << "ERROR: --trim-gappy needs a value in [0, 1] (got " << v << ").\n"; exit(1); }
            o.trimGappy = t;
            trimGappyGiven = true;
        }
        else if (allowTrim && flag(a, nullptr, "--trim-to")) { o.trimToName = val(); trimToGiven = true; }
        else if (allowTrim && flag(a, nullptr, "--write-columns")) o.writeColumnsFile = val();
        else if (allowCompare && flag(a, nullptr, "--compare")) o.compareFile = val();
        else if (allowCompare && flag(a, nullptr, "--write-compare")) o.writeCompareFile = val();
        else if (allowCompare && flag(a, nullptr, "--evaluate")) o.evaluateFile = val();
        else if (o.allowScore && flag(a, nullptr, "--score")) o.score = true;
        else if (o.allowScore && flag(a, nullptr, "--write-score")) o.writeScoreFile = val();
        else if (o.allowScore && flag(a, nullptr, "--score-alignment")) o.scoreAlignmentFile = val();
        else if (flag(a, nullptr, "--overwrite")) {}
        else if (flag(a, "-h", "--help")) return false;
        else { std::cerr << "ERROR: unsupported option " << a << " (this build covers the tree+sequences alignment mode only)\n"; exit(1); }
    }
    if (maskGiven && o.iterations < 2) { std::cerr << "ERROR: --mask-gappy applies to the trees that --iterations 2 or more rebuilds from an alignment.\n"; exit(1); }
    if (o.retreeSeeds > 0 && o.iterations < 2) { std::cerr << "ERROR: --retree-seeds applies to the trees that --iterations 2 or more rebuilds from an alignment.\n"; exit(1); }
    if (!o.adjustDirection && (o.directionSeeds > 0 || !o.writeDirectionsFile.empty())) {
        std::cerr << "ERROR: --direction-seeds and --write-directions apply to a run with --adjust-direction.\n";
        exit(1);
    }
    if (!o.writeInsertionsFile.empty() && !o.keepLength) { std::cerr << "ERROR: --write-insertions applies to a run with --keep-length: only there are insertions left out.\n"; exit(1); }
    if (o.keepLength) {                    // placement at the backbone's length (place.cpp): -a without a tree only
        if (!o.msaDir.empty()) { std::cerr << "ERROR: --keep-length cannot be combined with -f: a merge has no backbone whose length could be kept.\n"; exit(1); }
        if (o.placeOnTree) { std::cerr << "ERROR: --keep-length is not available with --place-on-tree: the backbone's groups are re-aligned there, so no backbone coordinate is kept.\n"; exit(1); }
        if (o.backboneAlnFile.empty()) { std::cerr << "ERROR: --keep-length applies to placement into a backbone alignment: give it with -a.\n"; exit(1); }
        if (!o.writeInsertionsFile.empty() && o.writeInsertionsFile == o.outFile) { std::cerr << "ERROR: --write-insertions names the same file as -o.\n"; exit(1); }
    }
    if (trimGappyGiven && trimToGiven) { std::cerr << "ERROR: --trim-gappy and --trim-to cannot be combined: one rule decides the columns.\n"; exit(1); }
    if (!o.writeColumnsFile.empty() && !trimGappyGiven && !trimToGiven) { std::cerr << "ERROR: --write-columns applies to a run with --trim-gappy or --trim-to: only there are columns left out.\n"; exit(1); }
    if (trimGappyGiven || trimToGiven) {   // the output without its gappy columns (trim.cpp): decided on one GPU over the rows that are written
        if (!o.writeColumnsFile.empty() && o.writeColumnsFile == o.outFile) { std::cerr << "ERROR: --write-columns names the same file as -o.\n"; exit(1); }
        if (o.keepLength) { std::cerr << "ERROR: --trim-gappy and --trim-to cannot be combined with --keep-length: its backbone rows are written from the host and never enter the trim.\n"; exit(1); }
        if (o.hostStaged) { std::cerr << "ERROR: --host-staged is not available with --trim-gappy or --trim-to (the columns are decided on the device).\n"; exit(1); }
        if (o.gpuIdx.size() > 1 || o.gpuNum > 1) { std::cerr << "ERROR: --trim-gappy and --trim-to run on one GPU: give at most one --gpu-index.\n"; exit(1); }
        o.trimRule = trimToGiven ? 1 : 0;
    }
    if (!o.writeScoreFile.empty() && !o.score && o.scoreAlignmentFile.empty()) { std::cerr << "ERROR: --write-score applies to a run with --score or --score-alignment: only there is an alignment scored.\n"; exit(1); }
    if (!o.writeScoreFile.empty() && o.writeScoreFile == o.outFile) { std::cerr << "ERROR: --write-score names the same file as -o.\n"; exit(1); }
    if (!o.scoreAlignmentFile.empty()) {   // a file scored (score.cpp): nothing is run
        if (!o.treeFile.empty() || !o.seqFile.empty() || !o.backboneAlnFile.empty() || !o.msaDir.empty() || !o.outFile.empty() || subtreesGiven || iterationsGiven || !o.evaluateFile.empty()) {
            std::cerr << "ERROR: --score-alignment scores a file and runs nothing: it cannot be combined with -t, -i, -a, -f, -o, -m, --iterations or --evaluate.\n"; exit(1);
        }
        if (o.score) { std::cerr << "ERROR: --score-alignment cannot be combined with --score: --score applies to the alignment a run writes.\n"; exit(1); }
        if (o.hostStaged) { std::cerr << "ERROR: --host-staged is not available with --score-alignment (the score's integers are counted on the device).\n"; exit(1); }
        if (o.gpuIdx.size() > 1 || o.gpuNum > 1) { std::cerr << "ERROR: --score-alignment runs on one GPU: give at most one --gpu-index.\n"; exit(1); }
        if (access(o.scoreAlignmentFile.c_str(), R_OK) != 0) { std::cerr << "ERROR: --score-alignment: cant open file: " << o.scoreAlignmentFile << '\n'; exit(1); }
        if (o.gpuIdx.empty() && o.gpuNum > 0) for (int g = 0; g < o.gpuNum; ++g) o.gpuIdx.push_back(g);
        o.typeGiven = typeGiven;
        if (!typeGiven) o.type = io::detectType(o.scoreAlignmentFile);
        return true;
    }
    if (o.score) {                         // the written alignment scored (score.cpp): on one GPU, over the rows as they are written
        if (o.keepLength) { std::cerr << "ERROR: --score cannot be combined with --keep-length: the written rows leave insertions out, so the score would not be that of the sequences.\n"; exit(1); }
        if (trimGappyGiven || trimToGiven) { std::cerr << "ERROR: --score cannot be combined with --trim-gappy or --trim-to: the written rows leave columns out, so the score would not be that of the alignment.\n"; exit(1); }
        if (o.hostStaged) { std::cerr << "ERROR: --host-staged is not available with --score (the score's integers are counted on the device).\n"; exit(1); }
        if (o.gpuIdx.size() > 1 || o.gpuNum > 1) { std::cerr << "ERROR: --score runs on one GPU: give at most one --gpu-index.\n"; exit(1); }
    }
    if (!o.writeCompareFile.empty() && o.compareFile.empty()) { std::cerr << "ERROR: --write-compare applies to a run with --compare: only there is an alignment compared.\n"; exit(1); }
    if (!o.evaluateFile.empty() && o.compareFile.empty()) { std::cerr << "ERROR: --evaluate needs --compare: the reference alignment the file is compared with.\n"; exit(1); }
    if (!o.compareFile.empty()) {          // the written alignment compared with a reference alignment (compare.cpp): on one GPU, over the rows as the input holds them
        if (!o.evaluateFile.empty() && (!o.treeFile.empty() || !o.seqFile.empty() || !o.backboneAlnFile.empty() || !o.msaDir.empty() || !o.outFile.empty() || subtreesGiven || iterationsGiven)) {
            std::cerr << "ERROR: --evaluate compares two files and runs nothing: it cannot be combined with -t, -i, -a, -f, -o, -m or --iterations.\n"; exit(1);
        }
        if (!o.writeCompareFile.empty() && o.writeCompareFile == o.outFile) { std::cerr << "ERROR: --write-compare names the same file as -o.\n"; exit(1); }
        if (o.adjustDirection) { std::cerr << "ERROR: --compare cannot be combined with --adjust-direction: a turned row does not hold the residues of its reference row.\n"; exit(1); }
        if (o.keepLength) { std::cerr << "ERROR: --compare cannot be combined with --keep-length: the written rows leave insertions out, so they are not the input's residues.\n"; exit(1); }
        if (trimGappyGiven || trimToGiven) { std::cerr << "ERROR: --compare cannot be combined with --trim-gappy or --trim-to: the written rows leave columns out, so they are not the input's residues.\n"; exit(1); }
        if (o.hostStaged) { std::cerr << "ERROR: --host-staged is not available with --compare (the comparison runs on the device).\n"; exit(1); }
        if (o.gpuIdx.size() > 1 || o.gpuNum > 1) { std::cerr << "ERROR: --compare runs on one GPU: give at most one --gpu-index.\n"; exit(1); }
        // the last check in front of the run: a mistyped path must not cost the run (nothing is read here)
        if (!o.evaluateFile.empty() && access(o.evaluateFile.c_str(), R_OK) != 0) { std::cerr << "ERROR: --evaluate: cant open file: " << o.evaluateFile << '\n'; exit(1); }
        if (access(o.compareFile.c_str(), R_OK) != 0) { std::cerr << "ERROR: --compare: cant open file: " << o.compareFile << '\n'; exit(1); }
        if (!o.evaluateFile.empty()) {     // nothing else is read or run
            if (o.gpuIdx.empty() && o.gpuNum > 0) for (int g = 0; g < o.gpuNum; ++g) o.gpuIdx.push_back(g);
            return true;
        }
    }
    if (o.adjustDirection) {               // directions (strand.cpp): decided on one GPU before anything else reads -i; the records of -i only
        if (!o.msaDir.empty()) { std::cerr << "ERROR: --adjust-direction cannot be combined with -f: the rows of an alignment cannot be turned.\n"; exit(1); }
        if (o.placeOnTree) { std::cerr << "ERROR: --adjust-direction is not available with --place-on-tree.\n"; exit(1); }
        if (o.hostStaged) { std::cerr << "ERROR: --host-staged is not available with --adjust-direction (the directions are decided on the device).\n"; exit(1); }
        if (o.gpuIdx.size() > 1 || o.gpuNum > 1) { std::cerr << "ERROR: --adjust-direction runs on one GPU: give at most one --gpu-index.\n"; exit(1); }
        if (typeGiven && o.type != 'n') { std::cerr << "ERROR: --adjust-direction applies to nucleotide sequences (--type n): a protein has no reverse complement.\n"; exit(1); }
    }
    if (o.iterations > 1) {                // iterations (retree.cpp): the tree+sequences run or the run that builds its tree, repeated on one GPU, rows device-resident
        if (!o.backboneAlnFile.empty() || !o.msaDir.empty() || subtreesGiven) { std::cerr << "ERROR: --iterations cannot be combined with -a, -f or -m.\n"; exit(1); }
        if (!o.noFilter) { std::cerr << "ERROR: --iterations cannot be combined with --filter: the rebuilt tree would lack the excluded sequences.\n"; exit(1); }
        if (o.hostStaged) { std::cerr << "ERROR: --host-staged is not available with --iterations.\n"; exit(1); }
        if (o.gpuIdx.size() > 1 || o.gpuNum > 1) { std::cerr << "ERROR: --iterations runs on one GPU: give at most one --gpu-index.\n"; exit(1); }
    }
    if (o.placeOnTree) {                   // placement along a tree (place_tree.cpp): -a, -t, -i, -o on one GPU, rows device-resident
        if (o.backboneAlnFile.empty() || o.treeFile.empty()) { std::cerr << "ERROR: --place-on-tree needs both -a (the backbone alignment) and -t (a tree over its rows and the new sequences).\n"; exit(1); }
        if (subtreesGiven || !o.msaDir.empty()) { std::cerr << "ERROR: --place-on-tree cannot be combined with -m or -f.\n"; exit(1); }
        if (o.hostStaged) { std::cerr << "ERROR: --host-staged is not available with --place-on-tree.\n"; exit(1); }
        if (o.gpuIdx.size() > 1 || o.gpuNum > 1) { std::cerr << "ERROR: --place-on-tree runs on one GPU: give at most one --gpu-index.\n"; exit(1); }
        if (!o.writeTreeFile.empty() || o.treeSeeds > 0) { std::cerr << "ERROR: --place-on-tree cannot be combined with --write-tree or --tree-seeds: the tree is given with -t.\n"; exit(1); }
    }
    if (subtreesGiven) {                   // subtrees (subtrees.cpp): the tree+sequences mode only, on one GPU, rows device-resident
        if (!o.msaDir.empty() || !o.backboneAlnFile.empty()) { std::cerr << "ERROR: -m (alignment in subtrees) cannot be combined with -a or -f.\n"; exit(1); }
        if (o.hostStaged) { std::cerr << "ERROR: --host-staged is not available with -m (alignment in subtrees).\n"; exit(1); }
        if (o.gpuIdx.size() > 1 || o.gpuNum > 1) { std::cerr << "ERROR: -m (alignment in subtrees) runs on one GPU: give at most one --gpu-index.\n"; exit(1); }
    }
    if (!o.msaDir.empty()) {               // merge (reference option.cpp: -f -o, nothing else to read)
        if (!o.treeFile.empty() || !o.seqFile.empty() || !o.backboneAlnFile.empty()) { std::cerr << "ERROR: -f (merging alignments) cannot be combined with -t, -i or -a.\n"; exit(1); }
        if (o.outFile.empty()) return false;
        if (o.hostStaged) { std::cerr << "ERROR: --host-staged is not available in merge mode (-f).\n"; exit(1); }
        if (o.gpuIdx.size() > 1 || o.gpuNum > 1) { std::cerr << "ERROR: merge mode (-f) runs on one GPU: give at most one --gpu-index.\n"; exit(1); }
        o.alnMode = MERGE_MSA;
    } else if (o.placeOnTree) {                   // placement along a tree (reference option.cpp: -t -a -i -o); its refusals are above
        if (o.seqFile.empty() || o.outFile.empty()) return false;
        o.alnMode = PLACE_W_TREE;
    } else if (!o.backboneAlnFile.empty()) {      // placement (reference option.cpp:15-22): -a -i -o without -t
        if (!o.treeFile.empty()) {
            std::cerr << "ERROR: -a together with -t (placement with a tree) is not supported yet without --place-on-tree: it re-aligns the backbone's groups along the tree.\n";
            exit(1);
        }
        if (o.seqFile.empty() || o.outFile.empty()) return false;
        if (o.hostStaged) { std::cerr << "ERROR: --host-staged is not available in placement mode (-a).\n"; exit(1); }
        if (o.gpuIdx.size() > 1 || o.gpuNum > 1) { std::cerr << "ERROR: placement mode (-a) runs on one GPU: give at most one --gpu-index.\n"; exit(1); }
        o.alnMode = PLACE_WO_TREE;
    } else if (allowGuide && o.treeFile.empty() && !o.seqFile.empty() && !o.outFile.empty()) {      // no tree: it is built from the sequences (guide.cpp), on one GPU, before anything else runs
        if (o.gpuIdx.size() > 1 || o.gpuNum > 1) { std::cerr << "ERROR: without -t the guide tree is built on one GPU before the run starts: give at most one --gpu-index, or bring a tree with -t for a run on several.\n"; exit(1); }
        if (o.hostStaged) { std::cerr << "ERROR: --host-staged is not available without -t (the guide tree is built on the device).\n"; exit(1); }
        o.buildTree = true;
    } else if (o.treeFile.empty() || o.seqFile.empty() || o.outFile.empty()) return false;
    if (!o.writeTreeFile.empty() && !o.buildTree) {
        std::cerr << (o.treeFile.empty() ? "ERROR: --write-tree applies to a run that builds its guide tree (-i and -o without -t, -a or -f).\n"
                                         : "ERROR: --write-tree cannot be combined with -t: a tree is written only where the run builds it.\n");
        exit(1);
    }
    if (o.treeSeeds > 0 && !o.buildTree) {
        std::cerr << "ERROR: --tree-seeds applies to a run that builds its guide tree (-i and -o without -t, -a or -f).\n";
        exit(1);
    }
    if (o.cpuOnly) {       // the reference's GPU builds route to their CPU kernel here (hip/alignment-gpu.hip.cpp:19-21); this build has no CPU alignment path
        std::cerr << "ERROR: --cpu-only is not available: twilight-mi355x has no CPU alignment path (the CPU checker oracle/e2e_oracle is test infrastructure).\n";
        exit(1);
    }
    if (o.gappyVertical > 1 || o.gappyVertical <= 0) { std::cerr << "ERROR: Invalid value for --remove-gappy. The value of --remove-gappy should be in (0,1]\n"; exit(1); }
    if (o.gpuIdx.empty() && o.gpuNum > 0) for (int g = 0; g < o.gpuNum; ++g) o.gpuIdx.push_back(g);
    o.typeGiven = typeGiven;
    if (!typeGiven && o.alnMode != MERGE_MSA) o.type = io::detectType(o.seqFile);      // (a merge takes it from its first file: merge.cpp)
    if (o.adjustDirection && o.type != 'n') {
        std::cerr << "ERROR: --adjust-direction applies to nucleotide sequences; " << o.seqFile << " reads as protein (a protein has no reverse complement).\n";
        exit(1);
    }
    const int maxCpu = effectiveCpus();
    if (o.cpuNum <= 0 || o.cpuNum > maxCpu) o.cpuNum = maxCpu;       // -C/--cpu, default: all usable cores (option.cpp:41-46)
    omp_set_num_threads(o.cpuNum);
    return true;
}

Tree *openTree(const Option &option)
{
    return option.treeText.empty() ? new Tree(option.treeFile) : new Tree(Tree::FromText{}, option.treeText);
}

int runDefaultAlignment(Option &option, alnFunction kernel, alnFunction deferredKernel, bool writeOutput, const std::function<void(SequenceDB *)> &atEnd,
                        const std::function<void(SequenceDB *)> &beforeAlign)
{
    auto clk = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = clk();
    SequenceDB database;
    database.updateSeqTh = option.updateSeqTh;
    database.trimRequested = writeOutput && option.trimRule >= 0;           // (of --iterations only the run that is written carries it)
    Params param(option, option.type);
    Tree *T = openTree(option);                                             // twilight-main.cpp:122
    phylogeny::assignSinglePartition(T->root);                              // :129-130 with maxSubtree = INT32_MAX
    Tree *subT = new Tree(T->root, option.reroot);                          // :145
    const double t1 = clk();
    io::readSequences(option.seqFile, &database, &option, subT);           // :146
    const double t2 = clk();
    if (beforeAlign) beforeAlign(&database);      // (a sharded run sets its communicator up here: main.cpp)
    progressive::msaOnSubtree(subT, &database, &option, param, kernel, deferredKernel);   // :148
    const double t3 = clk();
    if (option.debug && !database.debug()) std::cerr << "WARNING: --check found an illegal alignment row.\n";
    int alnLen = subT->root->getAlnLen(database.currentTask);
    if (database.trimRequested) {          // the rows lost their gappy columns in the last download, or lose them now on an uploaded copy (trim.cpp)
        if (database.trimmedLen >= 0) alnLen = database.trimmedLen;
        else if (option.trimHostRows) alnLen = option.trimHostRows(&database, &option, alnLen);
        else { std::cerr << "ERROR: this build cannot trim the alignment.\n"; exit(1); }
    }
    if (writeOutput) io::writeFinalMSA(&database, &option, alnLen);        // :165
    if (option.printDetail)
        std::cerr << "Driver phases (s): tree " << t1 - t0 << ", read " << t2 - t1 << ", align " << t3 - t2 << ", write " << clk() - t3 << '\n';
    database.finalAlnLen = alnLen;
    if (atEnd) atEnd(&database);
    delete subT;
    delete T;
    return alnLen;
}

}  // namespace msa
