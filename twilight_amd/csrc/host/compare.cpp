// twilight_amd/csrc/host/compare.cpp -- `--compare REF`, `--write-compare FILE`, `--evaluate EST`: the alignment that was written, or a file, compared
// with a reference alignment of the same sequences.  The rows are matched by name (the reader's rule: first word, a
// duplicate keeps its first record), the rows both sides hold are uploaded into one compare object (include/twl_compare.h), and the sums of
// what comes back are printed as one line: shared residue pairs over the reference's pairs (SP), over the output's pairs (modeler), reference
// columns recovered whole (TC).  Every writer of -o calls Option::compareWritten once its file is closed (seqdb_io.cpp): a comparison that fails
// ends the run with exit code 1 and leaves -o in place.
#include "align_gpu.hpp"

#include "../../../include/twl_compare.h"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <unordered_map>

#include <climits>

namespace msa {

using progressive::gpu::die;
using progressive::gpu::nowMs;

namespace {

struct AlignedFile { std::vector<std::string> names, rows; int32_t W = 0; };

// every record of an alignment file, a duplicate name keeping its first record; rows of two lengths end the run
AlignedFile readAligned(const std::string &path, const char *flag)
{
    AlignedFile f;
    std::unordered_map<std::string, size_t> seen;
    io::readRecords(path, [&](std::string &name, std::string &seq) {
        if (!seen.emplace(name, f.names.size()).second) return;
        f.names.push_back(name); f.rows.push_back(std::move(seq));
    });
    if (f.rows.empty()) { std::cerr << "ERROR: " << flag << ": " << path << " holds no record.\n"; exit(1); }
    if (f.rows[0].size() > (size_t)INT32_MAX) { std::cerr << "ERROR: " << flag << ": the rows of " << path << " hold " << f.rows[0].size() << " columns, more than an alignment of this tool can.\n"; exit(1); }
    f.W = (int32_t)f.rows[0].size();
    for (size_t k = 1; k < f.rows.size(); ++k)
        if (f.rows[k].size() != f.rows[0].size()) {
            std::cerr << "ERROR: " << flag << ": the rows of " << path << " differ in length (\"" << f.names[k] << "\" holds " << f.rows[k].size() << " columns, \"" << f.names[0] << "\" "
                      << f.rows[0].size() << "): an alignment has rows of one length.\n";
            exit(1);
        }
    return f;
}

std::string ratio(uint64_t a, uint64_t b)
{
    if (b == 0) return "nan";
    char buf[64];
    snprintf(buf, sizeof buf, "%.6f", (double)a / (double)b);
    return buf;
}

int64_t lettersOf(const char *row, int32_t W) { int64_t n = 0; for (int32_t c = 0; c < W; ++c) n += row[c] != '-'; return n; }

// the rows `names` / `rows` (W columns each) against the file option.compareFile; ends the process on every refusal
void compareRows(Option &option, const std::vector<std::string> &names, const std::vector<const char *> &rows, int32_t W)
{
    const double t0 = nowMs();
    const AlignedFile ref = readAligned(option.compareFile, "--compare");
    std::unordered_map<std::string, size_t> refAt;
    for (size_t k = 0; k < ref.names.size(); ++k) refAt.emplace(ref.names[k], k);
    std::vector<const char *> est, rf;
    std::vector<size_t> common;      // index into names
    std::unordered_map<std::string, size_t> outSeen;
    size_t outDistinct = 0;
    for (size_t k = 0; k < names.size(); ++k) {
        if (!outSeen.emplace(names[k], k).second) continue;
        ++outDistinct;
        const auto it = refAt.find(names[k]);
        if (it == refAt.end()) continue;
        common.push_back(k); est.push_back(rows[k]); rf.push_back(ref.rows[it->second].data());
    }
    const size_t n = common.size(), onlyOut = outDistinct - n, onlyRef = ref.names.size() - n;
    if (n < 2) {
        std::cerr << "ERROR: --compare: the output and " << option.compareFile << " have " << n << " name(s) in common; a comparison needs at least 2 ("
                  << onlyOut << " only in the output, " << onlyRef << " only in the reference).\n";
        exit(1);
    }
    if (n > (size_t)TWL_COMPARE_MAX_ROWS) { std::cerr << "ERROR: --compare: " << n << " common rows; at most " << TWL_COMPARE_MAX_ROWS << " are compared.\n"; exit(1); }
    progressive::gpu::ensureInit(&option);
    const int device = progressive::gpu::selectedDevices().empty() ? 0 : progressive::gpu::selectedDevices()[0];
    twl_compare *cmp = nullptr;
    int32_t bad = -1;
    int rc = twl_compare_create(device, (int32_t)n, W, est.data(), ref.W, rf.data(), &cmp, &bad);
    if (rc != TWL_OK && bad >= 0) {
        const int64_t le = lettersOf(est[(size_t)bad], W), lr = lettersOf(rf[(size_t)bad], ref.W);
        std::cerr << "ERROR: --compare: the row \"" << names[common[(size_t)bad]] << "\" does not hold the sequence of its row in " << option.compareFile << ": ";
        if (le != lr) std::cerr << "the letter count differs (" << le << " in the output, " << lr << " in the reference).\n";
        else std::cerr << "the letters differ (both hold " << le << ").\n";
        exit(1);
    }
    if (rc != TWL_OK) die("twl_compare_create", rc);
    std::vector<uint64_t> shared((size_t)W);
    std::vector<uint32_t> letters((size_t)W), distinct((size_t)W), refLetters((size_t)ref.W);
    std::vector<uint8_t> recovered((size_t)W);
    if ((rc = twl_compare_columns(cmp, shared.data(), letters.data(), distinct.data(), recovered.data(), refLetters.data())) != TWL_OK) die("twl_compare_columns", rc);
    double upMs = 0, keysMs = 0, colsMs = 0, downMs = 0;
    (void)twl_compare_timing(cmp, &upMs, &keysMs, &colsMs, &downMs);
    twl_compare_destroy(cmp);
    uint64_t sShared = 0, pairsOut = 0, pairsRef = 0, nRecovered = 0, refColumns = 0;
    for (int32_t c = 0; c < W; ++c) { sShared += shared[c]; pairsOut += (uint64_t)letters[c] * (letters[c] ? letters[c] - 1 : 0) / 2; nRecovered += recovered[c]; }
    for (int32_t b = 0; b < ref.W; ++b) { pairsRef += (uint64_t)refLetters[b] * (refLetters[b] ? refLetters[b] - 1 : 0) / 2; refColumns += refLetters[b] >= 2 ? 1 : 0; }
    const std::string sp = ratio(sShared, pairsRef), modeler = ratio(sShared, pairsOut);
    std::cerr << "compare: rows " << n << " (" << onlyOut << " only in the output, " << onlyRef << " only in the reference) pairs_out " << pairsOut << " pairs_ref " << pairsRef
              << " shared " << sShared << " SP " << sp << " modeler " << modeler << " TC " << nRecovered << '/' << refColumns << " columns " << W << '/' << ref.W << '\n';
    int32_t consts[4] = {0, 1, 0, 0};      // [1]: the column tile the keys' pitch is rounded up to
    (void)twl_compare_describe(consts);
    if (option.printDetail)
        fprintf(stderr, "Compare phases (ms): upload %.3f, key kernels %.3f, column kernel %.3f, download %.3f, all with reading the reference %.3f; residue keys %.1f MB on the device\n",
                upMs, keysMs, colsMs, downMs, nowMs() - t0, (double)n * (double)(((int64_t)W + consts[1] - 1) / consts[1] * consts[1]) * 4.0 / 1e6);
    if (!option.writeCompareFile.empty()) {
        std::ofstream out(option.writeCompareFile, std::ios::binary);
        if (!out) { std::cerr << "ERROR: Failed to open file: " << option.writeCompareFile << '\n'; exit(1); }
        std::string text;
        text += "#rows\t" + std::to_string(n) + "\n#only_in_output\t" + std::to_string(onlyOut) + "\n#only_in_reference\t" + std::to_string(onlyRef) + "\n#pairs_out\t" + std::to_string(pairsOut) +
                "\n#pairs_ref\t" + std::to_string(pairsRef) + "\n#shared\t" + std::to_string(sShared) + "\n#SP\t" + sp + "\n#modeler\t" + modeler + "\n#TC_recovered\t" + std::to_string(nRecovered) +
                "\n#TC_columns\t" + std::to_string(refColumns) + "\n#columns_out\t" + std::to_string(W) + "\n#columns_ref\t" + std::to_string(ref.W) + '\n';
        for (int32_t c = 0; c < W; ++c)
            text += std::to_string(c) + '\t' + std::to_string(letters[c]) + '\t' + std::to_string((uint64_t)letters[c] * (letters[c] ? letters[c] - 1 : 0) / 2) + '\t' + std::to_string(shared[c]) + '\t' +
                    std::to_string(distinct[c]) + '\t' + std::to_string((int)recovered[c]) + '\n';
        out << text;
        out.close();
        if (!out) { std::cerr << "ERROR: Failed to write file: " << option.writeCompareFile << '\n'; exit(1); }
    }
}

}  // namespace

void enableCompare(Option &option)
{
    if (option.compareFile.empty()) return;
    Option *opt = &option;
    option.compareWritten = [opt](const std::vector<std::string> &names, const std::vector<const char *> &rows, int W) { compareRows(*opt, names, rows, (int32_t)W); };
}

int runEvaluate(Option &option)
{
    const AlignedFile est = readAligned(option.evaluateFile, "--evaluate");
    std::vector<const char *> rows;
    for (const std::string &r : est.rows) rows.push_back(r.data());
    compareRows(option, est.names, rows, est.W);
    return 0;
}

}  // namespace msa
