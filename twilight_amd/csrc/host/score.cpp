// twilight_amd/csrc/host/score.cpp -- `--score`, `--write-score FILE`, `--score-alignment FILE`: the affine sum-of-pairs score of the alignment that was
// written, or of a file, under the run's own substitution scores and gap penalties.  Every writer of -o calls
// Option::scoreWritten once its file is closed (seqdb_io.cpp), --iterations also with the finished rows of every run but the last (retree.cpp).  The
// rows go into a store made for them (the path the trim takes for rows that exist on the host only), twl_store_score_rows (include/twl_score.h)
// counts the exact integers on the device, and the score is their linear function, in double, here.  A score that fails ends the run with exit
// code 1 and leaves -o in place.
#include "align_gpu.hpp"

#include "../../../include/twl_score.h"
#include "../twl_score_plan.inc.hip"      // (pure) score_classes, score_sub_entries, score_sub_index

#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <numeric>
#include <unordered_map>

#include <climits>

namespace msa {

using progressive::gpu::die;
using progressive::gpu::nowMs;

namespace {

std::string fixed6(double v)
{
    char buf[80];
    snprintf(buf, sizeof buf, "%.6f", v);
    return buf;
}

// the rows `names` / `rows` (W columns each) scored; ends the process on every refusal
void scoreRows(Option &option, const std::vector<std::string> &names, const std::vector<const char *> &rows, int32_t W, const char *flag)
{
    const double t0 = nowMs();
    const size_t n = rows.size();
    if (n < 2) { std::cerr << "ERROR: " << flag << ": " << n << " row(s); a sum-of-pairs score needs at least 2.\n"; exit(1); }
    if (n > (size_t)TWL_SCORE_MAX_ROWS) { std::cerr << "ERROR: " << flag << ": " << n << " rows; at most " << TWL_SCORE_MAX_ROWS << " are scored.\n"; exit(1); }
    if (W < 1) { std::cerr << "ERROR: " << flag << ": the alignment has no column.\n"; exit(1); }
    const int32_t K = score_classes(option.type);
    if (K == 0) { std::cerr << "ERROR: " << flag << ": unknown sequence type " << option.type << " (--type n or p).\n"; exit(1); }
    Params param(option, option.type);
    progressive::gpu::ensureInit(&option);
    const int device = progressive::gpu::selectedDevices().empty() ? 0 : progressive::gpu::selectedDevices()[0];
    std::vector<int32_t> lens(n, W), ids(n);
    std::iota(ids.begin(), ids.end(), 0);
    twl_store *st = nullptr;
    int rc = twl_store_create(device, option.type, (int32_t)n, rows.data(), lens.data(), &st);
    if (rc != TWL_OK) die("twl_store_create", rc);
    std::vector<uint64_t> sub((size_t)score_sub_entries(K)), runs(n);
    uint64_t totals[5] = {0, 0, 0, 0, 0};
    if ((rc = twl_store_score_rows(st, (int32_t)n, ids.data(), option.type, sub.data(), runs.data(), totals)) != TWL_OK) die("twl_store_score_rows", rc);
    double packMs = 0, colsMs = 0, pairsMs = 0;
    (void)twl_store_score_timing(st, &packMs, &colsMs, &pairsMs);
    twl_store_destroy(st);
    const uint64_t R = totals[0], G = totals[1], RT = totals[2], GT = totals[3], letters = totals[4];
    const uint64_t pairs = (uint64_t)n * (uint64_t)(n - 1) / 2;
    // the score, in double from exact integers, in the order of DESIGN.md section 4o; a pair with the class "other" scores 0
    double S = 0;
    for (int32_t a = 0; a < K; ++a)
        for (int32_t b = a; b < K; ++b) S += (double)sub[(size_t)score_sub_index(K, a, b)] * (double)param.scoringMatrix[a][b];
    S += (double)param.gapOpen * (double)(R - RT);
    S += (double)param.gapExtend * (double)((G - GT) - (R - RT));
    S += (double)param.gapBoundary * (double)GT;
    const std::string s = fixed6(S), perPair = fixed6(S / (double)pairs);
    if (option.scoreRun > 0) std::cerr << "run " << option.scoreRun << ' ';
    std::cerr << "score: rows " << n << " columns " << W << " pairs " << pairs << " letters " << letters << " gapcols " << G << " runs " << R << " terminal " << RT << '/' << GT
              << " score " << s << " per_pair " << perPair << '\n';
    if (option.printDetail)
        fprintf(stderr, "Score kernels (ms): pack %.3f, columns %.3f, pairs %.3f; all with the upload of the rows %.3f\n", packMs, colsMs, pairsMs, nowMs() - t0);
    if (!option.writeScoreFile.empty()) {
        std::ofstream out(option.writeScoreFile, std::ios::binary);
        if (!out) { std::cerr << "ERROR: Failed to open file: " << option.writeScoreFile << '\n'; exit(1); }
        std::string text;
        text += "#rows\t" + std::to_string(n) + "\n#columns\t" + std::to_string(W) + "\n#pairs\t" + std::to_string(pairs) + "\n#letters\t" + std::to_string(letters) + "\n#gapcols\t" + std::to_string(G) +
                "\n#runs\t" + std::to_string(R) + "\n#terminal_runs\t" + std::to_string(RT) + "\n#terminal_gapcols\t" + std::to_string(GT) + "\n#score\t" + s + "\n#per_pair\t" + perPair + '\n';
        for (int32_t a = 0; a <= K; ++a)
            for (int32_t b = a; b <= K; ++b) text += "#sub_" + std::to_string(a) + '_' + std::to_string(b) + '\t' + std::to_string(sub[(size_t)score_sub_index(K, a, b)]) + '\n';
        for (size_t k = 0; k < n; ++k) {
            uint64_t l = 0;
            for (int32_t c = 0; c < W; ++c) l += rows[k][c] != '-';
            text += names[k] + '\t' + std::to_string(l) + '\t' + std::to_string(runs[k]) + '\n';
        }
        out << text;
        out.close();
        if (!out) { std::cerr << "ERROR: Failed to write file: " << option.writeScoreFile << '\n'; exit(1); }
    }
}

}  // namespace

void enableScore(Option &option)
{
    if (!option.score) return;
    Option *opt = &option;
    option.scoreWritten = [opt](const std::vector<std::string> &names, const std::vector<const char *> &rows, int W) { scoreRows(*opt, names, rows, (int32_t)W, "--score"); };
}

int runScoreAlignment(Option &option)
{
    std::vector<std::string> names, seqs;
    io::readRecords(option.scoreAlignmentFile, [&](std::string &name, std::string &seq) { names.push_back(name); seqs.push_back(std::move(seq)); });
    if (seqs.empty()) { std::cerr << "ERROR: --score-alignment: " << option.scoreAlignmentFile << " holds no record.\n"; exit(1); }
    if (seqs[0].size() > (size_t)INT32_MAX) { std::cerr << "ERROR: --score-alignment: the rows of " << option.scoreAlignmentFile << " hold " << seqs[0].size() << " columns, more than an alignment of this tool can.\n"; exit(1); }
    for (size_t k = 1; k < seqs.size(); ++k)
        if (seqs[k].size() != seqs[0].size()) {
            std::cerr << "ERROR: --score-alignment: the rows of " << option.scoreAlignmentFile << " differ in length (\"" << names[k] << "\" holds " << seqs[k].size() << " columns, \"" << names[0]
                      << "\" " << seqs[0].size() << "): an alignment has rows of one length.\n";
            exit(1);
        }
    std::vector<const char *> rows;
    for (const std::string &r : seqs) rows.push_back(r.data());
    scoreRows(option, names, rows, (int32_t)seqs[0].size(), "--score-alignment");
    return 0;
}

}  // namespace msa
