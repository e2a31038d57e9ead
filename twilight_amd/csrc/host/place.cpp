// twilight_amd/csrc/host/place.cpp -- PLACE_WO_TREE: new sequences placed into an existing alignment, without a tree
// (reference src/twilight-main.cpp:212-236, `twilight -a backbone.aln -i new.fa -o out.aln`).
//
// Every new sequence is aligned, independently, to the profile of the whole backbone (alignment-cpu.cpp with currentTask 2: gapCharScore 0,
// a failed pair retried until it passes, low-quality sequences neither aligned nor written).  All of it runs on one device:
//   backbone rows + new sequences -> one store; twl_store_count_columns -> the backbone's profile (readAlignment, io.cpp:200-238)
//   chunks of new sequences       -> twl_level_prepare / twl_level_align / twl_level_restore, unchanged (include/twl_level.h)
//   twl_place_collect             -> their final paths kept in HBM, the longest insertion per backbone slot (mergeInsertions)
//   twl_place_finish              -> every row at the final width (io.cpp:355-449), read back once and written
// With --keep-length (include/twl_keep.h) the last step is twl_place_finish_keep instead: the placed sequences become rows of the
// backbone's own length, their insertions are left out (and listed with --write-insertions); the backbone rows are written from the host copy, which
// is kept in this mode, and only the placed rows are read back.
// Two deliberate differences from the reference: a backbone row of another length is refused (the reference warns and writes the row at
// its own width), and the output order is fixed: the backbone rows in file order, then the placed sequences in input order (the reference
// concatenates its temporary files by shell glob).
#include "align_gpu.hpp"

#include "../../../include/twl_place.h"
#include "../../../include/twl_keep.h"

#include <algorithm>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <numeric>
#include <string>
#include <vector>

namespace msa {

using progressive::gpu::baseParams;
using progressive::gpu::die;
using progressive::gpu::nowMs;
using progressive::gpu::alignWithRetry;
using progressive::gpu::finalPathsOfLevel;

namespace {

// Device memory one pair of a chunk takes in the level buffers: raw profiles and packed DP columns of both sides (2 * seq_len * (2P + 2)
// floats), the DP output and the column info.  A chunk gets kChunkBudget of it.
constexpr double kChunkBudget = 16.0 * (1 << 30);
constexpr int kMaxChunk = 4096;

struct Totals { double count = 0, dp = 0, restore = 0, collect = 0, finish = 0, runs = 0, read = 0, write = 0; progressive::gpu::DpTotals run; int restoredOnHost = 0; };

// The finish of --keep-length (include/twl_keep.h): the placed sequences become rows of the backbone's length L on the device and are read back; the backbone
// rows are written from the host copy as they were read; the runs of letters left out are counted, and listed where --write-insertions asks for them.
// Ends the placement and the store.  Returns L.
int finishKeepingLength(Option &option, twl_store *st, twl_place *pl, int32_t L, const std::vector<std::string> &bbNames, const std::vector<std::string> &bbRows,
                        const std::vector<SequenceDB::SequenceInfo *> &placed, Totals &tot, int32_t nChunks, int32_t chunk)
{
    const int32_t B = (int32_t)bbRows.size(), M = (int32_t)placed.size();
    int rc;
    double t;
    std::vector<int32_t> collected;                    // store ids with a path, in input order (an empty sequence has none when L is 0)
    for (int32_t k = 0; k < M; ++k) if (placed[k]->len > 0 || L > 0) collected.push_back(B + k);
    const int32_t nC = (int32_t)collected.size();
    int64_t runs = 0, letters = 0;
    t = nowMs();
    if ((rc = twl_place_finish_keep(pl, &runs, &letters)) != TWL_OK) die("twl_place_finish_keep", rc);
    tot.finish = nowMs() - t;
    t = nowMs();
    std::vector<int32_t> longest((size_t)L + 1), nRuns((size_t)nC), nLetters((size_t)nC);
    if ((rc = twl_place_read_insertions(pl, longest.data())) != TWL_OK) die("twl_place_read_insertions", rc);
    int64_t merged = L;
    for (int32_t v : longest) merged += v;
    if ((rc = twl_place_dropped_counts(pl, nC, collected.data(), nRuns.data(), nLetters.data())) != TWL_OK) die("twl_place_dropped_counts", rc);
    int32_t withRuns = 0;
    std::vector<int64_t> runOff((size_t)nC + 1, 0);
    for (int32_t i = 0; i < nC; ++i) { runOff[i + 1] = runOff[i] + nRuns[i]; withRuns += nRuns[i] > 0; }
    if (!option.writeInsertionsFile.empty()) {
        std::vector<int32_t> col((size_t)runOff[nC] + 1), qpos((size_t)runOff[nC] + 1), len((size_t)runOff[nC] + 1);
        if ((rc = twl_place_dropped_runs(pl, nC, collected.data(), runOff.data(), col.data(), qpos.data(), len.data())) != TWL_OK) die("twl_place_dropped_runs", rc);
        std::ofstream ins(option.writeInsertionsFile, std::ios::binary);
        if (!ins) { std::cerr << "ERROR: Failed to open file: " << option.writeInsertionsFile << '\n'; exit(1); }
        for (int32_t i = 0; i < nC; ++i) {
            const auto *s = placed[collected[i] - B];
            const bool reversed = option.reversedNames.count(s->name) > 0;
            for (int64_t r = runOff[i]; r < runOff[i + 1]; ++r) {
                if (qpos[r] < 0 || len[r] < 1 || (int64_t)qpos[r] + len[r] > s->len) { std::cerr << "ERROR: a dropped run of " << s->name << " lies outside its sequence.\n"; exit(1); }
                ins << (reversed ? "_R_" : "") << s->name << '\t' << col[r] << '\t';
                ins.write(s->alnStorage[0] + qpos[r], len[r]);
                ins << '\n';
            }
        }
        ins.close();
        if (!ins) { std::cerr << "ERROR: Failed to write file: " << option.writeInsertionsFile << '\n'; exit(1); }
    }
    tot.runs = nowMs() - t;
    double rowsKernelMs = 0, runsKernelMs = 0;
    (void)twl_place_keep_timing(pl, &rowsKernelMs, &runsKernelMs);
    t = nowMs();
    std::vector<int32_t> outIds((size_t)M), outLen((size_t)M);
    std::iota(outIds.begin(), outIds.end(), B);
    std::vector<char> rows((size_t)M * (size_t)L + 1);
    if ((rc = twl_store_read_rows_of(st, M, outIds.data(), rows.data(), outLen.data())) != TWL_OK) die("twl_store_read_rows_of", rc);
    for (int32_t k = 0; k < M; ++k)
        if (outLen[k] != L) { std::cerr << "ERROR: the row of " << placed[k]->name << " has " << outLen[k] << " columns, not the backbone's " << L << ".\n"; exit(1); }
    tot.read = nowMs() - t;
    twl_place_destroy(pl);
    twl_store_destroy(st);
    t = nowMs();
    {
        std::vector<const std::string *> names;
        std::vector<const char *> rowAt;
        for (int32_t k = 0; k < B; ++k) { names.push_back(&bbNames[k]); rowAt.push_back(bbRows[k].data()); }
        for (int32_t k = 0; k < M; ++k) { names.push_back(&placed[k]->name); rowAt.push_back(&rows[(size_t)k * (size_t)L]); }
        io::writeRecords(option.outFile, names, rowAt, L, &option, (size_t)B);      // (only new sequences are ever turned)
    }
    tot.write = nowMs() - t;
    std::cerr << "Placed " << M << " sequences into " << B << " backbone rows: final alignment length " << L << " (backbone " << L << "), "
              << nChunks << " chunk(s) of at most " << chunk << ", " << tot.run.retries << " retried DP run(s)\n";
    std::cerr << "Kept the backbone's length " << L << ": " << runs << " insertion run(s), " << letters << " letter(s) of " << withRuns
              << " sequence(s) left out (merged they would make " << merged << " columns)\n";
    if (option.printDetail)
        fprintf(stderr, "Placement phases (ms): count %.3f, prepare+DP %.3f, restore %.3f, collect %.3f, keep-finish %.3f, runs %.3f, read-back %.3f, write %.3f; "
                        "DP kernel %.3f ms, %llu band cells; restored on the host %d; keep kernels: rows %.3f ms, runs %.3f ms\n", tot.count, tot.dp, tot.restore,
                tot.collect, tot.finish, tot.runs, tot.read, tot.write, tot.run.kernel, (unsigned long long)tot.run.cells, tot.restoredOnHost, rowsKernelMs, runsKernelMs);
    return L;
}

}  // namespace

int runPlacement(Option &option)
{
    using progressive::gpu::ensureInit;
    using progressive::gpu::selectedDevices;
    Totals tot;
    Params param(option, option.type);

    // ---- the backbone: every row must have the first row's length ----
    std::vector<std::string> bbNames, bbRows;
    const int32_t L = io::readAlignedRows(option.backboneAlnFile, "a backbone alignment", bbNames, bbRows);
    if (L < 0) { std::cerr << "ERROR: no rows were read from the backbone alignment " << option.backboneAlnFile << ".\n"; exit(1); }
    std::cerr << "==== Backbone Alignment ====\nNumber : " << bbRows.size() << "\nLength:  " << L << '\n';

    // ---- new sequences, read and flagged as readSequences does: the "tree" is the star of their names (twilight-main.cpp:214-217) ----
    SequenceDB database;
    database.currentTask = 2;
    Tree *names = new Tree();
    io::readRecords(option.seqFile, [&](std::string &name, std::string &) {
        if (names->allNodes.count(name)) return;
        Node *leaf = new Node(name, 0.0f);
        leaf->grpID = 0;
        leaf->weight = 1.0f;
        names->allNodes[name] = leaf;
    });
    io::readSequences(option.seqFile, &database, &option, names);
    delete names;
    std::vector<SequenceDB::SequenceInfo *> placed;
    int lowQ = 0;
    for (auto *s : database.sequences) { if (s->lowQuality) ++lowQ; else placed.push_back(s); }
    std::cerr << "Low-quality sequences (not placed): " << lowQ << '\n';

    // ---- one store: backbone rows [0, B), placed sequences [B, B + M) ----
    ensureInit(&option);
    const int device = selectedDevices().empty() ? 0 : selectedDevices()[0];
    const int32_t B = (int32_t)bbRows.size(), M = (int32_t)placed.size();
    std::vector<const char *> rowPtr;
    std::vector<int32_t> rowLen;
    for (auto &r : bbRows) { rowPtr.push_back(r.data()); rowLen.push_back(L); }
    for (auto *s : placed) { rowPtr.push_back(s->alnStorage[0]); rowLen.push_back(s->len); }
    twl_store *st = nullptr;
    int rc = twl_store_create(device, option.type, B + M, rowPtr.data(), rowLen.data(), &st);
    if (rc != TWL_OK) die("twl_store_create", rc);
    if (!option.keepLength) for (auto &r : bbRows) std::string().swap(r);      // (--keep-length writes the backbone from these very bytes)
    std::vector<int32_t> bbIds(B);
    std::iota(bbIds.begin(), bbIds.end(), 0);
    double t = nowMs();
    constexpr int32_t kBackboneCache = 0;
    if ((rc = twl_store_count_columns(st, B, bbIds.data(), kBackboneCache)) != TWL_OK) die("twl_store_count_columns", rc);
    tot.count = nowMs() - t;
    twl_place *pl = nullptr;
    if ((rc = twl_place_create(st, L, &pl)) != TWL_OK) die("twl_place_create", rc);

    // ---- one pair per sequence: reference side = the backbone's cached profile (num = weight = B), query side = the sequence ----
    const twl_params tp = baseParams(param);
    twl_params tz = tp;
    tz.gap_char = 0;                                       // alignment-cpu.cpp:88 (currentTask 2)
    const int P = option.type == 'n' ? 6 : 22;

    // an empty sequence: L reference-only codes (alignment-cpu.cpp:90), straight from the host
    std::vector<int32_t> todo;                             // store ids of the sequences that go through the DP
    {
        std::vector<int32_t> ids, lens;
        for (int32_t k = 0; k < M; ++k) {
            if (placed[k]->len == 0) { ids.push_back(B + k); lens.push_back(L); }
            else todo.push_back(B + k);
        }
        if (!ids.empty() && L > 0) {
            std::vector<int8_t> rows(ids.size() * (size_t)L, 2);
            t = nowMs();
            if ((rc = twl_place_collect(pl, st, (int32_t)ids.size(), ids.data(), rows.data(), lens.data(), L, nullptr)) != TWL_OK) die("twl_place_collect", rc);
            tot.collect += nowMs() - t;
        }
    }
    const auto qlen = [&](int32_t id) { return placed[id - B]->len; };

    // one level of the pairs of `ids`; returns the error code of every pair (those with err != 0 are not collected).  errIn: ONE pair whose
    // first DP run ended with (*errIn)[0] != 0
    auto runLevel = [&](const std::vector<int32_t> &ids, const twl_params &prm, std::vector<int16_t> *errIn) {
        const int32_t n = (int32_t)ids.size();
        int32_t maxLen = L;
        for (int32_t id : ids) maxLen = std::max(maxLen, qlen(id));
        std::vector<twl_side> sides(2 * (size_t)n);
        std::vector<float> mw((size_t)n, 1.0f);           // seq.weight / groupWeight * num of a lone sequence
        std::vector<int32_t> sideLen(2 * (size_t)n);
        for (int32_t i = 0; i < n; ++i) {
            sides[2 * i] = twl_side{0, 0, L, B, (float)B, kBackboneCache, -1, 0};
            sides[2 * i + 1] = twl_side{1, i, qlen(ids[i]), 1, 1.0f, -1, -1, 0};
            sideLen[2 * i] = L; sideLen[2 * i + 1] = qlen(ids[i]);
        }
        std::vector<int32_t> lenOut(2 * (size_t)n), alnLen((size_t)n);
        std::vector<int16_t> err((size_t)n);
        double t0 = nowMs();
        if ((rc = twl_level_prepare(st, &tp, option.gappyVertical, n, sides.data(), ids.data(), mw.data(), maxLen, lenOut.data(), nullptr)) != TWL_OK) die("twl_level_prepare", rc);
        // a pair that failed in its chunk (alignment-cpu.cpp:95-128 with currentTask != 0): alone, retried until errorType 0
        const std::string what = errIn ? "sequence " + placed[ids[0] - B]->name : std::string();
        alignWithRetry(st, device, prm, option, errIn ? &what : nullptr, errIn ? errIn->data() : nullptr, std::min(lenOut[0], lenOut[1]), alnLen.data(), err.data(), tot.run);
        tot.dp += nowMs() - t0;
        // gappy columns back (alignment-helper.cpp:324-375) for the pairs that lost a column; the others are final as the DP left them
        t0 = nowMs();
        const progressive::gpu::AlignedLevel al{n, sideLen.data(), lenOut.data(), alnLen.data(), err.data(), maxLen, L + maxLen};
        const progressive::gpu::FinalPaths fin = finalPathsOfLevel(st, tp, param, option, al);
        tot.restoredOnHost += fin.restoredOnHost;
        tot.restore += nowMs() - t0;
        t0 = nowMs();
        if ((rc = twl_place_collect(pl, st, n, ids.data(), nullptr, fin.pathLen.data(), al.pathStride, fin.fromDp.data())) != TWL_OK) die("twl_place_collect", rc);
        tot.collect += nowMs() - t0;
        return err;
    };

    // ---- chunks of pairs sized to the device-memory budget (the level buffers of every pair of a 10 kbp input do not fit at once) ----
    int32_t maxQ = 1;
    for (int32_t id : todo) maxQ = std::max(maxQ, qlen(id));
    const double perPair = 2.0 * std::max(L, maxQ) * (2 * P + 2) * sizeof(float) + 4.0 * std::max(L, maxQ);
    int32_t chunk = (int32_t)std::max(1.0, std::min<double>(kMaxChunk, kChunkBudget / perPair));
    if (option.testPlaceChunk > 0) chunk = option.testPlaceChunk;
    int32_t nChunks = 0;
    for (size_t at = 0; at < todo.size(); at += (size_t)chunk, ++nChunks) {
        std::vector<int32_t> ids(todo.begin() + at, todo.begin() + std::min(todo.size(), at + (size_t)chunk));
        std::vector<int16_t> err = runLevel(ids, tz, nullptr);
        for (size_t i = 0; i < ids.size(); ++i)
            if (err[i] != 0) {
                std::vector<int16_t> e1{err[i]};
                runLevel(std::vector<int32_t>{ids[i]}, tz, &e1);
            }
    }

    if (option.keepLength) return finishKeepingLength(option, st, pl, L, bbNames, bbRows, placed, tot, nChunks, chunk);      // 

    // ---- merged insertions, final rows, output ----
    int32_t W = 0;
    t = nowMs();
    if ((rc = twl_place_finish(pl, B, bbIds.data(), &W)) != TWL_OK) die("twl_place_finish", rc);
    tot.finish = nowMs() - t;
    t = nowMs();
    std::vector<int32_t> outIds(bbIds);
    for (int32_t k = 0; k < M; ++k) outIds.push_back(B + k);
    std::vector<int32_t> outLen(outIds.size());
    std::vector<char> rows;
    const int32_t mergedW = W;
    if (option.trimRule >= 0)              // the rows lose their gappy columns on the device first (trim.cpp): W is the kept length from here on
        W = trimAndReadRows(option, st, (int32_t)outIds.size(), outIds.data(),
                            [&](int32_t k) { return k < B ? bbNames[(size_t)k] : writtenNameOf(option, placed[(size_t)(k - B)]->name); }, rows);      // (only new sequences are ever turned)
    else {
        rows.resize((size_t)outIds.size() * (size_t)W + 1);
        if ((rc = twl_store_read_rows_of(st, (int32_t)outIds.size(), outIds.data(), rows.data(), outLen.data())) != TWL_OK) die("twl_store_read_rows_of", rc);
    }
    tot.read = nowMs() - t;
    twl_place_destroy(pl);
    twl_store_destroy(st);
    t = nowMs();
    {
        std::vector<const std::string *> names;
        std::vector<const char *> rowAt;
        for (size_t k = 0; k < outIds.size(); ++k) { names.push_back(k < (size_t)B ? &bbNames[k] : &placed[k - B]->name); rowAt.push_back(&rows[k * (size_t)W]); }
        io::writeRecords(option.outFile, names, rowAt, W, &option, (size_t)B);      // (only new sequences are ever turned)
    }
    tot.write = nowMs() - t;
    std::cerr << "Placed " << M << " sequences into " << B << " backbone rows: final alignment length " << mergedW << " (backbone " << L << "), "
              << nChunks << " chunk(s) of at most " << chunk << ", " << tot.run.retries << " retried DP run(s)\n";
    if (option.printDetail)
        fprintf(stderr, "Placement phases (ms): count %.3f, prepare+DP %.3f, restore %.3f, collect %.3f, finish %.3f, read-back %.3f, write %.3f; "
                        "DP kernel %.3f ms, %llu band cells; restored on the host %d\n", tot.count, tot.dp, tot.restore, tot.collect, tot.finish, tot.read, tot.write,
                tot.run.kernel, (unsigned long long)tot.run.cells, tot.restoredOnHost);
    return W;
}

}  // namespace msa
