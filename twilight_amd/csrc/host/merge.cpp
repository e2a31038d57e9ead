// twilight_amd/csrc/host/merge.cpp -- MERGE_MSA: the alignments of a directory merged into one
// (reference src/twilight-main.cpp:197-211, `twilight -f DIR -o out.aln`).
//
// Every file becomes a node whose profile is its column counts (readAlignment, io.cpp:200-238: alnNum = rows, alnWeight = (float)rows).
// The tree is a star (readAlignments_and_buildTree, io.cpp:240-299): the nodes sorted by row count, descending, the first one the root,
// the others its children.  scheduling mode 1 (progressive.cpp:81-95) pairs every child with the root, one pair per level;
// collectPostOrder (node.cpp:58-71) leaves the LAST child on top of the stack, so the last child is merged first.  Every pair is aligned
// profile against profile with currentTask 2 (alignment-cpu.cpp:86-130: gapCharScore 0, a failed pair retried until it passes), and no row is
// touched: what a merge changes is the column map of every file under its two sides (updateAlignment's subtreeAln branch,
// alignment-helper.cpp:402-423, :449-470).  All of it runs on one device:
//   all rows of all files -> one store; twl_store_count_columns per file -> its cached profile
//   per child: twl_level_prepare (two cached sides, no members) / twl_level_align / twl_level_restore, unchanged (include/twl_level.h)
//   twl_merge_apply           -> the maps of the files under both sides composed with the final path (include/twl_merge.h)
//   twl_level_commit_from_dp  -> the two cached profiles merged (updateFrequency, alignment-helper.cpp:506-539)
//   twl_merge_finish          -> every row rewritten through its file's map, once (io.cpp:355-449), read back once and written
// The output holds the files in sorted order with their rows in file order, which is what the reference's concatenation of its
// per-file outputs gives for names that sort alike.
// Two deliberate differences from the reference: a file whose rows differ in length is refused with exit 1 (the reference warns, leaves
// the row out of the profile and then miswrites it), and there is no temporary directory (-d, -k and -c are not part of this mode: the
// rows never leave the device between the merges).  A file without rows or without columns is refused as well.
#include "align_gpu.hpp"

#include "../../../include/twl_merge.h"
#include "../../../include/twl_place.h"

#include <algorithm>
#include <cstdio>
#include <filesystem>
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

struct MsaFile { std::string path; std::vector<std::string> names, rows; int32_t L = 0, firstId = 0; };

struct MergeTotals { double count = 0, finish = 0, read = 0, write = 0; progressive::gpu::MergeLevelTotals level; };

// the files' records in order; rows: all rows at W columns back to back, or nullptr for the rows as they were read
void writeRecords(const Option &option, const std::vector<MsaFile> &files, const char *rows, int32_t W)
{
    std::vector<const std::string *> names;
    std::vector<const char *> rowAt;
    for (const MsaFile &f : files)
        for (size_t r = 0; r < f.names.size(); ++r) {
            rowAt.push_back(rows ? rows + names.size() * (size_t)W : f.rows[r].data());
            names.push_back(&f.names[r]);
        }
    io::writeRecords(option.outFile, names, rowAt, W, &option);      // (no name is ever turned in a merge: --adjust-direction is refused with -f)
}

}  // namespace

namespace progressive {
namespace gpu {

// One level of merges of cached profiles (alignment-cpu.cpp:50-175 with currentTask 2), shared by the merge of a directory (runMerge below:
// a star, one pair per level) and the merge along the tree of subtrees (subtrees.cpp: levels of several pairs).  The level goes to the device
// as ONE level of n pairs: prepare with two cached sides and no members, DP with gapCharScore 0, gappy columns back, then twl_merge_apply over
// the groups under both sides of every pair and twl_level_commit_from_dp, which merges the two cached profiles into the reference side's.
// A failed pair is retried until it passes (alignment-cpu.cpp:95-128).  The level's one pair is retried in place.  In a level of several
// pairs the pairs that passed are finished first; every failed pair then becomes a level of its own, its first DP run already known (the DP
// of a pair does not depend on the level it runs in, and the pairs of a level share no node).  Returns the final path length of every pair.
std::vector<int32_t> mergeProfileLevel(twl_store *st, twl_merge *mg, int device, const twl_params &tp, Params &param, const Option &option,
                                       const std::vector<ProfilePair> &pairs, MergeLevelTotals &tot, const int16_t *knownErr)
{
    const int32_t n = (int32_t)pairs.size();
    std::vector<twl_side> sides;
    std::vector<int32_t> sideLen, refOff{0}, qryOff{0}, refGroups, qryGroups;
    int32_t maxLen = 1, stride = 1;
    for (const ProfilePair &p : pairs) {
        sides.push_back(twl_side{0, 0, p.refLen, p.refNum, p.refWeight, p.refCache, -1, 0});
        sides.push_back(twl_side{0, 0, p.qryLen, p.qryNum, p.qryWeight, p.qryCache, -1, 0});
        sideLen.push_back(p.refLen); sideLen.push_back(p.qryLen);
        maxLen = std::max(maxLen, std::max(p.refLen, p.qryLen));
        stride = std::max(stride, p.refLen + p.qryLen);
        refGroups.insert(refGroups.end(), p.refGroups.begin(), p.refGroups.end());
        qryGroups.insert(qryGroups.end(), p.qryGroups.begin(), p.qryGroups.end());
        refOff.push_back((int32_t)refGroups.size()); qryOff.push_back((int32_t)qryGroups.size());
    }
    std::vector<int32_t> lenOut(2 * (size_t)n, 0), alnLen((size_t)n, 0);
    std::vector<int16_t> err((size_t)n, 0);
    twl_params tz = tp;
    tz.gap_char = 0;                                       // alignment-cpu.cpp:88 (currentTask 2)
    int rc;
    double t0 = nowMs();
    if ((rc = twl_level_prepare(st, &tp, option.gappyVertical, n, sides.data(), nullptr, nullptr, maxLen, lenOut.data(), nullptr)) != TWL_OK) die("twl_level_prepare", rc);
    // alignment-cpu.cpp:95-128 with currentTask 2: retried until errorType 0
    alignWithRetry(st, device, tz, option, n == 1 ? &pairs[0].what : nullptr, n == 1 ? knownErr : nullptr, std::min(lenOut[0], lenOut[1]), alnLen.data(), err.data(), tot.run);
    tot.dp += nowMs() - t0;

    // gappy columns back (alignment-helper.cpp:324-375) when a side lost a column; otherwise the path is final as the DP left it
    t0 = nowMs();
    const AlignedLevel al{n, sideLen.data(), lenOut.data(), alnLen.data(), err.data(), maxLen, stride};
    const FinalPaths fin = finalPathsOfLevel(st, tp, param, option, al);
    tot.restoredOnHost += fin.restoredOnHost;
    tot.restore += nowMs() - t0;

    // the maps of the groups under both sides, then the two profiles (updateAlignment / updateFrequency, alignment-cpu.cpp:169-170)
    t0 = nowMs();
    if ((rc = twl_merge_apply(mg, st, n, refOff.data(), refGroups.data(), qryOff.data(), qryGroups.data(), nullptr, fin.pathLen.data(), stride, fin.fromDp.data())) != TWL_OK) die("twl_merge_apply", rc);
    tot.apply += nowMs() - t0;
    t0 = nowMs();
    if ((rc = twl_level_commit_from_dp(st, nullptr, fin.pathLen.data(), stride, fin.fromDp.data())) != TWL_OK) die("twl_level_commit_from_dp", rc);
    tot.commit += nowMs() - t0;
    std::vector<int32_t> pathLen = fin.pathLen;
    for (int32_t i = 0; i < n; ++i)
        if (err[i] != 0) pathLen[i] = mergeProfileLevel(st, mg, device, tp, param, option, {pairs[i]}, tot, &err[i])[0];
    return pathLen;
}

}  // namespace gpu
}  // namespace progressive

int runMerge(Option &option)
{
    namespace fs = std::filesystem;
    using progressive::gpu::ensureInit;
    using progressive::gpu::selectedDevices;
    MergeTotals tot;

    // ---- the files: every regular file under the directory, sorted by path (io.cpp:246-261) ----
    std::vector<std::string> paths;
    {
        std::error_code ec;
        if (!fs::is_directory(option.msaDir, ec)) { std::cerr << "ERROR: " << option.msaDir << " is not a directory.\n"; exit(1); }
        for (fs::recursive_directory_iterator it(option.msaDir, fs::directory_options::skip_permission_denied, ec), end; !ec && it != end; it.increment(ec))
            if (it->is_regular_file(ec)) paths.push_back(it->path().string());
        std::sort(paths.begin(), paths.end());
    }
    if (paths.empty()) { std::cerr << "ERROR: no alignment file was found under " << option.msaDir << ".\n"; exit(1); }
    if (!option.typeGiven) option.type = io::detectType(paths[0]);
    Params param(option, option.type);

    std::vector<MsaFile> files(paths.size());
    std::cerr << "====== Alignment Info ======\n";
    int32_t nRows = 0;
    for (size_t k = 0; k < paths.size(); ++k) {
        MsaFile &f = files[k];
        f.path = paths[k];
        f.firstId = nRows;
        f.L = io::readAlignedRows(f.path, "an alignment", f.names, f.rows);
        if (f.L < 0) { std::cerr << "ERROR: no rows were read from " << f.path << ".\n"; exit(1); }
        if (f.L == 0) { std::cerr << "ERROR: the rows of " << f.path << " have no columns.\n"; exit(1); }
        nRows += (int32_t)f.rows.size();
        std::cerr << '[' << k + 1 << '/' << paths.size() << "] " << fs::path(f.path).filename().string() << " (Count: " << f.rows.size() << ", Length: " << f.L << ")\n";
    }
    const int32_t G = (int32_t)files.size();
    if (G == 1 && option.trimRule >= 0) {      // nothing to merge, but columns to leave out: the file's rows through a store of their own (trim.cpp)
        std::vector<const char *> rowPtr;
        for (const std::string &r : files[0].rows) rowPtr.push_back(r.data());
        std::vector<char> rows;
        const int32_t kept = trimHostRows(option, rowPtr, files[0].L, [&](int32_t k) { return files[0].names[(size_t)k]; }, rows);
        writeRecords(option, files, rows.data(), kept);
        return kept;
    }
    if (G == 1) {      // nothing to merge: the file comes back as it is
        writeRecords(option, files, nullptr, files[0].L);
        return files[0].L;
    }

    // ---- one store: the rows of file k are the ids [firstId, firstId + rows); group k = file k, its cached profile has the id k ----
    ensureInit(&option);
    const int device = selectedDevices().empty() ? 0 : selectedDevices()[0];
    std::vector<const char *> rowPtr;
    std::vector<int32_t> rowLen, groupOff{0}, rowIds((size_t)nRows);
    for (const MsaFile &f : files) {
        for (const std::string &r : f.rows) { rowPtr.push_back(r.data()); rowLen.push_back(f.L); }
        groupOff.push_back((int32_t)rowPtr.size());
    }
    std::iota(rowIds.begin(), rowIds.end(), 0);
    twl_store *st = nullptr;
    int rc = twl_store_create(device, option.type, nRows, rowPtr.data(), rowLen.data(), &st);
    if (rc != TWL_OK) die("twl_store_create", rc);
    for (MsaFile &f : files) for (std::string &r : f.rows) std::string().swap(r);
    double t = nowMs();
    for (int32_t k = 0; k < G; ++k)
        if ((rc = twl_store_count_columns(st, groupOff[k + 1] - groupOff[k], rowIds.data() + groupOff[k], k)) != TWL_OK) die("twl_store_count_columns", rc);
    tot.count = nowMs() - t;
    twl_merge *mg = nullptr;
    if ((rc = twl_merge_create(st, G, groupOff.data(), rowIds.data(), &mg)) != TWL_OK) die("twl_merge_create", rc);

    // ---- the star: most rows first (a stable sort: ties keep the files' order, which the reference's std::sort leaves open) ----
    std::vector<int32_t> order((size_t)G);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return files[a].names.size() > files[b].names.size(); });
    const int32_t root = order[0];
    int32_t rootLen = files[root].L, rootNum = (int32_t)files[root].names.size();
    float rootWeight = (float)rootNum;
    std::vector<int32_t> rootGroups{root};

    const twl_params tp = baseParams(param);

    // ---- one level per child, the last child first ----
    for (int32_t at = G - 1; at >= 1; --at) {
        const int32_t child = order[at];
        const int32_t qLen = files[child].L, qNum = (int32_t)files[child].names.size();
        const float qWeight = (float)qNum;
        progressive::gpu::ProfilePair pr{root, child, rootLen, qLen, rootNum, qNum, rootWeight, qWeight, rootGroups, {child},
                                         "alignment " + fs::path(files[child].path).filename().string()};
        const int32_t pathLen = progressive::gpu::mergeProfileLevel(st, mg, device, tp, param, option, {pr}, tot.level)[0];
        // alignment-helper.cpp:474-477
        rootNum += qNum;
        rootLen = pathLen;
        rootWeight += qWeight;
        rootGroups.push_back(child);
        if (option.printDetail)
            std::cerr << "Merged " << fs::path(files[child].path).filename().string() << " (" << qNum << " rows, " << qLen << " columns): " << rootNum << " rows, " << rootLen << " columns\n";
    }

    // ---- every row through its file's map, once; one read-back; output ----
    int32_t W = 0;
    t = nowMs();
    if ((rc = twl_merge_finish(mg, &W)) != TWL_OK) die("twl_merge_finish", rc);
    tot.finish = nowMs() - t;
    t = nowMs();
    std::vector<int32_t> outLen((size_t)nRows);
    std::vector<char> rows;
    if (option.trimRule >= 0) {            // the rows lose their gappy columns on the device first (trim.cpp): W is the kept length from here on
        std::vector<const std::string *> nameOf;
        for (const MsaFile &f : files) for (const std::string &nm : f.names) nameOf.push_back(&nm);
        W = trimAndReadRows(option, st, nRows, rowIds.data(), [&](int32_t k) { return *nameOf[(size_t)k]; }, rows);
    } else {
        rows.resize((size_t)nRows * (size_t)W + 1);
        if ((rc = twl_store_read_rows_of(st, nRows, rowIds.data(), rows.data(), outLen.data())) != TWL_OK) die("twl_store_read_rows_of", rc);
    }
    tot.read = nowMs() - t;
    twl_merge_destroy(mg);
    twl_store_destroy(st);
    t = nowMs();
    writeRecords(option, files, rows.data(), W);
    tot.write = nowMs() - t;
    std::cerr << "Merged " << G << " alignments (" << nRows << " rows): final alignment length " << W << ", " << tot.level.run.retries << " retried DP run(s)\n";
    if (option.printDetail)
        fprintf(stderr, "Merge phases (ms): count %.3f, prepare+DP %.3f, restore %.3f, apply %.3f, commit %.3f, finish %.3f, read-back %.3f, write %.3f; "
                        "DP kernel %.3f ms, %llu band cells; restored on the host %d\n", tot.count, tot.level.dp, tot.level.restore, tot.level.apply, tot.level.commit, tot.finish, tot.read, tot.write,
                tot.level.run.kernel, (unsigned long long)tot.level.run.cells, tot.level.restoredOnHost);
    return W;
}

}  // namespace msa
