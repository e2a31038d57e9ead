// twilight_amd/csrc/host/trim.cpp -- `--trim-gappy T`, `--trim-to NAME`, `--write-columns FILE`: the alignment written without its gappy columns
// (DESIGN.md section 4m).  Every mode ends with its rows in a store; the rows that are written lose their columns there, by ONE call
// (twl_store_trim_columns, include/twl_trim.h), in front of the read-back, so that only kept columns cross to the host and reach the file:
//
//   merge.cpp, subtrees.cpp, place.cpp   trimAndReadRows between the finish call and the write
//   the default flow, --place-on-tree    Option::trimResidentRows in the download that is the run's last (align_resident.cpp, materialise)
//   final rows that exist on the host    trimHostRows / trimDatabaseRows: a store made for them, the same call (--check, compressed groups, a run that left the device)
//
// N, the number of rows, is the number of rows written; --trim-gappy keeps the columns with at most floor(T * N) gaps (retree_max_gaps, in double).
#include "align_gpu.hpp"

#include "../../../include/twl_trim.h"
#include "../twl_retree_plan.inc.hip"      // (pure) retree_max_gaps

#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <numeric>

namespace msa {

using progressive::gpu::die;
using progressive::gpu::nowMs;

TrimReport trimStoreRows(const Option &option, twl_store *st, int32_t n, const int32_t *ids, const std::function<std::string(int32_t)> &writtenName, bool resident)
{
    TrimReport r;
    r.rows = n;
    r.resident = resident;
    int32_t arg = 0;
    if (option.trimRule == TWL_TRIM_TO_ROW) {
        int32_t at = -1;
        for (int32_t k = 0; k < n && at < 0; ++k) if (writtenName(k) == option.trimToName) at = k;
        if (at < 0) { std::cerr << "ERROR: --trim-to: no written row is called " << option.trimToName << ".\n"; exit(1); }
        arg = ids[at];
    } else {
        r.limit = retree_max_gaps(option.trimGappy, n);
        arg = r.limit;
    }
    std::vector<int32_t> lens((size_t)n);
    int rc = twl_store_read_rows_of(st, n, ids, nullptr, lens.data());
    if (rc != TWL_OK) die("twl_store_read_rows_of", rc);
    r.W = n > 0 ? lens[0] : 0;
    if ((rc = twl_store_trim_columns(st, n, ids, option.trimRule, arg, &r.kept)) != TWL_OK) die("twl_store_trim_columns", rc);
    if (r.kept < 1) {
        std::cerr << "ERROR: no column is kept: ";
        if (option.trimRule == TWL_TRIM_TO_ROW) std::cerr << "the row " << option.trimToName << " holds '-' in all " << r.W << " columns.\n";
        else std::cerr << "each of the " << r.W << " columns has more than " << r.limit << " gaps in " << n << " rows (--trim-gappy " << option.trimGappy << ").\n";
        exit(1);
    }
    (void)twl_store_trim_timing(st, &r.kernelMs);
    if (!option.writeColumnsFile.empty()) {
        std::vector<int32_t> cols((size_t)r.kept);
        std::vector<uint32_t> gaps((size_t)r.W);
        if ((rc = twl_store_trim_read(st, cols.data(), gaps.data())) != TWL_OK) die("twl_store_trim_read", rc);
        std::ofstream out(option.writeColumnsFile, std::ios::binary);
        if (!out) { std::cerr << "ERROR: Failed to open file: " << option.writeColumnsFile << '\n'; exit(1); }
        std::string text;
        for (int32_t k = 0; k < r.kept; ++k) text += std::to_string(k) + '\t' + std::to_string(cols[k]) + '\t' + std::to_string(gaps[cols[k]]) + '\n';
        out << text;
        out.close();
        if (!out) { std::cerr << "ERROR: Failed to write file: " << option.writeColumnsFile << '\n'; exit(1); }
    }
    return r;
}

void reportTrim(const Option &option, const TrimReport &r, const std::function<const char *(int32_t)> &rowAt)
{
    int64_t allGap = 0;
#pragma omp parallel for schedule(static) reduction(+ : allGap)
    for (int32_t k = 0; k < r.rows; ++k) {
        const char *row = rowAt(k);
        bool any = false;
        for (int32_t j = 0; j < r.kept && !any; ++j) any = row[j] != '-';
        allGap += any ? 0 : 1;
    }
    std::cerr << "Trimmed the alignment: " << r.kept << " of " << r.W << " columns kept (";
    if (option.trimRule == TWL_TRIM_TO_ROW) std::cerr << "--trim-to " << option.trimToName << ": the columns of that row";
    else std::cerr << "--trim-gappy " << option.trimGappy << ": at most " << r.limit << " gaps in " << r.rows << " rows";
    std::cerr << "); " << allGap << " row(s) became all '-'\n";
    if (option.printDetail)
        fprintf(stderr, "Trim kernels %.3f ms on %s\n", r.kernelMs, r.resident ? "the resident rows" : "an uploaded copy of the final rows");
}

int32_t trimAndReadRows(const Option &option, twl_store *st, int32_t n, const int32_t *ids, const std::function<std::string(int32_t)> &writtenName, std::vector<char> &rows)
{
    const TrimReport r = trimStoreRows(option, st, n, ids, writtenName, true);
    std::vector<int32_t> outLen((size_t)n);
    rows.assign((size_t)n * (size_t)r.kept + 1, 0);
    const int rc = twl_store_read_rows_of(st, n, ids, rows.data(), outLen.data());
    if (rc != TWL_OK) die("twl_store_read_rows_of", rc);
    reportTrim(option, r, [&](int32_t k) { return rows.data() + (size_t)k * (size_t)r.kept; });
    return r.kept;
}

int32_t trimHostRows(Option &option, const std::vector<const char *> &rows, int32_t W, const std::function<std::string(int32_t)> &writtenName, std::vector<char> &out)
{
    progressive::gpu::ensureInit(&option);
    const int device = progressive::gpu::selectedDevices().empty() ? 0 : progressive::gpu::selectedDevices()[0];
    const int32_t n = (int32_t)rows.size();
    std::vector<int32_t> lens((size_t)n, W), ids((size_t)n);
    std::iota(ids.begin(), ids.end(), 0);
    twl_store *st = nullptr;
    int rc = twl_store_create(device, option.type, n, rows.data(), lens.data(), &st);
    if (rc != TWL_OK) die("twl_store_create", rc);
    const TrimReport r = trimStoreRows(option, st, n, ids.data(), writtenName, false);
    out.assign((size_t)n * (size_t)r.kept + 1, 0);
    if ((rc = twl_store_read_rows_of(st, n, ids.data(), out.data(), lens.data())) != TWL_OK) die("twl_store_read_rows_of", rc);
    twl_store_destroy(st);
    reportTrim(option, r, [&](int32_t k) { return out.data() + (size_t)k * (size_t)r.kept; });
    return r.kept;
}

namespace {
// the sequences of a database that are written, in the order they are written (io::writeAlignment)
std::vector<SequenceDB::SequenceInfo *> writtenSequences(SequenceDB *database)
{
    std::vector<SequenceDB::SequenceInfo *> w;
    for (auto *s : database->sequences) if (!s->lowQuality) w.push_back(s);
    return w;
}
}  // namespace

int trimDatabaseRows(SequenceDB *database, Option *option, int alnLen)
{
    const std::vector<SequenceDB::SequenceInfo *> w = writtenSequences(database);
    if (w.empty()) { std::cerr << "ERROR: no row is written: nothing to trim.\n"; exit(1); }
    std::vector<const char *> rows;
    for (const auto *s : w) rows.push_back(s->alnStorage[s->storage]);
    std::vector<char> out;
    const int32_t kept = trimHostRows(*option, rows, alnLen, [&](int32_t k) { return writtenNameOf(*option, w[(size_t)k]->name); }, out);
    for (size_t k = 0; k < w.size(); ++k) { memcpy(w[k]->alnStorage[w[k]->storage], out.data() + k * (size_t)kept, (size_t)kept); w[k]->len = kept; }
    return kept;
}

// Option::trimResidentRows of the binaries that carry the trim: the written rows of the run's own store, in front of the last download
std::function<void()> trimResidentDatabaseRows(SequenceDB *database, Option *option, void *store)
{
    const std::vector<SequenceDB::SequenceInfo *> w = writtenSequences(database);
    if (w.empty()) return nullptr;
    std::vector<int32_t> ids;                      // (sequence i of the database is row i of its store)
    for (size_t i = 0; i < database->sequences.size(); ++i) if (!database->sequences[i]->lowQuality) ids.push_back((int32_t)i);
    const TrimReport r = trimStoreRows(*option, static_cast<twl_store *>(store), (int32_t)ids.size(), ids.data(), [&](int32_t k) { return writtenNameOf(*option, w[(size_t)k]->name); }, true);
    database->trimmedLen = r.kept;
    const Option *opt = option;
    return [opt, r, w]() { reportTrim(*opt, r, [&](int32_t k) { return (const char *)w[(size_t)k]->alnStorage[w[(size_t)k]->storage]; }); };
}

void enableTrim(Option &option)
{
    if (option.trimRule < 0) return;
    option.trimHostRows = trimDatabaseRows;
    option.trimResidentRows = trimResidentDatabaseRows;
}

}  // namespace msa
