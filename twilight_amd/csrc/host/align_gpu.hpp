// twilight_amd/csrc/host/align_gpu.hpp -- shared by the two level kernels (align_gpu.cpp: host-staged, align_resident.cpp: device-resident).
#pragma once
#include "twl_host.hpp"

#include "../../../include/twl_align.h"
#include "../../../include/twl_level.h"

struct twl_merge;

#include <chrono>
#include <functional>

namespace msa {
namespace progressive {
namespace gpu {

void ensureInit(Option *option);

struct RunCtx {
    std::vector<twl_store *> stores;      // device-resident mode: one replica per device (or per virtual device in tests)
    std::vector<int> storeDev;
    bool finished = false;                         // the main pass is over: rows are back on the host
    int nextCacheId = 0;
    LevelTotals totals;
    std::vector<LevelRecord> levels;
    Shard shard;
    std::function<void(twl_store *)> onStoreCreated;      // createStore calls it once per replica, behind the upload and ahead of the first level, then forgets it (place_tree.cpp squeezes the backbone's groups there)
    struct Raw { char *p = nullptr; size_t cap = 0; bool pinned = false; char *get(size_t n); ~Raw(); Raw() = default; Raw(Raw &&o) noexcept : p(o.p), cap(o.cap), pinned(o.pinned) { o.p = nullptr; o.cap = 0; } Raw(const Raw &) = delete; };      // grow-only, never zero-filled host buffer
    ~RunCtx();
};
// (the level policy both kernels follow -- which pairs go to the DP, retry, defer, the deal of the pairs to owners -- is level_policy.hpp)
[[noreturn]] void die(const char *what, int rc);      // "ERROR: <what> failed (<rc>): <twl_last_error()>", exit 1
void refuseCpuOnly(Option *option);                   // --cpu-only ends the run: there is no CPU alignment path
// What one twl_stats (a device's last DP call) adds to a level's record: cells, relaunched pairs, tile counts, and once the kernel's
// identity.  The times stay with the caller: devices run concurrently, so they combine by max, not by sum.
void foldStats(LevelRecord &rec, const twl_stats &st);
// The end of a level in both kernels: the deferred pairs join the failed ones and go to fallback2cpu, the record gets the level's time
// and joins the run's totals and records.  (Each kernel prints its own -v "phases" line after it.)
void closeLevel(RunCtx &ctx, LevelRecord &rec, double tStart, const std::vector<char> &deferred, std::vector<int> &fallbackPairs, NodePairVec &nodes,
                SequenceDB *database, Option *option);
// All-gather of the paths the ranks aligned: on return paths/errs hold every pair of the level on every rank.
void exchangePaths(RunCtx &ctx, const std::vector<int> &owner, const std::vector<char> &takesPart, int pathCap, std::vector<alnPath> &paths,
                   std::vector<int16_t> &errs, LevelRecord &rec);
// The same for the device-resident level kernel when the processes can all-gather DEVICE blocks (Shard::exchangeDev): every rank's final
// paths (gappy columns already restored, in the store's path buffer / DP output) are packed into one device block, all-gathered, and the
// other ranks' paths unpacked into their rows of the path buffer -- HBM to HBM, one collective per level.  bound[i] = refLen + qryLen of
// pair i before removal (every rank knows it: the block size is agreed on without a collective).  On return fromDp / dpLen / errs describe
// every pair of the level on every rank (fromDp 2 = row in the path buffer).
void exchangeFinalPaths(RunCtx &ctx, twl_store *store, int device, const twl_params &tp, const std::vector<int> &owner, const std::vector<char> &takesPart,
                        const std::vector<int32_t> &bound, int pathStride, std::vector<uint8_t> &fromDp, std::vector<int32_t> &dpLen, std::vector<int16_t> &errs,
                        LevelRecord &rec);
const std::vector<int> &selectedDevices();
twl_params baseParams(Params &param);          // == Talco_xdrop::Params(msa::Params&), TALCO-XDrop.cpp:36-53
// Consensus string and removed-column runs of one side from the column info of twl_level_prepare (letters: "ACGTN" / the 20 acids + 'X').
void runsAndConsensus(const uint8_t *info, int len, bool removal, const char *letters, IntPairVec &runs, std::string &cons);
const char *consensusLetters(char type);       // the letter of a column-info code, for runsAndConsensus
// Column info of one pair for addGappyColumnsBack: removed-column runs and consensus of the two sides.
struct ColumnInfo { std::pair<IntPairVec, IntPairVec> gappy; stringPair consensus; };
// Gappy columns back on the host for one pair (alignment-helper.cpp:324-375): `full` from its DP path.  Returns the codes != 1 and != 2 of
// `full`; a path longer than the row pitch of the final paths ends the run.
IntPair restoreOnHost(alnPath &dp, ColumnInfo &cols, Params &param, int pathStride, alnPath &full);

// The n pairs of a store's prepared and aligned level: sideLen / lenOut [2n] = length of every side before / after gappy-column removal,
// alnLen / err [n] = what the DP left, stride / pathStride = row pitch of the level (its longest side) and of its final paths.
struct AlignedLevel { int32_t n; const int32_t *sideLen, *lenOut, *alnLen; const int16_t *err; int32_t stride, pathStride; };
// (rare: a two-sided run too large for the device) the pairs twl_level_restore handed back: their column info and DP paths (dpLen codes) come
// to the host, the host puts the columns back and writes the result into the level's path buffer.  Returns the final length of each;
// post(pair, codes != 1, codes != 2), if given, sees every restored path.
std::vector<int32_t> restoreHandedBack(twl_store *st, Params &param, const Option &option, const AlignedLevel &lv, const std::vector<int32_t> &pairs,
                                       const std::vector<int32_t> &dpLen, const std::function<void(int, int, int)> &post = nullptr);
// The final path of every pair with err == 0, all in HBM: as the DP left it (fromDp 1) when no column was removed, otherwise with its gappy
// columns back (fromDp 2: twl_level_restore, or restoreHandedBack for the pairs it hands back).
struct FinalPaths { std::vector<uint8_t> fromDp; std::vector<int32_t> pathLen; int restoredOnHost = 0; };
FinalPaths finalPathsOfLevel(twl_store *st, const twl_params &tp, Params &param, const Option &option, const AlignedLevel &lv);
// twl_level_align over the store's prepared level, the device's stats added to `tot`; with retryWhat, the level's ONE pair is retried until it
// passes (alignment-cpu.cpp:95-128 with currentTask != 0; -v: "Retry <retryWhat> ...").  knownErr: that pair's DP has run already and ended
// with *knownErr.  minLen: its shorter side after gappy-column removal.
struct DpTotals { double kernel = 0; uint64_t cells = 0; int retries = 0; };
void alignWithRetry(twl_store *st, int device, const twl_params &prm, const Option &option, const std::string *retryWhat, const int16_t *knownErr, int32_t minLen,
                    int32_t *alnLen, int16_t *err, DpTotals &tot);
// One pair of a level of merges of cached profiles (merge.cpp): the cache ids of its two sides with their Node bookkeeping (alnLen, alnNum,
// alnWeight), the groups of the merge under each side, and what a -v retry line calls the pair.
struct ProfilePair { int32_t refCache, qryCache, refLen, qryLen, refNum, qryNum; float refWeight, qryWeight; std::vector<int32_t> refGroups, qryGroups; std::string what; };
struct MergeLevelTotals { double dp = 0, restore = 0, apply = 0, commit = 0; DpTotals run; int restoredOnHost = 0; };
std::vector<int32_t> mergeProfileLevel(twl_store *st, twl_merge *mg, int device, const twl_params &tp, Params &param, const Option &option,
                                       const std::vector<ProfilePair> &pairs, MergeLevelTotals &tot, const int16_t *knownErr = nullptr);
inline double nowMs() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace gpu
}  // namespace progressive

// ---- --trim-gappy / --trim-to (trim.cpp; include/twl_trim.h): the rows that are written lose their gappy columns on the device ----
// One decision for every mode: twl_store_trim_columns over the n rows `ids` of a store, which are the rows that are written, in that order
// (writtenName(k): the name row k is written under).  Either on the run's own store, between its last kernel and its read-back (resident), or
// on a store made for it from the final host rows.  Ends the run, before any file is written, when --trim-to names no written row or no column is kept;
// writes --write-columns.  What it returns goes to reportTrim once the trimmed rows are on the host (rowAt(k): the kept bytes of row k).
struct TrimReport { int32_t W = 0, kept = 0, rows = 0, limit = 0; double kernelMs = 0; bool resident = true; };
TrimReport trimStoreRows(const Option &option, twl_store *st, int32_t n, const int32_t *ids, const std::function<std::string(int32_t)> &writtenName, bool resident);
void reportTrim(const Option &option, const TrimReport &r, const std::function<const char *(int32_t)> &rowAt);
// ... and the read-back of those rows behind it (merge.cpp, subtrees.cpp, place.cpp): rows = the n trimmed rows back to back.  Returns the kept length.
int32_t trimAndReadRows(const Option &option, twl_store *st, int32_t n, const int32_t *ids, const std::function<std::string(int32_t)> &writtenName, std::vector<char> &rows);
// Rows that exist on the host only (n rows of W bytes): uploaded into a store of their own, trimmed there, read back into `out` back to back.  Returns the kept length.
int32_t trimHostRows(Option &option, const std::vector<const char *> &rows, int32_t W, const std::function<std::string(int32_t)> &writtenName, std::vector<char> &out);
// The same for the finished rows of a SequenceDB (what writeAlignment writes: the sequences that are not low-quality): trimmed in place.  Returns the kept length.
int trimDatabaseRows(SequenceDB *database, Option *option, int alnLen);
// The name a sequence of option.seqFile is written under: _R_<name> where --adjust-direction turned it.
inline std::string writtenNameOf(const Option &option, const std::string &name) { return (option.reversedNames.count(name) ? "_R_" : "") + name; }

}  // namespace msa
