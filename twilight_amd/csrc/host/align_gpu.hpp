// twilight_amd/csrc/host/align_gpu.hpp -- shared by the two level kernels (align_gpu.cpp: host-staged, align_resident.cpp: device-resident).
#pragma once
#include "twl_host.hpp"

#include "../../../include/twl_align.h"
#include "../../../include/twl_level.h"

#include <chrono>

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
inline double nowMs() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace gpu
}  // namespace progressive
}  // namespace msa
