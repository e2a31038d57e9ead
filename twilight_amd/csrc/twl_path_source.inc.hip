// twilight_amd/csrc/twl_path_source.inc.hip -- where the final path of a pair lives when a call takes it (twl_place_collect, twl_merge_apply), as PURE
// functions of the call's arguments: from_dp 0 = a host row the call uploads, 1 = the level's DP output (row pitch 2 * seq_len), 2 = the level's
// path buffer as twl_level_restore staged it (row pitch path_stride).  No HIP call and no global in this file: tests/place_plan_kats.cpp and
// tests/merge_plan_kats.cpp include it through the plans.  Included by twl_place_plan.inc.hip and twl_merge_plan.inc.hip (one translation unit).
#pragma once
#include <cstdint>
#include <vector>

// What a taking call needs to know of the store's level (from_dp != NULL reads its buffers).
struct PathLevelView {
    bool prepared = false;       // a level is prepared and holds its buffers
    int32_t n_pairs = 0;
    int64_t dp_stride = 0;       // row pitch of the DP output (2 * seq_len)
    bool has_dp = false;         // the DP output exists
    int32_t staged_stride = 0;   // > 0: twl_level_restore staged the paths at this pitch
};

// The source tables of the taking pairs of one call, in order (what twl::PathSrc reads on the device).
struct PathSources {
    std::vector<uint8_t> which;          // per taking pair: 0 host row, 1 DP output, 2 path buffer
    std::vector<int64_t> srcOff;         // per taking pair: offset of its path in that source
    std::vector<int32_t> hostRows;       // pairs whose path comes from the host, in upload order
};

// A call with from_dp reads the level of exactly its pairs: the message, or nullptr.
inline const char *check_path_level(const uint8_t *from_dp, int32_t n_pairs, const PathLevelView &lv)
{
    if (from_dp && (!lv.prepared || lv.n_pairs != n_pairs)) return "from_dp needs the prepared and aligned level of these pairs";
    return nullptr;
}

// Pair i of the call takes part with a path of n codes: the message, or nullptr with the pair appended to `src`.
inline const char *add_path_source(PathSources &src, int32_t i, int32_t n, const uint8_t *from_dp, bool havePaths, int32_t path_stride, const PathLevelView &lv)
{
    const int w = from_dp ? from_dp[i] : 0;
    if (w > 2) return "from_dp must be 0, 1 or 2";
    if (w == 1 && ((int64_t)n > lv.dp_stride || !lv.has_dp)) return "from_dp 1 without a DP output of that length";
    if (w == 2 && (!lv.staged_stride || lv.staged_stride != path_stride)) return "from_dp 2: twl_level_restore first, with this row pitch";
    if (w == 0 && !havePaths) return "host rows missing";
    src.which.push_back((uint8_t)w);
    if (w == 0) { src.srcOff.push_back((int64_t)src.hostRows.size() * path_stride); src.hostRows.push_back(i); }
    else src.srcOff.push_back((int64_t)i * (w == 1 ? lv.dp_stride : (int64_t)path_stride));
    return nullptr;
}
