// twilight_amd/csrc/twl_retree_set_plan.inc.hip -- what the twl_retree_set_* calls (include/twl_retree_set.h) decide on the host,
// as PURE functions of the calls' arguments: everything they reject, the slabs of rows that the pack launches and the staging take, and the bytes
// a set needs.  No HIP call and no global in this file: tests/retree_set_plan_kats.cpp includes it directly.  Included by twl_retree_set.inc.hip
// (one translation unit).  The tile list of twl_retree_set_pair_groups is plan_guide_groups of twl_guide_set_plan.inc.hip, unchanged: the blocks
// of both calls are laid out alike.
//
// Every index a kernel of retree_stage_kernels.hip.h gathers through passes through here: a seed id, a row id and a group offset that this file
// lets through is read on the device without a further check.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>
#include "twl_guide_set_plan.inc.hip"
#include "twl_retree_plan.inc.hip"

constexpr int32_t kRetreeSetMaxSeqs = 1048576;               // TWL_RETREE_SET_MAX_SEQS
constexpr int32_t kRetreeSetMaxSeeds = 16384;                // seeds of one assign call, and rows of one group: the one-stage cap
constexpr uint64_t kRetreeGroupsMaxWords = 1ull << 28;       // the sum of m_g^2 of one twl_retree_set_pair_groups, per matrix: 1 GiB
constexpr int32_t kRetreePackMaxRows = 65535;                // retree_pack_kernel takes its row from blockIdx.y: rows of one launch
constexpr uint64_t kRetreeStageBytes = 64ull << 20;          // the host block the rows are staged through on their way to the device

// twl_retree_set_create: what check_retree_pairs refuses, with the cap of a set
inline const char *check_retree_set_create(char type, int32_t n, int32_t width, const char *const *rows, int32_t max_gaps, const void *set_out, const void *kept_out)
{
    if (retree_planes(type) == 0) return "the type must be 'n' or 'p'";
    if (n < 1) return "no rows";
    if (n > kRetreeSetMaxSeqs) return "more than 1048576 rows in a set";
    if (width < 1) return "the rows have no columns";
    if (!rows) return "bad argument";
    for (int32_t i = 0; i < n; ++i)
        if (!rows[i]) return "bad argument";
    if (max_gaps < 0 || max_gaps > n) return "max_gaps must lie in 0 .. n";
    if (!set_out || !kept_out) return "bad argument";
    return nullptr;
}

// twl_retree_set_assign on a set of n rows (has_set: the handle is not null); match_out and both_out may be null
inline const char *check_retree_set_assign(bool has_set, int32_t n, int32_t n_seeds, const int32_t *seed_ids, const void *seed_out)
{
    if (!has_set || !seed_ids || !seed_out) return "bad argument";
    if (n_seeds < 1 || n_seeds > kRetreeSetMaxSeeds) return "the number of seeds must be between 1 and 16384";
    std::vector<bool> seen((size_t)n, false);
    for (int32_t t = 0; t < n_seeds; ++t) {
        if (seed_ids[t] < 0 || seed_ids[t] >= n) return "seed id out of range";
        if (seen[(size_t)seed_ids[t]]) return "the same row is a seed twice";
        seen[(size_t)seed_ids[t]] = true;
    }
    return nullptr;
}

// twl_retree_set_pair_groups on a set of n rows: the message, or nullptr with *words the sum of m_g^2 (the size of each output)
inline const char *check_retree_set_groups(bool has_set, int32_t n, int32_t n_groups, const int32_t *group_off, const int32_t *ids, const void *match_out, const void *both_out,
                                           uint64_t *words)
{
    if (!has_set || !group_off || !ids || !match_out || !both_out) return "bad argument";
    if (n_groups < 1) return "no groups";
    if (n_groups > kRetreeSetMaxSeqs) return "more than 1048576 groups";
    if (group_off[0] != 0) return "the first group must start at 0";
    uint64_t sum = 0;
    for (int32_t g = 0; g < n_groups; ++g) {
        if (group_off[g + 1] < group_off[g]) return "the group offsets decrease";
        const int64_t m = (int64_t)group_off[g + 1] - group_off[g];
        if (m == 0) return "an empty group";
        if (m > kRetreeSetMaxSeeds) return "a group of more than 16384 rows";
        sum += (uint64_t)m * (uint64_t)m;
        if (sum > kRetreeGroupsMaxWords) return "the groups' matrices hold more than 2^28 entries each";
    }
    for (int32_t k = 0; k < group_off[n_groups]; ++k)
        if (ids[k] < 0 || ids[k] >= n) return "row id out of range";
    if (words) *words = sum;
    return nullptr;
}

// The rows [first, first + count) of slab s when n rows are taken at most max_rows at a time; retree_slabs(n, max_rows) of them cover the rows
// exactly once, in order.
inline int32_t retree_slabs(int32_t n, int32_t max_rows) { return (int32_t)(((int64_t)n + max_rows - 1) / max_rows); }
inline void retree_slab(int32_t n, int32_t max_rows, int32_t s, int32_t *first, int32_t *count)
{
    const int64_t f = (int64_t)s * max_rows;
    *first = (int32_t)f;
    *count = (int32_t)(f + max_rows <= n ? max_rows : n - f);
}

// rows of one staged host block: as many as fit kRetreeStageBytes, at least one, at most all
inline int32_t retree_stage_rows(int32_t n, int32_t width)
{
    const uint64_t fit = kRetreeStageBytes / (uint64_t)width;
    return (int32_t)(fit < 1 ? 1 : fit > (uint64_t)n ? (uint64_t)n : fit);
}

// device bytes while a set is made (the rows and the gap counts leave again) and of the set that stays: the planes and the letters of every row
inline uint64_t retree_set_stay_bytes(char type, int32_t n, int64_t words_pad) { return (uint64_t)n * (uint64_t)retree_planes(type) * (uint64_t)words_pad * 8 + (uint64_t)n * 4; }
inline uint64_t retree_set_create_bytes(char type, int32_t n, int32_t width, int64_t words_pad)
{
    return (uint64_t)n * (uint64_t)width + (uint64_t)width * 4 + retree_set_stay_bytes(type, n, words_pad);
}
