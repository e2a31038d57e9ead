// twilight_amd/csrc/twl_guide_set_plan.inc.hip -- what the twl_guide_set_* calls (include/twl_guide.h) decide on the host, as
// PURE functions of the calls' arguments: everything they reject, and the tile list of twl_guide_set_shared_groups.  No HIP call and no
// global in this file: tests/guide_set_plan_kats.cpp includes it directly.  Included by twl_guide_set.inc.hip (one translation unit).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>
#include "twl_guide_plan.inc.hip"

constexpr int32_t kGuideSetMaxSeqs = 1048576;               // TWL_GUIDE_SET_MAX_SEQS
constexpr uint64_t kGuideGroupsMaxWords = 1ull << 28;       // the sum of m_g^2 of one twl_guide_set_shared_groups: the 1 GiB of the one-stage matrix

// twl_guide_set_create: the message, or nullptr with *total the letters of all sequences
inline const char *check_guide_set_create(char type, int32_t n, const char *const *seqs, const int32_t *lens, const void *set_out, uint64_t *total)
{
    if (guide_bins(type) == 0) return "the type must be 'n' or 'p'";
    if (n < 1) return "no sequences";
    if (n > kGuideSetMaxSeqs) return "more than 1048576 sequences in a set";
    if (!seqs || !lens || !set_out) return "bad argument";
    uint64_t sum = 0;
    for (int32_t i = 0; i < n; ++i) {
        if (lens[i] < 0) return "negative sequence length";
        if (lens[i] > 0 && !seqs[i]) return "bad argument";
        sum += (uint64_t)lens[i];
    }
    if (total) *total = sum;
    return nullptr;
}

// twl_guide_set_assign on a set of n sequences (has_set: the handle is not null); shared_out may be null
inline const char *check_guide_set_assign(bool has_set, int32_t n, int32_t n_seeds, const int32_t *seed_ids, const void *seed_out)
{
    if (!has_set || !seed_ids || !seed_out) return "bad argument";
    if (n_seeds < 1 || n_seeds > kGuideMaxSeqs) return "the number of seeds must be between 1 and 16384";
    std::vector<bool> seen((size_t)n, false);
    for (int32_t t = 0; t < n_seeds; ++t) {
        if (seed_ids[t] < 0 || seed_ids[t] >= n) return "seed id out of range";
        if (seen[(size_t)seed_ids[t]]) return "the same sequence is a seed twice";
        seen[(size_t)seed_ids[t]] = true;
    }
    return nullptr;
}

// twl_guide_set_shared_groups on a set of n sequences: the message, or nullptr with *words the sum of m_g^2 (the size of `out`)
inline const char *check_guide_set_groups(bool has_set, int32_t n, int32_t n_groups, const int32_t *group_off, const int32_t *ids, const void *out, uint64_t *words)
{
    if (!has_set || !group_off || !ids || !out) return "bad argument";
    if (n_groups < 1) return "no groups";
    if (n_groups > kGuideSetMaxSeqs) return "more than 1048576 groups";
    if (group_off[0] != 0) return "the first group must start at 0";
    uint64_t sum = 0;
    for (int32_t g = 0; g < n_groups; ++g) {
        if (group_off[g + 1] < group_off[g]) return "the group offsets decrease";
        const int64_t m = (int64_t)group_off[g + 1] - group_off[g];
        if (m == 0) return "an empty group";
        if (m > kGuideMaxSeqs) return "a group of more than 16384 sequences";
        sum += (uint64_t)m * (uint64_t)m;
        if (sum > kGuideGroupsMaxWords) return "the groups' matrices hold more than 2^28 entries together";
    }
    for (int32_t k = 0; k < group_off[n_groups]; ++k)
        if (ids[k] < 0 || ids[k] >= n) return "sequence id out of range";
    if (words) *words = sum;
    return nullptr;
}

// One tile of one group's matrix, as guide_groups_kernel takes it (twl::GuideGroupTile has the same members): the tile (ti, tj), ti <= tj, of
// the group of rows ids[first .. first + m), whose m x m block starts `block` entries into the output.
struct GuideGroupTilePlan {
    int32_t first, m, ti, tj;
    unsigned long long block;
};

// The tiles of `tile` x `tile` pairs on or above the diagonal of every group's block, group by group, row of tiles by row of tiles.
// Block g starts at the sum of m_h^2 over the groups h < g.  The arguments have passed check_guide_set_groups.
inline std::vector<GuideGroupTilePlan> plan_guide_groups(int32_t n_groups, const int32_t *group_off, int32_t tile)
{
    std::vector<GuideGroupTilePlan> tiles;
    unsigned long long block = 0;
    for (int32_t g = 0; g < n_groups; ++g) {
        const int32_t m = group_off[g + 1] - group_off[g], T = (m + tile - 1) / tile;
        for (int32_t ti = 0; ti < T; ++ti)
            for (int32_t tj = ti; tj < T; ++tj) tiles.push_back(GuideGroupTilePlan{group_off[g], m, ti, tj, block});
        block += (unsigned long long)m * (unsigned long long)m;
    }
    return tiles;
}
