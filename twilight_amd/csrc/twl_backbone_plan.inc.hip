// twilight_amd/csrc/twl_backbone_plan.inc.hip -- what twl_store_squeeze_groups (include/twl_backbone.h) decides on the host, as PURE functions of
// the call's arguments and of the store's bookkeeping: everything the call rejects, and the tile list its first kernel runs over.  No HIP
// call and no global in this file: tests/backbone_plan_kats.cpp includes it directly.  Included by twl_backbone.inc.hip (one translation unit).
#pragma once
#include <cstdint>
#include <vector>

// One entry of the tile list of squeeze_flags_kernel (the layout of twl::SqueezeTile, backbone_kernels.hip.h): columns [col0, col0 + colTile)
// of the rows ids[row0, row1) of group `group`.
struct SqueezeTilePlan { int32_t group, col0, row0, row1; };

// The groups of a call as its kernels address them.
struct SqueezeGroups {
    std::vector<int32_t> len;          // [n_groups] the one row length of every group
    std::vector<int64_t> flagOff;      // [n_groups] first keep word of the group (ceil(len / 32) words each)
    std::vector<int64_t> preOff;       // [n_groups] first scan entry of the group (one per word and one behind them)
    std::vector<int32_t> rowGroup;     // [n_rows] group of every listed row
    int64_t flagWords = 0, preInts = 0;
    int32_t maxLen = 0;
};

// Everything twl_store_squeeze_groups rejects: the message, or nullptr with `g` filled in.  row_len[q]: current row length of sequence q.
inline const char *check_squeeze_groups(int32_t n_groups, const int32_t *group_off, const int32_t *ids, bool haveLenOut, int32_t n_seqs, const int32_t *row_len,
                                        bool levelPrepared, SqueezeGroups &g)
{
    g = SqueezeGroups{};
    if (n_groups < 0) return "bad argument";
    if (levelPrepared) return "a level is still prepared on the store: commit it first";
    if (n_groups == 0) return nullptr;
    if (!group_off || !ids || !haveLenOut) return "bad argument";
    if (group_off[0] != 0) return "group offsets must start at 0";
    for (int32_t k = 0; k < n_groups; ++k) {
        if (group_off[k + 1] < group_off[k]) return "group offsets do not ascend";
        if (group_off[k + 1] == group_off[k]) return "an empty group";
    }
    std::vector<uint8_t> seen((size_t)n_seqs, 0);
    g.rowGroup.resize((size_t)group_off[n_groups]);
    for (int32_t k = 0; k < n_groups; ++k) {
        int32_t L = -1;
        for (int32_t t = group_off[k]; t < group_off[k + 1]; ++t) {
            const int32_t id = ids[t];
            if (id < 0 || id >= n_seqs) return "sequence id out of range";
            if (seen[id]) return "a sequence id is listed twice";
            seen[id] = 1;
            if (L < 0) L = row_len[id];
            else if (row_len[id] != L) return "the rows of a group differ in length";
            g.rowGroup[t] = k;
        }
        g.len.push_back(L);
        g.flagOff.push_back(g.flagWords);
        g.preOff.push_back(g.preInts);
        const int64_t words = ((int64_t)L + 31) / 32;
        g.flagWords += words;
        g.preInts += words + 1;
        g.maxLen = L > g.maxLen ? L : g.maxLen;
    }
    return nullptr;
}

// The tile list of the flags kernel: per group, column tiles of colTile columns by row slices of rowSlice rows, groups in order, a group's
// column tiles in order, a tile's slices in order.  A group of length 0 has no tile.
inline std::vector<SqueezeTilePlan> plan_squeeze_tiles(int32_t n_groups, const int32_t *group_off, const int32_t *len, int32_t colTile, int32_t rowSlice)
{
    std::vector<SqueezeTilePlan> tiles;
    for (int32_t k = 0; k < n_groups; ++k)
        for (int32_t c = 0; c < len[k]; c += colTile)
            for (int32_t r = group_off[k]; r < group_off[k + 1]; r += rowSlice)
                tiles.push_back(SqueezeTilePlan{k, c, r, r + rowSlice < group_off[k + 1] ? r + rowSlice : group_off[k + 1]});
    return tiles;
}
