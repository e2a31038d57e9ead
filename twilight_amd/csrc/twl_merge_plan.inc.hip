// twilight_amd/csrc/twl_merge_plan.inc.hip -- what the calls of include/twl_merge.h decide on the host, as PURE functions of the call's arguments and of
// the merge's bookkeeping: everything twl_merge_create / twl_merge_apply / twl_merge_finish reject, and the tables the apply's kernels read.
// No HIP call and no global in this file: tests/merge_plan_kats.cpp includes it directly.  Included by twl_merge.inc.hip (one translation unit).
#include <algorithm>
#include <cstdint>
#include <vector>
#include "../../include/twl_merge.h"
#include "twl_path_source.inc.hip"

// The groups of a merge as the host knows them.
struct MergeGroups {
    std::vector<int32_t> off, rows;      // CSR: the rows of group g are rows[off[g], off[g + 1])
    std::vector<int32_t> L;              // [n_groups] original length of the group's rows
    std::vector<int32_t> width;          // [n_groups] current width of the merged alignment the group is part of
    std::vector<int64_t> posOff;         // [n_groups] offset of the group's map in the map arena, in ints
    int64_t posInts = 0;
    int32_t maxL = 1;
    int32_t n() const { return (int32_t)L.size(); }
};

// Everything twl_merge_create rejects: the message, or nullptr with `g` filled in.  row_len[q]: current row length of sequence q.
inline const char *check_merge_create(int32_t n_groups, const int32_t *group_off, const int32_t *row_ids, int32_t n_seqs, const int32_t *row_len, MergeGroups &g)
{
    if (n_groups < 0 || !group_off || group_off[0] != 0) return "bad group table";
    for (int32_t k = 0; k < n_groups; ++k) {
        if (group_off[k + 1] < group_off[k]) return "bad group table";
        if (group_off[k + 1] == group_off[k]) return "a group without rows";
    }
    const int32_t nRows = group_off[n_groups];
    if (nRows > 0 && !row_ids) return "bad group table";
    std::vector<uint8_t> seen((size_t)std::max(n_seqs, 0), 0);
    g = MergeGroups{};
    for (int32_t k = 0; k < n_groups; ++k) {
        int32_t L = -1;
        for (int32_t t = group_off[k]; t < group_off[k + 1]; ++t) {
            const int32_t q = row_ids[t];
            if (q < 0 || q >= n_seqs) return "row id out of range";
            if (seen[q]) return "a row is listed twice";
            seen[q] = 1;
            if (L < 0) L = row_len[q];
            else if (row_len[q] != L) return "the rows of a group differ in length";
        }
        g.L.push_back(L);
        g.width.push_back(L);
        g.posOff.push_back(g.posInts);
        g.posInts += L;
        g.maxL = std::max(g.maxL, L);
    }
    g.off.assign(group_off, group_off + n_groups + 1);
    g.rows.assign(row_ids, row_ids + nRows);
    return nullptr;
}

// One map to compose: pos[pos_off + c] = ranks[tab_off + pos[pos_off + c]] for c < L.  Field for field twl::ComposeJob (merge_kernels.hip.h).
struct ComposeRow { int64_t pos_off, tab_off; int32_t L, tab_len; };

struct MergeApplyPlan {
    std::vector<int32_t> pair;           // the pairs that take part (path_len != 0), in order
    std::vector<int32_t> plen, wr, wq;   // per taking pair: path length, current width of its reference / query side
    PathSources src;                     // per taking pair: where its path lives (twl_path_source.inc.hip)
    std::vector<int64_t> rOff, qOff;     // per taking pair: where rpos / qpos start in the rank arena, in ints
    int64_t rankInts = 0;
    std::vector<ComposeRow> jobs;        // one per group under a side of a taking pair
    std::vector<int32_t> jobGroup, jobPair;   // the group of each job, and the index (into `pair`) of its pair
    int32_t maxL = 1;
};

// Everything twl_merge_apply rejects before a path is looked at: the message, or nullptr with `p` filled in.
inline const char *check_merge_apply(const MergeGroups &g, bool finished, int32_t n_pairs, const int32_t *ref_off, const int32_t *ref_groups, const int32_t *qry_off,
                                     const int32_t *qry_groups, bool havePaths, const int32_t *path_len, int32_t path_stride, const uint8_t *from_dp,
                                     const PathLevelView &lv, MergeApplyPlan &p)
{
    p = MergeApplyPlan{};
    if (n_pairs < 0 || (n_pairs > 0 && (!ref_off || !qry_off || !ref_groups || !qry_groups || !path_len || path_stride < 1))) return "bad argument";
    if (finished) return "twl_merge_apply after twl_merge_finish";
    if (const char *why = check_path_level(from_dp, n_pairs, lv)) return why;
    if (n_pairs > 0 && (ref_off[0] < 0 || qry_off[0] < 0)) return "bad group table";
    for (int32_t i = 0; i < n_pairs; ++i)
        if (ref_off[i + 1] < ref_off[i] || qry_off[i + 1] < qry_off[i]) return "bad group table";
    std::vector<uint8_t> seen((size_t)g.n(), 0);
    for (int32_t i = 0; i < n_pairs; ++i) {
        const int32_t n = path_len[i];
        if (n == 0) continue;
        int32_t w[2] = {-1, -1};
        for (int side = 0; side < 2; ++side) {
            const int32_t *off = side ? qry_off : ref_off, *grp = side ? qry_groups : ref_groups;
            if (off[i + 1] == off[i]) return "a side without groups";
            for (int32_t t = off[i]; t < off[i + 1]; ++t) {
                const int32_t k = grp[t];
                if (k < 0 || k >= g.n()) return "group id out of range";
                if (seen[k]) return "a group appears under two sides of one call";
                seen[k] = 1;
                if (w[side] < 0) w[side] = g.width[k];
                else if (g.width[k] != w[side]) return "the groups of a side differ in width";
            }
        }
        if (n < 0 || n > path_stride || (int64_t)n > (int64_t)w[0] + w[1]) return "path_len outside [0, min(path_stride, ref width + qry width)]";
        if (const char *why = add_path_source(p.src, i, n, from_dp, havePaths, path_stride, lv)) return why;
        const int32_t at = (int32_t)p.pair.size();
        p.pair.push_back(i); p.plen.push_back(n); p.wr.push_back(w[0]); p.wq.push_back(w[1]);
        p.rOff.push_back(p.rankInts); p.rankInts += w[0];
        p.qOff.push_back(p.rankInts); p.rankInts += w[1];
        for (int side = 0; side < 2; ++side) {
            const int32_t *off = side ? qry_off : ref_off, *grp = side ? qry_groups : ref_groups;
            for (int32_t t = off[i]; t < off[i + 1]; ++t) {
                const int32_t k = grp[t];
                p.jobs.push_back(ComposeRow{g.posOff[k], side ? p.qOff[at] : p.rOff[at], g.L[k], w[side]});
                p.jobGroup.push_back(k);
                p.jobPair.push_back(at);
                p.maxL = std::max(p.maxL, g.L[k]);
            }
        }
    }
    return nullptr;
}

// The second half of the apply's decision, on what the rank kernel counted in every taking path: counts[k] = {codes != 1, codes != 2,
// 1 when a code outside 0..2 was seen}.  The message, or nullptr: the maps may be composed.
inline const char *check_merge_counts(const MergeApplyPlan &p, const int32_t *counts)
{
    for (size_t k = 0; k < p.pair.size(); ++k) {
        if (counts[3 * k + 2]) return "a path holds a code other than 0, 1, 2";
        if (counts[3 * k] != p.wr[k]) return "a path's codes != 1 do not cover the columns of its reference side exactly";
        if (counts[3 * k + 1] != p.wq[k]) return "a path's codes != 2 do not cover the columns of its query side exactly";
    }
    return nullptr;
}

// After a passed apply: the groups of every taking pair are as wide as its path is long.
inline void merge_apply_done(MergeGroups &g, const MergeApplyPlan &p)
{
    for (size_t j = 0; j < p.jobs.size(); ++j) g.width[p.jobGroup[j]] = p.plen[p.jobPair[j]];
}

// What twl_merge_finish rejects: the message, or nullptr with *W the one width of all groups (0 for a merge without groups).
inline const char *check_merge_finish(const MergeGroups &g, bool finished, const int32_t *row_len, int32_t *W)
{
    if (finished) return "twl_merge_finish called twice";
    *W = g.n() ? g.width[0] : 0;
    for (int32_t k = 0; k < g.n(); ++k) {
        if (g.width[k] != *W) return "the groups have not been merged to one width";
        for (int32_t t = g.off[k]; t < g.off[k + 1]; ++t)
            if (row_len[g.rows[t]] != g.L[k]) return "a row has been rewritten since the merge began";
    }
    return nullptr;
}
