// twilight_amd/csrc/twl_level_plan.inc.hip -- what a level call decides on the host, as PURE functions of the call's arguments and of the store's
// bookkeeping: what twl_level_prepare and twl_level_commit_from_dp reject (check_sides, check_commit) and the tables their kernels read
// (plan_prepare, plan_align, plan_commit).  No HIP call and no global in this file: tests/level_plan_kats.cpp includes it directly.  Cached profiles
// appear as the caller's ids; twl_level.inc.hip turns them into device pointers.  Included by twl_align.hip (one translation unit).
#include <algorithm>
#include <cstdint>
#include <unordered_map>
#include <vector>
#include "../../include/twl_level.h"

// A side as the level kernels read it: field for field twl::SideDesc (level_kernels.hip.h; twl_level.inc.hip asserts the layout).
struct SideRow { int32_t n_members, member_off, len, num; float weight; int32_t cache_slot, store_slot, pad; };

// Everything twl_level_prepare rejects in its sides, decided before anything is allocated or registered: the message, or nullptr.
// row_len[q]: current row length of sequence q; cacheLen(id): length of the cached profile `id`, -1 when the store has none.
template <class CacheLen>
const char *check_sides(int32_t n_pairs, const twl_side *sides, int32_t seq_len, const int32_t *members, const float *member_weight, int32_t n_seqs,
                        const int32_t *row_len, CacheLen cacheLen)
{
    const size_t ns = (size_t)n_pairs * 2;
    size_t nm = 0;
    for (size_t i = 0; i < ns; ++i) {
        const twl_side &sd = sides[i];
        if (sd.n_members < 0 || sd.member_off < 0 || sd.len < 0 || sd.len > seq_len || sd.num < 1) return "bad side descriptor";
        nm = std::max(nm, (size_t)sd.member_off + (size_t)sd.n_members);
    }
    if (nm > 0 && (!members || !member_weight)) return "member tables missing";
    std::unordered_map<int32_t, int32_t> stored;      // profiles that earlier sides of this call store, and their lengths
    for (size_t i = 0; i < ns; ++i) {
        const twl_side &sd = sides[i];
        for (int32_t m = 0; m < sd.n_members; ++m) {
            const int32_t q = members[sd.member_off + m];
            if (q < 0 || q >= n_seqs) return "member sequence id out of range";
            if (row_len[q] != sd.len) return "member row length differs from the side's len";
        }
        if (sd.cache_id >= 0) {
            const auto it = stored.find(sd.cache_id);
            if ((it != stored.end() ? it->second : cacheLen(sd.cache_id)) != sd.len) return "cache id unknown or of another length";
        } else if (sd.store_id >= 0) {
            if (stored.count(sd.store_id) || cacheLen(sd.store_id) >= 0) return "store_id already in use";
            stored[sd.store_id] = sd.len;
        }
    }
    return nullptr;
}

struct PreparePlan {
    size_t nm = 0;                          // entries of the member tables
    std::vector<SideRow> dsides;            // [2 * n_pairs]
    std::vector<int32_t> slotIds;           // the cache pointer table, as ids: slot k holds the profile slotIds[k] (one slot per id)
    std::vector<int32_t> newIds, newLens;   // profiles this level stores (store_id sides, in side order) and their lengths
    std::vector<uint8_t> mplane;            // [nm] plane of every member's current row
    std::vector<int32_t> h_num;             // [2 * n_pairs] alnNum
    bool readsRows = false;                 // a side is built from rows (not from a cached profile)
    int32_t maxLen = 1;
};

// The tables of a prepare whose sides check_sides has passed.  plane[q]: plane of sequence q's current row.
inline PreparePlan plan_prepare(int32_t n_pairs, const twl_side *sides, const int32_t *members, const uint8_t *plane)
{
    PreparePlan pp;
    const size_t ns = (size_t)n_pairs * 2;
    for (size_t i = 0; i < ns; ++i) pp.nm = std::max(pp.nm, (size_t)sides[i].member_off + (size_t)sides[i].n_members);
    pp.mplane.assign(pp.nm, 0);
    pp.dsides.resize(ns);
    pp.h_num.resize(ns);
    std::unordered_map<int32_t, int32_t> slotOf;
    auto slot = [&](int32_t id) {
        const auto it = slotOf.find(id);
        if (it != slotOf.end()) return it->second;
        pp.slotIds.push_back(id);
        return slotOf[id] = (int32_t)pp.slotIds.size() - 1;
    };
    for (size_t i = 0; i < ns; ++i) {
        const twl_side &sd = sides[i];
        for (int32_t m = 0; m < sd.n_members; ++m) pp.mplane[sd.member_off + m] = plane[members[sd.member_off + m]];
        SideRow &ds = pp.dsides[i];
        ds.n_members = sd.n_members; ds.member_off = sd.member_off; ds.len = sd.len; ds.num = sd.num; ds.weight = sd.weight;
        ds.cache_slot = ds.store_slot = -1; ds.pad = 0;
        if (sd.cache_id >= 0) ds.cache_slot = slot(sd.cache_id);
        else if (sd.store_id >= 0) { pp.newIds.push_back(sd.store_id); pp.newLens.push_back(sd.len); ds.store_slot = slot(sd.store_id); }
        pp.h_num[i] = sd.num;
        pp.readsRows = pp.readsRows || (sd.cache_id < 0 && sd.n_members > 0);
        pp.maxLen = std::max(pp.maxLen, sd.len);
    }
    return pp;
}

struct AlignPlan {
    std::vector<int32_t> lm;      // [2 * n] the prepared lengths, 0 on both sides of a pair that does not run
    bool qryOneHot = true;        // every selected query side a single, uncached sequence: its profile rows hold one letter each (profile_kernel built them)
    int shape = 0;                // 2: every selected pair is two single uncached sequences -- no gap letter, denominators of 1 (run_device, shape)
};

inline AlignPlan plan_align(int32_t n, const std::vector<int32_t> &h_len, const twl_side *sides, const uint8_t *run_mask, int leaf_step)
{
    AlignPlan ap;
    ap.lm = h_len;
    if (run_mask)
        for (int32_t i = 0; i < n; ++i) if (!run_mask[i]) ap.lm[2 * i] = ap.lm[2 * i + 1] = 0;
    auto runs = [&](int32_t i) { return ap.lm[2 * i] > 0 && ap.lm[2 * i + 1] > 0; };
    for (int32_t i = 0; i < n && ap.qryOneHot; ++i)
        if (runs(i)) ap.qryOneHot = sides[2 * (size_t)i + 1].n_members == 1 && sides[2 * (size_t)i + 1].cache_id < 0;
    if (leaf_step) {
        bool leaf = true, any = false;
        for (int32_t i = 0; i < n && leaf; ++i) {
            if (!runs(i)) continue;
            any = true;
            for (int side = 0; side < 2; ++side) {
                const twl_side &sd = sides[2 * (size_t)i + side];
                leaf = leaf && sd.n_members == 1 && sd.cache_id < 0 && sd.num == 1;
            }
        }
        ap.shape = (any && leaf) ? 2 : 0;
    }
    return ap;
}

// Everything twl_level_commit_from_dp rejects once the level is known to be prepared: the message, or nullptr.  staged: the row pitch of
// twl_level_restore (0: not called); haveDp: the level holds a DP output.
inline const char *check_commit(int32_t n, int32_t seq_len, int32_t staged, bool haveDp, bool havePaths, const int32_t *path_len, int32_t path_stride,
                                const uint8_t *from_dp)
{
    if (n > 0 && ((!havePaths && !from_dp) || !path_len || path_stride < 1)) return "bad argument";
    if (staged && (!from_dp || staged != path_stride)) return "commit after twl_level_restore: from_dp and the restore's row pitch are required";
    if (from_dp && !staged) for (int32_t i = 0; i < n; ++i) if (from_dp[i] == 2) return "from_dp == 2 without twl_level_restore";
    if (from_dp) {
        for (int32_t i = 0; i < n; ++i) {
            if (from_dp[i] == 1 && (!haveDp || path_len[i] > 2 * seq_len)) return "from_dp without a DP output of this level";
            if (!from_dp[i] && path_len[i] > 0 && !havePaths) return "bad argument";
        }
    }
    for (int32_t i = 0; i < n; ++i) if (path_len[i] < 0 || path_len[i] > path_stride) return "path_len outside [0, path_stride]";
    return nullptr;
}

// Everything twl_level_paths_to_block / twl_level_paths_from_block reject in their row selection, decided before the first launch (a refused call
// has written nothing): the message, or nullptr.  where == nullptr: every row is a row of the path buffer (2).  staged, haveDp as in check_commit.
// room >= 0: the block starts inside one of the level's own exchange buffers with `room` bytes left from there on, and no row may leave them;
// room < 0: the block is the caller's memory, its size is not known here.  Rows of length <= 0 are not moved and not looked at.
inline const char *check_block_rows(bool toBlock, int32_t n_sel, const int32_t *pairs, const int32_t *lens, const uint8_t *where, const int64_t *blk_off,
                                    int32_t n_pairs, int32_t seq_len, int32_t staged, bool haveDp, int64_t room)
{
    for (int32_t t = 0; t < n_sel; ++t) {
        if (lens[t] <= 0) continue;
        const int w = where ? where[t] : 2;
        if (w != 1 && w != 2) return "bad row selection";
        if (w == 1 && (!toBlock || !haveDp)) return "bad row selection";      // (the DP output is only ever a source)
        if (pairs[t] < 0 || pairs[t] >= n_pairs || (int64_t)lens[t] > (w == 1 ? 2 * (int64_t)seq_len : (int64_t)staged)) return "bad row selection";
        if (room >= 0 && (blk_off[t] < 0 || blk_off[t] > room || (int64_t)lens[t] > room - blk_off[t])) return "bad row selection";
    }
    return nullptr;
}

constexpr int kRowGroup = 64;      // members per workgroup of the row rewrite (its scan of the path chunk is shared by them)

struct CommitPlan {                 // (kept by the store for its capacity)
    int32_t maxPath = 0, nChunks = 0;
    std::vector<int32_t> work;      // [3 * nWork] (side index, first member, members <= kRowGroup) of every workgroup of the row rewrite
    std::vector<int32_t> merge;     // [4 * nMerge] (pair, slots of the reference's, the query's and the merged profile in the pointer table)
    std::vector<float> mergew;      // [2 * nMerge] alnWeight of the two sides
    std::vector<int32_t> mergeIds;  // [2 * nMerge] cache ids of the two sides (pointer table: slots 3k, 3k + 1; the merged profile of pair merge[4k]: 3k + 2)
    std::vector<uint8_t> mplane;    // [members] plane of every member's current row
    std::vector<int32_t> flips;     // (sequence, length) of every member of a committed pair: its row goes to its other plane with the path's length
    bool hostRows = false;          // rows of the caller's `paths` are uploaded
    bool side = false;              // the row rewrite goes to the device's second stream
    unsigned nWork() const { return (unsigned)(work.size() / 3); }
    unsigned nMerge() const { return (unsigned)(merge.size() / 4); }
};

inline int32_t max_path(int32_t n, const int32_t *path_len)
{
    int32_t m = 0;
    for (int32_t i = 0; i < n; ++i) m = std::max(m, path_len[i]);
    return m;
}

// The tables of a commit that check_commit has passed.  sides / members: the prepared level's; plane[q] as in plan_prepare.
inline void plan_commit(CommitPlan &cp, int32_t n, const twl_side *sides, const std::vector<int32_t> &members, const uint8_t *plane, const int32_t *path_len,
                        const uint8_t *from_dp)
{
    cp.work.clear(); cp.merge.clear(); cp.mergew.clear(); cp.mergeIds.clear(); cp.flips.clear();
    cp.maxPath = max_path(n, path_len);
    cp.nChunks = (cp.maxPath + 255) / 256;
    cp.hostRows = !from_dp;
    for (int32_t i = 0; i < n; ++i) {
        if (path_len[i] == 0) continue;
        if (from_dp && !from_dp[i]) cp.hostRows = true;
        for (int sd = 0; sd < 2; ++sd) {
            const twl_side &x = sides[2 * (size_t)i + sd];
            for (int32_t m = 0; m < x.n_members; m += kRowGroup) { cp.work.push_back(2 * i + sd); cp.work.push_back(m); cp.work.push_back(std::min(kRowGroup, x.n_members - m)); }
            for (int32_t m = 0; m < x.n_members; ++m) { cp.flips.push_back(members[x.member_off + m]); cp.flips.push_back(path_len[i]); }
        }
        const twl_side &r = sides[2 * (size_t)i], &q = sides[2 * (size_t)i + 1];
        const int32_t rid = r.cache_id >= 0 ? r.cache_id : r.store_id, qid = q.cache_id >= 0 ? q.cache_id : q.store_id;
        if (rid >= 0 && qid >= 0) {             // updateFrequency: both nodes carry a cached profile
            const int32_t at = 3 * (int32_t)cp.nMerge();
            cp.merge.insert(cp.merge.end(), {i, at, at + 1, at + 2});
            cp.mergew.push_back(r.weight); cp.mergew.push_back(q.weight);
            cp.mergeIds.push_back(rid); cp.mergeIds.push_back(qid);
        }
    }
    // current planes of the members (prepare's table may be stale if a sequence took part in an earlier commit of this level: it cannot,
    // a sequence belongs to one node of one pair per level)
    cp.mplane.resize(members.size());
    for (size_t k = 0; k < members.size(); ++k) cp.mplane[k] = plane[members[k]];
    cp.side = cp.nWork() > 0 && n <= 32 && !cp.hostRows;
}
