// tests/level_plan_kats.cpp -- known answers of what a level call decides on the host: check_sides / plan_prepare / plan_align / check_commit / plan_commit,
// pure functions in twilight_amd/csrc/twl_level_plan.inc.hip (no HIP call: this program includes the file directly).  Every expected answer restates
// twilight_amd/csrc/twl_level.inc.hip of commit 3bf45a4 (twl_level_prepare 589-723, twl_level_align_mixed 748-820, twl_level_commit_from_dp 1037-1201), read as
// the specification; the line it restates is named.  Prints "OK <name>" / "FAIL <name>".
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include "../twilight_amd/csrc/twl_level_plan.inc.hip"

static int g_fail = 0;
#define CHECK(name, cond) do { if (cond) printf("OK %s\n", name); else { printf("FAIL %s\n", name); ++g_fail; } } while (0)

using V = std::vector<int32_t>;
static twl_side side(int32_t n_members, int32_t off, int32_t len, int32_t num = 1, int32_t cache_id = -1, int32_t store_id = -1, float weight = 1.0f)
{
    return twl_side{n_members, off, len, num, weight, cache_id, store_id, 0};
}
static bool is(const char *got, const char *want) { return got && want ? strcmp(got, want) == 0 : got == want; }

// a store of 8 sequences: rows 0-3 are 10 long, 4-5 are 20 long, 6 is empty, 7 is 10 long; it holds the cached profiles 5 (10 columns) and 6 (20 columns)
static const int32_t kRowLen[8] = {10, 10, 10, 10, 20, 20, 0, 10};
static const uint8_t kPlane[8] = {0, 1, 0, 1, 1, 0, 0, 1};
static const std::map<int32_t, int32_t> kCache = {{5, 10}, {6, 20}};
static int32_t cacheLen(int32_t id) { const auto it = kCache.find(id); return it == kCache.end() ? -1 : it->second; }
static const char *check(const std::vector<twl_side> &s, const V &members, int32_t seq_len = 32, bool tables = true)
{
    const std::vector<float> w(members.size() + 1, 1.0f);
    return check_sides((int32_t)s.size() / 2, s.data(), seq_len, tables ? members.data() : nullptr, tables ? w.data() : nullptr, 8, kRowLen, cacheLen);
}

static void prepare_kats()
{
    const V m2 = {0, 4};
    // ---- every rejection of twl_level_prepare, with its message ----
    CHECK("prepare_accepts_plain_pair", check({side(1, 0, 10), side(1, 1, 20)}, m2) == nullptr);
    // 612: n_members < 0 || member_off < 0 || len < 0 || len > seq_len || num < 1
    CHECK("prepare_rejects_negative_members", is(check({side(-1, 0, 10), side(1, 1, 20)}, m2), "bad side descriptor"));
    CHECK("prepare_rejects_negative_offset", is(check({side(1, -1, 10), side(1, 1, 20)}, m2), "bad side descriptor"));
    CHECK("prepare_rejects_negative_len", is(check({side(1, 0, -1), side(1, 1, 20)}, m2), "bad side descriptor"));
    CHECK("prepare_rejects_len_above_seq_len", is(check({side(1, 0, 10), side(1, 1, 20)}, m2, 19), "bad side descriptor"));
    CHECK("prepare_accepts_len_equal_seq_len", check({side(1, 0, 10), side(1, 1, 20)}, m2, 20) == nullptr);
    CHECK("prepare_rejects_num_0", is(check({side(1, 0, 10), side(1, 1, 20, 0)}, m2), "bad side descriptor"));
    // 612 comes before 631 for every side: a bad descriptor on the last side wins over a bad member on the first
    CHECK("prepare_descriptors_first", is(check({side(1, 0, 10), side(1, 1, 20, 0)}, {99, 4}), "bad side descriptor"));
    // 615: nm > 0 without the member tables
    CHECK("prepare_rejects_missing_tables", is(check({side(1, 0, 10), side(1, 1, 20)}, m2, 32, false), "member tables missing"));
    CHECK("prepare_accepts_no_members_no_tables", check({side(0, 0, 10, 1, 5), side(0, 0, 20, 1, 6)}, {}, 32, false) == nullptr);
    // 631: q < 0 || q >= n_seqs
    CHECK("prepare_rejects_member_8_of_8", is(check({side(1, 0, 10), side(1, 1, 20)}, {0, 8}), "member sequence id out of range"));
    CHECK("prepare_rejects_negative_member", is(check({side(1, 0, 10), side(1, 1, 20)}, {-1, 4}), "member sequence id out of range"));
    // 632: the member's row is not sd.len long
    CHECK("prepare_rejects_row_length", is(check({side(2, 0, 10), side(1, 2, 20)}, {0, 4, 5}), "member row length differs from the side's len"));
    CHECK("prepare_accepts_empty_rows", check({side(1, 0, 10), side(1, 1, 0)}, {0, 6}) == nullptr);
    // 640: cache id unknown, or of another length
    CHECK("prepare_rejects_unknown_cache_id", is(check({side(1, 0, 10, 1, 9), side(1, 1, 20)}, m2), "cache id unknown or of another length"));
    CHECK("prepare_rejects_cache_of_other_length", is(check({side(1, 0, 10, 1, 6), side(1, 1, 20)}, m2), "cache id unknown or of another length"));
    CHECK("prepare_accepts_cache_of_its_length", check({side(1, 0, 10, 1, 5), side(1, 1, 20, 1, 6)}, m2) == nullptr);
    // 643: store_id already in the store's table -- or registered by an earlier side of this very call (644-647 register at once)
    CHECK("prepare_rejects_store_id_in_use", is(check({side(1, 0, 10, 1, -1, 5), side(1, 1, 20)}, m2), "store_id already in use"));
    CHECK("prepare_rejects_store_id_twice_in_one_call", is(check({side(1, 0, 10, 1, -1, 3), side(1, 1, 20, 1, -1, 3)}, m2), "store_id already in use"));
    // 638 before 642: a side with a cache_id does not store, whatever its store_id says
    CHECK("prepare_cache_id_wins_over_store_id", check({side(1, 0, 10, 1, 5, 5), side(1, 1, 20)}, m2) == nullptr);
    // 639: the lookup sees what an earlier side of the call registered (647), with that side's length
    CHECK("prepare_cache_id_of_earlier_store_id", check({side(1, 0, 10, 1, -1, 3), side(1, 1, 10, 1, 3)}, {0, 1}) == nullptr);
    CHECK("prepare_cache_id_of_earlier_store_id_other_length", is(check({side(1, 0, 10, 1, -1, 3), side(1, 1, 20, 1, 3)}, m2), "cache id unknown or of another length"));
    // ---- a rejection on the LAST side after a valid store_id side: nothing may have been registered (the parent left id 3 behind: 647 runs before 631 of the later side)
    const std::vector<twl_side> late = {side(1, 0, 10, 1, -1, 3), side(1, 1, 10), side(1, 2, 10), side(1, 3, 10)};
    CHECK("prepare_rejects_last_side_member", is(check(late, {0, 1, 2, 99}), "member sequence id out of range"));
    CHECK("prepare_rejects_last_side_length", is(check(late, {0, 1, 2, 4}), "member row length differs from the side's len"));
    CHECK("prepare_corrected_call_passes", check(late, {0, 1, 2, 3}) == nullptr);       // (check_sides holds no state: the corrected call sees the store as it was)
    { std::vector<twl_side> s = late; s[3] = side(1, 3, 10, 1, 9);
      CHECK("prepare_rejects_last_side_cache_id", is(check(s, {0, 1, 2, 3}), "cache id unknown or of another length")); }

    // ---- plan_prepare ----
    {   // two pairs; cache id 5 on two sides (one slot: 621-626), a store_id side, a side of two members
        const std::vector<twl_side> s = {side(1, 0, 10, 3, 5, -1, 2.5f), side(2, 1, 10, 2, -1, 4, 0.5f), side(1, 3, 20, 1, 6), side(0, 4, 10, 7, 5)};
        const V mem = {0, 1, 3, 4};
        const PreparePlan pp = plan_prepare(2, s.data(), mem.data(), kPlane);
        CHECK("plan_prepare_nm", pp.nm == 4);                                                      // 613: max(member_off + n_members)
        CHECK("plan_prepare_slots_one_per_id", pp.slotIds == V({5, 4, 6}));                        // 621-626: first use order, one slot per id
        CHECK("plan_prepare_cache_slots", pp.dsides[0].cache_slot == 0 && pp.dsides[2].cache_slot == 2 && pp.dsides[3].cache_slot == 0);      // 641
        CHECK("plan_prepare_store_slot", pp.dsides[1].store_slot == 1 && pp.dsides[1].cache_slot == -1 && pp.dsides[0].store_slot == -1);      // 637, 648
        CHECK("plan_prepare_new_profiles", pp.newIds == V({4}) && pp.newLens == V({10}));           // 644-647
        CHECK("plan_prepare_side_fields", pp.dsides[1].n_members == 2 && pp.dsides[1].member_off == 1 && pp.dsides[1].len == 10 && pp.dsides[1].num == 2 &&
                                          pp.dsides[1].weight == 0.5f && pp.dsides[1].pad == 0 && pp.dsides[0].weight == 2.5f);      // 636-637
        CHECK("plan_prepare_member_planes", pp.mplane == std::vector<uint8_t>({0, 1, 1, 1}));       // 633: plane[members[k]]
        CHECK("plan_prepare_h_num", pp.h_num == V({3, 2, 1, 7}));                                   // 652
        CHECK("plan_prepare_reads_rows", pp.readsRows);                                             // 656: side 1 has no cache_id and two members
        CHECK("plan_prepare_max_len", pp.maxLen == 20);                                             // 696-697
    }
    {   // every side cached: nothing reads rows (656), although the sides list members
        const std::vector<twl_side> s = {side(1, 0, 10, 1, 5), side(1, 1, 20, 1, 6)};
        const V mem = {0, 4};
        CHECK("plan_prepare_all_cached_reads_no_rows", !plan_prepare(1, s.data(), mem.data(), kPlane).readsRows);
    }
    {   // an uncached side without members reads no row either (656: n_members > 0); maxLen starts at 1 (696)
        const std::vector<twl_side> s = {side(0, 0, 0), side(0, 0, 0)};
        const PreparePlan pp = plan_prepare(1, s.data(), nullptr, kPlane);
        CHECK("plan_prepare_empty_sides", !pp.readsRows && pp.maxLen == 1 && pp.nm == 0 && pp.slotIds.empty() && pp.mplane.empty());
    }
}

static void align_kats()
{
    // four pairs; prepared lengths after gappy-column removal
    const V h_len = {9, 10, 20, 20, 10, 0, 7, 7};
    const std::vector<twl_side> leaf = {side(1, 0, 10), side(1, 1, 10), side(1, 2, 20), side(1, 3, 20), side(1, 4, 10), side(1, 5, 0), side(1, 6, 7), side(1, 7, 7)};
    {   // all leaves, no mask: lm is h_len (762); pair 2 has an empty side and does not count (777, 784)
        const AlignPlan ap = plan_align(4, h_len, leaf.data(), nullptr, 1);
        CHECK("plan_align_all_leaf", ap.lm == h_len && ap.qryOneHot && ap.shape == 2);                   // 776-778, 791
        CHECK("plan_align_leaf_step_0", plan_align(4, h_len, leaf.data(), nullptr, 0).shape == 0 && plan_align(4, h_len, leaf.data(), nullptr, 0).qryOneHot);      // 781
    }
    {   // a mask zeroes both sides of the pairs that do not run (764)
        const uint8_t mask[4] = {1, 0, 1, 0};
        CHECK("plan_align_masked_lengths", plan_align(4, h_len, leaf.data(), mask, 1).lm == V({9, 10, 0, 0, 10, 0, 0, 0}));
    }
    {   // one cached REFERENCE side: the query is still one-hot (778 looks at side 1 only), the level is no leaf level (788)
        std::vector<twl_side> s = leaf; s[2] = side(1, 2, 20, 1, 5);
        const AlignPlan ap = plan_align(4, h_len, s.data(), nullptr, 1);
        CHECK("plan_align_cached_reference", ap.qryOneHot && ap.shape == 0);
        // ... masked out, it decides nothing (777, 784)
        const uint8_t mask[4] = {1, 0, 1, 1};
        const AlignPlan am = plan_align(4, h_len, s.data(), mask, 1);
        CHECK("plan_align_cached_reference_masked_out", am.qryOneHot && am.shape == 2);
    }
    {   // one cached QUERY side: not one-hot (778)
        std::vector<twl_side> s = leaf; s[1] = side(1, 1, 10, 1, 5);
        const AlignPlan ap = plan_align(4, h_len, s.data(), nullptr, 1);
        CHECK("plan_align_cached_query", !ap.qryOneHot && ap.shape == 0);
    }
    {   // a query side of two members: not one-hot, no leaf
        std::vector<twl_side> s = leaf; s[7] = side(2, 6, 7, 2);
        const AlignPlan ap = plan_align(4, h_len, s.data(), nullptr, 1);
        CHECK("plan_align_two_member_query", !ap.qryOneHot && ap.shape == 0);
    }
    {   // num > 1 on a single uncached sequence (a node that stands for several): one-hot (778 does not ask num) but no leaf (788: num == 1)
        std::vector<twl_side> s = leaf; s[0] = side(1, 0, 10, 3);
        const AlignPlan ap = plan_align(4, h_len, s.data(), nullptr, 1);
        CHECK("plan_align_num_above_1", ap.qryOneHot && ap.shape == 0);
    }
    {   // every pair masked: `any` stays false, shape 0 (791); qryOneHot keeps its initial true (776)
        const uint8_t mask[4] = {0, 0, 0, 0};
        const AlignPlan ap = plan_align(4, h_len, leaf.data(), mask, 1);
        CHECK("plan_align_all_masked", ap.shape == 0 && ap.qryOneHot && ap.lm == V(8, 0));
    }
}

static void commit_check_kats()
{
    const int32_t len3[3] = {30, 0, 12};
    const uint8_t dp110[3] = {1, 1, 0}, dp2[3] = {2, 0, 0}, dp000[3] = {0, 0, 0};
    // (n, seq_len, staged, haveDp, havePaths, path_len, path_stride, from_dp)
    CHECK("commit_accepts_host_paths", check_commit(3, 16, 0, true, true, len3, 30, nullptr) == nullptr);
    CHECK("commit_accepts_n_0_without_anything", check_commit(0, 16, 0, false, false, nullptr, 0, nullptr) == nullptr);      // 1043: n > 0 &&
    // 1043
    CHECK("commit_rejects_no_paths_no_from_dp", is(check_commit(3, 16, 0, true, false, len3, 30, nullptr), "bad argument"));
    CHECK("commit_rejects_no_path_len", is(check_commit(3, 16, 0, true, true, nullptr, 30, nullptr), "bad argument"));
    CHECK("commit_rejects_stride_0", is(check_commit(3, 16, 0, true, true, len3, 0, nullptr), "bad argument"));
    // 1044: after twl_level_restore the commit needs from_dp and the restore's pitch
    CHECK("commit_rejects_staged_without_from_dp", is(check_commit(3, 16, 30, true, true, len3, 30, nullptr), "commit after twl_level_restore: from_dp and the restore's row pitch are required"));
    CHECK("commit_rejects_staged_other_pitch", is(check_commit(3, 16, 32, true, true, len3, 30, dp110), "commit after twl_level_restore: from_dp and the restore's row pitch are required"));
    CHECK("commit_accepts_staged", check_commit(3, 16, 30, true, true, len3, 30, dp2) == nullptr);
    // 1045
    CHECK("commit_rejects_2_without_restore", is(check_commit(3, 16, 0, true, true, len3, 30, dp2), "from_dp == 2 without twl_level_restore"));
    // 1048: from_dp 1 needs the DP output, and a path that fits its rows (2 * seq_len)
    CHECK("commit_rejects_1_without_dp_output", is(check_commit(3, 16, 0, false, true, len3, 30, dp110), "from_dp without a DP output of this level"));
    CHECK("commit_rejects_1_longer_than_dp_row", is(check_commit(3, 14, 0, true, true, len3, 30, dp110), "from_dp without a DP output of this level"));
    CHECK("commit_accepts_1_at_dp_row_length", check_commit(3, 15, 0, true, true, len3, 30, dp110) == nullptr);
    // 1049: a host row without `paths`
    CHECK("commit_rejects_host_row_without_paths", is(check_commit(3, 16, 0, true, false, len3, 30, dp110), "bad argument"));
    { const int32_t l[3] = {30, 4, 0};
      CHECK("commit_accepts_no_paths_when_all_marked", check_commit(3, 16, 0, true, false, l, 30, dp110) == nullptr); }
    CHECK("commit_rejects_all_host_rows_without_paths", is(check_commit(3, 16, 0, true, false, len3, 30, dp000), "bad argument"));
    // 1054
    { const int32_t neg[3] = {30, -1, 12}, over[3] = {31, 0, 12};
      CHECK("commit_rejects_negative_path_len", is(check_commit(3, 16, 0, true, true, neg, 30, nullptr), "path_len outside [0, path_stride]"));
      CHECK("commit_rejects_path_len_above_stride", is(check_commit(3, 16, 0, true, true, over, 30, nullptr), "path_len outside [0, path_stride]")); }
}

static void commit_plan_kats()
{
    {   // members per workgroup: sides of 0, 1, 64, 65 and 129 members (1070: MG = 64; 1081)
        std::vector<twl_side> s;
        V members;
        const int counts[6] = {0, 1, 64, 65, 129, 2};
        for (int k = 0; k < 6; ++k) { s.push_back(side(counts[k], (int32_t)members.size(), 10, counts[k])); for (int m = 0; m < counts[k]; ++m) members.push_back((int32_t)members.size() % 8); }
        const int32_t plen[3] = {11, 12, 13};
        CommitPlan cp;
        plan_commit(cp, 3, s.data(), members, kPlane, plen, nullptr);
        CHECK("plan_commit_work_groups", cp.work == V({1, 0, 1, /* side 0: none */ 2, 0, 64, 3, 0, 64, 3, 64, 1, 4, 0, 64, 4, 64, 64, 4, 128, 1, 5, 0, 2}));
        CHECK("plan_commit_max_path_chunks", cp.maxPath == 13 && cp.nChunks == 1);                    // 1055, 1068
        CHECK("plan_commit_no_merge_without_ids", cp.nMerge() == 0 && cp.mergew.empty());             // 1085
        CHECK("plan_commit_member_planes", cp.mplane.size() == members.size() && cp.mplane[1] == kPlane[1] && cp.mplane[9] == kPlane[1]);      // 1100-1101
        CHECK("plan_commit_host_rows", cp.hostRows && !cp.side);                                      // 1103, 1152: from_dp NULL uploads every row
        CHECK("plan_commit_flips_every_member", cp.flips.size() == 2 * members.size() && cp.flips[0] == members[0] && cp.flips[1] == 11 &&
                                                cp.flips[2 * 1 + 1] == 12 && cp.flips.back() == 13);       // 1182-1190
    }
    {   // chunks of 256 path elements (1068)
        const std::vector<twl_side> s = {side(1, 0, 10), side(1, 1, 10)};
        const V members = {0, 1};
        CommitPlan cp;
        for (const auto &c : std::vector<std::pair<int32_t, int32_t>>{{1, 1}, {256, 1}, {257, 2}, {513, 3}}) {
            plan_commit(cp, 1, s.data(), members, kPlane, &c.first, nullptr);
            CHECK(("plan_commit_chunks_" + std::to_string(c.first)).c_str(), cp.maxPath == c.first && cp.nChunks == c.second);
        }
    }
    // four pairs of single sequences; pair 1 has path length 0 (1078: skipped everywhere), pairs 0 and 3 carry profile ids on both sides, pair 2 on one side only
    const std::vector<twl_side> s = {side(1, 0, 10, 1, 5, -1, 2.0f), side(1, 1, 10, 1, -1, 7, 3.0f), side(1, 2, 10, 1, 8), side(1, 3, 10, 1, 9),
                                     side(1, 4, 20, 1, 6), side(1, 5, 20), side(1, 6, 0, 1, -1, 11, 0.25f), side(1, 7, 10, 1, 12, 13, 0.75f)};
    const V members = {0, 1, 2, 3, 4, 5, 6, 7};
    const int32_t plen[4] = {300, 0, 40, 10};
    {
        const uint8_t dp[4] = {1, 1, 2, 1};
        CommitPlan cp;
        cp.work = {9, 9, 9}; cp.flips = {1, 2};       // (the plan is reused by the store: whatever it held is gone)
        plan_commit(cp, 4, s.data(), members, kPlane, plen, dp);
        CHECK("plan_commit_skips_length_0", cp.work == V({0, 0, 1, 1, 0, 1, 4, 0, 1, 5, 0, 1, 6, 0, 1, 7, 0, 1}));      // 1078, 1081
        // 1084-1094: ids are cache_id, else store_id; the pointer table holds (reference, query, merged) per merged pair, in order
        CHECK("plan_commit_merge_both_ids_only", cp.merge == V({0, 0, 1, 2, 3, 3, 4, 5}) && cp.mergeIds == V({5, 7, 11, 12}));
        CHECK("plan_commit_merge_weights", cp.mergew == std::vector<float>({2.0f, 3.0f, 0.25f, 0.75f}));      // 1093
        CHECK("plan_commit_from_dp_marked_no_host_rows", !cp.hostRows && cp.side);                        // 1103, 1113 (pair 1 is unmarked but empty), 1152
        CHECK("plan_commit_flips_committed_pairs_only", cp.flips == V({0, 300, 1, 300, 4, 40, 5, 40, 6, 10, 7, 10}));      // 1183: pairs of length 0 keep plane and length
        CHECK("plan_commit_chunks_300", cp.maxPath == 300 && cp.nChunks == 2);
    }
    {   // from_dp mixes: one unmarked pair WITH a path is a host row (1113) and keeps the rewrite on the first stream (1152)
        const uint8_t dp[4] = {1, 0, 0, 2};
        CommitPlan cp;
        plan_commit(cp, 4, s.data(), members, kPlane, plen, dp);
        CHECK("plan_commit_one_host_row", cp.hostRows && !cp.side);
        const uint8_t dp0[4] = {0, 0, 0, 0};
        plan_commit(cp, 4, s.data(), members, kPlane, plen, dp0);
        CHECK("plan_commit_from_dp_all_0", cp.hostRows && !cp.side);
        const uint8_t dp2[4] = {2, 2, 2, 2};
        plan_commit(cp, 4, s.data(), members, kPlane, plen, dp2);
        CHECK("plan_commit_from_dp_all_2", !cp.hostRows && cp.side);
    }
    {   // 1152: side = nWork > 0 && n <= 32 && !hostRows
        for (int n : {32, 33}) {
            std::vector<twl_side> w;
            V mem;
            for (int i = 0; i < 2 * n; ++i) { w.push_back(side(1, i, 10)); mem.push_back(i % 8); }
            const V len((size_t)n, 5);
            const std::vector<uint8_t> dp((size_t)n, 1);
            CommitPlan cp;
            plan_commit(cp, n, w.data(), mem, kPlane, len.data(), dp.data());
            CHECK(n == 32 ? "plan_commit_side_at_32_pairs" : "plan_commit_no_side_at_33_pairs", cp.side == (n == 32) && cp.nWork() == 2u * n);
        }
        // no member anywhere: nothing to rewrite, no second stream
        const std::vector<twl_side> none = {side(0, 0, 10, 1, 5), side(0, 0, 20, 1, 6)};
        const int32_t one[1] = {25};
        const uint8_t dp[1] = {1};
        CommitPlan cp;
        plan_commit(cp, 1, none.data(), V(), kPlane, one, dp);
        CHECK("plan_commit_no_work_no_side", cp.nWork() == 0 && !cp.side && cp.nMerge() == 1 && cp.flips.empty());
    }
}

int main()
{
    prepare_kats();
    align_kats();
    commit_check_kats();
    commit_plan_kats();
    printf("%d failed\n", g_fail);
    return g_fail ? 1 : 0;
}
