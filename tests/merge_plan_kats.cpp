// tests/merge_plan_kats.cpp -- known answers of what the calls of include/twl_merge.h decide on the host: check_merge_create / check_merge_apply /
// check_merge_counts / merge_apply_done / check_merge_finish, pure functions in twilight_amd/csrc/twl_merge_plan.inc.hip (no HIP call: this program
// includes the file directly).  The expected answers restate include/twl_merge.h.  Prints "OK <name>" / "FAIL <name>".
#include <cstdio>
#include <cstring>
#include <string>
#include "../twilight_amd/csrc/twl_merge_plan.inc.hip"

static int g_fail = 0;
#define CHECK(name, cond) do { if (cond) printf("OK %s\n", name); else { printf("FAIL %s\n", name); ++g_fail; } } while (0)

using V = std::vector<int32_t>;
static bool is(const char *got, const char *want) { return got && want ? strcmp(got, want) == 0 : got == want; }

// a store of 8 rows: 0-2 are 10 long, 3-4 are 7 long, 5 is 12 long, 6 is 10 long, 7 is empty
static const int32_t kRowLen[8] = {10, 10, 10, 7, 7, 12, 10, 0};

static const char *create(const V &off, const V &rows, MergeGroups &g) { return check_merge_create((int32_t)off.size() - 1, off.data(), rows.data(), 8, kRowLen, g); }

static void create_kats()
{
    MergeGroups g;
    CHECK("create_accepts_three_groups", create({0, 3, 5, 6}, {0, 1, 2, 3, 4, 5}, g) == nullptr);
    CHECK("create_lengths", g.L == V({10, 7, 12}) && g.width == V({10, 7, 12}));
    CHECK("create_map_offsets", g.posOff == std::vector<int64_t>({0, 10, 17}) && g.posInts == 29 && g.maxL == 12);
    CHECK("create_keeps_csr", g.off == V({0, 3, 5, 6}) && g.rows == V({0, 1, 2, 3, 4, 5}));
    CHECK("create_accepts_no_groups", create({0}, {}, g) == nullptr && g.n() == 0);
    CHECK("create_accepts_a_group_of_empty_rows", create({0, 1}, {7}, g) == nullptr && g.L == V({0}));
    CHECK("create_rejects_null_offsets", is(check_merge_create(1, nullptr, nullptr, 8, kRowLen, g), "bad group table"));
    CHECK("create_rejects_negative_count", is(check_merge_create(-1, V({0}).data(), nullptr, 8, kRowLen, g), "bad group table"));
    CHECK("create_rejects_offsets_not_from_0", is(create({1, 2}, {0, 1}, g), "bad group table"));
    CHECK("create_rejects_decreasing_offsets", is(create({0, 2, 1}, {0, 1}, g), "bad group table"));
    CHECK("create_rejects_empty_group", is(create({0, 2, 2}, {0, 1}, g), "a group without rows"));
    CHECK("create_rejects_row_8_of_8", is(create({0, 1}, {8}, g), "row id out of range"));
    CHECK("create_rejects_negative_row", is(create({0, 1}, {-1}, g), "row id out of range"));
    CHECK("create_rejects_row_in_two_groups", is(create({0, 2, 3}, {0, 1, 0}, g), "a row is listed twice"));
    CHECK("create_rejects_row_twice_in_a_group", is(create({0, 2}, {1, 1}, g), "a row is listed twice"));
    CHECK("create_rejects_rows_of_two_lengths", is(create({0, 2}, {0, 3}, g), "the rows of a group differ in length"));
}

struct Call {
    V refOff, refG, qryOff, qryG, plen;
    int32_t stride = 64;
    std::vector<uint8_t> fromDp;
    bool havePaths = true, finished = false;
    PathLevelView lv;
};
static const char *apply(const MergeGroups &g, const Call &c, MergeApplyPlan &p)
{
    return check_merge_apply(g, c.finished, (int32_t)c.plen.size(), c.refOff.data(), c.refG.data(), c.qryOff.data(), c.qryG.data(), c.havePaths, c.plen.data(), c.stride,
                             c.fromDp.empty() ? nullptr : c.fromDp.data(), c.lv, p);
}

static void apply_kats()
{
    // four groups: 0 (rows 0-2, 10 columns), 1 (rows 3-4, 7 columns), 2 (row 5, 12 columns), 3 (row 6, 10 columns)
    MergeGroups g;
    create({0, 3, 5, 6, 7}, {0, 1, 2, 3, 4, 5, 6}, g);
    MergeApplyPlan p;
    Call one;
    one.refOff = {0, 1}; one.refG = {0}; one.qryOff = {0, 1}; one.qryG = {1}; one.plen = {12};
    CHECK("apply_accepts_one_pair", apply(g, one, p) == nullptr);
    CHECK("apply_plan_widths", p.pair == V({0}) && p.wr == V({10}) && p.wq == V({7}) && p.plen == V({12}));
    CHECK("apply_plan_rank_tables", p.rOff == std::vector<int64_t>({0}) && p.qOff == std::vector<int64_t>({10}) && p.rankInts == 17);
    CHECK("apply_plan_jobs", p.jobs.size() == 2 && p.jobs[0].pos_off == 0 && p.jobs[0].tab_off == 0 && p.jobs[0].L == 10 && p.jobs[0].tab_len == 10 &&
                             p.jobs[1].pos_off == 10 && p.jobs[1].tab_off == 10 && p.jobs[1].L == 7 && p.jobs[1].tab_len == 7 && p.maxL == 10);
    CHECK("apply_plan_host_row", p.src.which == std::vector<uint8_t>({0}) && p.src.hostRows == V({0}) && p.src.srcOff == std::vector<int64_t>({0}));
    // the shape of a path is decided on what the rank kernel counted
    const int32_t good[3] = {10, 7, 0}, shortRef[3] = {9, 7, 0}, longQry[3] = {10, 8, 0}, badCode[3] = {10, 7, 1};
    CHECK("counts_accept_exact_cover", check_merge_counts(p, good) == nullptr);
    CHECK("counts_reject_reference_count", is(check_merge_counts(p, shortRef), "a path's codes != 1 do not cover the columns of its reference side exactly"));
    CHECK("counts_reject_query_count", is(check_merge_counts(p, longQry), "a path's codes != 2 do not cover the columns of its query side exactly"));
    CHECK("counts_reject_foreign_code", is(check_merge_counts(p, badCode), "a path holds a code other than 0, 1, 2"));
    // a passed apply widens both groups to the path's length; the others keep theirs
    MergeGroups g1 = g;
    merge_apply_done(g1, p);
    CHECK("done_sets_widths", g1.width == V({12, 12, 12, 10}));
    // ... after which group 0 and group 1 may share a side, and group 3 (10 wide) may not join them
    Call two;
    two.refOff = {0, 2}; two.refG = {0, 1}; two.qryOff = {0, 1}; two.qryG = {2}; two.plen = {20};
    CHECK("apply_accepts_two_groups_under_a_side", apply(g1, two, p) == nullptr && p.jobs.size() == 3 && p.wr == V({12}) && p.wq == V({12}));
    CHECK("apply_jobs_share_the_side_table", p.jobs[0].tab_off == 0 && p.jobs[1].tab_off == 0 && p.jobs[2].tab_off == 12 && p.jobs[1].pos_off == 10 && p.jobs[2].pos_off == 17);
    two.refG = {0, 3};
    CHECK("apply_rejects_widths_under_a_side", is(apply(g1, two, p), "the groups of a side differ in width"));
    CHECK("apply_rejects_before_first_apply_too", is(apply(g, Call{{0, 2}, {0, 1}, {0, 1}, {2}, {20}}, p), "the groups of a side differ in width"));

    Call c = one;
    c.qryG = {0};
    CHECK("apply_rejects_group_under_both_sides", is(apply(g, c, p), "a group appears under two sides of one call"));
    Call twoPairs;
    twoPairs.refOff = {0, 1, 2}; twoPairs.refG = {0, 2}; twoPairs.qryOff = {0, 1, 2}; twoPairs.qryG = {1, 0}; twoPairs.plen = {12, 15};
    CHECK("apply_rejects_group_in_two_pairs", is(apply(g, twoPairs, p), "a group appears under two sides of one call"));
    twoPairs.plen = {12, 0};
    CHECK("apply_skipped_pair_does_not_count", apply(g, twoPairs, p) == nullptr && p.pair == V({0}));
    twoPairs.qryG = {1, 3}; twoPairs.plen = {12, 15};
    CHECK("apply_accepts_two_pairs", apply(g, twoPairs, p) == nullptr && p.pair == V({0, 1}) && p.rOff == std::vector<int64_t>({0, 17}) && p.qOff == std::vector<int64_t>({10, 29}) &&
                                     p.rankInts == 39 && p.src.srcOff == std::vector<int64_t>({0, 64}) && p.maxL == 12);
    c = one; c.refG = {4};
    CHECK("apply_rejects_group_4_of_4", is(apply(g, c, p), "group id out of range"));
    c = one; c.qryG = {-1};
    CHECK("apply_rejects_negative_group", is(apply(g, c, p), "group id out of range"));
    c = one; c.qryOff = {0, 0};
    CHECK("apply_rejects_side_without_groups", is(apply(g, c, p), "a side without groups"));
    c = one; c.refOff = {1, 0};
    CHECK("apply_rejects_decreasing_offsets", is(apply(g, c, p), "bad group table"));
    c = one; c.plen = {18};
    CHECK("apply_rejects_path_longer_than_both_sides", is(apply(g, c, p), "path_len outside [0, min(path_stride, ref width + qry width)]"));
    c = one; c.plen = {17};
    CHECK("apply_accepts_path_as_long_as_both_sides", apply(g, c, p) == nullptr);
    c = one; c.stride = 11;
    CHECK("apply_rejects_path_longer_than_stride", is(apply(g, c, p), "path_len outside [0, min(path_stride, ref width + qry width)]"));
    c = one; c.plen = {-1};
    CHECK("apply_rejects_negative_path_len", is(apply(g, c, p), "path_len outside [0, min(path_stride, ref width + qry width)]"));
    c = one; c.stride = 0;
    CHECK("apply_rejects_stride_0", is(apply(g, c, p), "bad argument"));
    c = one; c.havePaths = false;
    CHECK("apply_rejects_missing_host_rows", is(apply(g, c, p), "host rows missing"));
    c = one; c.finished = true;
    CHECK("apply_rejects_after_finish", is(apply(g, c, p), "twl_merge_apply after twl_merge_finish"));
    c = one; c.plen = {0};
    CHECK("apply_all_skipped_is_empty", apply(g, c, p) == nullptr && p.pair.empty() && p.jobs.empty());
    CHECK("apply_no_pairs", check_merge_apply(g, false, 0, nullptr, nullptr, nullptr, nullptr, false, nullptr, 0, nullptr, PathLevelView{}, p) == nullptr);

    // paths that stay on the device
    c = one; c.fromDp = {1};
    CHECK("apply_from_dp_needs_a_level", is(apply(g, c, p), "from_dp needs the prepared and aligned level of these pairs"));
    c.lv.prepared = true; c.lv.n_pairs = 2;
    CHECK("apply_from_dp_needs_the_level_of_these_pairs", is(apply(g, c, p), "from_dp needs the prepared and aligned level of these pairs"));
    c.lv.n_pairs = 1; c.lv.dp_stride = 24;
    CHECK("apply_from_dp_1_needs_a_dp_output", is(apply(g, c, p), "from_dp 1 without a DP output of that length"));
    c.lv.has_dp = true;
    CHECK("apply_accepts_from_dp_1", apply(g, c, p) == nullptr && p.src.which == std::vector<uint8_t>({1}) && p.src.hostRows.empty() && p.src.srcOff == std::vector<int64_t>({0}));
    c.lv.dp_stride = 11;
    CHECK("apply_from_dp_1_longer_than_the_dp_row", is(apply(g, c, p), "from_dp 1 without a DP output of that length"));
    c.lv.dp_stride = 24; c.fromDp = {2};
    CHECK("apply_from_dp_2_needs_a_restore", is(apply(g, c, p), "from_dp 2: twl_level_restore first, with this row pitch"));
    c.lv.staged_stride = 32;
    CHECK("apply_from_dp_2_needs_the_restore_pitch", is(apply(g, c, p), "from_dp 2: twl_level_restore first, with this row pitch"));
    c.lv.staged_stride = 64;
    CHECK("apply_accepts_from_dp_2", apply(g, c, p) == nullptr && p.src.which == std::vector<uint8_t>({2}));
    c.fromDp = {3};
    CHECK("apply_rejects_from_dp_3", is(apply(g, c, p), "from_dp must be 0, 1 or 2"));
    // the second pair of a level reads its own row of the level's buffers
    Call lvl = twoPairs;
    lvl.fromDp = {2, 1}; lvl.lv.prepared = true; lvl.lv.n_pairs = 2; lvl.lv.dp_stride = 24; lvl.lv.has_dp = true; lvl.lv.staged_stride = 64;
    CHECK("apply_level_rows", apply(g, lvl, p) == nullptr && p.src.srcOff == std::vector<int64_t>({0, 24}) && p.src.which == std::vector<uint8_t>({2, 1}));
}

static void finish_kats()
{
    MergeGroups g;
    create({0, 3, 5}, {0, 1, 2, 3, 4}, g);
    int32_t W = -1;
    CHECK("finish_rejects_unmerged_groups", is(check_merge_finish(g, false, kRowLen, &W), "the groups have not been merged to one width"));
    g.width = {15, 15};
    CHECK("finish_accepts_one_width", check_merge_finish(g, false, kRowLen, &W) == nullptr && W == 15);
    CHECK("finish_rejects_second_call", is(check_merge_finish(g, true, kRowLen, &W), "twl_merge_finish called twice"));
    int32_t moved[8];
    memcpy(moved, kRowLen, sizeof moved);
    moved[4] = 15;
    CHECK("finish_rejects_rewritten_row", is(check_merge_finish(g, false, moved, &W), "a row has been rewritten since the merge began"));
    MergeGroups single;
    create({0, 1}, {5}, single);
    CHECK("finish_single_group_keeps_its_width", check_merge_finish(single, false, kRowLen, &W) == nullptr && W == 12);
    MergeGroups none;
    create({0}, {}, none);
    CHECK("finish_no_groups", check_merge_finish(none, false, kRowLen, &W) == nullptr && W == 0);
}

int main()
{
    create_kats();
    apply_kats();
    finish_kats();
    printf("%d failed\n", g_fail);
    return g_fail ? 1 : 0;
}
