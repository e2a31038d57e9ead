// tests/backbone_plan_kats.cpp -- known answers of what twl_store_squeeze_groups (include/twl_backbone.h) decides on the host: every refusal of
// check_squeeze_groups and the tile list of plan_squeeze_tiles, pure functions in twilight_amd/csrc/twl_backbone_plan.inc.hip (no HIP call: this
// program includes the file directly).  The expected answers restate include/twl_backbone.h.  Prints "OK <name>" / "FAIL <name>".
#include <cstdio>
#include <cstring>
#include <string>
#include "../twilight_amd/csrc/twl_backbone_plan.inc.hip"

static int g_fail = 0;
#define CHECK(name, cond) do { if (cond) printf("OK %s\n", name); else { printf("FAIL %s\n", name); ++g_fail; } } while (0)

using V = std::vector<int32_t>;
using V64 = std::vector<int64_t>;
static bool is(const char *got, const char *want) { return got && want ? strcmp(got, want) == 0 : got == want; }

// a store of 8 rows: 0-3 have 70 columns, 4 and 5 have 33, 6 is empty, 7 has 5
static const int32_t kRowLen[8] = {70, 70, 70, 70, 33, 33, 0, 5};

static void check_kats()
{
    SqueezeGroups g;
    const V off{0, 3, 5, 6}, ids{3, 0, 2, 5, 4, 6};
    CHECK("accepts_three_groups", check_squeeze_groups(3, off.data(), ids.data(), true, 8, kRowLen, false, g) == nullptr);
    CHECK("lengths_per_group", g.len == V({70, 33, 0}) && g.maxLen == 70);
    CHECK("row_groups", g.rowGroup == V({0, 0, 0, 1, 1, 2}));
    // 70 columns are 3 words, 33 are 2, 0 are none; the scan has one entry more per group
    CHECK("flag_offsets", g.flagOff == V64({0, 3, 5}) && g.flagWords == 5);
    CHECK("scan_offsets", g.preOff == V64({0, 4, 7}) && g.preInts == 8);
    CHECK("no_group_is_no_error", check_squeeze_groups(0, nullptr, nullptr, false, 8, kRowLen, false, g) == nullptr && g.len.empty() && g.flagWords == 0);
    CHECK("rejects_negative_count", is(check_squeeze_groups(-1, off.data(), ids.data(), true, 8, kRowLen, false, g), "bad argument"));
    CHECK("rejects_null_offsets", is(check_squeeze_groups(3, nullptr, ids.data(), true, 8, kRowLen, false, g), "bad argument"));
    CHECK("rejects_null_ids", is(check_squeeze_groups(3, off.data(), nullptr, true, 8, kRowLen, false, g), "bad argument"));
    CHECK("rejects_null_output", is(check_squeeze_groups(3, off.data(), ids.data(), false, 8, kRowLen, false, g), "bad argument"));
    CHECK("rejects_a_prepared_level", is(check_squeeze_groups(3, off.data(), ids.data(), true, 8, kRowLen, true, g), "a level is still prepared on the store: commit it first"));
    CHECK("rejects_a_prepared_level_without_groups", is(check_squeeze_groups(0, nullptr, nullptr, false, 8, kRowLen, true, g), "a level is still prepared on the store: commit it first"));
    CHECK("rejects_offsets_not_from_0", is(check_squeeze_groups(1, V({1, 3}).data(), ids.data(), true, 8, kRowLen, false, g), "group offsets must start at 0"));
    CHECK("rejects_descending_offsets", is(check_squeeze_groups(2, V({0, 3, 2}).data(), ids.data(), true, 8, kRowLen, false, g), "group offsets do not ascend"));
    CHECK("rejects_an_empty_group", is(check_squeeze_groups(2, V({0, 3, 3}).data(), ids.data(), true, 8, kRowLen, false, g), "an empty group"));
    CHECK("rejects_an_empty_first_group", is(check_squeeze_groups(2, V({0, 0, 3}).data(), ids.data(), true, 8, kRowLen, false, g), "an empty group"));
    CHECK("rejects_id_8_of_8", is(check_squeeze_groups(1, V({0, 2}).data(), V({0, 8}).data(), true, 8, kRowLen, false, g), "sequence id out of range"));
    CHECK("rejects_a_negative_id", is(check_squeeze_groups(1, V({0, 2}).data(), V({-1, 0}).data(), true, 8, kRowLen, false, g), "sequence id out of range"));
    CHECK("rejects_an_id_twice_in_a_group", is(check_squeeze_groups(1, V({0, 3}).data(), V({0, 1, 0}).data(), true, 8, kRowLen, false, g), "a sequence id is listed twice"));
    CHECK("rejects_an_id_in_two_groups", is(check_squeeze_groups(2, V({0, 2, 4}).data(), V({0, 1, 4, 1}).data(), true, 8, kRowLen, false, g), "a sequence id is listed twice"));
    CHECK("rejects_two_lengths_in_a_group", is(check_squeeze_groups(1, V({0, 2}).data(), V({0, 4}).data(), true, 8, kRowLen, false, g), "the rows of a group differ in length"));
    CHECK("rejects_an_empty_row_beside_a_longer_one", is(check_squeeze_groups(1, V({0, 2}).data(), V({6, 7}).data(), true, 8, kRowLen, false, g), "the rows of a group differ in length"));
    CHECK("accepts_a_single_empty_row", check_squeeze_groups(1, V({0, 1}).data(), V({6}).data(), true, 8, kRowLen, false, g) == nullptr && g.len == V({0}) && g.preInts == 1);
}

static bool same(const std::vector<SqueezeTilePlan> &got, const std::vector<SqueezeTilePlan> &want)
{
    if (got.size() != want.size()) return false;
    for (size_t k = 0; k < got.size(); ++k)
        if (got[k].group != want[k].group || got[k].col0 != want[k].col0 || got[k].row0 != want[k].row0 || got[k].row1 != want[k].row1) return false;
    return true;
}

static void tile_kats()
{
    // column tile 64, row slice 4
    const V one{0, 3};
    CHECK("one_tile", same(plan_squeeze_tiles(1, one.data(), V({10}).data(), 64, 4), {{0, 0, 0, 3}}));
    CHECK("one_tile_at_the_exact_size", same(plan_squeeze_tiles(1, V({0, 4}).data(), V({64}).data(), 64, 4), {{0, 0, 0, 4}}));
    CHECK("one_column_past_the_tile", same(plan_squeeze_tiles(1, V({0, 4}).data(), V({65}).data(), 64, 4), {{0, 0, 0, 4}, {0, 64, 0, 4}}));
    CHECK("one_row_past_the_slice", same(plan_squeeze_tiles(1, V({0, 5}).data(), V({64}).data(), 64, 4), {{0, 0, 0, 4}, {0, 0, 4, 5}}));
    CHECK("exact_multiples", same(plan_squeeze_tiles(1, V({0, 8}).data(), V({128}).data(), 64, 4), {{0, 0, 0, 4}, {0, 0, 4, 8}, {0, 64, 0, 4}, {0, 64, 4, 8}}));
    CHECK("one_past_both", same(plan_squeeze_tiles(1, V({0, 9}).data(), V({129}).data(), 64, 4),
                                {{0, 0, 0, 4}, {0, 0, 4, 8}, {0, 0, 8, 9}, {0, 64, 0, 4}, {0, 64, 4, 8}, {0, 64, 8, 9}, {0, 128, 0, 4}, {0, 128, 4, 8}, {0, 128, 8, 9}}));
    // groups in order; rows are positions in the id list; a group of length 0 has no tile
    CHECK("groups_in_order_and_none_for_length_0", same(plan_squeeze_tiles(3, V({0, 2, 7, 8}).data(), V({65, 0, 1}).data(), 64, 4), {{0, 0, 0, 2}, {0, 64, 0, 2}, {2, 0, 7, 8}}));
    CHECK("no_group_no_tile", plan_squeeze_tiles(0, V({0}).data(), nullptr, 64, 4).empty());
}

int main()
{
    check_kats();
    tile_kats();
    printf("%s\n", g_fail ? "SOME FAILED" : "ALL PASSED");
    return g_fail ? 1 : 0;
}
