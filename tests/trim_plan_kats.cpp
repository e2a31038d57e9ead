// tests/trim_plan_kats.cpp -- known answers of what twl_store_trim_columns (include/twl_trim.h) decides on the host: every refusal of
// check_trim_columns and the grids of plan_trim_grid, pure functions in twilight_amd/csrc/twl_trim_plan.inc.hip (no HIP call: this program
// includes the file directly).  The expected answers restate include/twl_trim.h.  Prints "OK <name>" / "FAIL <name>".
#include <cstdio>
#include <cstring>
#include <string>
#include "../twilight_amd/csrc/twl_trim_plan.inc.hip"

static int g_fail = 0;
#define CHECK(name, cond) do { if (cond) printf("OK %s\n", name); else { printf("FAIL %s\n", name); ++g_fail; } } while (0)

using V = std::vector<int32_t>;
static bool is(const char *got, const char *want) { return got && want ? strcmp(got, want) == 0 : got == want; }

// a store of 8 rows: 0-3 have 70 columns, 4 and 5 have 33, 6 is empty, 7 has 5
static const int32_t kRowLen[8] = {70, 70, 70, 70, 33, 33, 0, 5};
static const int32_t kTile = 4096;

static const char *chk(int32_t n, const int32_t *ids, int32_t rule, int32_t arg, TrimRows &t, bool store = true, bool out = true, bool prepared = false, const int32_t *len = kRowLen)
{
    return check_trim_columns(store, n, ids, out, rule, arg, 8, len, prepared, kTile, t);
}

static void check_kats()
{
    TrimRows t;
    const V ids{3, 0, 2};
    CHECK("accepts_three_rows_rule_0", chk(3, ids.data(), 0, 1, t) == nullptr && t.W == 70 && t.refIndex == -1);
    CHECK("accepts_rule_0_limit_0", chk(3, ids.data(), 0, 0, t) == nullptr);
    CHECK("accepts_rule_0_limit_n", chk(3, ids.data(), 0, 3, t) == nullptr);
    CHECK("accepts_rule_1_first", chk(3, ids.data(), 1, 3, t) == nullptr && t.refIndex == 0 && t.W == 70);
    CHECK("accepts_rule_1_last", chk(3, ids.data(), 1, 2, t) == nullptr && t.refIndex == 2);
    CHECK("accepts_a_single_empty_row", chk(1, V({6}).data(), 0, 0, t) == nullptr && t.W == 0);
    CHECK("accepts_one_row_as_its_own_reference", chk(1, V({7}).data(), 1, 7, t) == nullptr && t.W == 5 && t.refIndex == 0);
    CHECK("rejects_null_store", is(chk(3, ids.data(), 0, 1, t, false), "bad argument"));
    CHECK("rejects_null_ids", is(chk(3, nullptr, 0, 1, t), "bad argument"));
    CHECK("rejects_null_output", is(chk(3, ids.data(), 0, 1, t, true, false), "bad argument"));
    CHECK("rejects_no_rows", is(chk(0, ids.data(), 0, 0, t), "no rows listed"));
    CHECK("rejects_a_negative_count", is(chk(-1, ids.data(), 0, 0, t), "no rows listed"));
    CHECK("rejects_id_8_of_8", is(chk(2, V({0, 8}).data(), 0, 1, t), "sequence id out of range"));
    CHECK("rejects_a_negative_id", is(chk(2, V({-1, 0}).data(), 0, 1, t), "sequence id out of range"));
    CHECK("rejects_an_id_twice", is(chk(3, V({0, 1, 0}).data(), 0, 1, t), "a sequence id is listed twice"));
    CHECK("rejects_two_lengths", is(chk(2, V({0, 4}).data(), 0, 1, t), "the listed rows differ in length"));
    CHECK("rejects_an_empty_row_beside_a_longer_one", is(chk(2, V({6, 7}).data(), 0, 1, t), "the listed rows differ in length"));
    CHECK("rejects_a_prepared_level", is(chk(3, ids.data(), 0, 1, t, true, true, true), "a level is still prepared on the store: commit it first"));
    CHECK("rejects_rule_2", is(chk(3, ids.data(), 2, 1, t), "unknown trim rule"));
    CHECK("rejects_rule_minus_1", is(chk(3, ids.data(), -1, 1, t), "unknown trim rule"));
    CHECK("rejects_a_negative_limit", is(chk(3, ids.data(), 0, -1, t), "the gap limit lies outside 0 .. n_ids"));
    CHECK("rejects_a_limit_above_n", is(chk(3, ids.data(), 0, 4, t), "the gap limit lies outside 0 .. n_ids"));
    CHECK("rejects_a_reference_outside_ids", is(chk(3, ids.data(), 1, 1, t), "the reference sequence is not among the listed rows"));
    CHECK("rejects_a_reference_outside_the_store", is(chk(3, ids.data(), 1, 8, t), "the reference sequence is not among the listed rows"));
    CHECK("rejects_a_negative_reference", is(chk(3, ids.data(), 1, -1, t), "the reference sequence is not among the listed rows"));
    // the width bound: INT32_MAX - tile is the last width whose last tile ends inside int32
    int32_t wide[8] = {INT32_MAX - kTile, INT32_MAX - kTile + 1, 0, 0, 0, 0, 0, 0};
    CHECK("width_bound", trim_max_width(kTile) == INT32_MAX - 4096);
    CHECK("accepts_the_widest_row", chk(1, V({0}).data(), 0, 0, t, true, true, false, wide) == nullptr && t.W == INT32_MAX - kTile);
    CHECK("rejects_one_column_more", is(chk(1, V({1}).data(), 0, 0, t, true, true, false, wide), "rows too long for twl_store_trim_columns"));
    // a refusal leaves an empty answer
    CHECK("a_refusal_fills_nothing", chk(2, V({0, 4}).data(), 1, 0, t) != nullptr && t.W == 0);
}

static bool grid_is(const TrimGrid &g, int32_t words, int32_t colTiles, int32_t rowSlices, int32_t colBlocks, int32_t rowsY, int32_t rowsZ)
{
    return g.words == words && g.colTiles == colTiles && g.rowSlices == rowSlices && g.colBlocks == colBlocks && g.rowsY == rowsY && g.rowsZ == rowsZ;
}

static void grid_kats()
{
    TrimGrid g;
    // column tile 4096, row slice 512, 256 threads
    CHECK("one_of_everything", plan_trim_grid(1, 1, 4096, 512, 256, g) == nullptr && grid_is(g, 1, 1, 1, 1, 1, 1));
    CHECK("no_column", plan_trim_grid(0, 3, 4096, 512, 256, g) == nullptr && grid_is(g, 0, 0, 1, 0, 3, 1));
    CHECK("exact_sizes", plan_trim_grid(4096, 512, 4096, 512, 256, g) == nullptr && grid_is(g, 128, 1, 1, 16, 512, 1));
    CHECK("one_past_each", plan_trim_grid(4097, 513, 4096, 512, 256, g) == nullptr && grid_is(g, 129, 2, 2, 17, 513, 1));
    CHECK("a_word_boundary", plan_trim_grid(33, 2, 4096, 512, 256, g) == nullptr && g.words == 2 && g.colBlocks == 1);
    CHECK("rows_fill_y", plan_trim_grid(10, 65535, 4096, 512, 256, g) == nullptr && g.rowsY == 65535 && g.rowsZ == 1 && g.rowSlices == 128);
    CHECK("rows_spill_into_z", plan_trim_grid(10, 65536, 4096, 512, 256, g) == nullptr && g.rowsY == 65535 && g.rowsZ == 2);
    CHECK("a_hundred_thousand_rows", plan_trim_grid(38524, 100000, 4096, 512, 256, g) == nullptr && grid_is(g, 1204, 10, 196, 151, 65535, 2));
    CHECK("the_widest_row_does_not_wrap", plan_trim_grid(INT32_MAX - 4096, 2, 4096, 512, 256, g) == nullptr && g.colTiles == 524287 && g.words == 67108736 && g.colBlocks == 8388592);
    CHECK("slices_fill_y", plan_trim_grid(10, 65535 * 512, 4096, 512, 256, g) == nullptr && g.rowSlices == 65535);
    CHECK("rejects_more_slices_than_y_holds", is(plan_trim_grid(10, 65535 * 512 + 1, 4096, 512, 256, g), "too many rows for twl_store_trim_columns"));
}

int main()
{
    check_kats();
    grid_kats();
    printf("%s\n", g_fail ? "SOME FAILED" : "ALL PASSED");
    return g_fail ? 1 : 0;
}
