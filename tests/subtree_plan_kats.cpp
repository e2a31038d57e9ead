// tests/subtree_plan_kats.cpp -- known answers of what twl_store_weighted_columns (include/twl_subtree.h) decides on the host:
// check_weighted_columns, a pure function in twilight_amd/csrc/twl_subtree_plan.inc.hip (no HIP call: this program includes the file
// directly).  The expected answers restate include/twl_subtree.h.  Prints "OK <name>" / "FAIL <name>".
#include <cstdio>
#include <cstring>
#include <vector>
#include "../twilight_amd/csrc/twl_subtree_plan.inc.hip"

static int g_fail = 0;
#define CHECK(name, cond) do { if (cond) printf("OK %s\n", name); else { printf("FAIL %s\n", name); ++g_fail; } } while (0)

using V = std::vector<int32_t>;
static bool is(const char *got, const char *want) { return got && want ? strcmp(got, want) == 0 : got == want; }

// a store of 8 rows: 0-2 and 5 have 10 columns, 3 has 7, 4 has 12, 6 is empty, 7 is empty
static const int32_t kRowLen[8] = {10, 10, 10, 7, 12, 10, 0, 0};
static const float kW[4] = {0.5f, 0.25f, 0.125f, 1.0f};

int main()
{
    int32_t L = -2;
    const V sub{2, 0, 5, 1};
    CHECK("accepts_rows_of_one_length_in_any_order", check_weighted_columns(4, sub.data(), kW, 3, false, 8, kRowLen, &L) == nullptr && L == 10);
    L = -2;
    CHECK("accepts_one_row", check_weighted_columns(1, V({4}).data(), kW, 0, false, 8, kRowLen, &L) == nullptr && L == 12);
    CHECK("accepts_the_last_id", check_weighted_columns(1, V({5}).data(), kW, 0, false, 6, kRowLen, &L) == nullptr && L == 10);
    CHECK("rejects_no_ids", is(check_weighted_columns(0, sub.data(), kW, 0, false, 8, kRowLen, &L), "bad argument"));
    CHECK("rejects_a_negative_count", is(check_weighted_columns(-1, sub.data(), kW, 0, false, 8, kRowLen, &L), "bad argument"));
    CHECK("rejects_null_ids", is(check_weighted_columns(4, nullptr, kW, 0, false, 8, kRowLen, &L), "bad argument"));
    CHECK("rejects_null_weights", is(check_weighted_columns(4, sub.data(), nullptr, 0, false, 8, kRowLen, &L), "bad argument"));
    CHECK("rejects_a_negative_cache_id", is(check_weighted_columns(4, sub.data(), kW, -1, false, 8, kRowLen, &L), "bad argument"));
    CHECK("rejects_a_cache_id_in_use", is(check_weighted_columns(4, sub.data(), kW, 3, true, 8, kRowLen, &L), "cache id in use"));
    CHECK("bad_argument_before_cache_id", is(check_weighted_columns(0, sub.data(), kW, 3, true, 8, kRowLen, &L), "bad argument"));
    CHECK("rejects_id_8_of_8", is(check_weighted_columns(2, V({0, 8}).data(), kW, 0, false, 8, kRowLen, &L), "sequence id out of range"));
    CHECK("rejects_a_negative_first_id", is(check_weighted_columns(2, V({-1, 0}).data(), kW, 0, false, 8, kRowLen, &L), "sequence id out of range"));
    CHECK("rejects_an_id_given_twice", is(check_weighted_columns(3, V({0, 1, 0}).data(), kW, 0, false, 8, kRowLen, &L), "sequence id given twice"));
    CHECK("rejects_an_id_given_twice_in_a_row", is(check_weighted_columns(2, V({5, 5}).data(), kW, 0, false, 8, kRowLen, &L), "sequence id given twice"));
    CHECK("rejects_rows_of_two_lengths", is(check_weighted_columns(3, V({0, 1, 3}).data(), kW, 0, false, 8, kRowLen, &L), "the rows of the profile differ in length"));
    CHECK("rejects_a_longer_row", is(check_weighted_columns(2, V({0, 4}).data(), kW, 0, false, 8, kRowLen, &L), "the rows of the profile differ in length"));
    CHECK("rejects_an_empty_row", is(check_weighted_columns(1, V({6}).data(), kW, 0, false, 8, kRowLen, &L), "the rows of the profile are empty"));
    CHECK("rejects_empty_rows", is(check_weighted_columns(2, V({6, 7}).data(), kW, 0, false, 8, kRowLen, &L), "the rows of the profile are empty"));
    CHECK("length_before_emptiness", is(check_weighted_columns(2, V({6, 0}).data(), kW, 0, false, 8, kRowLen, &L), "the rows of the profile differ in length"));
    CHECK("the_first_offence_in_list_order_is_named",is(check_weighted_columns(3, V({0, 3, 9}).data(), kW, 0, false, 8, kRowLen, &L), "the rows of the profile differ in length"));
    CHECK("range_of_the_first_id_first", is(check_weighted_columns(2, V({9, 3}).data(), kW, 0, false, 8, kRowLen, &L), "sequence id out of range"));
    return g_fail ? 1 : 0;
}
