// tests/retree_set_plan_kats.cpp -- known answers of what the twl_retree_set_* calls (include/twl_retree_set.h) decide on the host: the check_...
// functions, the slabs of rows and the tile list of the groups call, pure functions in twilight_amd/csrc/twl_retree_set_plan.inc.hip (no HIP
// call: this program includes the file directly).  The expected answers restate include/twl_retree_set.h and DESIGN.md section 4j.
// Prints "OK <name>" / "FAIL <name>".
#include <cstdio>
#include <cstring>
#include <numeric>
#include <vector>
#include "../twilight_amd/csrc/twl_retree_set_plan.inc.hip"

static int g_fail = 0;
#define CHECK(name, ...) do { if (__VA_ARGS__) printf("OK %s\n", name); else { printf("FAIL %s\n", name); ++g_fail; } } while (0)
static bool is(const char *got, const char *want) { return got && want ? strcmp(got, want) == 0 : got == want; }

// the plan of groups of these sizes, checked against the definition: tiles on or above the diagonal only, every one of them once, in order,
// block g at the sum of the earlier m^2
static bool plan_ok(const std::vector<int32_t> &sizes, size_t want_tiles)
{
    std::vector<int32_t> off{0};
    for (int32_t m : sizes) off.push_back(off.back() + m);
    const std::vector<GuideGroupTilePlan> tiles = plan_guide_groups((int32_t)sizes.size(), off.data(), 64);
    if (tiles.size() != want_tiles) return false;
    size_t at = 0;
    unsigned long long block = 0;
    for (size_t g = 0; g < sizes.size(); ++g) {
        const int32_t m = sizes[g], T = (m + 63) / 64;
        for (int32_t ti = 0; ti < T; ++ti)
            for (int32_t tj = ti; tj < T; ++tj, ++at) {
                if (at >= tiles.size()) return false;
                const GuideGroupTilePlan &t = tiles[at];
                if (t.first != off[g] || t.m != m || t.ti != ti || t.tj != tj || t.block != block) return false;
                if (t.ti > t.tj || t.tj * 64 >= m) return false;      // none below the diagonal, none outside the block
            }
        block += (unsigned long long)m * m;
    }
    return at == tiles.size();
}

// the slabs of n rows, at most max_rows each: they cover 0 .. n once, in order, none empty, none above max_rows, and their number is `want`
static bool slabs_ok(int32_t n, int32_t max_rows, int32_t want, int32_t want_last)
{
    if (retree_slabs(n, max_rows) != want) return false;
    int64_t at = 0;
    int32_t first = -1, count = -1;
    for (int32_t s = 0; s < want; ++s) {
        retree_slab(n, max_rows, s, &first, &count);
        if (first != at || count < 1 || count > max_rows) return false;
        at += count;
    }
    return at == n && count == want_last;
}

int main()
{
    const char *rows[3] = {"AC-T", "A-GT", "acgu"};
    void *handle = nullptr;
    int32_t kept = 0;
    // twl_retree_set_create
    CHECK("create_accepts_three_rows", check_retree_set_create('n', 3, 4, rows, 2, &handle, &kept) == nullptr);
    CHECK("create_accepts_protein", check_retree_set_create('p', 3, 4, rows, 0, &handle, &kept) == nullptr);
    CHECK("create_rejects_type_x", is(check_retree_set_create('x', 3, 4, rows, 2, &handle, &kept), "the type must be 'n' or 'p'"));
    CHECK("create_rejects_no_rows", is(check_retree_set_create('n', 0, 4, rows, 0, &handle, &kept), "no rows"));
    CHECK("create_rejects_no_columns", is(check_retree_set_create('n', 3, 0, rows, 2, &handle, &kept), "the rows have no columns"));
    CHECK("create_rejects_null_rows", is(check_retree_set_create('n', 3, 4, nullptr, 2, &handle, &kept), "bad argument"));
    const char *withNull[3] = {"AC-T", nullptr, "acgu"};
    CHECK("create_rejects_a_null_row", is(check_retree_set_create('n', 3, 4, withNull, 2, &handle, &kept), "bad argument"));
    CHECK("create_rejects_negative_max_gaps", is(check_retree_set_create('n', 3, 4, rows, -1, &handle, &kept), "max_gaps must lie in 0 .. n"));
    CHECK("create_rejects_max_gaps_above_n", is(check_retree_set_create('n', 3, 4, rows, 4, &handle, &kept), "max_gaps must lie in 0 .. n"));
    CHECK("create_accepts_max_gaps_of_n", check_retree_set_create('n', 3, 4, rows, 3, &handle, &kept) == nullptr);
    CHECK("create_rejects_a_null_handle", is(check_retree_set_create('n', 3, 4, rows, 2, nullptr, &kept), "bad argument"));
    CHECK("create_rejects_a_null_kept", is(check_retree_set_create('n', 3, 4, rows, 2, &handle, nullptr), "bad argument"));
    {
        std::vector<const char *> many(1048577, "A");
        CHECK("the_set_cap_is_2_to_the_20", kRetreeSetMaxSeqs == 1048576 && kRetreeMaxSeqs == 16384);
        CHECK("create_accepts_16385_rows", check_retree_set_create('n', 16385, 1, many.data(), 0, &handle, &kept) == nullptr);
        CHECK("create_accepts_1048576_rows", check_retree_set_create('n', 1048576, 1, many.data(), 1048576, &handle, &kept) == nullptr);
        CHECK("create_rejects_1048577_rows", is(check_retree_set_create('n', 1048577, 1, many.data(), 0, &handle, &kept), "more than 1048576 rows in a set"));
    }
    // twl_retree_set_assign on a set of 100 rows
    int32_t out[4] = {0};
    const int32_t seeds[3] = {5, 99, 0};
    CHECK("assign_accepts_seeds_in_any_order", check_retree_set_assign(true, 100, 3, seeds, out) == nullptr);
    CHECK("assign_accepts_one_seed", check_retree_set_assign(true, 100, 1, seeds, out) == nullptr);
    CHECK("assign_rejects_a_null_set", is(check_retree_set_assign(false, 0, 3, seeds, out), "bad argument"));
    CHECK("assign_rejects_null_seeds", is(check_retree_set_assign(true, 100, 3, nullptr, out), "bad argument"));
    CHECK("assign_rejects_a_null_output", is(check_retree_set_assign(true, 100, 3, seeds, nullptr), "bad argument"));
    CHECK("assign_rejects_no_seeds", is(check_retree_set_assign(true, 100, 0, seeds, out), "the number of seeds must be between 1 and 16384"));
    CHECK("assign_rejects_16385_seeds", is(check_retree_set_assign(true, 100000, 16385, seeds, out), "the number of seeds must be between 1 and 16384"));
    {
        std::vector<int32_t> all(16384);
        std::iota(all.begin(), all.end(), 0);
        CHECK("assign_accepts_16384_seeds", check_retree_set_assign(true, 16384, 16384, all.data(), out) == nullptr);
    }
    const int32_t past[3] = {5, 100, 0}, below[3] = {5, -1, 0}, twice[3] = {5, 0, 5};
    CHECK("assign_rejects_a_seed_past_the_set", is(check_retree_set_assign(true, 100, 3, past, out), "seed id out of range"));
    CHECK("assign_rejects_a_negative_seed", is(check_retree_set_assign(true, 100, 3, below, out), "seed id out of range"));
    CHECK("assign_rejects_the_same_seed_twice", is(check_retree_set_assign(true, 100, 3, twice, out), "the same row is a seed twice"));
    // twl_retree_set_pair_groups on a set of 100 rows
    uint64_t words = 0;
    const int32_t off[4] = {0, 2, 3, 6}, ids[6] = {9, 3, 99, 0, 3, 50};      // (a row may serve two groups)
    CHECK("groups_accepts_three_groups", check_retree_set_groups(true, 100, 3, off, ids, out, out, &words) == nullptr && words == 4 + 1 + 9);
    CHECK("groups_rejects_a_null_set", is(check_retree_set_groups(false, 0, 3, off, ids, out, out, &words), "bad argument"));
    CHECK("groups_rejects_null_offsets", is(check_retree_set_groups(true, 100, 3, nullptr, ids, out, out, &words), "bad argument"));
    CHECK("groups_rejects_null_ids", is(check_retree_set_groups(true, 100, 3, off, nullptr, out, out, &words), "bad argument"));
    CHECK("groups_rejects_a_null_match", is(check_retree_set_groups(true, 100, 3, off, ids, nullptr, out, &words), "bad argument"));
    CHECK("groups_rejects_a_null_both", is(check_retree_set_groups(true, 100, 3, off, ids, out, nullptr, &words), "bad argument"));
    CHECK("groups_rejects_no_groups", is(check_retree_set_groups(true, 100, 0, off, ids, out, out, &words), "no groups"));
    const int32_t late[4] = {1, 2, 3, 6}, empty[4] = {0, 2, 2, 6}, back[4] = {0, 3, 2, 6};
    CHECK("groups_rejects_a_first_offset_above_0", is(check_retree_set_groups(true, 100, 3, late, ids, out, out, &words), "the first group must start at 0"));
    CHECK("groups_rejects_an_empty_group", is(check_retree_set_groups(true, 100, 3, empty, ids, out, out, &words), "an empty group"));
    CHECK("groups_rejects_decreasing_offsets", is(check_retree_set_groups(true, 100, 3, back, ids, out, out, &words), "the group offsets decrease"));
    const int32_t idPast[6] = {9, 3, 100, 0, 3, 50}, idBelow[6] = {9, 3, 99, 0, -3, 50};
    CHECK("groups_rejects_an_id_past_the_set", is(check_retree_set_groups(true, 100, 3, off, idPast, out, out, &words), "row id out of range"));
    CHECK("groups_rejects_a_negative_id", is(check_retree_set_groups(true, 100, 3, off, idBelow, out, out, &words), "row id out of range"));
    {
        std::vector<int32_t> zeros(40000, 0);
        const int32_t cap[2] = {0, 16384}, over[2] = {0, 16385};
        CHECK("groups_accepts_a_group_of_16384", check_retree_set_groups(true, 100, 1, cap, zeros.data(), out, out, &words) == nullptr && words == (1ull << 28));
        CHECK("groups_rejects_a_group_of_16385", is(check_retree_set_groups(true, 100, 1, over, zeros.data(), out, out, &words), "a group of more than 16384 rows"));
        const int32_t fits[3] = {0, 16383, 16383 + 181}, toomany[3] = {0, 16384, 16385};
        CHECK("groups_accepts_2_to_the_28_entries", 16383ull * 16383 + 181ull * 181 <= (1ull << 28) && check_retree_set_groups(true, 100, 2, fits, zeros.data(), out, out, &words) == nullptr);
        CHECK("groups_rejects_one_entry_more", is(check_retree_set_groups(true, 100, 2, toomany, zeros.data(), out, out, &words), "the groups' matrices hold more than 2^28 entries each"));
    }
    // the tile list: T (T + 1) / 2 tiles for a group of T rows of tiles
    CHECK("plan_group_of_1", plan_ok({1}, 1));
    CHECK("plan_group_of_2", plan_ok({2}, 1));
    CHECK("plan_group_of_63", plan_ok({63}, 1));
    CHECK("plan_group_of_64", plan_ok({64}, 1));
    CHECK("plan_group_of_65", plan_ok({65}, 3));
    CHECK("plan_group_of_130", plan_ok({130}, 6));
    CHECK("plan_all_sizes_in_one_call", plan_ok({65, 1, 130, 2, 64, 63}, 3 + 1 + 6 + 1 + 1 + 1));
    // the slabs of the pack launches: blockIdx.y holds at most 65535 rows
    CHECK("the_pack_slab_is_65535_rows", kRetreePackMaxRows == 65535);
    CHECK("slabs_of_1_row", slabs_ok(1, kRetreePackMaxRows, 1, 1));
    CHECK("slabs_of_65535_rows", slabs_ok(65535, kRetreePackMaxRows, 1, 65535));
    CHECK("slabs_of_65536_rows", slabs_ok(65536, kRetreePackMaxRows, 2, 1));
    CHECK("slabs_of_131071_rows", slabs_ok(131071, kRetreePackMaxRows, 3, 1));
    CHECK("slabs_of_131070_rows", slabs_ok(131070, kRetreePackMaxRows, 2, 65535));
    CHECK("slabs_of_the_cap", slabs_ok(1048576, kRetreePackMaxRows, 17, 1048576 - 16 * 65535));
    {
        int32_t first = 0, count = 0;
        retree_slab(131071, kRetreePackMaxRows, 1, &first, &count);
        CHECK("second_slab_of_131071_rows", first == 65535 && count == 65535);
        retree_slab(131071, kRetreePackMaxRows, 2, &first, &count);
        CHECK("third_slab_of_131071_rows", first == 131070 && count == 1);
    }
    // the staged host block: 64 MiB, at least one row, at most all rows
    CHECK("stage_rows_narrow", retree_stage_rows(100, 70) == 100);
    CHECK("stage_rows_wide", retree_stage_rows(100000, 1600) == 41943 && slabs_ok(100000, 41943, 3, 100000 - 2 * 41943));
    CHECK("stage_rows_wider_than_the_block", retree_stage_rows(5, 2147483647) == 1);
    // bytes: rows + gap counts + planes + letters while the set is made; planes + letters stay
    CHECK("bytes_of_a_set", retree_set_stay_bytes('n', 10, 8) == 10ull * 3 * 8 * 8 + 40 && retree_set_create_bytes('n', 10, 70, 8) == 700 + 280 + 10ull * 3 * 8 * 8 + 40);
    CHECK("bytes_of_a_protein_set", retree_set_stay_bytes('p', 1048576, 32) == 1048576ull * 6 * 32 * 8 + 1048576ull * 4);
    return g_fail ? 1 : 0;
}
