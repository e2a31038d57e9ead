// tests/guide_set_plan_kats.cpp -- known answers of what the twl_guide_set_* calls (include/twl_guide.h) decide on the host: the check_...
// functions and plan_guide_groups, pure functions in twilight_amd/csrc/twl_guide_set_plan.inc.hip (no HIP call: this program includes the
// file directly).  The expected answers restate include/twl_guide.h and DESIGN.md section 4g.  Prints "OK <name>" / "FAIL <name>".
#include <cstdio>
#include <cstring>
#include <numeric>
#include <vector>
#include "../twilight_amd/csrc/twl_guide_set_plan.inc.hip"

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

int main()
{
    const char *seqs[3] = {"ACGTACGT", "", "ACG"};
    const int32_t lens[3] = {8, 0, 3};
    void *handle = nullptr;
    uint64_t total = 99;
    // twl_guide_set_create
    CHECK("create_accepts_three_sequences", check_guide_set_create('n', 3, seqs, lens, &handle, &total) == nullptr && total == 11);
    CHECK("create_rejects_type_x", is(check_guide_set_create('x', 3, seqs, lens, &handle, &total), "the type must be 'n' or 'p'"));
    CHECK("create_rejects_no_sequences", is(check_guide_set_create('n', 0, seqs, lens, &handle, &total), "no sequences"));
    CHECK("create_rejects_null_sequences", is(check_guide_set_create('n', 3, nullptr, lens, &handle, &total), "bad argument"));
    CHECK("create_rejects_null_lengths", is(check_guide_set_create('n', 3, seqs, nullptr, &handle, &total), "bad argument"));
    CHECK("create_rejects_a_null_handle", is(check_guide_set_create('n', 3, seqs, lens, nullptr, &total), "bad argument"));
    const int32_t neg[3] = {8, -1, 3};
    CHECK("create_rejects_a_negative_length", is(check_guide_set_create('p', 3, seqs, neg, &handle, &total), "negative sequence length"));
    const char *withNull[2] = {"ACGT", nullptr};
    const int32_t fullLast[2] = {4, 2};
    CHECK("create_rejects_a_null_sequence_with_letters", is(check_guide_set_create('n', 2, withNull, fullLast, &handle, &total), "bad argument"));
    {
        std::vector<const char *> many(1048577, "");
        std::vector<int32_t> zeros(1048577, 0);
        CHECK("the_set_cap_is_2_to_the_20", kGuideSetMaxSeqs == 1048576);
        CHECK("create_accepts_16385_sequences", check_guide_set_create('n', 16385, many.data(), zeros.data(), &handle, &total) == nullptr);
        CHECK("create_accepts_1048576_sequences", check_guide_set_create('n', 1048576, many.data(), zeros.data(), &handle, &total) == nullptr && total == 0);
        CHECK("create_rejects_1048577_sequences", is(check_guide_set_create('n', 1048577, many.data(), zeros.data(), &handle, &total), "more than 1048576 sequences in a set"));
    }
    // twl_guide_set_assign on a set of 100 sequences
    int32_t out[4] = {0};
    const int32_t seeds[3] = {5, 99, 0};
    CHECK("assign_accepts_seeds_in_any_order", check_guide_set_assign(true, 100, 3, seeds, out) == nullptr);
    CHECK("assign_accepts_one_seed", check_guide_set_assign(true, 100, 1, seeds, out) == nullptr);
    CHECK("assign_rejects_a_null_set", is(check_guide_set_assign(false, 0, 3, seeds, out), "bad argument"));
    CHECK("assign_rejects_null_seeds", is(check_guide_set_assign(true, 100, 3, nullptr, out), "bad argument"));
    CHECK("assign_rejects_a_null_output", is(check_guide_set_assign(true, 100, 3, seeds, nullptr), "bad argument"));
    CHECK("assign_rejects_no_seeds", is(check_guide_set_assign(true, 100, 0, seeds, out), "the number of seeds must be between 1 and 16384"));
    CHECK("assign_rejects_16385_seeds", is(check_guide_set_assign(true, 100000, 16385, seeds, out), "the number of seeds must be between 1 and 16384"));
    {
        std::vector<int32_t> all(16384);
        std::iota(all.begin(), all.end(), 0);
        CHECK("assign_accepts_16384_seeds", check_guide_set_assign(true, 16384, 16384, all.data(), out) == nullptr);
    }
    const int32_t past[3] = {5, 100, 0}, below[3] = {5, -1, 0}, twice[3] = {5, 0, 5};
    CHECK("assign_rejects_a_seed_past_the_set", is(check_guide_set_assign(true, 100, 3, past, out), "seed id out of range"));
    CHECK("assign_rejects_a_negative_seed", is(check_guide_set_assign(true, 100, 3, below, out), "seed id out of range"));
    CHECK("assign_rejects_the_same_seed_twice", is(check_guide_set_assign(true, 100, 3, twice, out), "the same sequence is a seed twice"));
    // twl_guide_set_shared_groups on a set of 100 sequences
    uint64_t words = 0;
    const int32_t off[4] = {0, 2, 3, 6}, ids[6] = {9, 3, 99, 0, 3, 50};      // (an id may serve two groups)
    CHECK("groups_accepts_three_groups", check_guide_set_groups(true, 100, 3, off, ids, out, &words) == nullptr && words == 4 + 1 + 9);
    CHECK("groups_rejects_a_null_set", is(check_guide_set_groups(false, 0, 3, off, ids, out, &words), "bad argument"));
    CHECK("groups_rejects_null_offsets", is(check_guide_set_groups(true, 100, 3, nullptr, ids, out, &words), "bad argument"));
    CHECK("groups_rejects_null_ids", is(check_guide_set_groups(true, 100, 3, off, nullptr, out, &words), "bad argument"));
    CHECK("groups_rejects_a_null_output", is(check_guide_set_groups(true, 100, 3, off, ids, nullptr, &words), "bad argument"));
    CHECK("groups_rejects_no_groups", is(check_guide_set_groups(true, 100, 0, off, ids, out, &words), "no groups"));
    const int32_t late[4] = {1, 2, 3, 6}, empty[4] = {0, 2, 2, 6}, back[4] = {0, 3, 2, 6};
    CHECK("groups_rejects_a_first_offset_above_0", is(check_guide_set_groups(true, 100, 3, late, ids, out, &words), "the first group must start at 0"));
    CHECK("groups_rejects_an_empty_group", is(check_guide_set_groups(true, 100, 3, empty, ids, out, &words), "an empty group"));
    CHECK("groups_rejects_decreasing_offsets", is(check_guide_set_groups(true, 100, 3, back, ids, out, &words), "the group offsets decrease"));
    const int32_t idPast[6] = {9, 3, 100, 0, 3, 50}, idBelow[6] = {9, 3, 99, 0, -3, 50};
    CHECK("groups_rejects_an_id_past_the_set", is(check_guide_set_groups(true, 100, 3, off, idPast, out, &words), "sequence id out of range"));
    CHECK("groups_rejects_a_negative_id", is(check_guide_set_groups(true, 100, 3, off, idBelow, out, &words), "sequence id out of range"));
    {
        std::vector<int32_t> zeros(40000, 0);
        const int32_t cap[2] = {0, 16384}, over[2] = {0, 16385};
        CHECK("groups_accepts_a_group_of_16384", check_guide_set_groups(true, 100, 1, cap, zeros.data(), out, &words) == nullptr && words == (1ull << 28));
        CHECK("groups_rejects_a_group_of_16385", is(check_guide_set_groups(true, 100, 1, over, zeros.data(), out, &words), "a group of more than 16384 sequences"));
        const int32_t fits[3] = {0, 16383, 16383 + 181}, toomany[3] = {0, 16384, 16385};
        CHECK("groups_accepts_2_to_the_28_entries", 16383ull * 16383 + 181ull * 181 <= (1ull << 28) && check_guide_set_groups(true, 100, 2, fits, zeros.data(), out, &words) == nullptr);
        CHECK("groups_rejects_one_entry_more", is(check_guide_set_groups(true, 100, 2, toomany, zeros.data(), out, &words), "the groups' matrices hold more than 2^28 entries together"));
    }
    // plan_guide_groups: T (T + 1) / 2 tiles for a group of T rows of tiles
    CHECK("plan_group_of_1", plan_ok({1}, 1));
    CHECK("plan_group_of_2", plan_ok({2}, 1));
    CHECK("plan_group_of_63", plan_ok({63}, 1));
    CHECK("plan_group_of_64", plan_ok({64}, 1));
    CHECK("plan_group_of_65", plan_ok({65}, 3));
    CHECK("plan_group_of_130", plan_ok({130}, 6));
    CHECK("plan_all_sizes_in_one_call", plan_ok({65, 1, 130, 2, 64, 63}, 3 + 1 + 6 + 1 + 1 + 1));
    CHECK("plan_300_groups_of_1", plan_ok(std::vector<int32_t>(300, 1), 300));
    {
        std::vector<int32_t> off2{0, 65, 66, 196};
        const std::vector<GuideGroupTilePlan> t = plan_guide_groups(3, off2.data(), 64);
        CHECK("plan_block_offsets", t.size() == 10 && t[0].block == 0 && t[3].block == 65ull * 65 && t[4].block == 65ull * 65 + 1 && t[9].block == 65ull * 65 + 1 && t[9].ti == 2 && t[9].tj == 2);
    }
    return g_fail ? 1 : 0;
}
