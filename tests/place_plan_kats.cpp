// tests/place_plan_kats.cpp -- known answers of what the calls of include/twl_place.h decide on the host: check_count_columns / check_place_create /
// check_place_collect / place_collect_done / check_place_finish, pure functions in twilight_amd/csrc/twl_place_plan.inc.hip (no HIP call: this program
// includes the file directly).  The expected answers restate include/twl_place.h.  The refusals of the path source itself (from_dp 1 / 2 / 3 and what
// they need of the level, twl_path_source.inc.hip) have their known answers in tests/merge_plan_kats.cpp, once for both callers; here every one of them
// is reached once through a collect.  Prints "OK <name>" / "FAIL <name>".
#include <cstdio>
#include <cstring>
#include <string>
#include "../twilight_amd/csrc/twl_place_plan.inc.hip"

static int g_fail = 0;
#define CHECK(name, cond) do { if (cond) printf("OK %s\n", name); else { printf("FAIL %s\n", name); ++g_fail; } } while (0)

using V = std::vector<int32_t>;
using V64 = std::vector<int64_t>;
using V8 = std::vector<uint8_t>;
static bool is(const char *got, const char *want) { return got && want ? strcmp(got, want) == 0 : got == want; }

// a store of 8 rows: 0-2 are backbone rows of 10 columns, 3 is a sequence of 7, 4 of 12, 5 of 10, 6 is empty, 7 of 3
static const int32_t kRowLen[8] = {10, 10, 10, 7, 12, 10, 0, 3};

static void count_kats()
{
    int32_t L = -2;
    const V bb{0, 1, 2};
    CHECK("count_accepts_the_backbone", check_count_columns(3, bb.data(), 0, false, 8, kRowLen, &L) == nullptr && L == 10);
    CHECK("count_accepts_an_empty_row", check_count_columns(1, V({6}).data(), 4, false, 8, kRowLen, &L) == nullptr && L == 0);
    CHECK("count_rejects_no_ids", is(check_count_columns(0, bb.data(), 0, false, 8, kRowLen, &L), "bad argument"));
    CHECK("count_rejects_null_ids", is(check_count_columns(3, nullptr, 0, false, 8, kRowLen, &L), "bad argument"));
    CHECK("count_rejects_negative_cache_id", is(check_count_columns(3, bb.data(), -1, false, 8, kRowLen, &L), "bad argument"));
    CHECK("count_rejects_cache_id_in_use", is(check_count_columns(3, bb.data(), 0, true, 8, kRowLen, &L), "cache id in use"));
    CHECK("count_bad_argument_before_cache_id", is(check_count_columns(0, bb.data(), 0, true, 8, kRowLen, &L), "bad argument"));
    CHECK("count_rejects_id_8_of_8", is(check_count_columns(2, V({0, 8}).data(), 0, false, 8, kRowLen, &L), "sequence id out of range"));
    CHECK("count_rejects_negative_first_id", is(check_count_columns(2, V({-1, 0}).data(), 0, false, 8, kRowLen, &L), "sequence id out of range"));
    CHECK("count_rejects_rows_of_two_lengths", is(check_count_columns(3, V({0, 1, 3}).data(), 0, false, 8, kRowLen, &L), "the rows to count differ in length"));
}

static PlaceBook book(int32_t L = 10)
{
    PlaceBook b;
    int64_t bytes = -1;
    check_place_create(L, 8, kRowLen, b, &bytes);
    return b;
}

static void create_kats()
{
    PlaceBook b;
    int64_t bytes = -1;
    CHECK("create_accepts", check_place_create(10, 8, kRowLen, b, &bytes) == nullptr && b.L == 10 && !b.finished && b.placed.empty());
    CHECK("create_slots", b.slot == V64({0, 20, 40, 60, 77, 99, 119, 129}) && bytes == 142);
    CHECK("create_nothing_collected", b.plen == V(8, -1) && b.qlen == V(kRowLen, kRowLen + 8));
    CHECK("create_accepts_L_0", check_place_create(0, 8, kRowLen, b, &bytes) == nullptr && bytes == 62);
    CHECK("create_rejects_negative_L", is(check_place_create(-1, 8, kRowLen, b, &bytes), "bad argument"));
}

struct Call {
    V ids, plen;
    int32_t stride = 64;
    V8 fromDp;
    bool havePaths = true;
    PathLevelView lv;
    const int32_t *rowLen = kRowLen;
};
static const char *collect(const PlaceBook &b, const Call &c, PlaceCollectPlan &p)
{
    return check_place_collect(b, (int32_t)c.ids.size(), c.ids.data(), c.havePaths, c.plen.data(), c.stride, c.fromDp.empty() ? nullptr : c.fromDp.data(), 8, c.rowLen, c.lv, p);
}

static void collect_kats()
{
    const PlaceBook b = book();
    PlaceCollectPlan p;
    Call one;
    one.ids = {3}; one.plen = {12};
    CHECK("collect_accepts_one_host_row", collect(b, one, p) == nullptr && p.ids == V({3}) && p.plen == V({12}) && p.qlen == V({7}) && p.dstOff == V64({60}));
    CHECK("collect_host_row_source", p.src.which == V8({0}) && p.src.srcOff == V64({0}) && p.src.hostRows == V({0}));

    // four pairs of a level, sources 2, 0, (skipped), 1: the host row is the first upload, the level's rows are addressed by the pair's index
    Call four;
    four.ids = {4, 3, 5, 7}; four.plen = {15, 11, 0, 13}; four.fromDp = {2, 0, 1, 1};
    four.lv.prepared = true; four.lv.n_pairs = 4; four.lv.dp_stride = 24; four.lv.has_dp = true; four.lv.staged_stride = 64;
    CHECK("collect_accepts_four_pairs", collect(b, four, p) == nullptr);
    CHECK("collect_four_taking_pairs", p.ids == V({4, 3, 7}) && p.plen == V({15, 11, 13}) && p.qlen == V({12, 7, 3}) && p.dstOff == V64({77, 60, 129}));
    CHECK("collect_four_sources", p.src.which == V8({2, 0, 1}) && p.src.srcOff == V64({0, 0, 3 * 24}) && p.src.hostRows == V({1}));
    Call twoHost = four;
    twoHost.fromDp = {0, 2, 1, 0};
    CHECK("collect_host_rows_pack_in_upload_order", collect(b, twoHost, p) == nullptr && p.src.which == V8({0, 2, 0}) && p.src.srcOff == V64({0, 64, 64}) &&
                                                     p.src.hostRows == V({0, 3}));

    // one bad flag: the other paths are collected, in order; what was collected cannot be collected again
    PlaceBook b1 = b;
    collect(b1, four, p);
    const int32_t bad[3] = {0, 1, 0};
    CHECK("done_counts_the_bad_path", place_collect_done(b1, p, bad) == 1);
    CHECK("done_marks_the_passed_paths", b1.placed == V({4, 7}) && b1.plen == V({-1, -1, -1, -1, 15, -1, -1, 13}));
    Call again;
    again.ids = {3}; again.plen = {11};
    CHECK("collect_accepts_the_refused_sequence_again", collect(b1, again, p) == nullptr);
    again.ids = {7};
    CHECK("collect_rejects_collected_sequence", is(collect(b1, again, p), "sequence collected twice"));
    const int32_t none[3] = {0, 0, 0};
    PlaceBook b2 = b;
    collect(b2, four, p);
    CHECK("done_all_passed", place_collect_done(b2, p, none) == 0 && b2.placed == V({4, 3, 7}));

    Call c = one;
    c.stride = 0;
    CHECK("collect_rejects_stride_0", is(collect(b, c, p), "bad argument"));
    CHECK("collect_rejects_negative_count", is(check_place_collect(b, -1, nullptr, false, nullptr, 1, nullptr, 8, kRowLen, PathLevelView{}, p), "bad argument"));
    CHECK("collect_rejects_null_ids", is(check_place_collect(b, 1, nullptr, true, one.plen.data(), 64, nullptr, 8, kRowLen, PathLevelView{}, p), "bad argument"));
    CHECK("collect_no_pairs", check_place_collect(b, 0, nullptr, false, nullptr, 0, nullptr, 8, kRowLen, PathLevelView{}, p) == nullptr && p.ids.empty());
    PlaceBook fin = b;
    fin.finished = true;
    CHECK("collect_rejects_after_finish", is(collect(fin, one, p), "twl_place_collect after twl_place_finish"));
    c = one; c.ids = {8};
    CHECK("collect_rejects_id_8_of_8", is(collect(b, c, p), "sequence id out of range"));
    c = one; c.ids = {-1};
    CHECK("collect_rejects_negative_id", is(collect(b, c, p), "sequence id out of range"));
    c = one; c.ids = {8}; c.plen = {0};
    CHECK("collect_skipped_pair_is_not_looked_at", collect(b, c, p) == nullptr && p.ids.empty());
    c = one; c.ids = {3, 3}; c.plen = {12, 12};
    CHECK("collect_rejects_sequence_twice_in_a_call", is(collect(b, c, p), "sequence collected twice"));
    int32_t moved[8];
    memcpy(moved, kRowLen, sizeof moved);
    moved[3] = 17;
    c = one; c.rowLen = moved;
    CHECK("collect_rejects_rewritten_row", is(collect(b, c, p), "the sequence's row has been rewritten since the placement began"));
    c = one; c.plen = {18};
    CHECK("collect_rejects_path_longer_than_L_plus_len", is(collect(b, c, p), "path_len outside [0, min(path_stride, L + len)]"));
    c = one; c.plen = {17};
    CHECK("collect_accepts_path_of_L_plus_len", collect(b, c, p) == nullptr);
    c = one; c.stride = 11;
    CHECK("collect_rejects_path_longer_than_stride", is(collect(b, c, p), "path_len outside [0, min(path_stride, L + len)]"));
    c = one; c.plen = {-1};
    CHECK("collect_rejects_negative_path_len", is(collect(b, c, p), "path_len outside [0, min(path_stride, L + len)]"));
    c = one; c.havePaths = false;
    CHECK("collect_rejects_missing_host_rows", is(collect(b, c, p), "host rows missing"));

    // paths that stay on the device: each refusal of the source once, and the level check in front of every per-pair check
    c = one; c.fromDp = {1};
    CHECK("collect_from_dp_needs_a_level", is(collect(b, c, p), "from_dp needs the prepared and aligned level of these pairs"));
    c.ids = {8};
    CHECK("collect_level_check_comes_before_the_pairs", is(collect(b, c, p), "from_dp needs the prepared and aligned level of these pairs"));
    c = one; c.fromDp = {1}; c.lv.prepared = true; c.lv.n_pairs = 2;
    CHECK("collect_from_dp_needs_the_level_of_these_pairs", is(collect(b, c, p), "from_dp needs the prepared and aligned level of these pairs"));
    c.lv.n_pairs = 1; c.lv.dp_stride = 24;
    CHECK("collect_from_dp_1_needs_a_dp_output", is(collect(b, c, p), "from_dp 1 without a DP output of that length"));
    c.lv.has_dp = true;
    CHECK("collect_accepts_from_dp_1", collect(b, c, p) == nullptr && p.src.which == V8({1}) && p.src.hostRows.empty());
    c.fromDp = {2};
    CHECK("collect_from_dp_2_needs_a_restore", is(collect(b, c, p), "from_dp 2: twl_level_restore first, with this row pitch"));
    c.fromDp = {3};
    CHECK("collect_rejects_from_dp_3", is(collect(b, c, p), "from_dp must be 0, 1 or 2"));
    c.plen = {18};
    CHECK("collect_path_len_comes_before_the_source", is(collect(b, c, p), "path_len outside [0, min(path_stride, L + len)]"));
}

static void finish_kats()
{
    PlaceBook b = book();
    PlaceCollectPlan p;
    Call two;
    two.ids = {3, 4}; two.plen = {12, 14};
    collect(b, two, p);
    const int32_t none[2] = {0, 0};
    place_collect_done(b, p, none);
    const V bb{0, 1, 2};
    CHECK("finish_accepts_the_backbone", check_place_finish(b, 3, bb.data(), 8, kRowLen) == nullptr);
    CHECK("finish_accepts_no_backbone", check_place_finish(b, 0, nullptr, 8, kRowLen) == nullptr);
    CHECK("finish_accepts_an_uncollected_row_of_length_L", check_place_finish(b, 2, V({0, 5}).data(), 8, kRowLen) == nullptr);
    CHECK("finish_rejects_negative_count", is(check_place_finish(b, -1, bb.data(), 8, kRowLen), "bad argument"));
    CHECK("finish_rejects_null_ids", is(check_place_finish(b, 3, nullptr, 8, kRowLen), "bad argument"));
    PlaceBook fin = b;
    fin.finished = true;
    CHECK("finish_rejects_second_call", is(check_place_finish(fin, 3, bb.data(), 8, kRowLen), "twl_place_finish called twice"));
    CHECK("finish_rejects_id_8_of_8", is(check_place_finish(b, 2, V({0, 8}).data(), 8, kRowLen), "backbone id out of range or not of length L"));
    CHECK("finish_rejects_negative_id", is(check_place_finish(b, 1, V({-1}).data(), 8, kRowLen), "backbone id out of range or not of length L"));
    CHECK("finish_rejects_row_not_of_length_L", is(check_place_finish(b, 2, V({0, 7}).data(), 8, kRowLen), "backbone id out of range or not of length L"));
    CHECK("finish_rejects_backbone_id_twice", is(check_place_finish(b, 3, V({0, 1, 0}).data(), 8, kRowLen), "a backbone id is listed twice or was collected"));
    // sequence 5 is 10 long, as the backbone is: collected, it cannot be a backbone row as well
    PlaceBook b5 = b;
    Call five;
    five.ids = {5}; five.plen = {10};
    collect(b5, five, p);
    place_collect_done(b5, p, none);
    CHECK("finish_rejects_collected_backbone_id", is(check_place_finish(b5, 2, V({0, 5}).data(), 8, kRowLen), "a backbone id is listed twice or was collected"));
    int32_t moved[8];
    memcpy(moved, kRowLen, sizeof moved);
    moved[4] = 20;
    CHECK("finish_rejects_rewritten_placed_row", is(check_place_finish(b, 3, bb.data(), 8, moved), "a placed sequence's row has been rewritten since it was collected"));
    CHECK("width_accepts_L_and_more", check_place_width(b, 10) == nullptr && check_place_width(b, 31) == nullptr);
    CHECK("width_rejects_less_than_L", is(check_place_width(b, 9), "final width below the backbone's"));
}

int main()
{
    count_kats();
    create_kats();
    collect_kats();
    finish_kats();
    printf("%d failed\n", g_fail);
    return g_fail ? 1 : 0;
}
