// tests/compare_plan_kats.cpp -- known answers of what twl_compare_create (include/twl_compare.h) decides on the host from its arguments alone:
// every refusal of plan_compare, the pitches, the byte counts and the 64-bit offsets, pure functions in
// twilight_amd/csrc/twl_compare_plan.inc.hip (no HIP call: this program includes the file directly; nothing is allocated).  The expected
// answers restate include/twl_compare.h.  Prints "OK <name>" / "FAIL <name>".
#include <cstdio>
#include <cstring>
#include "../twilight_amd/csrc/twl_compare_plan.inc.hip"

static int g_fail = 0;
#define CHECK(name, cond) do { if (cond) printf("OK %s\n", name); else { printf("FAIL %s\n", name); ++g_fail; } } while (0)

static bool is(const char *got, const char *want) { return got && want ? strcmp(got, want) == 0 : got == want; }

static const int32_t kTile = 64, kChunk = 1024;

static const char *plan(int32_t n, int32_t we, int32_t wr, ComparePlan &p, bool est = true, bool ref = true, bool cmp = true, bool bad = true)
{
    return plan_compare(n, we, est, wr, ref, cmp, bad, kTile, kChunk, p);
}

int main()
{
    ComparePlan p;
    CHECK("accepts_two_rows", plan(2, 5, 7, p) == nullptr && p.n == 2 && p.we == 5 && p.wr == 7 && p.pe == 64 && p.pr == 64 && p.colTiles == 1);
    CHECK("accepts_width_0", plan(2, 0, 0, p) == nullptr && p.pe == 0 && p.pr == 0 && p.colTiles == 0 && p.keyBytes == 0);
    CHECK("accepts_2_to_the_20_rows", plan(1 << 20, 3, 3, p) == nullptr && p.keyBytes == (uint64_t)(1 << 20) * 64u * 4u);
    CHECK("rejects_null_estimate", is(plan(2, 5, 7, p, false), "bad argument"));
    CHECK("rejects_null_reference", is(plan(2, 5, 7, p, true, false), "bad argument"));
    CHECK("rejects_null_object", is(plan(2, 5, 7, p, true, true, false), "bad argument"));
    CHECK("rejects_null_bad_row", is(plan(2, 5, 7, p, true, true, true, false), "bad argument"));
    CHECK("rejects_one_row", is(plan(1, 5, 7, p), "a comparison needs at least 2 rows"));
    CHECK("rejects_no_row", is(plan(0, 5, 7, p), "a comparison needs at least 2 rows"));
    CHECK("rejects_a_negative_count", is(plan(-3, 5, 7, p), "a comparison needs at least 2 rows"));
    CHECK("rejects_one_row_too_many", is(plan((1 << 20) + 1, 5, 7, p), "too many rows for twl_compare_create (at most 2^20)"));
    CHECK("rejects_a_negative_estimate_width", is(plan(2, -1, 7, p), "negative width"));
    CHECK("rejects_a_negative_reference_width", is(plan(2, 5, -1, p), "negative width"));
    CHECK("the_bound_is_that_of_a_scan_round", compare_max_width(kChunk) == INT32_MAX - kChunk);
    CHECK("accepts_the_widest_estimate", plan(2, INT32_MAX - kChunk, 7, p) == nullptr && p.pe == ((int64_t)INT32_MAX - kChunk + 63) / 64 * 64);
    CHECK("accepts_the_widest_reference", plan(2, 5, INT32_MAX - kChunk, p) == nullptr);
    CHECK("rejects_one_estimate_column_more", is(plan(2, INT32_MAX - kChunk + 1, 7, p), "rows too long for twl_compare_create"));
    CHECK("rejects_one_reference_column_more", is(plan(2, 5, INT32_MAX - kChunk + 1, p), "rows too long for twl_compare_create"));
    CHECK("rejects_the_largest_int", is(plan(2, INT32_MAX, INT32_MAX, p), "rows too long for twl_compare_create"));
    CHECK("a_refusal_leaves_an_empty_plan", p.n == 0 && p.createBytes == 0);

    // pitches around the tile
    CHECK("pitch_of_1", compare_pitch(1, kTile) == 64);
    CHECK("pitch_of_63", compare_pitch(63, kTile) == 64);
    CHECK("pitch_of_64", compare_pitch(64, kTile) == 64);
    CHECK("pitch_of_65", compare_pitch(65, kTile) == 128);
    CHECK("pitch_of_the_widest_row_does_not_wrap", compare_pitch(INT32_MAX - kChunk, kTile) > 0 && compare_pitch(INT32_MAX - kChunk, kTile) >= INT32_MAX - kChunk);

    // the two shapes this is built for: n x We passes 2^31, the keys pass 2^32 bytes
    CHECK("ten_thousand_by_hundred_thousand", plan(10000, 100000, 38000, p) == nullptr && p.pe == 100032 && p.estBytes == 1000320000ull && p.keyBytes == 4001280000ull &&
                                                  p.colTiles == 1563);
    CHECK("its_last_cell_lies_past_2_to_the_31_bytes", compare_cell_at(p.pe, 9999, 99999) == 1000319967ll && compare_cell_at(p.pe, 9999, 99999) * 4 > (1ll << 31));
    CHECK("hundred_thousand_by_38524", plan(100000, 38524, 38524, p) == nullptr && p.pe == 38528 && p.estBytes == 3852800000ull && p.keyBytes == 15411200000ull);
    CHECK("its_row_offsets_pass_2_to_the_31", compare_row_at(p.pe, 99999) == 3852761472ll && compare_row_at(p.pe, 99999) > (1ll << 31));
    CHECK("its_create_bytes_are_the_sum", p.createBytes == p.estBytes + p.refBytes + p.keyBytes + p.posBytes + p.smallBytes && p.posBytes == p.refBytes * 4);
    CHECK("the_largest_object_does_not_wrap", plan(1 << 20, INT32_MAX - kChunk, INT32_MAX - kChunk, p) == nullptr && p.keyBytes / 4 / (1u << 20) == (uint64_t)p.pe &&
                                                  p.createBytes > p.keyBytes);

    // upload slabs
    CHECK("a_slab_holds_whole_rows", compare_stage_rows(1000, 128, 1024) == 8);
    CHECK("a_slab_holds_one_row_at_least", compare_stage_rows(1000, 4096, 1024) == 1);
    CHECK("a_slab_holds_n_rows_at_most", compare_stage_rows(5, 64, 1 << 20) == 5);
    CHECK("a_slab_of_width_0", compare_stage_rows(5, 0, 1 << 20) == 5);
    return g_fail ? 1 : 0;
}
