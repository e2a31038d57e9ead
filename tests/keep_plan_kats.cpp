// tests/keep_plan_kats.cpp -- known answers of what the calls of include/twl_keep.h decide on the host: check_keep_finish / check_finish_after_keep /
// keep_finish_done / check_dropped_counts / check_dropped_runs, pure functions in twilight_amd/csrc/twl_keep_plan.inc.hip over the placement's PlaceBook
// (no HIP call: this program includes the file directly).  The expected answers restate include/twl_keep.h.  Prints "OK <name>" / "FAIL <name>".
#include <cstdio>
#include <cstring>
#include <string>
#include "../twilight_amd/csrc/twl_keep_plan.inc.hip"

static int g_fail = 0;
#define CHECK(name, cond) do { if (cond) printf("OK %s\n", name); else { printf("FAIL %s\n", name); ++g_fail; } } while (0)

using V = std::vector<int32_t>;
using V64 = std::vector<int64_t>;
static bool is(const char *got, const char *want) { return got && want ? strcmp(got, want) == 0 : got == want; }

// a store of 8 rows: 0-2 are backbone rows of 10 columns, 3 is a sequence of 7, 4 of 12, 5 of 10, 6 is empty, 7 of 3
static const int32_t kRowLen[8] = {10, 10, 10, 7, 12, 10, 0, 3};

// a placement that has collected sequences 4, 3 and 7 (in that order), paths of 15, 11 and 13 codes
static PlaceBook collected()
{
    PlaceBook b;
    int64_t bytes = -1;
    check_place_create(10, 8, kRowLen, b, &bytes);
    PlaceCollectPlan p;
    const V ids{4, 3, 7}, plen{15, 11, 13};
    check_place_collect(b, 3, ids.data(), true, plen.data(), 64, nullptr, 8, kRowLen, PathLevelView{}, p);
    const int32_t none[3] = {0, 0, 0};
    place_collect_done(b, p, none);
    return b;
}

// ... and finished keeping the length: sequence 4 dropped 2 runs of 5 letters, 3 dropped 1 of 1, 7 none
static void finished(PlaceBook &b, KeepBook &k)
{
    b = collected();
    k = KeepBook{};
    const int32_t runs[3] = {2, 1, 0}, letters[3] = {5, 1, 0};
    int64_t r = -1, l = -1;
    keep_finish_done(b, k, runs, letters, &r, &l);
}

static void finish_kats()
{
    PlaceBook b = collected();
    KeepBook k;
    CHECK("finish_keep_accepts", check_keep_finish(b, k, true, 8, kRowLen) == nullptr);
    CHECK("finish_keep_rejects_null_outputs", is(check_keep_finish(b, k, false, 8, kRowLen), "bad argument"));
    CHECK("finish_after_keep_accepts_before", check_finish_after_keep(k) == nullptr);
    int32_t moved[8];
    memcpy(moved, kRowLen, sizeof moved);
    moved[3] = 10;
    CHECK("finish_keep_rejects_rewritten_placed_row", is(check_keep_finish(b, k, true, 8, moved), "a placed sequence's row has been rewritten since it was collected"));
    moved[3] = 7; moved[0] = 99;
    CHECK("finish_keep_ignores_backbone_rows", check_keep_finish(b, k, true, 8, moved) == nullptr);
    PlaceBook empty;
    int64_t bytes = -1;
    check_place_create(10, 8, kRowLen, empty, &bytes);
    CHECK("finish_keep_accepts_nothing_collected", check_keep_finish(empty, k, true, 8, kRowLen) == nullptr);

    const int32_t runs[3] = {2, 1, 0}, letters[3] = {5, 1, 0};
    int64_t r = -1, l = -1;
    keep_finish_done(b, k, runs, letters, &r, &l);
    CHECK("done_totals", r == 3 && l == 6);
    CHECK("done_tables_by_sequence", k.runs == V({0, 0, 0, 1, 2, 0, 0, 0}) && k.letters == V({0, 0, 0, 1, 5, 0, 0, 0}));
    CHECK("done_ends_the_placement", k.done && b.finished);
    CHECK("finish_keep_rejects_second_call", is(check_keep_finish(b, k, true, 8, kRowLen), "twl_place_finish_keep called twice"));
    CHECK("finish_rejects_after_finish_keep", is(check_finish_after_keep(k), "twl_place_finish after twl_place_finish_keep"));
    PlaceCollectPlan p;
    const V id5{5}, len5{10};
    CHECK("collect_rejects_after_finish_keep", is(check_place_collect(b, 1, id5.data(), true, len5.data(), 64, nullptr, 8, kRowLen, PathLevelView{}, p), "twl_place_collect after twl_place_finish"));

    PlaceBook fin = collected();
    fin.finished = true;                        // (twl_place_finish has run)
    CHECK("finish_keep_rejects_after_finish", is(check_keep_finish(fin, KeepBook{}, true, 8, kRowLen), "twl_place_finish_keep after twl_place_finish"));
}

static void counts_kats()
{
    PlaceBook b;
    KeepBook k;
    finished(b, k);
    const V all{4, 3, 7};
    CHECK("counts_accepts_all", check_dropped_counts(b, k, 3, all.data(), true) == nullptr);
    CHECK("counts_accepts_a_subset_in_another_order", check_dropped_counts(b, k, 2, V({7, 4}).data(), true) == nullptr);
    CHECK("counts_accepts_n_0", check_dropped_counts(b, k, 0, nullptr, false) == nullptr);
    CHECK("counts_rejects_negative_n", is(check_dropped_counts(b, k, -1, all.data(), true), "bad argument"));
    CHECK("counts_rejects_null_ids", is(check_dropped_counts(b, k, 3, nullptr, true), "bad argument"));
    CHECK("counts_rejects_null_outputs", is(check_dropped_counts(b, k, 3, all.data(), false), "bad argument"));
    CHECK("counts_rejects_before_finish_keep", is(check_dropped_counts(collected(), KeepBook{}, 3, all.data(), true), "twl_place_dropped_counts before twl_place_finish_keep"));
    CHECK("counts_n_0_before_finish_keep_is_refused_too", is(check_dropped_counts(collected(), KeepBook{}, 0, nullptr, false), "twl_place_dropped_counts before twl_place_finish_keep"));
    CHECK("counts_rejects_id_8_of_8", is(check_dropped_counts(b, k, 2, V({4, 8}).data(), true), "sequence id out of range"));
    CHECK("counts_rejects_negative_id", is(check_dropped_counts(b, k, 1, V({-1}).data(), true), "sequence id out of range"));
    CHECK("counts_rejects_uncollected_sequence", is(check_dropped_counts(b, k, 2, V({4, 5}).data(), true), "the sequence was not collected"));
    CHECK("counts_rejects_backbone_row", is(check_dropped_counts(b, k, 1, V({0}).data(), true), "the sequence was not collected"));
    CHECK("counts_rejects_id_twice", is(check_dropped_counts(b, k, 3, V({4, 3, 4}).data(), true), "a sequence id is listed twice"));
}

static void runs_kats()
{
    PlaceBook b;
    KeepBook k;
    finished(b, k);
    KeepRunsPlan p;
    const V all{4, 3, 7};
    const V64 off{0, 2, 3, 3};
    CHECK("runs_accepts_all", check_dropped_runs(b, k, 3, all.data(), off.data(), true, p) == nullptr && p.total == 3);
    CHECK("runs_plan_tables", p.pathOff == V64({77, 60, 129}) && p.runOff == V64({0, 2, 3}) && p.plen == V({15, 11, 13}) && p.nRuns == V({2, 1, 0}));
    const V other{7, 4};
    const V64 offOther{0, 0, 2};
    CHECK("runs_accepts_a_subset_in_another_order", check_dropped_runs(b, k, 2, other.data(), offOther.data(), true, p) == nullptr && p.total == 2 &&
                                                     p.pathOff == V64({129, 77}) && p.runOff == V64({0, 0}) && p.nRuns == V({0, 2}));
    CHECK("runs_accepts_n_0", check_dropped_runs(b, k, 0, nullptr, nullptr, false, p) == nullptr && p.total == 0 && p.plen.empty());
    const V only7{7};
    const V64 off7{0, 0};
    CHECK("runs_accepts_a_sequence_without_runs", check_dropped_runs(b, k, 1, only7.data(), off7.data(), true, p) == nullptr && p.total == 0);
    CHECK("runs_rejects_run_off_not_from_0", is(check_dropped_runs(b, k, 3, all.data(), V64({1, 3, 4, 4}).data(), true, p), "run_off is not the exclusive scan of the dropped-run counts"));
    CHECK("runs_rejects_run_off_of_other_counts", is(check_dropped_runs(b, k, 3, all.data(), V64({0, 1, 3, 3}).data(), true, p), "run_off is not the exclusive scan of the dropped-run counts"));
    CHECK("runs_rejects_a_wrong_total", is(check_dropped_runs(b, k, 3, all.data(), V64({0, 2, 3, 4}).data(), true, p), "run_off is not the exclusive scan of the dropped-run counts"));
    CHECK("runs_rejects_run_off_in_collect_order_for_another_order", is(check_dropped_runs(b, k, 2, other.data(), V64({0, 2, 2}).data(), true, p), "run_off is not the exclusive scan of the dropped-run counts"));
    CHECK("runs_rejects_null_run_off", is(check_dropped_runs(b, k, 3, all.data(), nullptr, true, p), "bad argument"));
    CHECK("runs_rejects_null_outputs", is(check_dropped_runs(b, k, 3, all.data(), off.data(), false, p), "bad argument"));
    CHECK("runs_rejects_negative_n", is(check_dropped_runs(b, k, -1, all.data(), off.data(), true, p), "bad argument"));
    CHECK("runs_rejects_before_finish_keep", is(check_dropped_runs(collected(), KeepBook{}, 3, all.data(), off.data(), true, p), "twl_place_dropped_runs before twl_place_finish_keep"));
    CHECK("runs_rejects_uncollected_sequence", is(check_dropped_runs(b, k, 1, V({5}).data(), off7.data(), true, p), "the sequence was not collected"));
    CHECK("runs_rejects_id_twice", is(check_dropped_runs(b, k, 2, V({3, 3}).data(), V64({0, 1, 2}).data(), true, p), "a sequence id is listed twice"));
    CHECK("runs_rejects_id_8_of_8", is(check_dropped_runs(b, k, 1, V({8}).data(), off7.data(), true, p), "sequence id out of range"));
    CHECK("runs_ids_come_before_run_off", is(check_dropped_runs(b, k, 2, V({3, 3}).data(), V64({5, 5, 5}).data(), true, p), "a sequence id is listed twice"));
}

int main()
{
    finish_kats();
    counts_kats();
    runs_kats();
    printf("%d failed\n", g_fail);
    return g_fail ? 1 : 0;
}
