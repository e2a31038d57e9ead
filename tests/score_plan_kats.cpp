// tests/score_plan_kats.cpp -- known answers of what twl_store_score_rows (include/twl_score.h) decides on the host: every refusal of
// check_score_rows, the grids and padding of plan_score_grid, the tile-pair list, the layout of sub and the terminal runs of score_terminals,
// pure functions in twilight_amd/csrc/twl_score_plan.inc.hip (no HIP call: this program includes the file directly).  The expected answers
// restate include/twl_score.h.  Prints "OK <name>" / "FAIL <name>".
#include <cstdio>
#include <cstring>
#include <string>
#include "../twilight_amd/csrc/twl_score_plan.inc.hip"

static int g_fail = 0;
#define CHECK(name, cond) do { if (cond) printf("OK %s\n", name); else { printf("FAIL %s\n", name); ++g_fail; } } while (0)

using V = std::vector<int32_t>;
static bool is(const char *got, const char *want) { return got && want ? strcmp(got, want) == 0 : got == want; }

// a store of 8 rows: 0-3 have 70 columns, 4 and 5 have 33, 6 and 7 are empty
static const int32_t kRowLen[8] = {70, 70, 70, 70, 33, 33, 0, 0};
static const int32_t kTile = 1024;

static const char *chk(int32_t n, const int32_t *ids, char type, int32_t &W, bool store = true, bool sub = true, bool runs = true, bool totals = true, bool prepared = false,
                       const int32_t *len = kRowLen, int32_t n_seqs = 8)
{
    return check_score_rows(store, n, ids, type, sub, runs, totals, n_seqs, len, prepared, kTile, W);
}

static void check_kats()
{
    int32_t W = -1;
    const V ids{3, 0, 2};
    CHECK("accepts_three_rows", chk(3, ids.data(), 'n', W) == nullptr && W == 70);
    CHECK("accepts_protein", chk(2, V({4, 5}).data(), 'p', W) == nullptr && W == 33);
    CHECK("rejects_null_store", is(chk(3, ids.data(), 'n', W, false), "bad argument"));
    CHECK("rejects_null_ids", is(chk(3, nullptr, 'n', W), "bad argument"));
    CHECK("rejects_null_sub", is(chk(3, ids.data(), 'n', W, true, false), "bad argument"));
    CHECK("rejects_null_runs", is(chk(3, ids.data(), 'n', W, true, true, false), "bad argument"));
    CHECK("rejects_null_totals", is(chk(3, ids.data(), 'n', W, true, true, true, false), "bad argument"));
    CHECK("rejects_one_row", is(chk(1, ids.data(), 'n', W), "fewer than two rows listed"));
    CHECK("rejects_no_rows", is(chk(0, ids.data(), 'n', W), "fewer than two rows listed"));
    CHECK("rejects_a_negative_count", is(chk(-1, ids.data(), 'n', W), "fewer than two rows listed"));
    CHECK("rejects_id_8_of_8", is(chk(2, V({0, 8}).data(), 'n', W), "sequence id out of range"));
    CHECK("rejects_a_negative_id", is(chk(2, V({-1, 0}).data(), 'n', W), "sequence id out of range"));
    CHECK("rejects_an_id_twice", is(chk(3, V({0, 1, 0}).data(), 'n', W), "a sequence id is listed twice"));
    CHECK("rejects_two_lengths", is(chk(2, V({0, 4}).data(), 'n', W), "the listed rows differ in length"));
    CHECK("rejects_a_prepared_level", is(chk(3, ids.data(), 'n', W, true, true, true, true, true), "a level is still prepared on the store: commit it first"));
    CHECK("rejects_type_x", is(chk(3, ids.data(), 'x', W), "unknown sequence type"));
    CHECK("rejects_type_N", is(chk(3, ids.data(), 'N', W), "unknown sequence type"));
    CHECK("rejects_type_0", is(chk(3, ids.data(), '\0', W), "unknown sequence type"));
    CHECK("rejects_no_column", is(chk(2, V({6, 7}).data(), 'n', W), "the listed rows have no column"));
    CHECK("a_refusal_fills_nothing", chk(2, V({0, 4}).data(), 'n', W) != nullptr && W == 0);
    // 2^20 rows are the most; one more is refused before an id is read
    {
        const int32_t n = kScoreMaxRows;
        std::vector<int32_t> len((size_t)n + 1, 5), all((size_t)n + 1);
        for (int32_t k = 0; k <= n; ++k) all[k] = k;
        CHECK("accepts_2_20_rows", chk(n, all.data(), 'n', W, true, true, true, true, false, len.data(), n + 1) == nullptr && W == 5);
        CHECK("rejects_2_20_rows_and_one", is(chk(n + 1, all.data(), 'n', W, true, true, true, true, false, len.data(), n + 1), "more than 2^20 rows listed"));
        // n (n - 1) / 2 * W >= 2^63: 2^20 rows make 2^39 - 2^19 pairs; W = 2^24 is below the bound, 2^24 + 32 reaches it
        //   (2^39 - 2^19) * 2^24 = 2^63 - 2^43 < 2^63;   (2^39 - 2^19) * (2^24 + 32) = 2^63 - 2^43 + 2^44 - 2^24 >= 2^63
        std::fill(len.begin(), len.end(), 1 << 24);
        CHECK("accepts_totals_below_2_63", chk(n, all.data(), 'n', W, true, true, true, true, false, len.data(), n + 1) == nullptr);
        std::fill(len.begin(), len.end(), (1 << 24) + 32);
        CHECK("rejects_totals_of_2_63", is(chk(n, all.data(), 'n', W, true, true, true, true, false, len.data(), n + 1), "n (n - 1) / 2 * W reaches 2^63: the totals would not fit"));
    }
    // the width bound: INT32_MAX - tile is the last width whose last tile ends inside int32
    int32_t wide[8] = {INT32_MAX - kTile, INT32_MAX - kTile, INT32_MAX - kTile + 1, INT32_MAX - kTile + 1, 0, 0, 0, 0};
    CHECK("width_bound", score_max_width(kTile) == INT32_MAX - 1024);
    CHECK("accepts_the_widest_rows", chk(2, V({0, 1}).data(), 'n', W, true, true, true, true, false, wide) == nullptr && W == INT32_MAX - kTile);
    CHECK("rejects_one_column_more", is(chk(2, V({2, 3}).data(), 'n', W, true, true, true, true, false, wide), "rows too long for twl_store_score_rows"));
}

static void grid_kats()
{
    ScoreGrid g;
    // slice 16 words, tile 64 rows, counts tile 1024 columns, row slice 512, products block 256 columns
    CHECK("one_of_everything", plan_score_grid(1, 2, 16, 64, 1024, 512, 256, g) == nullptr && g.words == 1 && g.wordsPad == 16 && g.colTiles == 1 && g.rowSlices == 1 &&
                                   g.prodBlocks == 1 && g.tiles == 1 && g.tilePairs == 1);
    CHECK("a_whole_slice_has_no_pad", plan_score_grid(1024, 64, 16, 64, 1024, 512, 256, g) == nullptr && g.words == 16 && g.wordsPad == 16 && g.colTiles == 1 && g.prodBlocks == 4 &&
                                          g.tiles == 1);
    CHECK("one_past_each", plan_score_grid(1025, 513, 16, 64, 1024, 512, 256, g) == nullptr && g.words == 17 && g.wordsPad == 32 && g.colTiles == 2 && g.rowSlices == 2 &&
                               g.prodBlocks == 5 && g.tiles == 9 && g.tilePairs == 45);
    CHECK("a_word_boundary", plan_score_grid(65, 65, 16, 64, 1024, 512, 256, g) == nullptr && g.words == 2 && g.tiles == 2 && g.tilePairs == 3);
    CHECK("ten_thousand_rows", plan_score_grid(66000, 10000, 16, 64, 1024, 512, 256, g) == nullptr && g.words == 1032 && g.wordsPad == 1040 && g.tiles == 157 && g.tilePairs == 12403 &&
                                   g.rowSlices == 20 && g.colTiles == 65 && g.prodBlocks == 258);
    CHECK("the_most_rows", plan_score_grid(5, 1 << 20, 16, 64, 1024, 512, 256, g) == nullptr && g.tiles == 16384 && g.tilePairs == 134225920LL && g.rowSlices == 2048);
    CHECK("the_widest_row_does_not_wrap", plan_score_grid(INT32_MAX - 1024, 2, 16, 64, 1024, 512, 256, g) == nullptr && g.words == 33554416 && g.wordsPad == 33554416 &&
                                              g.colTiles == 2097151 && g.prodBlocks == 8388604);
    std::vector<uint32_t> tp;
    plan_score_tile_pairs(1, tp);
    CHECK("one_tile_pair", tp == std::vector<uint32_t>({0u}));
    plan_score_tile_pairs(3, tp);
    CHECK("six_tile_pairs", tp == std::vector<uint32_t>({0u, 1u, 2u, (1u << 16) | 1u, (1u << 16) | 2u, (2u << 16) | 2u}));
    plan_score_tile_pairs(157, tp);
    bool ordered = tp.size() == 12403;
    for (uint32_t e : tp) ordered = ordered && (e >> 16) <= (e & 0xFFFFu) && (e & 0xFFFFu) < 157;
    CHECK("every_pair_lies_on_or_above_the_diagonal", ordered);
}

static void layout_kats()
{
    CHECK("classes", score_classes('n') == 4 && score_classes('p') == 20 && score_classes('x') == 0);
    CHECK("entries", score_sub_entries(4) == 15 && score_sub_entries(20) == 231);
    bool dense = true;
    for (int32_t K : {4, 20}) {
        int32_t at = 0;
        for (int32_t a = 0; a <= K; ++a)
            for (int32_t b = a; b <= K; ++b) dense = dense && score_sub_index(K, a, b) == at++;
        dense = dense && at == score_sub_entries(K);
    }
    CHECK("sub_rows_one_after_the_other", dense);
}

static void terminal_kats()
{
    uint64_t RT = 0, GT = 0;
    // rows --GT---TA / ACGTACGTA: row 0 has a leading range of 2 columns in which row 1 holds 2 letters
    {
        const uint32_t let[9] = {1, 1, 2, 2, 1, 1, 1, 2, 2};
        const int32_t first[2] = {2, 0}, last[2] = {8, 8};
        score_terminals(2, 9, let, first, last, RT, GT);
        CHECK("a_leading_range", RT == 1 && GT == 2);
    }
    // rows ------- / AC--GT- / CA--TG-: the row without letters has one range against each of the two others, counted once; rows 1 and 2 end
    // together in front of the last column, which nobody fills
    {
        const uint32_t let[7] = {2, 2, 0, 0, 2, 2, 0};
        const int32_t first[3] = {7, 0, 0}, last[3] = {-1, 5, 5};
        score_terminals(3, 7, let, first, last, RT, GT);
        CHECK("a_row_without_letters", RT == 2 && GT == 8);
    }
    // rows ----AC-GTA / ACG---T---: row 0 leads with 3 letters of row 1 in front; row 1 trails with 3 letters of row 0 behind
    {
        const uint32_t let[10] = {1, 1, 1, 0, 1, 1, 1, 1, 1, 1};
        const int32_t first[2] = {4, 0}, last[2] = {9, 6};
        score_terminals(2, 10, let, first, last, RT, GT);
        CHECK("one_end_each", RT == 2 && GT == 6);
    }
    // three rows that start at one column: no leading run among them (first[j] < first[i] is strict)
    {
        const uint32_t let[3] = {3, 2, 1};
        const int32_t first[3] = {0, 0, 0}, last[3] = {2, 1, 0};
        score_terminals(3, 3, let, first, last, RT, GT);
        CHECK("equal_firsts_make_no_run", RT == 3 && GT == 1 + 3);      // row 2 trails rows 0 and 1 (2 + 1 letters), row 1 trails row 0 (1 letter)
    }
    // no letter anywhere
    {
        const uint32_t let[2] = {0, 0};
        const int32_t first[2] = {2, 2}, last[2] = {-1, -1};
        score_terminals(2, 2, let, first, last, RT, GT);
        CHECK("no_letter_anywhere", RT == 0 && GT == 0);
    }
}

int main()
{
    check_kats();
    grid_kats();
    layout_kats();
    terminal_kats();
    printf("%s\n", g_fail ? "SOME FAILED" : "ALL PASSED");
    return g_fail ? 1 : 0;
}
