// tests/retree_plan_kats.cpp -- known answers of what twl_retree_column_gaps and twl_retree_pair_counts (include/twl_retree.h) decide on the host:
// the checks, retree_max_gaps and the size functions, pure functions in twilight_amd/csrc/twl_retree_plan.inc.hip (no HIP call: this program
// includes the file directly).  The expected answers restate include/twl_retree.h.  Prints "OK <name>" / "FAIL <name>".
// With the argument "maxgaps" it reads pairs "T n" from stdin instead (T as a C hexadecimal float, exact) and prints retree_max_gaps of each.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../twilight_amd/csrc/twl_retree_plan.inc.hip"

static int g_fail = 0;
#define CHECK(name, cond) do { if (cond) printf("OK %s\n", name); else { printf("FAIL %s\n", name); ++g_fail; } } while (0)
static bool is(const char *got, const char *want) { return got && want ? strcmp(got, want) == 0 : got == want; }

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "maxgaps")) {
        char tok[128];
        int n;
        while (scanf("%127s %d", tok, &n) == 2) printf("%d\n", (int)retree_max_gaps(strtod(tok, nullptr), n));
        return 0;
    }
    const char *rows[3] = {"AC-T", "A-GT", "acgu"};
    uint32_t m[9] = {0}, b[9] = {0}, gaps[4] = {0};
    int32_t kept = 0;
    CHECK("pairs_accepts_three_rows", check_retree_pairs('n', 3, 4, rows, 2, m, b, &kept) == nullptr);
    CHECK("pairs_accepts_one_row", check_retree_pairs('p', 1, 4, rows, 1, m, b, &kept) == nullptr);
    CHECK("pairs_accepts_max_gaps_0", check_retree_pairs('n', 3, 4, rows, 0, m, b, &kept) == nullptr);
    CHECK("pairs_accepts_max_gaps_n", check_retree_pairs('n', 3, 4, rows, 3, m, b, &kept) == nullptr);
    CHECK("pairs_rejects_max_gaps_above_n", is(check_retree_pairs('n', 3, 4, rows, 4, m, b, &kept), "max_gaps must lie in 0 .. n"));
    CHECK("pairs_rejects_negative_max_gaps", is(check_retree_pairs('n', 3, 4, rows, -1, m, b, &kept), "max_gaps must lie in 0 .. n"));
    CHECK("pairs_rejects_type_x", is(check_retree_pairs('x', 3, 4, rows, 2, m, b, &kept), "the type must be 'n' or 'p'"));
    CHECK("pairs_rejects_type_N", is(check_retree_pairs('N', 3, 4, rows, 2, m, b, &kept), "the type must be 'n' or 'p'"));
    CHECK("pairs_rejects_type_0", is(check_retree_pairs('\0', 3, 4, rows, 2, m, b, &kept), "the type must be 'n' or 'p'"));
    CHECK("pairs_type_before_count", is(check_retree_pairs('x', 0, 4, rows, 2, m, b, &kept), "the type must be 'n' or 'p'"));
    CHECK("pairs_rejects_no_rows", is(check_retree_pairs('n', 0, 4, rows, 0, m, b, &kept), "no rows"));
    CHECK("pairs_rejects_a_negative_count", is(check_retree_pairs('n', -3, 4, rows, 0, m, b, &kept), "no rows"));
    CHECK("pairs_rejects_width_0", is(check_retree_pairs('n', 3, 0, rows, 2, m, b, &kept), "the rows have no columns"));
    CHECK("pairs_rejects_a_negative_width", is(check_retree_pairs('n', 3, -4, rows, 2, m, b, &kept), "the rows have no columns"));
    CHECK("pairs_rejects_null_rows", is(check_retree_pairs('n', 3, 4, nullptr, 2, m, b, &kept), "bad argument"));
    const char *withNull[3] = {"AC-T", nullptr, "acgu"};
    CHECK("pairs_rejects_a_null_row", is(check_retree_pairs('n', 3, 4, withNull, 2, m, b, &kept), "bad argument"));
    CHECK("pairs_ignores_rows_behind_n", check_retree_pairs('n', 1, 4, withNull, 1, m, b, &kept) == nullptr);
    CHECK("pairs_rejects_a_null_match", is(check_retree_pairs('n', 3, 4, rows, 2, nullptr, b, &kept), "bad argument"));
    CHECK("pairs_rejects_a_null_both", is(check_retree_pairs('n', 3, 4, rows, 2, m, nullptr, &kept), "bad argument"));
    CHECK("pairs_rejects_a_null_kept", is(check_retree_pairs('n', 3, 4, rows, 2, m, b, nullptr), "bad argument"));
    CHECK("gaps_accepts_three_rows", check_retree_gaps(3, 4, rows, gaps) == nullptr);
    CHECK("gaps_rejects_no_rows", is(check_retree_gaps(0, 4, rows, gaps), "no rows"));
    CHECK("gaps_rejects_width_0", is(check_retree_gaps(3, 0, rows, gaps), "the rows have no columns"));
    CHECK("gaps_rejects_null_rows", is(check_retree_gaps(3, 4, nullptr, gaps), "bad argument"));
    CHECK("gaps_rejects_a_null_row", is(check_retree_gaps(3, 4, withNull, gaps), "bad argument"));
    CHECK("gaps_rejects_a_null_output", is(check_retree_gaps(3, 4, rows, nullptr), "bad argument"));
    // the cap: 16384 passes, 16385 does not (the pointers are looked at only up to n: one row repeated)
    std::vector<const char *> many(16385, "A");
    CHECK("the_cap_is_16384", kRetreeMaxSeqs == 16384);
    CHECK("pairs_accepts_16384_rows", check_retree_pairs('n', 16384, 1, many.data(), 16384, m, b, &kept) == nullptr);
    CHECK("pairs_rejects_16385_rows", is(check_retree_pairs('n', 16385, 1, many.data(), 16384, m, b, &kept), "more than 16384 rows"));
    CHECK("gaps_rejects_16385_rows", is(check_retree_gaps(16385, 1, many.data(), gaps), "more than 16384 rows"));
    CHECK("count_before_pointers", is(check_retree_pairs('n', 16385, 1, nullptr, 0, nullptr, nullptr, nullptr), "more than 16384 rows"));
    // the mask's threshold
    CHECK("max_gaps_T_1_is_n", retree_max_gaps(1.0, 7) == 7 && retree_max_gaps(1.0, 16384) == 16384);
    CHECK("max_gaps_half_of_4", retree_max_gaps(0.5, 4) == 2);
    CHECK("max_gaps_quarter_of_3", retree_max_gaps(0.25, 3) == 0);
    CHECK("max_gaps_default_of_20", retree_max_gaps(0.95, 20) == 19);
    // sizes
    CHECK("planes", retree_planes('n') == 3 && retree_planes('p') == 6 && retree_planes('q') == 0);
    CHECK("words_of_one_column", retree_words_padded(1, 64, 8) == 8);
    CHECK("words_of_a_full_slice", retree_words_padded(512, 64, 8) == 8);
    CHECK("words_one_above_a_slice", retree_words_padded(513, 64, 8) == 16);
    CHECK("words_do_not_wrap", retree_words_padded(INT32_MAX, 64, 8) == 33554432);
    CHECK("two_matrices_of_1_GiB_at_the_cap", retree_device_bytes('n', 16384, 64, 8) == 16384ull * 64 + 64 * 4 + 16384ull * 3 * 8 * 8 + (2ull << 30));
    return g_fail ? 1 : 0;
}
