// tests/guide_plan_kats.cpp -- known answers of what twl_guide_kmer_counts and twl_guide_shared (include/twl_guide.h) decide on the host:
// check_guide and the two size functions, pure functions in twilight_amd/csrc/twl_guide_plan.inc.hip (no HIP call: this program includes the
// file directly).  The expected answers restate include/twl_guide.h.  Prints "OK <name>" / "FAIL <name>".
#include <cstdio>
#include <cstring>
#include <vector>
#include "../twilight_amd/csrc/twl_guide_plan.inc.hip"

static int g_fail = 0;
#define CHECK(name, cond) do { if (cond) printf("OK %s\n", name); else { printf("FAIL %s\n", name); ++g_fail; } } while (0)
static bool is(const char *got, const char *want) { return got && want ? strcmp(got, want) == 0 : got == want; }

int main()
{
    const char *seqs[3] = {"ACGTACGT", "", "ACG"};
    const int32_t lens[3] = {8, 0, 3};
    uint32_t out[9] = {0};
    uint64_t total = 99;
    CHECK("accepts_three_sequences", check_guide('n', 3, seqs, lens, out, &total) == nullptr && total == 11);
    total = 99;
    CHECK("accepts_one_sequence", check_guide('p', 1, seqs, lens, out, &total) == nullptr && total == 8);
    CHECK("accepts_without_a_total", check_guide('n', 3, seqs, lens, out, nullptr) == nullptr);
    const char *withNull[2] = {"ACGT", nullptr};
    const int32_t emptyLast[2] = {4, 0}, fullLast[2] = {4, 2};
    CHECK("accepts_a_null_sequence_of_length_0", check_guide('n', 2, withNull, emptyLast, out, &total) == nullptr && total == 4);
    CHECK("rejects_a_null_sequence_with_letters", is(check_guide('n', 2, withNull, fullLast, out, &total), "bad argument"));
    CHECK("rejects_no_sequences", is(check_guide('n', 0, seqs, lens, out, &total), "no sequences"));
    CHECK("rejects_a_negative_count", is(check_guide('n', -5, seqs, lens, out, &total), "no sequences"));
    CHECK("rejects_type_x", is(check_guide('x', 3, seqs, lens, out, &total), "the type must be 'n' or 'p'"));
    CHECK("rejects_type_N", is(check_guide('N', 3, seqs, lens, out, &total), "the type must be 'n' or 'p'"));
    CHECK("rejects_type_0", is(check_guide('\0', 3, seqs, lens, out, &total), "the type must be 'n' or 'p'"));
    CHECK("type_before_count", is(check_guide('x', 0, seqs, lens, out, &total), "the type must be 'n' or 'p'"));
    CHECK("rejects_null_sequences", is(check_guide('n', 3, nullptr, lens, out, &total), "bad argument"));
    CHECK("rejects_null_lengths", is(check_guide('n', 3, seqs, nullptr, out, &total), "bad argument"));
    CHECK("rejects_a_null_output", is(check_guide('n', 3, seqs, lens, nullptr, &total), "bad argument"));
    const int32_t neg[3] = {8, -1, 3};
    CHECK("rejects_a_negative_length", is(check_guide('n', 3, seqs, neg, out, &total), "negative sequence length"));
    const int32_t negLast[3] = {8, 0, INT32_MIN};
    CHECK("rejects_a_negative_last_length", is(check_guide('p', 3, seqs, negLast, out, &total), "negative sequence length"));
    // the cap: 16384 passes, 16385 does not (the pointers are looked at only up to n: one empty sequence repeated)
    std::vector<const char *> many(16385, "");
    std::vector<int32_t> zeros(16385, 0);
    CHECK("the_cap_is_16384", kGuideMaxSeqs == 16384);
    CHECK("accepts_16384_sequences", check_guide('n', 16384, many.data(), zeros.data(), out, &total) == nullptr && total == 0);
    CHECK("rejects_16385_sequences", is(check_guide('n', 16385, many.data(), zeros.data(), out, &total), "more than 16384 sequences"));
    CHECK("count_before_pointers", is(check_guide('n', 16385, nullptr, nullptr, nullptr, &total), "more than 16384 sequences"));
    // the total does not wrap 32 bits
    std::vector<int32_t> big(4, INT32_MAX);
    const char *four[4] = {"A", "A", "A", "A"};
    CHECK("the_total_is_64_bit", check_guide('n', 4, four, big.data(), out, &total) == nullptr && total == 4ull * INT32_MAX);
    CHECK("bins_n", guide_bins('n') == 4096);
    CHECK("bins_p", guide_bins('p') == 7776);
    CHECK("bins_other", guide_bins('q') == 0);
    CHECK("padding_keeps_a_multiple", guide_bins_padded(4096, 128) == 4096);
    CHECK("padding_rounds_up", guide_bins_padded(7776, 128) == 7808);
    return g_fail ? 1 : 0;
}
