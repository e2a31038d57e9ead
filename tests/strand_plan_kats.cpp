// tests/strand_plan_kats.cpp -- known answers of the pure checks of the strand calls (twilight_amd/csrc/twl_strand_plan.inc.hip).  g++ alone;
// prints one OK / FAIL line per check.
#include "../twilight_amd/csrc/twl_strand_plan.inc.hip"

#include <cstdio>
#include <cstring>

static int failed = 0;
static void check(bool ok, const char *what)
{
    printf("%s %s\n", ok ? "OK" : "FAIL", what);
    if (!ok) ++failed;
}
static bool says(const char *got, const char *want) { return want ? (got && strstr(got, want)) : got == nullptr; }

int main()
{
    // ---- rc(b) ----
    check(strand_rc_bin(0) == 4095 && strand_rc_bin(4095) == 0, "AAAAAA <-> TTTTTT");
    check(strand_rc_bin(1) == 2 * 1024 + 1023, "AAAAAC -> GTTTTT");
    check(strand_rc_bin(0 * 1024 + 1 * 256 + 2 * 64 + 3 * 16 + 0 * 4 + 1) == 2 * 1024 + 3 * 256 + 0 * 64 + 1 * 16 + 2 * 4 + 3, "ACGTAC -> GTACGT");
    check(strand_rc_bin(-1) == -1 && strand_rc_bin(4096) == -1, "outside 0 .. 4095");
    {
        bool ok = true;
        int fixed = 0;
        for (int b = 0; b < 4096; ++b) { ok = ok && strand_rc_bin(strand_rc_bin(b)) == b; fixed += strand_rc_bin(b) == b; }
        check(ok, "an involution");
        check(fixed == 64, "64 palindromic 6-mers");
    }
    // ---- twl_guide_set_opposite ----
    const int32_t ids[4] = {0, 3, 2, 9};
    uint32_t out[16] = {0};
    check(says(check_strand_opposite(true, 'n', 10, 4, ids, out), nullptr), "opposite: a legal call");
    check(says(check_strand_opposite(false, 'n', 10, 4, ids, out), "bad argument"), "opposite: no set");
    check(says(check_strand_opposite(true, 'n', 10, 4, nullptr, out), "bad argument"), "opposite: no ids");
    check(says(check_strand_opposite(true, 'n', 10, 4, ids, nullptr), "bad argument"), "opposite: no output");
    check(says(check_strand_opposite(true, 'p', 10, 4, ids, out), "nucleotide"), "opposite: a protein set");
    check(says(check_strand_opposite(true, 'n', 10, 0, ids, out), "between 1 and 16384"), "opposite: no id");
    check(says(check_strand_opposite(true, 'n', 10, 16385, ids, out), "between 1 and 16384"), "opposite: too many ids");
    check(says(check_strand_opposite(true, 'n', 9, 4, ids, out), "id out of range"), "opposite: an id behind the set");
    {
        const int32_t neg[2] = {1, -1}, twice[3] = {4, 1, 4};
        check(says(check_strand_opposite(true, 'n', 10, 2, neg, out), "id out of range"), "opposite: a negative id");
        check(says(check_strand_opposite(true, 'n', 10, 3, twice, out), "listed twice"), "opposite: the same id twice");
    }
    // ---- twl_guide_set_strand_assign ----
    const uint8_t flip[4] = {0, 1, 1, 0};
    int32_t seed[10] = {0};
    uint8_t dir[10] = {0};
    check(says(check_strand_assign(true, 'n', 10, 4, ids, flip, seed, dir), nullptr), "assign: a legal call");
    check(says(check_strand_assign(false, 'n', 10, 4, ids, flip, seed, dir), "bad argument"), "assign: no set");
    check(says(check_strand_assign(true, 'n', 10, 4, nullptr, flip, seed, dir), "bad argument"), "assign: no seeds");
    check(says(check_strand_assign(true, 'n', 10, 4, ids, nullptr, seed, dir), "bad argument"), "assign: no flips");
    check(says(check_strand_assign(true, 'n', 10, 4, ids, flip, nullptr, dir), "bad argument"), "assign: no seed_out");
    check(says(check_strand_assign(true, 'n', 10, 4, ids, flip, seed, nullptr), "bad argument"), "assign: no dir_out");
    check(says(check_strand_assign(true, 'p', 10, 4, ids, flip, seed, dir), "nucleotide"), "assign: a protein set");
    check(says(check_strand_assign(true, 'n', 10, 0, ids, flip, seed, dir), "seeds must be between 1 and 16384"), "assign: no seed");
    check(says(check_strand_assign(true, 'n', 10, 16385, ids, flip, seed, dir), "seeds must be between 1 and 16384"), "assign: too many seeds");
    check(says(check_strand_assign(true, 'n', 9, 4, ids, flip, seed, dir), "seed id out of range"), "assign: a seed behind the set");
    {
        const int32_t twice[3] = {4, 1, 4};
        const uint8_t bad[4] = {0, 1, 2, 0};
        check(says(check_strand_assign(true, 'n', 10, 3, twice, flip, seed, dir), "a seed twice"), "assign: the same seed twice");
        check(says(check_strand_assign(true, 'n', 10, 4, ids, bad, seed, dir), "flip must be 0 or 1"), "assign: a flip of 2");
    }
    return failed ? 1 : 0;
}
