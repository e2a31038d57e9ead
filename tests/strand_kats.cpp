// tests/strand_kats.cpp -- known answers of the host steps of --adjust-direction (twilight_amd/csrc/host/strand_orient.hpp): the seeds' directions
// on hand-made matrices, the complement table, the U rule and the default number of seeds.  g++ alone; prints one OK / FAIL line per check.
#include "../twilight_amd/csrc/host/strand_orient.hpp"

#include <cstdio>
#include <cstring>

using namespace msa::strand;

static int failed = 0;
static void check(bool ok, const char *what)
{
    printf("%s %s\n", ok ? "OK" : "FAIL", what);
    if (!ok) ++failed;
}

static std::string rc(std::string s) { reverseComplement(s); return s; }

static bool flipsAre(int S, std::vector<uint32_t> F, std::vector<uint32_t> R, std::vector<uint8_t> want)
{
    return seedFlips(S, F.data(), R.data()) == want;
}

// `strand_kats random`: 300 small matrices of small numbers (ties everywhere, some w = 0) from a generator that the Python test repeats; one line
// "R <flips>" each, which the test compares with the naive O(S^3) form of tests/strand_oracle.py
static uint32_t g_x = 12345;
static uint32_t draw(uint32_t mod) { g_x = (g_x * 1103515245u + 12345u) & 0x7FFFFFFFu; return (g_x >> 16) % mod; }
static void randomCases()
{
    for (int k = 0; k < 300; ++k) {
        const int S = 2 + k % 9;
        std::vector<uint32_t> F((size_t)S * S), R((size_t)S * S);
        for (int u = 0; u < S; ++u)
            for (int v = u; v < S; ++v) {
                F[(size_t)u * S + v] = F[(size_t)v * S + u] = u == v ? draw(4) * 2 : draw(4);
                R[(size_t)u * S + v] = R[(size_t)v * S + u] = draw(4);
            }
        printf("R ");
        for (uint8_t f : seedFlips(S, F.data(), R.data())) printf("%d", (int)f);
        printf("\n");
    }
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "random")) { randomCases(); return 0; }
    // ---- the seeds' directions ----
    check(flipsAre(1, {10}, {3}, {0}), "one seed is forward");
    // seed 1 shares more with the reverse of seed 0, seed 2 more with seed 1 as it stands: 1 and 2 both lie reversed
    check(flipsAre(3, {10, 1, 1, 1, 10, 8, 1, 8, 10}, {0, 9, 2, 9, 0, 1, 2, 1, 0}, {0, 1, 1}), "a chain: the flip is handed on");
    // ... and where seed 2 shares more with the reverse of seed 1, it is forward again
    check(flipsAre(3, {10, 1, 1, 1, 10, 1, 1, 1, 10}, {0, 9, 2, 9, 0, 8, 2, 8, 0}, {0, 1, 0}), "a chain: two opposite links cancel");
    // a tie between the kinds: F = R on the link, kind 0 wins
    check(flipsAre(2, {10, 5, 5, 10}, {0, 5, 5, 0}, {0, 0}), "a tie between the kinds goes to the same strand");
    // a tie between v: seed 2 is equally close to seed 0 (same strand) and, later, to seed 1 (opposite strand); seed 1 lies reversed.  The link to
    // the smaller v is taken at equal ratio and kind; here the kinds differ: kind 0 to v = 0 wins over kind 1 to v = 1
    check(flipsAre(3, {10, 1, 6, 1, 10, 1, 6, 1, 10}, {0, 9, 1, 9, 0, 6, 1, 6, 0}, {0, 1, 0}), "equal ratios: kind 0 before the smaller v");
    // a tie between v with equal kinds: seed 2 shares 6 with both inside seeds on the same strand; v = 0 or v = 1 give the same flip only when
    // flip[0] == flip[1], so make seed 1 reversed: through v = 0 seed 2 is forward, through v = 1 it would be reversed
    check(flipsAre(3, {10, 1, 6, 1, 10, 6, 6, 6, 10}, {0, 9, 1, 9, 0, 1, 1, 1, 0}, {0, 1, 0}), "equal ratios and kinds: the smaller v");
    // the order of joining: seed 2 (ratio 0.9 to seed 0) joins before seed 1 (0.5 to seed 0, 0.8 opposite to seed 2)
    check(flipsAre(3, {10, 5, 9, 5, 10, 1, 9, 1, 10}, {0, 1, 1, 1, 0, 8, 1, 8, 0}, {0, 1, 0}), "the best link joins first and later links build on it");
    // a seed with w = 0: every ratio is 0 / 1, kind 0, v = 0: forward, whatever R says
    check(flipsAre(3, {10, 0, 1, 0, 0, 0, 1, 0, 10}, {0, 0, 9, 0, 0, 0, 9, 0, 0}, {0, 0, 1}), "a seed without windows is forward");
    // the ratio divides by the smaller w: seed 1 (4 / 5) joins before seed 2 (7 / 10), which then takes its opposite link to seed 1 (4 / 5);
    // had seed 2 joined first, seed 1's tie between its two links would have kept all three forward
    check(flipsAre(3, {10, 4, 7, 4, 5, 1, 7, 1, 10}, {0, 1, 1, 1, 0, 4, 1, 4, 0}, {0, 0, 1}), "ratios over the smaller w, compared exactly");
    {
        Link a, b;
        a.num = 1u << 28; a.den = (1u << 28) + 1; b.num = (1u << 28) - 1; b.den = 1u << 28;
        check(before(a, b) && !before(b, a), "the cross products are taken in 64 bits");
    }
    // ---- the reverse complement ----
    check(rc("ACGT") == "ACGT" && rc("AACG") == "CGTT" && rc("") == "" && rc("A") == "T" && rc("ACG") == "CGT", "plain letters, even and odd lengths");
    check(rc("RYKMBVDH") == "DHBVKMRY", "the IUPAC pairs R-Y K-M B-V D-H");
    check(rc("SWN-.*X") == "X*.-NWS", "S, W, N and every other byte stay");
    check(rc("acgtRyKm") == "kMrYacgt", "case is kept");
    check(rc("AACGU") == "ACGUU" && rc("aacgu") == "acguu", "a record with U and no T: A <-> U");
    check(rc("AUT") == "AUT", "a record with U and T: T -> A, A -> T, U stays");
    check(rc("AAN") == "NTT", "no U: A -> T");
    {
        std::string t = "ACGTNRYKMBVDHSWacgtn";
        check(rc(rc(t)) == t, "twice is the identity");
    }
    // ---- the default number of seeds ----
    check(defaultSeeds(1, 1) == 1, "N = 1");
    check(defaultSeeds(2, 2) == 2, "N = 2: 3 * 3 >= 8, clipped to N");
    check(defaultSeeds(200, 200) == 29, "N = 200");
    check(defaultSeeds(1 << 20, 1 << 20) == 2048, "N = 2^20");
    check(defaultSeeds(20, 20) == 9 && defaultSeeds(579, 479) == 49, "the fixtures");
    check(defaultSeeds(1 << 20, 100) == 100 && defaultSeeds(1ll << 40, 1ll << 40) == 16384, "clipped to the cap and to 16384");
    return failed ? 1 : 0;
}
