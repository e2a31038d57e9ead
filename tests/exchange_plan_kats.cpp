// tests/exchange_plan_kats.cpp -- known answers of the layout of the device blocks in which ranks exchange a level's final paths: planExchange /
// exchangeRowOffsets / exchangeHeader, pure functions in twilight_amd/csrc/host/exchange_plan.hpp (this program includes the file alone), and of
// check_block_rows (twilight_amd/csrc/twl_level_plan.inc.hip), what twl_level_paths_to_block / twl_level_paths_from_block refuse before a launch.
// Every expected number is worked out by hand from the layout written at the top of exchange_plan.hpp.  Prints "OK <name>" / "FAIL <name>".
//
//   exchange_plan_kats          the known answers
//   exchange_plan_kats --dump   reads cases from stdin (name world n, then n numbers each of owner, takesPart, bound, length, errorType) and prints
//                               the plan and every rank's block as hex over a buffer of 0xEE: tests/test_exchange_plan_cpu.py holds the restatement
//                               of tests/exchange_cases.py to it
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include "../twilight_amd/csrc/host/exchange_plan.hpp"
#include "../twilight_amd/csrc/twl_level_plan.inc.hip"

using namespace msa::progressive;

static int g_fail = 0;
#define CHECK(name, cond) do { if (cond) printf("OK %s\n", name); else { printf("FAIL %s\n", name); ++g_fail; } } while (0)

using VI = std::vector<int>;
using V32 = std::vector<int32_t>;
using V64 = std::vector<int64_t>;
using VV = std::vector<std::vector<int>>;
using VS = std::vector<size_t>;

static bool is(const char *got, const char *want) { return got && want ? strcmp(got, want) == 0 : got == want; }

static void layout_kats()
{
    CHECK("pad8_0_1_7_8_9", pad8(0) == 0 && pad8(1) == 8 && pad8(7) == 8 && pad8(8) == 8 && pad8(9) == 16);
    {   // rank 1 of 3 owns nothing: its header is the four words alone, and it still has a block of blockMax bytes
        const ExchangePlan xp = planExchange({0, 2, 0, 2}, {1, 1, 1, 1}, {10, 20, 30, 40}, 3);
        CHECK("nothing_mine", xp.mine == VV({{0, 2}, {}, {1, 3}}));
        CHECK("nothing_hdr", xp.hdr == VS({48, 32, 48}) && xp.hdrMax == 48);
        // rank 0: 48 + 16 + 32 = 96, rank 2: 48 + 24 + 40 = 112 -> 256
        CHECK("nothing_blockMax", xp.blockMax == 256);
        V64 off;
        CHECK("nothing_rank1_offsets", exchangeRowOffsets(xp, 1, {}, off) == 32 && off.empty());
        // rank 2: pair 1 failed (length 0: no room), pair 3 has 40 codes
        CHECK("nothing_rank2_offsets", exchangeRowOffsets(xp, 2, {0, 40}, off) == 88 && off == V64({48, 48}));
        CHECK("nothing_rank0_offsets", exchangeRowOffsets(xp, 0, {10, 7}, off) == 72 && off == V64({48, 64}));
    }
    {   // rank 1 of 2 owns every pair
        const ExchangePlan xp = planExchange({1, 1, 1}, {1, 1, 1}, {8, 9, 7}, 2);
        CHECK("all_mine", xp.mine == VV({{}, {0, 1, 2}}));
        CHECK("all_hdr", xp.hdr == VS({32, 56}) && xp.hdrMax == 56);
        CHECK("all_blockMax", xp.blockMax == 256);      // 56 + 8 + 16 + 8 = 88
        V64 off;
        CHECK("all_offsets", exchangeRowOffsets(xp, 1, {8, 9, 1}, off) == 88 && off == V64({56, 64, 80}));
    }
    {   // pairs that take no part are in no block and their bound is not read: 1000 would show in blockMax
        const ExchangePlan xp = planExchange({0, 1, 0, 1, 0}, {1, 0, 0, 1, 1}, {5, 1000, 1000, 6, 7}, 2);
        CHECK("no_part_mine", xp.mine == VV({{0, 4}, {3}}));
        CHECK("no_part_hdr", xp.hdr == VS({48, 40}) && xp.hdrMax == 48);
        CHECK("no_part_blockMax", xp.blockMax == 256);
    }
    {   // lengths 0, 1, 7, 8 and 9: rooms of 0, 8, 8, 8 and 16 bytes behind a header of 32 + 40
        const ExchangePlan xp = planExchange({0, 0, 0, 0, 0}, {1, 1, 1, 1, 1}, {0, 1, 7, 8, 9}, 1);
        V64 off;
        CHECK("pad8_offsets", exchangeRowOffsets(xp, 0, {0, 1, 7, 8, 9}, off) == 112 && off == V64({72, 72, 80, 88, 96}));
        CHECK("pad8_blockMax", xp.hdr == VS({72}) && xp.blockMax == 256);
        CHECK("pad8_negative_length_takes_no_room", exchangeRowOffsets(xp, 0, {-1, 1, 7, 8, 9}, off) == 112);
    }
    {   // blockMax: a capacity of exactly 256 stays, 257 becomes 512.  rank 0: 40 + 216 = 256; rank 1: 48 + 104 + pad8(105) = 264
        CHECK("round_256_stays", planExchange({0}, {1}, {216}, 1).blockMax == 256);
        CHECK("round_257_goes_up", planExchange({0}, {1}, {217}, 1).blockMax == 512);
        const ExchangePlan xp = planExchange({0, 1, 1}, {1, 1, 1}, {216, 104, 105}, 2);
        CHECK("round_largest_rank", xp.blockMax == 512 && xp.hdrMax == 48);
    }
    {   // an empty level: headers only
        const ExchangePlan xp = planExchange({}, {}, {}, 2);
        CHECK("empty_level", xp.mine == VV({{}, {}}) && xp.hdr == VS({32, 32}) && xp.hdrMax == 32 && xp.blockMax == 256);
    }
    {   // the header: little-endian words, the magic over the level number, {length, errorType} per pair
        const ExchangePlan xp = planExchange({0, 0}, {1, 1}, {300, 300}, 1);
        const std::vector<char> h = exchangeHeader(xp, 0, 0x0102030405060708ull, 9, 1.5, 77, {258, 0}, {0, -3});
        const unsigned char want[48] = {8, 7, 6, 5, 4, 3, 2, 1, 9, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0xF8, 0x3F, 77, 0, 0, 0, 0x44, 0x4C, 0x57, 0x54,
                                        2, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0xFD, 0xFF, 0xFF, 0xFF};
        CHECK("header_bytes", h.size() == 48 && memcmp(h.data(), want, 48) == 0);
    }
}

// check_block_rows(toBlock, n_sel, pairs, lens, where, blk_off, n_pairs, seq_len, staged, haveDp, room): a level of 4 pairs, seq_len 100 (DP rows of 200),
// path buffer rows of 150
static const char *rows(bool toBlock, const V32 &pairs, const V32 &lens, const std::vector<uint8_t> &where, const V64 &off, int64_t room = -1, bool haveDp = true)
{
    return check_block_rows(toBlock, (int32_t)pairs.size(), pairs.data(), lens.data(), where.empty() ? nullptr : where.data(), off.data(), 4, 100, 150, haveDp, room);
}

static void refusal_kats()
{
    const char *bad = "bad row selection";
    CHECK("rows_accepts_both_kinds", rows(true, {0, 3}, {200, 150}, {1, 2}, {0, 200}) == nullptr);
    CHECK("rows_accepts_nothing", rows(true, {}, {}, {}, {}) == nullptr);
    CHECK("rows_rejects_pair_4_of_4", is(rows(true, {0, 4}, {10, 10}, {1, 2}, {0, 16}), bad));
    CHECK("rows_rejects_negative_pair", is(rows(false, {-1}, {10}, {}, {0}), bad));
    CHECK("rows_rejects_201_of_a_dp_row", is(rows(true, {0}, {201}, {1}, {0}), bad));
    CHECK("rows_rejects_151_of_a_path_row", is(rows(true, {0}, {151}, {2}, {0}), bad));
    CHECK("rows_rejects_151_into_a_path_row", is(rows(false, {0}, {151}, {}, {0}), bad));
    CHECK("rows_accepts_150_into_a_path_row", rows(false, {0}, {150}, {}, {0}) == nullptr);
    CHECK("rows_rejects_dp_row_as_destination", is(rows(false, {0}, {10}, {1}, {0}), bad));
    CHECK("rows_rejects_dp_row_without_dp_output", is(rows(true, {0}, {10}, {1}, {0}, -1, false), bad));
    CHECK("rows_accepts_path_row_without_dp_output", rows(true, {0}, {10}, {2}, {0}, -1, false) == nullptr);
    CHECK("rows_rejects_kind_0_and_3", is(rows(true, {0}, {10}, {0}, {0}), bad) && is(rows(true, {0}, {10}, {3}, {0}), bad));
    // a bad row of kind 2 behind good rows of kind 1 is found before anything is launched (one pass over the whole selection)
    CHECK("rows_judges_the_whole_selection", is(rows(true, {0, 1, 2}, {10, 10, 151}, {1, 1, 2}, {0, 16, 32}), bad));
    // rows of length 0 are not moved: nothing about them is looked at
    CHECK("rows_skips_empty_rows", rows(true, {99, 0}, {0, 10}, {7, 2}, {-5, 0}, 64) == nullptr);
    // a block inside the level's own buffer with 256 bytes left
    CHECK("rows_in_room_ends_at_its_end", rows(true, {0}, {56}, {2}, {200}, 256) == nullptr);
    CHECK("rows_in_room_one_past", is(rows(true, {0}, {57}, {2}, {200}, 256), bad));
    CHECK("rows_in_room_negative_offset", is(rows(true, {0}, {8}, {2}, {-8}, 256), bad));
    CHECK("rows_in_room_offset_2_to_40", is(rows(false, {0}, {8}, {}, {(int64_t)1 << 40}, 256), bad));
    CHECK("rows_in_room_offset_int64_max", is(rows(false, {0}, {8}, {}, {INT64_MAX}, 256), bad));
    CHECK("rows_unknown_room_is_the_callers", rows(false, {0}, {8}, {}, {(int64_t)1 << 40}) == nullptr);
}

static int dump()
{
    std::string name;
    int world, n;
    while (std::cin >> name >> world >> n) {
        VI owner(n);
        std::vector<char> takes(n);
        V32 bound(n), lens(n), errs(n);
        for (int &x : owner) std::cin >> x;
        for (char &x : takes) { int v; std::cin >> v; x = (char)v; }
        for (int32_t &x : bound) std::cin >> x;
        for (int32_t &x : lens) std::cin >> x;
        for (int32_t &x : errs) std::cin >> x;
        if (!std::cin) return 2;
        const ExchangePlan xp = planExchange(owner, takes, bound, world);
        printf("case %s hdrMax %zu blockMax %zu\n", name.c_str(), xp.hdrMax, xp.blockMax);
        for (int r = 0; r < world; ++r) {
            V32 ln, er;
            for (int i : xp.mine[r]) { ln.push_back(lens[i]); er.push_back(errs[i]); }
            V64 off;
            const size_t end = exchangeRowOffsets(xp, r, ln, off);
            printf("rank %d hdr %zu mine", r, xp.hdr[r]);
            for (int i : xp.mine[r]) printf(" %d", i);
            printf(" | off");
            for (int64_t o : off) printf(" %lld", (long long)o);
            printf(" | end %zu\n", end);
            if (end > xp.blockMax) return 3;
            std::vector<unsigned char> blk(xp.blockMax, 0xEE);
            const std::vector<char> h = exchangeHeader(xp, r, 1234567890123ull, 42, 3.25, 7, ln, er);
            memcpy(blk.data(), h.data(), h.size());
            for (size_t t = 0; t < ln.size(); ++t)
                for (int32_t k = 0; k < ln[t]; ++k) blk[(size_t)off[t] + (size_t)k] = (unsigned char)((xp.mine[r][t] * 131 + k) % 3);
            printf("block ");
            for (unsigned char b : blk) printf("%02x", b);
            printf("\n");
        }
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && strcmp(argv[1], "--dump") == 0) return dump();
    layout_kats();
    refusal_kats();
    printf("%s (%d failed)\n", g_fail ? "FAILED" : "all known answers hold", g_fail);
    return g_fail ? 1 : 0;
}
