// tests/exit_kats.cpp -- the tile exit and the steps of the traceback walk that the three DP kernels share (twilight_amd/csrc/talco_exit.hip.h: plain
// functions on ints, no HIP call: this program includes the header directly).  It holds no expected answer: it prints what the functions return, and
// tests/test_exit_fn_cpu.py holds that to the reference's text and to the oracle's exit records.  One mode per run, named by the first argument:
//   walk                      for state 0..2 and nibble 0..15: "st v dir st' dkk dii dqi dri"
//   exits                     stdin, one tile per line: "conv_logic last_k marker conv_value refLen qLen R Q ref_idx qry_idx"
//                             -> "bad conv_r conv_q tb_state start_k ended adv_bad ref_idx qry_idx last tailDir tailLen" (the advance only where the exit is not bad)
//   append CAP N0 COUNT       COUNT appends of code 1 from n = N0 into a buffer of CAP codes -> "n" and the CAP + 4 bytes of the buffer (4 canaries of 7 behind it)
//   fill CAP RI QI            border_fill from n = 0 -> the same
//   emit N SKIP DIR LEN STRIDE  a reverse buffer 0 1 2 0 1 2 ... of N codes, emitted at position 3 by STRIDE threads -> "pos" and the N + LEN + 8 output bytes (9 = untouched)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../twilight_amd/csrc/talco_exit.hip.h"

static void print_bytes(const std::vector<int8_t> &b)
{
    for (size_t t = 0; t < b.size(); ++t) printf("%d", (int)b[t]);
    printf("\n");
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const auto arg = [&](int t) { return t < argc ? atoi(argv[t]) : 0; };
    if (!strcmp(argv[1], "walk")) {
        for (int st0 = 0; st0 < 3; ++st0)
            for (int v = 0; v < 16; ++v) {
                int st = st0, kk = 1000, ii = 100, qi = 50, ri = 70;
                const int dir = twl::walk_step(st, v, kk, ii, qi, ri);
                printf("%d %d %d %d %d %d %d %d\n", st0, v, dir, st, kk - 1000, ii - 100, qi - 50, ri - 70);
            }
    } else if (!strcmp(argv[1], "exits")) {
        int conv_logic, last_k, marker, conv_value, refLen, qLen, R, Q, ref_idx, qry_idx;
        while (scanf("%d %d %d %d %d %d %d %d %d %d", &conv_logic, &last_k, &marker, &conv_value, &refLen, &qLen, &R, &Q, &ref_idx, &qry_idx) == 10) {
            const twl::TileExit e = twl::tile_exit(conv_logic != 0, last_k, marker, conv_value, refLen, qLen);
            twl::PairAdvance a{false, 0, 0, false};
            if (!e.bad) a = twl::pair_advance(R, Q, e.conv_r, e.conv_q, ref_idx, qry_idx);
            printf("%d %d %d %d %d %d %d %d %d %d %d %d\n", (int)e.bad, e.conv_r, e.conv_q, e.tb_state, e.start_k, (int)e.ended_before_marker, (int)a.bad, ref_idx, qry_idx,
                   (int)(e.ended_before_marker || a.last_tile), a.tailDir, a.tailLen);
        }
    } else if (!strcmp(argv[1], "append") || !strcmp(argv[1], "fill")) {
        const int cap = arg(2);
        std::vector<int8_t> buf((size_t)cap + 4, (int8_t)7);
        int n = 0;
        if (argv[1][0] == 'a') { n = arg(3); for (int t = 0; t < arg(4); ++t) twl::rev_append(buf.data(), cap, n, 1); }
        else twl::border_fill(buf.data(), cap, n, arg(3), arg(4));
        printf("%d\n", n);
        print_bytes(buf);
    } else if (!strcmp(argv[1], "emit")) {
        const int n = arg(2), skip = arg(3), dir = arg(4), len = arg(5), stride = arg(6);
        std::vector<int8_t> rev((size_t)n), out((size_t)(n + len + 8), (int8_t)9);
        for (int t = 0; t < n; ++t) rev[(size_t)t] = (int8_t)(t % 3);
        int pos = -1;
        for (int th = 0; th < stride; ++th) {
            const int p = twl::emit_segment(out.data(), 3, rev.data(), n, skip, dir, len, th, stride);
            if (th > 0 && p != pos) return 3;      // every thread learns the same position
            pos = p;
        }
        printf("%d\n", pos);
        print_bytes(out);
    } else return 2;
    return 0;
}
