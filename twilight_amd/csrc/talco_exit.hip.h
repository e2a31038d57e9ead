// twilight_amd/csrc/talco_exit.hip.h -- the tile exit (TALCO-XDrop.cpp:615-682) and the steps of the traceback walk (:134-231) that talco_kernel.hip.h and
// talco_global.hip.h share: small functions on plain ints, no kernel state, no barrier, no LDS layout.  What differs per kernel stays in the kernel: how
// CS[last_k][0] and a pointer nibble are fetched, the flush of a partial group of 8 diagonals.  talco_nuc.hip.h still has its own text of the same lines
// (DESIGN.md section 3.4 says why).  Compiles under g++ without HIP (tests/exit_kats.cpp), as the *_plan.inc.hip files do.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define TWL_EXIT_FN __device__ __forceinline__
// (one lane fills a few codes: vectorized by 8 with a guard per code, the loop costs a kernel up to 12 VGPRs)
#define TWL_EXIT_PLAIN_LOOP _Pragma("clang loop vectorize(disable)")
#else
#define TWL_EXIT_FN inline
#define TWL_EXIT_PLAIN_LOOP
#endif

namespace twl {

struct TileExit {
    int conv_q, conv_r;             // the cell the tile ends in, relative to its start: the next tile starts there
    int tb_state, start_k;          // the walk's start: state 0 S, 1 I, 2 D, 3 the S cell one diagonal in front of the marker; its diagonal
    bool bad;                       // the "bug" code 3: boundary sentinel / unset (the reference indexes out of range here), or a cell in front of the tile
    bool ended_before_marker;       // the pair ended in this tile (:625-632): the last one
};

// conv_value: the converged pointer (conv_logic), or CS[last_k][0] of a tile that ended at or behind the marker unconverged (:633-635); unused otherwise
TWL_EXIT_FN TileExit tile_exit(bool conv_logic, int last_k, int marker, int conv_value, int refLen, int qLen)
{
    int conv_q = 0, conv_r = 0, tb_state = 0, start_k = 0;
    bool bad = false, ended = false;
    if (conv_logic || last_k >= marker) {
        conv_q = conv_value & 0xFFFF;
        tb_state = (conv_value >> 16) & 0xFFFF;
        if (tb_state > 3) bad = true;
        else {
            conv_r = marker - conv_q - ((tb_state == 3) ? 1 : 0);
            start_k = (tb_state == 3) ? marker - 1 : marker;
            if (conv_r < 0) bad = true;
        }
    } else {                                                              // :625-632
        conv_q = qLen - 1; conv_r = refLen - 1; start_k = last_k; ended = true;
    }
    return TileExit{conv_q, conv_r, tb_state, start_k, bad, ended};
}

struct PairAdvance {
    bool bad;                       // the advance left the pair (:659-668): code 3
    int tailDir, tailLen;           // the run of one gap code behind the last tile (0: none)
    bool last_tile;
};

// the advance of the pair by a tile's end cell (:654-655) and the three cases in which that cell lies on the pair's last row or column (:671-679)
TWL_EXIT_FN PairAdvance pair_advance(int R, int Q, int conv_r, int conv_q, int &ref_idx, int &qry_idx)
{
    ref_idx += conv_r; qry_idx += conv_q;
    int tailDir = 0, tailLen = 0;
    bool last = false;
    const bool bad = R - ref_idx < 0 || Q - qry_idx < 0;
    if (ref_idx == R - 1 && qry_idx < Q - 1) { tailDir = 1; tailLen = Q - qry_idx - 1; last = true; }      // :671-674
    if (qry_idx == Q - 1 && ref_idx < R - 1) { tailDir = 2; tailLen = R - ref_idx - 1; last = true; }      // :675-678
    if (ref_idx == R - 1 && qry_idx == Q - 1) last = true;                                                 // :679
    return PairAdvance{bad, tailDir, tailLen, last};
}

// One step of the walk from cell (diagonal kk, row ii) whose pointer nibble is v: v & 3 is the S cell's move (0 diagonal, 1 I, 2 D), bit 4 = I extends,
// bit 8 = D extends.  Returns the code of the step; st, the cell and the columns left (qi, ri) move with it.
TWL_EXIT_FN int walk_step(int &st, int v, int &kk, int &ii, int &qi, int &ri)
{
    int dir;
    if (st == 0) {
        st = v & 3;
        if (st == 0) dir = 0;
        else if (st == 1) { dir = 1; st = (v & 4) ? 1 : 0; }
        else { dir = 2; st = (v & 8) ? 2 : 0; }
    } else if (st == 1) { dir = 1; st = (v & 4) ? 1 : 0; }
    else { dir = 2; st = (v & 8) ? 2 : 0; }
    // (on copies, written back once: a store through a reference under a condition keeps the caller's variable in scratch memory)
    int k = kk, i = ii, q = qi, r = ri;
    if (dir == 0) { k -= 2; i -= 1; q--; r--; }
    else if (dir == 1) { k -= 1; i -= 1; q--; }
    else { k -= 1; r--; }
    kk = k; ii = i; qi = q; ri = r;
    return dir;
}

// The walk writes its codes back to front into a buffer of cap codes.  A code past the end is counted and not written: n > cap afterwards ends the pair
// with code 3 (never on valid data: a tile's path is at most 2 * marker + 1 codes long).
TWL_EXIT_FN void rev_append(int8_t *rev, int cap, int &n, int code)
{
    if (n < cap) rev[n] = (int8_t)code;
    ++n;
}

// the first tile's walk left through the border (:221-230): the columns left on either side are gaps
TWL_EXIT_FN void border_fill(int8_t *rev, int cap, int &n, int ri, int qi)
{
    TWL_EXIT_PLAIN_LOOP while (ri > -1) { rev_append(rev, cap, n, 2); ri--; }
    TWL_EXIT_PLAIN_LOOP while (qi > -1) { rev_append(rev, cap, n, 1); qi--; }
}

// A tile's segment of the path: its n codes reversed, without the first one for later tiles (skip = 1, :98-102), then the trailing run; spread over the
// threads first_thread, first_thread + stride, ...  Returns the position behind it (the caller has checked that it fits).
TWL_EXIT_FN int emit_segment(int8_t *out, int pos, const int8_t *rev, int n, int skip, int tailDir, int tailLen, int first_thread, int stride)
{
    const int cnt = n - skip;
    for (int t = first_thread; t < cnt; t += stride) out[pos + t] = rev[n - 1 - skip - t];
    for (int t = first_thread; t < tailLen; t += stride) out[pos + cnt + t] = (int8_t)tailDir;
    return pos + cnt + tailLen;
}

}  // namespace twl
