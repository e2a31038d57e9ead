// twilight_amd/csrc/talco_mt.hip.h -- tile-parallel alignment: the design note of the MT instantiations of talco_lean_kernel (talco_nuc.hip.h), the
// record layout, and what runs around those launches: mt_chain_kernel (tile starts from the scouts' path samples), the scouts' start cells, and
// mt_anchor_kernel (where the consensus letters of the two profiles put the path).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace twl {

// ---- tile-parallel alignment (MT != 0) ----
// A tile is a pure function of its start cell (TALCO-XDrop.cpp:77-93: Tile() reads reference_idx / query_idx and `tile == 0`, nothing else
// of the previous tile), and every tile after the first advances ref_idx + qry_idx by marker or marker - 1 (:616-619).  So if the start
// cells of all tiles of a pair were known, the tiles could run side by side on as many compute units.  They can be PREDICTED: a DP that
// starts a few hundred anti-diagonals before a tile boundary, from a cell merely NEAR the optimal path, runs into that path (the band
// opens by a row per diagonal, the X-drop keeps everything within `xdrop` of the best cell) and from there on its traceback path IS the
// optimal path.  Four launches per level:
//   MT 2  scouts   one workgroup per (pair, tile boundary t): a short tile from the cell of anti-diagonal (marker-1)*t - 1 - lead that lies on
//                  the straight line between the corners, stopped right after its own marker (placed mt_marg diagonals behind the boundary
//                  range), traced back from the better of the best cells of its two marker diagonals; writes where its path crosses the
//                  anti-diagonals [(marker-1)*t - 1, marker*t + 1] into mt_spath
//   MT 4  pair scout  one workgroup per pair (wide re-runs, round 4): the DP from (0, 0) to the last anti-diagonal with every traceback word kept, no
//                  marker and no convergence test; its path from the end cell gives mt_spath for ALL anti-diagonals.  For pairs whose tiles do not
//                  converge (diffuse profiles: every tile runs to the end of the pair and its successor starts where the path from the END cell
//                  crosses the marker diagonal) a local scout cannot know that path; the suffix of the pair's global path does
//   (mt_chain_kernel: walks mt_spath from (0, 0): start of tile t = the path cell on diagonal s + marker, or on s + marker - 1 when the
//                  path steps over that diagonal -- the reference's state 3, :520-524)
//   MT 1  tiles    one workgroup per (pair, tile): the tile from the predicted start, result + path segment into mt_rec / mt_seg
//   MT 3  stitch   one workgroup per pair runs the ordinary tile loop; a tile whose TRUE start equals the start a record was computed
//                  from takes the record (same function, same argument), any other tile is computed in line as always.
// A wrong prediction that also gets the anti-diagonal wrong (marker vs marker - 1) would shift every later boundary of the pair, so the
// chain / tiles / stitch launches run in ROUNDS: a stitch launch that is not the last one suspends a pair at the first tile without a
// matching record (mt_front), the next chain launch re-derives the pair's remaining starts from that TRUE cell, the next tile launch runs
// the tiles whose record does not match the new prediction; the last stitch launch computes whatever is still missing in line.
// Results are those of the plain loop by construction; predictions only decide how much of it is already done.
constexpr int kMtRec = 12;     // {1 = valid / 2 = the job failed, start ref, start qry, next ref, next qry, last_tile, segment bytes, tail dir, tail len, band cells, error code of a failed job, its window rows}

// start cells of all tiles of a pair from the scouts' path samples (one thread per pair)
__global__ void mt_chain_kernel(const int32_t *spath, int sp_pitch, const int32_t *len, const int32_t *items, int n_items, int32_t *chain, int slots,
                                int marker, int perturb, const int32_t *front)
{
    const int it = blockIdx.x * blockDim.x + threadIdx.x;
    if (it >= n_items) return;
    const int pair = items[it];
    const int R = len[2 * pair], Q = len[2 * pair + 1];
    // (the tables of a tile-parallel level are indexed by the pair's position in the launch, not by its id: they cost memory and fills for the pairs that run only)
    const int32_t *sp = spath + (size_t)it * (size_t)sp_pitch;
    int32_t *ch = chain + (size_t)it * (size_t)slots * 2;
    const int32_t *fr = front + (size_t)it * 8;
    if (fr[0] == 2) return;                       // the pair is finished
    int s = 0, t = 1;
    if (fr[0] == 1) {                             // later rounds: from the true start of the first tile without a record
        t = fr[1];
        if (t >= slots) return;
        ch[2 * t] = fr[2]; ch[2 * t + 1] = fr[3];
        s = fr[2] + fr[3];
        t += 1;
    } else { ch[0] = 0; ch[1] = 0; }
    for (; t < slots; ++t) {
        const int d = s + marker;
        if (d > R + Q - 2) break;
        int q = sp[d];
        if (q >= 0) s = d;
        else if (q == -1 && d - 1 > s && sp[d - 1] >= 0) { q = sp[d - 1]; s = d - 1; }
        else break;
        int r = s - q;
        // development / test aid: spoil every perturb-th prediction, so that the stitch kernel has tiles to compute in line
        if (perturb > 0 && (t % perturb) == 0) { if (q > 0 && r + 1 < R) { q -= 1; r += 1; } else if (r > 0 && q + 1 < Q) { q += 1; r -= 1; } }
        if (r < 0 || r >= R || q >= Q) break;
        ch[2 * t] = r; ch[2 * t + 1] = q;
    }
    for (; t < slots; ++t) { ch[2 * t] = -1; ch[2 * t + 1] = -1; }
}

// ---- anchored scouts (round 5) ----
// A scout needs its long lead (320 anti-diagonals) because the straight line between the corners is up to ~55 rows off the path on the families
// measured: the band has to open that far before the scout can run into the path.  Where the path IS can be read off the profiles before any DP: around
// the cell of the straight line the consensus letters of the two profiles agree on one diagonal offset and on no other (tests/study/tile_predict_study.c:
// +-32 columns, offsets -128..127).  mt_anchor_kernel finds that offset for every tile boundary; a scout whose anchor is trusted -- or lies between two
// trusted ones that agree (the path drifts by a few rows per tile; an offset that jumps is a long indel and says nothing about its neighbours) -- starts
// from the anchored cell only mt_lead2 (96) anti-diagonals ahead.  On the 154 pairs of levels 15-31 of 10 000 x 10 kbp (the CPU study, with the nine windows of
// mt_anchor_kernel): all but 2 of 3080 boundaries anchored, 3078 true starts found against 3079 with the long lead, 61 % fewer scout diagonals; on the device the scouts of a
// pass 39 -> 15 ms.  Predictions only: a wrong anchor costs what any wrong prediction costs -- a second round of its level.
constexpr int kAnchorHalf = 32, kAnchorOffsets = 256, kAnchorNear = 3, kAnchorJump = 12;
constexpr int kAnchorMinMatches = 36, kAnchorMinGap = 8;      // trusted: >= 55 % of the 64 columns agree and the best other offset (not a neighbour) is >= 12 % behind

// the cell of anti-diagonal d0 on the straight line between the corners (false: none)
__device__ __forceinline__ bool scout_line_cell(int d0, int R, int Q, int &r, int &q)
{
    q = (int)(((long long)d0 * Q) / (R + Q));
    q = min(q, Q - 1);
    r = d0 - q;
    if (r > R - 1) { r = R - 1; q = d0 - r; }
    return !(q > Q - 1 || r < 0);
}
// the anchor of boundary `slot` of a pair from the table of its row: its own when trusted, else between two trusted neighbours that agree
__device__ __forceinline__ bool scout_anchor(const int32_t *an, int slot, int slots, int &o)
{
    const int w = __builtin_amdgcn_readfirstlane(an[slot]);
    if (w >= 0) { o = w - 128; return true; }
    int l = -1, r = -1, ol = 0, orr = 0;
    for (int u = 1; u <= kAnchorNear; ++u) {
        if (l < 0 && slot - u >= 1) { const int v = __builtin_amdgcn_readfirstlane(an[slot - u]); if (v >= 0) { l = slot - u; ol = v - 128; } }
        if (r < 0 && slot + u < slots) { const int v = __builtin_amdgcn_readfirstlane(an[slot + u]); if (v >= 0) { r = slot + u; orr = v - 128; } }
    }
    if (l < 0 || r < 0 || abs(orr - ol) > kAnchorJump * (r - l)) return false;
    o = ol + (orr - ol) * (slot - l) / (r - l);
    return true;
}
// the anchored start cell on anti-diagonal d0: q - r moved by o (rounded away from zero to an even step)
__device__ __forceinline__ bool scout_anchored_cell(int d0, int R, int Q, int o, int &r, int &q)
{
    int r0, q0;
    if (!scout_line_cell(d0, R, Q, r0, q0)) return false;
    q = q0 + (o >= 0 ? (o + 1) / 2 : -((-o + 1) / 2));
    r = d0 - q;
    if (q < 0) { q = 0; r = d0; }
    if (r < 0) { r = 0; q = d0; }
    return q < Q && r < R;
}

// one workgroup of 256 threads per scout job {pair, slot, row}: thread t counts the columns i in [-32, 32) with consensus(ref, r0 + i) == consensus(qry, q0 + i + t - 128),
// first in the window around the straight line's cell, then -- until one is trusted -- in windows moved along the diagonal by +24, -24, +48, ... -96 columns (the path's
// offset is the same a few columns on unless an indel lies between; the top 52 pairs of 10 000 x 10 kbp: 18 % of the boundaries without an anchor with the one window, 0.2 % with the nine)
constexpr int kAnchorShift = 24, kAnchorShifts = 4, kAnchorPad = kAnchorShift * kAnchorShifts;
template <int P>
__global__ __launch_bounds__(256) void mt_anchor_kernel(const float *cols, const int32_t *len, int seq_len, const int32_t *jobs, int n_jobs, int32_t *anchor, int slots, int marker, int lead2)
{
    static_assert(kAnchorOffsets == 256 && 2 * kAnchorHalf + 2 * kAnchorPad == 256, "one thread per offset, one per staged reference letter");
    __shared__ unsigned char s_r[2 * kAnchorHalf + 2 * kAnchorPad], s_q[2 * kAnchorHalf + 2 * kAnchorPad + kAnchorOffsets];
    __shared__ int s_cnt[kAnchorOffsets], s_done;
    const int job = blockIdx.x;
    if (job >= n_jobs) return;
    const int pair = jobs[3 * job], slot = jobs[3 * job + 1], row = jobs[3 * job + 2];
    const int R = len[2 * pair], Q = len[2 * pair + 1];
    const int spLo = (marker - 1) * slot - 1;
    const int d0 = max(spLo - lead2, 0);
    int r0, q0;
    if (spLo > R + Q - 2 || R < 2 || Q < 2 || !scout_line_cell(d0, R, Q, r0, q0)) return;      // (the table is filled with -1)
    // consensus letter of a column: the most frequent of A, C, G, T (of the twenty amino acids) when it is at least as frequent as the gap; else a letter that matches nothing
    auto letter = [&](int side, int col, int n) -> unsigned char {
        if (col < 0 || col >= n) return (unsigned char)(100 + side);
        const float *pf = cols + (((size_t)pair * 2 + side) * (size_t)seq_len + col) * (P + 2);
        int best = 0; float bc = pf[0];
        for (int j = 1; j < P - 2; ++j) if (pf[j] > bc) { bc = pf[j]; best = j; }
        return (bc > 0.0f && bc >= pf[P - 1]) ? (unsigned char)best : (unsigned char)(100 + side);
    };
    const int t = threadIdx.x;
    s_r[t] = letter(0, r0 - kAnchorHalf - kAnchorPad + t, R);
    for (int u = t; u < 2 * kAnchorHalf + 2 * kAnchorPad + kAnchorOffsets; u += 256) s_q[u] = letter(1, q0 - kAnchorHalf - kAnchorPad - kAnchorOffsets / 2 + u, Q);
    if (t == 0) s_done = 0;
    __syncthreads();
    for (int sh = 0; sh <= 2 * kAnchorShifts; ++sh) {
        const int base = kAnchorPad + ((sh == 0) ? 0 : ((sh & 1) ? kAnchorShift * ((sh + 1) / 2) : -kAnchorShift * (sh / 2)));
        int c = 0;
        for (int i = 0; i < 2 * kAnchorHalf; ++i) c += (s_r[base + i] == s_q[base + i + t]) ? 1 : 0;      // offset o = t - 128
        s_cnt[t] = c;
        __syncthreads();
        if (t < 64) {
            // the best offset: most matches, ties to the smallest |o|, the negative one first (the order 0, -1, 1, -2, 2, ... of the study)
            int key = -1;
            for (int u = t; u < kAnchorOffsets; u += 64) {
                const int o = u - kAnchorOffsets / 2;
                const int rank = (o == 0) ? 0 : (o < 0 ? -2 * o - 1 : 2 * o);
                key = max(key, (s_cnt[u] << 16) | (0xFFFF - rank));
            }
            for (int m = 32; m >= 1; m >>= 1) key = max(key, __shfl_xor(key, m, 64));
            const int rank = 0xFFFF - (key & 0xFFFF);
            const int bo = (rank == 0) ? 0 : ((rank & 1) ? -(rank + 1) / 2 : rank / 2);
            int second = -1;
            for (int u = t; u < kAnchorOffsets; u += 64) if (abs(u - kAnchorOffsets / 2 - bo) > 2) second = max(second, s_cnt[u]);
            for (int m = 32; m >= 1; m >>= 1) second = max(second, __shfl_xor(second, m, 64));
            const int bc = key >> 16;
            if (t == 0 && bc >= kAnchorMinMatches && bc - second >= kAnchorMinGap) { anchor[(size_t)row * slots + slot] = 128 + bo; s_done = 1; }
        }
        __syncthreads();
        if (s_done) break;
    }
}

}  // namespace twl
