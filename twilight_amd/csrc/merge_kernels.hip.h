// twilight_amd/csrc/merge_kernels.hip.h -- device side of the merge of existing alignments (include/twl_merge.h): how the columns of
// every input alignment move as the merges pile up (the reference's SequenceDB::subtreeAln), and the one rewrite of every row at the end.
//
//   merge_iota_kernel      the identity maps of twl_merge_create
//   merge_ranks_kernel     per final path: rpos[r] = position of the r-th code != 1, qpos[q] = position of the q-th code != 2
//                          (what src/alignment-helper.cpp:409-418 / :456-465 walk per input alignment, once per path here)
//   merge_compose_kernel   pos_g[c] = rpos[pos_g[c]] (reference side) / qpos[pos_g[c]] (query side), all groups of a level in one launch
//   merge_inverse_kernel   inv_g[pos_g[c]] = c over a table of -1
//   merge_rewrite_kernel   out[w] = inv_g[w] >= 0 ? row[inv_g[w]] : '-'  (src/io.cpp:383-392)
//
// Path codes: 0 = both, 1 = query only, 2 = reference only.  Conventions of place_kernels.hip.h: 256-thread workgroups, paths walked in
// LDS-staged tiles of kPlTile codes.  All byte / int streams, HBM-bound; plain vector loads and stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "place_kernels.hip.h"

namespace twl {

constexpr int kMgCols = 16;                        // columns per thread of the rewrite: one 16-byte store
constexpr int kMgColTile = kPlThreads * kMgCols;   // columns per workgroup of the rewrite
constexpr int kMgRows = 16;                        // rows per workgroup of the rewrite (they share the inverse map held in registers)

// grid: (n_groups, ceil(maxL / 256)): pos[pos_off[g] + c] = c
__global__ void __launch_bounds__(kPlThreads) merge_iota_kernel(const int64_t *pos_off, const int32_t *L, int32_t *pos)
{
    const int g = blockIdx.x;
    const int c = blockIdx.y * kPlThreads + threadIdx.x;
    if (c < L[g]) pos[pos_off[g] + c] = c;
}

// grid: n_paths, 256 threads.  One workgroup walks its path a tile at a time; inside a tile, 256 codes per round: every wave ranks its 64
// codes with a ballot and a popcount of the lanes below, the four wave totals meet in LDS (two buffers, so one barrier per round), and
// the totals are carried over the rounds and tiles.  A rank at or beyond the side's width is counted but not stored: counts[t] = {codes
// != 1, codes != 2, a code outside 0..2 seen}, which the host checks before anything is composed.
struct RankArgs {
    PathSrc from;                // [n] where every path lives (place_kernels.hip.h)
    const int32_t *wr, *wq;      // [n] width of the reference / query side
    const int64_t *r_off, *q_off;   // [n] where rpos / qpos start in ranks
    int32_t *ranks;
    int32_t *counts;             // [n][3]
};

__global__ void __launch_bounds__(kPlThreads) merge_ranks_kernel(RankArgs a)
{
    __shared__ int8_t s_tile[kPlTile];
    __shared__ int s_wave[2][2][kPlThreads / 64];
    __shared__ int s_bad;
    const int t = blockIdx.x;
    const int8_t *path = a.from.path(t);
    const int32_t n = a.from.plen[t], wr = a.wr[t], wq = a.wq[t];
    int32_t *rpos = a.ranks + a.r_off[t], *qpos = a.ranks + a.q_off[t];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    if (threadIdx.x == 0) s_bad = 0;
    int R = 0, Q = 0, bad = 0, round = 0;      // R, Q: carried over the rounds
    for (int base = 0; base < n; base += kPlTile) {
        const int m = min(kPlTile, n - base);
        for (int j = threadIdx.x; j < m; j += kPlThreads) s_tile[j] = path[base + j];
        __syncthreads();
        for (int j0 = 0; j0 < m; j0 += kPlThreads, ++round) {
            const int j = j0 + (int)threadIdx.x;
            const bool in = j < m;
            const int v = in ? (int)s_tile[j] : 0;
            if (in && (v < 0 || v > 2)) bad = 1;
            const bool isR = in && v != 1, isQ = in && v != 2;
            const unsigned long long bR = __ballot(isR), bQ = __ballot(isQ);
            int (*w)[kPlThreads / 64] = s_wave[round & 1];
            if (lane == 0) { w[0][wave] = __popcll(bR); w[1][wave] = __popcll(bQ); }
            __syncthreads();
            int r = R + __popcll(bR & below), q = Q + __popcll(bQ & below);
#pragma unroll
            for (int k = 0; k < kPlThreads / 64; ++k) {
                if (k < wave) { r += w[0][k]; q += w[1][k]; }
                R += w[0][k]; Q += w[1][k];
            }
            if (isR && r < wr) rpos[r] = base + j;
            if (isQ && q < wq) qpos[q] = base + j;
        }
        __syncthreads();                       // (s_tile is restaged next)
    }
    if (bad) s_bad = 1;
    __syncthreads();
    if (threadIdx.x == 0) { a.counts[3 * t] = R; a.counts[3 * t + 1] = Q; a.counts[3 * t + 2] = s_bad; }
}

// grid: (n_jobs, ceil(maxL / 256)), one job per group under a side of the level: the group's map through that side's rank table
struct ComposeJob { int64_t pos_off, tab_off; int32_t L, tab_len; };

__global__ void __launch_bounds__(kPlThreads) merge_compose_kernel(const ComposeJob *jobs, const int32_t *ranks, int32_t *pos)
{
    const ComposeJob jb = jobs[blockIdx.x];
    const int c = blockIdx.y * kPlThreads + threadIdx.x;
    if (c >= jb.L) return;
    const int32_t p = pos[jb.pos_off + c];
    if (p >= 0 && p < jb.tab_len) pos[jb.pos_off + c] = ranks[jb.tab_off + p];
}

// grid: (n_groups, ceil(maxL / 256)): inv[g * pitch + pos_g[c]] = c; the table holds -1 everywhere else (pitch >= W, a multiple of kMgCols)
__global__ void __launch_bounds__(kPlThreads) merge_inverse_kernel(const int64_t *pos_off, const int32_t *L, const int32_t *pos, int32_t W, int64_t pitch, int32_t *inv)
{
    const int g = blockIdx.x;
    const int c = blockIdx.y * kPlThreads + threadIdx.x;
    if (c >= L[g]) return;
    const int32_t p = pos[pos_off[g] + c];
    if (p >= 0 && p < W) inv[(int64_t)g * pitch + p] = c;
}

// grid: (ceil(W / kMgColTile), n_slices), 256 threads.  A slice is up to kMgRows rows of one group.  A thread owns kMgCols consecutive
// columns: it loads their entries of the group's inverse map once (four aligned 16-byte loads), then builds 16 bytes of every row of the
// slice and stores them with one 16-byte store (the planes' pitch is a multiple of 256 bytes, so column 16k of a row is 16-byte aligned);
// the last, partial chunk of a row goes out byte by byte.  Rows are read from their current plane and written to the other one.
struct RewriteArgs {
    const char *rows0, *rows1;   // current planes
    char *out0, *out1;           // the same planes, written on the other side: out[plane ^ 1]
    int64_t cap;
    const int32_t *ids;          // [n_rows] store ids, group by group
    const uint8_t *plane;        // [n_rows] current plane of each
    const int32_t *slice_group, *slice_first, *slice_n;   // [n_slices] group, first entry of ids, rows
    const int32_t *L;            // [n_groups]
    const int32_t *inv;          // [n_groups][pitch]
    int64_t pitch;
    int32_t W;
};

__global__ void __launch_bounds__(kPlThreads) merge_rewrite_kernel(RewriteArgs a)
{
    const int w0 = (blockIdx.x * kPlThreads + threadIdx.x) * kMgCols;
    if (w0 >= a.W) return;
    const int sl = blockIdx.y;
    const int g = a.slice_group[sl], first = a.slice_first[sl], n = a.slice_n[sl];
    const int32_t L = a.L[g];
    int32_t src[kMgCols];
    const int4 *iv = reinterpret_cast<const int4 *>(a.inv + (int64_t)g * a.pitch + w0);
#pragma unroll
    for (int k = 0; k < kMgCols / 4; ++k) {
        const int4 v = iv[k];
        src[4 * k] = v.x; src[4 * k + 1] = v.y; src[4 * k + 2] = v.z; src[4 * k + 3] = v.w;
    }
#pragma unroll
    for (int k = 0; k < kMgCols; ++k) if (src[k] >= L) src[k] = -1;
    const bool whole = w0 + kMgCols <= a.W;
    for (int r = 0; r < n; ++r) {
        const int s = a.ids[first + r];
        const bool pl = a.plane[first + r] != 0;
        const char *row = (pl ? a.rows1 : a.rows0) + (size_t)s * a.cap;
        char *out = (pl ? a.out0 : a.out1) + (size_t)s * a.cap + w0;
        unsigned int word[kMgCols / 4];
#pragma unroll
        for (int k = 0; k < kMgCols / 4; ++k) {
            unsigned int v = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int c = src[4 * k + b];
                const unsigned int ch = c >= 0 ? (unsigned int)(unsigned char)row[c] : (unsigned int)'-';
                v |= ch << (8 * b);
            }
            word[k] = v;
        }
        if (whole) *reinterpret_cast<uint4 *>(out) = make_uint4(word[0], word[1], word[2], word[3]);
        else {
#pragma unroll
            for (int k = 0; k < kMgCols; ++k)
                if (w0 + k < a.W) out[k] = (char)((word[k >> 2] >> (8 * (k & 3))) & 0xFF);
        }
    }
}

}  // namespace twl
