// twilight_amd/csrc/keep_kernels.hip.h -- device side of the placement finish that keeps the backbone's length (include/twl_keep.h,
// `twilight-mi355x -a ... --keep-length`): every placed sequence becomes a row of the backbone's L columns, its insertions are left out
// and reported.
//
//   keep_rows_kernel   the row of every collected sequence, on its other plane, and its dropped runs and letters
//   keep_runs_kernel   one (col, qpos, len) record per dropped run of the listed sequences
//
// Path codes as in place_kernels.hip.h: 0 = both, 1 = query only (an insertion: dropped here), 2 = backbone only.  A run is a maximal
// stretch of code 1; it ends on a code 1 that another code or the end of the path follows.  Byte / int streams, HBM-bound.
#pragma once
#include "place_kernels.hip.h"

namespace twl {

// grid: n collected sequences, 256 threads.  Row t is read from its current plane and written to the other one (a sequence may be longer
// than L: never in place).  Every column of [0, L) is written exactly once: by its path code, and '-' behind a path that covers fewer
// than L columns (collect has checked its shape already).  Reads stay inside [0, qlen).
struct KeepRowsArgs {
    const char *rows0, *rows1;   // current planes (the sequence itself)
    char *out0, *out1;           // the same planes, written on the other side: out[plane ^ 1]
    int64_t cap;
    const int32_t *ids;          // [n] store ids
    const uint8_t *plane;        // [n] current plane of each
    const int32_t *qlen;         // [n]
    const int64_t *path_off;     // [n] into arena
    const int32_t *plen;         // [n]
    const int8_t *arena;
    int32_t *runs, *letters;     // [n] dropped runs and letters of each
    int32_t L;
};

__global__ void __launch_bounds__(kPlThreads) keep_rows_kernel(KeepRowsArgs a)
{
    __shared__ int s_red[kPlThreads];
    const int t = blockIdx.x;
    const int s = a.ids[t];
    const char *row = (a.plane[t] ? a.rows1 : a.rows0) + (size_t)s * a.cap;
    char *out = (a.plane[t] ? a.out0 : a.out1) + (size_t)s * a.cap;
    const int8_t *path = a.arena + a.path_off[t];
    const int32_t n = a.plen[t], ql = a.qlen[t];
    int runs = 0, letters = 0, tc, tq;
    scan_path(path, n, [&](int, int8_t) {}, [&](int p, int v, int c, int q, int) {
        if (v == 1) {
            ++letters;
            if (p + 1 == n || path[p + 1] != 1) ++runs;
        } else if (c < a.L) {
            out[c] = (v == 0 && q < ql) ? row[q] : '-';
        }
    }, &tc, &tq);
    for (int c = max(tc, 0) + (int)threadIdx.x; c < a.L; c += kPlThreads) out[c] = '-';
    int totRuns, totLetters;
    block_excl_sum(runs, s_red, &totRuns);
    block_excl_sum(letters, s_red, &totLetters);
    if (threadIdx.x == 0) { a.runs[t] = totRuns; a.letters[t] = totLetters; }
}

// scan_path with one more scanned quantity: f(p, code, c, q, last, rank, end) also receives rank = run ends before p and end = whether a run
// ends at p.  Every thread of the block calls it; *tot_r receives the number of runs of the path.
template <class F>
__device__ void scan_path_runs(const int8_t *path, int32_t n, F f, int *tot_r)
{
    __shared__ int8_t s_tile[kPlTile];
    __shared__ int s_tmp[kPlThreads];
    int C = 0, Q = 0, M = -1, R = 0;           // carried over the tiles
    for (int base = 0; base < n; base += kPlTile) {
        const int m = min(kPlTile, n - base);
        for (int j = threadIdx.x; j < m; j += kPlThreads) s_tile[j] = path[base + j];
        __syncthreads();
        // the code behind the tile decides whether a run ends on the tile's last code (0: any code but 1, also for the end of the path)
        const int8_t behind = base + m < n ? path[base + m] : (int8_t)0;
        const int j0 = threadIdx.x * kPlItems, j1 = min(m, j0 + kPlItems);
        int a = 0, b = 0, e = 0, last = -1;
        for (int j = j0; j < j1; ++j) {
            const int8_t v = s_tile[j];
            if (v != 1) { ++a; last = base + j; }
            if (v != 2) ++b;
            if (v == 1 && (j + 1 < m ? s_tile[j + 1] : behind) != 1) ++e;
        }
        int ta, tb, tl, te;
        int c = C + block_excl_sum(a, s_tmp, &ta);
        int q = Q + block_excl_sum(b, s_tmp, &tb);
        int r = R + block_excl_sum(e, s_tmp, &te);
        int lst = max(M, block_excl_max(last, s_tmp, &tl));
        for (int j = j0; j < j1; ++j) {
            const int8_t v = s_tile[j];
            const bool end = v == 1 && (j + 1 < m ? s_tile[j + 1] : behind) != 1;
            f(base + j, (int)v, c, q, lst, r, end);
            if (v != 1) { ++c; lst = base + j; }
            if (v != 2) ++q;
            if (end) ++r;
        }
        C += ta; Q += tb; R += te; M = max(M, tl);
        __syncthreads();                       // (s_tile is restaged next)
    }
    *tot_r = R;
}

// grid: n listed sequences, 256 threads.  The run of sequence t that ends at position p with rank r (run ends before p) becomes record
// run_off[t] + r: col = backbone columns in front of it, len = p - last (last: the carried position of the last code != 1, so a run
// that crosses or fills tiles needs no second pass), qpos = index of its first letter.  A rank outside [0, n_runs[t]) writes nothing.
struct KeepRunsArgs {
    const int64_t *path_off;     // [n] into arena
    const int32_t *plen;         // [n]
    const int64_t *run_off;      // [n] first record of each
    const int32_t *n_runs;       // [n] records of each (what keep_rows_kernel counted)
    const int8_t *arena;
    int32_t *col, *qpos, *len;   // [total records]
};

__global__ void __launch_bounds__(kPlThreads) keep_runs_kernel(KeepRunsArgs a)
{
    const int t = blockIdx.x;
    const int64_t at = a.run_off[t];
    const int32_t cnt = a.n_runs[t];
    int tr;
    scan_path_runs(a.arena + a.path_off[t], a.plen[t], [&](int p, int, int c, int q, int last, int rank, bool end) {
        if (end && rank >= 0 && rank < cnt) {
            const int len = p - last;
            a.col[at + rank] = c;
            a.qpos[at + rank] = q - (len - 1);
            a.len[at + rank] = len;
        }
    }, &tr);
}

}  // namespace twl
