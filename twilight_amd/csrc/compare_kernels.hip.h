// twilight_amd/csrc/compare_kernels.hip.h -- device side of include/twl_compare.h: an alignment E compared with a reference alignment R of the
// same sequences, exactly, in integers (no floating point in this file).
//
//   compare_refpos_kernel    per R row: pos[k][i] = the R column of the row's i-th letter, the row's letter count, and nR(b) by integer atomics
//   compare_keys_kernel      per E row: key[k][c] = pos[k][rank of the letter at column c], -1 at a gap; a row whose letter count or letters
//                            differ from R's puts 2 * k (count) or 2 * k + 1 (letters) into *bad by an atomic min
//   compare_columns_kernel   per tile of E columns: letters, shared pairs, distinct R columns and the recovered flag of every column
//
// Layout (the builder's choice): everything is ROW-MAJOR with one pitch per alignment, the width rounded up to the column
// tile (64).  The bytes behind a row's width are '-', the keys behind it are -1.  A workgroup of the column kernel owns 64 columns; each of its
// four waves reads one row's 64 keys of the tile per load instruction, a 256-byte aligned run.  The scans give a thread 4 consecutive columns:
// a wave reads 256 bytes of a row per instruction and writes 1024 bytes of keys (one 16-byte store per lane).
//
// The column kernel's counters: s_cnt[T][64], counter (key - lo) of column `lane` at word (key - lo) * 64 + lane.  A 32-lane half of a wave hits 32
// different banks whatever the keys are (ds_add_u32 banks are word % 32), and LDS atomics on one word from several waves serialise exactly.
// 64 KiB of counters + 7 KiB of reduction tables per workgroup (72 712 bytes, 71 KiB): two workgroups share a CU's 160 KiB.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "trim_kernels.hip.h"          // trim_zero_bytes; backbone_kernels.hip.h: squeeze_excl_sum

namespace twl {

constexpr int kCmpThreads = 256;                          // every kernel below runs 256-thread workgroups (four waves)
constexpr int kCmpWaves = kCmpThreads / 64;
constexpr int kCmpWindowLog = 8;
constexpr int kCmpWindow = 1 << kCmpWindowLog;            // T: counters per column and key window
constexpr int kCmpColTile = 64;                           // columns of a tile of the column kernel: a lane per column
constexpr int kCmpUnroll = 8;                             // rows a wave has in flight per step
constexpr int kCmpRowStep = kCmpWaves * kCmpUnroll;       // rows a workgroup takes per step of the column kernel
constexpr int kCmpScanCols = 4;                           // columns a thread of the row scans owns per round
constexpr int kCmpScanChunk = kCmpThreads * kCmpScanCols; // columns the row scans walk per round
static_assert(kCmpThreads == kSqThreads, "squeeze_excl_sum scans kSqThreads values");
static_assert(kCmpColTile == 64, "a lane of a wave per column of the tile");
// words of LDS: the counters; per wave and column four 32-bit tables and one 64-bit table (6 words); per column four 32-bit tables; one word
static_assert((kCmpWindow * kCmpColTile + 6 * kCmpWaves * kCmpColTile + 4 * kCmpColTile + 1) * 4 * 2 <= 160 * 1024, "two workgroups of the column kernel per CU");

struct CompareArgs {
    const unsigned char *est, *ref;   // [n][pe], [n][pr] bytes; '-' behind the widths
    int64_t pe, pr;                   // pitches: we and wr rounded up to kCmpColTile; keys are pitched pe, pos is pitched pr
    int32_t n, we, wr;
    int32_t *pos;                     // [n][pr] R column of every letter of an R row, by rank
    int32_t *keys;                    // [n][pe]
    uint32_t *ref_letters;            // [wr] nR, zeroed before compare_refpos_kernel
    uint32_t *row_letters;            // [n] letters of every R row
    int32_t *bad;                     // [1] INT32_MAX before compare_keys_kernel
    unsigned long long *shared;       // [we] the column kernel's results
    uint32_t *letters, *distinct;     // [we]
    uint8_t *recovered;               // [we]
};

__device__ inline uint32_t compare_load4(const unsigned char *row, int64_t c0, int64_t pitch)
{
    return c0 < pitch ? *reinterpret_cast<const uint32_t *>(row + c0) : 0x2D2D2D2Du;     // (pitch is a multiple of 4: a word is inside or outside)
}
__device__ inline uint32_t compare_fold(uint32_t c) { return (c >= 'a' && c <= 'z') ? c - 32u : c; }

// grid: n rows, 256 threads.  The workgroup walks its R row kCmpScanChunk columns per round with a carry: a thread's 4 bytes, a 1 per gap byte,
// an exclusive sum of the letter counts over the workgroup; every letter writes its column at its rank and adds 1 to its column's count.
__global__ void __launch_bounds__(kCmpThreads) compare_refpos_kernel(CompareArgs a)
{
    __shared__ int s_tmp[kCmpThreads];
    const int64_t k = blockIdx.x;
    const unsigned char *row = a.ref + k * a.pr;
    int32_t *pos = a.pos + k * a.pr;
    int carry = 0;
    for (int64_t base = 0; base < a.pr; base += kCmpScanChunk) {
        const int64_t c0 = base + (int64_t)threadIdx.x * kCmpScanCols;
        const uint32_t gap = trim_zero_bytes(compare_load4(row, c0, a.pr) ^ 0x2D2D2D2Du);
        int tot;
        int at = carry + squeeze_excl_sum(kCmpScanCols - __popc(gap), s_tmp, &tot);
#pragma unroll
        for (int j = 0; j < kCmpScanCols; ++j)
            if (!((gap >> (8 * j)) & 1u)) {                                              // (a letter: c0 + j < wr, the padding is '-')
                pos[at++] = (int32_t)(c0 + j);
                atomicAdd(&a.ref_letters[c0 + j], 1u);
            }
        carry += tot;
    }
    if (threadIdx.x == 0) a.row_letters[k] = (uint32_t)carry;
}

// grid: n rows, 256 threads.  First the row's letter count (a row that holds another count than its R row writes nothing); then the same scan as
// above: the letter of rank i takes pos[k][i] as its key and is compared with R's letter there.
__global__ void __launch_bounds__(kCmpThreads) compare_keys_kernel(CompareArgs a)
{
    __shared__ int s_tmp[kCmpThreads];
    const int64_t k = blockIdx.x;
    const unsigned char *row = a.est + k * a.pe;
    const unsigned char *ref = a.ref + k * a.pr;
    const int32_t *pos = a.pos + k * a.pr;
    int32_t *keys = a.keys + k * a.pe;
    int mine = 0, tot;
    for (int64_t c0 = (int64_t)threadIdx.x * kCmpScanCols; c0 < a.pe; c0 += kCmpScanChunk)
        mine += kCmpScanCols - __popc(trim_zero_bytes(compare_load4(row, c0, a.pe) ^ 0x2D2D2D2Du));
    (void)squeeze_excl_sum(mine, s_tmp, &tot);
    if ((uint32_t)tot != a.row_letters[k]) {                                             // (uniform)
        if (threadIdx.x == 0) atomicMin(a.bad, (int32_t)(2 * k));
        return;
    }
    int carry = 0;
    bool differs = false;
    for (int64_t base = 0; base < a.pe; base += kCmpScanChunk) {
        const int64_t c0 = base + (int64_t)threadIdx.x * kCmpScanCols;
        const uint32_t v = compare_load4(row, c0, a.pe);
        const uint32_t gap = trim_zero_bytes(v ^ 0x2D2D2D2Du);
        int at = carry + squeeze_excl_sum(kCmpScanCols - __popc(gap), s_tmp, &tot);
        int32_t key[kCmpScanCols];
#pragma unroll
        for (int j = 0; j < kCmpScanCols; ++j) {
            key[j] = -1;
            if (!((gap >> (8 * j)) & 1u)) {                                              // (at < the row's letter count == R's: pos[at] is written)
                key[j] = pos[at++];
                differs |= compare_fold((v >> (8 * j)) & 0xFFu) != compare_fold(ref[key[j]]);
            }
        }
        if (c0 < a.pe) *reinterpret_cast<int4 *>(keys + c0) = make_int4(key[0], key[1], key[2], key[3]);
        carry += tot;
    }
    if (differs) atomicMin(a.bad, (int32_t)(2 * k + 1));
}

// grid: column tiles, 256 threads.  Lane l of every wave owns column col0 + l; wave w takes the rows w, w + 4, ... of a step of kCmpRowStep rows.
// Sweep 1: letters, smallest and largest key per column.  Then window j = 0, 1, ... of column c covers the keys [min_c + j T, min_c + (j + 1) T):
// every row's key inside it adds 1 to its counter; behind the sweep the tile's counters are summed (C(k, 2) in 64 bits, non-zero counters
// counted) and zeroed by the thread (l, w) over the counters w, w + 4, ... of column l.  The tile sweeps as often as its widest column needs;
// a column that is through adds nothing and reads none of its counters.
__global__ void __launch_bounds__(kCmpThreads) compare_columns_kernel(CompareArgs a)
{
    __shared__ uint32_t s_cnt[kCmpWindow * kCmpColTile];
    __shared__ uint32_t s_n[kCmpWaves][kCmpColTile], s_dist[kCmpWaves][kCmpColTile];
    __shared__ int32_t s_mn[kCmpWaves][kCmpColTile], s_mx[kCmpWaves][kCmpColTile];
    __shared__ unsigned long long s_sum[kCmpWaves][kCmpColTile];
    __shared__ int32_t s_min[kCmpColTile], s_max[kCmpColTile], s_win[kCmpColTile];
    __shared__ uint32_t s_letters[kCmpColTile];
    __shared__ int s_maxwin;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int64_t col0 = (int64_t)blockIdx.x * kCmpColTile;
    const int32_t *kp = a.keys + col0 + lane;                                           // (col0 + lane < pe)
    const int64_t n = a.n;
    for (int i = (int)threadIdx.x; i < kCmpWindow * kCmpColTile; i += kCmpThreads) s_cnt[i] = 0;
    if (threadIdx.x == 0) s_maxwin = 0;

    uint32_t cnt = 0;
    int32_t mn = INT32_MAX, mx = -1;
    for (int64_t base = 0; base < n; base += kCmpRowStep) {
        int32_t v[kCmpUnroll];
#pragma unroll
        for (int u = 0; u < kCmpUnroll; ++u) { const int64_t k = base + u * kCmpWaves + wave; v[u] = k < n ? kp[k * a.pe] : -1; }
#pragma unroll
        for (int u = 0; u < kCmpUnroll; ++u)
            if (v[u] >= 0) { ++cnt; mn = min(mn, v[u]); mx = max(mx, v[u]); }
    }
    s_n[wave][lane] = cnt; s_mn[wave][lane] = mn; s_mx[wave][lane] = mx;
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int w = 1; w < kCmpWaves; ++w) { cnt += s_n[w][lane]; mn = min(mn, s_mn[w][lane]); mx = max(mx, s_mx[w][lane]); }
        const int win = cnt ? ((mx - mn) >> kCmpWindowLog) + 1 : 0;
        s_letters[lane] = cnt; s_min[lane] = mn; s_max[lane] = mx; s_win[lane] = win;
        atomicMax(&s_maxwin, win);
    }
    __syncthreads();
    const int32_t myMin = s_min[lane];
    const int myWin = s_win[lane], maxWin = s_maxwin;

    unsigned long long sum = 0;
    uint32_t dist = 0;
    for (int j = 0; j < maxWin; ++j) {
        if (j < myWin) {
            for (int64_t base = 0; base < n; base += kCmpRowStep) {
                int32_t v[kCmpUnroll];
#pragma unroll
                for (int u = 0; u < kCmpUnroll; ++u) { const int64_t k = base + u * kCmpWaves + wave; v[u] = k < n ? kp[k * a.pe] : -1; }
#pragma unroll
                for (int u = 0; u < kCmpUnroll; ++u) {
                    const int32_t d = v[u] - myMin;                                      // (0 <= d for a key: both lie in [0, wr))
                    if (v[u] >= 0 && (d >> kCmpWindowLog) == j) atomicAdd(&s_cnt[(d & (kCmpWindow - 1)) * kCmpColTile + lane], 1u);
                }
            }
        }
        __syncthreads();
        if (j < myWin) {
            for (int off = wave; off < kCmpWindow; off += kCmpWaves) {
                const uint32_t c = s_cnt[off * kCmpColTile + lane];
                if (c) {
                    sum += (unsigned long long)c * (unsigned long long)(c - 1u) / 2ull;
                    ++dist;
                    s_cnt[off * kCmpColTile + lane] = 0;
                }
            }
        }
        __syncthreads();
    }
    s_sum[wave][lane] = sum; s_dist[wave][lane] = dist;
    __syncthreads();
    if (wave == 0 && col0 + lane < a.we) {
#pragma unroll
        for (int w = 1; w < kCmpWaves; ++w) { sum += s_sum[w][lane]; dist += s_dist[w][lane]; }
        const uint32_t letters = s_letters[lane];
        const int64_t c = col0 + lane;
        a.shared[c] = sum;
        a.letters[c] = letters;
        a.distinct[c] = dist;
        a.recovered[c] = (uint8_t)((letters >= 2 && myMin == s_max[lane] && a.ref_letters[myMin] == letters) ? 1 : 0);
    }
}

}  // namespace twl
