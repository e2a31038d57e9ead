// twilight_amd/csrc/trim_kernels.hip.h -- device side of include/twl_trim.h: the gappy columns taken out of every listed row of the store,
// by one keep table for all rows (the backbone squeeze, backbone_kernels.hip.h, has one per group and only the all-gap rule).
//
//   trim_counts_kernel    gaps[c] = listed rows that hold '-' at column c (exact: integer atomics)
//   trim_bits_kernel      one keep bit per column, from the counts (TWL_TRIM_MAX_GAPS) or from one row (TWL_TRIM_TO_ROW)
//   trim_scan_kernel      the bits counted into destination indices, one int per 32-column word, and the kept total
//   trim_list_kernel      the kept columns' original indices, ascending
//   trim_compact_kernel   every listed row's kept bytes, in order, into its other plane
//
// Rows are cap-pitched, cap is a multiple of 16 and above every row length (the driver refuses another pitch), so the 16 bytes at column
// 16k < W of any row lie inside the row's pitch: every kernel reads whole 16-byte words, and what lies behind column W never counts (the
// counts are not added there, the keep bits are zero there).
// All byte / int streams, HBM-bound: the rows are read twice and written once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "backbone_kernels.hip.h"      // squeeze_excl_sum

namespace twl {

constexpr int kTrThreads = 256;                       // every kernel below runs 256-thread workgroups
constexpr int kTrCols = 16;                           // columns a thread owns: one 16-byte load per row
constexpr int kTrColTile = kTrThreads * kTrCols;      // columns of a tile (counts and compaction)
constexpr int kTrRowSlice = 512;                      // rows a counts workgroup sums before its atomics
constexpr int kTrFlush = 252;                         // rows a packed byte counter takes before it is flushed into 32-bit counters (4 rows per step)
constexpr int kTrScanChunk = kTrThreads * 32;         // columns the scan walks per round: one 32-column word per thread
static_assert(kTrFlush <= 255 && kTrFlush % 4 == 0, "a byte counter holds 255; the row loop steps by 4");
static_assert(kTrThreads == kSqThreads, "squeeze_excl_sum scans kSqThreads values");

// What the kernels share: the W columns of the n listed rows (row k: store id ids[k] on plane plane[k]).
struct TrimArgs {
    const char *rows0, *rows1;   // current planes
    char *out0, *out1;           // the same planes, written on the other side: out[plane ^ 1]
    int64_t cap;
    const int32_t *ids;          // [n]
    const uint8_t *plane;        // [n]
    int32_t n, W;
    int32_t rule, arg;           // TWL_TRIM_MAX_GAPS: arg = the gap limit; TWL_TRIM_TO_ROW: arg = the index in ids of the reference row
    uint32_t *gaps;              // [W], zeroed before the first launch
    uint32_t *flags;             // [ceil(W / 32)] keep bits
    int32_t *pre;                // [ceil(W / 32) + 1] kept columns in front of every word; at the end the kept total
    int32_t *cols;               // [W] the kept columns (the first `kept` entries)
    int32_t *kept;               // [1]
};

// per byte of x: 1 where the byte is zero, 0 elsewhere
__device__ inline uint32_t trim_zero_bytes(uint32_t x)
{
    const uint32_t t = ((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x;      // bit 7 of a byte: the byte is not zero
    return (~t >> 7) & 0x01010101u;
}

// grid: (column tiles, row slices), 256 threads.  A thread owns 16 consecutive columns of its slice's rows: per row one 16-byte load, XOR with
// '-', a 1 per zero byte added to four words of packed byte counters; the packed counters are flushed into 16 32-bit counters every kTrFlush
// rows.  The workgroup's counts go through LDS so that one wave adds to 64 consecutive counters (a 256-byte run per atomic instruction).
__global__ void __launch_bounds__(kTrThreads) trim_counts_kernel(TrimArgs a)
{
    __shared__ uint32_t s_cnt[kTrColTile];
    const int32_t col0 = (int)blockIdx.x * kTrColTile;
    const int32_t col = col0 + (int)threadIdx.x * kTrCols;
    const int32_t r0 = (int)blockIdx.y * kTrRowSlice;
    const int32_t r1 = min(a.n, r0 + kTrRowSlice);
    uint32_t cnt[kTrCols];
#pragma unroll
    for (int j = 0; j < kTrCols; ++j) cnt[j] = 0;
    if (col < a.W) {
        for (int32_t f0 = r0; f0 < r1; f0 += kTrFlush) {
            const int32_t f1 = min(r1, f0 + kTrFlush);
            uint32_t acc[4] = {0, 0, 0, 0};
            int32_t k = f0;
            for (; k + 4 <= f1; k += 4) {
                uint4 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    v[u] = *reinterpret_cast<const uint4 *>((a.plane[k + u] ? a.rows1 : a.rows0) + (size_t)a.ids[k + u] * (size_t)a.cap + col);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    acc[0] += trim_zero_bytes(v[u].x ^ 0x2D2D2D2Du); acc[1] += trim_zero_bytes(v[u].y ^ 0x2D2D2D2Du);
                    acc[2] += trim_zero_bytes(v[u].z ^ 0x2D2D2D2Du); acc[3] += trim_zero_bytes(v[u].w ^ 0x2D2D2D2Du);
                }
            }
            for (; k < f1; ++k) {
                const uint4 v = *reinterpret_cast<const uint4 *>((a.plane[k] ? a.rows1 : a.rows0) + (size_t)a.ids[k] * (size_t)a.cap + col);
                acc[0] += trim_zero_bytes(v.x ^ 0x2D2D2D2Du); acc[1] += trim_zero_bytes(v.y ^ 0x2D2D2D2Du);
                acc[2] += trim_zero_bytes(v.z ^ 0x2D2D2D2Du); acc[3] += trim_zero_bytes(v.w ^ 0x2D2D2D2Du);
            }
#pragma unroll
            for (int j = 0; j < kTrCols; ++j) cnt[j] += (acc[j >> 2] >> (8 * (j & 3))) & 0xFFu;
        }
    }
#pragma unroll
    for (int j = 0; j < kTrCols; ++j) s_cnt[(int)threadIdx.x * kTrCols + j] = cnt[j];
    __syncthreads();
    for (int i = (int)threadIdx.x; i < kTrColTile; i += kTrThreads) {
        const uint32_t c = s_cnt[i];
        if (c && col0 + i < a.W) atomicAdd(&a.gaps[col0 + i], c);
    }
}

// grid: ceil(W / 256), 256 threads, a thread per column: its keep bit, gathered per wave by a ballot into two 32-column words.
__global__ void __launch_bounds__(kTrThreads) trim_bits_kernel(TrimArgs a)
{
    const int64_t c = (int64_t)blockIdx.x * kTrThreads + threadIdx.x;
    bool keep = false;
    if (c < a.W) {
        if (a.rule == 0) keep = a.gaps[c] <= (uint32_t)a.arg;
        else keep = ((a.plane[a.arg] ? a.rows1 : a.rows0) + (size_t)a.ids[a.arg] * (size_t)a.cap)[c] != '-';
    }
    const unsigned long long b = __ballot(keep);
    const int lane = (int)threadIdx.x & 63;
    const int64_t w = c >> 5;                                                         // (64 divides 256: a wave starts on an even word)
    if (lane == 0 && c < a.W) a.flags[w] = (uint32_t)b;
    if (lane == 32 && c < a.W) a.flags[w] = (uint32_t)(b >> 32);
}

// grid: 1, 256 threads.  The workgroup walks the words a chunk of 256 at a time with a carry (squeeze_scan_kernel's idiom): pre[w] = kept
// columns in front of word w, pre[words] = *kept = the kept total.
__global__ void __launch_bounds__(kTrThreads) trim_scan_kernel(TrimArgs a)
{
    __shared__ int s_tmp[kTrThreads];
    const int32_t words = (a.W + 31) >> 5;
    int carry = 0;
    for (int base = 0; base < words; base += kTrThreads) {
        const int w = base + (int)threadIdx.x;
        const int v = w < words ? __popc(a.flags[w]) : 0;
        int tot;
        const int ex = squeeze_excl_sum(v, s_tmp, &tot);
        if (w < words) a.pre[w] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) { a.pre[words] = carry; *a.kept = carry; }
}

// grid: ceil(W / 256), 256 threads, a thread per column: a kept column writes its index at its destination.
__global__ void __launch_bounds__(kTrThreads) trim_list_kernel(TrimArgs a)
{
    const int64_t c = (int64_t)blockIdx.x * kTrThreads + threadIdx.x;
    if (c >= a.W) return;
    const uint32_t word = a.flags[c >> 5];
    const int b = (int)(c & 31);
    if (word & (1u << b)) a.cols[a.pre[c >> 5] + __popc(word & ((1u << b) - 1u))] = (int32_t)c;
}

// grid: (column tiles, rows y, rows z), 256 threads: one workgroup per (row, column tile), row = z * gridDim.y + y.  As squeeze_compact_kernel:
// a thread reads its 16 columns and puts the kept ones into LDS at their destination index, counted from the 16-byte boundary at or below the
// tile's first destination byte; then the workgroup writes the tile's kept bytes as one contiguous run: 16-byte stores for the chunks the run
// covers whole, single bytes at its two ends.
__global__ void __launch_bounds__(kTrThreads) trim_compact_kernel(TrimArgs a)
{
    __shared__ __attribute__((aligned(16))) char s_out[kTrColTile + 16];
    const int64_t k = (int64_t)blockIdx.z * gridDim.y + blockIdx.y;
    if (k >= a.n) return;
    const int32_t W = a.W;
    const int32_t col0 = (int)blockIdx.x * kTrColTile;
    const int32_t words = (W + 31) >> 5;
    const size_t base = (size_t)a.ids[k] * (size_t)a.cap;
    const char *row = (a.plane[k] ? a.rows1 : a.rows0) + base;
    char *out = (a.plane[k] ? a.out0 : a.out1) + base;
    const int32_t dst0 = a.pre[col0 >> 5];                                            // (a tile starts on a word)
    const int32_t dst1 = a.pre[min(words, (col0 + kTrColTile) >> 5)];
    if (dst1 == dst0) return;                                                         // (uniform: nothing of this tile is kept)
    const int32_t shift = dst0 & 15;
    const int32_t col = col0 + (int)threadIdx.x * kTrCols;
    if (col < W) {
        const uint32_t word = a.flags[col >> 5];
        const uint32_t below = (col & 31) ? (word & 0xFFFFu) : 0u;
        const uint32_t m = (word >> (col & 31)) & 0xFFFFu;                            // (no bit at or behind column W)
        if (m) {
            int at = a.pre[col >> 5] + __popc(below) - dst0 + shift;
            const uint4 v = *reinterpret_cast<const uint4 *>(row + col);
            const uint32_t x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < kTrCols; ++j)
                if (m & (1u << j)) s_out[at++] = (char)((x[j >> 2] >> (8 * (j & 3))) & 0xFFu);
        }
    }
    __syncthreads();
    const int32_t lo = shift, hi = shift + (dst1 - dst0);                             // the run inside s_out
    char *dst = out + (dst0 - shift);                                                 // 16-byte aligned: s_out[i] goes to dst[i]
    for (int c = (int)threadIdx.x * 16; c < hi; c += kTrThreads * 16) {
        if (c >= lo && c + 16 <= hi) *reinterpret_cast<uint4 *>(dst + c) = *reinterpret_cast<const uint4 *>(s_out + c);
        else
            for (int i = max(c, lo); i < min(c + 16, hi); ++i) dst[i] = s_out[i];
    }
}

}  // namespace twl
