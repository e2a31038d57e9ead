// twilight_amd/csrc/backbone_kernels.hip.h -- device side of include/twl_backbone.h: the all-gap columns taken out of every group of
// backbone rows (reference src/sequencedb.cpp:171-210, a host loop there), all groups of a call in three launches.
//
//   squeeze_flags_kernel     one keep bit per column of a group: set when some row of the group holds anything but '-' there
//   squeeze_scan_kernel      the bits counted into destination indices, one int per 32-column word, and the kept count of the group
//   squeeze_compact_kernel   every row's kept bytes, in order, into its other plane
//
// Rows are cap-pitched and cap is a multiple of 16 (the driver refuses another pitch), so column 16k of any row is a 16-byte address.
// All byte / int streams, HBM-bound: the rows are read twice and written once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace twl {

constexpr int kSqThreads = 256;                       // every kernel below runs 256-thread workgroups
constexpr int kSqCols = 16;                           // columns a thread owns: one 16-byte load per row
constexpr int kSqColTile = kSqThreads * kSqCols;      // columns of a tile (flags and compaction)
constexpr int kSqRowSlice = 32;                       // rows whose "not '-'" a flags workgroup ORs in registers
constexpr int kSqScanChunk = kSqThreads * 32;         // columns the scan walks per round: one 32-column word per thread

// One entry of the tile list of squeeze_flags_kernel (made by plan_squeeze_tiles, twl_backbone_plan.inc.hip): columns [col0, col0 + kSqColTile)
// of the rows ids[row0, row1) of group `group`.
struct SqueezeTile { int32_t group, col0, row0, row1; };

// What the three kernels share.  Per group g: its one row length len[g], its keep bits at flags + flag_off[g] (ceil(len / 32) words, zeroed
// before the first launch) and its scan at pre + pre_off[g] (one int per word and one behind them: kept columns in front of the word, at the
// end the kept count).  Per listed row k: its store id, the plane that holds it, its group.
struct SqueezeArgs {
    const char *rows0, *rows1;   // current planes
    char *out0, *out1;           // the same planes, written on the other side: out[plane ^ 1]
    int64_t cap;
    const int32_t *ids;          // [n_rows]
    const uint8_t *plane;        // [n_rows]
    const int32_t *row_group;    // [n_rows]
    const int32_t *len;          // [n_groups]
    const int64_t *flag_off;     // [n_groups]
    const int64_t *pre_off;      // [n_groups]
    uint32_t *flags;
    int32_t *pre;
    int32_t *len_out;            // [n_groups]
    const SqueezeTile *tiles;
};

// 16 bits, bit j set when byte j of the 16 bytes in x differs from zero
__device__ inline uint32_t squeeze_nonzero_bytes(const uint32_t x[4])
{
    uint32_t m = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
        for (int b = 0; b < 4; ++b) m |= ((x[w] >> (8 * b)) & 0xFFu) ? (1u << (4 * w + b)) : 0u;
    return m;
}

// grid: the tile list, 256 threads.  A thread owns 16 consecutive columns of the tile's row slice: it XORs every row's 16 bytes with '-'
// and ORs the result over the rows (a byte stays zero only where every row holds '-'), then adds its 16 bits to the group's word with one
// atomic OR, none when all 16 columns are '-' in the whole slice.  The last columns of a row whose length is no multiple of 16 are read
// byte by byte.
__global__ void __launch_bounds__(kSqThreads) squeeze_flags_kernel(SqueezeArgs a)
{
    const SqueezeTile t = a.tiles[blockIdx.x];
    const int32_t L = a.len[t.group];
    const int32_t col = t.col0 + (int)threadIdx.x * kSqCols;
    if (col >= L) return;
    const bool whole = col + kSqCols <= L;
    uint32_t acc[4] = {0, 0, 0, 0}, tail = 0;
    for (int k = t.row0; k < t.row1; ++k) {
        const char *row = (a.plane[k] ? a.rows1 : a.rows0) + (size_t)a.ids[k] * (size_t)a.cap + col;
        if (whole) {
            const uint4 v = *reinterpret_cast<const uint4 *>(row);
            acc[0] |= v.x ^ 0x2D2D2D2Du; acc[1] |= v.y ^ 0x2D2D2D2Du; acc[2] |= v.z ^ 0x2D2D2D2Du; acc[3] |= v.w ^ 0x2D2D2D2Du;
        } else {
            for (int j = 0; j < L - col; ++j) tail |= (row[j] != '-' ? 1u : 0u) << j;
        }
    }
    const uint32_t m = whole ? squeeze_nonzero_bytes(acc) : tail;
    if (m) atomicOr(&a.flags[a.flag_off[t.group] + (col >> 5)], m << (col & 31));
}

// Block-wide exclusive sum of one int per thread (Hillis-Steele in LDS, `tmp` holds kSqThreads ints); *total: the sum over the block.
__device__ inline int squeeze_excl_sum(int v, int *tmp, int *total)
{
    const int t = threadIdx.x;
    tmp[t] = v;
    __syncthreads();
    for (int d = 1; d < kSqThreads; d <<= 1) {
        const int add = t >= d ? tmp[t - d] : 0;
        __syncthreads();
        tmp[t] += add;
        __syncthreads();
    }
    const int r = tmp[t] - v;
    *total = tmp[kSqThreads - 1];
    __syncthreads();
    return r;
}

// grid: n_groups, 256 threads.  The workgroup walks its group's words a chunk of 256 at a time with a carry (the idiom of
// place_scan_kernel): pre[w] = kept columns in front of word w, pre[words] = len_out[g] = the kept count.
__global__ void __launch_bounds__(kSqThreads) squeeze_scan_kernel(SqueezeArgs a)
{
    __shared__ int s_tmp[kSqThreads];
    const int g = blockIdx.x;
    const int32_t words = (a.len[g] + 31) >> 5;
    const uint32_t *flags = a.flags + a.flag_off[g];
    int32_t *pre = a.pre + a.pre_off[g];
    int carry = 0;
    for (int base = 0; base < words; base += kSqThreads) {
        const int w = base + (int)threadIdx.x;
        const int v = w < words ? __popc(flags[w]) : 0;
        int tot;
        const int ex = squeeze_excl_sum(v, s_tmp, &tot);
        if (w < words) pre[w] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) { pre[words] = carry; a.len_out[g] = carry; }
}

// grid: (n_rows, column tiles of the longest group), 256 threads: one workgroup per (row, column tile); a tile behind the row's length
// ends at once.  A thread reads its 16 columns and puts the kept ones into LDS at their destination index, counted from the 16-byte
// boundary at or below the tile's first destination byte, so that LDS offsets and destination addresses are aligned alike; then the
// workgroup writes the tile's kept bytes as one contiguous run from dst[tile start]: 16-byte stores for the chunks the run covers whole,
// single bytes at its two ends.
__global__ void __launch_bounds__(kSqThreads) squeeze_compact_kernel(SqueezeArgs a)
{
    __shared__ __attribute__((aligned(16))) char s_out[kSqColTile + 16];
    const int k = blockIdx.x;
    const int g = a.row_group[k];
    const int32_t L = a.len[g];
    const int32_t col0 = (int)blockIdx.y * kSqColTile;
    if (col0 >= L) return;
    const int32_t words = (L + 31) >> 5;
    const uint32_t *flags = a.flags + a.flag_off[g];
    const int32_t *pre = a.pre + a.pre_off[g];
    const size_t base = (size_t)a.ids[k] * (size_t)a.cap;
    const char *row = (a.plane[k] ? a.rows1 : a.rows0) + base;
    char *out = (a.plane[k] ? a.out0 : a.out1) + base;
    const int32_t dst0 = pre[col0 >> 5];                                             // (a tile starts on a word)
    const int32_t dst1 = pre[min(words, (col0 + kSqColTile) >> 5)];
    const int32_t shift = dst0 & 15;
    const int32_t col = col0 + (int)threadIdx.x * kSqCols;
    if (col < L) {
        const uint32_t word = flags[col >> 5];
        const uint32_t below = (col & 31) ? (word & 0xFFFFu) : 0u;
        const uint32_t m = (word >> (col & 31)) & 0xFFFFu;
        int at = pre[col >> 5] + __popc(below) - dst0 + shift;
        if (col + kSqCols <= L) {
            const uint4 v = *reinterpret_cast<const uint4 *>(row + col);
            const uint32_t x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < kSqCols; ++j)
                if (m & (1u << j)) s_out[at++] = (char)((x[j >> 2] >> (8 * (j & 3))) & 0xFFu);
        } else {
            for (int j = 0; j < L - col; ++j)
                if (m & (1u << j)) s_out[at++] = row[col + j];
        }
    }
    __syncthreads();
    const int32_t lo = shift, hi = shift + (dst1 - dst0);                            // the run inside s_out
    char *dst = out + (dst0 - shift);                                                // 16-byte aligned: s_out[i] goes to dst[i]
    for (int c = (int)threadIdx.x * 16; c < hi; c += kSqThreads * 16) {
        if (c >= lo && c + 16 <= hi) *reinterpret_cast<uint4 *>(dst + c) = *reinterpret_cast<const uint4 *>(s_out + c);
        else
            for (int i = max(c, lo); i < min(c + 16, hi); ++i) dst[i] = s_out[i];
    }
}

}  // namespace twl
