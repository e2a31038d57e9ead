// twilight_amd/csrc/score_kernels.hip.h -- device side of include/twl_score.h: the exact integers of the affine sum-of-pairs score of the
// listed rows of a store.
//
//   score_pack_kernel      one bit-plane `present` (byte != '-') per row, a 64-bit word per 64 columns by __ballot, zero words up to the
//                          staged-slice multiple; first[k] / last[k], the row's first and last letter column
//   score_counts_kernel    cnt[a][c] = listed rows whose byte at column c is of letter class a (exact: integer atomics)
//   score_products_kernel  sub[a][b] += cnt[a][c] * cnt[b][c] (a < b), C(cnt[a][c], 2) (a = b) over a block of columns; let[c], g[c]
//   score_pairs_kernel     runs_row[i] += gap runs of row i against row j, for every ordered pair of a 64 x 64 tile pair
//
// The pair kernel, per pair of rows with present-words A (row i) and B (row j): X = B & ~A are the columns of the pair's projection in which
// i holds '-'.  The A bits cut the columns into segments; a gap run of i against j is a segment that holds an X bit.  In S = X + ~A (one
// number over all words, low word first) every position of a segment holds a 1 of ~A, so the lowest X bit of a segment starts a carry that
// runs through the rest of the segment and stops in the A bit that closes it (there ~A and X are 0): S & A has exactly the closing bits of
// the segments that hold an X bit.  The top segment has no closing bit: its carry leaves the last word.  Pad words have A = 0 and X = 0,
// ~A all ones: the carry passes through them.
//
// Rows are cap-pitched and cap is a multiple of 16 above every row length (the driver refuses another pitch), so the 4 bytes at column
// 4k < W of a row lie inside its pitch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "retree_kernels.hip.h"      // retree_letter

namespace twl {

constexpr int kScThreads = 256;                       // every kernel below runs 256-thread workgroups
constexpr int kScTile = 64;                           // pairs tile: 64 x 64 per workgroup, 4 x 4 per thread
constexpr int kScSlice = 16;                          // words of the plane staged per step (1024 columns)
constexpr int kScCols = 4;                            // columns a counts thread owns: one 4-byte load per row
constexpr int kScColTile = kScThreads * kScCols;      // columns of a counts tile
constexpr int kScRowSlice = 512;                      // rows a counts workgroup sums
constexpr int kScFlush = 252;                         // rows a packed byte counter takes before it is flushed (4 rows per step)
constexpr int kScProdCols = 256;                      // columns of a products workgroup
constexpr int kScMaxClasses = 21;                     // K + 1 for 'p'
static_assert(kScFlush <= 255 && kScFlush % 4 == 0, "a byte counter holds 255; the row loop steps by 4");
static_assert(kScSlice % 2 == 0, "the staged pitch kScSlice + 1 is odd");

// What the kernels share: the W columns of the n listed rows (row k: store id ids[k] on plane plane[k]).
struct SopArgs {
    const char *rows0, *rows1;   // current planes
    char *out0, *out1;           // (fill_row_planes; never written here)
    int64_t cap;
    const int32_t *ids;          // [n]
    const uint8_t *plane;        // [n]
    int32_t n, W, K;             // K letter classes and the class "other"
    int64_t wordsPad;
    unsigned long long *present; // [n][wordsPad]
    int32_t *first, *last;       // [n]
    uint32_t *cnt;               // [K + 1][W], zeroed before the first launch
    uint32_t *let, *gaps;        // [W]
    unsigned long long *sub;     // [(K + 1)(K + 2) / 2], zeroed
    unsigned long long *runsRow; // [n], zeroed
    const uint32_t *tilePairs;   // ti << 16 | tj, ti <= tj
};

// class of a byte: 0 .. K - 1 a letter of the alphabet, K every other byte, 0xFF the gap
__device__ inline uint32_t score_class(int K, unsigned char c)
{
    if (c == '-') return 0xFFu;
    const int code = K == 4 ? retree_letter<3>(c) : retree_letter<6>(c);
    return code < 0 ? (uint32_t)K : (uint32_t)code;
}

// grid: n, 256 threads: a workgroup per row, a wave per word (word = 4 * step + wave), a lane per column.
__global__ void __launch_bounds__(kScThreads) score_pack_kernel(SopArgs a)
{
    __shared__ int32_t s_lo[kScThreads / 64], s_hi[kScThreads / 64];
    const int32_t k = (int32_t)blockIdx.x;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const char *row = (a.plane[k] ? a.rows1 : a.rows0) + (size_t)a.ids[k] * (size_t)a.cap;
    unsigned long long *out = a.present + (size_t)k * (size_t)a.wordsPad;
    int32_t lo = a.W, hi = -1;
    for (int64_t word = wave; word < a.wordsPad; word += kScThreads / 64) {
        const int64_t c = word * 64 + lane;
        const bool letter = c < a.W && row[c] != '-';
        const unsigned long long b = __ballot(letter);
        if (lane == 0) out[word] = b;
        if (b) {      // (uniform over the wave)
            lo = min(lo, (int32_t)(word * 64) + (int32_t)__builtin_ctzll(b));
            hi = max(hi, (int32_t)(word * 64) + 63 - (int32_t)__builtin_clzll(b));
        }
    }
    if (lane == 0) { s_lo[wave] = lo; s_hi[wave] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kScThreads / 64; ++w) { lo = min(lo, s_lo[w]); hi = max(hi, s_hi[w]); }
        a.first[k] = lo; a.last[k] = hi;
    }
}

// grid: (column tiles, row slices), 256 threads.  A thread owns 4 consecutive columns of its slice's rows: per row one 4-byte load, per
// letter byte a 1 added to the column's byte of the class's packed word, in LDS at s_pack[class][thread] (a wave's 64 lanes hit 64 banks
// whatever their classes).  Every kScFlush rows and at the end the packed words go into cnt by one atomic per class, thread and column that
// counted anything; a wave's atomics of one class and column offset lie in 1 KB.
__global__ void __launch_bounds__(kScThreads) score_counts_kernel(SopArgs a)
{
    __shared__ uint32_t s_pack[kScMaxClasses * kScThreads];
    __shared__ uint8_t s_class[256];
    const int tid = (int)threadIdx.x;
    const int classes = a.K + 1;
    s_class[tid] = (uint8_t)score_class(a.K, (unsigned char)tid);
    for (int x = 0; x < classes; ++x) s_pack[x * kScThreads + tid] = 0;
    __syncthreads();
    const int32_t col = (int32_t)blockIdx.x * kScColTile + tid * kScCols;
    if (col >= a.W) return;                                  // (no barrier below)
    const int32_t r0 = (int32_t)blockIdx.y * kScRowSlice;
    const int32_t r1 = min(a.n, r0 + kScRowSlice);
    const int live = min(kScCols, a.W - col);                // columns of this thread in front of W
    for (int32_t f0 = r0; f0 < r1; f0 += kScFlush) {
        const int32_t f1 = min(r1, f0 + kScFlush);
        int32_t k = f0;
        for (; k + 4 <= f1; k += 4) {
            uint32_t v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                v[u] = *reinterpret_cast<const uint32_t *>((a.plane[k + u] ? a.rows1 : a.rows0) + (size_t)a.ids[k + u] * (size_t)a.cap + col);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int j = 0; j < kScCols; ++j) {
                    const uint32_t cl = s_class[(v[u] >> (8 * j)) & 0xFFu];
                    if (cl != 0xFFu && j < live) s_pack[cl * kScThreads + tid] += 1u << (8 * j);
                }
        }
        for (; k < f1; ++k) {
            const uint32_t v = *reinterpret_cast<const uint32_t *>((a.plane[k] ? a.rows1 : a.rows0) + (size_t)a.ids[k] * (size_t)a.cap + col);
#pragma unroll
            for (int j = 0; j < kScCols; ++j) {
                const uint32_t cl = s_class[(v >> (8 * j)) & 0xFFu];
                if (cl != 0xFFu && j < live) s_pack[cl * kScThreads + tid] += 1u << (8 * j);
            }
        }
        for (int x = 0; x < classes; ++x) {
            const uint32_t p = s_pack[x * kScThreads + tid];
            if (!p) continue;
            s_pack[x * kScThreads + tid] = 0;
#pragma unroll
            for (int j = 0; j < kScCols; ++j) {
                const uint32_t c = (p >> (8 * j)) & 0xFFu;
                if (c) atomicAdd(&a.cnt[(size_t)x * (size_t)a.W + (size_t)(col + j)], c);      // (c != 0 only where j < live)
            }
        }
    }
}

// grid: ceil(W / 256), 256 threads.  The block's columns of cnt are staged in LDS at an odd pitch; thread t < (K + 1)(K + 2) / 2 owns the
// pair (a, b) of entry t and walks the columns: the threads of a wave read up to K + 1 different addresses a * pitch + c, in K + 1 different
// banks.  One 64-bit atomic per thread.  Thread t also owns column t: let[c] = the sum of its classes, gaps[c] = n - let[c].
__global__ void __launch_bounds__(kScThreads) score_products_kernel(SopArgs a)
{
    constexpr int kPitch = kScProdCols + 1;
    __shared__ uint32_t s_cnt[kScMaxClasses * kPitch];
    const int tid = (int)threadIdx.x;
    const int classes = a.K + 1;
    const int32_t col0 = (int32_t)blockIdx.x * kScProdCols;
    const int32_t cols = min(kScProdCols, a.W - col0);
    uint32_t letters = 0;
    for (int x = 0; x < classes; ++x) {
        const uint32_t v = tid < cols ? a.cnt[(size_t)x * (size_t)a.W + (size_t)(col0 + tid)] : 0u;
        s_cnt[x * kPitch + tid] = v;
        letters += v;
    }
    if (tid < cols) { a.let[col0 + tid] = letters; a.gaps[col0 + tid] = (uint32_t)a.n - letters; }
    __syncthreads();
    // entry tid of sub: rows x = 0 .. K one after the other, each from y = x
    int x = 0, at = tid;
    while (x < classes && at >= classes - x) { at -= classes - x; ++x; }
    if (x >= classes) return;
    const int y = x + at;
    unsigned long long sum = 0;
    if (x == y)
        for (int c = 0; c < cols; ++c) { const unsigned long long v = s_cnt[x * kPitch + c]; sum += v * (v - (v ? 1 : 0)) / 2; }
    else
        for (int c = 0; c < cols; ++c) sum += (unsigned long long)s_cnt[x * kPitch + c] * (unsigned long long)s_cnt[y * kPitch + c];
    if (sum) atomicAdd(&a.sub[tid], sum);
}

// One word of one ordered pair: `gone` = the word of the row whose runs are counted (A), `other` = the other row's (B); carry in {0, 1} comes
// in from the word below and leaves for the word above.  The carry out of x + m + cin is the top bit of (x & m) | ((x | m) & ~sum); x is a
// subset of m here, so that is x | (m & ~sum): plain integer arithmetic on the top halves, no comparison.
__device__ __forceinline__ uint32_t score_run_word(unsigned long long gone, unsigned long long other, uint32_t &carry)
{
    const unsigned long long m = ~gone, x = other & m;
    const unsigned long long s = x + m + carry;
    carry = (uint32_t)((x | (m & ~s)) >> 63);
    return (uint32_t)__popcll(s & gone);
}

// grid: the tile pairs (ti <= tj), 256 threads.  Thread (ty, tx) owns the pairs (i0 + ty + 16 r, j0 + tx + 16 c), r, c < 4, in both orders:
// ni[r][c] runs of i against j with its carry ci, nj[r][c] runs of j against i with cj.  A staged row is kScSlice + 1 words long, an odd
// number: the 16 rows tx + 16 c that the lanes of a 32-lane group ask an 8-byte read for sit in 16 different 8-byte slots of the 256-byte
// bank row, the two ty of the group in two more.  The words are walked in ascending order over all slices, so the carries hold between
// slices; the tile's whole word loop is this workgroup's.  Rows >= n of a ragged tile are staged as zeros and never written.  On a diagonal
// tile pair the tile holds both orders of every pair: only ni is kept, and i = j is skipped.
__global__ void __launch_bounds__(kScThreads) score_pairs_kernel(SopArgs a)
{
    constexpr int kPitch = kScSlice + 1;
    __shared__ unsigned long long panel[2][kScTile * kPitch];
    __shared__ unsigned long long s_rows[2][kScTile];
    const int tid = (int)threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const uint32_t tp = a.tilePairs[blockIdx.x];
    const int32_t i0 = (int32_t)(tp >> 16) * kScTile, j0 = (int32_t)(tp & 0xFFFFu) * kScTile;
    const bool diag = i0 == j0;
    if (tid < 2 * kScTile) s_rows[tid >> 6][tid & 63] = 0;
    uint32_t ni[4][4], nj[4][4], ci[4][4], cj[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) ni[r][c] = nj[r][c] = ci[r][c] = cj[r][c] = 0;
    for (int64_t w0 = 0; w0 < a.wordsPad; w0 += kScSlice) {
        for (int e = tid; e < 2 * kScTile * kScSlice; e += kScThreads) {
            const int side = e / (kScTile * kScSlice), rem = e - side * (kScTile * kScSlice), row = rem / kScSlice, u = rem - row * kScSlice;
            const int32_t g = (side ? j0 : i0) + row;
            unsigned long long v = 0;
            if (g < a.n) v = a.present[(size_t)g * (size_t)a.wordsPad + (size_t)w0 + (size_t)u];
            panel[side][row * kPitch + u] = v;
        }
        __syncthreads();
#pragma unroll 1
        for (int w = 0; w < kScSlice; ++w) {
            unsigned long long A[4], B[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) A[r] = panel[0][(ty + 16 * r) * kPitch + w];
#pragma unroll
            for (int c = 0; c < 4; ++c) B[c] = panel[1][(tx + 16 * c) * kPitch + w];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    ni[r][c] += score_run_word(A[r], B[c], ci[r][c]);
                    nj[r][c] += score_run_word(B[c], A[r], cj[r][c]);
                }
        }
        __syncthreads();
    }
    // the carry out of the last word is the top segment; then per row of the tile, over the thread's 4 and the 16 threads of its line
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        unsigned long long sum = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (!(diag && ty + 16 * r == tx + 16 * c)) sum += (unsigned long long)ni[r][c] + ci[r][c];
        if (sum) atomicAdd(&s_rows[0][ty + 16 * r], sum);
    }
    if (!diag) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            unsigned long long sum = 0;
#pragma unroll
            for (int r = 0; r < 4; ++r) sum += (unsigned long long)nj[r][c] + cj[r][c];
            if (sum) atomicAdd(&s_rows[1][tx + 16 * c], sum);
        }
    }
    __syncthreads();
    if (tid < 2 * kScTile) {
        const int side = tid >> 6, l = tid & 63;
        const int32_t g = (side ? j0 : i0) + l;
        const unsigned long long v = s_rows[side][l];
        if (g < a.n && v && !(side && diag)) atomicAdd(&a.runsRow[g], v);
    }
}

}  // namespace twl
