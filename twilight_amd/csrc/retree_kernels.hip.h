// twilight_amd/csrc/retree_kernels.hip.h -- kernels of include/twl_retree.h: from the rows of a finished alignment, the number of columns in
// which two rows both hold a letter and the number in which the letters are equal, for every pair of rows (the distances the guide tree is
// rebuilt from).
//
//   retree_gap_kernel    one thread per column, the rows cut into slices of kRetreeGapRows over the workgroups; partial counts of '-' meet in
//                        one 32-bit atomic add per thread
//   retree_pack_kernel   one wave per 64 columns of a row: __ballot turns the 64 bytes into one 64-bit word per bit-plane -- `valid` (a letter,
//                        in a column the mask keeps) and the bits of the letter's code (2 for 'n', 5 for 'p'); the code bits of a column that is
//                        not valid are zero.  The mask ends here: the pair kernel sees planes only
//   retree_pair_kernel   one workgroup per 64 x 64 tile of pairs on or above the diagonal, slices of the planes of its 64 + 64 rows staged in LDS;
//                        per word  v = valid_i & valid_j,  both += popc(v),  match += popc(v & ~OR_k(code_k,i ^ code_k,j))  into 32-bit accumulators
//
// Planes in device memory: planes[row][plane][words_pad] 64-bit words, column c of a row is bit c % 64 of word c / 64; words_pad is a multiple
// of kRetreeSlice, the words behind the width are zero.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace twl {

constexpr int kRetreeWordCols = 64;                                      // columns per packed word: one wave's ballot
constexpr int kRetreeTile = 64;                                          // pairs tile: 64 x 64 per workgroup, 4 x 4 per thread
constexpr int kRetreeSlice = 8;                                          // words of every plane staged per step (512 columns)
constexpr int kRetreeGapRows = 64;                                       // rows a workgroup of the gap kernel counts
constexpr int kRetreeThreads = 256;

// code of a letter for a row of P planes (3: A C G T/U as 0 .. 3; 6: ACDEFGHIKLMNPQRSTVWY as 0 .. 19), either case, or -1
template <int P> __device__ __forceinline__ int retree_letter(unsigned char c)
{
    const unsigned u = (c & 0xDFu) - 'A';      // upper case; letters land in [0, 26)
    if (((c | 0x20u) - 'a') >= 26u) return -1;
    if (P == 3) return u == 0 ? 0 : u == 2 ? 1 : u == 6 ? 2 : (u == 19 || u == 20) ? 3 : -1;
    //                              A   B  C  D  E  F  G  H  I   J  K  L   M   N   O   P   Q   R   S   T   U   V   W   X   Y   Z
    constexpr int8_t kCode[26] = {0, -1, 1, 2, 3, 4, 5, 6, 7, -1, 8, 9, 10, 11, -1, 12, 13, 14, 15, 16, -1, 17, 18, -1, 19, -1};
    return kCode[u];
}

// gaps[c] += the rows of slice blockIdx.y whose byte at column c is '-'; gaps is zero when the launch starts.  Consecutive threads read
// consecutive bytes of one row.
__global__ void __launch_bounds__(kRetreeThreads) retree_gap_kernel(const unsigned char *__restrict__ rows, int n, int width, uint32_t *__restrict__ gaps)
{
    const long long c = (long long)blockIdx.x * kRetreeThreads + threadIdx.x;
    if (c >= width) return;
    const int r0 = blockIdx.y * kRetreeGapRows, r1 = min(n, r0 + kRetreeGapRows);
    uint32_t mine = 0;
    for (int r = r0; r < r1; ++r) mine += rows[(size_t)r * (size_t)width + (size_t)c] == '-' ? 1u : 0u;
    if (mine) atomicAdd(&gaps[c], mine);
}

// planes[row][p][word] for row = blockIdx.y and the four words blockIdx.x * 4 + wave: every lane takes one column, the whole wave votes.
template <int P>
__global__ void __launch_bounds__(kRetreeThreads) retree_pack_kernel(const unsigned char *__restrict__ rows, const uint32_t *__restrict__ gaps, int width, uint32_t max_gaps,
                                                                     long long words_pad, unsigned long long *__restrict__ planes)
{
    const int row = blockIdx.y, lane = threadIdx.x & 63;
    const long long word = (long long)blockIdx.x * (kRetreeThreads / 64) + (threadIdx.x >> 6);
    if (word >= words_pad) return;      // (uniform over the wave)
    const long long c = word * kRetreeWordCols + lane;
    int code = -1;
    if (c < width && gaps[c] <= max_gaps) code = retree_letter<P>(rows[(size_t)row * (size_t)width + (size_t)c]);
    unsigned long long w[P];
    w[0] = __ballot(code >= 0);
#pragma unroll
    for (int k = 1; k < P; ++k) w[k] = __ballot(code >= 0 && ((code >> (k - 1)) & 1));
    if (lane == 0) {
        unsigned long long *out = planes + (size_t)row * P * (size_t)words_pad + (size_t)word;
#pragma unroll
        for (int k = 0; k < P; ++k) out[(size_t)k * (size_t)words_pad] = w[k];
    }
}

// both[i][j] = both[j][i] and match[i][j] = match[j][i] for the pairs of tile (blockIdx.y, blockIdx.x), blockIdx.x >= blockIdx.y (the
// workgroups below the diagonal leave at once).  Thread (ty, tx) owns the pairs (i0 + ty + 16 r, j0 + tx + 16 c), r, c < 4.  A staged row is
// P * kRetreeSlice + 1 words long, an odd number: the 16 rows tx + 16 c that the lanes of a 32-lane group ask an 8-byte read for sit in 16
// different 8-byte slots of the 256-byte bank row, the two ty of the group in two more: every panel read is conflict-free.  Rows >= n of a
// partial tile are staged as zeros (their `valid` is 0: they count nothing) and never written.
template <int P>
__global__ void __launch_bounds__(kRetreeThreads) retree_pair_kernel(const unsigned long long *__restrict__ planes, int n, long long words_pad, uint32_t *__restrict__ match,
                                                                     uint32_t *__restrict__ both)
{
    if (blockIdx.x < blockIdx.y) return;
    constexpr int kRow = P * kRetreeSlice, kPitch = kRow + 1;
    static_assert(2 * kRetreeTile * kPitch * 8 >= kRetreeTile * (kRetreeTile + 1) * 4, "the mirror tile is transposed in the panels");
    __shared__ unsigned long long panel[2][kRetreeTile * kPitch];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int i0 = blockIdx.y * kRetreeTile, j0 = blockIdx.x * kRetreeTile;
    uint32_t nb[4][4], nm[4][4];      // both, match
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) nb[r][c] = nm[r][c] = 0;
    for (long long w0 = 0; w0 < words_pad; w0 += kRetreeSlice) {
        // stage: 2 sides x 64 rows x P planes x kRetreeSlice words; neighbouring threads read the neighbouring words of one plane
        for (int e = tid; e < 2 * kRetreeTile * kRow; e += kRetreeThreads) {
            const int side = e / (kRetreeTile * kRow), rem = e - side * (kRetreeTile * kRow), row = rem / kRow, u = rem - row * kRow;
            const int g = (side ? j0 : i0) + row;
            unsigned long long v = 0;
            if (g < n) v = planes[((size_t)g * P + (size_t)(u / kRetreeSlice)) * (size_t)words_pad + (size_t)w0 + (size_t)(u % kRetreeSlice)];
            panel[side][row * kPitch + u] = v;
        }
        __syncthreads();
#pragma unroll 2
        for (int w = 0; w < kRetreeSlice; ++w) {
            unsigned long long a[4][P], b[4][P];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int k = 0; k < P; ++k) a[r][k] = panel[0][(ty + 16 * r) * kPitch + k * kRetreeSlice + w];
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int k = 0; k < P; ++k) b[c][k] = panel[1][(tx + 16 * c) * kPitch + k * kRetreeSlice + w];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const unsigned long long v = a[r][0] & b[c][0];
                    unsigned long long differ = 0;
#pragma unroll
                    for (int k = 1; k < P; ++k) differ |= a[r][k] ^ b[c][k];
                    nb[r][c] += (uint32_t)__popcll(v);
                    nm[r][c] += (uint32_t)__popcll(v & ~differ);
                }
        }
        __syncthreads();
    }
    // the tile itself: 16 neighbouring threads write 64 neighbouring bytes of a row
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int i = i0 + ty + 16 * r, j = j0 + tx + 16 * c;
            if (i < n && j < n) {
                match[(size_t)i * (size_t)n + (size_t)j] = nm[r][c];
                both[(size_t)i * (size_t)n + (size_t)j] = nb[r][c];
            }
        }
    if (blockIdx.x == blockIdx.y) return;      // a tile on the diagonal is its own mirror (uniform over the workgroup)
    // the mirrors, transposed through LDS (the panels are free: the last step ended in a barrier) so that their rows are written the same way
    uint32_t *tile = reinterpret_cast<uint32_t *>(&panel[0][0]);      // [64][65] words
    constexpr int kT = kRetreeTile + 1;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        uint32_t *out = m ? both : match;
        if (m) __syncthreads();      // (the first mirror has been read)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) tile[(tx + 16 * c) * kT + ty + 16 * r] = m ? nb[r][c] : nm[r][c];
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int jl = ty + 16 * r, il = tx + 16 * c;      // row j0 + jl of the mirror, column i0 + il
                if (j0 + jl < n && i0 + il < n) out[(size_t)(j0 + jl) * (size_t)n + (size_t)(i0 + il)] = tile[jl * kT + il];
            }
    }
}

}  // namespace twl
