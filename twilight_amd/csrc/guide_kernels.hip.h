// twilight_amd/csrc/guide_kernels.hip.h -- kernels of include/twl_guide.h: the k-mer counts of every sequence and the shared k-mer
// count of every pair of sequences (the distances a guide tree is built from).
//
//   guide_count_kernel    one workgroup per sequence, a histogram of 32-bit counters in LDS (LDS atomic adds), written out saturated to 16 bits
//   guide_shared_kernel   one workgroup per 64 x 64 tile of pairs on or above the diagonal, slices of the two count panels staged in LDS
//
// The shared count of a pair is S = sum_b min(x_b, y_b).  With min(x, y) = (x + y - |x - y|) / 2 it is (w_x + w_y - sum_b |x_b - y_b|) / 2,
// and the sum of absolute differences of TWO 16-bit bins added to a 32-bit accumulator is one instruction (v_sad_u16): no partial sum
// is ever held in 16 bits, so none can wrap.  The sum is at most w_x + w_y <= 2 * 7776 * 65535 < 2^32.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace twl {

constexpr int kGuideCountThreads = 256;                                  // threads of a count workgroup
constexpr int kGuideChunk = 16;                                          // windows (k-mer starts) a thread takes in a row: it reads chunk + k - 1 letters
constexpr int kGuideRound = kGuideCountThreads * kGuideChunk;            // windows the workgroup takes per round
constexpr int kGuideTile = 64;                                           // pairs tile: 64 x 64 per workgroup, 4 x 4 per thread
constexpr int kGuideSlice = 128;                                         // bins of both panels staged per step (256 bytes per row); the bins are padded to a multiple
constexpr int kGuidePitch = kGuideSlice * 2 + 16;                        // bytes between rows of a panel in LDS: row r starts at 16-byte slot r mod 16
constexpr int kGuideMaxBins = 7776;

// letter of the alphabet `B` (4: A C G T/U; 6: the Dayhoff classes AGPST C DENQ FWY HKR ILMV), or -1
template <int B> __device__ __forceinline__ int guide_letter(unsigned char c)
{
    const unsigned u = (c & 0xDFu) - 'A';      // upper case; letters land in [0, 26)
    if (((c | 0x20u) - 'a') >= 26u) return -1;
    if (B == 4) return u == 0 ? 0 : u == 2 ? 1 : u == 6 ? 2 : (u == 19 || u == 20) ? 3 : -1;
    //                               A   B   C  D  E  F  G  H  I   J  K  L  M  N   O  P  Q  R  S  T   U  V  W   X  Y   Z
    constexpr int8_t kClass[26] = {0, -1, 1, 2, 2, 3, 0, 4, 5, -1, 4, 5, 5, 2, -1, 0, 2, 4, 0, 0, -1, 5, 3, -1, 3, -1};
    return kClass[u];
}

// counts[s][b] = min(65535, windows of sequence s whose K letters read as the base-B number b), b < BINS = B^K; the padding bins
// [BINS, bins_pad) are zeroed; w[s] = sum_b counts[s][b].  Thread t of round r takes the windows [r * kGuideRound + t * kGuideChunk, + kGuideChunk):
// it rebuilds the rolling code from the chunk's first letter, so neighbouring chunks read K - 1 letters in common.
template <int B, int K, int BINS>
__global__ void __launch_bounds__(kGuideCountThreads) guide_count_kernel(const unsigned char *__restrict__ letters, const unsigned long long *__restrict__ off,
                                                                         const int32_t *__restrict__ len, int bins_pad, uint16_t *__restrict__ counts, uint32_t *__restrict__ w)
{
    __shared__ uint32_t hist[BINS];
    __shared__ uint32_t total;
    const int s = blockIdx.x, tid = threadIdx.x;
    for (int b = tid; b < BINS; b += kGuideCountThreads) hist[b] = 0;
    if (tid == 0) total = 0;
    __syncthreads();
    const unsigned char *seq = letters + off[s];
    const int L = len[s];
    const int windows = L - K + 1;      // (< 1 for a sequence shorter than K)
    constexpr int kTop = BINS / B;      // B^(K-1): the code without its first letter is code % kTop
    for (long long base = 0; base < windows; base += kGuideRound) {      // (64-bit: a length near 2^31 must not wrap the positions)
        const long long p0 = base + tid * kGuideChunk;
        if (p0 >= windows) continue;
        const long long pEnd = min(p0 + kGuideChunk, (long long)windows);      // one past the last window of this chunk
        int code = 0, run = 0;
        for (long long q = p0; q < pEnd + K - 1; ++q) {       // q < windows + K - 1 = L
            const int l = guide_letter<B>(seq[q]);
            if (l < 0) { run = 0; code = 0; continue; }
            code = (code % kTop) * B + l;
            if (++run >= K) atomicAdd(&hist[code], 1u);       // (run >= K implies q >= p0 + K - 1: the window starts inside the chunk)
        }
    }
    __syncthreads();
    uint16_t *row = counts + (size_t)s * (size_t)bins_pad;
    uint32_t mine = 0;
    for (int b = tid; b < bins_pad; b += kGuideCountThreads) {
        const uint32_t c = b < BINS ? min(hist[b], 65535u) : 0u;
        row[b] = (uint16_t)c;
        mine += c;
    }
    atomicAdd(&total, mine);
    __syncthreads();
    if (tid == 0) w[s] = total;
}

// out[i][j] = out[j][i] = sum_b min(counts[i][b], counts[j][b]) for the pairs of tile (blockIdx.y, blockIdx.x), blockIdx.x >= blockIdx.y
// (the workgroups below the diagonal leave at once).  Thread (ty, tx) owns the pairs (i0 + ty + 16 r, j0 + tx + 16 c), r, c < 4: with rows
// 272 bytes apart the 16 rows tx + 16 c that the lanes of a 16-byte read ask for sit in 16 different 16-byte slots of the 256-byte bank
// row, and the two ty of such a lane group in two more: every panel read is conflict-free.  Rows >= n of a partial tile are staged as
// zeros and never written.
__global__ void __launch_bounds__(256) guide_shared_kernel(const uint16_t *__restrict__ counts, const uint32_t *__restrict__ w, int n, int bins_pad, uint32_t *__restrict__ out)
{
    if (blockIdx.x < blockIdx.y) return;
    __shared__ __attribute__((aligned(16))) unsigned char panel[2][kGuideTile * kGuidePitch];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int i0 = blockIdx.y * kGuideTile, j0 = blockIdx.x * kGuideTile;
    uint32_t acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0;
    const size_t pitch = (size_t)bins_pad * sizeof(uint16_t);
    for (int b0 = 0; b0 < bins_pad; b0 += kGuideSlice) {
        // stage: 2 panels x 64 rows x 16 pieces of 16 bytes, 8 pieces per thread; 16 neighbouring threads read one row's 256 bytes
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int e = tid + 256 * (q & 3), side = q >> 2, row = e >> 4, piece = e & 15;
            const int g = (side ? j0 : i0) + row;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (g < n) v = *reinterpret_cast<const uint4 *>(reinterpret_cast<const unsigned char *>(counts) + (size_t)g * pitch + (size_t)b0 * 2 + piece * 16);
            *reinterpret_cast<uint4 *>(&panel[side][row * kGuidePitch + piece * 16]) = v;
        }
        __syncthreads();
#pragma unroll 2
        for (int piece = 0; piece < 16; ++piece) {
            uint4 a[4], b[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) a[r] = *reinterpret_cast<const uint4 *>(&panel[0][(ty + 16 * r) * kGuidePitch + piece * 16]);
#pragma unroll
            for (int c = 0; c < 4; ++c) b[c] = *reinterpret_cast<const uint4 *>(&panel[1][(tx + 16 * c) * kGuidePitch + piece * 16]);
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    uint32_t s = acc[r][c];
                    s = __builtin_amdgcn_sad_u16(a[r].x, b[c].x, s);
                    s = __builtin_amdgcn_sad_u16(a[r].y, b[c].y, s);
                    s = __builtin_amdgcn_sad_u16(a[r].z, b[c].z, s);
                    s = __builtin_amdgcn_sad_u16(a[r].w, b[c].w, s);
                    acc[r][c] = s;
                }
        }
        __syncthreads();
    }
    uint32_t wi[4], wj[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { const int i = i0 + ty + 16 * r; wi[r] = i < n ? w[i] : 0; }
#pragma unroll
    for (int c = 0; c < 4; ++c) { const int j = j0 + tx + 16 * c; wj[c] = j < n ? w[j] : 0; }
    // the tile itself: 16 neighbouring threads write 64 neighbouring bytes of a row
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            acc[r][c] = (wi[r] + wj[c] - acc[r][c]) >> 1;
            const int i = i0 + ty + 16 * r, j = j0 + tx + 16 * c;
            if (i < n && j < n) out[(size_t)i * (size_t)n + (size_t)j] = acc[r][c];
        }
    if (blockIdx.x == blockIdx.y) return;      // a tile on the diagonal is its own mirror (uniform over the workgroup)
    // the mirror, transposed through LDS (the panels are free: the last step ended in a barrier) so that its rows are written the same way
    uint32_t *tile = reinterpret_cast<uint32_t *>(&panel[0][0]);      // [64][65] words = 16 640 bytes <= one panel
    constexpr int kT = kGuideTile + 1;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) tile[(tx + 16 * c) * kT + ty + 16 * r] = acc[r][c];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int jl = ty + 16 * r, il = tx + 16 * c;      // row j0 + jl of the mirror, column i0 + il
            if (j0 + jl < n && i0 + il < n) out[(size_t)(j0 + jl) * (size_t)n + (size_t)(i0 + il)] = tile[jl * kT + il];
        }
}

}  // namespace twl
