// twilight_amd/csrc/retree_stage_kernels.hip.h -- kernels of the two-stage rebuilt guide tree (include/twl_retree_set.h),
// over the bit-planes that retree_pack_kernel (retree_kernels.hip.h) left in HBM:
//
//   retree_letters_kernel   one wave per row: letters[i] = both(i, i), the bits of the row's `valid` plane
//   retree_assign_kernel    one workgroup per 64-row tile of rows; it walks all tiles of 64 seeds (their rows gathered through seed_ids) and
//                           keeps, per row, the seed with the largest match / both (in LDS: the tile body of 6 planes leaves no register):
//                           only that seed and its two counts are written
//   retree_groups_kernel    one workgroup per entry of a tile list: a 64 x 64 tile on or above the diagonal of the two matrices of one group of rows
//
// The last two run the 64 x 64 x kRetreeSlice-word tile body of retree_pair_kernel.  The body is written out a second time here
// (retree_tile_counts), with gathered rows, and retree_pair_kernel is left as it was: its registers are what section 4h measured.
//
// Nothing here checks an index: seed_ids, ids and the tile list have passed twl_retree_set_plan.inc.hip on the host.
#pragma once
#include "retree_kernels.hip.h"

namespace twl {

// One entry of the tile list of retree_groups_kernel (made by plan_guide_groups, twl_guide_set_plan.inc.hip): the tile (ti, tj), ti <= tj, of
// the group whose rows are ids[first .. first + m) and whose m x m blocks start at match[block] and both[block].
struct RetreeGroupTile {
    int32_t first, m, ti, tj;
    unsigned long long block;
};

// letters[i] = popcount of plane 0 of row i, i < n; the waves of the grid stride over the rows.
template <int P>
__global__ void __launch_bounds__(kRetreeThreads) retree_letters_kernel(const unsigned long long *__restrict__ planes, int n, long long words_pad, uint32_t *__restrict__ letters)
{
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * (kRetreeThreads / 64);
    for (long long i = (long long)blockIdx.x * (kRetreeThreads / 64) + (threadIdx.x >> 6); i < n; i += waves) {
        const unsigned long long *row = planes + (size_t)i * P * (size_t)words_pad;
        uint32_t mine = 0;
        for (long long w = lane; w < words_pad; w += 64) mine += (uint32_t)__popcll(row[w]);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d, 64);
        if (lane == 0) letters[i] = mine;
    }
}

// nb[r][c] = both and nm[r][c] = match of the rows ga'(ty + 16 r) and gb'(tx + 16 c) over all words: ga[k] / gb[k] is the row of `planes` behind
// local row ty + 16 k of side A / B, or -1 for a row of zeros (its `valid` is 0: it counts nothing).  The 16 threads of a local row bring the
// same four indices a side; they meet in `rowid`, and from there on the staging is retree_pair_kernel's loop with a gathered row: neighbouring
// threads read the neighbouring words of one plane, and no index is held in a register through the tile body.  The staged row is
// P * kRetreeSlice + 1 words long, as in retree_pair_kernel: every panel read is conflict-free.  Ends in a barrier: the panels and rowid are
// free afterwards.
template <int P>
__device__ __forceinline__ void retree_tile_counts(const unsigned long long *__restrict__ planes, long long words_pad, unsigned long long (*panel)[kRetreeTile * (P * kRetreeSlice + 1)],
                                                   int (*rowid)[kRetreeTile], const int (&ga)[4], const int (&gb)[4], uint32_t (&nb)[4][4], uint32_t (&nm)[4][4])
{
    constexpr int kRow = P * kRetreeSlice, kPitch = kRow + 1;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    if (tx == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) { rowid[0][ty + 16 * k] = ga[k]; rowid[1][ty + 16 * k] = gb[k]; }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) nb[r][c] = nm[r][c] = 0;
    for (long long w0 = 0; w0 < words_pad; w0 += kRetreeSlice) {
        // stage: 2 sides x 64 rows x P planes x kRetreeSlice words
        for (int e = tid; e < 2 * kRetreeTile * kRow; e += kRetreeThreads) {
            const int side = e / (kRetreeTile * kRow), rem = e - side * (kRetreeTile * kRow), row = rem / kRow, u = rem - row * kRow;
            const int g = rowid[side][row];
            unsigned long long v = 0;
            if (g >= 0) v = planes[((size_t)g * P + (size_t)(u / kRetreeSlice)) * (size_t)words_pad + (size_t)w0 + (size_t)(u % kRetreeSlice)];
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
}

// A candidate seed of a row: the counts match and both of the row with the seed, and the seed's index t.  Its ratio is match / both, taken as
// 0 / 1 where both counts are 0.  Two candidates are not counts: the row's own seed is {1, 0, t} (a ratio above every other), a column behind
// the last seed is {0, 1, INT32_MAX} (which every seed is before).  before(a, b): a is the better one -- the larger ratio, compared exactly by
// cross-multiplying (the counts are below 2^31, so the products fit 64 bits), then the smaller t.  A total order: no two candidates of a row
// share t.
struct RetreeCand { uint32_t match, both; int32_t t; };
__device__ __forceinline__ unsigned long long retree_denominator(const RetreeCand &x) { return (x.match | x.both) == 0 ? 1ull : (unsigned long long)x.both; }
__device__ __forceinline__ bool retree_before(const RetreeCand &a, const RetreeCand &b)
{
    const unsigned long long l = (unsigned long long)a.match * retree_denominator(b), r = (unsigned long long)b.match * retree_denominator(a);
    return l > r || (l == r && a.t < b.t);
}

// seed_out[i] = the t < n_seeds that row i goes to, match_out[i] / both_out[i] = its counts with row seed_ids[t] (either may be null), i < n:
//   i == seed_ids[t]: that t, and letters[i] for both counts;
//   otherwise the t with the largest match(i, seed_ids[t]) / both(i, seed_ids[t]), 0 / 1 where both is 0; the smaller t among equals.
template <int P>
__global__ void __launch_bounds__(kRetreeThreads) retree_assign_kernel(const unsigned long long *__restrict__ planes, const uint32_t *__restrict__ letters, int n, long long words_pad,
                                                                       const int32_t *__restrict__ seed_ids, int n_seeds, int32_t *__restrict__ seed_out,
                                                                       uint32_t *__restrict__ match_out, uint32_t *__restrict__ both_out)
{
    constexpr int kPitch = P * kRetreeSlice + 1;
    __shared__ unsigned long long panel[2][kRetreeTile * kPitch];
    __shared__ int rowid[2][kRetreeTile];
    __shared__ RetreeCand best[kRetreeTile];      // the best seed so far of every row of the tile; only the row's lane 0 reads and writes it: no barrier
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const long long i0 = (long long)blockIdx.x * kRetreeTile;
    int ga[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long i = i0 + ty + 16 * r;
        ga[r] = i < n ? (int)i : -1;
        if (tx == 0) best[ty + 16 * r] = RetreeCand{0u, 1u, INT32_MAX};
    }
    for (int t0 = 0; t0 < n_seeds; t0 += kRetreeTile) {
        int gb[4];      // the seed rows this thread stages (local rows ty + 16 k)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ts = t0 + ty + 16 * k;
            gb[k] = ts < n_seeds ? seed_ids[ts] : -1;
        }
        uint32_t nb[4][4], nm[4][4];
        retree_tile_counts<P>(planes, words_pad, panel, rowid, ga, gb, nb, nm);
        int gc[4];      // the seed rows of its columns (tx + 16 c); read behind the tile body, where registers are scarce
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int tc = t0 + tx + 16 * k;
            gc[k] = tc < n_seeds ? seed_ids[tc] : -1;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            RetreeCand mine = RetreeCand{0u, 1u, INT32_MAX};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (gc[c] < 0) continue;
                RetreeCand x{nm[r][c], nb[r][c], t0 + tx + 16 * c};
                if (gc[c] == ga[r]) { x.match = 1; x.both = 0; }
                if (retree_before(x, mine)) mine = x;
            }
            // the 16 lanes of a row: a butterfly, so that every lane ends with the row's best
#pragma unroll
            for (int d = 8; d >= 1; d >>= 1) {
                RetreeCand o;
                o.match = __shfl_xor(mine.match, d, 16); o.both = __shfl_xor(mine.both, d, 16); o.t = __shfl_xor(mine.t, d, 16);
                if (retree_before(o, mine)) mine = o;
            }
            if (tx == 0 && retree_before(mine, best[ty + 16 * r])) best[ty + 16 * r] = mine;
        }
    }
    if (tx != 0) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (ga[r] < 0) continue;
        const RetreeCand b = best[ty + 16 * r];
        const bool own = b.match == 1 && b.both == 0;      // (counts never have match above both)
        seed_out[ga[r]] = b.t;
        if (match_out) match_out[ga[r]] = own ? letters[ga[r]] : b.match;
        if (both_out) both_out[ga[r]] = own ? letters[ga[r]] : b.both;
    }
}

// Tile tiles[blockIdx.x] of its group's blocks: match[block + a * m + b] = match[block + b * m + a] = match(ids[first + a], ids[first + b]) for
// the pairs (a, b) of the tile, a, b < m, and the same for both.  The diagonal needs no step of its own: both(i, i) = match(i, i) = letters[i]
// is what the tile body counts for a row against itself.  Rows >= m of a partial tile are staged as zeros and never written.
template <int P>
__global__ void __launch_bounds__(kRetreeThreads) retree_groups_kernel(const unsigned long long *__restrict__ planes, long long words_pad, const RetreeGroupTile *__restrict__ tiles,
                                                                       const int32_t *__restrict__ ids, uint32_t *__restrict__ match, uint32_t *__restrict__ both)
{
    constexpr int kPitch = P * kRetreeSlice + 1;
    static_assert(2 * kRetreeTile * kPitch * 8 >= kRetreeTile * (kRetreeTile + 1) * 4, "the mirror tile is transposed in the panels");
    __shared__ unsigned long long panel[2][kRetreeTile * kPitch];
    __shared__ int rowid[2][kRetreeTile];
    const RetreeGroupTile t = tiles[blockIdx.x];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int a0 = t.ti * kRetreeTile, b0 = t.tj * kRetreeTile;
    int ga[4], gb[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int a = a0 + ty + 16 * k, b = b0 + ty + 16 * k;
        ga[k] = a < t.m ? ids[t.first + a] : -1;
        gb[k] = b < t.m ? ids[t.first + b] : -1;
    }
    uint32_t nb[4][4], nm[4][4];
    retree_tile_counts<P>(planes, words_pad, panel, rowid, ga, gb, nb, nm);
    uint32_t *mblk = match + t.block, *bblk = both + t.block;
    const size_t m = (size_t)t.m;
    // the tile itself: 16 neighbouring threads write 64 neighbouring bytes of a row
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int a = a0 + ty + 16 * r, b = b0 + tx + 16 * c;
            if (a < t.m && b < t.m) {
                mblk[(size_t)a * m + (size_t)b] = nm[r][c];
                bblk[(size_t)a * m + (size_t)b] = nb[r][c];
            }
        }
    if (t.ti == t.tj) return;      // a tile on the diagonal is its own mirror (uniform over the workgroup)
    // the mirrors, transposed through LDS (the panels are free: the tile body ended in a barrier) so that their rows are written the same way
    uint32_t *tile = reinterpret_cast<uint32_t *>(&panel[0][0]);      // [64][65] words
    constexpr int kT = kRetreeTile + 1;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        uint32_t *out = s ? bblk : mblk;
        if (s) __syncthreads();      // (the first mirror has been read)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) tile[(tx + 16 * c) * kT + ty + 16 * r] = s ? nb[r][c] : nm[r][c];
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int bl = ty + 16 * r, al = tx + 16 * c;      // row b0 + bl of the mirror, column a0 + al
                if (b0 + bl < t.m && a0 + al < t.m) out[(size_t)(b0 + bl) * m + (size_t)(a0 + al)] = tile[bl * kT + al];
            }
    }
}

}  // namespace twl
