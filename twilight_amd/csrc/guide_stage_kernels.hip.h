// twilight_amd/csrc/guide_stage_kernels.hip.h -- kernels of the two-stage guide tree (include/twl_guide.h, twl_guide_set_*),
// over the count panels that guide_count_kernel (guide_kernels.hip.h) left in HBM:
//
//   guide_assign_kernel   one workgroup per 64-row tile of sequences; it walks all tiles of 64 seeds (their rows gathered through seed_ids) and
//                         keeps, per row, the seed with the largest S / min(w, w_seed): only that seed and its S are written
//   guide_groups_kernel   one workgroup per entry of a tile list: a 64 x 64 tile on or above the diagonal of the S-matrix of one group of rows
//
// Both run the 64 x 64 x 128-bin v_sad_u16 tile body of guide_shared_kernel.  The body is written out a second time here (guide_tile_sad)
// and guide_shared_kernel is left as it was: its registers and scratch are what section 4f measured.
#pragma once
#include "guide_kernels.hip.h"

namespace twl {

// One entry of the tile list of guide_groups_kernel (made by plan_guide_groups, twl_guide_set_plan.inc.hip): the tile (ti, tj), ti <= tj, of
// the group whose rows are ids[first .. first + m) and whose m x m block starts at out[block].
struct GuideGroupTile {
    int32_t first, m, ti, tj;
    unsigned long long block;
};

// acc[r][c] = sum over all bins of |counts[ga'(ty + 16 r)][b] - counts[gb'(tx + 16 c)][b]|, where this thread stages the local rows ty + 16 k
// of both sides: ga[k] / gb[k] is the row of `counts` behind local row ty + 16 k of side A / B, or -1 for a row of zeros.  Ends in a barrier:
// the panels are free afterwards.
__device__ __forceinline__ void guide_tile_sad(const uint16_t *__restrict__ counts, int bins_pad, unsigned char (*panel)[kGuideTile * kGuidePitch], const int (&ga)[4],
                                               const int (&gb)[4], uint32_t (&acc)[4][4])
{
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0;
    const size_t pitch = (size_t)bins_pad * sizeof(uint16_t);
    for (int b0 = 0; b0 < bins_pad; b0 += kGuideSlice) {
        // stage: 2 panels x 64 rows x 16 pieces of 16 bytes, 8 pieces per thread; 16 neighbouring threads read one row's 256 bytes
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int side = q >> 2, row = ty + 16 * (q & 3), piece = tx;
            const int g = side ? gb[q & 3] : ga[q & 3];
            uint4 v = make_uint4(0, 0, 0, 0);
            if (g >= 0) v = *reinterpret_cast<const uint4 *>(reinterpret_cast<const unsigned char *>(counts) + (size_t)g * pitch + (size_t)b0 * 2 + piece * 16);
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
}

// A candidate seed of a row: the ratio s / m and the seed's index t.  before(a, b): a is the better one -- the larger ratio, compared exactly
// by cross-multiplying (s, m < 2^29, so the products fit 64 bits), then the smaller t.  A total order: no two candidates of a row share t.
struct GuideCand { uint32_t s, m; int32_t t; };
__device__ __forceinline__ bool guide_before(const GuideCand &a, const GuideCand &b)
{
    const unsigned long long l = (unsigned long long)a.s * b.m, r = (unsigned long long)b.s * a.m;
    return l > r || (l == r && a.t < b.t);
}

// seed_out[i] = the t < n_seeds that sequence i goes to, shared_out[i] = S(i, seed_ids[t]) (shared_out may be null), i < n:
//   i == seed_ids[t]: that t (the candidate 1 / 0, which is before every other one);
//   otherwise the t with the largest S(i, seed_ids[t]) / min(w_i, w_seed), 0 / 1 where that minimum is 0; the smaller t among equals.
// A column behind the last seed is the candidate 0 / 1 with t = INT32_MAX, which every seed is before.
__global__ void __launch_bounds__(256) guide_assign_kernel(const uint16_t *__restrict__ counts, const uint32_t *__restrict__ w, int n, int bins_pad, const int32_t *__restrict__ seed_ids,
                                                           int n_seeds, int32_t *__restrict__ seed_out, uint32_t *__restrict__ shared_out)
{
    __shared__ __attribute__((aligned(16))) unsigned char panel[2][kGuideTile * kGuidePitch];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const long long i0 = (long long)blockIdx.x * kGuideTile;
    int ga[4];
    uint32_t wi[4];
    GuideCand best[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long i = i0 + ty + 16 * r;
        ga[r] = i < n ? (int)i : -1;
        wi[r] = i < n ? w[i] : 0;
        best[r] = GuideCand{0u, 1u, INT32_MAX};
    }
    for (int t0 = 0; t0 < n_seeds; t0 += kGuideTile) {
        int gb[4], gc[4];      // the seed rows this thread stages (local rows ty + 16 k) and the seed rows of its columns (tx + 16 c)
        uint32_t wj[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ts = t0 + ty + 16 * k, tc = t0 + tx + 16 * k;
            gb[k] = ts < n_seeds ? seed_ids[ts] : -1;
            gc[k] = tc < n_seeds ? seed_ids[tc] : -1;
            wj[k] = gc[k] >= 0 ? w[gc[k]] : 0;
        }
        uint32_t acc[4][4];
        guide_tile_sad(counts, bins_pad, panel, ga, gb, acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            GuideCand mine = GuideCand{0u, 1u, INT32_MAX};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (gc[c] < 0) continue;
                const uint32_t m = min(wi[r], wj[c]);
                GuideCand x{(wi[r] + wj[c] - acc[r][c]) >> 1, m, t0 + tx + 16 * c};
                if (m == 0) { x.s = 0; x.m = 1; }
                if (gc[c] == ga[r]) { x.s = 1; x.m = 0; }
                if (guide_before(x, mine)) mine = x;
            }
            // the 16 lanes of a row: a butterfly, so that every lane ends with the row's best
#pragma unroll
            for (int d = 8; d >= 1; d >>= 1) {
                GuideCand o;
                o.s = __shfl_xor(mine.s, d, 16); o.m = __shfl_xor(mine.m, d, 16); o.t = __shfl_xor(mine.t, d, 16);
                if (guide_before(o, mine)) mine = o;
            }
            if (guide_before(mine, best[r])) best[r] = mine;
        }
    }
    if (tx != 0) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (ga[r] < 0) continue;
        seed_out[ga[r]] = best[r].t;
        if (shared_out) shared_out[ga[r]] = best[r].m == 0 ? wi[r] : best[r].s;      // (its own seed: S(i, i) = w_i)
    }
}

// Tile tiles[blockIdx.x] of its group's block: out[block + a * m + b] = out[block + b * m + a] = S(ids[first + a], ids[first + b]) for the
// pairs (a, b) of the tile, a, b < m; w on the diagonal.  Rows >= m of a partial tile are staged as zeros and never written.
__global__ void __launch_bounds__(256) guide_groups_kernel(const uint16_t *__restrict__ counts, const uint32_t *__restrict__ w, int bins_pad, const GuideGroupTile *__restrict__ tiles,
                                                           const int32_t *__restrict__ ids, uint32_t *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) unsigned char panel[2][kGuideTile * kGuidePitch];
    const GuideGroupTile t = tiles[blockIdx.x];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int a0 = t.ti * kGuideTile, b0 = t.tj * kGuideTile;
    int ga[4], gb[4];
    uint32_t wi[4], wj[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int a = a0 + ty + 16 * k, bs = b0 + ty + 16 * k, bc = b0 + tx + 16 * k;
        ga[k] = a < t.m ? ids[t.first + a] : -1;
        gb[k] = bs < t.m ? ids[t.first + bs] : -1;
        wi[k] = ga[k] >= 0 ? w[ga[k]] : 0;
        wj[k] = bc < t.m ? w[ids[t.first + bc]] : 0;
    }
    uint32_t acc[4][4];
    guide_tile_sad(counts, bins_pad, panel, ga, gb, acc);
    uint32_t *blk = out + t.block;
    const size_t m = (size_t)t.m;
    // the tile itself: 16 neighbouring threads write 64 neighbouring bytes of a row
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            acc[r][c] = (wi[r] + wj[c] - acc[r][c]) >> 1;
            const int a = a0 + ty + 16 * r, b = b0 + tx + 16 * c;
            if (a < t.m && b < t.m) blk[(size_t)a * m + (size_t)b] = acc[r][c];
        }
    if (t.ti == t.tj) return;      // a tile on the diagonal is its own mirror (uniform over the workgroup)
    // the mirror, transposed through LDS (the panels are free: the tile body ended in a barrier) so that its rows are written the same way
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
            const int bl = ty + 16 * r, al = tx + 16 * c;      // row b0 + bl of the mirror, column a0 + al
            if (b0 + bl < t.m && a0 + al < t.m) blk[(size_t)(b0 + bl) * m + (size_t)(a0 + al)] = tile[bl * kT + al];
        }
}

}  // namespace twl
