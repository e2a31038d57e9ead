// twilight_amd/csrc/strand_kernels.hip.h -- kernels of include/twl_strand.h: on which strand every sequence of a twl_guide_set lies
// (`--adjust-direction`), over the count panels that guide_count_kernel (guide_kernels.hip.h) left in HBM.
//
// The 6-mer counts of a reverse complement are a permutation of the forward counts: c_rc(i)[b] = c_i[rc(b)], rc(b) = the code b with its
// base-4 digits reversed and every digit d replaced by 3 - d.  So the opposite-strand count O(i, j) = sum_b min(c_i[b], c_j[rc(b)]) is the
// shared count of row i with a permuted copy of row j, and the device never sees a reversed text.
//
//   strand_permute_kernel    one workgroup per listed row: out[t][b] = counts[ids[t]][rc(b)]
//   strand_assign_kernel     one workgroup per 64-row tile of sequences; it walks all tiles of 64 seeds and scores both strands of every seed
//                            from ONE staged A panel; per row only the best (seed, direction) and its count are written
//   strand_opposite_kernel   one workgroup per 64 x 64 tile on or above the diagonal of the O-matrix of one list of rows
//
// The tile body is the 64 x 64 x 128-bin v_sad_u16 body of guide_tile_sad (guide_stage_kernels.hip.h) with a second B panel and a second
// accumulator set; the guide kernels themselves are left as they are.
#pragma once
#include "guide_stage_kernels.hip.h"

namespace twl {

constexpr int kStrandBins = 4096;      // 4^6: nucleotides only

// rc(b) of a 12-bit code: complement every digit (3 - d = ~d in two bits), reverse the order of the six 2-bit digits
__device__ __forceinline__ uint32_t strand_rc_bin(uint32_t b)
{
    const uint32_t x = __brev(~b & 0xFFFu) >> 20;      // the 12 bits in reverse order: the digits are reversed, and so are the two bits of each
    return ((x & 0xAAAu) >> 1) | ((x & 0x555u) << 1);
}

// out[t][b] = counts[ids[t]][rc(b)], b < 4096; the padding bins [4096, bins_pad) of the row are zeroed.  blockIdx.x = t.
__global__ void __launch_bounds__(256) strand_permute_kernel(const uint16_t *__restrict__ counts, int bins_pad, const int32_t *__restrict__ ids, uint16_t *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) uint16_t row[kStrandBins];
    const int tid = threadIdx.x;
    const uint4 *src = reinterpret_cast<const uint4 *>(counts + (size_t)ids[blockIdx.x] * (size_t)bins_pad);
    for (int p = tid; p < kStrandBins / 8; p += 256) reinterpret_cast<uint4 *>(row)[p] = src[p];
    __syncthreads();
    uint4 *dst = reinterpret_cast<uint4 *>(out + (size_t)blockIdx.x * (size_t)bins_pad);
    for (int p = tid; p < bins_pad / 8; p += 256) {
        uint32_t v[4] = {0, 0, 0, 0};
        if (p < kStrandBins / 8) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t b = (uint32_t)p * 8 + 2 * k;
                v[k] = (uint32_t)row[strand_rc_bin(b)] | ((uint32_t)row[strand_rc_bin(b + 1)] << 16);
            }
        }
        dst[p] = make_uint4(v[0], v[1], v[2], v[3]);
    }
}

// accR[r][c] = sum over all bins of |counts[ga'(ty + 16 r)][b] - perm[gp'(tx + 16 c)][b]|, and with kBoth accF[r][c] the same against
// counts[gb'(tx + 16 c)][b].  This thread stages the local rows ty + 16 k of every side: ga[k] / gb[k] is the row of `counts`, gp[k] the row
// of `perm`, or -1 for a row of zeros.  Panels: 0 = A, 1 = the permuted B, 2 = the forward B (kBoth only).  Ends in a barrier.
template <bool kBoth>
__device__ __forceinline__ void strand_tile_sad(const uint16_t *__restrict__ counts, const uint16_t *__restrict__ perm, int bins_pad,
                                                unsigned char (*panel)[kGuideTile * kGuidePitch], const int (&ga)[4], const int (&gb)[4], const int (&gp)[4],
                                                uint32_t (&accF)[4][4], uint32_t (&accR)[4][4])
{
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) { accF[r][c] = 0; accR[r][c] = 0; }
    const size_t pitch = (size_t)bins_pad * sizeof(uint16_t);
    constexpr int kSides = kBoth ? 3 : 2;
    for (int b0 = 0; b0 < bins_pad; b0 += kGuideSlice) {
        // stage: kSides panels x 64 rows x 16 pieces of 16 bytes, 4 pieces per thread and panel; 16 neighbouring threads read one row's 256 bytes
#pragma unroll
        for (int q = 0; q < 4 * kSides; ++q) {
            const int side = q >> 2, row = ty + 16 * (q & 3), piece = tx;
            const int g = side == 0 ? ga[q & 3] : side == 1 ? gp[q & 3] : gb[q & 3];
            const unsigned char *base = reinterpret_cast<const unsigned char *>(side == 1 ? perm : counts);
            uint4 v = make_uint4(0, 0, 0, 0);
            if (g >= 0) v = *reinterpret_cast<const uint4 *>(base + (size_t)g * pitch + (size_t)b0 * 2 + piece * 16);
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
                    uint32_t s = accR[r][c];
                    s = __builtin_amdgcn_sad_u16(a[r].x, b[c].x, s);
                    s = __builtin_amdgcn_sad_u16(a[r].y, b[c].y, s);
                    s = __builtin_amdgcn_sad_u16(a[r].z, b[c].z, s);
                    s = __builtin_amdgcn_sad_u16(a[r].w, b[c].w, s);
                    accR[r][c] = s;
                }
            if (kBoth) {
#pragma unroll
                for (int c = 0; c < 4; ++c) b[c] = *reinterpret_cast<const uint4 *>(&panel[kSides - 1][(tx + 16 * c) * kGuidePitch + piece * 16]);
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        uint32_t s = accF[r][c];
                        s = __builtin_amdgcn_sad_u16(a[r].x, b[c].x, s);
                        s = __builtin_amdgcn_sad_u16(a[r].y, b[c].y, s);
                        s = __builtin_amdgcn_sad_u16(a[r].z, b[c].z, s);
                        s = __builtin_amdgcn_sad_u16(a[r].w, b[c].w, s);
                        accF[r][c] = s;
                    }
            }
        }
        __syncthreads();
    }
}

// A candidate (seed, strand) of a row: the ratio s / m, the seed's index t and the row's final direction d = r XOR flip[t].  before(a, b): a is the
// better one -- the larger ratio, compared exactly by cross-multiplying (s, m < 2^29), then the smaller t, then the smaller d.  A total order
// over the real candidates of a row: the two strands of one seed differ in d.
struct StrandCand { uint32_t s, m; int32_t t, d; };
__device__ __forceinline__ bool strand_before(const StrandCand &a, const StrandCand &b)
{
    const unsigned long long l = (unsigned long long)a.s * b.m, r = (unsigned long long)b.s * a.m;
    if (l != r) return l > r;
    if (a.t != b.t) return a.t < b.t;
    return a.d < b.d;
}

// For every sequence i < n: seed_out[i] = t, dir_out[i] = d, shared_out[i] = s (shared_out may be null) of the first candidate (t, r), t < n_seeds,
// r in {0, 1}, in the order of strand_before, where s = r ? O(i, seed t) : S(i, seed t), m = min(w_i, w_seed), 0 / 1 where m == 0, and
// d = r XOR flip[t].  i == seed_ids[t]: that t with d = flip[t] and s = w_i (the candidate 1 / 0, before every other one).  perm[t] is the
// permuted row of seed t (strand_permute_kernel over seed_ids).  A column behind the last seed is the candidate 0 / 1 with t = INT32_MAX.
__global__ void __launch_bounds__(256) strand_assign_kernel(const uint16_t *__restrict__ counts, const uint32_t *__restrict__ w, int n, int bins_pad, const int32_t *__restrict__ seed_ids,
                                                            const unsigned char *__restrict__ flip, const uint16_t *__restrict__ perm, int n_seeds,
                                                            int32_t *__restrict__ seed_out, unsigned char *__restrict__ dir_out, uint32_t *__restrict__ shared_out)
{
    __shared__ __attribute__((aligned(16))) unsigned char panel[3][kGuideTile * kGuidePitch];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const long long i0 = (long long)blockIdx.x * kGuideTile;
    int ga[4];
    uint32_t wi[4];
    StrandCand best[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long i = i0 + ty + 16 * r;
        ga[r] = i < n ? (int)i : -1;
        wi[r] = i < n ? w[i] : 0;
        best[r] = StrandCand{0u, 1u, INT32_MAX, 0};
    }
    for (int t0 = 0; t0 < n_seeds; t0 += kGuideTile) {
        int gb[4], gp[4], gc[4], fl[4];      // the seed rows this thread stages (local rows ty + 16 k), and the seed rows and flips of its columns (tx + 16 c)
        uint32_t wj[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ts = t0 + ty + 16 * k, tc = t0 + tx + 16 * k;
            gb[k] = ts < n_seeds ? seed_ids[ts] : -1;
            gp[k] = ts < n_seeds ? ts : -1;
            gc[k] = tc < n_seeds ? seed_ids[tc] : -1;
            fl[k] = tc < n_seeds ? (int)flip[tc] : 0;
            wj[k] = gc[k] >= 0 ? w[gc[k]] : 0;
        }
        uint32_t accF[4][4], accR[4][4];
        strand_tile_sad<true>(counts, perm, bins_pad, panel, ga, gb, gp, accF, accR);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            StrandCand mine = StrandCand{0u, 1u, INT32_MAX, 0};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (gc[c] < 0) continue;
                const uint32_t m = min(wi[r], wj[c]);
                const int32_t t = t0 + tx + 16 * c;
                StrandCand f{(wi[r] + wj[c] - accF[r][c]) >> 1, m, t, fl[c]}, o{(wi[r] + wj[c] - accR[r][c]) >> 1, m, t, fl[c] ^ 1};
                if (m == 0) { f.s = 0; f.m = 1; o.s = 0; o.m = 1; }
                if (gc[c] == ga[r]) { f.s = 1; f.m = 0; o.s = 0; o.m = 1; }
                if (strand_before(f, mine)) mine = f;
                if (strand_before(o, mine)) mine = o;
            }
            // the 16 lanes of a row: a butterfly, so that every lane ends with the row's best
#pragma unroll
            for (int d = 8; d >= 1; d >>= 1) {
                StrandCand x;
                x.s = __shfl_xor(mine.s, d, 16); x.m = __shfl_xor(mine.m, d, 16); x.t = __shfl_xor(mine.t, d, 16); x.d = __shfl_xor(mine.d, d, 16);
                if (strand_before(x, mine)) mine = x;
            }
            if (strand_before(mine, best[r])) best[r] = mine;
        }
    }
    if (tx != 0) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (ga[r] < 0) continue;
        seed_out[ga[r]] = best[r].t;
        dir_out[ga[r]] = (unsigned char)best[r].d;
        if (shared_out) shared_out[ga[r]] = best[r].m == 0 ? wi[r] : best[r].s;      // (its own seed: S(i, i) = w_i)
    }
}

// Tile (blockIdx.y, blockIdx.x), blockIdx.x >= blockIdx.y, of the m x m matrix out[a][b] = out[b][a] = O(ids[a], ids[b]); the workgroups below
// the diagonal leave at once.  perm[b] is the permuted row of ids[b].  O is symmetric (rc is an involution), the diagonal is O(i, i), not w.
// Rows >= m of a partial tile are staged as zeros and never written.
__global__ void __launch_bounds__(256) strand_opposite_kernel(const uint16_t *__restrict__ counts, const uint32_t *__restrict__ w, int bins_pad, const int32_t *__restrict__ ids,
                                                              const uint16_t *__restrict__ perm, int m, uint32_t *__restrict__ out)
{
    if (blockIdx.x < blockIdx.y) return;
    __shared__ __attribute__((aligned(16))) unsigned char panel[2][kGuideTile * kGuidePitch];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int a0 = blockIdx.y * kGuideTile, b0 = blockIdx.x * kGuideTile;
    int ga[4], gp[4];
    const int none[4] = {-1, -1, -1, -1};
    uint32_t wi[4], wj[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int a = a0 + ty + 16 * k, bs = b0 + ty + 16 * k, bc = b0 + tx + 16 * k;
        ga[k] = a < m ? ids[a] : -1;
        gp[k] = bs < m ? bs : -1;
        wi[k] = ga[k] >= 0 ? w[ga[k]] : 0;
        wj[k] = bc < m ? w[ids[bc]] : 0;
    }
    uint32_t unused[4][4], acc[4][4];
    strand_tile_sad<false>(counts, perm, bins_pad, panel, ga, none, gp, unused, acc);
    const size_t mm = (size_t)m;
    // the tile itself: 16 neighbouring threads write 64 neighbouring bytes of a row
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            acc[r][c] = (wi[r] + wj[c] - acc[r][c]) >> 1;
            const int a = a0 + ty + 16 * r, b = b0 + tx + 16 * c;
            if (a < m && b < m) out[(size_t)a * mm + (size_t)b] = acc[r][c];
        }
    if (blockIdx.x == blockIdx.y) return;      // a tile on the diagonal is its own mirror (uniform over the workgroup)
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
            if (b0 + bl < m && a0 + al < m) out[(size_t)(b0 + bl) * mm + (size_t)(a0 + al)] = tile[bl * kT + al];
        }
}

}  // namespace twl
