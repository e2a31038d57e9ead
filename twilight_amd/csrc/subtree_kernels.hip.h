// twilight_amd/csrc/subtree_kernels.hip.h -- device side of include/twl_subtree.h: the profile of a finished subtree, every row weighted by its
// sequence weight (SequenceDB::storeSubtreeProfile, reference src/sequencedb.cpp:122-138).
//
//   weighted_columns_kernel   out[c][letter of row t in column c] += weights[t], t = 0 .. n_ids - 1 IN THAT ORDER, in fp32
//
// The order is the contract (the reference adds sequence by sequence and the profile has to be the same bits), so a column's rows are never
// split: one thread owns one column, walks all rows in the order of the id list and keeps the column's P sums in registers.  Each
// (column, letter) sum is then one chain of fp32 additions; no atomics, no partial sums.  A byte stream, HBM-bound once the rows are many.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace twl {

constexpr int kWcThreads = 256;             // columns per workgroup: one thread each
constexpr int kWcRows = 256;                // rows whose address and weight are staged in LDS per round

// grid: ceil(L / 256), 256 threads; thread = one column of ALL rows.  Consecutive threads read consecutive bytes of one row.  A round stages
// where kWcRows rows begin (their plane and pitch resolved) and their weights in LDS, so that the loop over the rows has no dependent load in
// front of the row's byte and the loads of several rows are in flight while the additions run in order.  A letter that does not match adds
// nothing (a select, not an addition of zero).
template <int P>
__global__ void __launch_bounds__(kWcThreads) weighted_columns_kernel(const char *rows0, const char *rows1, int64_t cap, const uint8_t *plane, const int32_t *ids,
                                                                      const float *weights, int32_t n_ids, int32_t L, const uint8_t *lut, float *out)
{
    __shared__ uint8_t s_lut[256];
    __shared__ const char *s_row[kWcRows];
    __shared__ float s_w[kWcRows];
    s_lut[threadIdx.x] = lut[threadIdx.x];
    const int c = blockIdx.x * kWcThreads + threadIdx.x;
    const bool live = c < L;
    float acc[P];
#pragma unroll
    for (int k = 0; k < P; ++k) acc[k] = 0.0f;
    for (int r0 = 0; r0 < n_ids; r0 += kWcRows) {
        const int n = min(kWcRows, n_ids - r0);
        __syncthreads();                    // (the table; the previous round's rows have been read)
        if ((int)threadIdx.x < n) {
            const int s = ids[r0 + threadIdx.x];
            s_row[threadIdx.x] = (plane[s] ? rows1 : rows0) + (size_t)s * cap;
            s_w[threadIdx.x] = weights[r0 + threadIdx.x];
        }
        __syncthreads();
        if (live) {
#pragma unroll 8
            for (int r = 0; r < n; ++r) {
                const uint8_t v = s_lut[(uint8_t)s_row[r][c]];
                const float w = s_w[r];
#pragma unroll
                for (int k = 0; k < P; ++k) acc[k] = (v == k) ? acc[k] + w : acc[k];
            }
        }
    }
    if (live) {
#pragma unroll
        for (int k = 0; k < P; ++k) out[(size_t)c * P + k] = acc[k];
    }
}

}  // namespace twl
