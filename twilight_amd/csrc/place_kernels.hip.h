// twilight_amd/csrc/place_kernels.hip.h -- device side of placement without a tree (include/twl_place.h): new sequences aligned, one
// by one, to the profile of an existing alignment, then merged into it.
//
//   count_columns_kernel / counts_to_cache_kernel   readAlignment's column counts of the backbone (reference src/io.cpp:200-238)
//   place_collect_kernel                            the insertion part of mergeInsertions (src/alignment-helper.cpp:593-691): the
//                                                   longest run of query-only codes in front of every backbone column
//   place_scan_kernel                               where every insertion block and every backbone column lands in the final rows
//   place_expand_kernel / backbone_expand_kernel    the final rows of the placed sequences and of the backbone (src/io.cpp:355-449)
//
// Path codes: 0 = both, 1 = query only (an insertion), 2 = reference (backbone) only.  All byte / int streams, HBM-bound.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace twl {

constexpr int kPlThreads = 256;             // every kernel below runs 256-thread workgroups
constexpr int kPlItems = 16;                // path codes per thread and tile
constexpr int kPlTile = kPlThreads * kPlItems;
constexpr int kCountRows = 64;              // backbone rows per workgroup of the column count

// grid: (ceil(L / 256), ceil(n_ids / kCountRows)), 256 threads; thread = one column of a slice of the rows.  Consecutive threads read
// consecutive bytes of one row; the per-letter counts stay in registers (compare-and-add over the P letters: no indexed register array)
// and reach the int32 table with one atomic per non-zero letter.
template <int P>
__global__ void __launch_bounds__(kPlThreads) count_columns_kernel(const char *rows0, const char *rows1, int64_t cap, const uint8_t *plane, const int32_t *ids,
                                                                   int32_t n_ids, int32_t L, const uint8_t *lut, int32_t *counts)
{
    __shared__ uint8_t s_lut[256];
    s_lut[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
    const int c = blockIdx.x * kPlThreads + threadIdx.x;
    if (c >= L) return;
    int cnt[P];
#pragma unroll
    for (int k = 0; k < P; ++k) cnt[k] = 0;
    const int r0 = blockIdx.y * kCountRows, r1 = min(n_ids, r0 + kCountRows);
    for (int r = r0; r < r1; ++r) {
        const int s = ids[r];
        const uint8_t v = s_lut[(uint8_t)(plane[s] ? rows1 : rows0)[(size_t)s * cap + c]];
#pragma unroll
        for (int k = 0; k < P; ++k) cnt[k] += (v == k);
    }
#pragma unroll
    for (int k = 0; k < P; ++k)
        if (cnt[k]) atomicAdd(&counts[(size_t)c * P + k], cnt[k]);
}

// counts -> the float profile of a cached node (exact below 2^24 rows)
__global__ void __launch_bounds__(kPlThreads) counts_to_cache_kernel(const int32_t *counts, int64_t n, float *out)
{
    const int64_t i = (int64_t)blockIdx.x * kPlThreads + threadIdx.x;
    if (i < n) out[i] = (float)counts[i];
}

// Block-wide scans of one int per thread (Hillis-Steele in LDS; `tmp` holds kPlThreads ints): the value over the threads before this one,
// and in *total the value over all of them.  Every thread of the block calls them.
__device__ inline int block_excl_sum(int v, int *tmp, int *total)
{
    const int t = threadIdx.x;
    tmp[t] = v;
    __syncthreads();
    for (int d = 1; d < kPlThreads; d <<= 1) {
        const int add = t >= d ? tmp[t - d] : 0;
        __syncthreads();
        tmp[t] += add;
        __syncthreads();
    }
    const int r = tmp[t] - v;
    *total = tmp[kPlThreads - 1];
    __syncthreads();
    return r;
}
__device__ inline int block_excl_max(int v, int *tmp, int *total)
{
    const int t = threadIdx.x;
    tmp[t] = v;
    __syncthreads();
    for (int d = 1; d < kPlThreads; d <<= 1) {
        const int o = t >= d ? tmp[t - d] : INT32_MIN;
        __syncthreads();
        tmp[t] = max(tmp[t], o);
        __syncthreads();
    }
    const int r = t > 0 ? tmp[t - 1] : INT32_MIN;
    *total = tmp[kPlThreads - 1];
    __syncthreads();
    return r;
}

// Walks the path `path[0, n)` with the whole workgroup, a tile of kPlTile codes at a time (staged through LDS with coalesced loads), and calls
//   f(p, code, c, q, last)
// for every position p: c = backbone columns before p (codes != 1), q = query letters before p (codes != 2), last = position of the last
// code != 1 before p (-1: none), so that a code 1 at p is letter (p - last - 1) of the insertion block in front of column c.
// stage(p, code) sees every code once, as it is staged.  Every thread of the block calls it; *tot_c / *tot_q receive the totals.
template <class Stage, class F>
__device__ void scan_path(const int8_t *path, int32_t n, Stage stage, F f, int *tot_c, int *tot_q)
{
    __shared__ int8_t s_tile[kPlTile];
    __shared__ int s_tmp[kPlThreads];
    int C = 0, Q = 0, M = -1;                  // carried over the tiles
    for (int base = 0; base < n; base += kPlTile) {
        const int m = min(kPlTile, n - base);
        for (int j = threadIdx.x; j < m; j += kPlThreads) {
            const int8_t v = path[base + j];
            s_tile[j] = v;
            stage(base + j, v);
        }
        __syncthreads();
        const int j0 = threadIdx.x * kPlItems, j1 = min(m, j0 + kPlItems);
        int a = 0, b = 0, last = -1;
        for (int j = j0; j < j1; ++j) {
            const int8_t v = s_tile[j];
            if (v != 1) { ++a; last = base + j; }
            if (v != 2) ++b;
        }
        int ta, tb, tl;
        int c = C + block_excl_sum(a, s_tmp, &ta);
        int q = Q + block_excl_sum(b, s_tmp, &tb);
        int lst = max(M, block_excl_max(last, s_tmp, &tl));
        for (int j = j0; j < j1; ++j) {
            const int8_t v = s_tile[j];
            f(base + j, (int)v, c, q, lst);
            if (v != 1) { ++c; lst = base + j; }
            if (v != 2) ++q;
        }
        C += ta; Q += tb; M = max(M, tl);
        __syncthreads();                       // (s_tile is restaged next)
    }
    *tot_c = C;
    *tot_q = Q;
}

// Where the final paths of a call's taking pairs live (twl_place_collect, twl_merge_apply): pair t's path is plen[t] codes at src_off[t] of the
// buffer which[t] names.
struct PathSrc {
    const int8_t *src[3];        // [0] host rows (uploaded), [1] DP output, [2] staged path buffer
    const uint8_t *which;        // [n_pairs] index into src
    const int64_t *src_off;      // [n_pairs]
    const int32_t *plen;         // [n_pairs]
    __device__ const int8_t *path(int t) const { return src[which[t]] + src_off[t]; }
};

// grid: n_pairs, 256 threads.  Pair t's final path (DP output, the staged path buffer or an uploaded host row: PathSrc) is copied
// to its sequence's slot of the placement's arena, and every insertion run folded into longest[c] (atomicMax at the run's last code).  bad[t] = 1 when the path does not cover exactly L backbone columns and len[t] letters (nothing is folded then).
struct CollectArgs {
    PathSrc from;
    const int32_t *qlen;         // [n_pairs] letters of the sequence
    const int64_t *dst_off;      // [n_pairs] offset of the sequence's slot in the arena
    int8_t *arena;
    int32_t *longest;            // [L + 1]
    int32_t *bad;                // [n_pairs]
    int32_t L;
};

__global__ void __launch_bounds__(kPlThreads) place_collect_kernel(CollectArgs a)
{
    __shared__ int s_ok;
    const int t = blockIdx.x;
    const int8_t *path = a.from.path(t);
    const int32_t n = a.from.plen[t];
    int8_t *dst = a.arena + a.dst_off[t];
    int tc, tq;
    // first pass: copy + totals (the folding must not see a path of another shape)
    scan_path(path, n, [&](int p, int8_t v) { dst[p] = v; }, [&](int, int, int, int, int) {}, &tc, &tq);
    if (threadIdx.x == 0) { s_ok = (tc == a.L && tq == a.qlen[t]); a.bad[t] = s_ok ? 0 : 1; }
    __syncthreads();
    if (!s_ok) return;
    scan_path(path, n, [&](int, int8_t) {}, [&](int p, int v, int c, int, int last) {
        if (v == 1 && (p + 1 == n || path[p + 1] != 1) && c <= a.L) atomicMax(&a.longest[c], p - last);
    }, &tc, &tq);
}

// One workgroup: ins[k] = k + longest[0] + ... + longest[k-1] (k = 0..L: where insertion block k starts in the final rows; backbone column k
// follows its block at ins[k] + longest[k]), *W = L + the sum of all longest.
__global__ void __launch_bounds__(kPlThreads) place_scan_kernel(const int32_t *longest, int32_t L, int32_t *ins, int32_t *W)
{
    __shared__ int s_tmp[kPlThreads];
    int carry = 0;
    for (int base = 0; base <= L; base += kPlThreads) {
        const int k = base + (int)threadIdx.x;
        const int v = k <= L ? longest[k] : 0;
        int tot;
        const int ex = block_excl_sum(v, s_tmp, &tot);
        if (k <= L) ins[k] = k + carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) *W = L + carry;
}

// grid: ceil(L / 256): colsrc[ins[i] + longest[i]] = i (the other entries of colsrc[W] are -1: insertion columns)
__global__ void __launch_bounds__(kPlThreads) place_colsrc_kernel(const int32_t *longest, const int32_t *ins, int32_t L, int32_t *colsrc)
{
    const int i = blockIdx.x * kPlThreads + threadIdx.x;
    if (i < L) colsrc[ins[i] + longest[i]] = i;
}

// grid: n_placed, 256 threads.  The final row of placed sequence t: '.' everywhere, then its letters in the backbone columns (code 0), '-' in
// the columns it lacks (code 2) and its insertion letters left-aligned in their blocks (code 1).  Writes stay inside [0, W) whatever the path
// says (collect has checked its shape already).
struct ExpandArgs {
    const char *rows0, *rows1;   // current planes (the sequence itself)
    char *out0, *out1;           // the same planes, written on the other side: out[plane ^ 1]
    int64_t cap;
    const int32_t *ids;          // [n] store ids
    const uint8_t *plane;        // [n] current plane of each
    const int32_t *qlen;         // [n]
    const int64_t *path_off;     // [n] into arena
    const int32_t *plen;         // [n]
    const int8_t *arena;
    const int32_t *longest, *ins, *colsrc;
    int32_t L, W;
};

__global__ void __launch_bounds__(kPlThreads) place_expand_kernel(ExpandArgs a)
{
    const int t = blockIdx.x;
    const int s = a.ids[t];
    const char *row = (a.plane[t] ? a.rows1 : a.rows0) + (size_t)s * a.cap;
    char *out = (a.plane[t] ? a.out0 : a.out1) + (size_t)s * a.cap;
    for (int w = threadIdx.x; w < a.W; w += kPlThreads) out[w] = '.';
    __syncthreads();
    const int32_t ql = a.qlen[t];
    int tc, tq;
    scan_path(a.arena + a.path_off[t], a.plen[t], [&](int, int8_t) {}, [&](int p, int v, int c, int q, int last) {
        if (v == 1) {
            const int r = p - last - 1;
            if (c <= a.L && q < ql && r < a.longest[c]) out[a.ins[c] + r] = row[q];
        } else if (c < a.L) {
            const int w = a.ins[c] + a.longest[c];
            if (v == 0) { if (q < ql) out[w] = row[q]; }
            else out[w] = '-';
        }
    }, &tc, &tq);
}

// grid: (n_backbone, ceil(W / 256)), 256 threads: column w of a backbone row is its column colsrc[w], or '.' in an insertion column
__global__ void __launch_bounds__(kPlThreads) backbone_expand_kernel(ExpandArgs a)
{
    const int t = blockIdx.x;
    const int w = blockIdx.y * kPlThreads + threadIdx.x;
    if (w >= a.W) return;
    const int s = a.ids[t];
    const char *row = (a.plane[t] ? a.rows1 : a.rows0) + (size_t)s * a.cap;
    char *out = (a.plane[t] ? a.out0 : a.out1) + (size_t)s * a.cap;
    const int src = a.colsrc[w];
    out[w] = src >= 0 ? row[src] : '.';
}

}  // namespace twl
