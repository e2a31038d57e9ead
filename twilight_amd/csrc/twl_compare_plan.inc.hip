// twilight_amd/csrc/twl_compare_plan.inc.hip -- what twl_compare_create (include/twl_compare.h) decides on the host, as PURE functions of the call's
// arguments: everything the call rejects before it looks at a row, the pitches, the byte counts and every offset into its buffers (64-bit:
// n x We passes 2^31 on the shapes this is built for).  No HIP call and no global in this file: tests/compare_plan_kats.cpp includes it
// directly.  Included by twl_compare.inc.hip (one translation unit).
#pragma once
#include <cstdint>

constexpr int32_t kCompareMaxRows = 1 << 20;

// The widest row the kernels address: the row scans step through a row a round at a time, so the bound is the int32 arithmetic of a round's
// last column, base + scanChunk (as twl_trim_plan.inc.hip's trim_max_width).
inline int32_t compare_max_width(int32_t scanChunk) { return INT32_MAX - scanChunk; }

// The buffers of a compare object.  Pitches are in elements (bytes of a row, ints of its keys), the width rounded up to the column tile.
struct ComparePlan {
    int32_t n = 0, we = 0, wr = 0;
    int64_t pe = 0, pr = 0;               // pitches of E and of R
    int64_t colTiles = 0;                 // grid of the column kernel
    uint64_t estBytes = 0, refBytes = 0;  // the two alignments
    uint64_t keyBytes = 0, posBytes = 0;  // keys [n][pe] int32 (stay), pos [n][pr] int32 (freed when the keys stand)
    uint64_t smallBytes = 0;              // nR [wr], letters of the R rows [n], the results [we] x (8 + 4 + 4 + 1), the bad-row word
    uint64_t createBytes = 0;             // the most that is allocated at one time: all of the above
};

inline int64_t compare_pitch(int32_t w, int32_t colTile) { return ((int64_t)w + colTile - 1) / colTile * colTile; }
// element offsets of row k, of (k, c)
inline int64_t compare_row_at(int64_t pitch, int32_t k) { return pitch * (int64_t)k; }
inline int64_t compare_cell_at(int64_t pitch, int32_t k, int32_t c) { return pitch * (int64_t)k + (int64_t)c; }

// Everything twl_compare_create rejects from its arguments alone: the message, or nullptr with `p` filled in.
inline const char *plan_compare(int32_t n, int32_t w_est, bool haveEst, int32_t w_ref, bool haveRef, bool haveCmp, bool haveBad, int32_t colTile, int32_t scanChunk, ComparePlan &p)
{
    p = ComparePlan{};
    if (!haveEst || !haveRef || !haveCmp || !haveBad) return "bad argument";
    if (n < 2) return "a comparison needs at least 2 rows";
    if (n > kCompareMaxRows) return "too many rows for twl_compare_create (at most 2^20)";
    if (w_est < 0 || w_ref < 0) return "negative width";
    if (w_est > compare_max_width(scanChunk) || w_ref > compare_max_width(scanChunk)) return "rows too long for twl_compare_create";
    p.n = n; p.we = w_est; p.wr = w_ref;
    p.pe = compare_pitch(w_est, colTile); p.pr = compare_pitch(w_ref, colTile);
    p.colTiles = p.pe / colTile;
    p.estBytes = (uint64_t)p.pe * (uint64_t)n; p.refBytes = (uint64_t)p.pr * (uint64_t)n;
    p.keyBytes = p.estBytes * 4u; p.posBytes = p.refBytes * 4u;
    p.smallBytes = (uint64_t)w_ref * 4u + (uint64_t)n * 4u + (uint64_t)w_est * 17u + 16u;
    p.createBytes = p.estBytes + p.refBytes + p.keyBytes + p.posBytes + p.smallBytes;
    return nullptr;
}

// Rows of one upload slab: as many whole rows as fit stageBytes, at least one.
inline int32_t compare_stage_rows(int32_t n, int64_t pitch, int64_t stageBytes)
{
    if (pitch <= 0) return n;
    const int64_t per = stageBytes / pitch;
    return (int32_t)(per < 1 ? 1 : per > n ? n : per);
}
