// twilight_amd/csrc/twl_trim_plan.inc.hip -- what twl_store_trim_columns (include/twl_trim.h) decides on the host, as PURE functions of the call's
// arguments and of the store's bookkeeping: everything the call rejects, and the grids its kernels run on.  No HIP call and no global in this
// file: tests/trim_plan_kats.cpp includes it directly.  Included by twl_trim.inc.hip (one translation unit).
#pragma once
#include <cstdint>
#include <vector>

// The widest row the kernels address: column tiles lie on blockIdx.x (2^31 - 1 of them, more than an int32 width can fill), so the bound is
// the int32 arithmetic of a tile's last column, col0 + colTile, and not the grid.
inline int32_t trim_max_width(int32_t colTile) { return INT32_MAX - colTile; }

// The listed rows of a call as its kernels address them.
struct TrimRows {
    int32_t W = 0;           // the one current length of the listed rows
    int32_t refIndex = -1;   // TWL_TRIM_TO_ROW: the index in ids of the reference row
};

// Everything twl_store_trim_columns rejects: the message, or nullptr with `t` filled in.  row_len[q]: current row length of sequence q.
inline const char *check_trim_columns(bool haveStore, int32_t n_ids, const int32_t *ids, bool haveKeptOut, int32_t rule, int32_t arg, int32_t n_seqs, const int32_t *row_len,
                                      bool levelPrepared, int32_t colTile, TrimRows &t)
{
    t = TrimRows{};
    if (!haveStore || !ids || !haveKeptOut) return "bad argument";
    if (n_ids < 1) return "no rows listed";
    if (levelPrepared) return "a level is still prepared on the store: commit it first";
    if (rule != 0 && rule != 1) return "unknown trim rule";
    std::vector<uint8_t> seen((size_t)n_seqs, 0);
    int32_t W = -1;
    for (int32_t k = 0; k < n_ids; ++k) {
        const int32_t id = ids[k];
        if (id < 0 || id >= n_seqs) return "sequence id out of range";
        if (seen[id]) return "a sequence id is listed twice";
        seen[id] = 1;
        if (W < 0) W = row_len[id];
        else if (row_len[id] != W) return "the listed rows differ in length";
        if (rule == 1 && id == arg) t.refIndex = k;
    }
    if (rule == 0 && (arg < 0 || arg > n_ids)) return "the gap limit lies outside 0 .. n_ids";
    if (rule == 1 && t.refIndex < 0) return "the reference sequence is not among the listed rows";
    if (W > trim_max_width(colTile)) return "rows too long for twl_store_trim_columns";
    t.W = W;
    return nullptr;
}

// The grids of a call.  Counts: (column tiles, row slices).  Keep bits and the kept-column list: a thread per column.  Compaction: (column
// tiles, rows y, rows z), row = z * rowsY + y; a grid dimension beyond x holds 65535 at most.  W == 0 launches only the scan.
struct TrimGrid {
    int32_t words = 0;        // 32-column words of the keep bits
    int32_t colTiles = 0, rowSlices = 0, colBlocks = 0, rowsY = 0, rowsZ = 0;
};
inline const char *plan_trim_grid(int32_t W, int32_t n_ids, int32_t colTile, int32_t rowSlice, int32_t threads, TrimGrid &g)
{
    g = TrimGrid{};
    g.words = (int32_t)(((int64_t)W + 31) / 32);
    g.colTiles = (int32_t)(((int64_t)W + colTile - 1) / colTile);
    g.rowSlices = (int32_t)(((int64_t)n_ids + rowSlice - 1) / rowSlice);
    g.colBlocks = (int32_t)(((int64_t)W + threads - 1) / threads);
    g.rowsY = n_ids < 65535 ? n_ids : 65535;
    g.rowsZ = (int32_t)(((int64_t)n_ids + g.rowsY - 1) / g.rowsY);
    if (g.rowSlices > 65535) return "too many rows for twl_store_trim_columns";
    return nullptr;
}
