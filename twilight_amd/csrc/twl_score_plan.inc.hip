// twilight_amd/csrc/twl_score_plan.inc.hip -- what twl_store_score_rows (include/twl_score.h) decides on the host, as PURE functions of the call's
// arguments and of the store's bookkeeping: everything the call rejects, the grids of its kernels, the padding of the bit-planes, the list of
// tile pairs, and the terminal runs (which need no pair work).  No HIP call and no global in this file: tests/score_plan_kats.cpp includes it
// directly.  Included by twl_score.inc.hip (one translation unit).
#pragma once
#include <cstdint>
#include <vector>

constexpr int32_t kScoreMaxRows = 1 << 20;

// The widest row: the int32 column arithmetic of a column tile's last column (the bound of twl_trim_plan.inc.hip, with this call's tile).
inline int32_t score_max_width(int32_t colTile) { return INT32_MAX - colTile; }

// letter classes without "other": 4 for 'n', 20 for 'p', 0 for any other type
inline int32_t score_classes(char type) { return type == 'n' ? 4 : type == 'p' ? 20 : 0; }
// entries of sub: the pairs a <= b <= K
inline int32_t score_sub_entries(int32_t K) { return (K + 1) * (K + 2) / 2; }
// index of sub[a][b], a <= b <= K: rows a = 0 .. K one after the other, each from b = a
inline int32_t score_sub_index(int32_t K, int32_t a, int32_t b) { return a * (K + 1) - a * (a - 1) / 2 + (b - a); }

// Everything twl_store_score_rows rejects: the message, or nullptr with W filled in.  row_len[q]: current row length of sequence q.
inline const char *check_score_rows(bool haveStore, int32_t n_ids, const int32_t *ids, char type, bool haveSub, bool haveRuns, bool haveTotals, int32_t n_seqs,
                                    const int32_t *row_len, bool levelPrepared, int32_t colTile, int32_t &W)
{
    W = 0;
    if (!haveStore || !ids || !haveSub || !haveRuns || !haveTotals) return "bad argument";
    if (n_ids < 2) return "fewer than two rows listed";
    if (n_ids > kScoreMaxRows) return "more than 2^20 rows listed";
    if (levelPrepared) return "a level is still prepared on the store: commit it first";
    if (score_classes(type) == 0) return "unknown sequence type";
    std::vector<uint8_t> seen((size_t)n_seqs, 0);
    int32_t w = -1;
    for (int32_t k = 0; k < n_ids; ++k) {
        const int32_t id = ids[k];
        if (id < 0 || id >= n_seqs) return "sequence id out of range";
        if (seen[id]) return "a sequence id is listed twice";
        seen[id] = 1;
        if (w < 0) w = row_len[id];
        else if (row_len[id] != w) return "the listed rows differ in length";
    }
    if (w == 0) return "the listed rows have no column";
    if (w > score_max_width(colTile)) return "rows too long for twl_store_score_rows";
    // n (n - 1) / 2 * W < 2^63: every total (ordered pairs times columns at most twice that) then fits 64 bits
    const unsigned __int128 pairs = (unsigned __int128)n_ids * (unsigned __int128)(n_ids - 1) / 2;
    if (pairs * (unsigned __int128)w >= ((unsigned __int128)1 << 63)) return "n (n - 1) / 2 * W reaches 2^63: the totals would not fit";
    W = w;
    return nullptr;
}

// The grids of a call.  Pack: a workgroup per row.  Counts: (column tiles, row slices).  Products: a workgroup per block of columns.  Pairs: a
// workgroup per entry of the tile-pair list.
struct ScoreGrid {
    int64_t words = 0;        // 64-column words that hold a column
    int64_t wordsPad = 0;     // ... rounded up to whole staged slices: the words behind `words` are zero
    int32_t colTiles = 0, rowSlices = 0, prodBlocks = 0;
    int32_t tiles = 0;        // 64-row tiles
    int64_t tilePairs = 0;    // ti <= tj
};
inline const char *plan_score_grid(int32_t W, int32_t n_ids, int32_t slice, int32_t tile, int32_t colTile, int32_t rowSlice, int32_t prodCols, ScoreGrid &g)
{
    g = ScoreGrid{};
    g.words = ((int64_t)W + 63) / 64;
    g.wordsPad = (g.words + slice - 1) / slice * slice;
    g.colTiles = (int32_t)(((int64_t)W + colTile - 1) / colTile);
    g.rowSlices = (int32_t)(((int64_t)n_ids + rowSlice - 1) / rowSlice);
    g.prodBlocks = (int32_t)(((int64_t)W + prodCols - 1) / prodCols);
    g.tiles = (int32_t)(((int64_t)n_ids + tile - 1) / tile);
    g.tilePairs = (int64_t)g.tiles * (g.tiles + 1) / 2;
    if (g.rowSlices > 65535) return "too many rows for twl_store_score_rows";
    return nullptr;
}

// The tile pairs (ti <= tj), ti in the high half of an entry and tj in the low half, by ti and then by tj.
inline void plan_score_tile_pairs(int32_t tiles, std::vector<uint32_t> &out)
{
    out.clear();
    out.reserve((size_t)tiles * ((size_t)tiles + 1) / 2);
    for (int32_t ti = 0; ti < tiles; ++ti)
        for (int32_t tj = ti; tj < tiles; ++tj) out.push_back(((uint32_t)ti << 16) | (uint32_t)tj);
}

// The terminal runs over all ordered pairs, RT, and the columns they hold, GT, from let[c] (letters of column c), first[i] (first letter column
// of row i, W for a row without letters) and last[i] (-1 for such a row).  Row i has a leading run against every row j that holds a letter in
// front of first[i], that is first[j] < first[i], and the run holds j's letters there; the same behind last[i].  A row without letters has one
// range, all of W, counted once.
inline void score_terminals(int32_t n, int32_t W, const uint32_t *let, const int32_t *first, const int32_t *last, uint64_t &RT, uint64_t &GT)
{
    std::vector<uint64_t> pre((size_t)W + 1, 0);                   // pre[c]: letters in columns < c
    for (int32_t c = 0; c < W; ++c) pre[(size_t)c + 1] = pre[c] + let[c];
    std::vector<uint64_t> firstBelow((size_t)W + 2, 0), lastAbove((size_t)W + 2, 0);
    for (int32_t i = 0; i < n; ++i)
        if (first[i] < W) { firstBelow[(size_t)first[i] + 1] += 1; lastAbove[(size_t)last[i]] += 1; }
    // firstBelow[c]: rows whose first letter lies in a column < c; lastAbove[c]: rows whose last letter lies in a column > c
    for (int32_t c = 0; c <= W; ++c) firstBelow[(size_t)c + 1] += firstBelow[c];
    {
        uint64_t run = 0;
        for (int32_t c = W; c >= 0; --c) { const uint64_t here = lastAbove[c]; lastAbove[c] = run; run += here; }
    }
    RT = GT = 0;
    for (int32_t i = 0; i < n; ++i) {
        if (first[i] >= W) { RT += firstBelow[(size_t)W]; GT += pre[W]; continue; }
        RT += firstBelow[first[i]] + lastAbove[last[i]];
        GT += pre[first[i]] + (pre[W] - pre[(size_t)last[i] + 1]);
    }
}
