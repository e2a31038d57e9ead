// twilight_amd/csrc/twl_place_plan.inc.hip -- what the calls of include/twl_place.h decide on the host, as PURE functions of the call's arguments and of
// the placement's bookkeeping: everything twl_store_count_columns / twl_place_create / twl_place_collect / twl_place_finish reject, and the tables the
// collect's kernel reads.  No HIP call and no global in this file: tests/place_plan_kats.cpp includes it directly.  Included by twl_place.inc.hip
// (one translation unit).
#pragma once
#include <cstdint>
#include <unordered_set>
#include <vector>
#include "twl_path_source.inc.hip"

// A placement as the host knows it.
struct PlaceBook {
    int32_t L = 0;
    std::vector<int32_t> qlen;       // length of every store sequence when the placement began (its path covers that many letters)
    std::vector<int64_t> slot;       // its slot in the arena of final paths (L + qlen bytes)
    std::vector<int32_t> plen;       // collected path length, -1: not collected
    std::vector<int32_t> placed;     // collected ids, in order
    bool finished = false;
};

// Everything twl_store_count_columns rejects: the message, or nullptr with *L the one length of the rows.  row_len[q]: current row length of sequence q.
inline const char *check_count_columns(int32_t n_ids, const int32_t *ids, int32_t cache_id, bool cacheInUse, int32_t n_seqs, const int32_t *row_len, int32_t *L)
{
    if (n_ids < 1 || !ids || cache_id < 0) return "bad argument";
    if (cacheInUse) return "cache id in use";
    *L = (ids[0] >= 0 && ids[0] < n_seqs) ? row_len[ids[0]] : -1;
    for (int32_t t = 0; t < n_ids; ++t) {
        if (ids[t] < 0 || ids[t] >= n_seqs) return "sequence id out of range";
        if (row_len[ids[t]] != *L) return "the rows to count differ in length";
    }
    return nullptr;
}

// twl_place_create: the message, or nullptr with the book of a fresh placement and *arenaBytes the size of its arena.
inline const char *check_place_create(int32_t L, int32_t n_seqs, const int32_t *row_len, PlaceBook &b, int64_t *arenaBytes)
{
    if (L < 0 || n_seqs < 0) return "bad argument";
    b = PlaceBook{};
    b.L = L;
    b.qlen.assign(row_len, row_len + n_seqs);
    b.slot.resize((size_t)n_seqs);
    b.plen.assign((size_t)n_seqs, -1);
    int64_t total = 0;
    for (int32_t i = 0; i < n_seqs; ++i) { b.slot[i] = total; total += (int64_t)L + row_len[i]; }
    *arenaBytes = total;
    return nullptr;
}

struct PlaceCollectPlan {
    std::vector<int32_t> ids, plen, qlen;   // per taking pair (path_len != 0): its sequence, path length, letters
    std::vector<int64_t> dstOff;            // per taking pair: its sequence's slot in the arena
    PathSources src;                        // per taking pair: where its path lives (twl_path_source.inc.hip)
};

// Everything twl_place_collect rejects before a path is looked at: the message, or nullptr with `p` filled in.
inline const char *check_place_collect(const PlaceBook &b, int32_t n_pairs, const int32_t *seq_ids, bool havePaths, const int32_t *path_len, int32_t path_stride,
                                       const uint8_t *from_dp, int32_t n_seqs, const int32_t *row_len, const PathLevelView &lv, PlaceCollectPlan &p)
{
    p = PlaceCollectPlan{};
    if (n_pairs < 0 || (n_pairs > 0 && (!seq_ids || !path_len || path_stride < 1))) return "bad argument";
    if (b.finished) return "twl_place_collect after twl_place_finish";
    if (const char *why = check_path_level(from_dp, n_pairs, lv)) return why;
    std::unordered_set<int32_t> seen;
    for (int32_t i = 0; i < n_pairs; ++i) {
        const int32_t id = seq_ids[i], n = path_len[i];
        if (n == 0) continue;
        if (id < 0 || id >= n_seqs) return "sequence id out of range";
        if (b.plen[id] >= 0 || !seen.insert(id).second) return "sequence collected twice";
        if (row_len[id] != b.qlen[id]) return "the sequence's row has been rewritten since the placement began";
        if (n < 0 || n > path_stride || (int64_t)n > (int64_t)b.L + b.qlen[id]) return "path_len outside [0, min(path_stride, L + len)]";
        if (const char *why = add_path_source(p.src, i, n, from_dp, havePaths, path_stride, lv)) return why;
        p.ids.push_back(id); p.plen.push_back(n); p.qlen.push_back(b.qlen[id]); p.dstOff.push_back(b.slot[id]);
    }
    return nullptr;
}

// After the collect kernel: bad[k] != 0 when taking path k does not cover the backbone's columns and its sequence's letters exactly.  The
// passed paths are collected; returns how many were not.
inline int32_t place_collect_done(PlaceBook &b, const PlaceCollectPlan &p, const int32_t *bad)
{
    int32_t nBad = 0;
    for (size_t k = 0; k < p.ids.size(); ++k) {
        if (bad[k]) ++nBad;
        else { b.plen[p.ids[k]] = p.plen[k]; b.placed.push_back(p.ids[k]); }
    }
    return nBad;
}

// Everything twl_place_finish rejects: the message, or nullptr.
inline const char *check_place_finish(const PlaceBook &b, int32_t n_backbone, const int32_t *backbone_ids, int32_t n_seqs, const int32_t *row_len)
{
    if (n_backbone < 0 || (n_backbone > 0 && !backbone_ids)) return "bad argument";
    if (b.finished) return "twl_place_finish called twice";
    std::unordered_set<int32_t> seen(b.placed.begin(), b.placed.end());
    for (int32_t t = 0; t < n_backbone; ++t) {
        const int32_t id = backbone_ids[t];
        if (id < 0 || id >= n_seqs || row_len[id] != b.L) return "backbone id out of range or not of length L";
        if (!seen.insert(id).second) return "a backbone id is listed twice or was collected";
    }
    for (int32_t id : b.placed)
        if (row_len[id] != b.qlen[id]) return "a placed sequence's row has been rewritten since it was collected";
    return nullptr;
}

// What the scan kernel found: insertions can only add to the backbone's width.  The message, or nullptr.
inline const char *check_place_width(const PlaceBook &b, int32_t W) { return W < b.L ? "final width below the backbone's" : nullptr; }
