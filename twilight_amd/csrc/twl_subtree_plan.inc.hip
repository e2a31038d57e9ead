// twilight_amd/csrc/twl_subtree_plan.inc.hip -- what twl_store_weighted_columns (include/twl_subtree.h) decides on the host, as a PURE function of
// the call's arguments and of the store's row lengths: everything the call rejects.  No HIP call and no global in this file:
// tests/subtree_plan_kats.cpp includes it directly.  Included by twl_subtree.inc.hip (one translation unit).
#pragma once
#include <cstdint>
#include <unordered_set>

// Everything twl_store_weighted_columns rejects: the message, or nullptr with *L the one length of the rows.  row_len[q]: current row length of sequence q.
inline const char *check_weighted_columns(int32_t n_ids, const int32_t *ids, const float *weights, int32_t cache_id, bool cacheInUse, int32_t n_seqs,
                                          const int32_t *row_len, int32_t *L)
{
    if (n_ids < 1 || !ids || !weights || cache_id < 0) return "bad argument";
    if (cacheInUse) return "cache id in use";
    *L = (ids[0] >= 0 && ids[0] < n_seqs) ? row_len[ids[0]] : -1;
    std::unordered_set<int32_t> seen;
    for (int32_t t = 0; t < n_ids; ++t) {
        if (ids[t] < 0 || ids[t] >= n_seqs) return "sequence id out of range";
        if (!seen.insert(ids[t]).second) return "sequence id given twice";
        if (row_len[ids[t]] != *L) return "the rows of the profile differ in length";
    }
    if (*L == 0) return "the rows of the profile are empty";
    return nullptr;
}
