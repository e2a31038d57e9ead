// twilight_amd/csrc/twl_retree_plan.inc.hip -- what twl_retree_column_gaps and twl_retree_pair_counts (include/twl_retree.h) decide on the host, as
// PURE functions of the call's arguments: everything the calls reject, the mask's threshold and the sizes of what they allocate.  No HIP call
// and no global in this file: tests/retree_plan_kats.cpp includes it directly.  Included by twl_retree.inc.hip (one translation unit).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

constexpr int32_t kRetreeMaxSeqs = 16384;      // TWL_RETREE_MAX_SEQS: each of the two matrices of pair counts is 1 GiB then

// planes of a packed row: `valid` and the bits of the letter's code (4 letters: 2 bits; 20 letters: 5 bits); 0 for a type that is neither
inline int32_t retree_planes(char type) { return type == 'n' ? 3 : type == 'p' ? 6 : 0; }

// packed words of a row of `width` columns, padded with zero words to a multiple of the slice the pair kernel stages
inline int64_t retree_words_padded(int32_t width, int32_t columns_per_word, int32_t slice_words)
{
    const int64_t words = ((int64_t)width + columns_per_word - 1) / columns_per_word;
    return (words + slice_words - 1) / slice_words * slice_words;
}

// max_gaps = floor(T * n) in IEEE double: a column is kept iff at most that many of its n rows hold '-'
inline int32_t retree_max_gaps(double T, int32_t n) { return (int32_t)std::floor(T * (double)n); }

// device bytes of a pair_counts call: the rows, the gap counts, the planes and the two matrices
inline uint64_t retree_device_bytes(char type, int32_t n, int32_t width, int64_t words_pad)
{
    return (uint64_t)n * (uint64_t)width + (uint64_t)width * 4 + (uint64_t)n * (uint64_t)retree_planes(type) * (uint64_t)words_pad * 8 + 2 * (uint64_t)n * (uint64_t)n * 4;
}

// What both calls reject about the rows: the message, or nullptr.
inline const char *check_retree_rows(int32_t n, int32_t width, const char *const *rows)
{
    if (n < 1) return "no rows";
    if (n > kRetreeMaxSeqs) return "more than 16384 rows";
    if (width < 1) return "the rows have no columns";
    if (!rows) return "bad argument";
    for (int32_t i = 0; i < n; ++i)
        if (!rows[i]) return "bad argument";
    return nullptr;
}

// Everything twl_retree_column_gaps rejects.
inline const char *check_retree_gaps(int32_t n, int32_t width, const char *const *rows, const void *gaps_out)
{
    if (const char *why = check_retree_rows(n, width, rows)) return why;
    return gaps_out ? nullptr : "bad argument";
}

// Everything twl_retree_pair_counts rejects.
inline const char *check_retree_pairs(char type, int32_t n, int32_t width, const char *const *rows, int32_t max_gaps, const void *match_out, const void *both_out,
                                      const void *kept_out)
{
    if (retree_planes(type) == 0) return "the type must be 'n' or 'p'";
    if (const char *why = check_retree_rows(n, width, rows)) return why;
    if (max_gaps < 0 || max_gaps > n) return "max_gaps must lie in 0 .. n";
    if (!match_out || !both_out || !kept_out) return "bad argument";
    return nullptr;
}
