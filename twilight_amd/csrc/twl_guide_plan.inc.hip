// twilight_amd/csrc/twl_guide_plan.inc.hip -- what twl_guide_kmer_counts and twl_guide_shared (include/twl_guide.h) decide on the host, as PURE
// functions of the call's arguments: everything the calls reject, and the sizes of what they allocate.  No HIP call and no global in this
// file: tests/guide_plan_kats.cpp includes it directly.  Included by twl_guide.inc.hip (one translation unit).
#pragma once
#include <cstddef>
#include <cstdint>

constexpr int32_t kGuideMaxSeqs = 16384;      // TWL_GUIDE_MAX_SEQS: the matrix of shared counts is 1 GiB then

// bins of the type's k-mers (4^6, 6^5), 0 for a type that is neither
inline int32_t guide_bins(char type) { return type == 'n' ? 4096 : type == 'p' ? 7776 : 0; }

// the bins padded with zero bins to a multiple of the slice the all-pairs kernel stages
inline int32_t guide_bins_padded(int32_t bins, int32_t slice) { return (bins + slice - 1) / slice * slice; }

// Everything the two calls reject: the message, or nullptr with *total the letters of all sequences.  `out`: the call's output pointer.
inline const char *check_guide(char type, int32_t n, const char *const *seqs, const int32_t *lens, const void *out, uint64_t *total)
{
    if (guide_bins(type) == 0) return "the type must be 'n' or 'p'";
    if (n < 1) return "no sequences";
    if (n > kGuideMaxSeqs) return "more than 16384 sequences";
    if (!seqs || !lens || !out) return "bad argument";
    uint64_t sum = 0;
    for (int32_t i = 0; i < n; ++i) {
        if (lens[i] < 0) return "negative sequence length";
        if (lens[i] > 0 && !seqs[i]) return "bad argument";
        sum += (uint64_t)lens[i];
    }
    if (total) *total = sum;
    return nullptr;
}
