// twilight_amd/csrc/twl_strand_plan.inc.hip -- what the calls of include/twl_strand.h decide on the host, as PURE
// functions of the calls' arguments: rc(b) and everything the calls reject.  No HIP call and no global in this file:
// tests/strand_plan_kats.cpp includes it directly.  Included by twl_strand.inc.hip (one translation unit).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>
#include "twl_guide_set_plan.inc.hip"

// rc(b): the digits of the 6-digit base-4 number b in reverse order, every digit d replaced by 3 - d; -1 outside 0 .. 4095
inline int32_t strand_rc_bin(int32_t b)
{
    if (b < 0 || b > 4095) return -1;
    int32_t r = 0;
    for (int k = 0; k < 6; ++k) { r = r * 4 + (3 - b % 4); b /= 4; }
    return r;
}

// the ids of a call on a nucleotide set of n sequences: `count` of them, each inside the set, none twice
inline const char *check_strand_ids(int32_t n, int32_t count, const int32_t *ids, const char *range, const char *outside, const char *twice)
{
    if (count < 1 || count > kGuideMaxSeqs) return range;
    std::vector<bool> seen((size_t)n, false);
    for (int32_t t = 0; t < count; ++t) {
        if (ids[t] < 0 || ids[t] >= n) return outside;
        if (seen[(size_t)ids[t]]) return twice;
        seen[(size_t)ids[t]] = true;
    }
    return nullptr;
}

// twl_guide_set_opposite on a set of n sequences of `type` (has_set: the handle is not null)
inline const char *check_strand_opposite(bool has_set, char type, int32_t n, int32_t n_ids, const int32_t *ids, const void *out)
{
    if (!has_set || !ids || !out) return "bad argument";
    if (type != 'n') return "the strand calls work on a set of nucleotide sequences";
    return check_strand_ids(n, n_ids, ids, "the number of ids must be between 1 and 16384", "id out of range", "the same sequence is listed twice");
}

// twl_guide_set_strand_assign on a set of n sequences of `type`; shared_out may be null
inline const char *check_strand_assign(bool has_set, char type, int32_t n, int32_t n_seeds, const int32_t *seed_ids, const uint8_t *seed_flip, const void *seed_out,
                                       const void *dir_out)
{
    if (!has_set || !seed_ids || !seed_flip || !seed_out || !dir_out) return "bad argument";
    if (type != 'n') return "the strand calls work on a set of nucleotide sequences";
    if (const char *why = check_strand_ids(n, n_seeds, seed_ids, "the number of seeds must be between 1 and 16384", "seed id out of range", "the same sequence is a seed twice"))
        return why;
    for (int32_t t = 0; t < n_seeds; ++t)
        if (seed_flip[t] > 1) return "a seed's flip must be 0 or 1";
    return nullptr;
}
