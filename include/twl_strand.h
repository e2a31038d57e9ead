/*
 * include/twl_strand.h -- C ABI of libtwl_align, part 10: on which strand every sequence of a set lies
 * (`twilight-mi355x --adjust-direction`).  Nucleotides only.
 *
 * The calls work on a twl_guide_set (include/twl_guide.h), whose 6-mer counts c_i and sums w_i stay on the device.
 *
 *   rc(b)     the 6-mer code b (base 4, first letter most significant) of the reverse complement of the 6-mer: its digits in reverse
 *             order, every digit d replaced by 3 - d.  The counts of a reverse-complemented sequence are c_i[rc(b)].
 *   S(i, j)   sum over b of min(c_i[b], c_j[b])        (twl_guide.h)
 *   O(i, j)   sum over b of min(c_i[b], c_j[rc(b)])    what i shares with the reverse complement of j; O(i, j) = O(j, i)
 *
 * Same conventions as twl_align.h: plain C types, 0 or a negative twl_status, twl_last_error() for the text.  Refused before any device
 * work, each with a text of its own: a set of proteins, a NULL set or pointer, n_seeds or n_ids outside 1 .. TWL_GUIDE_MAX_SEQS, an id
 * outside the set, the same id twice, a flip byte other than 0 or 1.
 */
#ifndef TWL_STRAND_H
#define TWL_STRAND_H

#include "twl_guide.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rc(b), or -1 for b outside 0 .. 4095.  Needs no device. */
int32_t twl_strand_rc_bin(int32_t b);

/* out[a][b] = O(ids[a], ids[b]): n_ids x n_ids, row-major, symmetric; the diagonal is O(i, i), what a sequence shares with its own
   reverse complement. */
int twl_guide_set_opposite(twl_guide_set *set, int32_t n_ids, const int32_t *ids, uint32_t *out);

/* The direction of every sequence i of the set against seeds whose directions are known (seed_flip[t] = 1: seed t lies reversed).
   The candidates of i are (t, r), t < n_seeds, r in {0, 1}: s = r ? O(i, seed_ids[t]) : S(i, seed_ids[t]), m = min(w_i, w_seed), s / m
   taken as 0 / 1 where m is 0.  The first candidate wins in the order: larger s / m, compared exactly (by cross-multiplying in 64-bit
   integers), then smaller t, then smaller d = r XOR seed_flip[t].  A sequence that is a seed goes to itself with d = seed_flip[t] and
   s = w_i.  seed_out[i] = t, dir_out[i] = d (1: reverse-complement the sequence), shared_out[i] = s (shared_out may be NULL). */
int twl_guide_set_strand_assign(twl_guide_set *set, int32_t n_seeds, const int32_t *seed_ids, const uint8_t *seed_flip, int32_t *seed_out, uint8_t *dir_out,
                                uint32_t *shared_out);

/* Milliseconds the two calls above spent on this set since it was made: permute kernels, assign kernels, opposite kernels, and their
   downloads.  twl_guide_set_timing does not count them. */
int twl_guide_set_strand_timing(twl_guide_set *set, double *permute_ms, double *assign_ms, double *opposite_ms, double *download_ms);

#ifdef __cplusplus
}
#endif
#endif /* TWL_STRAND_H */
