/*
 * include/twl_retree_set.h -- C ABI of libtwl_align, part 9: the rows of a finished alignment kept on the device as bit-planes, for a guide tree
 * that is rebuilt in two stages (`twilight-mi355x -i seqs.fa -o out.aln --iterations K --retree-seeds S`).
 *
 * Mask, letters and counts are those of twl_retree.h: column c is kept iff gaps[c] <= max_gaps, both(i, j) counts the kept columns in which
 * rows i and j both hold a letter, match(i, j) those of them in which the letters are equal, letters[i] = both(i, i).
 *
 * A set keeps planes[n][P][words_pad] (P = 3 for 'n', 6 for 'p'; 64 columns per word) and letters[n] of up to TWL_RETREE_SET_MAX_SEQS rows in
 * device memory, and the calls below work on it; no matrix over the whole set is ever formed.  Rows are named by their index in the call that
 * made the set.  Device memory: while the set is made, n * width bytes of rows and width * 4 of gap counts beside the planes (3/8 or 6/8 of
 * the rows) and the letters; the rows and the gap counts are freed before twl_retree_set_create returns.  What does not fit the device's free
 * memory: TWL_ERR_HIP, the text says "out of device memory".
 *
 * Same conventions as twl_align.h: plain C types, 0 or a negative twl_status, twl_last_error() for the text.  Refused before any device work,
 * each with a text of its own: what twl_retree_pair_counts refuses (with the larger cap), a NULL set or pointer, n_seeds outside
 * 1 .. TWL_RETREE_MAX_SEQS, a seed or row id outside the set, the same seed twice, no group, an empty group, a group of more than
 * TWL_RETREE_MAX_SEQS rows, group offsets that do not start at 0 or that decrease, and groups whose blocks hold more than 2^28 entries
 * per matrix.
 */
#ifndef TWL_RETREE_SET_H
#define TWL_RETREE_SET_H

#include "twl_retree.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TWL_RETREE_SET_MAX_SEQS 1048576

typedef struct twl_retree_set twl_retree_set;

/* The geometry of the kernels, for tests that sit on their edges (no device needed): out[0] = rows of a tile of the assign kernel, out[1] =
   seeds of a tile of the assign kernel, out[2] = edge of the square tile of pairs of the groups kernel, out[3] = the largest number of rows
   one launch of the pack kernel takes.  Returns 4, the number of values. */
int twl_retree_set_describe(int32_t out[4]);

/* Uploads the n rows of `width` bytes, counts the gaps of the columns, packs the planes and counts the letters; *kept_out = the number of kept
   columns. */
int twl_retree_set_create(int device, char type, int32_t n, int32_t width, const char *const *rows, int32_t max_gaps, twl_retree_set **set, int32_t *kept_out);
int twl_retree_set_destroy(twl_retree_set *set);

/* out[i] = letters[i], i < n. */
int twl_retree_set_letters(twl_retree_set *set, uint32_t *out);

/* seed_out[i] = the index t into seed_ids of the seed row i goes to; match_out[i] and both_out[i] = the two counts of row i with row
   seed_ids[t] (either or both may be NULL).  A row that is a seed goes to itself, and its two counts are letters[i]; every other one to the t
   with the largest match(i, seed_ids[t]) / both(i, seed_ids[t]), taken as 0 / 1 where both is 0, compared exactly (by cross-multiplying in
   64-bit integers), the smaller t among equals. */
int twl_retree_set_assign(twl_retree_set *set, int32_t n_seeds, const int32_t *seed_ids, int32_t *seed_out, uint32_t *match_out, uint32_t *both_out);

/* The two matrices of every group in one call: the rows of group g are ids[group_off[g] .. group_off[g + 1]), m_g of them, and its blocks
   (m_g x m_g, row-major, symmetric, letters on the diagonal) start at match_out[sum of m_h^2 over h < g] and both_out[the same].  group_off
   has n_groups + 1 entries. */
int twl_retree_set_pair_groups(twl_retree_set *set, int32_t n_groups, const int32_t *group_off, const int32_t *ids, uint32_t *match_out, uint32_t *both_out);

/* Milliseconds spent on this set since it was made: upload, gap kernel, pack and letters kernels, assign kernels, group kernels, and all
   downloads. */
int twl_retree_set_timing(twl_retree_set *set, double *upload_ms, double *gaps_ms, double *pack_ms, double *assign_ms, double *groups_ms, double *download_ms);

#ifdef __cplusplus
}
#endif
#endif /* TWL_RETREE_SET_H */
