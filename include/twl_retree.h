/*
 * include/twl_retree.h -- C ABI of libtwl_align, part 7: what a guide tree is rebuilt from once an alignment exists
 * (`twilight-mi355x -i seqs.fa -o out.aln --iterations K`).
 *
 * Input: the n rows of a finished alignment, all `width` bytes long.
 *
 *   mask      gaps[c] = the number of rows whose byte at column c is '-' (that byte alone).  Column c is kept iff gaps[c] <= max_gaps; the
 *             caller computes max_gaps = floor(T * n) in double (retree_max_gaps in twl_retree_plan.inc.hip; T is --mask-gappy).
 *   letters   type 'n': A=0 C=1 G=2 T=U=3; type 'p': ACDEFGHIKLMNPQRSTVWY as 0 .. 19.  Either case.  Every other byte ('-', '.', N, X, B, Z,
 *             '*', ...) is no letter.
 *   counts    both(i, j)  = the kept columns in which rows i and j both hold a letter,
 *             match(i, j) = those of them in which the two letters are equal;
 *             exact 32-bit unsigned integers, symmetric, both(i, i) = match(i, i) = the letters of row i in kept columns.
 *
 * The calls need no store: they take the rows from the host, work on the device and bring the result back.  The distances
 * d = 1 - match / both, the clustering and the Newick text are host code (twilight_amd/csrc/host/retree.cpp, guide_upgma.hpp).
 *
 * Same conventions as twl_align.h: plain C types, 0 or a negative twl_status, twl_last_error() for the text.  Refused before any device
 * work: n < 1, n > TWL_RETREE_MAX_SEQS, width < 1, max_gaps < 0 or > n, a type other than 'n' or 'p', a NULL pointer (a row's included).
 * Device memory of a call: n * width bytes of rows, 3/8 ('n') or 6/8 ('p') of that again for the bit-planes, and the two n x n matrices:
 * 1 GiB each at the cap.  What does not fit the device's free memory: TWL_ERR_HIP, the text says "out of device memory".
 */
#ifndef TWL_RETREE_H
#define TWL_RETREE_H

#include "twl_align.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TWL_RETREE_MAX_SEQS 16384      /* match and both are 1 GiB each then */

/* The geometry of the kernels, for tests that sit on their edges (no device needed): out[0] = columns per packed word, out[1] = edge of the
   square tile of pairs of the pair kernel, out[2] = words of a staged slice (a row's words are padded with zero words to a multiple of it),
   out[3] = rows a workgroup of the gap kernel counts.  Returns 4, the number of values. */
int twl_retree_describe(int32_t out[4]);

/* gaps_out[c] = gaps[c], c < width.  Diagnostics and tests. */
int twl_retree_column_gaps(int device, int32_t n, int32_t width, const char *const *rows, uint32_t *gaps_out);

/* match_out[i][j] = match(i, j), both_out[i][j] = both(i, j): n x n each; *kept_out = the number of kept columns. */
int twl_retree_pair_counts(int device, char type, int32_t n, int32_t width, const char *const *rows, int32_t max_gaps,
                           uint32_t *match_out, uint32_t *both_out, int32_t *kept_out);

/* Milliseconds of the last twl_retree_pair_counts of this device: upload, gap kernel, pack kernel, pair kernel, download. */
int twl_retree_timing(int device, double *upload_ms, double *gaps_ms, double *pack_ms, double *pairs_ms, double *download_ms);

#ifdef __cplusplus
}
#endif
#endif /* TWL_RETREE_H */
