/*
 * include/twl_score.h -- C ABI of libtwl_align, part 11: the exact integers of the affine sum-of-pairs score of a store's finished rows.
 *
 * The library writes many different alignments of one set of sequences.  Which of two is better under the run's own substitution scores
 * and gap penalties is their sum-of-pairs score.  Its substitution part follows from per-column class counts; its gap part needs, for every
 * ordered pair of rows, the gap runs of the pair's projection.  One call returns every integer the score is a linear function of:
 *
 *   twl_store_score_rows     sub[a][b], runs_row[i] and the totals R, G, RT, GT, letters of the listed rows
 *
 * Only the byte 0x2D ('-') is a gap; every other byte is a letter (as in twl_trim.h and twl_compare.h).  Letter classes: type 'n' A, C, G,
 * T = U as 0 .. 3, type 'p' ACDEFGHIKLMNPQRSTVWY as 0 .. 19, either case; every other letter is class K, "other" (K = 4 or 20).
 *
 * Over the n listed rows of W columns, with cnt[c][a] the rows of class a at column c, g[c] the gaps and let[c] = n - g[c]:
 *   sub[a][b]    a <= b <= K: the sum over c of cnt[c][a] * cnt[c][b] (a < b), of cnt[c][a] (cnt[c][a] - 1) / 2 (a = b); (K + 1)(K + 2) / 2
 *                entries, the rows a = 0 .. K one after the other, each from b = a
 *   runs_row[i]  the sum over j != i of the gap runs of row i against row j: in the pair's projection (the columns where i or j holds a
 *                letter) the maximal stretches in which i holds '-'
 *   R            the sum of runs_row;   G  the sum over c of g[c] * let[c] (the gap columns over all ordered pairs)
 *   RT, GT       the runs that touch the first or the last projected column (one that touches both counts once) and the columns they hold
 *   letters      the sum of let
 *
 * Same conventions as twl_align.h: plain C types, 0 or a negative twl_status, twl_last_error() for the text.
 */
#ifndef TWL_SCORE_H
#define TWL_SCORE_H

#include "twl_level.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TWL_SCORE_MAX_ROWS (1 << 20)

/*
 * The rows ids[0 .. n_ids) of the store all have one current length W; they may lie on either plane, in any order; row k of the call is
 * ids[k].  sub_out takes (K + 1)(K + 2) / 2 entries, runs_row_out n_ids, totals_out R, G, RT, GT, letters.  Nothing in the store changes.
 * Refused: a null pointer; n_ids < 2 or n_ids > 2^20; an id outside the store or listed twice; two different lengths among the listed rows;
 * a level that is still prepared on the store; a type other than 'n' or 'p'; W = 0; W above 2^31 - 1 - (columns of a counts tile);
 * n (n - 1) / 2 * W >= 2^63 (the totals would not fit).  A device allocation that fails is refused with the bytes that were asked for.
 */
int twl_store_score_rows(twl_store *s, int32_t n_ids, const int32_t *ids, char type, uint64_t *sub_out, uint64_t *runs_row_out, uint64_t totals_out[5]);

/* HIP-event times of the last twl_store_score_rows on this store, in ms (0 before the first call): the pack kernel, the two column kernels,
   the pair kernel.  Any pointer may be NULL. */
int twl_store_score_timing(twl_store *s, double *pack_ms, double *columns_ms, double *pairs_ms);

/*
 * The constants of the kernels (the tests put their shapes around them; no device needed): out[0] 64-bit words of a row's plane staged per
 * step of the pair kernel (the plane is padded with zero words to a multiple of it), out[1] rows of a pair tile's edge, out[2] rows of a row
 * slice of the counts kernel, out[3] rows after which the counts kernel flushes its packed byte counters.
 */
int twl_score_describe(int32_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* TWL_SCORE_H */
