/*
 * include/twl_compare.h -- C ABI of libtwl_align, part 10: an alignment compared with a reference alignment of the same sequences.
 *
 * E is the estimate, R the reference; both hold the same n rows, row k of E and row k of R being the same sequence.  Residue (k, i) is the
 * i-th letter of row k; cE(k, i) and cR(k, i) are its columns in E and in R.  k(c, b) is the number of rows with a residue in E column c and
 * R column b; nE(c) and nR(b) are the letters of a column.  Per E column c:
 *
 *   shared[c]     sum over b of C(k(c, b), 2): the residue pairs of column c that R puts into one column too
 *   letters[c]    nE(c); the column's pairs are C(nE(c), 2)
 *   distinct[c]   the number of b with k(c, b) > 0
 *   recovered[c]  1 iff distinct[c] == 1, nE(c) >= 2 and nE(c) == nR(b) for that b: the two columns hold the same residues
 *
 * and per R column b: ref_letters[b] = nR(b).  Everything is exact integer work; the sums and ratios (SP-score, modeler score, TC) are the
 * caller's.  Only the byte 0x2D ('-') counts as a gap, every other byte is a letter (as in twl_trim.h).  Row k of E and of R must hold the
 * same number of letters, and the same letters after folding a-z to A-Z; a row without letters is allowed.
 *
 *   twl_compare_create    both alignments into device memory, the key of every residue: key[k][c] = cR(k, i) of the letter at E column c
 *   twl_compare_columns   the five arrays above
 *
 * Same conventions as twl_align.h: plain C types, 0 or a negative twl_status, twl_last_error() for the text.
 */
#ifndef TWL_COMPARE_H
#define TWL_COMPARE_H

#include "twl_level.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TWL_COMPARE_MAX_ROWS (1 << 20)

typedef struct twl_compare twl_compare;

/*
 * est_rows[k]: the w_est bytes of row k of E; ref_rows[k]: the w_ref bytes of row k of R (no terminator is read).  Uploads both, builds the
 * keys (n x w_est x 4 bytes, padded to the column tile) and the letters of every R column.
 * Refused, with nothing left allocated and *cmp == NULL: a null pointer (a width of 0 needs no row pointers, but the tables themselves);
 * n < 2 or n > TWL_COMPARE_MAX_ROWS; a negative width; a width above 2^31 - 1 - (columns of a scan round): the bound of the int32 column
 * arithmetic; an allocation that fails (the message gives the bytes asked for); a row whose letter count differs between E and R, or whose
 * letters differ after case folding: TWL_ERR_BAD_ARGUMENT, *bad_row is the SMALLEST such row and the message says whether its count or its
 * letters differ.  *bad_row is -1 in every other case.
 */
int twl_compare_create(int device, int32_t n, int32_t w_est, const char *const *est_rows, int32_t w_ref, const char *const *ref_rows, twl_compare **cmp, int32_t *bad_row);

/*
 * shared_out[w_est], letters_out[w_est], distinct_out[w_est], recovered_out[w_est], ref_letters_out[w_ref]; any pointer may be NULL.  The
 * column kernel runs at every call; the answer is the same every time.
 */
int twl_compare_columns(twl_compare *cmp, uint64_t *shared_out, uint32_t *letters_out, uint32_t *distinct_out, uint8_t *recovered_out, uint32_t *ref_letters_out);

/*
 * upload_ms: both alignments to the device (wall clock); keys_ms: the reference-position and key kernels of twl_compare_create (HIP events);
 * columns_ms: the column kernel of the last twl_compare_columns (HIP events, 0 before the first); download_ms: its copies back (wall clock).
 * Any pointer may be NULL.
 */
int twl_compare_timing(twl_compare *cmp, double *upload_ms, double *keys_ms, double *columns_ms, double *download_ms);

/*
 * The constants of the kernels (the tests put their shapes around them; no device needed): out[0] counters per key window T, out[1] columns
 * of a column tile, out[2] rows a workgroup takes per step of the column kernel, out[3] columns the row scans walk per round.
 */
int twl_compare_describe(int32_t out[4]);

int twl_compare_destroy(twl_compare *cmp);

#ifdef __cplusplus
}
#endif
#endif /* TWL_COMPARE_H */
