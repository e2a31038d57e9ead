/*
 * include/twl_trim.h -- C ABI of libtwl_align, part 9: the finished rows of a store written without their gappy columns.
 *
 * The alignments this library produces are several times wider than their sequences, and most of that width is gaps.  What reads them
 * next (a tree builder, a variant caller, a viewer) takes the columns that enough rows fill, or the columns of one sequence.  One call
 * decides the columns over the rows the store holds and compacts every listed row on the device, so that only kept columns are read back:
 *
 *   twl_store_trim_columns   one keep decision per column over all listed rows; every listed row becomes its kept bytes
 *   twl_store_trim_read      the kept columns' original indices and the gap count of every original column
 *
 * Only the byte 0x2D ('-') counts as a gap: '.' is not a gap.  Letter case and every other byte are kept as they are (as in twl_retree.h
 * and twl_backbone.h).
 *
 * Same conventions as twl_align.h: plain C types, 0 or a negative twl_status, twl_last_error() for the text.
 */
#ifndef TWL_TRIM_H
#define TWL_TRIM_H

#include "twl_level.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TWL_TRIM_MAX_GAPS 0   /* keep column c iff gaps[c] <= arg */
#define TWL_TRIM_TO_ROW   1   /* keep column c iff the current row of sequence `arg` (one of ids) holds a byte other than '-' at c */

/*
 * The rows ids[0 .. n_ids) of the store all have one current length W (0 is allowed); they may lie on either plane, in any order.
 * gaps[c] is the number of listed rows whose byte at column c is '-'.  Column c is kept by the rule above.  After the call every listed row
 * is its kept bytes, in order, on its other plane (its current row from here on), and its length is *kept_out.  Rows that are not listed and
 * cached profiles are untouched.  kept == 0 and kept == W are ordinary results (with kept == W the rows are rewritten all the same: the
 * kernels never wait for a count to come back).
 * The kept-column list and the gap counts stay in device buffers of the store until its next trim or twl_store_destroy.
 * Refused, with nothing changed: a null store, ids or kept_out; n_ids < 1; an id outside the store; an id listed twice; two different
 * lengths among the listed rows; a level that is still prepared on the store; an unknown rule; TWL_TRIM_MAX_GAPS with arg < 0 or
 * arg > n_ids; TWL_TRIM_TO_ROW with arg not among ids; W above 2^31 - 1 - (columns of a column tile): column tiles lie on the grid's x,
 * which holds more of them than an int32 width can fill, so the bound is that of the int32 column arithmetic inside a tile.
 * One zeroing and five kernel launches whatever the shape, nothing waits in between; kept_out is the one read-back.
 */
int twl_store_trim_columns(twl_store *s, int32_t n_ids, const int32_t *ids, int32_t rule, int32_t arg, int32_t *kept_out);

/*
 * Of the last twl_store_trim_columns on this store: cols_out[k] = the original column of kept column k (kept entries, ascending),
 * gaps_out[c] = gaps of original column c (W entries).  Either may be NULL.  Refused before a first trim.
 */
int twl_store_trim_read(twl_store *s, int32_t *cols_out /* kept, ascending original columns */, uint32_t *gaps_out /* W */);

/* HIP-event time of the kernels of the last twl_store_trim_columns on this store, in ms (0 before the first call). */
int twl_store_trim_timing(twl_store *s, double *ms);

/*
 * The constants of the kernels (the tests put their shapes around them; no device needed): out[0] columns of a column tile, out[1] rows of
 * a row slice of the counts kernel, out[2] columns the scan walks per round, out[3] rows after which the counts kernel flushes its packed
 * byte counters into 32-bit ones.  A thread owns 16 columns.
 */
int twl_trim_describe(int32_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* TWL_TRIM_H */
