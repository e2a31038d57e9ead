/*
 * include/twl_keep.h -- C ABI of libtwl_align, part 11: a placement finished at the backbone's own length
 * (`twilight-mi355x -a backbone.aln -i new.fa -o out.aln --keep-length`).
 *
 * twl_place_finish (include/twl_place.h) merges the insertions of the placed sequences: every row, the backbone's too, is rewritten
 * to the width W = L + the sum of longest[].  The finish below leaves the backbone's coordinates alone instead.  The row of a collected
 * sequence, from its final path (0 = both, 1 = query only, 2 = backbone only), has the L columns of the backbone:
 *   column c   the sequence's letter under code 0, case kept; '-' under code 2
 *   code 1     the letter is left out (dropped); a maximal stretch of code 1 is a dropped run
 * No '.' is written, and no backbone row is named, read or rewritten: the caller keeps the bytes it uploaded.
 * The result is the row twl_place_finish makes with every insertion column (the columns of the blocks longest[k]) deleted.
 *
 * A dropped run is reported as (col, qpos, len): col = 0 .. L backbone columns in front of it, qpos = index of its first letter in the
 * sequence, len = its letters.
 *
 * Same conventions as twl_align.h: plain C types, 0 or a negative twl_status, twl_last_error() for the text.
 */
#ifndef TWL_KEEP_H
#define TWL_KEEP_H

#include "twl_place.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Instead of twl_place_finish, once per placement (after either, both are refused).  Every collected sequence becomes a row of width L as
   above, on the other plane of the store, and is its current row afterwards.  Backbone rows are neither named nor touched.
   *runs_out / *letters_out: dropped runs and letters over all collected sequences. */
int twl_place_finish_keep(twl_place *pl, int64_t *runs_out, int64_t *letters_out);

/* After finish_keep: per listed sequence (collected, each id once) its dropped runs and letters. */
int twl_place_dropped_counts(twl_place *pl, int32_t n, const int32_t *seq_ids, int32_t *runs, int32_t *letters);

/* After finish_keep: the runs of the listed sequences.  Those of seq_ids[i] go to [run_off[i], run_off[i+1]) in path order.
   run_off must be the exclusive scan of the counts (n + 1 entries), else refused. */
int twl_place_dropped_runs(twl_place *pl, int32_t n, const int32_t *seq_ids, const int64_t *run_off, int32_t *col, int32_t *qpos, int32_t *len);

/* Milliseconds (HIP events) of the rows kernel of finish_keep and of the runs kernels of every dropped_runs call since. */
int twl_place_keep_timing(twl_place *pl, double *rows_ms, double *runs_ms);

#ifdef __cplusplus
}
#endif
#endif /* TWL_KEEP_H */
