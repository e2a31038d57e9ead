/*
 * include/twl_place.h -- C ABI of libtwl_align, part 3: new sequences placed into an existing alignment, without a tree
 * (the reference's PLACE_WO_TREE mode, `twilight -a backbone.aln -i new.fa -o out.aln`).
 *
 * Every new sequence is aligned, independently, to the profile of the whole backbone alignment: one wide level of the device-resident
 * level API (include/twl_level.h) whose reference sides all use the cached profile twl_store_count_columns made.  What follows the DP
 * moves onto the device too:
 *
 *   twl_store_count_columns   readAlignment's column counts (reference src/io.cpp:200-238)
 *   twl_place_collect         the final path of every pair kept in HBM; mergeInsertions' longest insertion in front of every
 *                             backbone column (src/alignment-helper.cpp:593-691), folded in as the pairs come
 *   twl_place_finish          every placed and every backbone row rewritten to the final width W (src/io.cpp:355-449)
 *
 * Path codes are those of the level API: 0 = both, 1 = query only (an insertion), 2 = reference only.  The final rows:
 *   a backbone row   its column i at ins[i] + longest[i], '.' in every insertion column
 *   a placed row     its letters in the backbone columns (code 0), '-' where it has none (code 2), its own insertion letters
 *                    left-aligned in each insertion block (code 1), '.' for the rest of the block
 * with longest[k] (k = 0..L) the longest run of code 1 any collected path has in front of backbone column k (k = L: after the last one),
 * ins[k] = k + longest[0] + ... + longest[k-1] and W = L + the sum of longest.  Letter case is kept.
 *
 * Same conventions as twl_align.h: plain C types, 0 or a negative twl_status, twl_last_error() for the text.
 */
#ifndef TWL_PLACE_H
#define TWL_PLACE_H

#include "twl_level.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Column counts of the rows ids[0, n_ids) of the store, which must all have one length L: float[L][P] with the count of letter index
   letterIdx(type, toupper(c)) in every column ('-' and '.' included), stored as the cached profile `cache_id` (an id new to the store) that
   twl_level_prepare then takes as a side's cache_id (num = weight = n_ids for readAlignment's node).  Counts are exact below 2^24 rows. */
int twl_store_count_columns(twl_store *s, int32_t n_ids, const int32_t *ids, int32_t cache_id);

typedef struct twl_place twl_place;     /* opaque: paths and insertion table of one placement, on the store's device */

/* A placement against a backbone of L columns, on store `s` (which must outlive it).  Room for one final path per sequence of the store. */
int  twl_place_create(twl_store *s, int32_t L, twl_place **out);
void twl_place_destroy(twl_place *pl);

/*
 * Takes the final paths of n_pairs sequences (seq_ids[i]: a store id whose current row is still the sequence itself; each id once per
 * placement) against the backbone's L columns:
 *   from_dp[i] == 1   row i of the prepared level's DP output (pair i of the level, path_len[i] = the length twl_level_align returned)
 *   from_dp[i] == 2   row i of the level's path buffer (twl_level_restore, or twl_level_write_final), path_stride = the restore's pitch
 *   from_dp[i] == 0   paths + i * path_stride, from the host (from_dp == NULL: every row; no level needed then)
 * path_len[i] == 0 skips pair i.  Each path must hold exactly L codes != 1 and len(sequence) codes != 2.  The paths are kept in the
 * placement, their insertions folded into longest[]; no row is rewritten and no cache merged.  A path of another shape is refused: the
 * call fails, nothing of that path is folded in and its sequence may be collected again, while the well-formed paths of the same call
 * stay collected (collecting one of them again is refused as collected twice).  With from_dp given, the level ends here
 * (its buffers go back to the device as at a commit): the next chunk of pairs starts with twl_level_prepare.
 */
int twl_place_collect(twl_place *pl, twl_store *s, int32_t n_pairs, const int32_t *seq_ids, const int8_t *paths, const int32_t *path_len,
                      int32_t path_stride, const uint8_t *from_dp);

/* The final rows: every collected sequence and the n_backbone rows backbone_ids[] (length L each) become rows of width *W_out, the
   store's current rows of those sequences (read them with twl_store_read_rows_of).  Once per placement. */
int twl_place_finish(twl_place *pl, int32_t n_backbone, const int32_t *backbone_ids, int32_t *W_out);

/* longest[0, L] as collected so far (out: L + 1 ints). */
int twl_place_read_insertions(twl_place *pl, int32_t *out);

#ifdef __cplusplus
}
#endif
#endif /* TWL_PLACE_H */
