/*
 * include/twl_merge.h -- C ABI of libtwl_align, part 4: existing alignments merged into one (the reference's MERGE_MSA mode,
 * `twilight -f DIR -o out.aln`; its currentTask == 2 machinery).
 *
 * The progressive pass of that mode works on PROFILES: every input alignment is a cached profile (twl_store_count_columns), a merge is a
 * level whose two sides are cached profiles with no members (include/twl_level.h), and the commit merges the two caches.  No row is
 * touched while the merges pile up.  What moves instead is one column map per input alignment (the reference's SequenceDB::subtreeAln,
 * src/alignment-helper.cpp:402-423, :449-470), and every row is rewritten through its alignment's map once, at the end
 * (src/io.cpp:355-449).
 *
 * A GROUP is one input alignment: rows of the store that all have one length L_g, and a column map pos_g[L_g] (identity at creation).
 * pos_g[c] is the column of the current merged alignment that holds the group's original column c.  Path codes are those of the level
 * API: 0 = both, 1 = query only, 2 = reference only.
 *
 *   twl_merge_apply    for every pair of a level: rpos[r] = the path position of the r-th code != 1, qpos[q] = that of the q-th code != 2;
 *                      pos_g[c] = rpos[pos_g[c]] for every group under the reference side, qpos for those under the query side
 *   twl_merge_finish   every row of every group rewritten to the final width W: out[w] = row[c] where pos_g[c] == w, '-' elsewhere
 *                      (letter case and '.' are kept)
 *
 * Same conventions as twl_align.h: plain C types, 0 or a negative twl_status, twl_last_error() for the text.
 */
#ifndef TWL_MERGE_H
#define TWL_MERGE_H

#include "twl_level.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct twl_merge twl_merge;     /* opaque: the column maps of one merge, on the store's device */

/* n_groups groups on store `s` (which must outlive the merge): group g holds the rows row_ids[group_off[g], group_off[g + 1]), at least
   one, all of one length, each row of the store in at most one group.  Every map starts as the identity. */
int  twl_merge_create(twl_store *s, int32_t n_groups, const int32_t *group_off, const int32_t *row_ids, twl_merge **out);
void twl_merge_destroy(twl_merge *mg);

/*
 * The final paths of the n_pairs pairs of a level, applied to the maps of the groups under their sides: pair i has the groups
 * ref_groups[ref_off[i], ref_off[i + 1]) under its reference side and qry_groups[qry_off[i], qry_off[i + 1]) under its query side.
 * Path sources as in twl_place_collect:
 *   from_dp[i] == 1   row i of the prepared level's DP output (path_len[i] = the length twl_level_align returned)
 *   from_dp[i] == 2   row i of the level's path buffer (twl_level_restore, or twl_level_write_final), path_stride = the restore's pitch
 *   from_dp[i] == 0   paths + i * path_stride, from the host (from_dp == NULL: every row; no level needed then)
 * path_len[i] == 0 skips pair i.  The call runs BEFORE the level's commit and leaves the level as it is, so that
 * twl_level_commit_from_dp can still merge the cached profiles.  Refused, with every map left as it was: a side without groups or whose
 * groups differ in their current width; a group under two sides of one call; a path whose count of codes != 1 differs from the
 * current width of its reference side's groups, or whose count of codes != 2 differs from that of its query side's groups, or that
 * holds a code other than 0, 1, 2.  After the call the current width of every group of pair i is path_len[i].
 */
int  twl_merge_apply(twl_merge *mg, twl_store *s, int32_t n_pairs, const int32_t *ref_off, const int32_t *ref_groups, const int32_t *qry_off,
                     const int32_t *qry_groups, const int8_t *paths, const int32_t *path_len, int32_t path_stride, const uint8_t *from_dp);

/* The final rows: every row of every group becomes a row of width *W_out, the store's current row of that sequence (read them with
   twl_store_read_rows_of).  All groups must have reached one width.  Once per merge. */
int  twl_merge_finish(twl_merge *mg, int32_t *W_out);

/* pos_g[0, L_g) of group `group` as it stands (out: L_g ints). */
int  twl_merge_read_map(twl_merge *mg, int32_t group, int32_t *out);

/* HIP-event times (ms), for reports: the kernels of every twl_merge_apply so far (with the check of the path counts between them), the
   kernels of twl_merge_finish, and of those the row rewrite alone.  Any pointer may be NULL. */
int  twl_merge_timing(twl_merge *mg, double *apply_ms, double *finish_ms, double *rewrite_ms);

#ifdef __cplusplus
}
#endif
#endif /* TWL_MERGE_H */
