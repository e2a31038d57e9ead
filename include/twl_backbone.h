/*
 * include/twl_backbone.h -- C ABI of libtwl_align, part 8: the rows of an existing alignment prepared for placement along a guide tree
 * (the reference's PLACE_W_TREE mode, `twilight -t tree.nwk -a backbone.aln -i new.fa -o out.aln`).
 *
 * In that mode the backbone falls into groups: the rows under one unplaced part of the tree stay aligned with each other and enter the
 * progressive alignment as one side.  Before they do, the columns in which every row of a group holds '-' leave the group (reference
 * src/sequencedb.cpp:171-210, a host loop over one group at a time).  Here all groups of the backbone are squeezed by one call, on the
 * rows the store already holds:
 *
 *   twl_store_squeeze_groups   per group: the all-gap columns out of every row
 *
 * Only the byte 0x2D ('-') counts as a gap: a column of '.' stays.  Letter case and every other byte are kept as they are.
 *
 * Same conventions as twl_align.h: plain C types, 0 or a negative twl_status, twl_last_error() for the text.
 */
#ifndef TWL_BACKBONE_H
#define TWL_BACKBONE_H

#include "twl_level.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Group g is the rows ids[group_off[g] .. group_off[g + 1]) of the store: at least one row, all of one current length L_g (0 is allowed, and
 * groups may differ in it); the ids may lie on either plane, in any order.  Column j of a group is dropped iff every row of the group holds
 * '-' there.  Every row of the group becomes its kept bytes, in order (its current row from here on); its length becomes the kept count,
 * which also goes to len_out[g].  Rows that are not listed are untouched.  n_groups == 0 does nothing.
 * Refused, with nothing changed: a null table, offsets that do not start at 0 or do not ascend, an empty group, an id outside the store,
 * an id listed twice (inside one group or across two), two lengths in one group, a level that is still prepared on the store.
 * All groups of a call run in three kernel launches; len_out is the one read-back.
 */
int twl_store_squeeze_groups(twl_store *s, int32_t n_groups, const int32_t *group_off /* n_groups + 1 */, const int32_t *ids, int32_t *len_out /* n_groups */);

/* HIP-event time of the kernels of the last twl_store_squeeze_groups on this store, in ms (0 before the first call and after a call without groups). */
int twl_store_squeeze_timing(twl_store *s, double *ms);

/* The constants of the kernels: columns of a column tile, rows of a row slice, columns the scan walks per round (the tests put their shapes around them). */
int twl_squeeze_describe(int32_t *col_tile, int32_t *row_slice, int32_t *scan_chunk);

#ifdef __cplusplus
}
#endif
#endif /* TWL_BACKBONE_H */
