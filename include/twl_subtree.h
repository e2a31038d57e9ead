/*
 * include/twl_subtree.h -- C ABI of libtwl_align, part 5: the profile of a finished subtree (the reference's -m / --max-subtree mode,
 * `twilight -t tree.nwk -i seqs.fa -o out.aln -m N`).
 *
 * With -m the reference aligns every subtree of the guide tree on its own, keeps one profile per subtree and then aligns those profiles
 * along the tree of subtrees.  The profile of a subtree whose root carries none is the sum of its rows' letters, each row weighted by its
 * sequence weight (SequenceDB::storeSubtreeProfile, reference src/sequencedb.cpp:122-138):
 *
 *   twl_store_weighted_columns   that sum, on the rows of the store, as a cached profile
 *
 * The sum is ORDERED: the reference adds row by row, in the order of the subtree root's seqsIncluded, in fp32, and the profile has to be
 * the same bits.  So every (column, letter) cell is one chain of additions over the rows in the order of the call's id list; no atomics,
 * no partial sums over slices of the rows.
 *
 * Same conventions as twl_align.h: plain C types, 0 or a negative twl_status, twl_last_error() for the text.
 */
#ifndef TWL_SUBTREE_H
#define TWL_SUBTREE_H

#include "twl_level.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The weighted column profile of the rows ids[0, n_ids) of the store, which must all have one length L > 0: float[L][P] with
     out[j][letterIdx(type, toupper(row_t[j]))] += weights[t]      for t = 0 .. n_ids - 1, in that order, in fp32
   ('-' and '.' land in the gap slot), stored as the cached profile `cache_id` (an id new to the store) that twl_level_prepare then takes
   as a side's cache_id.  Refused: n_ids < 1, an id out of range or given twice, rows of different lengths, L == 0, a cache id in use,
   a NULL pointer. */
int twl_store_weighted_columns(twl_store *s, int32_t n_ids, const int32_t *ids, const float *weights, int32_t cache_id);

#ifdef __cplusplus
}
#endif
#endif /* TWL_SUBTREE_H */
