/*
 * include/twl_guide.h -- C ABI of libtwl_align, part 6: what a guide tree is built from when the user brings none
 * (`twilight-mi355x -i seqs.fa -o out.aln` without -t).
 *
 * The distance of two sequences is taken from the k-mers they share:
 *
 *   letters   type 'n': A=0 C=1 G=2 T=U=3; type 'p': the six Dayhoff classes AGPST=0 C=1 DENQ=2 FWY=3 HKR=4 ILMV=5.  Either case.
 *             Every other byte is invalid.
 *   k-mers    k = 6 for 'n' (4096 bins), k = 5 for 'p' (7776 bins).  The code of a window of k letters is its letters read as a base-4
 *             (base-6) number, first letter most significant.  A window that holds an invalid byte is not counted; a sequence shorter
 *             than k has no window.  c_i[b] = the number of windows of sequence i with code b, saturated at 65535.
 *   shared    S(i, j) = sum over b of min(c_i[b], c_j[b]), an exact 32-bit unsigned integer; S(i, i) = sum over b of c_i[b] = w_i.
 *
 * The calls need no store: they take the sequences from the host, work on the device and bring the result back.  The distances, the
 * clustering and the Newick text are host code (twilight_amd/csrc/host/guide.cpp).
 *
 * Same conventions as twl_align.h: plain C types, 0 or a negative twl_status, twl_last_error() for the text.  Refused before any device
 * work: n < 1, n > TWL_GUIDE_MAX_SEQS, a negative length, a type other than 'n' or 'p', a NULL pointer.  n == 1 is legal.
 */
#ifndef TWL_GUIDE_H
#define TWL_GUIDE_H

#include "twl_align.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TWL_GUIDE_MAX_SEQS 16384      /* the matrix of shared counts is 1 GiB then */

/* 4096 for 'n', 7776 for 'p', TWL_ERR_BAD_ARGUMENT for any other type.  Needs no device. */
int twl_guide_bins(char type);

/* The geometry of the two kernels, for tests that sit on their edges (no device needed): out[0] = windows a thread of the count kernel
   takes in a row, out[1] = windows its workgroup takes per round, out[2] = edge of the square tile of pairs of the all-pairs kernel,
   out[3] = bins of a staged slice (the bins are padded with zeros to a multiple of it).  Returns 4, the number of values. */
int twl_guide_describe(int32_t out[4]);

/* counts_out[i][b] = c_i[b], b < twl_guide_bins(type).  Diagnostics and tests. */
int twl_guide_kmer_counts(int device, char type, int32_t n, const char *const *seqs, const int32_t *lens, uint16_t *counts_out);

/* shared_out[i][j] = S(i, j): n x n, symmetric, w_i on the diagonal. */
int twl_guide_shared(int device, char type, int32_t n, const char *const *seqs, const int32_t *lens, uint32_t *shared_out);

/* Milliseconds of the last twl_guide_shared of this device: upload + count kernel, all-pairs kernel, download. */
int twl_guide_timing(int device, double *count_ms, double *pairs_ms, double *download_ms);

/*
 * The two-stage tree (`--tree-seeds S`): a set keeps the counts c_i and the sums w_i of up to TWL_GUIDE_SET_MAX_SEQS
 * sequences on the device, and the calls below work on it; no matrix over the whole set is ever formed.  Sequences are named by their
 * index in the call that made the set.  Refused before any device work, each with a text of its own: what twl_guide_shared refuses (with the
 * larger cap), a NULL set or pointer, n_seeds outside 1 .. TWL_GUIDE_MAX_SEQS, a seed or sequence id outside the set, the same seed twice,
 * no group, an empty group, a group of more than TWL_GUIDE_MAX_SEQS sequences, group offsets that do not start at 0 or that decrease, and
 * groups whose matrices hold more than 2^28 entries together (the 1 GiB of twl_guide_shared's largest matrix).
 */
#define TWL_GUIDE_SET_MAX_SEQS 1048576

typedef struct twl_guide_set twl_guide_set;

/* Uploads the sequences and counts their k-mers.  Panels that do not fit the device's free memory: TWL_ERR_HIP, the text says "out of device memory". */
int twl_guide_set_create(int device, char type, int32_t n, const char *const *seqs, const int32_t *lens, twl_guide_set **set);
int twl_guide_set_destroy(twl_guide_set *set);

/* w_out[i] = w_i, i < n. */
int twl_guide_set_weights(twl_guide_set *set, uint32_t *w_out);

/* seed_out[i] = the index t into seed_ids of the seed sequence i goes to, shared_out[i] = S(i, seed_ids[t]) (shared_out may be NULL).
   A sequence that is a seed goes to itself; every other one to the t with the largest S(i, seed_ids[t]) / min(w_i, w_seed), taken as 0 / 1
   where that minimum is 0, compared exactly (by cross-multiplying in 64-bit integers), the smaller t among equals. */
int twl_guide_set_assign(twl_guide_set *set, int32_t n_seeds, const int32_t *seed_ids, int32_t *seed_out, uint32_t *shared_out);

/* The S-matrix of every group in one launch: the rows of group g are ids[group_off[g] .. group_off[g + 1]), m_g of them, and its block
   (m_g x m_g, row-major, symmetric, w on the diagonal) starts at out[sum of m_h^2 over h < g].  group_off has n_groups + 1 entries. */
int twl_guide_set_shared_groups(twl_guide_set *set, int32_t n_groups, const int32_t *group_off, const int32_t *ids, uint32_t *out);

/* Milliseconds spent on this set since it was made: upload + count kernel, assign kernels, group kernels, and all downloads. */
int twl_guide_set_timing(twl_guide_set *set, double *count_ms, double *assign_ms, double *groups_ms, double *download_ms);

#ifdef __cplusplus
}
#endif
#endif /* TWL_GUIDE_H */
