"""The guide tree rebuilt from an alignment in two stages (`--iterations K --retree-seeds S`), restated in numpy and exact integers from its
definition.  The letter table, the mask's threshold and the distances are those of tests/retree_oracle.py,
the seeds, the clusters and the UPGMA with grafted heights those of tests/guide_stage_oracle.py, all imported unchanged.  The mask is computed
once over ALL rows and sliced: retree_oracle.pair_counts would compute it anew from the rows it is handed, which is wrong for one cluster.
Independent of the C++ and of the kernels."""
import numpy as np

import guide_stage_oracle as G
import retree_oracle as R


def codes(rows, type_, mg):
    """int64 [n][kept]: the letter codes of the kept columns (-1: no letter), the mask taken over all rows.  `rows` is a list of bytes or a
    uint8 array [n][width]."""
    a = rows if isinstance(rows, np.ndarray) else R.matrix(rows)
    keep = (a == ord("-")).sum(axis=0) <= mg
    return R.letter_table(type_)[a][:, keep]


def counts_with(code, panel):
    """(match, both) int64 [n][len(panel)]: the counts of every row of `code` with every row of `panel`."""
    n, s = len(code), len(panel)
    match = np.zeros((n, s), dtype=np.int64)
    both = np.zeros((n, s), dtype=np.int64)
    valid = code >= 0
    for t in range(s):
        b = valid & (panel[t] >= 0)[None, :]
        both[:, t] = b.sum(axis=1)
        match[:, t] = (b & (code == panel[t][None, :])).sum(axis=1)
    return match, both


def assign(rows, type_, mg, seeds):
    """Step 3: (seed_of, match, both) per row: the position t in `seeds` (which may be in any order) and the two counts with that seed; for a
    row that is a seed, its own t and its letters twice.  The seeds are walked in ascending t, and a later one replaces the best so far only
    on a strictly larger cross-product, so equal ratios stay with the smaller t; both == 0 counts as 0 / 1."""
    code = codes(rows, type_, mg)
    n = len(code)
    seeds = [int(s) for s in seeds]
    assert len(set(seeds)) == len(seeds) and code.shape[1] < 2 ** 31      # (the products below stay under 2^62: exact in int64)
    match, both = counts_with(code, code[np.asarray(seeds)])
    bm, bb, bt = np.zeros(n, dtype=np.int64), np.ones(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for t in range(len(seeds)):
        m = np.where(both[:, t] > 0, match[:, t], 0)
        b = np.where(both[:, t] > 0, both[:, t], 1)
        ahead = (m * bb > bm * b) if t else np.ones(n, dtype=bool)
        bm, bb, bt = np.where(ahead, m, bm), np.where(ahead, b, bb), np.where(ahead, t, bt)
    rows_ix = np.arange(n)
    out_m, out_b = match[rows_ix, bt], both[rows_ix, bt]
    letters = (code >= 0).sum(axis=1)
    for t, s in enumerate(seeds):
        bt[s], out_m[s], out_b[s] = t, letters[s], letters[s]
    return bt.astype(np.int32), out_m.astype(np.uint32), out_b.astype(np.uint32)


def pair_counts(code):
    """(match, both) uint32 [m][m] of the rows of `code` (already masked)."""
    match, both = counts_with(code, code)
    return match.astype(np.uint32), both.astype(np.uint32)


def _tree_of_members(names, code, members):
    """Step 5 for one set of rows: the section 4h tree of these rows in this order, as (text without ';', root height)."""
    match, both = pair_counts(code[np.asarray(members)])
    return G.upgma([names[i] for i in members], [0.0] * len(members), R.distances(match, both))


def tree_of(names, rows, type_, s, T=0.95):
    """(text of the two-stage tree, clusters)."""
    n = len(names)
    mg = R.max_gaps(T, n)
    code = codes(rows, type_, mg)
    seeds = G.seed_ids(n, s)
    seed_of, _, _ = assign(rows, type_, mg, seeds)
    k = G.clusters(s, [int(t) for t in seed_of])
    assert max(len(x) for x in k) <= 16384
    parts = [_tree_of_members(names, code, members) for members in k]
    match, both = pair_counts(code[np.asarray(seeds)])
    text, _ = G.upgma([p[0] for p in parts], [p[1] for p in parts], R.distances(match, both))
    return text + ";\n", k
