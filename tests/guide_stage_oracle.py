"""The two-stage guide tree of `--tree-seeds S`, restated in numpy and Python integers from its definition.
Counts, shared counts and distances are those of tests/guide_oracle.py, imported unchanged; the naive UPGMA is restated here once more,
because the graft needs the height of every cluster's root.  Independent of the C++ and of the kernels."""
import numpy as np

import guide_oracle as O


def seed_ids(n, s):
    """Step 1: seed t is sequence floor(t * n / s) (Python integers do not wrap)."""
    assert 2 <= s <= min(n, 16384)
    return [t * n // s for t in range(s)]


def shared_with(row, panel):
    """S(i, j) for the rows j of `panel`, as int64, from the counts `row` of sequence i.  Only the bins sequence i has can add to a minimum."""
    nz = np.flatnonzero(row)
    return np.minimum(row[nz].astype(np.int64)[None, :], panel[:, nz].astype(np.int64)).sum(axis=1)


def better(sa, ma, ta, sb, mb, tb):
    """The ratio sa / ma is larger than sb / mb, by cross-multiplying in Python integers; equal ratios: the smaller t."""
    l, r = sa * mb, sb * ma
    assert l < 2 ** 64 and r < 2 ** 64
    return l > r or (l == r and ta < tb)


def best_seed(s, m):
    """The t that is `better` than every other one, for the shared counts s[t] and the minima m[t] of one sequence (int64 arrays; the
    products stay below 2^58).  The candidates are walked in ascending t: a later one replaces the best so far only with a strictly larger
    ratio, so equal ratios stay with the smaller t."""
    s = np.where(m > 0, s, 0)
    m = np.where(m > 0, m, 1)
    assert int(s.max()) < 2 ** 29 and int(m.max()) < 2 ** 29
    best = 0
    while True:
        ahead = np.flatnonzero(s[best + 1:] * m[best] > s[best] * m[best + 1:])
        if len(ahead) == 0:
            return best
        best += 1 + int(ahead[0])


def assign(counts, seeds):
    """Step 2: (seed index of every sequence, S(i, its seed)).  `seeds` may be in any order; t is the position in it."""
    w = counts.astype(np.int64).sum(axis=1)
    where = {s: t for t, s in enumerate(seeds)}
    assert len(where) == len(seeds)
    panel = counts[np.asarray(seeds)]
    w_seed = w[np.asarray(seeds)]
    out, shared = [], []
    for i in range(len(counts)):
        s = shared_with(counts[i], panel)
        t = where[i] if i in where else best_seed(s, np.minimum(w[i], w_seed))
        out.append(t)
        shared.append(int(s[t]))
    return out, shared


def clusters(n_seeds, seed_of):
    """Step 3: K_t in input order."""
    k = [[] for _ in range(n_seeds)]
    for i, t in enumerate(seed_of):
        k[t].append(i)
    return k


def _length(parent, child):
    v = parent - child
    return "%.6f" % (0.0 if v < 0 else v)


def upgma(texts, heights, d):
    """The naive UPGMA of section 4f on leaves that already have a text and a height: (text without ';', root height).  With names and zero
    heights it is guide_oracle.upgma_newick."""
    d = np.array(d, dtype=np.float64)
    n = len(texts)
    text, height, size = list(texts), [float(h) for h in heights], [1] * n
    live = list(range(n))
    for _ in range(n - 1):
        idx = np.array(live)
        sub = d[np.ix_(idx, idx)].copy()
        sub[np.tril_indices(len(idx))] = np.inf
        x, y = divmod(int(np.argmin(sub)), len(idx))      # the first of equals in row-major order: the smaller a, then the smaller b
        a, b, h = int(idx[x]), int(idx[y]), sub[x, y] / 2
        text[a] = "(%s:%s,%s:%s)" % (text[a], _length(h, height[a]), text[b], _length(h, height[b]))
        na, nb = np.float64(size[a]), np.float64(size[b])
        live.remove(b)
        rest = np.array([c for c in live if c != a], dtype=np.int64)
        d[a, rest] = d[rest, a] = (na * d[a, rest] + nb * d[b, rest]) / (na + nb)      # two products, a sum and a quotient, each rounded once
        size[a] += size[b]
        height[a] = h
    return text[live[0]], height[live[0]]


def _tree_of_members(names, counts, members):
    """Steps 4 and 5 for one set of rows: the section 4f tree of these sequences in this order."""
    c = counts[np.asarray(members)]
    c = c[:, np.flatnonzero(c.any(axis=0))]      # bins no member has add 0 to every minimum
    d = O.distances(O.shared_counts(c))
    return upgma([names[i] for i in members], [0.0] * len(members), d)


def tree_from_counts(names, counts, s):
    n = len(names)
    seeds = seed_ids(n, s)
    seed_of, _ = assign(counts, seeds)
    k = clusters(s, seed_of)
    assert max(len(x) for x in k) <= 16384
    parts = [_tree_of_members(names, counts, members) for members in k]
    c = counts[np.asarray(seeds)]
    d = O.distances(O.shared_counts(c[:, np.flatnonzero(c.any(axis=0))]))
    text, _ = upgma([p[0] for p in parts], [p[1] for p in parts], d)      # step 6: V with leaf t standing at h_t
    return text + ";\n", k


def tree_of(names, seqs, type_, s):
    """The text of the two-stage tree."""
    return tree_from_counts(names, O.counts_matrix(seqs, type_), s)[0]


def cluster_sizes(seqs, type_, s):
    counts = O.counts_matrix(seqs, type_)
    return [len(x) for x in clusters(s, assign(counts, seed_ids(len(seqs), s))[0])]
