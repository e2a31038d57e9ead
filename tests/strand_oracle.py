"""`--adjust-direction` restated in numpy from its definition, over guide_oracle.py: rc(b), the opposite-strand counts O,
the seeds' directions as a maximum spanning tree in its naive O(S^3) form, the assignment of every sequence, the reverse complement of a
record's text and the default number of seeds.  Independent of the C++: tests compare the library, the host code and the command line with it."""
import numpy as np

import guide_oracle as G

_PAIRS = "AT CG RY KM BV DH"


def rc_bin(b):
    """The code of the reverse complement of the 6-mer with code b: its base-4 digits in reverse order, every digit d replaced by 3 - d."""
    if not 0 <= b <= 4095:
        return -1
    digits = [(b // 4 ** k) % 4 for k in range(6)]      # last letter first
    return sum((3 - d) * 4 ** (5 - k) for k, d in enumerate(digits))


def perm():
    """perm[b] = rc(b): counts(rc(seq)) == counts(seq)[perm]."""
    return np.array([rc_bin(b) for b in range(4096)], dtype=np.int64)


def reverse_complement(seq):
    """bytes -> bytes: reversed, complemented over the IUPAC table, case kept; A <-> U in a record that holds a U/u and no T/t."""
    text = bytes(seq).decode("latin-1")
    rna = ("U" in text.upper()) and ("T" not in text.upper())
    table = {}
    for a, b in _PAIRS.split():
        for x, y in ((a, b), (b, a)):
            table[x] = y
            table[x.lower()] = y.lower()
    if rna:
        table.update({"A": "U", "a": "u", "U": "A", "u": "a"})
    return "".join(table.get(c, c) for c in reversed(text)).encode("latin-1")


def default_seeds(total, cap):
    """The smallest S with S * S >= 4 * total, clipped to [1, min(cap, 16384)]."""
    s = 1
    while s * s < 4 * total:
        s += 1
    return max(1, min(s, cap, 16384))


def seed_ids(n, s):
    return [t * n // s for t in range(s)]


def cross_counts(ca, cb):
    """sum_b min(ca[i][b], cb[j][b]) as int64 [len(ca)][len(cb)]."""
    a, b = ca.astype(np.int64), cb.astype(np.int64)
    out = np.zeros((len(a), len(b)), dtype=np.int64)
    for i in range(len(a)):
        out[i] = np.minimum(a[i][None, :], b).sum(axis=1)
    return out


def opposite_counts(counts):
    """O[i][j] = sum_b min(c_i[b], c_j[rc(b)]) as uint32 [n][n]."""
    return cross_counts(counts, counts[:, perm()]).astype(np.uint32)


def _ratio(s, m):
    return (0, 1) if m == 0 else (int(s), int(m))


def _larger(a, b):
    """a, b = (num, den): -1 when a is the larger ratio, 1 when b is, 0 when equal; exact."""
    l, r = a[0] * b[1], b[0] * a[1]
    return -1 if l > r else (1 if l < r else 0)


def seed_flips(F, R):
    """Prim from seed 0, every step over all links (u outside, v inside, kind): the first in the order larger ratio, kind 0, smaller v, smaller u."""
    S = len(F)
    w = [int(F[t][t]) for t in range(S)]
    flip = [0] * S
    inside = [0]
    while len(inside) < S:
        best = None
        for u in range(S):
            if u in inside:
                continue
            for v in inside:
                for kind in (0, 1):
                    x = (_ratio((R if kind else F)[u][v], min(w[u], w[v])), kind, v, u)
                    if best is None:
                        best = x
                        continue
                    c = _larger(x[0], best[0])
                    if c < 0 or (c == 0 and x[1:] < best[1:]):
                        best = x
        _, kind, v, u = best
        flip[u] = flip[v] ^ kind
        inside.append(u)
    return np.array(flip, dtype=np.uint8)


def assign(counts, seeds, flip):
    """(t, d, s) of every row of `counts`: the first candidate (t, r) in the order larger s / m, smaller t, smaller d = r ^ flip[t]; a seed goes to
    itself with d = flip[t] and s = w."""
    c = counts.astype(np.int64)
    w = c.sum(axis=1)
    sc = counts[list(seeds)]
    Sf = cross_counts(counts, sc)
    So = cross_counts(counts, sc[:, perm()])
    pos = {int(i): t for t, i in enumerate(seeds)}
    n = len(c)
    t_out, d_out, s_out = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint32)
    for i in range(n):
        if i in pos:
            t_out[i], d_out[i], s_out[i] = pos[i], flip[pos[i]], w[i]
            continue
        best = None
        for t, j in enumerate(seeds):
            m = min(w[i], w[j])
            for r in (0, 1):
                s = int((So if r else Sf)[i][t])
                x = (_ratio(s, m), t, r ^ int(flip[t]), 0 if m == 0 else s)
                if best is None:
                    best = x
                    continue
                k = _larger(x[0], best[0])
                if k < 0 or (k == 0 and x[1:3] < best[1:3]):
                    best = x
        t_out[i], d_out[i], s_out[i] = best[1], best[2], best[3]
    return t_out, d_out, s_out


def directions(seqs, n_seeds=None):
    """The direction (0 forward, 1 reversed) of every sequence of a run without -a."""
    counts = G.counts_matrix(seqs, "n")
    n = len(seqs)
    S = n_seeds or default_seeds(n, n)
    seeds = seed_ids(n, S)
    sc = counts[seeds]
    F = cross_counts(sc, sc)
    R = cross_counts(sc, sc[:, perm()])
    return assign(counts, seeds, seed_flips(F, R))[1]


def directions_on_backbone(backbone, seqs, n_seeds=None):
    """With -a: the set is the backbone's degapped rows and then the new sequences; the seeds are backbone rows, all forward.  The directions of
    the new sequences."""
    B = len(backbone)
    counts = G.counts_matrix(list(backbone) + list(seqs), "n")
    S = n_seeds or default_seeds(B + len(seqs), B)
    return assign(counts, seed_ids(B, S), np.zeros(S, dtype=np.uint8))[1][B:]


def plant(seqs):
    """Every record i with i % 3 == 1 reverse-complemented: (the planted records, the planted directions)."""
    return [reverse_complement(s) if i % 3 == 1 else s for i, s in enumerate(seqs)], np.array([1 if i % 3 == 1 else 0 for i in range(len(seqs))], dtype=np.uint8)
