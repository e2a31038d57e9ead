"""The guide tree of a run without -t, restated in numpy from its definition: k-mer counts, shared counts, distances,
the naive UPGMA and the Newick text.  Independent of the C++: tests compare the library, the host code and the command line with it."""
import gzip

import numpy as np

K = {"n": 6, "p": 5}
BASE = {"n": 4, "p": 6}
BINS = {"n": 4096, "p": 7776}
_CLASSES = {"n": ["A", "C", "G", "TU"], "p": ["AGPST", "C", "DENQ", "FWY", "HKR", "ILMV"]}


def letter_table(type_):
    """256 entries: the letter's number, -1 for an invalid byte; either case."""
    t = np.full(256, -1, dtype=np.int64)
    for v, letters in enumerate(_CLASSES[type_]):
        for ch in letters:
            t[ord(ch)] = v
            t[ord(ch.lower())] = v
    return t


def kmer_counts(seq, type_):
    """c[b]: windows of `seq` (bytes) with code b, saturated at 65535, as uint16 [bins]."""
    k, base = K[type_], BASE[type_]
    out = np.zeros(BINS[type_], dtype=np.int64)
    x = letter_table(type_)[np.frombuffer(bytes(seq), dtype=np.uint8)]
    if len(x) >= k:
        win = np.lib.stride_tricks.sliding_window_view(x, k)
        ok = (win >= 0).all(axis=1)
        code = (win[ok] * (base ** np.arange(k - 1, -1, -1))).sum(axis=1)
        out = np.bincount(code, minlength=BINS[type_])
    return np.minimum(out, 65535).astype(np.uint16)


def counts_matrix(seqs, type_):
    return np.stack([kmer_counts(s, type_) for s in seqs])


def shared_counts(counts):
    """S[i][j] = sum_b min(c_i[b], c_j[b]) as uint32 [n][n]; the diagonal is w."""
    c = counts.astype(np.int64)
    n = len(c)
    out = np.zeros((n, n), dtype=np.int64)
    for i in range(n):
        out[i] = np.minimum(c[i][None, :], c).sum(axis=1)
    assert out.max(initial=0) < 2 ** 32
    return out.astype(np.uint32)


def distances(shared):
    """d(i, j) = 1 - S / min(w_i, w_j) in double, 1 where the smaller w is 0, 0 on the diagonal."""
    s = shared.astype(np.float64)
    w = np.diag(shared).astype(np.float64)
    m = np.minimum(w[:, None], w[None, :])
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.where(m == 0, 1.0, 1.0 - s / m)
    np.fill_diagonal(d, 0.0)
    return d


def upgma_newick(names, d):
    """The naive algorithm, step by step, and its text."""
    d = np.array(d, dtype=np.float64)
    n = len(names)
    if n == 1:
        return names[0] + ";\n"
    live = list(range(n))
    size = [1] * n
    height = [0.0] * n
    text = list(names)

    def length(parent, child):
        v = parent - child
        return "%.6f" % (0.0 if v < 0 else v)

    for _ in range(n - 1):
        # the smallest d(a, b) over the live pairs a < b; argmin takes the first of equals in row-major order: the smaller a, then the smaller b
        idx = np.array(live)
        sub = d[np.ix_(idx, idx)].copy()
        sub[np.tril_indices(len(idx))] = np.inf
        x, y = divmod(int(np.argmin(sub)), len(idx))
        a, b, dab = int(idx[x]), int(idx[y]), sub[x, y]
        h = dab / 2
        text[a] = "(%s:%s,%s:%s)" % (text[a], length(h, height[a]), text[b], length(h, height[b]))
        na, nb = float(size[a]), float(size[b])
        live.remove(b)
        for c in live:
            if c != a:
                p1 = np.float64(na) * d[a, c]
                p2 = np.float64(nb) * d[b, c]
                d[a, c] = d[c, a] = (p1 + p2) / np.float64(na + nb)
        size[a] += size[b]
        height[a] = h
    return text[live[0]] + ";\n"


def read_fasta(path, limit=None):
    """(names, sequences as bytes): the first record of every name, the name up to the first blank, at most `limit` records."""
    names, seqs, seen = [], [], set()
    op = gzip.open if str(path).endswith(".gz") else open
    name, parts = None, []

    def flush():
        if name is not None and name not in seen:
            seen.add(name)
            names.append(name)
            seqs.append("".join(parts).encode())

    with op(path, "rt") as f:
        for line in f:
            line = line.rstrip("\r\n")
            if line.startswith(">"):
                flush()
                if limit is not None and len(names) >= limit:
                    name = None
                    break
                name, parts = line[1:].split(" ")[0].split("\t")[0], []
            elif name is not None:
                parts.append("".join(line.split()))
        flush()
    return names[:limit], seqs[:limit]


def tree_of(names, seqs, type_):
    return upgma_newick(names, distances(shared_counts(counts_matrix(seqs, type_))))
