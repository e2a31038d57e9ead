"""Small inputs of placement along a tree (-t -a -i --place-on-tree) for tests/test_place_tree_oracle_cpu.py and tests/test_gpu_place_tree.py:
a tree over old and new names, a backbone alignment of the old ones (rows of one length, with columns that are all '-' inside some groups)
and the new sequences.  Everything is derived from fixed seeds."""
import os

import numpy as np

NUC, AMINO = b"ACGT", b"ACDEFGHIKLMNPQRSTVWY"


def _mutate(rng, seq, letters, rate):
    out = bytearray()
    for c in seq:
        r = rng.random()
        if r < rate / 3:
            continue                                              # deletion
        out.append(letters[rng.integers(len(letters))] if r < rate else c)
        if rng.random() < rate / 3:
            out.append(letters[rng.integers(len(letters))])       # insertion
    return bytes(out)


def _newick(rng, names):
    """A random binary tree over `names`, with branch lengths."""
    parts = ["%s:%.3f" % (n, 0.05 + 0.4 * rng.random()) for n in names]
    while len(parts) > 1:
        i = int(rng.integers(len(parts) - 1))
        a, b = parts.pop(i), parts.pop(i)
        parts.insert(i, "(%s,%s):%.3f" % (a, b, 0.02 + 0.3 * rng.random()))
    return parts[0].rsplit(":", 1)[0] + ";"


def _backbone_rows(rng, seqs, width):
    """Rows of `width` columns: every sequence's letters in order at random columns, '-' elsewhere (any rows of one length are a backbone)."""
    rows = []
    for s in seqs:
        assert len(s) <= width
        cols = np.sort(rng.choice(width, size=len(s), replace=False))
        row = bytearray(b"-" * width)
        for c, ch in zip(cols, s):
            row[c] = ch
        rows.append(bytes(row))
    return rows


def _write(d, stem, tree, old, rows, new):
    t, a, i = (os.path.join(d, stem + ext) for ext in (".nwk", ".backbone.aln", ".new.fa"))
    open(t, "w").write(tree + "\n")
    with open(a, "wb") as f:
        for n, r in zip(old, rows):
            f.write(b">" + n.encode() + b"\n" + r + b"\n")
    with open(i, "wb") as f:
        for n, s in new:
            f.write(b">" + n.encode() + b"\n" + s + b"\n")
    return t, a, i


def family(d, stem, *, seq_type="n", n_old=8, n_new=4, length=48, width=60, seed=1, rate=0.12, new_last=False, ambiguous=()):
    """(tree, backbone, new sequences, type, {name: ungapped sequence}) of a family of n_old backbone rows of `width` columns and n_new new sequences.
    new_last: the new names end the tree's leaf list (they sit together) instead of being spread.  ambiguous: indices of new sequences that
    get every third letter replaced by N / X (over --max-ambig 0.1: low quality)."""
    rng = np.random.default_rng(seed)
    letters = NUC if seq_type == "n" else AMINO
    root = bytes(letters[k] for k in rng.integers(len(letters), size=length))
    old = ["old%02d" % k for k in range(n_old)]
    new = ["new%02d" % k for k in range(n_new)]
    seqs = {n: _mutate(rng, root, letters, rate)[: width] for n in old + new}
    for k in ambiguous:
        s = bytearray(seqs[new[k]])
        s[::3] = (b"N" if seq_type == "n" else b"X") * len(s[::3])
        seqs[new[k]] = bytes(s)
    names = list(old)
    for k, n in enumerate(new):
        names.insert(len(names) if new_last else min(len(names), 1 + k * (1 + n_old // max(1, n_new))), n)
    tree = _newick(rng, names)
    rows = _backbone_rows(rng, [seqs[n] for n in old], width)
    t, a, i = _write(d, stem, tree, old, rows, [(n, seqs[n]) for n in new])
    return t, a, i, seq_type, seqs


def hand_family(d):
    """A dozen sequences of 60 columns on a tree written by hand: the new leaves n1 .. n4 sit beside backbone leaves, inside a backbone clade and
    next to each other; the clade (b5, b6, b7) hangs under an unplaced node, so its rows form one group with the columns 10-19 all '-'."""
    tree = "(((b1:0.1,n1:0.2):0.1,(b2:0.1,b3:0.3):0.2):0.1,((n2:0.1,n3:0.2):0.1,b4:0.2):0.3,(((b5:0.1,b6:0.1):0.1,b7:0.2):0.1,(n4:0.3,b8:0.1):0.2):0.2);"
    rng = np.random.default_rng(42)
    root = bytes(NUC[k] for k in rng.integers(4, size=50))
    old = ["b%d" % k for k in range(1, 9)]
    new = ["n%d" % k for k in range(1, 5)]
    seqs = {n: _mutate(rng, root, NUC, 0.1)[:50] for n in old + new}
    rows = []
    for n in old:
        s = seqs[n][:40] if n in ("b5", "b6", "b7") else seqs[n]
        if n in ("b5", "b6", "b7"):
            seqs[n] = s
            cols = np.sort(rng.choice(np.r_[0:10, 20:60], size=len(s), replace=False))
        else:
            cols = np.sort(rng.choice(60, size=len(s), replace=False))
        row = bytearray(b"-" * 60)
        for c, ch in zip(cols, s):
            row[c] = ch
        rows.append(bytes(row))
    t, a, i = _write(d, "hand", tree, old, rows, [(n, seqs[n]) for n in new])
    return t, a, i, "n", seqs


def multifurcation(d):
    """A tree with a node of five children (two of them new) and a root of three, for --rooted: convert2binaryTree is not run, the schedule pairs
    the children of a node left to right."""
    tree = "((a1:0.1,x1:0.1,a2:0.2,x2:0.1,a3:0.3):0.2,(a4:0.1,a5:0.2):0.1,(x3:0.2,a6:0.1):0.3);"
    rng = np.random.default_rng(77)
    root = bytes(NUC[k] for k in rng.integers(4, size=40))
    old = ["a%d" % k for k in range(1, 7)]
    new = ["x%d" % k for k in range(1, 4)]
    seqs = {n: _mutate(rng, root, NUC, 0.1)[:48] for n in old + new}
    rows = _backbone_rows(rng, [seqs[n] for n in old], 48)
    t, a, i = _write(d, "multi", tree, old, rows, [(n, seqs[n]) for n in new])
    return t, a, i, "n", seqs
