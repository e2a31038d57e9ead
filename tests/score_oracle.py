"""Oracle of the affine sum-of-pairs score of include/twl_score.h, stated naively and stated twice (numpy / pure Python, no device).

(a) walk: per ordered pair (i, j) the projection is built as a string ('L' where row i holds a letter, '-' where only row j does, the columns
    where neither does left out) and its stretches of '-' are the gap runs of i against j; a stretch that touches the string's first or last
    position is terminal (once, also when it touches both).
(b) carry: the rows as Python integers, bit c = the row holds a letter at column c; with X = B & ~A the runs of i against j are
    popcount((X + ~A) & A) + the carry out of the top bit, whatever the number of bits >= W the integers are given.
    G, RT and GT of (b) come from column counts, first / last letter columns and prefix sums, not from pairs.

sub, the class counts and the score are stated once each.  Only the byte 0x2D is a gap."""
import re

import numpy as np

GAP = 0x2D
NUC = b"ACGT"
PROT = b"ACDEFGHIKLMNPQRSTVWY"
TOTALS = ("R", "G", "RT", "GT", "letters")


def classes(seq_type):
    return {"n": 4, "p": 20}[seq_type]


def class_of(byte, seq_type):
    """0 .. K - 1 a letter of the alphabet (either case, U = T), K every other byte that is no gap, None the gap."""
    if byte == GAP:
        return None
    ch = bytes([byte]).upper()
    if seq_type == "n":
        ch = b"T" if ch == b"U" else ch
        at = NUC.find(ch)
    else:
        at = PROT.find(ch)
    return at if at >= 0 and ch.isalpha() else classes(seq_type)


def class_counts(rows, seq_type):
    """cnt[c][a], a <= K."""
    K = classes(seq_type)
    lut = np.full(256, K + 1, dtype=np.int64)
    for b in range(256):
        cl = class_of(b, seq_type)
        if cl is not None:
            lut[b] = cl
    m = lut[np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), -1)]
    return np.stack([(m == a).sum(axis=0) for a in range(K + 1)], axis=1).astype(object)


def sub_table(rows, seq_type):
    """sub[a][b] for a <= b <= K (zero below the diagonal), Python integers."""
    K = classes(seq_type)
    cnt = class_counts(rows, seq_type)
    sub = np.zeros((K + 1, K + 1), dtype=object)
    for a in range(K + 1):
        for b in range(a, K + 1):
            sub[a, b] = int(sum(int(x) * (int(x) - 1) // 2 for x in cnt[:, a])) if a == b else int(sum(int(x) * int(y) for x, y in zip(cnt[:, a], cnt[:, b])))
    return sub


def present(rows):
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), -1) != GAP


# ---- (a) the walk ----
def projection(pi, pj):
    """pi, pj: the present masks of rows i and j."""
    keep = pi | pj
    return np.where(pi[keep], ord("L"), GAP).astype(np.uint8).tobytes()


def walk_pair(pi, pj):
    """(runs, gap columns, terminal runs, terminal gap columns) of row i against row j."""
    s = projection(pi, pj)
    runs = cols = truns = tcols = 0
    for m in re.finditer(rb"-+", s):
        runs += 1
        cols += m.end() - m.start()
        if m.start() == 0 or m.end() == len(s):
            truns += 1
            tcols += m.end() - m.start()
    return runs, cols, truns, tcols


def walk_all(rows, pairs=None):
    """runs_row and the totals R, G, RT, GT by the walk, over all ordered pairs or over the listed ones."""
    p = present(rows)
    n = len(rows)
    runs_row = [0] * n
    tot = dict(R=0, G=0, RT=0, GT=0)
    for i, j in (pairs if pairs is not None else ((i, j) for i in range(n) for j in range(n) if i != j)):
        r, g, rt, gt = walk_pair(p[i], p[j])
        runs_row[i] += r
        tot["R"] += r; tot["G"] += g; tot["RT"] += rt; tot["GT"] += gt
    return runs_row, tot


# ---- (b) the carry ----
def as_integers(rows):
    return [int.from_bytes(np.packbits(m, bitorder="little").tobytes(), "little") for m in present(rows)]


def carry_pair(A, B, bits):
    """Runs of the row A against the row B, both integers of `bits` bits."""
    mask = (1 << bits) - 1
    X = B & ~A & mask
    S = X + (~A & mask)
    return bin(S & A).count("1") + (S >> bits)


def carry_runs_row(rows, bits=None, pairs=None):
    ints = as_integers(rows)
    bits = len(rows[0]) if bits is None else bits
    n = len(rows)
    runs_row = [0] * n
    for i, j in (pairs if pairs is not None else ((i, j) for i in range(n) for j in range(n) if i != j)):
        runs_row[i] += carry_pair(ints[i], ints[j], bits)
    return runs_row


def column_totals(rows):
    """G, RT, GT and the letters from let[], first / last and prefix sums."""
    p = present(rows)
    n, W = p.shape
    let = p.sum(axis=0).astype(object)
    G = int(sum(int(l) * (n - int(l)) for l in let))
    pre = [0]
    for l in let:
        pre.append(pre[-1] + int(l))
    first = [int(np.argmax(r)) if r.any() else W for r in p]
    last = [W - 1 - int(np.argmax(r[::-1])) if r.any() else -1 for r in p]
    RT = GT = 0
    lettered = [k for k in range(n) if first[k] < W]
    for i in range(n):
        if first[i] >= W:
            RT += len(lettered); GT += pre[W]
            continue
        RT += sum(1 for j in lettered if first[j] < first[i]) + sum(1 for j in lettered if last[j] > last[i])
        GT += pre[first[i]] + pre[W] - pre[last[i] + 1]
    return dict(G=G, RT=RT, GT=GT, letters=pre[W])


def expected(rows, seq_type):
    """What twl_store_score_rows returns: (sub, runs_row, totals) by statement (b)."""
    runs_row = carry_runs_row(rows)
    tot = column_totals(rows)
    tot["R"] = sum(runs_row)
    return sub_table(rows, seq_type), runs_row, tot


# ---- the score ----
def nucleotide_matrix(match=18.0, mismatch=-8.0, transition=-4.0):
    """s(a, b) of the default nucleotide scoring: A C G T as 0 .. 3, a transition is |a - b| = 2."""
    return [[match if a == b else transition if abs(a - b) == 2 else mismatch for b in range(4)] for a in range(4)]


def score(sub, tot, s, gap_open, gap_extend, gap_ends, K):
    """In double from exact integers, in the order of the definition."""
    S = 0.0
    for a in range(K):
        for b in range(a, K):
            S += float(int(sub[a][b])) * float(s[a][b])
    S += float(gap_open) * float(tot["R"] - tot["RT"])
    S += float(gap_extend) * float((tot["G"] - tot["GT"]) - (tot["R"] - tot["RT"]))
    S += float(gap_ends) * float(tot["GT"])
    return S


def read_fasta(path):
    names, rows = [], []
    for line in open(path, "rb").read().split(b"\n"):
        if line.startswith(b">"):
            names.append(line[1:].split()[0].decode() if line[1:].split() else ""); rows.append(b"")
        elif names:
            rows[-1] += line.strip()
    return names, rows
