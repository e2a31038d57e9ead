"""Directed inputs of the comparison (include/twl_compare.h), each with the branch of the kernels it is for.  Shapes come from the constants of
twl_compare_describe: T counters per key window, TILE columns of a column tile, STEP rows per step of the column kernel, CHUNK columns per scan
round.  A case is (name, branch, E rows, R rows); build() makes the two alignments from residues given as (E column, R column) per row."""
import collections

import numpy as np

Case = collections.namedtuple("Case", "name branch est ref")
LETTERS = b"ACGT"


def build(rows, We, Wr, letters=None):
    """rows[k]: the residues of row k as (E column, R column), ascending in both.  Letter i of row k is letters[k][i] (default: a fixed cycle)."""
    E, R = [], []
    for k, res in enumerate(rows):
        e, r = bytearray(b"-" * We), bytearray(b"-" * Wr)
        for i, (c, b) in enumerate(res):
            ch = letters[k][i] if letters else LETTERS[(k + i) % 4]
            assert e[c] == 0x2D and r[b] == 0x2D and (i == 0 or (c > res[i - 1][0] and b > res[i - 1][1]))
            e[c], r[b] = ch, ch
        E.append(bytes(e)); R.append(bytes(r))
    return E, R


def span_cases(T):
    """One E column whose keys span T - 1 .. 2T + 1 reference columns, duplicates at both ends, so that the first and the last window both add pairs."""
    out = []
    for span in (T - 2, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1):
        lo, Wr = 3, 2 * T + 8
        keys = [lo, lo, lo + 1, lo + span // 2, lo + span, lo + span, lo + span]
        E, R = build([[(1, b)] for b in keys], 3, Wr)
        out.append(Case(f"largest key - smallest key = {span}", f"{span // T + 1} window(s); keys on both ends", E, R))
    lo = 5
    keys = [lo] + [lo + T - 1] * 3 + [lo + T] * 3
    E, R = build([[(0, b)] for b in keys], 1, lo + T + 1)
    out.append(Case("equal counts on keys lo + T - 1 and lo + T", "the last counter of a window and the first of the next", E, R))
    return out


def row_count_cases(STEP):
    out = []
    for n in sorted({2, 63, 64, 65, 255, 256, 257, STEP - 1, STEP, STEP + 1} - {0, 1}):
        E, R = build([[(0, 0)] for _ in range(n)], 1, 1)
        out.append(Case(f"n = {n}, all keys equal", "shared = C(n, 2), recovered", E, R))
        E, R = build([[(0, k)] for k in range(n)], 1, n)
        out.append(Case(f"n = {n}, all keys distinct", "shared = 0, distinct = n", E, R))
    return out


def random_rows(rng, n, We, Wr, empty_rows=0.0, full_rows=0.0):
    """The residues of n rows with random letter counts; the letters sit at random columns of E and, independently, of R."""
    L = min(We, Wr)
    rows = []
    for _ in range(n):
        u = rng.random()
        m = 0 if u < empty_rows else L if u < empty_rows + full_rows else int(rng.integers(0, L + 1))
        c = np.sort(rng.choice(We, m, replace=False))
        b = np.sort(rng.choice(Wr, m, replace=False))
        rows.append(list(zip(c.tolist(), b.tolist())))
    return rows


def random_pair(rng, n, We, Wr, empty_rows=0.0, full_rows=0.0):
    return build(random_rows(rng, n, We, Wr, empty_rows, full_rows), We, Wr)


def width_cases(TILE, CHUNK, seed=11):
    rng = np.random.default_rng(seed)
    out = []
    for W in sorted({1, 15, 17, 63, 64, 65, TILE - 1, TILE, TILE + 1, CHUNK - 1, CHUNK, CHUNK + 1}):
        for We, Wr in ((W, W + 3), (W + 5, W)):
            E, R = random_pair(rng, 5, We, Wr, empty_rows=0.2, full_rows=0.2)
            out.append(Case(f"We = {We}, Wr = {Wr}", "a width one below, on, one above a tile / a scan round; not a multiple of 16", E, R))
    return out


def scan_cases(TILE, CHUNK):
    out = []
    W = 3 * CHUNK
    strad = [(CHUNK - 2 + i, 2 * CHUNK - 3 + i) for i in range(5)]             # letters on both sides of a round boundary, in E and in R
    holes = [(i, CHUNK + i) for i in range(3)] + [(2 * CHUNK + i, 2 * CHUNK + 7 + i) for i in range(3)]      # E's second round is all gaps, R's first
    E, R = build([strad, holes, strad, holes], W, W)
    out.append(Case("letters straddle a scan round; gaps fill a whole round", "the carry crosses a round with and without letters in it", E, R))
    We = 3 * TILE
    rows = [[(c, c) for c in list(range(0, TILE, 3)) + list(range(2 * TILE, 3 * TILE, 2))] for _ in range(3)]
    rows.append([])                                                             # a row without letters
    E, R = build(rows, We, We)
    out.append(Case("a whole tile of gaps, columns of gaps, rows without letters", "a tile that ends after the first sweep", E, R))
    full = [(c, c) for c in range(9)]
    E, R = build([full, full, [(0, 2), (4, 5)], []], 9, 9)
    out.append(Case("rows of letters only beside a row without letters", "no gap in a row; no letter in a row", E, R))
    E, R = build([[(0, 0), (2, 1)], [(0, 0), (2, 2)]], 3, 3, letters=[b"aC", b"Ac"])
    E[1] = E[1].swapcase()
    out.append(Case("a against A", "letters are compared after folding a-z to A-Z", E, R))
    return out


def big_cell_cases():
    """One cell holds every row: C(n, 2) passes 32 bits from n = 92 683, the product n (n - 1) from n = 65 537."""
    out = []
    for n, We, Wr in ((65537, 2, 3), (92700, 4, 2)):
        E, R = build([[(1, 1)]] * n, We, Wr)
        out.append(Case(f"{n} rows in one cell", "the 64-bit product and sum", E, R))
    return out


def moved_gaps_family(seed):
    """A reference of random rows and an estimate that is the reference with its gaps moved: most rows keep their columns, so that most E columns
    have their keys in one window, some rows are shifted far."""
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(2, 301)) if seed % 4 == 0 else int(rng.integers(2, 40))
    Wr = int(rng.integers(1, 3001)) if seed % 5 == 0 else int(rng.integers(1, 400))
    We = Wr + int(rng.integers(0, 1 + Wr // 4))
    rows = []
    for _ in range(n):
        m = int(rng.integers(0, Wr + 1)) if rng.random() < 0.9 else 0
        b = np.sort(rng.choice(Wr, m, replace=False))
        if rng.random() < 0.6:
            c = b + (We - Wr if rng.random() < 0.3 else 0)                      # the same columns, or all shifted to the right end
        else:
            c = np.sort(rng.choice(We, m, replace=False))
        rows.append(list(zip(c.tolist(), b.tolist())))
    return build(rows, We, Wr)


def known_answer():
    return [b"ACG-T", b"ACCGT", b"-A-GT"], [b"AC-GT", b"ACCGT", b"A--GT"]
