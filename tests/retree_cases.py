"""Alignments for the tests of the rebuilt guide tree.

HAND: small alignments whose counts and trees were derived by hand; the expected values below are written out, not computed.
The rest builds the rows the GPU tests run: seeded rows over everything a row can hold, and directed rows, each with a check (on the CPU,
against the numpy restatement) that it is what it is listed for."""
import numpy as np

import retree_oracle as R

# ---- hand-derived ----
# 'n', 4 x 8, T = 0.5 -> max_gaps = 2.  Column 2 has exactly 2 gaps (kept), column 4 has 3 (dropped, with row r3's G in it); lower case;
# U against T in column 3; N against N in column 7 (no letter: not in both); C against c in column 6.
HAND_N = {
    "type": "n", "T": 0.5, "names": ["r0", "r1", "r2", "r3"],
    "rows": [b"ACGT--aN",
             b"ACGU--CN",
             b"AG-T-Ac-",
             b"-C-tGA--"],
    "max_gaps": 2,
    "gaps": [1, 0, 2, 0, 3, 2, 1, 2],
    "kept": [1, 1, 1, 1, 0, 1, 1, 1],
    "both": [[5, 5, 4, 2], [5, 5, 4, 2], [4, 4, 5, 3], [2, 2, 3, 3]],
    "match": [[5, 4, 2, 2], [4, 5, 3, 2], [2, 3, 5, 2], [2, 2, 2, 3]],
    # d01 = 0.2, d02 = 0.5, d12 = 0.25, d23 = 1/3, d03 = d13 = 0: the tie goes to the smaller a, (r0, r3) at height 0; then d(03, 1) = 0.1,
    # d(03, 2) = (0.5 + 1/3) / 2 = 0.416667: (03, 1) at 0.05; d(031, 2) = (2 * 0.416667 + 0.25) / 3 = 0.361111: height 0.180556
    "tree": "(((r0:0.000000,r3:0.000000):0.050000,r1:0.050000):0.130556,r2:0.180556);\n",
}
# the same rows with T = 1: max_gaps = 4 keeps column 4 too; only r3 holds a letter there, so only its diagonal entry grows
HAND_N_ALL = dict(HAND_N, T=1.0, max_gaps=4, kept=[1] * 8,
                  both=[[5, 5, 4, 2], [5, 5, 4, 2], [4, 4, 5, 3], [2, 2, 3, 4]], match=[[5, 4, 2, 2], [4, 5, 3, 2], [2, 3, 5, 2], [2, 2, 2, 4]])
# 'n', 3 x 6, T = 1: x and y share no column: both = 0, d = 1
HAND_DISJOINT = {
    "type": "n", "T": 1.0, "names": ["x", "y", "z"],
    "rows": [b"ACG---",
             b"---ACG",
             b"ACGACT"],
    "max_gaps": 3,
    "gaps": [1, 1, 1, 1, 1, 1],
    "kept": [1] * 6,
    "both": [[3, 0, 3], [0, 3, 3], [3, 3, 6]],
    "match": [[3, 0, 3], [0, 3, 2], [3, 2, 6]],
    # (x, z) at 0; d(xz, y) = (1 + 1/3) / 2 = 0.666667: height 0.333333
    "tree": "((x:0.000000,z:0.000000):0.333333,y:0.333333);\n",
}
# 'p', 3 x 6, T = 1: X, B, Z, *, U are no letters; lower case
HAND_P = {
    "type": "p", "T": 1.0, "names": ["p0", "p1", "p2"],
    "rows": [b"ACDX-w",
             b"acEBYW",
             b"AZD*YU"],
    "max_gaps": 3,
    "gaps": [0, 0, 0, 0, 1, 0],
    "kept": [1] * 6,
    "both": [[4, 4, 2], [4, 5, 3], [2, 3, 3]],
    "match": [[4, 3, 2], [3, 5, 2], [2, 2, 3]],
    # d01 = 0.25, d02 = 0, d12 = 1/3: (p0, p2) at 0; d(02, 1) = (0.25 + 1/3) / 2 = 0.291667: height 0.145833
    "tree": "((p0:0.000000,p2:0.000000):0.145833,p1:0.145833);\n",
}
HAND = {"n_mask": HAND_N, "n_all": HAND_N_ALL, "disjoint": HAND_DISJOINT, "protein": HAND_P}

# ---- rows for the device ----
ALPHABET = {"n": b"ACGTacgtUu" + b"ACGT" * 4 + b"----NnRYKM.", "p": b"ACDEFGHIKLMNPQRSTVWY" * 2 + b"acdefghiklmnpqrstvwy" + b"BZXJOU*----."}


def seeded_rows(type_, n, width, seed):
    """n rows of `width` bytes drawn from ALPHABET[type_]; every third column is drawn gappier, so that the mask drops some."""
    rng = np.random.default_rng(seed)
    pool = np.frombuffer(ALPHABET[type_], dtype=np.uint8)
    a = rng.choice(pool, (n, width))
    gappy = rng.random((n, width)) < np.where(np.arange(width) % 3 == 0, 0.6, 0.05)[None, :]
    a[gappy] = ord("-")
    return [r.tobytes() for r in a]


def directed_rows(width, slice_columns, seed):
    """(rows, facts) for type 'n': seeded filler rows followed by directed rows; `facts` names what each directed row or pair is listed for,
    as (kind, i, j) with indices into rows.  width > slice_columns + 1."""
    assert width > slice_columns + 1
    rows = seeded_rows("n", 9, width, seed)
    base = len(rows)
    rng = np.random.default_rng(seed + 1)
    ident = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), width).tobytes()
    half = width // 2
    left = ident[:half] + b"-" * (width - half)
    right = b"-" * half + ident[half:]
    only_last_a = b"A" * (width - 1) + b"G"
    only_last_b = b"C" * (width - 1) + b"g"
    first_of_slice_a = bytearray(b"A" * width)
    first_of_slice_b = bytearray(b"C" * width)
    first_of_slice_b[slice_columns] = ord("a")
    rows += [ident, ident, b"-" * width, b"N" * width, left, right, only_last_a, only_last_b, bytes(first_of_slice_a), bytes(first_of_slice_b)]
    facts = [("identical", base, base + 1), ("all_gap", base + 2, None), ("all_N", base + 3, None), ("no_common_column", base + 4, base + 5),
             ("match_only_in_last_column", base + 6, base + 7), ("match_only_in_first_column_of_a_slice", base + 8, base + 9)]
    return rows, facts


def check_directed(rows, facts, slice_columns):
    """Asserts, with the restatement and every column kept, that the directed rows are what they are listed for."""
    n, width = len(rows), len(rows[0])
    match, both, kept = R.pair_counts(rows, "n", n)
    assert kept == width
    a = R.matrix(rows)
    for kind, i, j in facts:
        if kind == "identical":
            assert rows[i] == rows[j] and match[i, j] == both[i, j] == width
        elif kind == "all_gap":
            assert (a[i] == ord("-")).all() and not both[i].any() and not both[:, i].any()
        elif kind == "all_N":
            assert (a[i] == ord("N")).all() and not both[i].any() and not both[:, i].any()
        elif kind == "no_common_column":
            assert both[i, j] == 0 and both[i, i] > 0 and both[j, j] > 0
        elif kind == "match_only_in_last_column":
            eq = (R.letter_table("n")[a[i]] == R.letter_table("n")[a[j]])
            assert match[i, j] == 1 and both[i, j] == width and eq[-1] and not eq[:-1].any()
        elif kind == "match_only_in_first_column_of_a_slice":
            eq = (R.letter_table("n")[a[i]] == R.letter_table("n")[a[j]])
            assert match[i, j] == 1 and both[i, j] == width and np.flatnonzero(eq).tolist() == [slice_columns]
        else:
            raise AssertionError(kind)


def masked_match_rows(n_fill, width, seed):
    """(rows, i, j, column, gaps_there): two rows whose only equal letters stand in `column`, where exactly gaps_there of the other rows hold
    '-' and no other column holds more than 1: with max_gaps = gaps_there the pair's match is 1, with max_gaps = gaps_there - 1 it is 0 (the
    column sits at max_gaps + 1) and both is one less."""
    rng = np.random.default_rng(seed)
    fill = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), (n_fill, width))
    column, gaps_there = width // 2, n_fill // 2
    fill[:gaps_there, column] = ord("-")
    fill[0, 0] = ord("-")      # one gap elsewhere: below every max_gaps used
    rows = [r.tobytes() for r in fill]
    x = bytearray(b"A" * width)
    y = bytearray(b"C" * width)
    x[column] = y[column] = ord("T")
    rows += [bytes(x), bytes(y)]
    i, j = n_fill, n_fill + 1
    g = R.column_gaps(rows)
    assert g[column] == gaps_there and g.max() == gaps_there and (np.delete(g, column) <= 1).all() and gaps_there >= 3
    m1, b1, k1 = R.pair_counts(rows, "n", gaps_there)
    m0, b0, k0 = R.pair_counts(rows, "n", gaps_there - 1)
    assert (m1[i, j], b1[i, j], k1) == (1, width, width) and (m0[i, j], b0[i, j], k0) == (0, width - 1, width - 1)
    return rows, i, j, column, gaps_there
