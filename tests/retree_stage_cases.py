"""Alignments for the tests of the two-stage rebuilt guide tree: rows whose ratios with a set of seeds spread from 0 to
1, and directed rows, each built so that the property it is listed for can be read off its construction."""
import numpy as np

LETTERS = {"n": b"ACGT", "p": b"ACDEFGHIKLMNPQRSTVWY"}
NO_LETTER = {"n": b"NnRY.", "p": b"XBZ*xbzJOU."}


def family(type_, n, width, seed, lower=0.0):
    """uint8 [n][width]: every row is one of three unrelated ancestors with 0, 2, 10 or 30 % of its letters redrawn, 2 % of its bytes '-'
    (95 % in every fifth column, so that the default mask drops about half of those), 2 % a byte that is no letter, and the part `lower` of
    its letters in lower case."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(LETTERS[type_], dtype=np.uint8)
    anc = rng.choice(letters, (3, width))
    a = anc[rng.integers(0, 3, n)]
    hit = rng.random((n, width)) < rng.choice([0.0, 0.02, 0.1, 0.3], n)[:, None]
    a = np.where(hit, rng.choice(letters, (n, width)), a)
    if lower:
        a = np.where(rng.random((n, width)) < lower, a | 0x20, a)
    junk = rng.random((n, width)) < 0.02
    a = np.where(junk, rng.choice(np.frombuffer(NO_LETTER[type_], dtype=np.uint8), (n, width)), a)
    gap = rng.random((n, width)) < np.where(np.arange(width) % 5 == 0, 0.95, 0.02)[None, :]
    return np.ascontiguousarray(np.where(gap, ord("-"), a).astype(np.uint8))


def as_bytes(a):
    return [r.tobytes() for r in a]


def near_tie_rows():
    """(rows, seeds, row): width 8193; with the seed at t = 0 the row has 8191 / 8192 (one column without a letter, one mismatch), with the seed
    at t = 1 it has 8192 / 8193.  8192 * 8192 = 67108864 > 8191 * 8193 = 67108863: t = 1 is closer, by a quarter of an fp32 ulp."""
    w = 8193
    a = b"N" + b"C" + b"A" * (w - 2)
    b = b"C" + b"A" * (w - 1)
    x = b"A" * w
    return [a, b, x], [0, 1], 2


def deciding_column_rows():
    """(rows, seeds, row, gaps_there): 21 columns.  The row is A x 10 + C x 11, seed 0 is all A, seed 1 all C: 10 / 21 against 11 / 21, seed 1.
    Column 20 holds '-' in gaps_there = 4 of the six filler rows and no other column holds any: with max_gaps = 3 it is dropped, both seeds
    stand at 10 / 20 and the smaller t takes the row."""
    rng = np.random.default_rng(8)
    fill = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), (6, 21))
    fill[:4, 20] = ord("-")
    return [b"A" * 21, b"C" * 21] + as_bytes(fill) + [b"A" * 10 + b"C" * 11], [0, 1], 8, 4


def twin_seed_rows(ta, tb, seed):
    """(rows, seeds): 170 rows of 300 letters; rows 0, 128 and 169 are one text X, rows 1 .. 127 unrelated to it, rows 129 .. 168 mutants of X.
    The 129 seeds are rows 1 .. 127 with row 128 put at position ta and row 0 at position tb > ta: every mutant of X, and the copy that is no
    seed, has the same ratio with both, and the seed at the smaller t has the LARGER id, so that an order by id would show."""
    assert ta < tb
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    x = rng.choice(letters, 300)
    others = [rng.choice(letters, 300).tobytes() for _ in range(127)]
    mutants = []
    for _ in range(40):
        m = x.copy()
        hit = rng.random(300) < 0.03
        m[hit] = rng.choice(letters, int(hit.sum()))
        mutants.append(m.tobytes())
    rows = [x.tobytes()] + others + [x.tobytes()] + mutants + [x.tobytes()]
    seeds = list(range(1, 128))
    seeds.insert(ta, 128)
    seeds.insert(tb, 0)
    assert len(seeds) == 129 and seeds[ta] == 128 and seeds[tb] == 0
    return rows, seeds
