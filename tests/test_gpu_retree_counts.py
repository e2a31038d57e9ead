"""twl_retree_column_gaps and twl_retree_pair_counts on the MI355X against the numpy restatement (tests/retree_oracle.py), exactly: row counts on
every edge of the tile of pairs and of the gap kernel's row slice, widths on every edge of a packed word and of a staged slice (all taken
from twl_retree_describe), guard words behind every output, symmetry, the diagonal, directed rows, a count that does not fit 16 bits, and
the protein letters."""
import numpy as np
import pytest

import retree_cases as K
import retree_oracle as R

pytestmark = pytest.mark.gpu

GUARD = 256


def _geometry():
    from twilight_amd import retree

    d = retree.describe()
    return d["word_columns"], d["pair_tile"], d["word_columns"] * d["slice_words"], d["gap_rows"]


def _combos():
    """(n, width): every n of {1, 2, tile - 1, tile, tile + 1, 2 tiles + 1} and every width of {1, word - 1 and its half, word, word + 1, slice - 1,
    slice, slice + 1, 2 slices + 1} at least once, not the full cross."""
    w, t, s, _ = _geometry()
    return [(1, 1), (2, w // 2 - 1), (t - 1, w // 2), (t, w // 2 + 1), (t + 1, w - 1), (2 * t + 1, w), (2, w + 1), (t + 1, s - 1), (t, s), (t - 1, s + 1), (2 * t + 1, 2 * s + 1),
            (1, s + 1)]


def _check_pairs(rows, type_, mg):
    """One call with guards; returns (match, both) after holding them to the restatement, symmetry and the diagonal."""
    from twilight_amd import retree

    n = len(rows)
    want_m, want_b, want_kept = R.pair_counts(rows, type_, mg)
    fm, fb, kept = retree.pair_counts(rows, type_, mg, guard_words=GUARD)
    assert (fm[n * n:] == 0xFFFFFFFF).all() and (fb[n * n:] == 0xFFFFFFFF).all(), "the call wrote behind an n x n output"
    m, b = fm[: n * n].reshape(n, n), fb[: n * n].reshape(n, n)
    assert kept == want_kept
    bad = np.argwhere((m != want_m) | (b != want_b))
    assert len(bad) == 0, (n, len(rows[0]), bad[:5], [(int(m[tuple(x)]), int(want_m[tuple(x)]), int(b[tuple(x)]), int(want_b[tuple(x)])) for x in bad[:5]])
    assert (m == m.T).all() and (b == b.T).all()
    letters = (R.letter_table(type_)[R.matrix(rows)][:, R.kept_columns(rows, mg)] >= 0).sum(axis=1)
    assert (np.diag(m) == letters).all() and (np.diag(b) == letters).all()
    return m, b


@pytest.mark.parametrize("which", range(12))
def test_sizes_on_every_edge(gpu, which):
    from twilight_amd import retree

    n, width = _combos()[which]
    rows = K.seeded_rows("n", n, width, seed=1000 * n + width)
    flat = retree.column_gaps(rows, guard_words=GUARD)
    assert (flat[width:] == 0xFFFFFFFF).all(), "the call wrote behind its output"
    assert (flat[:width] == R.column_gaps(rows)).all()
    mg = R.max_gaps(0.5, n)
    if n > 2:
        kept = R.kept_columns(rows, mg)
        assert width < 8 or (kept.any() and not kept.all()), "the mask must drop some columns and keep some"
    _check_pairs(rows, "n", mg)
    _check_pairs(rows, "n", n)


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_gap_counts_around_the_row_slice(gpu, delta):
    from twilight_amd import retree

    _, _, _, g = _geometry()
    for n in (g + delta, 2 * g + delta):
        rows = K.seeded_rows("n", n, 300, seed=77 + n)
        flat = retree.column_gaps(rows, guard_words=GUARD)
        assert (flat[300:] == 0xFFFFFFFF).all()
        assert (flat[:300] == R.column_gaps(rows)).all()


def test_directed_rows(gpu):
    _, _, s, _ = _geometry()
    rows, facts = K.directed_rows(s + 90, s, seed=11)
    K.check_directed(rows, facts, s)
    n, width = len(rows), len(rows[0])
    m, b = _check_pairs(rows, "n", n)
    f = {kind: (i, j) for kind, i, j in facts}
    i, j = f["identical"]
    assert m[i, j] == b[i, j] == width
    for kind in ("all_gap", "all_N"):
        i = f[kind][0]
        assert not m[i].any() and not b[i].any() and not m[:, i].any() and not b[:, i].any()
    i, j = f["no_common_column"]
    assert b[i, j] == 0 and m[i, j] == 0
    for kind in ("match_only_in_last_column", "match_only_in_first_column_of_a_slice"):
        i, j = f[kind]
        assert m[i, j] == 1 and b[i, j] == width
    _check_pairs(rows, "n", R.max_gaps(0.5, n))


def test_a_match_in_a_column_the_mask_drops(gpu):
    rows, i, j, column, g = K.masked_match_rows(10, 40, seed=6)
    m, b = _check_pairs(rows, "n", g)
    assert m[i, j] == 1 and b[i, j] == 40, "the column sits exactly at max_gaps: kept"
    m, b = _check_pairs(rows, "n", g - 1)
    assert m[i, j] == 0 and b[i, j] == 39, "the column sits at max_gaps + 1: dropped"


def test_a_count_above_16_bits(gpu):
    """Two identical rows of 70 001 letters and an unrelated one: match(0, 1) = both(0, 1) = 70 001.  A partial sum held in 16 bits gets this wrong."""
    rng = np.random.default_rng(20261019)
    a = bytes(rng.choice(list(b"ACGT"), 70001).tolist())
    c = bytes(rng.choice(list(b"ACGT"), 70001).tolist())
    m, b = _check_pairs([a, a, c], "n", 3)
    print("match =", m.tolist(), "both =", b.tolist())
    assert m[0, 1] == b[0, 1] == 70001 and b[0, 2] == 70001 and 0 < m[0, 2] < 65536


def test_protein_letters(gpu):
    """n = tile + 1, width 33: all twenty letters in both cases, and B Z X J O U * which are none."""
    _, t, _, _ = _geometry()
    rows = K.seeded_rows("p", t + 1, 33, seed=33)
    seen = set(b"".join(rows))
    assert set(b"ACDEFGHIKLMNPQRSTVWY") <= seen and set(b"BZXJOU*") <= seen
    _check_pairs(rows, "p", R.max_gaps(0.5, t + 1))
    _check_pairs(rows, "p", t + 1)
    # every letter against every letter, and against itself in lower case
    letters = b"ACDEFGHIKLMNPQRSTVWYBZXJOU*"
    rows = [bytes([x]) * len(letters) for x in letters] + [letters, letters.lower()]
    m, b = _check_pairs(rows, "p", len(rows))
    assert m[len(letters), len(letters) + 1] == 20 and b[len(letters), len(letters) + 1] == 20
