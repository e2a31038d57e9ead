"""Directed inputs of twl_store_score_rows (include/twl_score.h), each listed for what it reaches in the kernels (score_kernels.hip.h), on the
constants of twl_score_describe: S 64-bit words of a plane per staged slice, T rows of a pair tile's edge, R rows of a counts row slice,
F rows per flush of the packed byte counters.  tests/test_score_oracle_cpu.py proves every claim from the oracle; the GPU tests run every
case.  No device needed here."""
from collections import namedtuple

import numpy as np

GAP = 0x2D
# rows: bytes of one length; seq_type 'n' / 'p'; reaches: the claim in words; claim: None or a function (oracle module, case) -> None that asserts it
Case = namedtuple("Case", "name rows seq_type reaches claim")


def sparse_row(W, letters, fill=b"A"):
    """'-' everywhere but at the listed columns."""
    r = bytearray(b"-" * W)
    for c in letters:
        r[c] = fill[0]
    return bytes(r)


def random_rows(rng, n, W, p_gap=0.5, alphabet=b"ACGT"):
    letters = np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), size=(n, W))]
    gaps = rng.random((n, W)) < p_gap
    return [bytes(r) for r in np.where(gaps, GAP, letters).astype(np.uint8)]


def _bits(row):
    return {c for c, b in enumerate(row) if b != GAP}


def _claim_run_closes(x_col, a_col, runs01):
    """Row 0 holds '-' at x_col where row 1 holds a letter (an X bit); the A bit that closes its segment is row 0's letter at a_col; no letter of
    row 0 lies between; the pair (0, 1) has runs01 runs by both statements."""
    def claim(O, case):
        a, b = _bits(case.rows[0]), _bits(case.rows[1])
        assert x_col in b and x_col not in a and a_col in a
        assert not any(x_col < c < a_col for c in a)
        p = O.present(case.rows)
        ints = O.as_integers(case.rows)
        assert O.walk_pair(p[0], p[1])[0] == runs01 == O.carry_pair(ints[0], ints[1], len(case.rows[0]))
    return claim


def carry_cases(S):
    W = 64 * 5
    out = []
    out.append(Case("closing bit in the next word", [sparse_row(W, [0, 70]), sparse_row(W, [40])], "n",
                    "an X bit in word 0, its closing A bit in word 1", _claim_run_closes(40, 70, 1)))
    out.append(Case("closing bit three words up", [sparse_row(W, [0, 200]), sparse_row(W, [40])], "n",
                    "an X bit in word 0, its closing A bit in word 3, words 1 and 2 all '-' in both rows: the carry passes whole words",
                    _claim_run_closes(40, 200, 1)))
    out.append(Case("bit 63 and bit 0", [sparse_row(W, [3, 64]), sparse_row(W, [63])], "n", "an X bit at bit 63 of word 0, the A bit at bit 0 of word 1",
                    _claim_run_closes(63, 64, 1)))

    def last_column(O, case):
        p = O.present(case.rows)
        r, g, rt, gt = O.walk_pair(p[0], p[1])
        assert (r, g, rt, gt) == (1, 10, 1, 10) and case.rows[1][-1] != GAP and case.rows[0][-1] == GAP
        assert len(case.rows[0]) % 64 != 0 and O.carry_pair(*O.as_integers(case.rows), len(case.rows[0])) == 1
    out.append(Case("run to the last column", [sparse_row(100, [10]), sparse_row(100, range(90, 100))], "n",
                    "a run that ends at the last real column: the carry leaves through the rest of the word and the pad words", last_column))

    def last_column_of_a_slice(O, case):
        assert len(case.rows[0]) == S * 64 and O.carry_runs_row(case.rows) == [1, 1]
    out.append(Case("run to the last column of a whole slice", [sparse_row(S * 64, [0]), sparse_row(S * 64, [S * 64 - 1])], "n",
                    "the plane has no pad word: the carry out of the slice's last word is the top segment", last_column_of_a_slice))

    def second_slice(O, case):
        assert len(case.rows[0]) > S * 64 and O.carry_runs_row(case.rows) == [2, 2]
    out.append(Case("a run across two slices", [sparse_row(S * 64 + 70, [0, S * 64 + 5]), sparse_row(S * 64 + 70, [S * 64 - 2, S * 64 + 60])], "n",
                    "a carry that is open when the pair kernel stages its second slice", second_slice))
    return out


def content_cases():
    out = []

    def letterless(O, case):
        runs, tot = O.walk_all(case.rows)
        assert runs == [2, 0, 0] and tot == dict(R=2, G=8, RT=2, GT=8)      # one run of 4 columns against each lettered row, terminal, counted once
    out.append(Case("a row without letters", [b"-------", b"AC--GT-", b"CA--TG-"], "n", "a row without letters: one run per lettered row that touches both ends", letterless))

    def identical(O, case):
        runs, tot = O.walk_all(case.rows)
        assert runs == [0, 0] and tot["G"] == 0
    out.append(Case("two identical rows", [b"AC--GT-A", b"AC--GT-A"], "n", "two identical rows: no run, every column of the projection holds two letters", identical))

    def all_empty(O, case):
        assert O.walk_all(case.rows)[0] == [0, 0, 0] and O.column_totals(case.rows)["letters"] == 0
    out.append(Case("no letter at all", [b"-----"] * 3, "n", "every projection is empty", all_empty))

    def one_end(O, case):
        p = O.present(case.rows)
        assert O.walk_pair(p[0], p[1]) == (2, 4, 1, 3)      # ---LL-LLL: the leading run is terminal, the inner one is not; no trailing run
        assert O.walk_pair(p[1], p[0]) == (2, 5, 1, 3)      # LLL--L---: an inner run of 2, a trailing run of 3; no leading run
    out.append(Case("terminal runs at one end only", [b"----AC-GTA", b"ACG---T---"], "n", "a leading run without a trailing one, and the reverse", one_end))

    def every_class(seq_type, alphabet):
        def claim(O, case):
            K = O.classes(seq_type)
            cnt = O.class_counts(case.rows, seq_type)
            assert all(int(cnt[:, a].sum()) > 0 for a in range(K + 1))
            sub = O.sub_table(case.rows, seq_type)
            assert all(int(sub[a, K]) > 0 for a in range(K)) and int(sub[K, K]) > 0
        return claim
    nuc = [b"ACGTUacgtuNn.*\x80-", b"acgtuACGTUXR-N\xff.", b"TGCAATGCAANNNNNN", b"NNNNNNNNNNACGTAC"]
    out.append(Case("every nucleotide class", nuc, "n", "A C G T U in both cases, N, '.', '*' and bytes >= 0x80 as the class other", every_class("n", b"ACGT")))
    prot_letters = b"ACDEFGHIKLMNPQRSTVWY"
    prot = [prot_letters + b"BJOUXZ*.-", prot_letters.lower() + b"bjouxz-\x80X", prot_letters[::-1] + b"XXXXXXXXX", b"X" * 20 + prot_letters[:9]]
    out.append(Case("every protein class", prot, "p", "the 20 amino acids in both cases, B J O U X Z '*' '.' and a byte >= 0x80 as the class other", every_class("p", prot_letters)))
    return out


def width_cases(S, seed=11):
    rng = np.random.default_rng(seed)
    out = []
    for W in (1, 63, 64, 65, S * 64 - 1, S * 64, S * 64 + 1):
        def claim(O, case, W=W):
            assert len(case.rows[0]) == W
        out.append(Case(f"W = {W}", random_rows(rng, 5, W, 0.5), "n", "a width below, on and above a word and a staged slice", claim))
    return out


def row_count_cases(T, seed=12):
    rng = np.random.default_rng(seed)
    out = []
    for n in (2, T - 1, T, T + 1, 2 * T + 1):
        def claim(O, case, n=n):
            assert len(case.rows) == n
        out.append(Case(f"n = {n}", random_rows(rng, n, 70, 0.5), "n", "one tile, a full tile, a ragged second tile, three tiles: diagonal and off-diagonal tile pairs", claim))
    return out


def counter_cases(R, F, seed=13):
    """A first column that is 'A' in every row wraps a byte counter that is not flushed; W = 9 leaves the last thread one live column."""
    rng = np.random.default_rng(seed)
    out = []
    for n in (F - 1, F, F + 1, R - 1, R, R + 1):
        rows = [b"A" + r for r in random_rows(rng, n, 8, 0.3)]

        def claim(O, case, n=n):
            assert len(case.rows) == n and all(r[0] == ord("A") for r in case.rows) and len(case.rows[0]) == 9
        out.append(Case(f"{n} rows over the counters", rows, "n", "rows around the flush period and around the row slice of the counts kernel", claim))
    return out


def all_cases(S, T, R, F):
    return carry_cases(S) + content_cases() + width_cases(S) + row_count_cases(T) + counter_cases(R, F)
