"""twl_store_score_rows (include/twl_score.h; score_kernels.hip.h, twl_score.inc.hip) through the binding, on stores built from host rows,
against tests/score_oracle.py, exactly: sub, runs_row and the totals on every directed case of tests/score_cases.py (on the constants of
twl_score_describe) and on seeded random rows, with rows on both planes and unlisted rows, and what the call refuses; then `--score`,
`--write-score` and `--score-alignment` of twilight-mi355x on the fixtures under tests/golden.  Every CLI run has its own time limit."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import score_cases as SC
import score_oracle as SO
import strand_cases as STC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "twilight_amd", "twilight-mi355x")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def consts(gpu):
    from twilight_amd import score

    S, T, R, F = score.describe()
    assert S >= 2 and T >= 2 and 4 < F < R
    return S, T, R, F


def _score_and_compare(st, rows, ids, seq_type, what=""):
    """rows: the listed rows in the order of ids."""
    from twilight_amd import score

    sub, runs, tot = score.score_rows(st, ids, seq_type)
    want_sub, want_runs, want_tot = SO.expected(rows, seq_type)
    assert [int(x) for x in runs] == want_runs, what
    assert tot == want_tot, what
    assert (sub.astype(object) == want_sub).all(), what
    pack, cols, pairs = score.score_ms(st)
    assert pack > 0 and cols > 0 and pairs > 0
    return tot


def _run_cases(cases):
    from twilight_amd import level

    for c in cases:
        st = level.Store(c.rows, c.seq_type)
        try:
            _score_and_compare(st, c.rows, list(range(len(c.rows))), c.seq_type, f"{c.name} ({c.reaches})")
            assert st.rows() == list(c.rows), "nothing in the store changes"
        finally:
            st.close()


def test_carries(gpu, consts):
    """A carry into the next word, through two all-gap words, from bit 63 into bit 0, out of the last real column into the pad, out of a plane
    without pad, and one that is open between two staged slices."""
    S, T, R, F = consts
    cases = SC.carry_cases(S)
    assert len(cases) == 6
    _run_cases(cases)


def test_contents(gpu, consts):
    """A row without letters, identical rows, no letter at all, terminal runs at one end only, every class of both alphabets."""
    _run_cases(SC.content_cases())


def test_widths(gpu, consts):
    S, T, R, F = consts
    cases = SC.width_cases(S)
    assert {len(c.rows[0]) for c in cases} == {1, 63, 64, 65, S * 64 - 1, S * 64, S * 64 + 1}
    _run_cases(cases)


def test_row_counts(gpu, consts):
    """One tile pair, a full tile, a ragged second tile, three tiles: diagonal and off-diagonal tile pairs."""
    S, T, R, F = consts
    cases = SC.row_count_cases(T)
    assert {len(c.rows) for c in cases} == {2, T - 1, T, T + 1, 2 * T + 1}
    _run_cases(cases)


def test_counters(gpu, consts):
    """Row counts around the flush period of the packed byte counters and around the counts kernel's row slice, a column that would wrap."""
    S, T, R, F = consts
    cases = SC.counter_cases(R, F)
    assert {len(c.rows) for c in cases} == {F - 1, F, F + 1, R - 1, R, R + 1}
    _run_cases(cases)


@pytest.mark.parametrize("seed,n,W,p_gap,seq_type", [(21, 200, 4096, 0.6, "n"), (22, 150, 1111, 0.95, "n"), (23, 67, 1500, 0.3, "p"), (24, 131, 2049, 0.05, "n")])
def test_random_rows(gpu, consts, seed, n, W, p_gap, seq_type):
    from twilight_amd import level

    rng = np.random.default_rng(seed)
    rows = SC.random_rows(rng, n, W, p_gap, b"ACGTN" if seq_type == "n" else SO.PROT + b"X")
    rows[3] = b"-" * W
    rows[5] = rows[4]
    st = level.Store(rows, seq_type)
    try:
        tot = _score_and_compare(st, rows, list(range(n)), seq_type, f"seed {seed}")
        assert tot["R"] > 0 and tot["RT"] > 0
    finally:
        st.close()


def test_rows_on_both_planes_in_any_order_beside_unlisted_rows(gpu, consts):
    """Every second row moved to the store's other plane (a squeeze over rows without an all-gap column rewrites them there at the same
    length, the stale copies stay behind), the ids listed in a shuffled order, rows of another length unlisted among them."""
    from twilight_amd import backbone, level

    S, T, R, F = consts
    rng = np.random.default_rng(31)
    n, W = T + 7, S * 64 + 9
    live = SC.random_rows(rng, n, W, 0.3)
    extra = [b"ACGT", b"", b"AC-GTACGT"]
    st = level.Store(live[:10] + extra + live[10:], "n")
    try:
        id_of = list(range(10)) + list(range(13, n + 3))      # the store id of live row k
        moved = [id_of[k] for k in range(0, n, 2)]
        assert backbone.squeeze_groups(st, [moved]) == [W], "no all-gap column among the moved rows"
        order = [int(k) for k in rng.permutation(n)]
        _score_and_compare(st, [live[k] for k in order], [id_of[k] for k in order], "n", "two planes")
        got = st.rows()
        assert [got[i] for i in id_of] == live and got[10:13] == extra
    finally:
        st.close()


def test_refusals(gpu):
    import twilight_amd as twl
    from twilight_amd import level, score

    st = level.Store([b"AC-GT", b"A--GT", b"ACG", b"", b""], "n")
    try:
        for ids, seq_type, message in (([0], "n", "fewer than two rows listed"), ([0, 0], "n", "a sequence id is listed twice"), ([0, 5], "n", "sequence id out of range"),
                                       ([0, 2], "n", "the listed rows differ in length"), ([0, 1], "x", "unknown sequence type"), ([3, 4], "n", "the listed rows have no column")):
            with pytest.raises(twl.TwlError, match=message):
                score.score_rows_raw(st, len(ids), ids, seq_type)
        with pytest.raises(twl.TwlError, match="bad argument"):
            score.score_rows_raw(st, 2, [0, 1], "n", want_runs=False)
        sub, runs, tot = score.score_rows(st, [1, 0], "n")
        assert [int(x) for x in runs] == [1, 0] and tot == dict(R=1, G=1, RT=0, GT=0, letters=7)
    finally:
        st.close()


# ---- the command line ----
def _cli(*args, timeout=240, ok=True):
    r = subprocess.run(["timeout", "-k", "10", str(timeout), EXE, *args], capture_output=True, text=True, timeout=timeout + 30)
    if ok:
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    return r


LINE = re.compile(r"(?:run (\d+) )?score: rows (\d+) columns (\d+) pairs (\d+) letters (\d+) gapcols (\d+) runs (\d+) terminal (\d+)/(\d+) score (-?\d+\.\d{6}) per_pair (-?\d+\.\d{6})")


def _lines(stderr):
    return [l for l in stderr.splitlines() if "score: rows " in l]


def _check_line(line, path, run=None):
    """Every integer of the line is the oracle's on the file; S within 1e-12 relative of the oracle's."""
    m = LINE.fullmatch(line)
    assert m, line
    names, rows = SO.read_fasta(path)
    sub, runs, tot = SO.expected(rows, "n")
    n, W = len(rows), len(rows[0])
    assert m.group(1) == (None if run is None else str(run))
    assert [int(x) for x in m.groups()[1:9]] == [n, W, n * (n - 1) // 2, tot["letters"], tot["G"], tot["R"], tot["RT"], tot["GT"]]
    want = SO.score(sub, tot, SO.nucleotide_matrix(), -50.0, -5.0, -5.0, 4)
    got = float(m.group(10))
    print("score", got, "oracle", want)
    assert abs(got - float("%.6f" % want)) <= 1e-12 * abs(want)
    per_pair = want / (n * (n - 1) // 2)      # printed with 6 decimals: S's 1e-12 relative may move the last printed digit by one
    assert abs(float(m.group(11)) - float("%.6f" % per_pair)) <= 1e-12 * abs(per_pair) + 1.0000001e-6
    return names, runs, sub, tot


@pytest.fixture(scope="module")
def work(built, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("score"))
    sars = os.path.join(d, "sars_20.fa")
    with open(sars, "wb") as f:
        f.write(gzip.open(os.path.join(GOLDEN, "sars_20.fa.gz")).read())
    names, seqs, _, _ = STC.rnasim200()
    rna200 = STC.write_fasta(os.path.join(d, "rnasim200.fa"), names, seqs)
    return {"dir": d, "sars": ("-t", os.path.join(GOLDEN, "sars_20.nwk"), "-i", sars), "rna200": ("-i", rna200, "--type", "n")}


@pytest.mark.parametrize("which", ["sars", "rna200"])
def test_the_written_alignment_is_scored(gpu, work, which):
    """The integers and S of the --score line are the oracle's on the written file; --write-score lists them and the rows; --score-alignment on
    that file prints the same line and writes the same file; -o is the bytes of the run without the flag."""
    d = work["dir"]
    plain, out, tsv, tsv2 = (os.path.join(d, which + e) for e in (".plain.aln", ".aln", ".tsv", ".2.tsv"))
    r = _cli(*work[which], "-o", plain)
    assert not _lines(r.stderr)
    r = _cli(*work[which], "-o", out, "--score", "--write-score", tsv, "-v")
    assert open(out, "rb").read() == open(plain, "rb").read(), "a run with --score writes the -o of the run without it"
    lines = _lines(r.stderr)
    assert len(lines) == 1 and "Score kernels (ms): pack " in r.stderr
    names, runs, sub, tot = _check_line(lines[0], out)
    assert len(names) == (20 if which == "sars" else 200)
    text = open(tsv).read().splitlines()
    keys = dict(l[1:].split("\t") for l in text if l.startswith("#"))
    assert [keys[k] for k in ("rows", "letters", "gapcols", "runs", "terminal_runs", "terminal_gapcols")] == [str(v) for v in (len(names), tot["letters"], tot["G"], tot["R"], tot["RT"], tot["GT"])]
    assert all(keys[f"sub_{a}_{b}"] == str(int(sub[a, b])) for a in range(5) for b in range(a, 5))
    assert keys["score"] == LINE.fullmatch(lines[0]).group(10)
    rows = SO.read_fasta(out)[1]
    assert [l.split("\t") for l in text if not l.startswith("#")] == [[nm, str(sum(1 for b in row if b != SO.GAP)), str(rn)] for nm, row, rn in zip(names, rows, runs)]
    r = _cli("--score-alignment", out, "--type", "n", "--write-score", tsv2)
    assert _lines(r.stderr) == lines and open(tsv2).read() == open(tsv).read()


def test_a_line_per_iteration(gpu, work):
    """--iterations 2 --score: two lines, `run 1` of the alignment the second tree was built from, `run 2` of the written one."""
    out = os.path.join(work["dir"], "iter.aln")
    r = _cli(*work["sars"], "-o", out, "--iterations", "2", "--score")
    lines = _lines(r.stderr)
    assert len(lines) == 2 and lines[0].startswith("run 1 score: ") and lines[1].startswith("run 2 score: ")
    _check_line(lines[1], out, run=2)
    assert LINE.fullmatch(lines[0]).group(2) == "20"
