"""`--trim-gappy T`, `--trim-to NAME` and `--write-columns FILE` of twilight-mi355x on the MI355X, one case per mode, on the fixtures under
tests/golden: the output with the flag is the output of the same command without it with the columns deleted that tests/trim_oracle.py
deletes (those untrimmed outputs are pinned by the modes' own end-to-end tests); names and order are unchanged; the column file is the
oracle's text.  Bytes only.  Every CLI run has its own time limit."""
import gzip
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import strand_cases as SC
import trim_oracle as TO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "twilight_amd", "twilight-mi355x")
sys.path.insert(0, GOLDEN)

pytestmark = pytest.mark.gpu


def _cli(*args, timeout=240, ok=True):
    r = subprocess.run(["timeout", "-k", "10", str(timeout), EXE, *args], capture_output=True, text=True, timeout=timeout + 30)
    if ok:
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    return r


def _commands(d):
    """mode -> the arguments of its command without -o, on committed fixtures (written into d where the tool reads plain files)."""
    sars = os.path.join(d, "sars_20.fa")
    with open(sars, "wb") as f:
        f.write(gzip.open(os.path.join(GOLDEN, "sars_20.fa.gz")).read())
    sars_tree = os.path.join(GOLDEN, "sars_20.nwk")
    names, seqs, _, _ = SC.rnasim200()
    rna200 = SC.write_fasta(os.path.join(d, "rnasim200.fa"), names, seqs)
    snames, sseqs, splanted, sdirs = SC.sars20()
    plant = SC.write_fasta(os.path.join(d, "sars_planted.fa"), snames, splanted)
    assert sdirs.sum() > 0
    import make_place_expected as MPE
    import make_place_tree_expected as MK

    sub = os.path.join(d, "RNASim_sub.fa")
    MPE.write_sub_fasta(sub)
    ptree, pbackbone, pnew = MK.sample_inputs(d)
    return {
        "default_sars": ("-t", sars_tree, "-i", sars),
        "default_rnasim200_no_tree": ("-i", rna200, "--type", "n"),
        "subtrees": ("-t", sars_tree, "-i", sars, "-m", "8"),
        "merge": ("-f", os.path.join(GOLDEN, "RNASim_subalignments")),
        "place": ("-a", os.path.join(GOLDEN, "RNASim_backbone.aln.gz"), "-i", sub),
        "place_on_tree": ("-t", ptree, "-a", pbackbone, "-i", pnew, "--type", "n", "--place-on-tree"),
        "iterations": ("-t", sars_tree, "-i", sars, "--iterations", "2"),
        "adjust_direction": ("-t", sars_tree, "-i", plant, "--type", "n", "--adjust-direction"),
        "check": ("-t", sars_tree, "-i", sars, "--check"),
    }, [n for n, r in zip(snames, sdirs) if r]


@pytest.fixture(scope="module")
def work(built, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("trim"))
    commands, reversed_names = _commands(d)
    return {"dir": d, "commands": commands, "reversed": reversed_names, "plain": {}}


MODES = ["default_sars", "default_rnasim200_no_tree", "subtrees", "merge", "place", "place_on_tree", "iterations", "adjust_direction", "check"]


def _plain(work, mode):
    """The untrimmed output of a mode: (names, rows), made once and shared."""
    if mode not in work["plain"]:
        out = os.path.join(work["dir"], mode + ".plain.aln")
        r = _cli(*work["commands"][mode], "-o", out)
        assert "Trimmed" not in r.stderr
        names, rows = TO.read_fasta(out)
        assert len(names) >= 2 and len({len(x) for x in rows}) == 1
        work["plain"][mode] = (names, rows, open(out, "rb").read())
    return work["plain"][mode]


def _fasta(names, rows):
    return b"".join(b">" + n.encode() + b"\n" + r + b"\n" for n, r in zip(names, rows))


def _summary(stderr):
    m = re.search(r"Trimmed the alignment: (\d+) of (\d+) columns kept \((.*)\); (\d+) row\(s\) became all '-'", stderr)
    assert m, stderr[-2000:]
    return int(m.group(1)), int(m.group(2)), m.group(3), int(m.group(4))


def _where(stderr):
    m = re.search(r"Trim kernels ([0-9.]+) ms on (the resident rows|an uploaded copy of the final rows)", stderr)
    assert m, stderr[-2000:]
    assert float(m.group(1)) > 0
    return m.group(2)


@pytest.mark.parametrize("mode", MODES)
def test_trim_gappy(gpu, work, mode):
    """A T from the oracle on the untrimmed output: the limit is the middle one of the gap counts its columns have, T = (limit + 1/2) / N, so
    that columns lie on both sides of it.  The rows, the column file, the stderr line; -v says where the trim ran."""
    names, rows, _ = _plain(work, mode)
    N, W = len(rows), len(rows[0])
    distinct = sorted(set(TO.gap_counts(rows).tolist()))
    assert len(distinct) > 1, "the fixture's columns differ in their gap counts"
    limit = distinct[(len(distinct) - 1) // 2]
    T = (limit + 0.5) / N
    assert TO.max_gaps(T, N) == limit
    mask, want = TO.agree(rows, TO.MAX_GAPS, limit)
    assert 0 < mask.sum() < W
    out, cols = os.path.join(work["dir"], mode + ".gappy.aln"), os.path.join(work["dir"], mode + ".cols.tsv")
    r = _cli(*work["commands"][mode], "-o", out, "--trim-gappy", repr(T), "--write-columns", cols, "-v")
    assert open(out, "rb").read() == _fasta(names, want)
    assert open(cols).read() == TO.column_text(rows, mask)
    kept, width, rule, all_gap = _summary(r.stderr)
    assert (kept, width) == (int(mask.sum()), W)
    assert rule.startswith("--trim-gappy ") and rule.endswith(f": at most {limit} gaps in {N} rows")
    assert all_gap == sum(1 for x in want if x == b"-" * kept)
    assert f"(length {kept})" in r.stderr
    assert _where(r.stderr) == ("an uploaded copy of the final rows" if mode == "check" else "the resident rows")
    if mode == "check":
        assert "WARNING: --check" not in r.stderr


@pytest.mark.parametrize("mode", MODES)
def test_trim_to(gpu, work, mode):
    """The columns of one written row: the first row from the middle on that holds a gap; with --adjust-direction a turned record, under
    the name it is written by."""
    names, rows, _ = _plain(work, mode)
    if mode == "adjust_direction":
        among = [names.index("_R_" + n) for n in work["reversed"]]
    else:
        among = list(range(len(names) // 2, len(names))) + list(range(len(names) // 2))
    ref = next(k for k in among if b"-" in rows[k])
    mask, want = TO.agree(rows, TO.TO_ROW, ref)
    assert 0 < mask.sum() < len(rows[0])
    out = os.path.join(work["dir"], mode + ".to.aln")
    r = _cli(*work["commands"][mode], "-o", out, "--trim-to", names[ref])
    got_names, got_rows = TO.read_fasta(out)
    assert got_names == names
    assert got_rows == want
    assert b"-" not in got_rows[ref] and got_rows[ref] == rows[ref].replace(b"-", b"")
    kept, width, rule, _ = _summary(r.stderr)
    assert (kept, width) == (int(mask.sum()), len(rows[0])) and rule == f"--trim-to {names[ref]}: the columns of that row"
    assert "Trim kernels" not in r.stderr      # (-v only)


def test_trim_gappy_1_writes_the_untrimmed_bytes(gpu, work):
    for mode in ("default_sars", "merge"):
        names, rows, blob = _plain(work, mode)
        out = os.path.join(work["dir"], mode + ".one.aln")
        r = _cli(*work["commands"][mode], "-o", out, "--trim-gappy", "1")
        assert open(out, "rb").read() == blob
        kept, width, _, _ = _summary(r.stderr)
        assert kept == width == len(rows[0])


def test_trim_gappy_0_keeps_the_gap_free_columns(gpu, work):
    mode = next(m for m in MODES if int(TO.gap_counts(_plain(work, m)[1]).min()) == 0)      # (from the oracle: an output with a gap-free column)
    names, rows, _ = _plain(work, mode)
    mask, want = TO.agree(rows, TO.MAX_GAPS, 0)
    assert mask.sum() > 0
    out = os.path.join(work["dir"], "zero.aln")
    _cli(*work["commands"][mode], "-o", out, "--trim-gappy", "0")
    assert open(out, "rb").read() == _fasta(names, want)
    assert not any(b"-" in x for x in want)


def test_no_column_survives(gpu, work, tmp_path):
    """A fixture and a T from the oracle: the first mode whose untrimmed output has no gap-free column, at the largest T whose limit lies
    below its least gap count.  Where every mode's output has a gap-free column, a merge of one file in which every column holds a gap."""
    chosen = None
    for mode in ("place", "merge", "place_on_tree", "default_rnasim200_no_tree"):
        names, rows, _ = _plain(work, mode)
        least = int(TO.gap_counts(rows).min())
        if least > 0:
            chosen = (work["commands"][mode], (least - 0.5) / len(rows), rows)
            break
    if chosen is None:
        d = tmp_path / "one"
        d.mkdir()
        rows = [b"AC-T", b"A-GT", b"-CGT", b"ACG-"]
        (d / "only.aln").write_bytes(_fasta(["a", "b", "c", "d"], rows))
        chosen = (("-f", str(d)), 0.0, rows)
    command, T, rows = chosen
    assert not TO.keep_mask(rows, TO.MAX_GAPS, TO.max_gaps(T, len(rows))).any()
    out, cols = tmp_path / "none.aln", tmp_path / "none.tsv"
    r = _cli(*command, "-o", str(out), "--trim-gappy", repr(T), "--write-columns", str(cols), ok=False)
    assert r.returncode == 1, r.stderr[-2000:]
    assert "ERROR: no column is kept" in r.stderr
    assert not out.exists() and not cols.exists()


def test_trim_to_a_name_that_is_not_written(gpu, work, tmp_path):
    out = tmp_path / "o.aln"
    r = _cli(*work["commands"]["default_sars"], "-o", str(out), "--trim-to", "no-such-row", ok=False)
    assert r.returncode == 1 and "ERROR: --trim-to: no written row is called no-such-row" in r.stderr
    assert not out.exists()
    # a turned record is written as _R_<name>: its input name is no written row
    r = _cli(*work["commands"]["adjust_direction"], "-o", str(out), "--trim-to", work["reversed"][0], ok=False)
    assert r.returncode == 1 and "no written row is called " + work["reversed"][0] in r.stderr
    assert not out.exists()
