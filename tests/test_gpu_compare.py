"""`--compare REF`, `--write-compare FILE` and `--evaluate EST` of twilight-mi355x on the MI355X, on the fixtures under tests/golden and on a
small family with its true alignment (tools/true_family.py): the line on stderr and the file are the text tests/compare_oracle.py makes from
the two alignment files; an alignment against itself scores 1; -o is the same bytes with the flag and without it.  Every CLI run has its own
time limit."""
import gzip
import importlib.util
import os
import re
import subprocess

import pytest

import compare_oracle as CO
import strand_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "twilight_amd", "twilight-mi355x")

pytestmark = pytest.mark.gpu


def _cli(*args, timeout=240, ok=True):
    r = subprocess.run(["timeout", "-k", "10", str(timeout), EXE, *args], capture_output=True, text=True, timeout=timeout + 30)
    if ok:
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    return r


def _line(stderr):
    lines = [l for l in stderr.splitlines() if l.startswith("compare: ")]
    assert len(lines) == 1, stderr[-2000:]
    return lines[0]


def _numbers(line):
    m = re.fullmatch(r"compare: rows (\d+) \((\d+) only in the output, (\d+) only in the reference\) pairs_out (\d+) pairs_ref (\d+) shared (\d+) SP (\S+) modeler (\S+) "
                     r"TC (\d+)/(\d+) columns (\d+)/(\d+)", line)
    assert m, line
    return m.groups()


@pytest.fixture(scope="module")
def work(built, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("compare"))
    sars = os.path.join(d, "sars_20.fa")
    with open(sars, "wb") as f:
        f.write(gzip.open(os.path.join(GOLDEN, "sars_20.fa.gz")).read())
    names, seqs, _, _ = SC.rnasim200()
    rna200 = SC.write_fasta(os.path.join(d, "rnasim200.fa"), names, seqs)
    spec = importlib.util.spec_from_file_location("true_family", os.path.join(ROOT, "tools", "true_family.py"))
    tf = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tf)
    tf.write_family(os.path.join(d, "fam"), *tf.make_true_family(60, 400, seed=5, sub=0.03, indel=0.004))
    return {"dir": d, "sars": ("-t", os.path.join(GOLDEN, "sars_20.nwk"), "-i", sars), "rna200": ("-i", rna200, "--type", "n"),
            "rnasim": ("-t", os.path.join(GOLDEN, "RNASim.nwk"), "-i", os.path.join(GOLDEN, "RNASim.fa.gz")), "fam": os.path.join(d, "fam")}


@pytest.mark.parametrize("which", ["sars", "rna200"])
def test_an_output_against_itself(gpu, work, which):
    """SP = modeler = 1.000000, TC = all, shared = both pair counts; the second run writes the bytes of the first."""
    first, again = os.path.join(work["dir"], which + ".aln"), os.path.join(work["dir"], which + ".again.aln")
    r = _cli(*work[which], "-o", first)
    assert "compare:" not in r.stderr
    r = _cli(*work[which], "-o", again, "--compare", first)
    assert open(again, "rb").read() == open(first, "rb").read(), "a run with --compare writes the -o of the run without it"
    rows, a, b, pout, pref, shared, sp, modeler, tc, tcall, we, wr = _numbers(_line(r.stderr))
    assert (a, b) == ("0", "0") and int(rows) == (20 if which == "sars" else 200)
    assert pout == pref == shared and int(shared) > 0 and (sp, modeler) == ("1.000000", "1.000000") and tc == tcall and int(tc) > 0 and we == wr
    assert _line(r.stderr) == CO.compare_files(again, first)[0]


@pytest.mark.parametrize("mode", ["merge", "place", "place_on_tree", "iterations"])
def test_every_writer_of_the_output_compares(gpu, work, mode):
    """-f, -a, --place-on-tree and the last run of --iterations: the rows as each mode writes them, against the mode's own output."""
    import sys

    if GOLDEN not in sys.path:
        sys.path.insert(0, GOLDEN)
    import make_place_expected as MPE
    import make_place_tree_expected as MK

    d = work["dir"]
    if mode == "merge":
        args = ("-f", os.path.join(GOLDEN, "RNASim_subalignments"))
    elif mode == "place":
        sub = os.path.join(d, "RNASim_sub.fa")
        MPE.write_sub_fasta(sub)
        args = ("-a", os.path.join(GOLDEN, "RNASim_backbone.aln.gz"), "-i", sub)
    elif mode == "place_on_tree":
        ptree, pbackbone, pnew = MK.sample_inputs(d)
        args = ("-t", ptree, "-a", pbackbone, "-i", pnew, "--type", "n", "--place-on-tree")
    else:
        args = work["sars"] + ("--iterations", "2")
    first, again = os.path.join(d, mode + ".aln"), os.path.join(d, mode + ".again.aln")
    _cli(*args, "-o", first)
    r = _cli(*args, "-o", again, "--compare", first)
    assert open(again, "rb").read() == open(first, "rb").read()
    line = _line(r.stderr)
    assert line == CO.compare_files(again, first)[0]
    rows, a, b, pout, pref, shared, sp, modeler, tc, tcall, we, wr = _numbers(line)
    assert (a, b) == ("0", "0") and pout == pref == shared and (sp, modeler) == ("1.000000", "1.000000") and tc == tcall


def test_rnasim_against_the_backbone_fixture(gpu, work):
    """The RNASim run with -t against tests/golden/RNASim_backbone.aln.gz: the names both hold, every number of the line and of
    --write-compare as the oracle computes them from the two files; --evaluate on the written file prints the same line and file; -v adds the
    phase times."""
    out, tsv, tsv2 = os.path.join(work["dir"], "rnasim.aln"), os.path.join(work["dir"], "rnasim.tsv"), os.path.join(work["dir"], "rnasim2.tsv")
    ref = os.path.join(GOLDEN, "RNASim_backbone.aln.gz")
    r = _cli(*work["rnasim"], "-o", out, "--compare", ref, "--write-compare", tsv, "-v")
    line, text = CO.compare_files(out, ref)
    assert _line(r.stderr) == line
    rows, a, b = (int(x) for x in _numbers(line)[:3])
    assert rows >= 2 and a > 0, "the backbone holds a part of the family's names"
    assert open(tsv).read() == "\n".join(text) + "\n"
    m = re.search(r"Compare phases \(ms\): upload ([0-9.]+), key kernels ([0-9.]+), column kernel ([0-9.]+), download ([0-9.]+)", r.stderr)
    assert m and float(m.group(2)) > 0 and float(m.group(3)) > 0
    e = _cli("--evaluate", out, "--compare", ref, "--write-compare", tsv2)
    assert _line(e.stderr) == line and open(tsv2).read() == open(tsv).read()
    assert "Compare phases" not in e.stderr


@pytest.mark.parametrize("mode", ["tree", "subtrees", "no_tree"])
def test_a_true_family(gpu, work, mode):
    """A family of tools/true_family.py under -t, -m and without a tree, each against its truth: the oracle's line (how much of the truth a mode finds is measured,
    tools/compare_bench.py, not asserted)."""
    fam = work["fam"]
    args = {"tree": ("-t", os.path.join(fam, "t.nwk")), "subtrees": ("-t", os.path.join(fam, "t.nwk"), "-m", "16"), "no_tree": ("--type", "n")}[mode]
    out = os.path.join(work["dir"], "fam." + mode + ".aln")
    truth = os.path.join(fam, "true.aln")
    r = _cli(*args, "-i", os.path.join(fam, "s.fa"), "-o", out, "--compare", truth)
    line = _line(r.stderr)
    assert line == CO.compare_files(out, truth)[0]
    rows, a, b, pout, pref, shared, sp, modeler, tc, tcall, we, wr = _numbers(line)
    assert (rows, a, b) == ("60", "0", "0") and 0 < int(shared) <= min(int(pout), int(pref)) and int(tc) <= int(tcall)


def test_refusals_after_the_inputs_are_read(gpu, work):
    """A common row whose letters or letter count differ: the message names the row and says which; exit 1, -o stays in place, no file of
    --write-compare appears.  Fewer than 2 common names."""
    d = work["dir"]
    first = os.path.join(d, "sars.ref.aln")
    _cli(*work["sars"], "-o", first)
    names, rows = CO.read_alignment(first)
    for what, edit, say in (("letters", lambda r: r.replace(b"A", b"#", 1), "the letters differ"), ("count", lambda r: re.sub(rb"[^-]", b"-", r, count=1), "the letter count differs")):
        bad = os.path.join(d, "sars.bad." + what + ".aln")
        victim = names[7]
        with open(bad, "wb") as f:
            for n in names:
                f.write(b">" + n.encode() + b"\n" + (edit(rows[n]) if n in (victim, names[11]) else rows[n]) + b"\n")
        out, tsv = os.path.join(d, "sars.out." + what + ".aln"), os.path.join(d, "sars.bad." + what + ".tsv")
        r = _cli(*work["sars"], "-o", out, "--compare", bad, "--write-compare", tsv, ok=False)
        assert r.returncode == 1 and f'ERROR: --compare: the row "{victim}" does not hold the sequence of its row in {bad}: {say}' in r.stderr, r.stderr[-2000:]
        assert open(out, "rb").read() == open(first, "rb").read() and not os.path.exists(tsv)
    few = os.path.join(d, "sars.few.aln")
    with open(few, "wb") as f:
        f.write(b">" + names[0].encode() + b"\n" + rows[names[0]] + b"\n>nobody\n" + rows[names[1]] + b"\n")
    r = _cli("--evaluate", first, "--compare", few, ok=False)
    assert r.returncode == 1 and "have 1 name(s) in common; a comparison needs at least 2 (19 only in the output, 1 only in the reference)" in r.stderr
