"""`--adjust-direction` on the MI355X, through the command line, on the three fixtures with a reverse complement planted at every record i with
i % 3 == 1: --write-directions is the plant exactly, and the alignment is, apart from the _R_ names, byte for byte the alignment of the run
without the flag on the original file -- without -t (the written trees are equal byte for byte too), with -t on the written tree, and with
-a.  A run whose plant is empty writes the bytes of the run without the flag.  Every CLI run has its own time limit."""
import os
import subprocess

import pytest

import strand_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "twilight_amd", "twilight-mi355x")

pytestmark = pytest.mark.gpu


def _cli(*args, timeout=300):
    r = subprocess.run(["timeout", "-k", "10", str(timeout), EXE, *args], capture_output=True, text=True, timeout=timeout + 30)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    return r


def _read(path):
    return open(path, "rb").read()


def _without_marks(blob, names, dirs):
    """The alignment with the _R_ taken off the names of the planted records; every planted record must carry it, no other may."""
    marked = {b">_R_" + n.encode() for n, d in zip(names, dirs) if d}
    lines = blob.split(b"\n")
    seen = set()
    for k, l in enumerate(lines):
        if l.startswith(b">_R_"):
            assert l in marked, l
            seen.add(l)
            lines[k] = b">" + l[4:]
    assert seen == marked
    return b"\n".join(lines)


def _directions(path):
    return [tuple(l.split("\t")) for l in open(path).read().splitlines()]


def _want_directions(names, dirs):
    return [(n, "-" if d else "+") for n, d in zip(names, dirs)]


@pytest.mark.parametrize("family,seeds", [("rnasim200", None), ("rnasim200", 8), ("sars20", None)])
def test_without_a_tree_and_with_the_written_tree(gpu, tmp_path, family, seeds):
    names, seqs, planted, dirs = getattr(SC, family)()
    orig, plant = SC.write_fasta(tmp_path / "orig.fa", names, seqs), SC.write_fasta(tmp_path / "plant.fa", names, planted)
    a, b, c, ta, tb, d = (str(tmp_path / x) for x in ("a.aln", "b.aln", "c.aln", "a.nwk", "b.nwk", "d.tsv"))
    flags = ["--adjust-direction"] + (["--direction-seeds", str(seeds)] if seeds else [])
    _cli("-i", orig, "-o", a, "--write-tree", ta, "--type", "n")
    r = _cli("-i", plant, "-o", b, "--write-tree", tb, "--type", "n", "--write-directions", d, "--check", "-v", *flags)
    assert "Directions: %d of %d sequences lie reversed" % (int(dirs.sum()), len(names)) in r.stderr and "spanning tree" in r.stderr
    assert "WARNING: --check" not in r.stderr
    assert _directions(d) == _want_directions(names, dirs)
    assert _read(ta) == _read(tb)                             # the tree is built from the oriented records and keeps the original names
    assert _without_marks(_read(b), names, dirs) == _read(a)
    _cli("-t", tb, "-i", plant, "-o", c, "--type", "n", *flags)
    assert _read(c) == _read(b)                               # -t on the written tree with the same flags repeats the run


def test_placement_into_a_backbone(gpu, tmp_path):
    backbone, names, seqs, planted, dirs = SC.placement()
    bb = os.path.join(GOLDEN, "RNASim_backbone.aln.gz")
    orig, plant = SC.write_fasta(tmp_path / "orig.fa", names, seqs), SC.write_fasta(tmp_path / "plant.fa", names, planted)
    a, b, d = (str(tmp_path / x) for x in ("a.aln", "b.aln", "d.tsv"))
    _cli("-a", bb, "-i", orig, "-o", a, "--type", "n")
    r = _cli("-a", bb, "-i", plant, "-o", b, "--type", "n", "--adjust-direction", "--write-directions", d)
    assert "Directions: %d of 100 sequences lie reversed" % int(dirs.sum()) in r.stderr and "49 seeds, rows of the backbone" in r.stderr
    assert _directions(d) == _want_directions(names, dirs)
    assert _without_marks(_read(b), names, dirs) == _read(a)
    assert _read(b).count(b">") == len(backbone) + 100


def test_an_empty_plant_changes_nothing(gpu, tmp_path):
    names, seqs, _, _ = SC.rnasim200()
    orig = SC.write_fasta(tmp_path / "orig.fa", names, seqs)
    a, b, ta, tb, d = (str(tmp_path / x) for x in ("a.aln", "b.aln", "a.nwk", "b.nwk", "d.tsv"))
    _cli("-i", orig, "-o", a, "--write-tree", ta, "--type", "n")
    _cli("-i", orig, "-o", b, "--write-tree", tb, "--type", "n", "--adjust-direction", "--write-directions", d)
    assert _read(a) == _read(b) and _read(ta) == _read(tb)
    assert _directions(d) == [(n, "+") for n in names]


@pytest.mark.parametrize("mode", [("-m", "50"), ("--iterations", "2"), ("--tree-seeds", "8")])
def test_composes_with_subtrees_iterations_and_the_two_stage_tree(gpu, tmp_path, mode):
    names, seqs, planted, dirs = SC.rnasim200()
    orig, plant = SC.write_fasta(tmp_path / "orig.fa", names, seqs), SC.write_fasta(tmp_path / "plant.fa", names, planted)
    a, b = str(tmp_path / "a.aln"), str(tmp_path / "b.aln")
    _cli("-i", orig, "-o", a, "--type", "n", *mode)
    _cli("-i", plant, "-o", b, "--type", "n", "--adjust-direction", *mode)
    assert _without_marks(_read(b), names, dirs) == _read(a)
