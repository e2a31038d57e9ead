"""The command line of `--tree-seeds S` (the guide tree built in two stages) where it needs no device: what it refuses, at parse time or after
reading the records, the usage text, and the checker's build of the same main.cpp, which carries no such option.  These tests fail on a
build that does not know the option.  No GPU needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cli(*args, timeout=60):
    exe = os.path.join(ROOT, "twilight_amd", "twilight-mi355x")
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=timeout)


def _refused(r, *words):
    assert r.returncode == 1, r.stderr
    for w in words:
        assert w in r.stderr, (w, r.stderr)
    assert "twl_init" not in r.stderr and "usage:" not in r.stderr and "unsupported option" not in r.stderr, r.stderr


def test_usage_names_the_flag(built):
    r = _cli()
    assert r.returncode == 1 and "-i <sequences.fa[.gz]> -o <out.aln> [--write-tree <tree.nwk>] [--tree-seeds S]" in r.stderr
    assert "two stages" in r.stderr


@pytest.mark.parametrize("value", ["1", "0", "x", "16385", "-4", "12x", ""])
def test_refuses_a_bad_number_of_seeds_at_parse_time(built, tmp_path, value):
    """Before the file is even opened: it does not exist."""
    r = _cli("-i", str(tmp_path / "none.fa"), "-o", str(tmp_path / "o.aln"), "--tree-seeds", value)
    _refused(r, "--tree-seeds needs a number of seeds from 2 to 16384", "(got %s)" % value)
    assert "open" not in r.stderr


def test_refuses_a_missing_value(built, tmp_path):
    r = _cli("-i", str(tmp_path / "none.fa"), "-o", str(tmp_path / "o.aln"), "--tree-seeds")
    assert r.returncode == 1 and "missing value for --tree-seeds" in r.stderr


@pytest.mark.parametrize("mode", ["-t", "-a", "-f"])
def test_refused_where_the_run_builds_no_tree(built, tmp_path, mode):
    o = str(tmp_path / "o.aln")
    args = {"-t": ("-t", "x.nwk", "-i", "x.fa", "-o", o), "-a": ("-a", "x.aln", "-i", "x.fa", "-o", o), "-f": ("-f", str(tmp_path), "-o", o)}[mode]
    r = _cli(*args, "--tree-seeds", "8")
    _refused(r, "--tree-seeds applies to a run that builds its guide tree")
    assert not os.path.exists(o)


def test_refuses_more_seeds_than_sequences_after_reading(built, tmp_path):
    fa = tmp_path / "s.fa"
    fa.write_text("".join(">s%d\nACGTACGTAC\n" % i for i in range(5)) + ">s0\nACGTACGTAA\n")      # the second s0 is dropped: 5 sequences
    r = _cli("-i", str(fa), "-o", str(tmp_path / "o.aln"), "--type", "n", "--tree-seeds", "6")
    _refused(r, "--tree-seeds 6 is more than the 5 sequences")
    assert not (tmp_path / "o.aln").exists()


def test_the_name_checks_come_first(built, tmp_path):
    fa = tmp_path / "s.fa"
    fa.write_text(">ok\nACGTACGTAC\n>a(b\nACGTACGTAA\n>fine\nACGTACGTCC\n")
    r = _cli("-i", str(fa), "-o", str(tmp_path / "o.aln"), "--type", "n", "--tree-seeds", "2")
    _refused(r, "cannot be written into a Newick tree")


def test_the_one_stage_refusal_points_at_the_flag(built, tmp_path):
    """Its words stay (tests/test_guide_cli_cpu.py); a hint is appended."""
    fa = tmp_path / "many.fa"
    fa.write_text("".join(">s%d\nACGTACGT\n" % i for i in range(16385)))
    r = _cli("-i", str(fa), "-o", str(tmp_path / "o.aln"), "--type", "n")
    _refused(r, "16385 sequences", "at most 16384", "bring a tree with -t", "--tree-seeds")


def test_checker_binary_rejects_the_option(built, tmp_path):
    exe = os.path.join(ROOT, "oracle", "twilight-cpucheck")
    r = subprocess.run([exe, "-t", "x.nwk", "-i", "x.fa", "-o", str(tmp_path / "o.aln"), "--tree-seeds", "8"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "unsupported option --tree-seeds" in r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--tree-seeds" not in r.stderr
