"""The command line of a run without -t (the guide tree is built from the sequences) where it needs no device: what it refuses, at parse time
or after reading the records, and the checker's build of the same main.cpp, which carries no such mode.  These tests fail on a build that
takes `-i X -o Y` for a usage error.  No GPU needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cli(*args, timeout=60):
    exe = os.path.join(ROOT, "twilight_amd", "twilight-mi355x")
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=timeout)


def _fasta(path, records):
    path.write_text("".join(">%s\n%s\n" % r for r in records))
    return str(path)


def _refused(r, *words):
    assert r.returncode == 1, r.stderr
    for w in words:
        assert w in r.stderr, (w, r.stderr)
    assert "twl_init" not in r.stderr and "usage:" not in r.stderr, r.stderr


def test_usage_names_the_new_form(built):
    r = _cli()
    assert r.returncode == 1 and "-i <sequences.fa[.gz]> -o <out.aln> [--write-tree <tree.nwk>]" in r.stderr
    # the earlier forms are still listed as they were
    assert "usage: twilight-mi355x -t <tree.nwk> -i <sequences.fa[.gz]> -o <out.aln>" in r.stderr and "-m <max. leaves per subtree>" in r.stderr


def test_still_a_usage_error_without_input_or_output(built, tmp_path):
    for args in (("-i", "x.fa"), ("-o", str(tmp_path / "o.aln"))):
        r = _cli(*args)
        assert r.returncode == 1 and "usage:" in r.stderr


def test_refuses_fewer_than_two_sequences(built, tmp_path):
    one = _fasta(tmp_path / "one.fa", [("a", "ACGTACGTAC")])
    _refused(_cli("-i", one, "-o", str(tmp_path / "o.aln")), "at least 2 sequences")
    twice = _fasta(tmp_path / "twice.fa", [("a", "ACGTACGTAC"), ("a", "ACGTACGTAA")])      # a duplicate name keeps its first record: one sequence
    _refused(_cli("-i", twice, "-o", str(tmp_path / "o.aln")), "at least 2 sequences", "holds 1")
    assert not (tmp_path / "o.aln").exists()


def test_refuses_more_than_16384_sequences(built, tmp_path):
    many = _fasta(tmp_path / "many.fa", [("s%d" % i, "ACGTACGT") for i in range(16385)])
    _refused(_cli("-i", many, "-o", str(tmp_path / "o.aln"), "--type", "n"), "16385 sequences", "at most 16384", "bring a tree with -t")


def test_refuses_several_gpus_at_parse_time(built, tmp_path):
    """Before the file is even opened: it does not exist."""
    for extra in (("--gpu-index", "0,1"), ("-G", "2")):
        r = _cli("-i", str(tmp_path / "none.fa"), "-o", str(tmp_path / "o.aln"), *extra)
        _refused(r, "one GPU", "-t")
        assert "open" not in r.stderr


def test_refuses_host_staged(built, tmp_path):
    r = _cli("-i", str(tmp_path / "none.fa"), "-o", str(tmp_path / "o.aln"), "--host-staged")
    _refused(r, "--host-staged is not available without -t")


@pytest.mark.parametrize("name", ["a(b", "a)b", "a,b", "a:b", "a;b", "a\vb", "node_7", "nodeX", ""])
def test_refuses_names_a_newick_tree_cannot_hold(built, tmp_path, name):
    fa = _fasta(tmp_path / "s.fa", [("ok", "ACGTACGTAC"), (name, "ACGTACGTAA"), ("fine", "ACGTACGTCC")])
    r = _cli("-i", fa, "-o", str(tmp_path / "o.aln"), "--type", "n")
    if name == "":
        _refused(r, "without a name")
    elif name.startswith("node"):
        _refused(r, name, 'begins with "node"')
    else:
        _refused(r, "cannot be written into a Newick tree")
    assert not (tmp_path / "o.aln").exists()


def test_a_blank_ends_the_name_as_everywhere(built, tmp_path):
    """'>a b' is the sequence a: blanks never reach the name (readSequences cuts there too), so the header alone is no reason to refuse;
    the run gets as far as the device it needs."""
    fa = _fasta(tmp_path / "s.fa", [("a b", "ACGTACGTAC"), ("c\td", "ACGTACGTAA")])
    r = _cli("-i", fa, "-o", str(tmp_path / "o.aln"), "--type", "n")
    assert "Newick" not in r.stderr and "usage:" not in r.stderr


def test_write_tree_is_refused_with_a_tree(built, tmp_path):
    r = _cli("-t", "x.nwk", "-i", "x.fa", "-o", str(tmp_path / "o.aln"), "--write-tree", str(tmp_path / "t.nwk"))
    _refused(r, "--write-tree cannot be combined with -t")
    assert not (tmp_path / "t.nwk").exists()
    r = _cli("-a", "x.aln", "-i", "x.fa", "-o", str(tmp_path / "o.aln"), "--write-tree", str(tmp_path / "t.nwk"))
    _refused(r, "--write-tree applies to a run that builds its guide tree")


def test_placement_with_a_tree_stays_refused(built, tmp_path):
    r = _cli("-a", "x.aln", "-t", "x.nwk", "-i", "x.fa", "-o", str(tmp_path / "o.aln"))
    assert r.returncode == 1 and "placement with a tree" in r.stderr


def test_checker_binary_behaves_as_before(built, tmp_path):
    """The CPU-check build of the same main.cpp carries no guide mode: -i and -o without -t stay a usage error, --write-tree an unknown option."""
    exe = os.path.join(ROOT, "oracle", "twilight-cpucheck")
    r = subprocess.run([exe, "-i", "x.fa", "-o", str(tmp_path / "o.aln")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stderr.startswith("usage:") and "--write-tree" not in r.stderr
    r = subprocess.run([exe, "-t", "x.nwk", "-i", "x.fa", "-o", str(tmp_path / "o.aln"), "--write-tree", "t"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "unsupported option --write-tree" in r.stderr


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(twl_[a-z_]+)\s*\(", text)))


def test_guide_header_matches_binding_and_library(built):
    import twilight_amd as twl
    from twilight_amd import guide

    assert {"twl_guide_bins", "twl_guide_kmer_counts", "twl_guide_shared"} <= set(_declared("twl_guide.h"))
    assert set(_declared("twl_guide.h")) == set(guide.exported_symbols())
    lib = twl.load_library()
    for name in _declared("twl_guide.h"):
        assert getattr(lib, name) is not None, name
    import __graft_entry__ as g

    for f in ("twl_guide.inc.hip", "twl_guide_plan.inc.hip", "guide_kernels.hip.h"):
        assert f in g.KERNEL_SOURCES
    assert guide.MAX_SEQS == 16384 and "#define TWL_GUIDE_MAX_SEQS 16384" in open(os.path.join(ROOT, "include", "twl_guide.h")).read()
