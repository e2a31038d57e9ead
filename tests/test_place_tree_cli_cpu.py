"""The command line of placement along a tree (-t -a -i -o --place-on-tree) where it needs no device: everything it refuses, with the text, before a
device is opened; the header of the backbone squeeze against its binding and the library; the two known-answer programs of the mode
(tests/backbone_plan_kats.cpp, tests/place_tree_kats.cpp), plain and under the address and undefined-behaviour sanitizers; and the checker's build
of the same sources, which carries none of it.  No GPU needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "twilight_amd", "csrc", "host")
TREE = "((a:0.1,n1:0.2):0.1,(b:0.1,(c:0.2,n2:0.1):0.1):0.2);\n"


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
    assert "twl_init" not in r.stderr and "usage:" not in r.stderr and "Sequences resident" not in r.stderr, r.stderr


def _mode(tmp_path):
    return ("-t", str(tmp_path / "none.nwk"), "-a", str(tmp_path / "none.aln"), "-i", str(tmp_path / "none.fa"), "-o", str(tmp_path / "o.aln"), "--place-on-tree")


def test_usage_names_the_mode(built):
    r = _cli()
    assert r.returncode == 1 and "-t <tree.nwk> -a <backbone.aln[.gz]> -i <new_sequences.fa[.gz]> -o <out.aln> --place-on-tree" in r.stderr
    assert "re-aligned against each other" in r.stderr


def test_without_the_flag_a_and_t_stay_refused(built, tmp_path):
    r = _cli("-a", "x.aln", "-t", "x.nwk", "-i", "x.fa", "-o", str(tmp_path / "o.aln"))
    _refused(r, "placement with a tree", "not supported yet", "--place-on-tree", "re-aligns the backbone's groups")


def test_the_flag_needs_both_a_and_t(built, tmp_path):
    out = ("-i", str(tmp_path / "none.fa"), "-o", str(tmp_path / "o.aln"), "--place-on-tree")
    for given in ((), ("-a", "x.aln"), ("-t", "x.nwk")):
        _refused(_cli(*out, *given), "--place-on-tree needs both -a", "and -t")


def test_refuses_the_other_modes_and_host_staged(built, tmp_path):
    _refused(_cli(*_mode(tmp_path), "-m", "50"), "--place-on-tree cannot be combined with -m or -f")
    _refused(_cli(*_mode(tmp_path), "-f", str(tmp_path)), "--place-on-tree cannot be combined with -m or -f")
    _refused(_cli(*_mode(tmp_path), "--host-staged"), "--host-staged is not available with --place-on-tree")
    _refused(_cli(*_mode(tmp_path), "--iterations", "2"), "--iterations cannot be combined with -a, -f or -m")


def test_refuses_several_gpus_at_parse_time(built, tmp_path):
    """Before any file is opened: none of them exists."""
    for extra in (("--gpu-index", "0,1"), ("-G", "2")):
        r = _cli(*_mode(tmp_path), *extra)
        _refused(r, "--place-on-tree runs on one GPU")
        assert "open" not in r.stderr


def test_refuses_write_tree_and_tree_seeds(built, tmp_path):
    _refused(_cli(*_mode(tmp_path), "--write-tree", str(tmp_path / "t.nwk")), "--place-on-tree cannot be combined with --write-tree or --tree-seeds")
    _refused(_cli(*_mode(tmp_path), "--tree-seeds", "16"), "--place-on-tree cannot be combined with --write-tree or --tree-seeds")


def test_still_a_usage_error_without_sequences_or_output(built, tmp_path):
    r = _cli("-t", "x.nwk", "-a", "x.aln", "-o", str(tmp_path / "o.aln"), "--place-on-tree")
    assert r.returncode == 1 and r.stderr.startswith("usage:")


def _inputs(tmp_path, backbone, new, tree=TREE):
    (tmp_path / "t.nwk").write_text(tree)
    a = _fasta(tmp_path / "b.aln", backbone)
    i = _fasta(tmp_path / "n.fa", new)
    return ("-t", str(tmp_path / "t.nwk"), "-a", a, "-i", i, "-o", str(tmp_path / "o.aln"), "--place-on-tree", "--type", "n")


def test_refused_after_reading_the_inputs(built, tmp_path):
    """Rows of two lengths, a leaf in neither file, no new sequence, no backbone row: after the reads, before a device is opened."""
    good_b = [("a", "AC-GT-A"), ("b", "ACGGT-A"), ("c", "A--GTCA")]
    good_n = [("n1", "ACGTA"), ("n2", "ACGGTA")]
    _refused(_cli(*_inputs(tmp_path, [("a", "AC-GT-A"), ("b", "ACGGT-"), ("c", "A--GTCA")], good_n)), 'length of "b" (6) does not match', "must all have one length")
    _refused(_cli(*_inputs(tmp_path, good_b[:2], good_n)), 'the tree\'s leaf "c" is neither a row of', "nor a sequence of")
    _refused(_cli(*_inputs(tmp_path, good_b, good_n[:1])), 'the tree\'s leaf "n2" is neither a row of')
    _refused(_cli(*_inputs(tmp_path, good_b, [("x1", "ACGTA")])), "no new sequence of", "is a leaf of the tree")
    _refused(_cli(*_inputs(tmp_path, [("y", "ACGT")], good_n)), "no backbone row of", "is a leaf of the tree")
    assert not os.path.exists(tmp_path / "o.aln")


def test_checker_binary_knows_none_of_it(built, tmp_path):
    exe = os.path.join(ROOT, "oracle", "twilight-cpucheck")
    r = subprocess.run([exe, "-t", "x.nwk", "-i", "x.fa", "-o", str(tmp_path / "o.aln"), "--place-on-tree"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "unsupported option --place-on-tree" in r.stderr
    r = subprocess.run([exe, "-t", "x.nwk", "-a", "x.aln", "-i", "x.fa", "-o", str(tmp_path / "o.aln")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "unsupported option -a" in r.stderr
    syms = subprocess.run(["nm", "-D", "--defined-only", "-C", exe], capture_output=True, text=True).stdout + subprocess.run(["nm", "-C", exe], capture_output=True, text=True).stdout
    assert "squeeze" not in syms and "runPlacementOnTree" not in syms and "readPlacementInputs" not in syms


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(twl_[a-z_]+)\s*\(", text)))


def test_backbone_header_matches_binding_and_library(built):
    import twilight_amd as twl
    from twilight_amd import backbone

    assert _declared("twl_backbone.h") == sorted(["twl_store_squeeze_groups", "twl_store_squeeze_timing", "twl_squeeze_describe"])
    assert set(_declared("twl_backbone.h")) == set(backbone.exported_symbols())
    lib = twl.load_library()
    for name in _declared("twl_backbone.h"):
        assert getattr(lib, name) is not None, name
    import __graft_entry__ as g

    for f in ("twl_backbone.inc.hip", "twl_backbone_plan.inc.hip", "backbone_kernels.hip.h"):
        assert f in g.KERNEL_SOURCES
    # the plan file is pure: no HIP call, no global of the library
    plan = open(os.path.join(ROOT, "twilight_amd", "csrc", "twl_backbone_plan.inc.hip")).read()
    assert "hip" not in re.sub(r"//.*", "", plan).lower().replace(".inc.hip", "") and "g_err" not in plan
    # the files the CPU checker links name no symbol of the new header
    for f in ("align_resident.cpp", "progressive.cpp", "driver.cpp", "align_gpu.cpp", "phylo.cpp", "seqdb_io.cpp", "helpers.cpp"):
        text = open(os.path.join(HOST, f)).read()
        assert "squeeze" not in text and "twl_backbone" not in text, f


SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all"]


def _kats(exe, *args):
    r = subprocess.run([str(exe), *args], capture_output=True, text=True)
    lines = [l for l in r.stdout.splitlines() if l.startswith(("OK", "FAIL"))]
    failed = [l for l in lines if l.startswith("FAIL")]
    assert not failed and r.returncode == 0, r.stdout + r.stderr
    return len(lines)


@pytest.mark.parametrize("san", [[], SAN], ids=["plain", "asan_ubsan"])
def test_backbone_plan_known_answers(tmp_path, san):
    exe = tmp_path / "backbone_plan_kats"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *san, "-o", str(exe), os.path.join(ROOT, "tests", "backbone_plan_kats.cpp")])
    assert _kats(exe) >= 31


@pytest.mark.parametrize("san", [[], SAN], ids=["plain", "asan_ubsan"])
def test_placement_reroot_known_answers(tmp_path, san):
    exe = tmp_path / "place_tree_kats"
    srcs = [os.path.join(HOST, f) for f in ("phylo.cpp", "seqdb_io.cpp", "helpers.cpp", "progressive.cpp", "driver.cpp")]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-ffp-contract=off", "-Wall", *san, "-o", str(exe), os.path.join(ROOT, "tests", "place_tree_kats.cpp")] + srcs + ["-lz"])
    assert _kats(exe, str(tmp_path)) >= 8
