"""The merge of existing alignments (-f, include/twl_merge.h) on the CPU: the oracle's maps on a hand-worked example, the oracle against its
pinned RNASim result, the pure checks of the C ABI (tests/merge_plan_kats.cpp), the ABI's symbol list, the command line's refusals.  No GPU
needed."""
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import merge_oracle as MO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

# Three files, two merges, worked by hand.  A has the most rows, so it is the root; B and C tie, so the star keeps them in file order and
# the LAST child, C, is merged first.
#   merge 1: A (3 columns) against C (4 columns), path 1 1 0 2 0: it starts with a run of query-only codes.
#            codes != 1 sit at 2 3 4  -> A's columns 0 1 2 move to 2 3 4;  codes != 2 sit at 0 1 2 4 -> C's columns 0..3 move to 0 1 2 4
#   merge 2: {A, C} (5 columns) against B (2 columns), path 2 1 0 2 2 2: it ends with a run of reference-only codes.
#            codes != 1 sit at 0 2 3 4 5 -> A: 2 3 4 -> 3 4 5, C: 0 1 2 4 -> 0 2 3 5;  codes != 2 sit at 1 2 -> B's columns 0 1 move to 1 2
HAND_FILES = [[b"ACG", b"A-G"], [b"TT"], [b"gc.t"]]
HAND_PATHS = [[1, 1, 0, 2, 0], [2, 1, 0, 2, 2, 2]]
HAND_MAPS_AFTER_1 = [[2, 3, 4], [0, 1], [0, 1, 2, 4]]
HAND_MAPS_AFTER_2 = [[3, 4, 5], [1, 2], [0, 2, 3, 5]]
HAND_ROWS = [[b"---ACG", b"---A-G"], [b"-TT---"], [b"g-c.-t"]]


def test_hand_worked_example():
    assert MO.schedule([2, 1, 1]) == (0, [2, 1])
    r, q = MO.path_ranks(HAND_PATHS[0])
    assert r.tolist() == [2, 3, 4] and q.tolist() == [0, 1, 2, 4]
    r, q = MO.path_ranks(HAND_PATHS[1])
    assert r.tolist() == [0, 2, 3, 4, 5] and q.tolist() == [1, 2]
    m = MO.Maps([3, 2, 4])
    m.apply([[0]], [[2]], [HAND_PATHS[0]])
    assert [p.tolist() for p in m.pos] == HAND_MAPS_AFTER_1 and m.width == [5, 2, 5]
    m.apply([[0, 2]], [[1]], [HAND_PATHS[1]])
    assert [p.tolist() for p in m.pos] == HAND_MAPS_AFTER_2 and m.width == [6, 6, 6]
    rows, W = m.rows(HAND_FILES)
    assert W == 6 and rows == HAND_ROWS


def test_path_shape_check():
    assert MO.path_ok([1, 1, 0, 2, 0], 3, 4)
    assert not MO.path_ok([1, 1, 0, 2, 0], 4, 4) and not MO.path_ok([1, 1, 0, 2, 0], 3, 3) and not MO.path_ok([1, 3, 0, 2, 0], 3, 4)


def test_schedule_is_a_stable_star():
    """Most rows first; ties keep the files' order; the last child is merged first."""
    assert MO.schedule([153, 166, 95, 165]) == (1, [2, 0, 3])
    assert MO.schedule([5, 5, 5]) == (0, [2, 1])
    assert MO.schedule([1, 9]) == (1, [0])


def _invariants(files, records, W):
    """What holds whatever the DP decides: one width; every row degapped is its input degapped; inside a file, only columns that are all-gap
    in that file were added."""
    at = 0
    for recs in files:
        out = records[at: at + len(recs)]
        at += len(recs)
        assert [n for n, _ in out] == [n for n, _ in recs]
        assert all(len(r) == W for _, r in out)
        for (_, a), (_, b) in zip(out, recs):
            assert a.replace(b"-", b"") == b.replace(b"-", b"")

        def squeeze(rows):
            m = np.array([np.frombuffer(r, dtype=np.uint8) for r in rows])
            return m[:, ~np.all(m == ord("-"), axis=0)].tobytes()

        assert squeeze([r for _, r in out]) == squeeze([r for _, r in recs])
    assert at == len(records)


@pytest.fixture(scope="module")
def rnasim():
    files = [MO.PO.read_fasta(f) for f in MO.list_files(os.path.join(GOLDEN, "RNASim_subalignments"))]
    records, W, maps, paths = MO.merge(files, "n")
    return files, records, W, maps, paths


def test_oracle_reproduces_pinned_rnasim(rnasim):
    files, records, W, maps, paths = rnasim
    want = json.load(open(os.path.join(GOLDEN, "merge_expected.json")))
    assert [len(f) for f in files] == [153, 166, 95, 165]
    assert W == want["width"] and len(records) == want["rows"] and [len(p) for p in paths] == want["path_lengths"]
    assert hashlib.md5(MO.to_bytes(records)).hexdigest() == want["md5"]


def test_oracle_invariants_rnasim(rnasim):
    files, records, W, maps, _ = rnasim
    _invariants(files, records, W)
    for pos, recs in zip(maps.pos, files):
        assert len(pos) == len(recs[0][1]) and np.all(np.diff(pos) > 0) and pos[-1] < W


def test_oracle_single_file_is_unchanged():
    recs = [(b"a", b"AC-g."), (b"b", b"ACTG-")]
    out, W, _, _ = MO.merge([recs], "n")
    assert out == recs and W == 5


def test_merge_plans_known_answers(tmp_path):
    """The pure checks of twl_merge_create / twl_merge_apply / twl_merge_finish (twilight_amd/csrc/twl_merge_plan.inc.hip), compiled by g++ alone."""
    exe = tmp_path / "merge_plan_kats"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "merge_plan_kats.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    lines = [l for l in r.stdout.splitlines() if l.startswith(("OK", "FAIL"))]
    failed = [l for l in lines if l.startswith("FAIL")]
    assert not failed and r.returncode == 0, r.stdout + r.stderr
    assert len(lines) >= 63


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(twl_[a-z_]+)\s*\(", text)))


def test_merge_header_matches_binding():
    from twilight_amd import merge

    assert set(_declared("twl_merge.h")) == set(merge.exported_symbols())


def test_merge_symbols_are_exported(built):
    import twilight_amd as twl

    lib = twl.load_library()
    for name in _declared("twl_merge.h"):
        assert getattr(lib, name) is not None, name


def _cli(*args, timeout=60):
    exe = os.path.join(ROOT, "twilight_amd", "twilight-mi355x")
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize("extra", [("-t", "x.nwk"), ("-i", "x.fa"), ("-a", "x.aln")])
def test_cli_refuses_f_with_other_inputs(built, tmp_path, extra):
    r = _cli("-f", str(tmp_path), "-o", str(tmp_path / "o.aln"), *extra)
    assert r.returncode == 1 and "cannot be combined" in r.stderr


def test_cli_refuses_host_staged_and_several_gpus_in_merge(built, tmp_path):
    r = _cli("-f", str(tmp_path), "-o", str(tmp_path / "o.aln"), "--host-staged")
    assert r.returncode == 1 and "--host-staged" in r.stderr
    r = _cli("-f", str(tmp_path), "-o", str(tmp_path / "o.aln"), "--gpu-index", "0,1")
    assert r.returncode == 1 and "one GPU" in r.stderr


def test_cli_refuses_an_empty_directory(built, tmp_path):
    d = tmp_path / "empty"
    (d / "sub").mkdir(parents=True)
    r = _cli("-f", str(d), "-o", str(tmp_path / "o.aln"))
    assert r.returncode == 1 and "no alignment file" in r.stderr
    r = _cli("-f", str(tmp_path / "missing"), "-o", str(tmp_path / "o.aln"))
    assert r.returncode == 1 and "not a directory" in r.stderr


def test_cli_refuses_a_file_with_rows_of_two_lengths(built, tmp_path):
    d = tmp_path / "in"
    d.mkdir()
    (d / "a.aln").write_bytes(b">x\nACGT\n>y\nAC-T\n")
    (d / "b.aln").write_bytes(b">z\nACGT\n>w\nACG\n")
    r = _cli("-f", str(d), "-o", str(tmp_path / "o.aln"))
    assert r.returncode == 1 and "does not match" in r.stderr and "b.aln" in r.stderr
    assert not (tmp_path / "o.aln").exists()


def test_checker_binaries_keep_refusing_f(built):
    """The CPU-check build of the same main.cpp carries no merge mode: -f stays an unsupported option there."""
    exe = os.path.join(ROOT, "oracle", "twilight-cpucheck")
    r = subprocess.run([exe, "-f", "x", "-o", "o.aln"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "unsupported option -f" in r.stderr
