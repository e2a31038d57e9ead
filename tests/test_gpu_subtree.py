"""The subtree mode on the MI355X (`twilight-mi355x -t T -i S -o O -m N`, twilight_amd/csrc/host/subtrees.cpp) through the command line, against
the CPU restatement of the mode (tests/subtree_oracle.py): the committed fixture tests/golden/subtree_expected.json for the repository's two
sample families, the restatement run in the test for two small synthetic ones.  Every CLI run has its own time limit."""
import gzip
import hashlib
import json
import os
import re
import subprocess

import pytest

import subtree_cases as SC
import subtree_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "twilight_amd", "twilight-mi355x")
EXPECTED = json.load(open(os.path.join(GOLDEN, "subtree_expected.json")))

pytestmark = pytest.mark.gpu


def _cli(*args, timeout=120):
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=timeout)


def _md5(path):
    return hashlib.md5(open(path, "rb").read()).hexdigest()


def _totals(stderr):
    m = re.search(r"Aligned (\d+) subtrees \((\d+) rows\) and merged them: subtrees (\d+) pairs, (\d+) band cells; merge (\d+) band cells, (\d+) retried", stderr)
    assert m, stderr[-2000:]
    return [int(x) for x in m.groups()]


def _merge_levels(stderr):
    return [int(x) for x in re.findall(r"Subtree merge level \d+: (\d+) pairs? in one twl_merge_apply", stderr)]


def _sources(stderr):
    return {int(k): ("cached" if what.startswith("cached") else "weighted") for k, what in re.findall(r"Subtree (\d+) profile: (cached msaFreq|weighted columns)", stderr)}


@pytest.mark.parametrize("case", sorted(EXPECTED))
def test_sample_families_equal_the_fixture(gpu, tmp_path, case):
    """sars_20 at -m 8 (four subtrees) and RNASim at -m 100 (seven): md5 and width of the output, band cells of both phases, and a first merge
    level of two pairs that reaches the device as one level (twl_merge_apply with n_pairs = 2)."""
    fx = EXPECTED[case]
    fa = tmp_path / "s.fa"
    fa.write_bytes(gzip.open(os.path.join(GOLDEN, fx["sequences"])).read())
    out = tmp_path / "o.aln"
    r = _cli("-t", os.path.join(GOLDEN, fx["tree"]), "-i", str(fa), "-o", str(out), "-m", str(fx["max_subtree"]), "-v")
    assert r.returncode == 0, r.stderr[-2000:]
    subtrees, rows, _, cells_a, cells_b, retries = _totals(r.stderr)
    assert (subtrees, rows) == (fx["subtrees"], fx["rows"])
    assert f"(length {fx['width']})" in r.stderr
    assert _md5(out) == fx["md5"]
    assert (cells_a, cells_b, retries) == (fx["band_cells_subtrees"], fx["band_cells_merge"], fx["merge_retries"])
    assert _merge_levels(r.stderr) == fx["merge_pairs_per_level"] and max(fx["merge_pairs_per_level"]) >= 2
    assert _sources(r.stderr) == {int(k): v for k, v in fx["profile_source"].items()}


def test_a_tree_that_is_not_split_is_the_default_run(gpu, tmp_path):
    """-m 1000000 on 20 leaves: one partition, the default run, the same bytes as the run without -m."""
    fa = tmp_path / "s.fa"
    fa.write_bytes(gzip.open(os.path.join(GOLDEN, "sars_20.fa.gz")).read())
    tree = os.path.join(GOLDEN, "sars_20.nwk")
    a, b = tmp_path / "a.aln", tmp_path / "b.aln"
    r = _cli("-t", tree, "-i", str(fa), "-o", str(a))
    assert r.returncode == 0, r.stderr[-2000:]
    r = _cli("-t", tree, "-i", str(fa), "-o", str(b), "-m", "1000000")
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Decomposed the tree" not in r.stderr and "level kernel:" in r.stderr
    assert a.read_bytes() == b.read_bytes()


def _against_the_oracle(tmp_path, family):
    tree, fasta, seq_type, m, flags = family(str(tmp_path))
    want = SO.run(tree, fasta, seq_type, m, SO.build_dump(str(tmp_path)), flags=flags)
    out = tmp_path / "o.aln"
    r = _cli("-t", tree, "-i", fasta, "-o", str(out), "--type", seq_type, "-m", str(m), "-v", *flags)
    assert r.returncode == 0, r.stderr[-2000:]
    assert out.read_bytes() == SO.to_bytes(want.records)
    subtrees, rows, _, cells_a, cells_b, _ = _totals(r.stderr)
    assert (subtrees, rows, cells_a, cells_b) == (want.n_parts, len(want.records), want.cells_a, want.cells_b)
    assert _merge_levels(r.stderr) == want.pairs_per_level
    assert _sources(r.stderr) == want.sources
    return want, r


def test_protein_family_with_an_excluded_sequence(gpu, tmp_path):
    """60 x 300 aa at -m 16 with --filter: one sequence far off its subtree's median length is excluded from its subtree's alignment, from
    its profile and from the output; the first merge level holds two pairs."""
    want, r = _against_the_oracle(tmp_path, SC.protein_family)
    assert len(want.records) == 59 and b"s20" not in [n for n, _ in want.records]
    assert want.pairs_per_level[0] == 2


def test_cached_and_weighted_profiles_in_one_run(gpu, tmp_path):
    """--test-cal-profile-th 6: two subtrees hand their root's cached profile on (twl_store_write_cache), two have theirs summed on the device
    (twl_store_weighted_columns); which was taken is read from the -v output."""
    want, r = _against_the_oracle(tmp_path, SC.mixed_profile_family)
    assert sorted(want.sources.values()) == ["cached", "cached", "weighted", "weighted"]
    assert r.stderr.count("profile: cached msaFreq") == 2 and r.stderr.count("profile: weighted columns") == 2
