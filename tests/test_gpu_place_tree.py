"""Placement along a tree on the MI355X (`twilight-mi355x -t T -a A -i S -o O --place-on-tree`, twilight_amd/csrc/host/place_tree.cpp) through the
command line, against the CPU restatement of the mode (tests/place_tree_oracle.py), byte for byte: the committed fixture
tests/golden/place_tree_expected.json for the reference's own sample, the restatement run in the test for small families.  Every CLI run has
its own time limit."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

import place_tree_cases as PC
import place_tree_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
EXE = os.path.join(ROOT, "twilight_amd", "twilight-mi355x")
EXPECTED = json.load(open(os.path.join(GOLDEN, "place_tree_expected.json")))

pytestmark = pytest.mark.gpu


def _cli(*args, timeout=120):
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=timeout)


def _records(path):
    out = []
    for line in open(path, "rb").read().splitlines():
        if line.startswith(b">"):
            out.append([line[1:], b""])
        else:
            out[-1][1] += line
    return [(n, r) for n, r in out]


@pytest.fixture(scope="module")
def work(built, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("place_tree"))
    return d, PO.build_dump(d)


def _place(d, tree, backbone, new, seq_type, flags, stem):
    out = os.path.join(d, stem + ".out.aln")
    r = _cli("-t", tree, "-a", backbone, "-i", new, "-o", out, "--type", seq_type, "--place-on-tree", "--check", *flags)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "WARNING: --check" not in r.stderr and "did not match" not in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    return out, r


def _invariants(records, doc, derived):
    """What does not rest on the oracle's alignment: one width; every row degapped is its input degapped; for every group of the dump, its
    output rows without the columns that are all-gap inside the group equal its squeezed input rows."""
    rows = dict(records)
    widths = {len(r) for _, r in records}
    assert len(widths) == 1
    by_name = {s["name"].encode(): s for s in doc["sequences"]}
    for name, row in records:
        want = by_name[name]["seq"].encode("latin-1").replace(b"-", b"").replace(b".", b"")
        assert row.replace(b"-", b"").replace(b".", b"") == want, name
    for node, g in doc["groups"].items():
        names = [doc["sequences"][s]["name"].encode() for s in g["ids"]]
        assert PO.squeeze_group([rows[n] for n in names]) == PO.squeeze_group([by_name[n]["seq"].encode("latin-1") for n in names]), node


def _against_the_oracle(work, inputs, flags, stem, dump_flags=None):
    d, exe = work
    tree, backbone, new, seq_type, _ = inputs
    doc = PO.dump(exe, tree, backbone, new, seq_type, list(flags if dump_flags is None else dump_flags))
    want = PO.run(doc, flags=list(flags))
    out, r = _place(d, tree, backbone, new, seq_type, flags, stem)
    got = _records(out)
    assert [n for n, _ in got] == [n for n, _ in want.records]
    assert open(out, "rb").read() == PO.to_bytes(want.records)
    _invariants(got, doc, want.derived)
    return want, r, doc


def test_hand_family(gpu, work):
    """A dozen sequences of 60 columns; -v prints the phase line of the mode."""
    want, r, doc = _against_the_oracle(work, PC.hand_family(work[0]), ("-v",), "hand")
    line = [l for l in r.stderr.splitlines() if l.startswith("Placement-on-tree phases:")]
    assert len(line) == 1 and "groups %d, rows 8, columns %d -> " % (len(doc["groups"]), 60 * len(doc["groups"])) in line[0], r.stderr[-1500:]
    assert "squeeze kernels" in line[0] and "levels %d" % len(doc["levels"]) in line[0]
    assert len(want.records) == 12 and want.width >= 50


@pytest.mark.parametrize("flags", [(), ("--rooted",), ("-r", "1"), ("--gap-open", "-30", "--gap-extend", "-3"), ("-w",)], ids=["default", "rooted", "r1", "gaps", "wildcard"])
def test_hand_family_flags(gpu, work, flags):
    _against_the_oracle(work, PC.hand_family(work[0]), flags, "hand_" + "_".join(f.strip("-") for f in flags))


@pytest.mark.parametrize("variant", sorted(EXPECTED))
def test_rnasim_sample_against_the_golden_file(gpu, work, variant):
    """The reference's own sample for the mode: 100 new sequences into 479 backbone rows of 3864 columns."""
    import make_place_tree_expected as MK

    d, exe = work
    fx = EXPECTED[variant]
    tree, backbone, new = MK.sample_inputs(d)
    out, r = _place(d, tree, backbone, new, "n", fx["flags"], "rnasim_" + variant)
    got = _records(out)
    assert len(got) == fx["rows"] and {len(row) for _, row in got} == {fx["width"]}
    assert hashlib.md5(open(out, "rb").read()).hexdigest() == fx["md5"]
    doc = PO.dump(exe, tree, backbone, new, "n", fx["flags"])
    assert len(doc["groups"]) == fx["groups"] and len(doc["levels"]) == fx["levels"]
    _invariants(got, doc, None)


def test_protein_family(gpu, work):
    _against_the_oracle(work, PC.family(work[0], "prot", seq_type="p", n_old=11, n_new=5, length=70, width=90, seed=5), (), "prot")
    _against_the_oracle(work, PC.family(work[0], "prot62", seq_type="p", n_old=11, n_new=5, length=70, width=90, seed=5), ("-b", "45"), "prot45")


def test_new_sequences_that_sit_together(gpu, work):
    """The new names end the tree's leaf list: inner nodes without members, paired as in the default mode."""
    _against_the_oracle(work, PC.family(work[0], "tail", n_old=9, n_new=6, seed=8, new_last=True), (), "tail")


def test_a_deferred_new_sequence_runs_the_second_pass_on_the_placement_tree(gpu, work):
    """One new sequence is over --max-ambig: it is deferred and joins the root in the deferred pass."""
    inputs = PC.family(work[0], "ambig", n_old=8, n_new=4, seed=3, ambiguous=(1,))
    want, r, doc = _against_the_oracle(work, inputs, (), "ambig")
    assert sum(s["low_quality"] for s in doc["sequences"]) == 1 and "Realign profiles that have been deferred" in r.stderr
    assert len(want.records) == 12


def test_the_same_with_filter(gpu, work):
    inputs = PC.family(work[0], "ambigf", n_old=8, n_new=4, seed=3, ambiguous=(1,))
    want, r, doc = _against_the_oracle(work, inputs, ("--filter",), "ambig_filter")
    assert len(want.records) == 11 and b"new01" not in [n for n, _ in want.records]


def test_a_single_new_sequence(gpu, work):
    for k, flags in enumerate(((), ("--rooted",))):
        want, r, doc = _against_the_oracle(work, PC.family(work[0], "single", n_old=7, n_new=1, seed=13), flags, "single%d" % k)
        assert len(want.records) == 8 and sum(v["new"] for v in doc["tree"].values()) == 1


def test_without_the_flag_a_and_t_still_exit_1(gpu, work):
    tree, backbone, new, seq_type, _ = PC.hand_family(work[0])
    out = os.path.join(work[0], "refused.aln")
    r = _cli("-t", tree, "-a", backbone, "-i", new, "-o", out, timeout=60)
    assert r.returncode == 1 and "placement with a tree" in r.stderr and "not supported yet" in r.stderr and not os.path.exists(out)
