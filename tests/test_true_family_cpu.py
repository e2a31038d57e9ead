"""tools/true_family.py: a synthetic family with the alignment that is true by construction.  The true rows without their gaps are the FASTA
records, all rows have one width, no column is all gaps, the tree is one the command line reads, the oracle finds the truth equal to itself,
and the family is a function of its seed.  No GPU needed."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import compare_oracle as CO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "twilight_amd", "twilight-mi355x")


def _tool():
    spec = importlib.util.spec_from_file_location("true_family", os.path.join(ROOT, "tools", "true_family.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def family():
    return _tool().make_true_family(40, 300, seed=7, sub=0.03, indel=0.01)


def test_rows_degapped_are_the_records(family):
    _, seqs, rows = family
    assert [n for n, _ in seqs] == [n for n, _ in rows] == [f"s{k}" for k in range(40)]
    for (_, s), (_, r) in zip(seqs, rows):
        assert r.replace("-", "") == s and set(s) <= set("ACGT")


def test_one_width_and_no_column_of_gaps(family):
    _, seqs, rows = family
    W = len(rows[0][1])
    assert all(len(r) == W for _, r in rows)
    m = np.frombuffer("".join(r for _, r in rows).encode(), dtype=np.uint8).reshape(len(rows), W)
    assert (m != 0x2D).any(axis=0).all()
    assert W > 300 and any("-" in r for _, r in rows), "indels happened: the truth is wider than the root and has gaps"
    assert len({len(s) for _, s in seqs}) > 1


def test_homologous_letters_mostly_agree(family):
    """Columns hold sites of one ancestry: at these rates most columns with several letters are dominated by one letter."""
    _, _, rows = family
    m = np.frombuffer("".join(r for _, r in rows).encode(), dtype=np.uint8).reshape(len(rows), -1)
    full = [c for c in range(m.shape[1]) if (m[:, c] != 0x2D).sum() >= 20]
    agree = [np.bincount(m[:, c][m[:, c] != 0x2D]).max() / (m[:, c] != 0x2D).sum() for c in full]
    assert len(full) > 100 and np.mean(agree) > 0.7


def test_truth_against_itself(family):
    _, _, rows = family
    E = [r.encode() for _, r in rows]
    cols = CO.per_column_np(E, E)
    t = CO.totals(cols)
    assert t["shared"] == t["pairs_out"] == t["pairs_ref"] > 0 and t["recovered"] == t["ref_columns"] > 0
    assert " SP 1.000000 modeler 1.000000 " in CO.report(cols, len(E), 0, 0)
    small = CO.agree(E[:5], E[:5])
    assert CO.totals(small)["shared"] == CO.totals(small)["pairs_ref"]


def test_deterministic_for_its_seed():
    tf = _tool()
    a, b, c = tf.make_true_family(12, 120, seed=3), tf.make_true_family(12, 120, seed=3), tf.make_true_family(12, 120, seed=4)
    assert a == b and a != c


def test_the_main_writes_three_files_the_command_line_reads(built, tmp_path):
    """t.nwk, s.fa, true.aln; with no device visible a run on them reads the tree and the sequences without complaint and stops at twl_init."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "true_family.py"), str(tmp_path / "fam"), "--leaves", "9", "--length", "80", "--seed", "2", "--indel", "0.02"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    fam = tmp_path / "fam"
    assert sorted(os.listdir(fam)) == ["s.fa", "t.nwk", "true.aln"]
    names, rows = CO.read_alignment(fam / "true.aln")
    snames, seqs = CO.read_alignment(fam / "s.fa")
    assert names == snames == [f"s{k}" for k in range(9)] and all(rows[n].replace(b"-", b"") == seqs[n] for n in names)
    nwk = (fam / "t.nwk").read_text()
    assert nwk.count("(") == 8 and all(f"s{k}:" in nwk for k in range(9))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    run = subprocess.run([EXE, "-t", str(fam / "t.nwk"), "-i", str(fam / "s.fa"), "-o", str(tmp_path / "o.aln")], capture_output=True, text=True, timeout=60, env=env)
    assert run.returncode == 1 and "twl_init failed" in run.stderr, run.stderr
    assert "Number : 9" in run.stderr and "-> 9 (after pruning)" in run.stderr and "Missing s" not in run.stderr, "every leaf of the tree has its record"
