"""The CPU restatement of the subtree mode (tests/subtree_oracle.py) held to what must be true of any run of the mode, and to the committed
fixture tests/golden/subtree_expected.json that the GPU suite holds the product's command line to; and the proof that the inputs of the
weighted-profile kernel test depend on the order of the additions.  No GPU needed."""
import gzip
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import subtree_cases as SC
import subtree_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EXPECTED = json.load(open(os.path.join(GOLDEN, "subtree_expected.json")))


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("subtree_oracle"))
    return d, SO.build_dump(d)


@pytest.fixture(scope="module")
def sample_runs(work):
    """The restatement on both sample families, once for all tests of this file."""
    d, exe = work
    runs = {}
    for case, fx in EXPECTED.items():
        fa = os.path.join(d, case + ".fa")
        with open(fa, "wb") as f:
            f.write(gzip.open(os.path.join(GOLDEN, fx["sequences"])).read())
        seqs = {}
        for line in open(fa):
            if line.startswith(">"):
                name = line[1:].strip()
                seqs[name] = ""
            else:
                seqs[name] += line.strip()
        runs[case] = (SO.run(os.path.join(GOLDEN, fx["tree"]), fa, "n", fx["max_subtree"], exe), seqs)
    return runs


def test_a_tree_that_is_not_split_is_the_plain_replay(built, work):
    """-m >= the number of leaves: one partition, and the restatement is oracle/msa_replay.py on oracle/schedule_dump, byte for byte."""
    d, exe = work
    tree, fasta, seq_type, _, _ = SC.mixed_profile_family(d)
    for m in (40, 1000000):
        r = SO.run(tree, fasta, seq_type, m, exe)
        assert r.n_parts == 1 and set(r.leaf_grp.values()) == {0}
        dump = subprocess.run([os.path.join(ROOT, "oracle", "schedule_dump"), "-t", tree, "-i", fasta, "-o", "x", "--type", seq_type], capture_output=True, text=True, check=True)
        with open(os.path.join(d, "plain.json"), "w") as f:
            f.write(dump.stdout)
        plain = os.path.join(d, "plain.aln")
        p = subprocess.run([sys.executable, os.path.join(ROOT, "oracle", "msa_replay.py"), os.path.join(d, "plain.json"), plain], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-2000:]
        assert SO.to_bytes(r.records) == open(plain, "rb").read()
    assert SO.run(tree, fasta, seq_type, 39, exe).n_parts == 2


@pytest.mark.parametrize("case", sorted(EXPECTED))
def test_sample_family_invariants_and_fixture(sample_runs, case):
    r, seqs = sample_runs[case]
    fx = EXPECTED[case]
    # every output row degapped is its input sequence; all rows have one width; every sequence is there once
    assert sorted(n.decode() for n, _ in r.records) == sorted(seqs)
    for name, row in r.records:
        assert len(row) == r.width
        assert row.replace(b"-", b"").replace(b".", b"").decode() == seqs[name.decode()]
    # the rows of each subtree, without the columns that are all-gap inside that subtree, are that subtree's own alignment from the replay;
    # subtrees in ascending index, rows in input order
    at = 0
    for k, rep in zip(sorted(r.sub_len), r.replays):
        n = rep.root.aln_len
        own = [(s["name"].encode(), row[:n]) for s, row, lq in zip(rep.seqs, rep.rows, rep.low_q) if not lq]
        got = r.records[at: at + len(own)]
        at += len(own)
        assert [nm for nm, _ in got] == [nm for nm, _ in own]
        block = np.array([np.frombuffer(row, dtype=np.uint8) for _, row in got])
        keep = ~np.all(block == ord("-"), axis=0)
        own_block = np.array([np.frombuffer(row, dtype=np.uint8) for _, row in own])
        own_keep = ~np.all(own_block == ord("-"), axis=0)
        assert np.array_equal(block[:, keep], own_block[:, own_keep]), f"subtree {k}"
        assert {s["name"] for s in rep.seqs} == {leaf for leaf, g in r.leaf_grp.items() if g == k}
    assert at == len(r.records)
    # the committed fixture
    assert r.n_parts == fx["subtrees"] and {str(k): v for k, v in r.sub_len.items()} == fx["subtree_length"]
    assert dict(sorted(r.leaf_grp.items())) == fx["partition"]
    assert r.width == fx["width"] and len(r.records) == fx["rows"]
    assert hashlib.md5(SO.to_bytes(r.records)).hexdigest() == fx["md5"]
    assert (r.cells_a, r.cells_b, r.pairs_per_level) == (fx["band_cells_subtrees"], fx["band_cells_merge"], fx["merge_pairs_per_level"])
    assert {str(k): v for k, v in r.sources.items()} == fx["profile_source"]


def test_the_roots_list_holds_every_sequence_twice(sample_runs):
    """What storeSubtreeProfile walks (progressive.cpp:222-228): the members of the root, then every sequence of the subtree again; alnNum is
    the length of that list."""
    r, _ = sample_runs["sars_20_m8"]
    for rep in r.replays:
        n = len(rep.rows)
        assert len(rep.root.seqs) == 2 * n and sorted(rep.root.seqs[:n]) == list(range(n)) and rep.root.seqs[n:] == list(range(n))
        rows, weights = SO.profile_entries(rep)
        assert len(rows) == 2 * n and len(weights) == 2 * n
        once = SC.weighted_profile(rows[:n], weights[:n], "n")
        twice = SC.weighted_profile(rows, weights, "n")
        assert np.allclose(twice, 2 * once, rtol=1e-5)      # (bit for bit only where the weights add up exactly, as this tree's do: it has no branch lengths)


@pytest.mark.parametrize("seq_type", ["n", "p"])
def test_kernel_test_inputs_are_order_sensitive(seq_type):
    """Adding the rows of a kernel-test case in reversed order changes at least one fp32 entry (for every case of three rows or more: two
    numbers add up the same in either order), so tests/test_gpu_subtree_kernel.py sees a kernel that sums in another order."""
    rows = SC.store_rows(seq_type)
    new = SC.rewritten_rows(seq_type, rows)
    rows = [new.get(i, r) for i, r in enumerate(rows)]
    assert len(new) == len(rows) // 2
    for L in SC.COLUMNS:
        for n in SC.ROWS:
            ids, w = SC.case(seq_type, L, n)
            assert len(set(ids)) == n and all(len(rows[i]) == L for i in ids)
            assert np.all(w > 0) and w.dtype == np.float32 and not np.any(np.log2(w.astype(np.float64)) == np.round(np.log2(w.astype(np.float64))))
            if n >= 65:
                assert w.max() / w.min() > 100          # three decades drawn, more than two present
            fwd = SC.weighted_profile([rows[i] for i in ids], w, seq_type)
            rev = SC.weighted_profile([rows[i] for i in ids[::-1]], w[::-1], seq_type)
            assert np.allclose(fwd, rev, rtol=1e-4)
            if n >= 65 and L > 1:
                assert not np.array_equal(fwd.view(np.uint32), rev.view(np.uint32)), (L, n)
            if L > SC.SAME_LETTER_COLUMN:
                assert np.count_nonzero(fwd[SC.SAME_LETTER_COLUMN]) == 1
    # the single column, all rows: one chain of 300 additions
    ids, w = SC.case(seq_type, 1, 300)
    fwd = SC.weighted_profile([rows[i] for i in ids], w, seq_type)
    rev = SC.weighted_profile([rows[i] for i in ids[::-1]], w[::-1], seq_type)
    assert not np.array_equal(fwd.view(np.uint32), rev.view(np.uint32))
