"""The CPU restatement of placement along a tree (tests/place_tree_oracle.py) held to hand-derived examples of its marks, groups, squeeze and
schedule, to the committed fixture tests/golden/place_tree_expected.json that the GPU suite holds the product's command line to, and -- through
tests/place_tree_dump.cpp -- to what the product's host half says of the same inputs.  No GPU needed."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

import place_tree_cases as PC
import place_tree_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
EXPECTED = json.load(open(os.path.join(GOLDEN, "place_tree_expected.json")))
F = np.float32


def _tree(spec, new):
    """{name: children} -> the dump's tree; a name without children is a leaf."""
    names = set(spec) | {c for v in spec.values() for c in v}
    return {n: {"leaf": int(n not in spec), "new": int(n in new), "children": list(spec.get(n, []))} for n in names}


# ---- hand-derived ----

def test_marks_groups_and_schedule_of_a_chain():
    """One new leaf n1 beside b1; the rest of the backbone hangs under the root's other, unplaced child.  Placed: n1 and its two ancestors.  The
    root's group is what lies below node_3, depth first in child order; node_2's is b1.  Both inner nodes bring members and have one placed child:
    each is paired with that child, the root one level later."""
    t = _tree({"node_1": ["node_2", "node_3"], "node_2": ["b1", "n1"], "node_3": ["node_4", "b4"], "node_4": ["b2", "b3"]}, {"n1"})
    placed = PO.placed_marks(t, "node_1")
    assert placed == {"n1", "node_2", "node_1"}
    ids = {"b1": 0, "b2": 1, "b3": 2, "b4": 3, "n1": 4}
    assert PO.group_of(t, placed, "node_1", ids) == [1, 2, 3] and PO.group_of(t, placed, "node_2", ids) == [0] and PO.group_of(t, placed, "n1", ids) == []
    nodes = PO.placement_tree(t, "node_1", placed)
    assert {k: v["children"] for k, v in nodes.items()} == {"node_1": ["node_2"], "node_2": ["n1"], "n1": []}
    assert PO.schedule_mode0(nodes, "node_1", lambda n: n in ("node_1", "node_2")) == [[("node_2", "n1")], [("node_1", "node_2")]]


def test_schedule_pairs_placed_siblings_and_walks_in_reverse_preorder():
    """Two cherries (new leaf, backbone leaf) under the root: every inner node is placed, the root brings no members.  The schedule pops the
    pre-order walk from its end: node_3's pair comes before node_2's on level 0; the root pairs its two children one level up."""
    t = _tree({"node_1": ["node_2", "node_3"], "node_2": ["n1", "b1"], "node_3": ["n2", "b2"]}, {"n1", "n2"})
    placed = PO.placed_marks(t, "node_1")
    assert placed == {"n1", "n2", "node_1", "node_2", "node_3"}
    ids = {"b1": 0, "b2": 1, "n1": 2, "n2": 3}
    assert [PO.group_of(t, placed, n, ids) for n in ("node_1", "node_2", "node_3")] == [[], [0], [1]]
    nodes = PO.placement_tree(t, "node_1", placed)
    assert PO.schedule_mode0(nodes, "node_1", lambda n: n in ("node_2", "node_3")) == [[("node_3", "n2"), ("node_2", "n1")], [("node_2", "node_3")]]


def test_schedule_splices_a_unary_node_without_members():
    """A node whose only child is placed and that brings no members (a unary node of a --rooted tree) gives its place to that child."""
    t = _tree({"node_1": ["node_2", "n3"], "node_2": ["node_3"], "node_3": ["n1", "n2"]}, {"n1", "n2", "n3"})
    placed = PO.placed_marks(t, "node_1")
    nodes = PO.placement_tree(t, "node_1", placed)
    assert PO.schedule_mode0(nodes, "node_1", lambda n: False) == [[("n1", "n2")], [("node_3", "n3")]]
    assert nodes["node_1"]["children"] == ["node_3", "n3"] and nodes["node_3"]["parent"] == "node_1"


def test_schedule_of_a_node_with_three_placed_children_and_members():
    """Children are paired left to right, the odd one joins the next round; then the node itself, with its members, meets its first child."""
    t = _tree({"node_1": ["n1", "n2", "n3", "b1"]}, {"n1", "n2", "n3"})
    placed = PO.placed_marks(t, "node_1")
    nodes = PO.placement_tree(t, "node_1", placed)
    assert PO.schedule_mode0(nodes, "node_1", lambda n: n == "node_1") == [[("n1", "n2")], [("n1", "n3")], [("node_1", "n1")]]


def test_squeeze_group_by_hand():
    """Only '-' counts: '.' keeps a column; one letter in any row keeps it; every row loses the same columns."""
    assert PO.squeeze_group([b"A-.-", b"--.-", b"C--G"]) == [b"A.-", b"-.-", b"C-G"]
    assert PO.squeeze_group([b"----"]) == [b""] and PO.squeeze_group([b"", b""]) == [b"", b""]
    assert PO.squeeze_group([b"-a-", b"---"]) == [b"a", b"-"]
    assert PO.squeeze_group([b"ACGT"]) == [b"ACGT"]


def test_group_weight_is_summed_in_member_order_in_fp32():
    w = [F(0.1), F(1.0e8), F(-1.0e8), F(0.3)]
    num, a = PO.group_num_weight([0, 1, 2, 3], w)
    _, b = PO.group_num_weight([1, 2, 0, 3], w)
    assert num == 4 and a == F(0.3) and b == F(F(0.1) + F(0.3)) and a != b


# ---- the dump of the product's host half against the restatement ----

@pytest.fixture(scope="module")
def work(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("place_tree_oracle"))
    return d, PO.build_dump(d)


def _invariants(res, seqs=None):
    """What must be true of any run of the mode: one width; every row degapped is its input degapped; every group's rows, without the columns that are
    all-gap inside the group, are its squeezed input rows."""
    rows = dict(res.records)
    d = res.replay
    for s in d.seqs:
        if s["name"].encode() not in rows:
            continue
        row = rows[s["name"].encode()]
        assert len(row) == res.width
        want = s["seq"].encode("latin-1").replace(b"-", b"").replace(b".", b"") if seqs is None else seqs[s["name"]].replace(b"-", b"")
        assert row.replace(b"-", b"").replace(b".", b"") == want, s["name"]
    for name, ids in res.derived.groups.items():
        out = PO.squeeze_group([rows[d.seqs[s]["name"].encode()] for s in ids])
        assert out == [res.derived.rows[s] for s in ids], name


@pytest.mark.parametrize("variant", sorted(EXPECTED))
def test_the_oracle_reproduces_the_golden_file_and_the_dump_agrees(built, work, variant):
    """RNASim: 479 backbone rows, 100 new sequences.  run() holds marks, groups, weights and levels equal to the dump's before it aligns."""
    import make_place_tree_expected as MK

    d, exe = work
    fx = EXPECTED[variant]
    tree, backbone, new = MK.sample_inputs(d)
    r = PO.run(PO.dump(exe, tree, backbone, new, "n", fx["flags"]), flags=fx["flags"])
    assert (r.width, len(r.records), len(r.derived.groups), len(r.derived.levels)) == (fx["width"], fx["rows"], fx["groups"], fx["levels"])
    assert hashlib.md5(PO.to_bytes(r.records)).hexdigest() == fx["md5"]
    _invariants(r)
    # every backbone row lands in exactly one group; the new sequences are the placed leaves
    listed = sorted(s for ids in r.derived.groups.values() for s in ids)
    assert listed == list(range(479)) and len(r.replay.seqs) == 579


@pytest.mark.parametrize("case,flags", [("hand", ()), ("hand", ("--rooted",)), ("multi", ("--rooted",)), ("multi", ())])
def test_dump_equals_oracle_on_small_families(built, work, case, flags):
    d, exe = work
    tree, backbone, new, seq_type, seqs = (PC.hand_family if case == "hand" else PC.multifurcation)(d)
    doc = PO.dump(exe, tree, backbone, new, seq_type, list(flags))
    r = PO.run(doc, flags=list(flags))          # (asserts groups, weights, placement tree and levels equal to the dump's)
    _invariants(r, seqs)
    assert len(r.records) == len(seqs)
    if case == "hand":
        # the clade (b5, b6, b7) hangs under one unplaced node: one group, in the tree's order, and its ten all-gap columns are gone
        grp = [ids for ids in r.derived.groups.values() if set(ids) == {4, 5, 6}]
        assert grp == [[4, 5, 6]] and len(r.derived.rows[4]) <= 50
    else:
        assert r.derived.groups and (not flags or max(len(v["children"]) for v in doc["tree"].values()) == 5)
