"""The partition of the guide tree for -m N (twilight_amd/csrc/host/partition.cpp: PartitionInfo::partitionTree, bipartition, the centroid search,
constructTreeFromPartitions) on trees small enough to work out by hand, and against the Python restatement of tests/subtree_oracle.py, which
shares no code with it.  No GPU needed.

The rule (reference partitionInfo.cpp:7-110, minPartitionSize 0): a subtree with more than N leaves is cut at the internal node whose number
of leaves inside the subtree is closest to half of the subtree's (at least 1); the first such node in post-order wins; a leaf is never cut
off; the part cut off gets the next free index and is cut further before the rest is; a subtree whose best cut is its own root stays."""
import os
import re
import subprocess

import pytest

import subtree_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "twilight_amd", "csrc", "host")

# internal nodes are node_1, node_2, ... in the order of their '('
CATERPILLAR_7 = "((((((a,b),c),d),e),f),g);"        # node_1 .. node_6 from the root down; node_k has 8 - k leaves
BALANCED_8 = "(((a,b),(c,d)),((e,f),(g,h)));"       # node_2 = abcd (node_3 = ab, node_4 = cd), node_5 = efgh (node_6 = ef, node_7 = gh)
STAR_5 = "(a,b,c,d,e);"

# (leaf -> subtree, subtree -> root, tree of subtrees), worked out by hand
KNOWN = {
    # caterpillar, 7 leaves: half = 3, node_5 (abc) is exact -> subtree 1.  Then per N:
    ("cat7", 6): ("a:1,b:1,c:1,d:0,e:0,f:0,g:0", "0:node_1,1:node_5", "node_1(node_5)"),
    #   N = 3: the rest (d e f g under node_1..node_4) has 4 leaves, half = 2: node_4 holds d alone (1), node_3 holds d e (2, exact) -> subtree 2
    ("cat7", 3): ("a:1,b:1,c:1,d:2,e:2,f:0,g:0", "0:node_1,1:node_5,2:node_3", "node_1(node_3(node_5))"),
    #   N = 2: subtree 1 (abc, half 1) is cut first: node_6 (ab, off by 1) beats node_5 (off by 2) -> subtree 2, c stays in 1;
    #          then the rest as for N = 3, with the index 3
    ("cat7", 2): ("a:2,b:2,c:1,d:3,e:3,f:0,g:0", "0:node_1,1:node_5,2:node_6,3:node_3", "node_1(node_3(node_5(node_6)))"),
    #   N = 1: as N = 2 down to subtrees of two leaves; ab (node_6) cannot be cut (its only internal node is its root); c alone is fine;
    #          d e under node_3 (half 1): node_4 (d alone, exact) -> subtree 4, e stays in 3; f g under node_1 (half 1): node_2 (f alone) -> 5
    ("cat7", 1): ("a:2,b:2,c:1,d:4,e:3,f:5,g:0", "0:node_1,1:node_5,2:node_6,3:node_3,4:node_4,5:node_2", "node_1(node_2(node_3(node_4(node_5(node_6)))))"),
    ("cat7", 7): ("a:0,b:0,c:0,d:0,e:0,f:0,g:0", "0:node_1", "node_1"),
    ("cat7", 8): ("a:0,b:0,c:0,d:0,e:0,f:0,g:0", "0:node_1", "node_1"),
    # balanced, 8 leaves: half = 4, node_2 (abcd) is the first exact node -> subtree 1
    ("bal8", 7): ("a:1,b:1,c:1,d:1,e:0,f:0,g:0,h:0", "0:node_1,1:node_2", "node_1(node_2)"),
    #   N = 3 and N = 2: subtree 1 (half 2): node_3 (ab) exact -> 2; the rest of subtree 0 (efgh, half 2): node_6 (ef) -> 3
    ("bal8", 3): ("a:2,b:2,c:1,d:1,e:3,f:3,g:0,h:0", "0:node_1,1:node_2,2:node_3,3:node_6", "node_1(node_2(node_3),node_6)"),
    ("bal8", 2): ("a:2,b:2,c:1,d:1,e:3,f:3,g:0,h:0", "0:node_1,1:node_2,2:node_3,3:node_6", "node_1(node_2(node_3),node_6)"),
    #   N = 1: every cherry is cut off whole (it cannot be cut itself); node_2 and node_1 are left as subtrees without a leaf
    ("bal8", 1): ("a:2,b:2,c:3,d:3,e:4,f:4,g:5,h:5", "0:node_1,1:node_2,2:node_3,3:node_4,4:node_6,5:node_7", "node_1(node_2(node_3,node_4),node_6,node_7)"),
    ("bal8", 8): ("a:0,b:0,c:0,d:0,e:0,f:0,g:0,h:0", "0:node_1", "node_1"),
    ("bal8", 9): ("a:0,b:0,c:0,d:0,e:0,f:0,g:0,h:0", "0:node_1", "node_1"),
    # a star: the root is the only internal node, so the best cut is the root itself: nothing is split and no subtree is recorded
    ("star5", 1): ("a:-1,b:-1,c:-1,d:-1,e:-1", "-", "-"),
    ("star5", 2): ("a:-1,b:-1,c:-1,d:-1,e:-1", "-", "-"),
    ("star5", 3): ("a:-1,b:-1,c:-1,d:-1,e:-1", "-", "-"),
    ("star5", 4): ("a:-1,b:-1,c:-1,d:-1,e:-1", "-", "-"),
    ("star5", 5): ("a:0,b:0,c:0,d:0,e:0", "0:node_1", "node_1"),
    ("star5", 6): ("a:0,b:0,c:0,d:0,e:0", "0:node_1", "node_1"),
}
TREES = {"cat7": CATERPILLAR_7, "bal8": BALANCED_8, "star5": STAR_5}


@pytest.fixture(scope="module")
def kats(tmp_path_factory):
    d = tmp_path_factory.mktemp("partition")
    exe = d / "partition_kats"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "partition_kats.cpp"),
                           os.path.join(HOST, "phylo.cpp"), os.path.join(HOST, "partition.cpp")])

    def run(tree_file, ms):
        r = subprocess.run([str(exe), str(tree_file)] + [str(m) for m in ms], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out = {}
        for line in r.stdout.splitlines():
            if line.startswith("PARTITION"):
                kv = dict(x.split("=", 1) for x in line.split()[1:])
                out[int(kv["m"])] = kv
        return out

    return d, run


def _python_answer(text, m):
    leaf_grp, roots, (top, children), n = SO.partition_newick(text, m)
    _, nodes = SO.parse_newick(text)

    def show(name):
        return name + ("(" + ",".join(show(c) for c in children[name]) + ")" if children[name] else "")

    leaves = ",".join("%s:%d" % (k, leaf_grp[k]) for k, v in nodes.items() if not v.children)
    return n, leaves, ",".join("%d:%s" % (g, roots[g]) for g in sorted(roots)) or "-", show(top) if top else "-"


@pytest.mark.parametrize("tree", sorted(TREES))
def test_known_answers(kats, tree):
    """-m 1, 2, 3, n - 1, n, n + 1 on each tree: the subtree of every leaf, the root of every subtree, the tree of subtrees."""
    d, run = kats
    f = d / (tree + ".nwk")
    f.write_text(TREES[tree] + "\n")
    ms = sorted(m for t, m in KNOWN if t == tree)
    n = TREES[tree].count(",") + 1
    assert ms == sorted({1, 2, 3, n - 1, n, n + 1})
    got = run(f, ms)
    for m in ms:
        leaves, roots, subtree_tree = KNOWN[(tree, m)]
        kv = got[m]
        assert kv["leaves"] == leaves, (tree, m)
        assert re.sub(r"(\d+:node_\d+):\d+", r"\1", kv["roots"]) == roots, (tree, m)
        assert kv["tree"] == subtree_tree, (tree, m)
        assert int(kv["parts"]) == (0 if roots == "-" else roots.count(",") + 1)
        assert _python_answer(TREES[tree], m) == (int(kv["parts"]), leaves, roots, subtree_tree), ("the Python restatement", tree, m)
        if m >= n:
            assert int(kv["parts"]) == 1 and set(x.split(":")[1] for x in leaves.split(",")) == {"0"}


def test_leaf_counts_of_the_subtrees(kats):
    """partitionsRoot keeps the number of leaves of every subtree as it stands after the last cut."""
    d, run = kats
    f = d / "cat7.nwk"
    f.write_text(CATERPILLAR_7 + "\n")
    got = run(f, [1, 2, 3])
    assert got[3]["roots"] == "0:node_1:2,1:node_5:3,2:node_3:2"
    assert got[2]["roots"] == "0:node_1:2,1:node_5:1,2:node_6:2,3:node_3:2"
    assert got[1]["roots"] == "0:node_1:1,1:node_5:1,2:node_6:2,3:node_3:1,4:node_4:1,5:node_2:1"


def test_a_best_cut_at_the_root_stops_without_splitting(kats):
    """breakEdge == root: a cherry at -m 1 stays whole (inside bal8 above); at the top of the tree nothing at all is recorded."""
    d, run = kats
    f = d / "star5.nwk"
    f.write_text(STAR_5 + "\n")
    got = run(f, [4])[4]
    assert got["parts"] == "0" and got["roots"] == "-" and got["tree"] == "-"
    f = d / "cherry.nwk"
    f.write_text("(a,b);\n")
    got = run(f, [1])[1]
    assert got["parts"] == "0" and got["leaves"] == "a:-1,b:-1"


@pytest.mark.parametrize("m", [50, 100, 333])
def test_port_and_restatement_agree_on_rnasim(kats, m):
    d, run = kats
    tree = os.path.join(ROOT, "tests", "golden", "RNASim.nwk")
    kv = run(tree, [m])[m]
    n, leaves, roots, subtree_tree = _python_answer(open(tree).read().splitlines()[0], m)
    assert n > 1 and int(kv["parts"]) == n
    assert kv["leaves"] == leaves
    assert re.sub(r"(\d+:node_\d+):\d+", r"\1", kv["roots"]) == roots
    assert kv["tree"] == subtree_tree
    sizes = [int(x.split(":")[2]) for x in kv["roots"].split(",")]
    assert sum(sizes) == 579 and max(sizes) <= m
