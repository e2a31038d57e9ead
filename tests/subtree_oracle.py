"""tests/subtree_oracle.py -- CPU restatement of the subtree mode (the reference's `twilight -t T -i S -o O -m N`, twilight-main.cpp:129-192).

TEST INFRASTRUCTURE ONLY.  Written from the reference source; it shares no code with twilight_amd/csrc/host/{partition,subtrees}.cpp:
  1. the partition of the guide tree (partitionInfo.cpp:7-110 with minPartitionSize 0) and the tree of the subtrees' roots
     (phylogeny.cpp:13-39), on a Newick parser of its own (internal nodes are node_1, node_2, ... in the order of their '(')
  2. per subtree, in ascending index: the independent replay oracle/msa_replay.py (imported, unchanged) on what tests/subtree_dump.cpp
     prints for that subtree (the subtree's own tree, rerooted; its sequences with the weights of that tree; its level batches)
  3. per subtree the profile of SequenceDB::storeSubtreeProfile (sequencedb.cpp:122-138): the replay's root profile when it left one,
     otherwise the sum of the rows of the root's seqsIncluded, row by row IN THAT ORDER in fp32, each weighted by its sequence weight.
     The list is what progressive::updateAlignment leaves (progressive.cpp:222-228): the members the root had, then EVERY sequence of the
     subtree's database again (readSequences gives them all the subtree index -1, io.cpp:84 with tree.cpp:252), so a sequence is added
     twice, at two places of the order, and alnNum = the length of that list (tree.cpp:522).  Sequences that --filter excluded have no
     row of the alignment's length and are left out of the sum (the reference reads past their end); they still count in alnNum.
  4. the merge along the tree of subtrees: scheduling mode 1 (progressive.cpp:81-95 over node.cpp:58-71), every pair as the merge of two
     cached profiles (tests/merge_oracle.py: merge_pair, Maps), updateFrequency, alnNum / alnWeight / alnLen as alignment-helper.cpp:474-476
  5. output: subtrees in ascending index, rows in input order, every row through its subtree's map; low-quality rows left out
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
for _p in (_ROOT, os.path.join(_ROOT, "oracle"), _HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import level_oracle as LO  # noqa: E402
import merge_oracle as MO  # noqa: E402
import msa_replay as MR  # noqa: E402
import subtree_cases as SC  # noqa: E402

F = np.float32


# ---- 1. the tree and its partition ----

class TNode:
    def __init__(self, ident, parent):
        self.id, self.parent, self.children, self.grp = ident, parent, [], -1
        if parent is not None:
            parent.children.append(self)


def parse_newick(text):
    """Topology only.  Returns (root, nodes by name)."""
    text = text.strip().rstrip(";")
    nodes, stack, cur, n_internal, i, root = {}, [], None, 0, 0, None
    while i < len(text):
        c = text[i]
        if c == "(":
            n_internal += 1
            cur = TNode("node_%d" % n_internal, stack[-1] if stack else None)
            nodes[cur.id] = cur
            root = root or cur
            stack.append(cur)
            i += 1
        elif c == ")":
            stack.pop()
            i += 1
            while i < len(text) and text[i] not in ",()":      # the node's own label / branch length
                i += 1
        elif c == ",":
            i += 1
        else:
            j = i
            while j < len(text) and text[j] not in ",()":
                j += 1
            name = text[i:j].split(":")[0].strip().strip("'")
            if name:
                nodes[name] = TNode(name, stack[-1])
            i = j
    return root, nodes


def _leaves(node, grp):
    """getNumLeaves (partitionInfo.cpp:7-14)."""
    total, work = 0, [node]
    while work:
        n = work.pop()
        if n.grp != grp:
            continue
        if not n.children:
            total += 1
        work.extend(n.children)
    return total


def _centroid(root):
    """getCentroidEdge / updateCentroidEdge (partitionInfo.cpp:16-38): post-order, the first strictly better node wins, leaves never."""
    n = _leaves(root, root.grp)
    half = max(1, n // 2)
    best, imbalance = root, n
    order, work = [], [(root, False)]
    while work:
        node, done = work.pop()
        if node.grp != root.grp or not node.children:
            continue
        if done:
            order.append(node)
            continue
        work.append((node, True))
        for ch in reversed(node.children):
            work.append((ch, False))
    for node in order:
        d = abs(half - _leaves(node, root.grp))
        if d < imbalance:
            best, imbalance = node, d
    return best


def _set_group(node, old, new):
    work = [node]
    while work:
        n = work.pop()
        if n.grp != old:
            continue
        n.grp = new
        work.extend(n.children)


class Partition:
    """PartitionInfo (phylogeny.hpp:55-71): roots = {name of a subtree's root: leaves}; every node's grp is its subtree."""

    def __init__(self, max_size):
        self.max, self.num, self.roots = max_size, 0, {}

    def _bipartition(self, root, edge):
        """partitionInfo.cpp:54-74."""
        id1 = 0 if root.grp == -1 else root.grp
        id2 = 1 if root.grp == -1 else self.num + 1
        self.num += 1
        head = edge.parent
        while head.parent is not None and head.parent.grp == head.grp:
            head = head.parent
        old1 = head.grp
        _set_group(edge, edge.grp, id2)
        if head.grp == -1:
            _set_group(head, old1, id1)
        return head, edge

    def partition(self, root):
        """partitionInfo.cpp:76-110 (the recursion: the split-off part first, then the rest)."""
        total = _leaves(root, root.grp)
        if total <= self.max:
            if not self.roots:
                _set_group(root, root.grp, 0)
                self.roots[root.id] = _leaves(root, root.grp)
            return
        edge = _centroid(root)
        if edge is root:
            return
        t1, t2 = self._bipartition(root, edge)
        n1, n2 = _leaves(t1, t1.grp), _leaves(t2, t2.grp)
        self.roots[t2.id] = n2
        self.roots[t1.id] = n1
        if n2 > self.max:
            self.partition(t2)
        if n1 > self.max:
            self.partition(t1)


def subtree_tree(root, part):
    """constructTreeFromPartitions (phylogeny.cpp:13-39): (root name, {name: children names in order}) over the subtrees' roots."""
    children, top, work = {}, None, [(root, None)]
    while work:
        node, parent = work.pop()
        if node.id in part.roots:
            children[node.id] = []
            if parent is None:
                top = node.id
            else:
                children[parent].append(node.id)
            parent = node.id
        for ch in reversed(node.children):
            work.append((ch, parent))
    return top, children


def partition_newick(text, max_size):
    """(leaf -> subtree index, subtree index -> root name, (top, children) of the tree of subtrees, number of partitions)."""
    root, nodes = parse_newick(text)
    part = Partition(max_size)
    part.partition(root)
    leaf_grp = {k: n.grp for k, n in nodes.items() if not n.children}
    roots = {nodes[name].grp: name for name in part.roots}
    return leaf_grp, roots, subtree_tree(root, part), len(part.roots)


def schedule_mode1(top, children):
    """scheduling(root, levels, 1): collectPostOrder pushes a node, then its children first to last (node.cpp:58-71); the stack is popped
    from its top and every node but the root is paired with its parent, one level above the later of the two (progressive.cpp:81-95)."""
    pushed, work, parent = [], [top], {}
    while work:
        n = work.pop()
        pushed.append(n)
        for ch in reversed(children[n]):
            parent[ch] = n
            work.append(ch)
    order, levels = {}, []
    for n in reversed(pushed):
        if n not in parent:
            continue
        p = parent[n]
        lvl = max(order[n] + 1 if n in order else 0, order[p] + 1 if p in order else 0)
        order[n] = order[p] = lvl
        while len(levels) <= lvl:
            levels.append([])
        levels[lvl].append((p, n))
    return levels


# ---- 2. the dump of every subtree ----

DUMP_SOURCES = ("phylo.cpp", "seqdb_io.cpp", "helpers.cpp", "progressive.cpp", "driver.cpp", "partition.cpp")


def build_dump(out_dir):
    """tests/subtree_dump.cpp with the host sources it needs, by plain g++."""
    exe = os.path.join(out_dir, "subtree_dump")
    host = os.path.join(_ROOT, "twilight_amd", "csrc", "host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fopenmp", "-ffp-contract=off", "-Wall", "-o", exe, os.path.join(_HERE, "subtree_dump.cpp")] +
                          [os.path.join(host, f) for f in DUMP_SOURCES] + ["-lz"])
    return exe


def dump_subtrees(exe, tree, fasta, seq_type, max_subtree, flags=()):
    """One JSON document per subtree, in ascending subtree index (the format of oracle/schedule_dump, plus "subtree")."""
    r = subprocess.run([exe, "-t", tree, "-i", fasta, "-o", "x", "--type", seq_type, "-m", str(max_subtree)] + list(flags), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]


# ---- 3. the profile of a finished subtree ----

def subtree_profile(rep):
    """(msaFreq float32[alnLen][P], alnNum, "cached" | "weighted") of a replayed subtree."""
    root = rep.root
    if root.freq is not None:
        return np.asarray(root.freq, dtype=F), len(root.seqs), "cached"
    rows, weights = profile_entries(rep)
    return SC.weighted_profile(rows, weights, rep.type), len(root.seqs), "weighted"


def profile_entries(rep):
    """The rows and weights storeSubtreeProfile adds, in its order."""
    n = rep.root.aln_len
    excluded = [lq and not rep.no_filter for lq in rep.low_q]
    ids = [s for s in rep.root.seqs if not excluded[s]]
    return [rep.rows[s][:n] for s in ids], [rep.weight[s] for s in ids]


# ---- the mode ----

def replay_kwargs(flags):
    """The CLI flags the replay and the merge have to know (the others are already applied in the dump)."""
    kw, it = {}, iter(flags)
    names = {"-r": ("gappy", float), "--remove-gappy": ("gappy", float), "--match": ("match", float), "--mismatch": ("mismatch", float), "--transition": ("transition", float),
             "--gap-open": ("gap_open", float), "--gap-extend": ("gap_extend", float), "-b": ("blosum", int), "--blosum": ("blosum", int),
             "--test-cal-profile-th": ("cal_profile_th", int), "--test-update-seq-th": ("update_seq_th", int)}
    for f in it:
        if f in names:
            kw[names[f][0]] = names[f][1](next(it))
        elif f in ("-w", "--wildcard"):
            kw["wildcard"] = True
        elif f == "--filter":
            kw["no_filter"] = False
        elif f in ("--length-deviation", "--max-ambig", "--max-len", "--min-len", "--type"):
            next(it)
    return kw


class Result:
    pass


def run(tree, fasta, seq_type, max_subtree, exe, *, flags=()):
    """The whole mode.  Returns a Result: records [(name, row)], width, leaf_grp, sub_len, sources, cells_a, cells_b, pairs_per_level, replays."""
    replay_kw = replay_kwargs(flags)
    leaf_grp, roots, (top, children), n_parts = partition_newick(open(tree).read().splitlines()[0], max_subtree)
    dumps = dump_subtrees(exe, tree, fasta, seq_type, max_subtree, flags)
    res = Result()
    res.leaf_grp, res.n_parts = leaf_grp, n_parts
    if n_parts <= 1:                                       # the default run
        assert len(dumps) == 1 and dumps[0]["subtree"] == -1
        rep = MR.Replay(dumps[0], **replay_kw)
        rep.run()
        n = rep.root.aln_len
        res.records = [(s["name"].encode(), row[:n]) for s, row, lq in zip(rep.seqs, rep.rows, rep.low_q) if not lq]
        res.width, res.sub_len, res.sources, res.cells_a, res.cells_b, res.pairs_per_level, res.replays = n, {0: n}, {}, rep.cells, 0, [], [rep]
        return res
    assert [d["subtree"] for d in dumps] == sorted(roots), "the dump lists the subtrees in ascending index"
    group_of = {roots[k]: g for g, k in enumerate(sorted(roots))}          # root name -> group (position in ascending index)
    freq, num, weight, rows, names, res.sub_len, res.sources, res.replays, res.cells_a = [], [], [], [], [], {}, {}, [], 0
    for d in dumps:
        k = d["subtree"]
        assert d["root_in_tree"] == roots[k]
        assert {s["name"] for s in d["sequences"]} <= {leaf for leaf, g in leaf_grp.items() if g == k}, "the C++ partition and this one agree on the leaves read"
        rep = MR.Replay(d, **replay_kw)
        rep.run()
        f, n_aln, source = subtree_profile(rep)
        n = rep.root.aln_len
        assert f.shape[0] == n
        keep = [i for i, lq in enumerate(rep.low_q) if not lq]
        freq.append(f); num.append(n_aln); weight.append(F(rep.root.aln_weight))
        rows.append([rep.rows[i][:n] for i in keep]); names.append([rep.seqs[i]["name"].encode() for i in keep])
        res.sub_len[k], res.sources[k] = n, source
        res.replays.append(rep)
        res.cells_a += rep.cells
    matrix = res.replays[0].matrix
    maps = MO.Maps([f.shape[0] for f in freq])
    under = [[g] for g in range(len(freq))]
    res.cells_b, res.pairs_per_level, res.retries = 0, [], []
    import oracle_lib as O

    cells = [0]
    real_align = O.align_pair

    def counting(*a, **kw):
        out = real_align(*a, **kw)
        cells[0] += out[2].cells
        return out

    O.align_pair = counting
    try:
        for level in schedule_mode1(top, children):
            res.pairs_per_level.append(len(level))
            refs, qrys, paths = [], [], []
            for p, c in level:
                r, q = group_of[p], group_of[c]
                path = MO.merge_pair(freq[r], num[r], weight[r], freq[q], num[q], weight[q], seq_type, matrix, gap_open=float(res.replays[0].gap_open),
                                     gap_extend=float(res.replays[0].gap_extend), thr=res.replays[0].gappy, log=lambda x, f: res.retries.append((x, f)))
                freq[r] = LO.update_frequency(freq[r], freq[q], path, weight[r], weight[q])
                refs.append(list(under[r])); qrys.append(list(under[q])); paths.append(path)
                num[r], weight[r] = num[r] + num[q], F(weight[r] + weight[q])
                under[r] += under[q]
            maps.apply(refs, qrys, paths)
    finally:
        O.align_pair = real_align
    res.cells_b = cells[0]
    out_rows, res.width = maps.rows(rows)
    res.records = [(n, r) for nn, rr in zip(names, out_rows) for n, r in zip(nn, rr)]
    res.maps = maps
    return res


def to_bytes(records):
    return b"".join(b">" + n + b"\n" + r + b"\n" for n, r in records)
