"""tests/place_tree_oracle.py -- TEST INFRASTRUCTURE ONLY.  Placement along a tree (-t -a -i --place-on-tree) restated from the REFERENCE source,
sharing no code with twilight_amd/csrc/host/place_tree.cpp:

    the placed marks, the backbone groups, their squeeze, alnNum / alnWeight       reference src/sequencedb.cpp:148-210
    the placement tree                                                              sequencedb.cpp:212-239
    the mode-0 schedule over a tree whose inner nodes bring members                 progressive.cpp:10-80, node.cpp:58-71
    the alignment itself                                                            oracle/msa_replay.py, imported unchanged
    the result at the root and the output order                                     tree.cpp:698-704, io.cpp:512-525

The input is what tests/place_tree_dump.cpp prints of the product's host half: the whole tree AFTER the reroot (tests/place_tree_kats.cpp holds the
reroot to hand-derived answers), which leaves are new, and the sequences with weight, quality flag and row.  Marks, groups and levels are
computed here and held equal to the dump's before anything is aligned.

One deliberate difference from the reference is shared with the product and is no part of this file: with a single new sequence the
reference's reroot moves the root into that leaf and then finds no placed leaf; the product keeps the root (Tree::reroot).
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
sys.path.insert(0, os.path.join(_ROOT, "oracle"))

import msa_replay as MR  # noqa: E402

F = np.float32


# ---- 1. marks and groups (sequencedb.cpp:148-170) ----

def parents_of(tree, root):
    par = {root: None}
    for name, n in tree.items():
        for c in n["children"]:
            par[c] = name
    return par


def placed_marks(tree, root):
    """The new leaves and every ancestor of one."""
    par = parents_of(tree, root)
    placed = set()
    for name, n in tree.items():
        if n["leaf"] and n.get("new"):
            placed.add(name)
            cur = name
            while par[cur] is not None and par[cur] not in placed:
                placed.add(par[cur])
                cur = par[cur]
    return placed


def group_of(tree, placed, owner, name_to_id):
    """The backbone leaves below the unplaced children of `owner`, depth first, children in order."""
    out = []

    def walk(name):
        n = tree[name]
        if n["leaf"] and name not in placed:
            out.append(name_to_id[name])
        for c in n["children"]:
            if c not in placed:
                walk(c)

    walk(owner)
    return out


def squeeze_group(rows):
    """The rows of one group without the columns in which every row holds '-' ('.' keeps a column): sequencedb.cpp:171-210."""
    if not rows:
        return []
    L = len(rows[0])
    assert all(len(r) == L for r in rows)
    if L == 0:
        return [b"" for _ in rows]
    block = np.array([np.frombuffer(r, dtype=np.uint8) for r in rows]).reshape(len(rows), L)
    keep = ~np.all(block == 0x2D, axis=0)
    return [block[k, keep].tobytes() for k in range(len(rows))]


def group_num_weight(ids, weight):
    """alnNum, and alnWeight summed in member order in fp32 (sequencedb.cpp:205-207)."""
    w = F(0)
    for s in ids:
        w = F(w + F(weight[s]))
    return len(ids), w


# ---- 2. the placement tree and its schedule ----

def placement_tree(tree, root, placed):
    """name -> {"leaf", "children" (the placed ones, in order), "parent"} of the placed nodes (sequencedb.cpp:212-231)."""
    par = parents_of(tree, root)
    return {name: {"leaf": bool(tree[name]["leaf"]), "children": [c for c in tree[name]["children"] if c in placed], "parent": par[name]} for name in tree if name in placed}


def schedule_mode0(nodes, root, has_members):
    """progressive.cpp:10-80 and :109-124 with one group for all nodes.  Changes nodes[*]["children"] / ["parent"] as the reference does (a unary
    node without members is spliced out).  Returns the levels: lists of (first, second)."""
    pre, stack = [], [root]
    while stack:                                    # node.cpp:58-71: the walk pushes in pre-order, the schedule pops in reverse
        cur = stack.pop()
        pre.append(cur)
        stack.extend(reversed(nodes[cur]["children"]))
    order, pairs = {}, []

    def nxt(name):
        return order[name] + 1 if name in order else 0

    for name in reversed(pre):
        n = nodes[name]
        if n["leaf"]:
            continue
        children = list(n["children"])
        if not children and not has_members(name):
            raise AssertionError("a placed inner node without a placed child and without members")
        if len(children) == 1 and n["parent"] is not None and not has_members(name):
            sib = nodes[n["parent"]]["children"]
            sib[sib.index(name)] = children[0]
            nodes[children[0]]["parent"] = n["parent"]
            continue
        while len(children) > 1:
            left = []
            for i in range(0, len(children) - 1, 2):
                lvl = max(nxt(children[i]), nxt(children[i + 1]))
                order[children[i]] = order[children[i + 1]] = lvl
                pairs.append(((children[i], children[i + 1]), lvl))
                left.append(children[i])
            if len(children) % 2 == 1:
                left.append(children[-1])
            children = left
        if len(children) == 1 and has_members(name):
            first = n["children"][0]
            lvl = max(nxt(name), nxt(first))
            order[name] = order[first] = lvl
            pairs.append(((name, first), lvl))
        order[name] = order.setdefault(children[0], 0)      # (std::map::operator[] makes the entry, :77)
    levels = []
    for pr, lvl in pairs:
        while len(levels) < lvl + 1:
            levels.append([])
        levels[lvl].append(pr)
    return levels


# ---- 3. the dump ----

DUMP_SOURCES = ("phylo.cpp", "seqdb_io.cpp", "helpers.cpp", "progressive.cpp", "driver.cpp", "partition.cpp", "place_tree.cpp")


def build_dump(out_dir):
    """tests/place_tree_dump.cpp with the host sources it needs, by plain g++ (place_tree.cpp: its host half only)."""
    exe = os.path.join(out_dir, "place_tree_dump")
    host = os.path.join(_ROOT, "twilight_amd", "csrc", "host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fopenmp", "-ffp-contract=off", "-Wall", "-DTWL_PLACE_TREE_HOST_ONLY", "-o", exe, os.path.join(_HERE, "place_tree_dump.cpp")] +
                          [os.path.join(host, f) for f in DUMP_SOURCES] + ["-lz"])
    return exe


def dump(exe, tree, backbone, fasta, seq_type, flags=()):
    r = subprocess.run([exe, "-t", tree, "-a", backbone, "-i", fasta, "-o", "x", "--type", seq_type, "--place-on-tree"] + list(flags), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    docs = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    assert len(docs) == 1
    return docs[0]


# ---- the mode ----

def replay_kwargs(flags):
    """The CLI flags the replay has to know (the others are already applied in the dump)."""
    kw, it = {}, iter(flags)
    names = {"-r": ("gappy", float), "--remove-gappy": ("gappy", float), "--match": ("match", float), "--mismatch": ("mismatch", float), "--transition": ("transition", float),
             "--gap-open": ("gap_open", float), "--gap-extend": ("gap_extend", float), "-b": ("blosum", int), "--blosum": ("blosum", int)}
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


def derive(d):
    """Marks, groups (ids, squeezed rows, num, weight), placement tree and levels of a dump, all computed here."""
    res = Result()
    tree, root = d["tree"], d["tree_root"]
    name_to_id = {s["name"]: s["id"] for s in d["sequences"]}
    weight = [F(s["weight"]) for s in d["sequences"]]
    res.placed = placed_marks(tree, root)
    res.groups = {}
    for name in sorted(res.placed):
        ids = group_of(tree, res.placed, name, name_to_id)
        if ids and not tree[name]["leaf"]:
            res.groups[name] = ids
    res.rows = {}
    res.group_len, res.group_num, res.group_weight = {}, {}, {}
    for name, ids in res.groups.items():
        sq = squeeze_group([d["sequences"][s]["seq"].encode("latin-1") for s in ids])
        for s, row in zip(ids, sq):
            res.rows[s] = row
        res.group_len[name] = len(sq[0])
        res.group_num[name], res.group_weight[name] = group_num_weight(ids, weight)
    res.nodes = placement_tree(tree, root, res.placed)
    res.levels = schedule_mode0(res.nodes, root, lambda n: n in res.groups)
    res.root = root
    return res


def check_against_dump(d, res):
    """The product's host half said the same."""
    assert {k: v["ids"] for k, v in d["groups"].items()} == res.groups
    for k, v in d["groups"].items():
        assert v["num"] == res.group_num[k]
        assert F(v["weight"]) == res.group_weight[k], (k, v["weight"], res.group_weight[k])
    assert d["root"] == res.root
    assert [[tuple(p) for p in lv] for lv in d["levels"]] == res.levels
    reach, stack = set(), [res.root]
    while stack:
        cur = stack.pop()
        reach.add(cur)
        stack.extend(res.nodes[cur]["children"])
    assert set(d["nodes"]) == reach
    for name in reach:
        assert d["nodes"][name]["children"] == res.nodes[name]["children"], name


def run(d, *, flags=()):
    """The whole mode on a dump.  Returns a Result: records [(name, row)], width, derived (marks, groups, levels), replay."""
    der = derive(d)
    check_against_dump(d, der)
    doc = {"type": d["type"], "root": der.root, "sequences": d["sequences"],
           "nodes": {k: {"leaf": v["leaf"], "grp": -1, "children": v["children"]} for k, v in der.nodes.items()},
           "levels": [[list(p) for p in lv] for lv in der.levels]}
    rep = MR.Replay(doc, **replay_kwargs(flags))
    rep.rows = [s["seq"].encode("latin-1") for s in d["sequences"]]
    for s, row in der.rows.items():
        rep.rows[s] = row
    for name, ids in der.groups.items():
        n = rep.nodes[name]
        n.seqs, n.aln_len, n.aln_num, n.aln_weight = list(ids), der.group_len[name], der.group_num[name], der.group_weight[name]
    rep.run()
    res = Result()
    res.derived, res.replay = der, rep
    res.width = rep.root.aln_len                      # (extractResult hands the placement root's result to the tree's root: the same node name)
    res.records = [(s["name"].encode(), row[: res.width]) for s, row, lq in zip(rep.seqs, rep.rows, rep.low_q) if not lq]
    return res


def to_bytes(records):
    return b"".join(b">" + n + b"\n" + r + b"\n" for n, r in records)
