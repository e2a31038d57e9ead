"""Writes tests/golden/place_tree_expected.json: md5 and width of what tests/place_tree_oracle.py (the CPU restatement of placement along a tree,
on oracle/msa_replay.py) makes of the reference's own sample for the mode -- RNASim.nwk, RNASim_backbone.aln.gz and the 100 sequences of
RNASim.fa.gz that RNASim_sub.names.txt names -- with default flags, with --rooted and with -r 1.  Runs on the CPU:
    python tests/golden/make_place_tree_expected.py
"""
import gzip
import hashlib
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import place_tree_oracle as PO  # noqa: E402

VARIANTS = {"default": [], "rooted": ["--rooted"], "r1": ["-r", "1"]}


def sample_inputs(out_dir):
    """(tree, backbone, new sequences) of the sample as files the CLI and the dump read."""
    names = set(open(os.path.join(HERE, "RNASim_sub.names.txt")).read().split())
    new = os.path.join(out_dir, "RNASim_new.fa")
    with open(new, "w") as f:
        keep = False
        for line in gzip.open(os.path.join(HERE, "RNASim.fa.gz"), "rt"):
            if line.startswith(">"):
                keep = line[1:].split()[0] in names
            if keep:
                f.write(line)
    return os.path.join(HERE, "RNASim.nwk"), os.path.join(HERE, "RNASim_backbone.aln.gz"), new


def main():
    out = {}
    with tempfile.TemporaryDirectory() as d:
        exe = PO.build_dump(d)
        tree, backbone, new = sample_inputs(d)
        for name, flags in VARIANTS.items():
            r = PO.run(PO.dump(exe, tree, backbone, new, "n", flags), flags=flags)
            out[name] = {"flags": flags, "width": r.width, "rows": len(r.records), "groups": len(r.derived.groups), "levels": len(r.derived.levels),
                         "md5": hashlib.md5(PO.to_bytes(r.records)).hexdigest()}
            print(name, out[name])
    with open(os.path.join(HERE, "place_tree_expected.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
