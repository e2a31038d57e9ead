"""Writes tests/golden/place_expected.json: the md5 of what tests/place_oracle.py places for the RNASim fixture
(RNASim_backbone.aln.gz: 479 rows x 3864 columns; the 100 new sequences named in RNASim_sub.names.txt, taken from RNASim.fa.gz),
with the CLI's defaults.  Run from the repository root:  python tests/golden/make_place_expected.py"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import place_oracle as PO  # noqa: E402


def rnasim_inputs():
    """(backbone records, new records) of the fixture."""
    backbone = PO.read_fasta(os.path.join(HERE, "RNASim_backbone.aln.gz"))
    full = dict(PO.read_fasta(os.path.join(HERE, "RNASim.fa.gz")))
    names = [n.strip().encode() for n in open(os.path.join(HERE, "RNASim_sub.names.txt")) if n.strip()]
    return backbone, [(n, full[n]) for n in names]


def write_sub_fasta(path):
    _, new = rnasim_inputs()
    PO.write(new, path)


def main():
    backbone, new = rnasim_inputs()
    out, longest, retries = PO.place(backbone, new)
    blob = PO.to_bytes(out)
    rec = {"rnasim": {"md5": hashlib.md5(blob).hexdigest(), "width": len(out[0][1]), "rows": len(out), "inserted_columns": int(longest.sum()),
                      "retries": len(retries)}}
    with open(os.path.join(HERE, "place_expected.json"), "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(rec)


if __name__ == "__main__":
    main()
