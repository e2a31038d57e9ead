"""Writes tests/golden/subtree_expected.json from the CPU restatement of the subtree mode (tests/subtree_oracle.py): for the repository's RNASim
fixture at -m 100 and sars_20 at -m 8, default flags, the partition (leaf -> subtree index), every subtree's own alignment length, the final
width, the md5 of the output, the pairs per level of the merge and the band cells of both phases.

    python tests/golden/make_subtree_expected.py
"""
import gzip
import hashlib
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import subtree_oracle as SO  # noqa: E402

CASES = {"sars_20_m8": ("sars_20.nwk", "sars_20.fa.gz", 8), "RNASim_m100": ("RNASim.nwk", "RNASim.fa.gz", 100)}


def expected(name, work):
    tree, fasta, m = CASES[name]
    fa = os.path.join(work, name + ".fa")
    with open(fa, "wb") as f:
        f.write(gzip.open(os.path.join(HERE, fasta)).read())
    r = SO.run(os.path.join(HERE, tree), fa, "n", m, SO.build_dump(work))
    return {"tree": tree, "sequences": fasta, "max_subtree": m, "subtrees": r.n_parts, "partition": dict(sorted(r.leaf_grp.items())),
            "subtree_length": {str(k): int(v) for k, v in sorted(r.sub_len.items())}, "profile_source": {str(k): v for k, v in sorted(r.sources.items())},
            "rows": len(r.records), "width": int(r.width), "md5": hashlib.md5(SO.to_bytes(r.records)).hexdigest(),
            "merge_pairs_per_level": r.pairs_per_level, "merge_retries": len(r.retries), "band_cells_subtrees": int(r.cells_a), "band_cells_merge": int(r.cells_b)}


def main():
    with tempfile.TemporaryDirectory() as work:
        out = {name: expected(name, work) for name in CASES}
    with open(os.path.join(HERE, "subtree_expected.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print({k: {x: v[x] for x in ("subtrees", "width", "md5", "band_cells_subtrees", "band_cells_merge")} for k, v in out.items()})


if __name__ == "__main__":
    main()
