"""Writes tests/golden/merge_expected.json: width, row count and md5 of what the CPU restatement of the merge mode (tests/merge_oracle.py)
gives for the four sub-alignments under tests/golden/RNASim_subalignments/ (the reference's sample for `-f`, gzipped), default flags.

    python tests/golden/make_merge_expected.py
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import merge_oracle as MO  # noqa: E402


def main():
    retries = []
    records, W, _, paths = MO.merge_dir(os.path.join(HERE, "RNASim_subalignments"), "n", log=lambda x, f: retries.append([x, f]))
    out = {"case": "RNASim_subalignments, default flags", "files": [os.path.basename(f) for f in MO.list_files(os.path.join(HERE, "RNASim_subalignments"))],
           "rows": len(records), "width": W, "path_lengths": [int(len(p)) for p in paths], "retries": retries,
           "md5": hashlib.md5(MO.to_bytes(records)).hexdigest()}
    with open(os.path.join(HERE, "merge_expected.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(out)


if __name__ == "__main__":
    main()
