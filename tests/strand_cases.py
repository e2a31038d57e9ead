"""The families the `--adjust-direction` tests share: the three fixtures with a reverse complement planted at every record i with i % 3 == 1
(record 0 forward).  Read once per process and never changed."""
import os
import sys

import guide_oracle as G
import strand_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
_CACHE = {}


def rnasim200():
    """(names, original sequences, planted sequences, planted directions) of the first 200 RNASim records."""
    if "rnasim" not in _CACHE:
        names, seqs = G.read_fasta(os.path.join(GOLDEN, "RNASim.fa.gz"), limit=200)
        assert len(names) == 200
        _CACHE["rnasim"] = (names, seqs) + SO.plant(seqs)
    return _CACHE["rnasim"]


def sars20():
    if "sars" not in _CACHE:
        names, seqs = G.read_fasta(os.path.join(GOLDEN, "sars_20.fa.gz"))
        assert len(names) == 20
        _CACHE["sars"] = (names, seqs) + SO.plant(seqs)
    return _CACHE["sars"]


def placement():
    """(backbone records (name, row), names, original, planted, directions of the 100 new sequences) of the placement fixture."""
    if "place" not in _CACHE:
        if GOLDEN not in sys.path:
            sys.path.insert(0, GOLDEN)
        import make_place_expected as MPE

        backbone, new = MPE.rnasim_inputs()
        assert len(backbone) == 479 and len(new) == 100
        names, seqs = [n.decode() for n, _ in new], [s for _, s in new]
        _CACHE["place"] = (backbone, names, seqs) + SO.plant(seqs)
    return _CACHE["place"]


def degapped(backbone):
    return [r.replace(b"-", b"").replace(b".", b"") for _, r in backbone]


def write_fasta(path, names, seqs):
    with open(path, "wb") as f:
        for n, s in zip(names, seqs):
            f.write(b">" + (n if isinstance(n, bytes) else n.encode()) + b"\n" + s + b"\n")
    return str(path)
