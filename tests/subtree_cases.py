"""tests/subtree_cases.py -- the inputs of the weighted column profile's tests (twl_store_weighted_columns, include/twl_subtree.h), in one place:
the shape table, the rows, the weights and the numpy statement of the sum.  tests/test_subtree_oracle_cpu.py proves on the CPU that these
inputs are order-sensitive; tests/test_gpu_subtree_kernel.py holds the kernel to them bit for bit.

weighted_columns_kernel (subtree_kernels.hip.h) gives a workgroup 256 columns, one thread each, and stages the rows 256 at a time:
  COLUMNS   1, 255, 256, 257, 513   on both sides of one and of two column tiles
  ROWS      1, 2, 65, 300           and 255, 256, 257: on both sides of one staging round of 256 rows (300 = a full round and a partial one)
"""
import numpy as np

COLUMNS = (1, 255, 256, 257, 513)
ROWS = (1, 2, 65, 255, 256, 257, 300)
ROWS_PER_CLASS = 300
SAME_LETTER_COLUMN = 100          # in rows of more than 100 columns this column holds the letter A (either case) in every row

ALPHABET = {"n": list(b"ACGTUNacgtun-.RYKMSW"), "p": list(b"ACDEFGHIKLMNPQRSTVWYacdefghiklmnpqrstvwyXxBZJ-.")}


def lut(seq_type):
    """letterIdx(type, toupper(c)) for every byte (reference src/scoring-matrix.cpp:26-79)."""
    t = np.zeros(256, dtype=np.int64)
    for c in range(256):
        u = chr(c).upper() if c < 128 else chr(c)
        if seq_type == "n":
            t[c] = {"A": 0, "C": 1, "G": 2, "T": 3, "U": 3, "-": 5, ".": 5}.get(u, 4)
        else:
            t[c] = 21 if u in "-." else "ACDEFGHIKLMNPQRSTVWY".find(u) if u in "ACDEFGHIKLMNPQRSTVWY" else 20
    return t


def store_rows(seq_type):
    """ROWS_PER_CLASS rows of every length of COLUMNS, interleaved (row i has COLUMNS[i % 5] columns): lower case, '-', '.', ambiguity letters."""
    rng = np.random.default_rng(20 if seq_type == "n" else 21)
    rows = []
    for i in range(ROWS_PER_CLASS * len(COLUMNS)):
        r = bytearray(rng.choice(ALPHABET[seq_type], COLUMNS[i % len(COLUMNS)]).astype(np.uint8).tobytes())
        if len(r) > SAME_LETTER_COLUMN:
            r[SAME_LETTER_COLUMN] = ord("Aa"[i % 2])
        rows.append(bytes(r))
    return rows


def rewritten_rows(seq_type, rows):
    """{id: new row} for the odd-numbered rows of every class: what the test writes with twl_store_write_rows before it counts."""
    rng = np.random.default_rng(22 if seq_type == "n" else 23)
    out = {}
    for i, r in enumerate(rows):
        if (i // len(COLUMNS)) % 2 == 1:
            new = bytearray(rng.choice(ALPHABET[seq_type], len(r)).astype(np.uint8).tobytes())
            if len(new) > SAME_LETTER_COLUMN:
                new[SAME_LETTER_COLUMN] = ord("aA"[i % 2])
            out[i] = bytes(new)
    return out


def class_ids(L):
    k = COLUMNS.index(L)
    return [k + len(COLUMNS) * j for j in range(ROWS_PER_CLASS)]


def case(seq_type, L, n):
    """(ids, weights) of one call: n rows of L columns in a shuffled (non-monotonic) order; weights spread over three decades, none a
    power of two (what Tree::calSeqWeight leaves: sums of branch / leaves, scaled to a maximum of 1)."""
    rng = np.random.default_rng(1000 * COLUMNS.index(L) + n + (0 if seq_type == "n" else 500))
    ids = rng.permutation(class_ids(L))[:n].tolist()
    if n > 2 and ids == sorted(ids):
        ids[0], ids[1] = ids[1], ids[0]
    w = (10.0 ** rng.uniform(-3.0, 0.0, n)).astype(np.float32)
    w[np.log2(w) == np.round(np.log2(w))] *= np.float32(1.1)
    return ids, w


def weighted_profile(rows, weights, seq_type):
    """SequenceDB::storeSubtreeProfile (reference src/sequencedb.cpp:122-138): row by row in the given order, in fp32."""
    P = 6 if seq_type == "n" else 22
    table = lut(seq_type)
    L = len(rows[0])
    out = np.zeros((L, P), dtype=np.float32)
    cols = np.arange(L)
    for r, w in zip(rows, weights):
        assert len(r) == L
        out[cols, table[np.frombuffer(r, dtype=np.uint8)]] += np.float32(w)
    return out


# ---- the families of the command-line tests (tests/test_gpu_subtree.py; the CPU restatement runs in the test) ----

def write_family(d, tag, nwk, seqs):
    import os

    t, f = os.path.join(d, tag + ".nwk"), os.path.join(d, tag + ".fa")
    with open(t, "w") as fh:
        fh.write(nwk + "\n")
    with open(f, "w") as fh:
        for name, s in seqs:
            fh.write(f">{name}\n{s}\n")
    return t, f


def protein_family(d):
    """60 x 300 aa at -m 16: five subtrees of 10, 16, 12, 15 and 7 leaves, a first merge level of two pairs; sequence s20 is cut to 90 residues,
    far off its subtree's median, so --length-deviation 0.5 --filter excludes it.  Returns (tree, fasta, type, m, flags)."""
    from twilight_amd import synth

    nwk, seqs = synth.make_family(60, 300, P=22, seed=3, sub=0.1, indel=0.02)
    seqs[20] = (seqs[20][0], seqs[20][1][:90])
    t, f = write_family(d, "prot", nwk, seqs)
    return t, f, "p", 16, ["--filter", "--length-deviation", "0.5"]


def mixed_profile_family(d):
    """40 x 300 nt at -m 16 with --test-cal-profile-th 6: four subtrees of 8, 14, 9 and 9 leaves; the passes of subtrees 1 and 2 reach the
    threshold and leave their roots a cached profile, those of subtrees 0 and 3 do not.  Returns (tree, fasta, type, m, flags)."""
    from twilight_amd import synth

    nwk, seqs = synth.make_family(40, 300, P=6, seed=5, sub=0.08, indel=0.02)
    t, f = write_family(d, "mixed", nwk, seqs)
    return t, f, "n", 16, ["--test-cal-profile-th", "6"]
