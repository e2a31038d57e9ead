"""tests/place_oracle.py -- CPU restatement of placement without a tree (the reference's PLACE_WO_TREE mode, `twilight -a ... -i ... -o`).

TEST INFRASTRUCTURE ONLY.  Built from oracle/level_oracle.py (profile, gappy columns, PSGP, addGappyColumnsBack) and the DP checker
(tests/oracle_lib.py: talco_oracle.c), following what the reference does in that mode:
  1. backbone profile: counts of letterIdx(type, toupper(c)) per column over all rows (readAlignment, io.cpp:200-238), num = weight = rows
  2. new sequences read and flagged low-quality as readSequences does; low-quality ones are neither aligned nor written
  3. one pair per sequence: backbone profile / the sequence, gappy columns removed at -r, PSGP, gapCharScore 0 (currentTask 2)
  4. a failed DP is retried until errorType 0 (errorType 1: xdrop doubles; 2: the band limit grows; alignment-cpu.cpp:95-128)
  5. gappy columns back (addGappyColumnsBack)
  6. mergeInsertions: longest[i] = the longest run of query-only codes in front of backbone column i over all sequences; W = L + sum
  7. output: the backbone rows ('.' in the insertion columns), then the placed sequences (letters left-aligned in their insertion blocks)
"""
from __future__ import annotations

import gzip
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
for _p in (_ROOT, os.path.join(_ROOT, "oracle"), _HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import level_oracle as LO  # noqa: E402
import oracle_lib as O  # noqa: E402

F = np.float32


def read_fasta(path):
    """(name, sequence) records as the product's reader delivers them: name up to the first blank, lines joined, blanks dropped."""
    op = gzip.open if open(path, "rb").read(2) == b"\x1f\x8b" else open
    out, name, parts = [], None, []
    with op(path, "rb") as f:
        for line in f:
            line = line.rstrip(b"\r\n")
            if line.startswith(b">"):
                if name is not None:
                    out.append((name, b"".join(parts)))
                name, parts = line[1:].split(None, 1)[0] if line[1:].split() else b"", []
            elif name is not None:
                parts.append(b"".join(line.split()))
    if name is not None:
        out.append((name, b"".join(parts)))
    return out


def backbone_profile(rows, seq_type):
    """float[L][P] column counts (the reference adds 1.0 per row; counts are exact)."""
    P = 6 if seq_type == "n" else 22
    L = len(rows[0])
    table = LO.lut(seq_type)
    prof = np.zeros((L, P), dtype=np.int64)
    cols = np.arange(L)
    for r in rows:
        np.add.at(prof, (cols, table[np.frombuffer(r, dtype=np.uint8)]), 1)
    return prof.astype(F)


def low_quality(seqs, seq_type, *, min_len=0, max_len=2**31 - 1, len_dev=0.0, max_ambig=0.1):
    """readSequences' flags (io.cpp:134-162): outside the length bounds, or more than max_ambig N / X letters."""
    lens = sorted(len(s) for s in seqs)
    med = lens[len(lens) // 2]
    lo = int(F(med) * F(1 - F(len_dev))) if len_dev > 0 else min_len
    hi = int(F(med) * F(1 + F(len_dev))) if len_dev > 0 else max_len
    amb = 4 if seq_type == "n" else 20
    table = LO.lut(seq_type)
    out = []
    for s in seqs:
        bad = len(s) > hi or len(s) < lo
        if not bad:
            cnt = int(np.count_nonzero(table[np.frombuffer(s, dtype=np.uint8)] == amb)) if s else 0
            bad = cnt > F(len(s)) * F(max_ambig)
        out.append(bad)
    return out


def place_one(prof, B, seq, seq_type, matrix, *, gap_open=-50.0, gap_extend=-5.0, thr=0.95, log=None):
    """Final path of one sequence against the backbone profile (codes 0/1/2 over all L columns); log(xdrop, flen) per retry."""
    L, P = prof.shape
    if len(seq) == 0:
        return np.full(L, 2, dtype=np.int8)
    rp = LO.profile_from_cache(prof, B, B)
    qp = LO.calculate_profile([seq], [1.0], P, seq_type)
    cr, ir, runs_r = LO.prepare_side(rp, B, thr, gap_open, gap_extend, seq_type)
    cq, iq, runs_q = LO.prepare_side(qp, 1, thr, gap_open, gap_extend, seq_type)
    prm = O.make_params(matrix, gap_open=gap_open, gap_extend=gap_extend, gap_char=0.0)
    min_len = min(cr.shape[0], cq.shape[0])
    while True:
        path, err, _ = O.align_pair(prm, cr[:, :P], cq[:, :P], cr[:, P], cr[:, P + 1], cq[:, P], cq[:, P + 1], B, 1)
        if err == 0:
            break
        assert err != 3, "errorType 3"
        if err == 2:
            prm.flen = min(int(prm.flen * 1.2) << 1, min_len)
        else:
            prm.xdrop = int(prm.xdrop * 2)
            prm.flen = min(int(prm.xdrop * 4) << 1, min_len)
        if log is not None:
            log(prm.xdrop, prm.flen)
    full = LO.add_gappy_columns_back(path, runs_r if thr != 1.0 else [], runs_q if thr != 1.0 else [], (ir & 0x7F).astype(np.int64),
                                     (iq & 0x7F).astype(np.int64), matrix, gap_open, gap_extend)
    return full


def merge_insertions(L, paths):
    """longest[0..L]: the longest run of code 1 in front of backbone column i (i = L: after the last column), over all paths."""
    longest = np.zeros(L + 1, dtype=np.int64)
    for p in paths:
        c, run = 0, 0
        for v in p:
            if v == 1:
                run += 1
                continue
            longest[c] = max(longest[c], run)
            run = 0
            c += 1
        longest[c] = max(longest[c], run)
    return longest


def expand_backbone(row: bytes, longest) -> bytes:
    out = bytearray()
    for i, ch in enumerate(row):
        out += b"." * int(longest[i])
        out.append(ch)
    out += b"." * int(longest[len(row)])
    return bytes(out)


def expand_placed(seq: bytes, path, longest) -> bytes:
    out = bytearray()
    c, q, run = 0, 0, bytearray()

    def flush():
        out.extend(run)
        out.extend(b"." * (int(longest[c]) - len(run)))

    for v in path:
        if v == 1:
            run.append(seq[q])
            q += 1
            continue
        flush()
        run = bytearray()
        if v == 0:
            out.append(seq[q])
            q += 1
        else:
            out.append(ord("-"))
        c += 1
    flush()
    assert c == len(longest) - 1 and q == len(seq)
    return bytes(out)


def place(backbone, new, seq_type="n", *, matrix=None, gap_open=-50.0, gap_extend=-5.0, thr=0.95, min_len=0, max_len=2**31 - 1, len_dev=0.0,
          max_ambig=0.1, log=None):
    """backbone, new: lists of (name, bytes).  Returns (records [(name, row)], longest, retries)."""
    from twilight_amd import synth

    if matrix is None:
        matrix = synth.nucleotide_matrix() if seq_type == "n" else synth.protein_matrix()
    rows = [r for _, r in backbone]
    L = len(rows[0])
    assert all(len(r) == L for r in rows), "backbone rows of unequal length"
    seen, uniq = set(), []
    for n, s in new:
        if n not in seen:
            seen.add(n)
            uniq.append((n, s))
    lowq = low_quality([s for _, s in uniq], seq_type, min_len=min_len, max_len=max_len, len_dev=len_dev, max_ambig=max_ambig)
    placed = [x for x, bad in zip(uniq, lowq) if not bad]
    prof = backbone_profile(rows, seq_type)
    retries = []
    paths = [place_one(prof, len(rows), s, seq_type, matrix, gap_open=gap_open, gap_extend=gap_extend, thr=thr,
                       log=(lambda x, f, n=n: retries.append((n, x, f)))) for n, s in placed]
    longest = merge_insertions(L, paths)
    out = [(n, expand_backbone(r, longest)) for n, r in backbone]
    out += [(n, expand_placed(s, p, longest)) for (n, s), p in zip(placed, paths)]
    return out, longest, retries


def write(records, path):
    with open(path, "wb") as f:
        for n, r in records:
            f.write(b">" + n + b"\n" + r + b"\n")


def to_bytes(records) -> bytes:
    return b"".join(b">" + n + b"\n" + r + b"\n" for n, r in records)
