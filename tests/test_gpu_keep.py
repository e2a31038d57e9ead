"""`twilight-mi355x -a BACKBONE -i NEW -o OUT --keep-length [--write-insertions FILE]` on the MI355X: the output is the output of the same
command without the flag with every insertion column deleted, the backbone records are the input's byte for byte, and the insertions
file gives every sequence back.  Against tests/keep_oracle.py over tests/place_oracle.py; bytes only.  Every CLI run has its own time limit."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import keep_cases as KC
import keep_oracle as KO
import place_oracle as PO
import strand_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "twilight_amd", "twilight-mi355x")

pytestmark = pytest.mark.gpu


def _write(records, path):
    PO.write(records, path)
    return str(path)


def _cli(tmp_path, backbone, new, *flags, tag="run", keep=True, timeout=300):
    """One run; with keep: --keep-length --write-insertions.  Returns (alignment bytes, insertions bytes or None, the process)."""
    bb = backbone if isinstance(backbone, str) else _write(backbone, tmp_path / f"{tag}_bb.aln")
    nw = new if isinstance(new, str) else _write(new, tmp_path / f"{tag}_new.fa")
    out, ins = tmp_path / f"{tag}_out.aln", tmp_path / f"{tag}_ins.tsv"
    extra = ("--keep-length", "--write-insertions", str(ins)) if keep else ()
    r = subprocess.run(["timeout", "-k", "10", str(timeout), EXE, "-a", bb, "-i", nw, "-o", str(out), *extra, *flags], capture_output=True, text=True,
                       timeout=timeout + 30)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert keep or not ins.exists()
    return open(out, "rb").read(), (open(ins, "rb").read() if keep else None), r


def _records(blob):
    return [tuple(x.split(b"\n")[:2]) for x in blob.split(b">")[1:]]


def _lines(ins):
    """[(name, k, letters)] of an insertions file: no header, three tab-separated fields per line."""
    out = []
    for l in ins.split(b"\n")[:-1]:
        name, k, letters = l.split(b"\t")
        assert letters
        out.append((name, int(k), letters))
    assert ins == b"" or ins.endswith(b"\n")
    return out


def _summary(r):
    import re

    m = re.search(r"Kept the backbone's length (\d+): (\d+) insertion run\(s\), (\d+) letter\(s\) of (\d+) sequence\(s\) left out \(merged they would make (\d+) columns\)", r.stderr)
    assert m, r.stderr[-2000:]
    return tuple(int(x) for x in m.groups())


def _against_oracle(tmp_path, bb, new, flags=(), tag="f", seq_type="n", **oracle_kw):
    """The two files of a run against strip(place()) and the records of the merged rows."""
    blob, ins, r = _cli(tmp_path, bb, new, *flags, tag=tag)
    merged, longest, _ = PO.place(bb, new, seq_type, **oracle_kw)
    B, L = len(bb), len(bb[0][1])
    want = KO.strip(merged, longest)
    assert want[:B] == list(bb)
    assert blob == PO.to_bytes(want)
    want_lines = [(n, k, letters) for n, row in merged[B:] for k, letters in KO.records_of_merged(row, longest)]
    assert _lines(ins) == want_lines
    seqs = dict(new[::-1])                                     # (of two records with one name the first is kept)
    for n, row in want[B:]:
        assert KO.rebuild(row, [(k, x) for m, k, x in want_lines if m == n]) == seqs[n]
    assert _summary(r) == (L, len(want_lines), sum(len(x) for _, _, x in want_lines), len({n for n, _, _ in want_lines}), L + int(longest.sum()))
    return blob, ins, r, longest


def test_cli_rnasim_fixture(gpu, tmp_path):
    """479 x 3 864 backbone, the 100 RNASim_sub sequences."""
    sys.path.insert(0, GOLDEN)
    import make_place_expected as MPE

    backbone, new = MPE.rnasim_inputs()
    assert len(backbone) == 479 and len(new) == 100 and not any(b"." in r for _, r in backbone)
    sub = str(tmp_path / "RNASim_sub.fa")
    MPE.write_sub_fasta(sub)
    bbfile = os.path.join(GOLDEN, "RNASim_backbone.aln.gz")
    merged_blob, _, _ = _cli(tmp_path, bbfile, sub, tag="merged", keep=False)
    exp = json.load(open(os.path.join(GOLDEN, "place_expected.json")))["rnasim"]
    assert hashlib.md5(merged_blob).hexdigest() == exp["md5"]
    blob, ins, r = _cli(tmp_path, bbfile, sub, "-v", tag="kept")

    merged = _records(merged_blob)
    rows = np.array([np.frombuffer(row, dtype=np.uint8) for _, row in merged[:479]])
    drop = (rows == ord(".")).all(axis=0)                     # the columns in which every backbone row holds '.'
    assert int(drop.sum()) == exp["inserted_columns"] == 537
    want = [(n, np.frombuffer(row, dtype=np.uint8)[~drop].tobytes()) for n, row in merged]
    assert blob == PO.to_bytes(want)
    got = _records(blob)
    assert got[:479] == backbone                              # the input file's records, byte for byte
    assert all(len(row) == 3864 for _, row in got) and len(got) == 579
    assert not any(b"." in row for _, row in got[479:])

    lines = _lines(ins)
    L, runs, letters, n_seq, W = _summary(r)
    assert (L, runs, W) == (3864, len(lines), exp["width"]) and letters == sum(len(x) for _, _, x in lines) and n_seq == len({n for n, _, _ in lines})
    assert letters >= 537
    order = [n for n, _ in new]
    assert [n for n, _, _ in lines] == sorted([n for n, _, _ in lines], key=order.index)          # sequences in input order
    for (n, s), (gn, row) in zip(new, got[479:]):
        mine = [(k, x) for m, k, x in lines if m == n]
        assert gn == n and [k for k, _ in mine] == sorted({k for k, _ in mine})                   # runs by ascending k, one per slot
        assert KO.rebuild(row, mine) == s
    assert "keep-finish" in r.stderr and ", runs " in r.stderr


def test_cli_nucleotide_family(gpu, tmp_path):
    bb, new = KC.nucleotide_family()
    _, ins, _, longest = _against_oracle(tmp_path, bb, new)
    assert longest.sum() > 0 and any(x != x.upper() for _, _, x in _lines(ins))      # the case of the letters is kept


def test_cli_protein_blosum62(gpu, tmp_path):
    bb, new = KC.protein_family()
    _, _, _, longest = _against_oracle(tmp_path, bb, new, ("--type", "p", "-b", "62"), seq_type="p")
    assert longest.sum() > 0


def test_cli_chunks_give_the_same_two_files(gpu, tmp_path):
    bb, new = KC.chunk_family()
    one, ins1, _ = _cli(tmp_path, bb, new, tag="one")
    seven, ins7, r = _cli(tmp_path, bb, new, "--test-place-chunk", "7", tag="seven")
    assert seven == one and ins7 == ins1 and ins1
    assert "8 chunk(s)" in r.stderr


def test_cli_low_quality_and_empty_sequences(gpu, tmp_path):
    bb, new = KC.filtered_family()
    blob, ins, r, _ = _against_oracle(tmp_path, bb, new)
    L = len(bb[0][1])
    assert b">ambiguous" not in blob and b">empty\n" + b"-" * L + b"\n" in blob
    assert b"ambiguous" not in ins and b"empty" not in ins
    assert "Low-quality sequences (not placed): 1" in r.stderr


def test_cli_no_insertion_is_the_run_without_the_flag(gpu, tmp_path):
    bb, new = KC.plain_family()
    blob, ins, r = _cli(tmp_path, bb, new, tag="kept")
    plain, _, _ = _cli(tmp_path, bb, new, tag="plain", keep=False)
    assert ins == b"" and blob == plain
    assert _summary(r) == (800, 0, 0, 0, 800)


def test_cli_adjust_direction(gpu, tmp_path):
    """The placement fixture with every third record reversed: the same bytes as on the unreversed file, apart from the _R_ names, in
    both files."""
    backbone, names, seqs, planted, dirs = SC.placement()
    bbfile = os.path.join(GOLDEN, "RNASim_backbone.aln.gz")
    orig, plant = SC.write_fasta(tmp_path / "orig.fa", names, seqs), SC.write_fasta(tmp_path / "plant.fa", names, planted)
    a, ins_a, _ = _cli(tmp_path, bbfile, orig, "--type", "n", tag="orig")
    b, ins_b, r = _cli(tmp_path, bbfile, plant, "--type", "n", "--adjust-direction", tag="plant")
    assert "Directions: %d of 100 sequences lie reversed" % int(dirs.sum()) in r.stderr
    marked = {n.encode() for n, d in zip(names, dirs) if d}
    assert marked

    def unmark(blob, lead):
        out, seen = [], set()
        for l in blob.split(b"\n"):
            if l.startswith(lead + b"_R_"):
                name = l[len(lead) + 3:].split(b"\t")[0]
                assert name in marked, l
                seen.add(name)
                l = lead + l[len(lead) + 3:]
            else:
                assert not (l.startswith(lead) and l[len(lead):].split(b"\t")[0] in marked and lead == b">"), l
            out.append(l)
        return b"\n".join(out), seen

    got, seen = unmark(b, b">")
    assert got == a and seen == marked
    got_ins, seen_ins = unmark(ins_b, b"")
    assert got_ins == ins_a and seen_ins == {n for n, _, _ in _lines(ins_a)} & marked
