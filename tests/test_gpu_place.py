"""Placement without a tree on the MI355X (include/twl_place.h, `twilight-mi355x -a BACKBONE -i NEW -o OUT`), against the CPU oracle
tests/place_oracle.py byte for byte.  Every CLI run has its own time limit."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import place_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "twilight_amd", "twilight-mi355x")

pytestmark = pytest.mark.gpu


# ---- the device kernels through the C ABI ----

def _store(seqs, seq_type="n"):
    from twilight_amd import level

    return level.Store(list(seqs), seq_type)


def _np_counts(rows, seq_type):
    return PO.backbone_profile(rows, seq_type)


def test_count_columns_rnasim(gpu):
    from twilight_amd import place

    bb = [r for _, r in PO.read_fasta(os.path.join(GOLDEN, "RNASim_backbone.aln.gz"))]
    st = _store(bb + [b"ACGU"])
    place.count_columns(st, range(len(bb)), 3)
    got = st.cache(3)
    assert got.shape == (3864, 6)
    assert np.array_equal(got, _np_counts(bb, "n"))
    with pytest.raises(Exception):
        place.count_columns(st, range(len(bb) + 1), 4)      # rows of another length
    st.close()


def test_count_columns_protein_with_lowercase_and_wildcards(gpu):
    from twilight_amd import place

    rng = np.random.default_rng(11)
    alphabet = list(b"ACDEFGHIKLMNPQRSTVWYacdefghiklmnpqrstvwyXxNn-.BZ")
    rows = [rng.choice(alphabet, 2500).astype(np.uint8).tobytes() for _ in range(150)]      # (150 rows: three row slices per column)
    st = _store(rows, "p")
    place.count_columns(st, range(150), 0)
    assert np.array_equal(st.cache(0), _np_counts(rows, "p"))
    st.close()


def _check_merge(backbone, seqs, paths, groups):
    """collect (host rows, in the given groups of calls) + finish == the oracle's longest, W and rows."""
    from twilight_amd import place

    B = len(backbone)
    st = _store(list(backbone) + list(seqs))
    pl = place.Placement(st, len(backbone[0]))
    for g in groups:
        pl.collect_host([B + k for k in g], [paths[k] for k in g])
    longest = PO.merge_insertions(len(backbone[0]), paths)
    assert np.array_equal(pl.insertions(), longest)
    W = pl.finish(range(B))
    assert W == len(backbone[0]) + int(longest.sum())
    got = st.rows_of(list(range(B + len(seqs))))
    want = [PO.expand_backbone(r, longest) for r in backbone] + [PO.expand_placed(s, np.asarray(p), longest) for s, p in zip(seqs, paths)]
    assert got == want
    pl.close()
    st.close()


def test_collect_finish_hand_example(gpu):
    backbone = [b"AC-G", b"A-TG"]
    seqs = [b"AXYCTG", b"ZACTG", b"ACG", b"ACTGWW"]
    paths = [np.array(p, dtype=np.int8) for p in ([0, 1, 1, 0, 0, 0], [1, 0, 0, 0, 0], [0, 0, 2, 0], [0, 0, 0, 0, 1, 1])]
    _check_merge(backbone, seqs, paths, [[0, 1], [2], [3]])


def _random_path(rng, L):
    """A path over L backbone columns with some deletions and insertion runs; returns (path, number of letters)."""
    codes = []
    for c in range(L + 1):
        if rng.random() < 0.03:
            codes += [1] * int(rng.integers(1, 40))
        if c < L:
            codes.append(2 if rng.random() < 0.1 else 0)
    p = np.array(codes, dtype=np.int8)
    return p, int(np.count_nonzero(p != 2))


def test_collect_finish_random_long_paths_over_several_calls(gpu):
    """Paths longer than one tile of the scan (4096 codes), insertions at both ends, lowercase letters, several collect calls."""
    rng = np.random.default_rng(3)
    L = 6000
    backbone = [rng.choice(list(b"ACGTacgt-"), L).astype(np.uint8).tobytes() for _ in range(5)]
    seqs, paths = [], []
    for k in range(23):
        p, n = _random_path(rng, L)
        if k == 0:
            p = np.concatenate([np.ones(7, np.int8), p, np.ones(5, np.int8)]); n += 12
        seqs.append(rng.choice(list(b"ACGTNacgtn"), n).astype(np.uint8).tobytes())
        paths.append(p)
    _check_merge(backbone, seqs, paths, [list(range(0, 9)), list(range(9, 10)), list(range(10, 23))])


def test_collect_refuses_a_path_of_the_wrong_shape(gpu):
    from twilight_amd import place

    st = _store([b"ACGT", b"ACGT", b"AC"])
    pl = place.Placement(st, 4)
    with pytest.raises(Exception):
        pl.collect_host([2], [np.array([0, 0, 0], dtype=np.int8)])       # 3 backbone columns, 2 letters: not L = 4
    pl.collect_host([2], [np.array([0, 2, 2, 0], dtype=np.int8)])
    assert pl.finish([0, 1]) == 4
    assert st.rows_of([0, 1, 2]) == [b"ACGT", b"ACGT", b"A--C"]
    pl.close()
    st.close()


# ---- the command line against the oracle ----

def _write(records, path):
    PO.write(records, path)
    return str(path)


def _cli(tmp_path, backbone, new, *flags, tag="run", timeout=600):
    bb = backbone if isinstance(backbone, str) else _write(backbone, tmp_path / f"{tag}_bb.aln")
    nw = new if isinstance(new, str) else _write(new, tmp_path / f"{tag}_new.fa")
    out = tmp_path / f"{tag}_out.aln"
    r = subprocess.run(["timeout", "-k", "10", str(timeout), EXE, "-a", bb, "-i", nw, "-o", str(out), *flags], capture_output=True, text=True,
                       timeout=timeout + 30)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    return open(out, "rb").read(), r


def _invariants(blob, backbone, new_placed):
    recs = [tuple(x.split(b"\n")[:2]) for x in blob.split(b">")[1:]]
    W = len(recs[0][1])
    assert all(len(r) == W for _, r in recs)
    B = len(backbone)
    keep = [j for j in range(W) if not all(r[j] == ord(".") for _, r in recs[:B])]
    for (n, r), (bn, br) in zip(recs[:B], backbone):
        assert n == bn and bytes(r[j] for j in keep) == br
    for (n, r), (sn, s) in zip(recs[B:], new_placed):
        assert n == sn and r.replace(b"-", b"").replace(b".", b"") == s
    assert len(recs) == B + len(new_placed)


def test_cli_rnasim_fixture(gpu, tmp_path):
    import sys

    sys.path.insert(0, GOLDEN)
    import make_place_expected as MPE

    sub = str(tmp_path / "RNASim_sub.fa")
    MPE.write_sub_fasta(sub)
    blob, _ = _cli(tmp_path, os.path.join(GOLDEN, "RNASim_backbone.aln.gz"), sub, tag="rnasim")
    backbone, new = MPE.rnasim_inputs()
    want, _, _ = PO.place(backbone, new)
    assert blob == PO.to_bytes(want)
    exp = json.load(open(os.path.join(GOLDEN, "place_expected.json")))["rnasim"]
    assert hashlib.md5(blob).hexdigest() == exp["md5"]
    _invariants(blob, backbone, new)


# synthetic families

def _family(rng, letters, L, n_bb, n_new, *, gap_rate=0.04, gappy_cols=20, sub=0.05, ins=()):
    """A backbone of n_bb rows over one core (some columns almost all gaps, scattered gaps) and n_new new sequences: the core mutated, with
    the given (position, length) insertions of random letters."""
    core = rng.choice(letters, L).astype(np.uint8)
    bb = []
    gcols = rng.choice(L, gappy_cols, replace=False)
    for k in range(n_bb):
        r = core.copy()
        r[rng.random(L) < gap_rate] = ord("-")
        r[gcols] = ord("-")
        if k == 0:
            r[gcols] = core[gcols]                 # one row carries letters there: a gappy column, not an empty one
        bb.append((b"bb%d" % k, r.tobytes()))
    new = []
    for k in range(n_new):
        s = core.copy()
        m = rng.random(L) < sub
        s[m] = rng.choice(letters, int(m.sum()))
        s = bytearray(s.tobytes())
        for pos, ln in ins[k % len(ins)] if ins else ():
            s[pos:pos] = rng.choice(letters, ln).astype(np.uint8).tobytes()
        new.append((b"new%d" % k, bytes(s)))
    return bb, new


NUC = list(b"ACGT")
AA = list(b"ACDEFGHIKLMNPQRSTVWY")


def _against_oracle(tmp_path, bb, new, cli_flags=(), tag="f", seq_type="n", **oracle_kw):
    blob, r = _cli(tmp_path, bb, new, *cli_flags, tag=tag)
    want, longest, retries = PO.place(bb, new, seq_type, **oracle_kw)
    assert blob == PO.to_bytes(want)
    return blob, r, longest, retries


def test_cli_nucleotide_insertions(gpu, tmp_path):
    rng = np.random.default_rng(21)
    bb, new = _family(rng, NUC, 900, 30, 12, ins=[[(0, 5)], [(300, 12), (600, 3)], [(900, 8)], []])
    _, _, longest, _ = _against_oracle(tmp_path, bb, new)
    assert longest.sum() > 0


def test_cli_protein_blosum62(gpu, tmp_path):
    rng = np.random.default_rng(22)
    bb, new = _family(rng, AA, 500, 20, 10, ins=[[(100, 6)], []])
    _against_oracle(tmp_path, bb, new, ("--type", "p", "-b", "62"), seq_type="p")


def test_cli_gappy_threshold_one(gpu, tmp_path):
    rng = np.random.default_rng(23)
    bb, new = _family(rng, NUC, 700, 25, 8, ins=[[(50, 4)]])
    _against_oracle(tmp_path, bb, new, ("-r", "1"), thr=1.0)


def test_cli_low_quality_and_empty_sequences(gpu, tmp_path):
    rng = np.random.default_rng(24)
    bb, new = _family(rng, NUC, 600, 15, 6, ins=[[(200, 5)]])
    new.insert(2, (b"ambiguous", b"N" * 400 + new[0][1][:200]))
    new.insert(4, (b"empty", b""))
    new.append((b"new0", b"ACGT"))                       # a duplicate name: the first one is kept
    blob, r, _, _ = _against_oracle(tmp_path, bb, new)
    assert b">ambiguous" not in blob and b">empty\n" in blob
    assert "Low-quality sequences (not placed): 1" in r.stderr


def test_cli_no_insertion_keeps_backbone_rows(gpu, tmp_path):
    rng = np.random.default_rng(25)
    core = rng.choice(NUC, 800).astype(np.uint8).tobytes()
    bb = [(b"bb%d" % k, core) for k in range(10)]
    new = [(b"n%d" % k, core) for k in range(5)]
    blob, _, longest, _ = _against_oracle(tmp_path, bb, new)
    assert not longest.any()
    assert blob.startswith(PO.to_bytes(bb))


def test_cli_chunks_give_the_same_bytes(gpu, tmp_path):
    rng = np.random.default_rng(26)
    bb, new = _family(rng, NUC, 400, 12, 50, ins=[[(10, 3)], [(200, 7)], [], [(400, 2)]])
    one, _ = _cli(tmp_path, bb, new, tag="one")
    seven, r = _cli(tmp_path, bb, new, "--test-place-chunk", "7", tag="seven")
    assert seven == one
    assert "8 chunk(s)" in r.stderr
    want, _, _ = PO.place(bb, new)
    assert one == PO.to_bytes(want)


def test_cli_retries(gpu, tmp_path):
    """Pairs that fail the X-drop test (errorType 1) at a small X-drop are retried alone with a larger X-drop and band limit until they pass;
    -v shows each retry.  (The band-limit growth of errorType 2 goes through the same helper, nextRetryParams, as the deferred pass.)"""
    rng = np.random.default_rng(27)
    bb, new = _family(rng, NUC, 1500, 10, 3, sub=0.02)
    s = bytearray(new[1][1])
    s[500:500] = rng.choice(NUC, 600).astype(np.uint8).tobytes()          # an unrelated stretch
    new[1] = (new[1][0], bytes(s))
    blob, r, _, retries = _against_oracle(tmp_path, bb, new, ("--gap-extend", "-0.1", "-v"), gap_extend=-0.1)
    assert retries, "the oracle saw no retry: the case does not exercise the policy"
    lines = [x for x in r.stdout.splitlines() if x.startswith("Retry sequence")]
    assert lines == ["Retry sequence %s\txdrop %d flen %d" % (n.decode(), x, f) for n, x, f in retries]
