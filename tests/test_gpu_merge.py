"""The merge of existing alignments on the MI355X (include/twl_merge.h, `twilight-mi355x -f DIR -o OUT`): the map kernels and the row rewrite
through twilight_amd/merge.py with host-supplied paths, against their numpy versions (tests/merge_oracle.py) byte for byte, and the command
line against the CPU restatement of the mode.  Every CLI run has its own time limit."""
import gzip
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import merge_oracle as MO
from test_merge_cpu import HAND_FILES, HAND_MAPS_AFTER_1, HAND_MAPS_AFTER_2, HAND_PATHS, HAND_ROWS, _invariants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "twilight_amd", "twilight-mi355x")

pytestmark = pytest.mark.gpu

TILE = 4096        # kPlTile (place_kernels.hip.h): path codes per LDS tile of the rank kernel
ROWS_PER_WG = 16   # kMgRows (merge_kernels.hip.h): rows one workgroup of the rewrite takes
ALPHABET = list(b"ACGTacgtNn-.")


def _rows(rng, n, L):
    return [rng.choice(ALPHABET, L).astype(np.uint8).tobytes() for _ in range(n)]


def _path(rng, wr, wq, n0, lead1=0, tail2=0):
    """A path with exactly wr codes != 1 and wq codes != 2, n0 of them code 0: lead1 codes 1 first, tail2 codes 2 last, the rest shuffled."""
    n1, n2 = wq - n0 - lead1, wr - n0 - tail2
    assert n1 >= 0 and n2 >= 0
    mid = np.array([0] * n0 + [1] * n1 + [2] * n2, dtype=np.int8)
    rng.shuffle(mid)
    return np.concatenate([np.ones(lead1, np.int8), mid, np.full(tail2, 2, np.int8)])


class _Case:
    """A store, a device merge and its numpy twin, held together call by call."""

    def __init__(self, files):
        from twilight_amd import level, merge

        self.files = files
        flat = [r for f in files for r in f]
        self.ids, at = [], 0
        for f in files:
            self.ids.append(list(range(at, at + len(f))))
            at += len(f)
        self.store = level.Store(flat, "n")
        self.dev = merge.Merge(self.store, self.ids)
        self.ref = MO.Maps([len(f[0]) for f in files])

    def maps(self):
        return [self.dev.map(g).tolist() for g in range(len(self.files))]

    def check_maps(self):
        assert self.maps() == [p.tolist() for p in self.ref.pos]

    def apply(self, ref_groups, qry_groups, paths):
        self.dev.apply_host(ref_groups, qry_groups, paths)
        self.ref.apply(ref_groups, qry_groups, paths)
        self.check_maps()

    def finish(self):
        want, W = self.ref.rows(self.files)
        assert self.dev.finish() == W
        for ids, rows in zip(self.ids, want):
            assert self.store.rows_of(ids) == rows
        return W

    def close(self):
        self.dev.close()
        self.store.close()


def test_hand_worked_example(gpu):
    c = _Case(HAND_FILES)
    assert c.maps() == [[0, 1, 2], [0, 1], [0, 1, 2, 3]]
    c.dev.apply_host([[0]], [[2]], [np.array(HAND_PATHS[0], np.int8)])
    assert c.maps() == HAND_MAPS_AFTER_1
    c.dev.apply_host([[0, 2]], [[1]], [np.array(HAND_PATHS[1], np.int8)])
    assert c.maps() == HAND_MAPS_AFTER_2
    assert c.dev.finish() == 6
    assert [c.store.rows_of(ids) for ids in c.ids] == HAND_ROWS
    c.close()


@pytest.mark.parametrize("T", [TILE - 1, TILE, TILE + 1, 2 * TILE + 3])
def test_path_lengths_around_the_tile(gpu, T):
    """One merge whose path is T codes long: a tile less one, a tile, a tile and one, two tiles and three (W = T: neither a multiple of the 16
    columns a thread of the rewrite stores nor of its 4096-column workgroup).  The query group has one row."""
    rng = np.random.default_rng(T)
    wq, n0 = 501, 203
    wr = T - (wq - n0)
    c = _Case([_rows(rng, 3, wr), _rows(rng, 1, wq)])
    p = _path(rng, wr, wq, n0)
    assert len(p) == T
    c.apply([[0]], [[1]], [p])
    assert c.finish() == T
    c.close()


def test_path_of_zeros_only(gpu):
    """Both maps stay the identity, over more than one tile."""
    rng = np.random.default_rng(1)
    L = TILE + 777
    c = _Case([_rows(rng, 2, L), _rows(rng, 2, L)])
    c.apply([[0]], [[1]], [np.zeros(L, np.int8)])
    assert c.maps()[0] == list(range(L)) and c.maps()[1] == list(range(L))
    assert c.finish() == L
    assert c.store.rows_of([0, 1, 2, 3]) == c.files[0] + c.files[1]
    c.close()


def test_runs_longer_than_a_tile(gpu):
    """A run of query-only codes and a run of reference-only codes that each span more than a tile: whole rounds and tiles in which one of the
    two ranks does not move."""
    rng = np.random.default_rng(2)
    lead1, tail2 = TILE + 50, 2 * TILE + 7
    wr, wq, n0 = tail2 + 900, lead1 + 700, 333
    c = _Case([_rows(rng, 2, wr), _rows(rng, 3, wq)])
    c.apply([[0]], [[1]], [_path(rng, wr, wq, n0, lead1=lead1, tail2=tail2)])
    c.finish()
    c.close()


def test_row_slices_of_the_rewrite(gpu):
    """A group of 2 * 16 + 5 rows (three workgroups of the rewrite per column tile, the last one partial) next to a group of one row; L_g and W
    are odd."""
    rng = np.random.default_rng(3)
    c = _Case([_rows(rng, 2 * ROWS_PER_WG + 5, 301), _rows(rng, 1, 77), _rows(rng, ROWS_PER_WG, 130)])
    c.apply([[0]], [[1]], [_path(rng, 301, 77, 40)])
    c.apply([[0, 1]], [[2]], [_path(rng, 338, 130, 99)])
    assert c.finish() == 369
    c.close()


def test_three_successive_merges_as_a_star(gpu):
    """The CLI's shape: one pair per level, the reference side grows by a group each time, so the first groups' maps are composed three times."""
    rng = np.random.default_rng(4)
    L = [1500, 1400, 1700, 1601]
    c = _Case([_rows(rng, n, l) for n, l in zip([5, 3, 4, 2], L)])
    w = L[0]
    under = [0]
    for ch in (3, 2, 1):
        n0 = int(min(w, L[ch]) * 0.8)
        c.apply([list(under)], [[ch]], [_path(rng, w, L[ch], n0, lead1=int(ch == 2) * 9, tail2=int(ch == 1) * 11)])
        w = w + L[ch] - n0
        under.append(ch)
    assert c.finish() == w
    c.close()


def test_two_pairs_in_one_call_then_their_merge(gpu):
    """A level of two pairs in one launch, then a level whose two sides both hold two groups; a skipped pair (path_len 0) is left alone."""
    rng = np.random.default_rng(5)
    L = [5000, 4100, 300, 290]
    c = _Case([_rows(rng, 2, l) for l in L])
    pa, pb = _path(rng, L[0], L[1], 3900), _path(rng, L[2], L[3], 250)
    c.apply([[0], [2]], [[1], [3]], [pa, np.zeros(0, np.int8)])
    assert c.maps()[2] == list(range(L[2])) and c.maps()[3] == list(range(L[3]))
    c.apply([[2]], [[3]], [pb])
    c.apply([[0, 1]], [[2, 3]], [_path(rng, len(pa), len(pb), 300, lead1=5)])
    c.finish()
    c.close()


def test_a_malformed_path_is_refused_and_the_maps_stay(gpu):
    rng = np.random.default_rng(6)
    c = _Case([_rows(rng, 2, 3000), _rows(rng, 2, 2500), _rows(rng, 1, 40), _rows(rng, 1, 50)])
    c.apply([[2]], [[3]], [_path(rng, 40, 50, 30)])
    before = c.maps()
    good = _path(rng, 3000, 2500, 500)                              # (5000 codes: more than a tile)
    bad_ref = np.concatenate([good[good != 2][:10], good])           # ten codes != 2 more: the query side's count is off, the reference's too
    short = good[:-1]
    foreign = good.copy()
    foreign[TILE + 5] = 3
    small = _path(rng, 60, 60, 50)
    for paths, groups in (([bad_ref], ([[0]], [[1]])), ([short], ([[0]], [[1]])), ([foreign], ([[0]], [[1]])),
                          ([good, small[:-1]], ([[0], [2]], [[1], [3]]))):      # (a good and a malformed path in one call: neither is applied)
        with pytest.raises(Exception):
            c.dev.apply_host(groups[0], groups[1], paths)
        assert c.maps() == before
    with pytest.raises(Exception):
        c.dev.apply_host([[0]], [[0]], [good])                           # a group under both sides
    with pytest.raises(Exception):
        c.dev.apply_host([[0, 2]], [[1]], [good])                        # groups of two widths under one side
    assert c.maps() == before
    with pytest.raises(Exception):
        c.dev.finish()                                                   # not merged to one width yet
    c.apply([[0], [2]], [[1], [3]], [good, small])
    c.apply([[0, 1]], [[2, 3]], [_path(rng, len(good), len(small), 55)])
    c.finish()
    c.close()


def test_finish_twice_is_refused(gpu):
    rng = np.random.default_rng(7)
    c = _Case([_rows(rng, 2, 100), _rows(rng, 2, 90)])
    p = _path(rng, 100, 90, 70)
    c.apply([[0]], [[1]], [p])
    W = c.finish()
    rows = c.store.rows_of([0, 1, 2, 3])
    with pytest.raises(Exception):
        c.dev.finish()
    with pytest.raises(Exception):
        c.dev.apply_host([[0]], [[1]], [np.zeros(W, np.int8)])
    assert c.store.rows_of([0, 1, 2, 3]) == rows
    c.close()


def test_create_refuses_rows_of_two_lengths(gpu):
    from twilight_amd import level, merge

    st = level.Store([b"ACGT", b"ACG", b"AC"], "n")
    with pytest.raises(Exception):
        merge.Merge(st, [[0, 1], [2]])
    with pytest.raises(Exception):
        merge.Merge(st, [[0], [0]])
    st.close()


# ---- the command line ----

def _cli(*args, timeout=120):
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=timeout)


def _read_dir(d):
    return [MO.PO.read_fasta(f) for f in MO.list_files(d)]


def test_cli_rnasim_subalignments_match_the_pin(gpu, tmp_path):
    src = os.path.join(GOLDEN, "RNASim_subalignments")
    out = tmp_path / "out.aln"
    r = _cli("-f", src, "-o", str(out))
    assert r.returncode == 0, r.stderr
    want = json.load(open(os.path.join(GOLDEN, "merge_expected.json")))
    data = out.read_bytes()
    records = MO.PO.read_fasta(str(out))
    assert len(records) == want["rows"] and len(records[0][1]) == want["width"]
    _invariants(_read_dir(src), records, want["width"])
    assert hashlib.md5(data).hexdigest() == want["md5"]


def _protein_files(rng):
    """Three small alignments of one protein family: per file its own variant of a 260-letter ancestor (a deletion, an insertion), rows with
    point changes, a few lowercase letters and gaps."""
    acids = list(b"ACDEFGHIKLMNPQRSTVWY")
    anc = rng.choice(acids, 260).astype(np.uint8)
    files = []
    for k, n_rows in enumerate((4, 7, 5)):
        v = anc.copy()
        cut = int(rng.integers(20, 200))
        v = np.concatenate([v[:cut], v[cut + 6 + 3 * k:]])
        at = int(rng.integers(20, 200))
        v = np.concatenate([v[:at], rng.choice(acids, 4 + 5 * k).astype(np.uint8), v[at:]])
        recs = []
        for r in range(n_rows):
            row = v.copy()
            hit = rng.random(len(row)) < 0.08
            row[hit] = rng.choice(acids, int(hit.sum())).astype(np.uint8)
            gap = rng.random(len(row)) < 0.04
            row[gap] = ord("-")
            low = rng.random(len(row)) < 0.03
            row[low & ~gap] |= 0x20
            recs.append((b"f%d_r%d" % (k, r), row.tobytes()))
        files.append(recs)
    return files


def test_cli_three_protein_files_match_the_oracle(gpu, tmp_path):
    rng = np.random.default_rng(12)
    files = _protein_files(rng)
    d = tmp_path / "in"
    (d / "sub").mkdir(parents=True)
    for name, recs in zip(("a.aln", "b.aln.gz", "sub/c.aln"), files):      # (sorted by path: a nested directory last, one file gzipped)
        (d / name).write_bytes(gzip.compress(MO.to_bytes(recs)) if name.endswith(".gz") else MO.to_bytes(recs))
    want, W, _, _ = MO.merge(files, "p")
    out = tmp_path / "out.aln"
    r = _cli("-f", str(d), "-o", str(out), "--type", "p", "-b", "62")
    assert r.returncode == 0, r.stderr
    records = MO.PO.read_fasta(str(out))
    _invariants(files, records, len(records[0][1]))
    assert out.read_bytes() == MO.to_bytes(want) and len(records[0][1]) == W
    # the type is found in the first file when it is not given
    out2 = tmp_path / "out2.aln"
    r = _cli("-f", str(d), "-o", str(out2), "-b", "62")
    assert r.returncode == 0, r.stderr
    assert out2.read_bytes() == out.read_bytes()


def test_cli_single_file_is_written_back(gpu, tmp_path):
    d = tmp_path / "in"
    d.mkdir()
    data = b">a\nAC-g.\n>b\nACTG-\n"
    (d / "only.aln").write_bytes(data)
    out = tmp_path / "out.aln"
    r = _cli("-f", str(d), "-o", str(out))
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == data


def _files_with_one_gappy_block(rng, n_rows=24, flank=25, block=150):
    """Two nucleotide alignments of n_rows rows x (2 * flank + block) columns over one ancestor: in each, `block` columns at column `flank`
    in which exactly one row has letters and the others have gaps."""
    anc = rng.choice(list(b"ACGT"), 2 * flank).astype(np.uint8)
    files = []
    for k in range(2):
        recs = []
        for r in range(n_rows):
            mid = rng.choice(list(b"ACGT"), block).astype(np.uint8) if r == k else np.full(block, ord("-"), np.uint8)
            recs.append((b"f%d_r%d" % (k, r), np.concatenate([anc[:flank], mid, anc[flank:]]).tobytes()))
        files.append(recs)
    return files


def test_cli_two_sided_run_too_large_for_the_device_is_restored_on_the_host(gpu, tmp_path):
    """Both profiles lose a run of 150 columns at one step of the path (23 of 24 rows have gaps there: 23/24 > -r 0.95, compared with > in
    level_oracle.gappy_mask): the 151 x 151 alignment of the two runs does not fit the restore kernel's scratch (NW_CELLS), the device hands
    the pair back and the final path is made on the host -- the final-path step the tree path shares with -f and -a.  -v must say so and
    the output must be the oracle's, byte for byte.  (Placement has no such test: its query side is one sequence, which never loses a
    column, so no step of a placement's path has a run on both sides and nothing is handed back.)"""
    import level_cases as LC
    import level_oracle as LO

    files = _files_with_one_gappy_block(np.random.default_rng(24))
    # on the CPU first: both sides lose one run of 150 columns, at the same column, and the two together are too big for the device
    runs = []
    for recs in files:
        prof = MO.PO.backbone_profile([r for _, r in recs], "n")
        side = LO.profile_from_cache(prof, MO.F(len(recs)), len(recs))
        runs.append([tuple(int(x) for x in run) for run in LO.prepare_side(side, len(recs), 0.95, -50.0, -5.0, "n")[2]])
    assert runs[0] == runs[1] == [(25, 150)], runs
    assert LC.too_big(runs[0][0][1], runs[1][0][1])
    want, W, _, _ = MO.merge(files, "n")
    d = tmp_path / "in"
    d.mkdir()
    for name, recs in zip(("a.aln", "b.aln"), files):
        (d / name).write_bytes(MO.to_bytes(recs))
    out = tmp_path / "out.aln"
    r = _cli("-f", str(d), "-o", str(out), "-v")
    assert r.returncode == 0, r.stderr
    handed = sum(int(l.split("restored on the host ")[1].split(";")[0]) for l in r.stderr.splitlines() if "restored on the host" in l)
    assert handed >= 1, r.stderr
    assert out.read_bytes() == MO.to_bytes(want) and len(MO.PO.read_fasta(str(out))[0][1]) == W
