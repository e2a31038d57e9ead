"""The placement kernels (place_kernels.hip.h, twl_place.inc.hip) where scan_path's tiles and thread chunks, place_scan_kernel's rounds, the
row slices of count_columns_kernel, the planes and the path sources of twl_place_collect switch, against tests/place_oracle.py byte for
byte: integers and bytes only, no tolerance anywhere.  The inputs come from tests/place_cases.py; tests/test_place_edge_inputs_cpu.py
proves that each of them reaches the branch it is listed for."""
import numpy as np
import pytest

import place_cases as PC
import place_oracle as PO

pytestmark = pytest.mark.gpu


def _want(backbone, seqs, paths):
    longest = PO.merge_insertions(len(backbone[0]), paths)
    rows = [PO.expand_backbone(r, longest) for r in backbone] + [PO.expand_placed(s, np.asarray(p), longest) for s, p in zip(seqs, paths)]
    return longest, rows


def _place(backbone, seqs, paths, calls, extra=(), minimal_pitch=False):
    """One store (backbone rows, sequences, then `extra` rows that are never placed), one placement, collect_host in the given calls (lists
    of sequence indices; the insertion table is checked after every call against the oracle over what has been collected), finish:
    longest, W and every row equal the oracle's, and the extra rows are what they were."""
    import twilight_amd as twl
    from twilight_amd import api, level, place

    B, L = len(backbone), len(backbone[0])
    all_rows = list(backbone) + list(seqs) + list(extra)
    if minimal_pitch:
        twl.set_knob(api.KNOB_FAIL_ROW_ALLOCS, 1)          # the generous pitch fails: the store starts at the pitch its sequences need
    try:
        st = level.Store(all_rows, "n")
    finally:
        twl.set_knob(api.KNOB_FAIL_ROW_ALLOCS, 0)
    pl = place.Placement(st, L)
    done = []
    for g in calls:
        pl.collect_host([B + k for k in g], [paths[k] for k in g])
        done += list(g)
        assert np.array_equal(pl.insertions(), PO.merge_insertions(L, [paths[k] for k in done])), f"longest[] after the call of {list(g)}"
    assert sorted(done) == list(range(len(seqs)))
    longest, want = _want(backbone, seqs, paths)
    W = pl.finish(range(B))
    assert W == L + int(longest.sum())
    got = st.rows_of(list(range(len(all_rows))))
    for i, (g, w) in enumerate(zip(got, want + list(extra))):
        assert g == w, f"row {i} ({'backbone' if i < B else 'placed' if i < B + len(seqs) else 'not placed'})"
    pl.close()
    st.close()
    return W


# ---- (a) scan tiles ----

SCAN_CALLS = {
    "tiles-one_call_each": ("tiles", [[k] for k in range(8)]),
    "tiles-calls_of_3_1_4": ("tiles", [[0, 1, 2], [3], [4, 5, 6, 7]]),          # the atomicMax folds across calls as well
    "tiles2": ("tiles2", [[0, 1]]),
    "chunks": ("chunks", [[0, 1, 2, 3, 4, 5, 6]]),
    "len4095": ("len4095", [[0, 1]]),
    "len4096": ("len4096", [[1], [0]]),
    "len4097": ("len4097", [[0, 1]]),
}


@pytest.mark.parametrize("case", list(SCAN_CALLS))
def test_scan_tiles_and_thread_chunks(gpu, case):
    """scan_path: insertion runs that end on a tile's last code, cross a tile edge, fill one and two whole tiles, start the path and end it;
    runs on positions 14-17 of a thread's 16 codes; two runs of 3 and 5 in one slot; paths of exactly 4095, 4096 and 4097 codes."""
    name, calls = SCAN_CALLS[case]
    backbone, seqs, paths = PC.group_inputs(name)
    assert len(seqs) == sum(len(c) for c in calls)
    W = _place(backbone, seqs, paths, calls)
    if name == "tiles":
        assert W == 24250


# ---- (b) scan rounds and final width ----

@pytest.mark.parametrize("L", sorted(PC.ROUND_CASES))
def test_scan_rounds_and_final_width(gpu, L):
    """place_scan_kernel / place_colsrc_kernel / backbone_expand_kernel: L + 1 = 2, 256, 257, 258, 512, 513, 514, 1025 slots with insertions
    in slot 0, on both sides of every round's edge and in slot L; W = 256 (L = 1) and 257 (L = 255) exactly; at L = 257 the store starts at
    the pitch its sequences need and W lies beyond it, so twl_place_finish re-pitches the planes; a sequence that is not placed keeps its row."""
    backbone, seqs, paths, _ = PC.round_inputs(L)
    extra = [b"acgtNNAC-gt" * 3]
    W = _place(backbone, seqs, paths, [[0, 1], [2, 3]], extra=extra, minimal_pitch=bool(PC.ROUND_CASES[L][1]))
    total = PC.ROUND_CASES[L][0]
    if total is not None:
        assert W == L + total and W in (256, 257)


# ---- (c) column counts ----

COUNT_LENS = (1, 255, 256, 257)
COUNT_IDS = (1, 63, 64, 65, 128, 129)


def _count_rows(seq_type):
    """Rows of four lengths, interleaved (row i < 516 has length COUNT_LENS[i % 4]), then 871 more of 257 columns: 1000 of that length, all
    with the letter A (either case) in column 100.  Row 2 (256 columns) holds every byte value once, 0x00 and 0x80-0xFF included."""
    rng = np.random.default_rng(77)
    alphabet = list(b"ACGTUNacgtun-.RYKM") if seq_type == "n" else list(b"ACDEFGHIKLMNPQRSTVWYacdefghiklmnpqrstvwyXxNn-.BZ")
    lens = [COUNT_LENS[i % 4] for i in range(4 * 129)] + [257] * 871
    rows = [bytearray(rng.choice(alphabet, n).astype(np.uint8).tobytes()) for n in lens]
    for i, r in enumerate(rows):
        if len(r) == 257:
            r[100] = ord("Aa"[i % 2])
    rows[2] = bytearray(range(256))
    return [bytes(r) for r in rows]


@pytest.mark.parametrize("seq_type", ["n", "p"])
def test_count_columns_row_slices_and_lengths(gpu, seq_type):
    """count_columns_kernel: n_ids on both sides of one and two slices of 64 rows, L on both sides of one workgroup of 256 columns, a
    shuffled id list out of an interleaved store, 1000 rows whose 16 slices add into one cell, and every byte value: the device's table
    and level_oracle.lut agree on all 256 (bytes >= 0x80 and 0x00 are the wildcard, as the reference's unsigned table lookup has it)."""
    from twilight_amd import level, place

    rows = _count_rows(seq_type)
    st = level.Store(rows, seq_type)
    rng = np.random.default_rng(5)
    cache_id = 0
    for L in COUNT_LENS:
        cls = [i for i, r in enumerate(rows) if len(r) == L]
        for n in COUNT_IDS + ((1000,) if L == 257 else ()):
            ids = rng.permutation(cls)[:n].tolist()
            if L == 256 and 2 not in ids:
                ids[int(rng.integers(n))] = 2
            assert len(set(ids)) == n and (n < 8 or ids != sorted(ids))
            place.count_columns(st, ids, cache_id)
            want = PO.backbone_profile([rows[i] for i in ids], seq_type)
            assert np.array_equal(st.cache(cache_id), want), f"n_ids {n}, L {L}"
            if n == 1000:
                assert want[100, 0] == 1000
            cache_id += 1
    st.close()


# ---- (d) two rounds on one store ----

def test_second_round_reads_rows_of_both_planes(gpu):
    """After a first placement's finish its rows live in plane 1 at width W; a second round on the same store counts their columns together
    with a row of W columns that is still in plane 0, places further sequences (plane 0) and finishes with all of those as the backbone."""
    from twilight_amd import level, place

    rng = np.random.default_rng(41)
    L, B = 300, 2
    backbone = [rng.choice(list(b"ACGTacgt-"), L).astype(np.uint8).tobytes() for _ in range(B)]
    runs1 = [{0: 3, 150: 2}, {150: 6, 300: 1}, {}, {299: 4}]
    paths1 = [PC.make_path(L, r, tuple(range(k, L, 37))) for k, r in enumerate(runs1)]
    seqs1 = [PC.make_seq(rng, p) for p in paths1]
    longest1, rows1 = _want(backbone, seqs1, paths1)
    W1 = L + int(longest1.sum())
    assert W1 == 300 + 3 + 6 + 4 + 1
    late = rng.choice(list(b"ACGTacgt-"), W1).astype(np.uint8).tobytes()          # W1 columns from the start: never rewritten, plane 0
    runs2 = [{0: 2, 255: 3, 256: 1}, {W1: 5}, {256: 4, 100: 1}]
    paths2 = [PC.make_path(W1, r, tuple(range(3 + k, W1, 29))) for k, r in enumerate(runs2)]
    seqs2 = [PC.make_seq(rng, p) for p in paths2]
    backbone2 = rows1 + [late]
    longest2, rows2 = _want(backbone2, seqs2, paths2)

    n1 = B + len(seqs1)
    st = level.Store(backbone + seqs1 + [late] + seqs2, "n")
    pl = place.Placement(st, L)
    pl.collect_host(range(B, n1), paths1)
    assert pl.finish(range(B)) == W1
    assert st.rows_of(list(range(n1))) == rows1
    ids2 = list(range(n1 + 1))
    place.count_columns(st, ids2[::-1], 9)                                        # planes 1 ... 1, 0 in one launch
    assert np.array_equal(st.cache(9), PO.backbone_profile(backbone2, "n"))
    pl2 = place.Placement(st, W1)
    pl2.collect_host(range(n1 + 1, n1 + 1 + len(seqs2)), paths2)
    assert np.array_equal(pl2.insertions(), longest2)
    assert pl2.finish(ids2) == W1 + int(longest2.sum())
    assert st.rows_of(list(range(n1 + 1 + len(seqs2)))) == rows2
    pl2.close()
    pl.close()
    st.close()


# ---- (e) path sources through the ABI ----

def _abi_family():
    """8 backbone rows of 300 columns (columns 0, 50-52, 120 and 299 hold '-' in every row: removed at -r 0.95, kept at -r 1) and 6 new
    sequences: the core with substitutions and insertions."""
    rng = np.random.default_rng(91)
    L, B = 300, 8
    nuc = list(b"ACGT")
    core = rng.choice(nuc, L).astype(np.uint8)
    empty = [0, 50, 51, 52, 120, 299]
    backbone = []
    for k in range(B):
        r = core.copy()
        r[rng.random(L) < 0.04] = ord("-")
        r[empty] = ord("-")
        backbone.append(r.tobytes())
    keep = np.ones(L, dtype=bool)
    keep[empty] = False
    ins = [[(0, 5)], [(100, 12), (200, 3)], [(294, 8)], [], [(150, 30)], [(40, 2), (41, 2)]]
    seqs = []
    for k in range(6):
        s = core[keep].copy()
        m = rng.random(len(s)) < 0.05
        s[m] = rng.choice(nuc, int(m.sum()))
        s = bytearray(s.tobytes())
        for pos, n in reversed(ins[k]):
            s[pos:pos] = rng.choice(nuc, n).astype(np.uint8).tobytes()
        seqs.append(bytes(s))
    return backbone, seqs


ABI_RUNS = {
    # thr, pairs restored first, from_dp per pair (pair 2 is skipped with path_len 0; a 0 is a downloaded row handed back from the host)
    "thr1_dp_output": (1.0, [], [1, 0, 1, 1, 1, 1]),
    "thr1_dp_output_and_path_buffer": (1.0, [3, 5], [1, 0, 1, 2, 1, 2]),
    "thr095_path_buffer": (0.95, [0, 1, 2, 3, 4, 5], [2, 2, 2, 0, 2, 2]),
}


@pytest.mark.parametrize("run", list(ABI_RUNS))
def test_collect_from_the_level_buffers(gpu, run):
    """twl_place_collect's three sources as host/place.cpp drives them: count_columns, twl_level_prepare with the cached backbone as side
    0, twl_level_align with gapCharScore 0, (twl_level_restore,) collect with from_dp 1 = the DP output at pitch 2 * seq_len, 2 = the path
    buffer at the restore's pitch, 0 = a host row, and pair 2 of 6 skipped (path_len 0): the pairs behind it keep their own rows.
    twl_level_restore accepts a subset of pairs when no column was removed (-r 1) and copies their DP paths, so one run mixes 1 and 2."""
    import twilight_amd as twl
    from twilight_amd import level, place, synth

    thr, restored, from_dp = ABI_RUNS[run]
    backbone, seqs = _abi_family()
    B, L, n = len(backbone), len(backbone[0]), len(seqs)
    M = synth.nucleotide_matrix()
    st = level.Store(backbone + seqs, "n")
    place.count_columns(st, range(B), 0)
    prof = PO.backbone_profile(backbone, "n")
    assert np.array_equal(st.cache(0), prof)
    want_paths = [PO.place_one(prof, B, s, "n", M, thr=thr) for s in seqs]
    assert sum(int(np.count_nonzero(p == 1)) > 0 for p in want_paths) >= 4

    p, pz = twl.make_params(M), twl.make_params(M, gap_char=0.0)
    max_len = max([L] + [len(s) for s in seqs])
    pairs = [[level.Side(members=[], member_weight=[], len=L, num=B, weight=float(B), cache_id=0),
              level.Side(members=[B + k], member_weight=[1.0], len=len(seqs[k]), num=1, weight=1.0)] for k in range(n)]
    lens, _ = st.prepare(p, pairs, gappy_threshold=thr, seq_len=max_len)
    assert (lens[:, 0] < L).all() == (thr < 1.0)
    aln_len, err = st.align_in_hbm(pz)
    assert not err.any()
    stride = L + max_len
    plen = [int(x) for x in aln_len]
    got = [st.read_path(i, plen[i]) for i in range(n)]
    if restored:
        fin = st.restore(p, restored, stride)
        assert (fin > 0).all(), fin
        for t, i in enumerate(restored):
            plen[i] = int(fin[t])
            got[i] = st.read_final(i, plen[i])
    for i in range(n):
        assert np.array_equal(got[i], want_paths[i]), f"pair {i}: final path"

    skipped = 2
    pl = place.Placement(st, L)
    pl2 = place.Placement(st, L)
    call_len = [0 if i == skipped else plen[i] for i in range(n)]
    pl.collect_level([B + i for i in range(n)], call_len, stride, from_dp, paths=[got[i] if from_dp[i] == 0 and i != skipped else None for i in range(n)])
    first = [i for i in range(n) if i != skipped]
    pl2.collect_host([B + i for i in first], [got[i] for i in first])
    want_first = PO.merge_insertions(L, [want_paths[i] for i in first])
    assert np.array_equal(pl.insertions(), pl2.insertions())
    assert np.array_equal(pl.insertions(), want_first)
    pl.collect_host([B + skipped], [got[skipped]])                  # the skipped sequence arrives with a later call
    longest, want = _want(backbone, seqs, want_paths)
    assert np.array_equal(pl.insertions(), longest)
    assert pl.finish(range(B)) == L + int(longest.sum())
    assert st.rows_of(list(range(B + n))) == want
    pl2.close()
    pl.close()
    st.close()


# ---- (f) refusals ----

def test_bad_paths_next_to_good_ones(gpu):
    """One call with three good and three malformed paths is refused as a whole, the good three stay collected (include/twl_place.h) and
    nothing of the others is folded in: the right number of columns with one letter too few, one column too many, and a path of more than
    one tile whose only fault lies in its second tile."""
    from twilight_amd import level, place

    rng = np.random.default_rng(13)
    L, B = 4100, 2
    backbone = [rng.choice(list(b"ACGTacgt-"), L).astype(np.uint8).tobytes() for _ in range(B)]
    runs = [{4090: 6}, {7: 9, 2000: 2}, {0: 3, L: 4}, {7: 20}, {L: 11, 300: 1}, {4000: 120}]
    paths = [PC.make_path(L, r, (k, 4097 - k)) for k, r in enumerate(runs)]
    seqs = [PC.make_seq(rng, p) for p in paths]
    bad = {}
    bad[1] = paths[1].copy()
    bad[1][np.flatnonzero(bad[1] == 0)[5]] = 2                                   # L columns, one letter too few
    bad[3] = np.concatenate([paths[3], np.array([2], np.int8)])                  # L + 1 columns, within L + len
    bad[5] = paths[5].copy()
    at = 4096 + int(np.flatnonzero(bad[5][4096:] == 0)[3])
    bad[5][at] = 2                                                               # tile 0 is as it should be
    assert len(bad[5]) > 4096 and np.array_equal(bad[5][:4096], paths[5][:4096]) and len(bad[3]) <= L + len(seqs[3])
    good = [0, 2, 4]

    st = level.Store(backbone + seqs, "n")
    pl = place.Placement(st, L)
    with pytest.raises(Exception, match="3 paths"):
        pl.collect_host([B + k for k in range(6)], [bad.get(k, paths[k]) for k in range(6)])
    assert np.array_equal(pl.insertions(), PO.merge_insertions(L, [paths[k] for k in good]))
    with pytest.raises(Exception, match="collected twice"):
        pl.collect_host([B + good[1]], [paths[good[1]]])
    pl.collect_host([B + k for k in sorted(bad)], [paths[k] for k in sorted(bad)])
    longest, want = _want(backbone, seqs, paths)
    assert np.array_equal(pl.insertions(), longest)
    assert pl.finish(range(B)) == L + int(longest.sum())
    assert st.rows_of(list(range(B + 6))) == want
    pl.close()
    st.close()
