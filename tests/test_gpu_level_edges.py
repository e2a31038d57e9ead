"""The kernels around the DP (level_kernels.hip.h, restore_kernels.hip.h) where their scans, chunks and scratch tiers switch, against
oracle/level_oracle.py, bit for bit: floats as uint32, paths and rows as bytes, lengths and -1 codes as integers.  No tolerance anywhere.

The inputs come from level_cases.make_edge_case; what a restore case is meant to reach is written beside it (level_cases.restore_specs)
and asserted on the device's own DP path with level_cases.classify, as tests/test_level_edge_inputs_cpu.py asserts it on the DP oracle's."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import level_cases as LC  # noqa: E402
import level_oracle as LO  # noqa: E402
from test_gpu_level import _bits, _level  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32

SIDE_LENS = [(1, 4099), (2, 1025), (1024, 3), (4, 1023), (5, 257), (255, 256)]       # a short side next to a long one: chunks wholly behind a side's end
MEMBERS = {"n": [(1, 1000), (15, 16), (17, 33), (16, 1), (33, 17), (2, 15)], "p": [(1, 301), (2, 3), (3, 2), (301, 1), (2, 1), (3, 3)]}


def _side_shape(L):
    """kwargs of one side of `L` columns in all: longer sides carry a lead, a run and a trail of removed columns."""
    return dict(length=L, lead=0, trail=0, runs=()) if L < 8 else dict(length=L - 4, lead=1, trail=1, runs=((L // 2, 2),))


def _shaped_case(seq_type, seed, lens, members, thr, cached=0):
    a, b = _side_shape(lens[0]), _side_shape(lens[1])
    c = LC.make_edge_case(seq_type, seed, members=members, length=(a["length"], b["length"]), lead=(a["lead"], b["lead"]), trail=(a["trail"], b["trail"]),
                          runs=(a["runs"], b["runs"]), thr=thr, cached=cached)
    assert (len(c.sides[0].rows[0]), len(c.sides[1].rows[0])) == tuple(lens)
    return c


@pytest.mark.parametrize("thr", [0.6, 0.95, 1.0])
@pytest.mark.parametrize("seq_type", ["n", "p"])
def test_profiles_compaction_psgp_at_chunk_and_unroll_edges(gpu, seq_type, thr):
    """profile_kernel / compact_kernel: sides of 1-5, 255-257, 1 023-1 025 and 4 099 columns in ONE level (stride 4 099), member counts around
    the unrolled loads (16 nucleotide, 2 protein) up to 1 000 / 301, random fp32 weights (the order of the sum matters)."""
    import twilight_amd as twl
    from twilight_amd import level as L

    cases = [_shaped_case(seq_type, 40 + i, SIDE_LENS[i], MEMBERS[seq_type][i], thr) for i in range(len(SIDE_LENS))]
    seqs, pairs, ids = _level(cases, store_all=True)
    p = twl.make_params(LC.matrix_of(seq_type))
    st = L.Store(seqs, seq_type)
    lens, info = st.prepare(p, pairs, gappy_threshold=thr)
    removed = 0
    for i, c in enumerate(cases):
        for sd in range(2):
            s = c.sides[sd]
            k = len(s.rows)
            prof = LC.side_profile(c, sd)
            cols, inf, runs = LO.prepare_side(prof, k, thr, LC.GAP_OPEN, LC.GAP_EXTEND, seq_type)
            removed += len(runs)
            assert lens[i, sd] == cols.shape[0], f"pair {i} side {sd}: length after removal"
            assert np.array_equal(_bits(st.columns(i, sd)), _bits(cols)), f"pair {i} side {sd}: packed columns"
            assert np.array_equal(info[i, sd, : len(s.rows[0])], inf), f"pair {i} side {sd}: consensus / gappy flags"
            assert np.array_equal(_bits(st.cache(2 * i + sd)), _bits(LO.cache_from_profile(prof, s.group_weight, k))), f"pair {i} side {sd}: stored profile"
    assert (removed > 0) == (thr < 1.0)
    st.close()


@pytest.mark.parametrize("seq_type", ["n", "p"])
def test_cached_profiles_of_lengths_no_multiple_of_four(gpu, seq_type):
    """Level 1 stores every side's profile and merges the pairs' on commit; level 2 reads the merged profiles (cache_slot >= 0) of lengths
    that are no multiple of 4, next to each other in one level."""
    import twilight_amd as twl
    from twilight_amd import level as L

    shapes = [((1, 4099), (3, 2)), ((2, 1025), (2, 3)), ((5, 257), (17, 2)), ((255, 1023), (2, 16))]
    cases = [_shaped_case(seq_type, 60 + i, ln, mem, 0.95) for i, (ln, mem) in enumerate(shapes)]
    seqs, pairs, ids = _level(cases, store_all=True)
    p = twl.make_params(LC.matrix_of(seq_type))
    st = L.Store(seqs, seq_type)
    st.prepare(p, pairs)
    exps = [LC.expected(c) for c in cases]
    st.commit([e["path_full"] for e in exps])
    merged, sides2 = [], []
    for i, (c, e) in enumerate(zip(cases, exps)):
        caches = [LO.cache_from_profile(LC.side_profile(c, sd), c.sides[sd].group_weight, len(c.sides[sd].rows)) for sd in range(2)]
        m = LO.update_frequency(caches[0], caches[1], e["path_full"], c.sides[0].group_weight, c.sides[1].group_weight)
        assert np.array_equal(_bits(st.cache(2 * i)), _bits(m)), f"pair {i}: merged cache"
        merged.append(m)
        k = len(c.sides[0].rows) + len(c.sides[1].rows)
        gw = float(F(F(c.sides[0].group_weight) + F(c.sides[1].group_weight)))
        w_all = np.concatenate([c.sides[0].seq_weights, c.sides[1].seq_weights])
        sides2.append((L.Side(members=ids[i][0] + ids[i][1], member_weight=LO.member_weights(w_all, gw, k), len=len(e["path_full"]), num=k, weight=gw, cache_id=2 * i), k, gw))
    assert sum(len(m) % 4 != 0 for m in merged) >= 2
    lens, info = st.prepare(p, [[sides2[0][0], sides2[1][0]], [sides2[3][0], sides2[2][0]]])
    for pi, sd, j in ((0, 0, 0), (0, 1, 1), (1, 0, 3), (1, 1, 2)):
        prof = LO.profile_from_cache(merged[j], sides2[j][2], sides2[j][1])
        cols, inf, _ = LO.prepare_side(prof, sides2[j][1], 0.95, LC.GAP_OPEN, LC.GAP_EXTEND, seq_type)
        assert lens[pi, sd] == cols.shape[0]
        assert np.array_equal(_bits(st.columns(pi, sd)), _bits(cols)), f"level 2 pair {pi} side {sd}: columns from the merged cache"
        assert np.array_equal(info[pi, sd, : len(merged[j])], inf)
    st.close()


def _path_of(rng, len_r, len_q, n):
    """A path of exactly n elements over len_r reference and len_q query columns."""
    m = len_r + len_q - n
    assert 0 <= m <= min(len_r, len_q)
    codes = np.concatenate([np.zeros(m, np.int8), np.full(len_r - m, 2, np.int8), np.full(len_q - m, 1, np.int8)])
    return rng.permutation(codes)


COMMIT_LEVELS = {
    # (path length or 0 for a pair left out, members ref, members query); the longest path is the row pitch of the path buffer
    "pitch_140001": [(140001, 130, 1), (65537, 65, 9), (65536, 64, 8), (0, 3, 2), (65535, 63, 7), (257, 1, 1), (256, 7, 2), (255, 2, 9)],      # rows 1.. not 16-byte aligned
    "pitch_65536": [(65536, 9, 65), (65535, 8, 1), (0, 2, 2), (65536, 1, 64), (257, 63, 2), (256, 2, 7), (255, 1, 1)],                          # every row aligned
}


@pytest.mark.parametrize("level", sorted(COMMIT_LEVELS))
def test_write_back_of_caller_built_paths(gpu, level):
    """path_scan_kernel (one scan round per 65 536 elements, the 16-byte path only for aligned rows and full chunks), apply_path_kernel
    (8 members per round, 64 per workgroup), merge_cache_kernel on the chunk bases of a long path; one pair is left out like a deferred
    pair, and the aligned level starts from the minimal row pitch, so its commit has to re-pitch the planes."""
    import twilight_amd as twl
    from twilight_amd import api, level as L

    rng = np.random.default_rng(len(level))
    spec = COMMIT_LEVELS[level]
    cases, paths = [], []
    for i, (n, kr, kq) in enumerate(spec):
        nn = n if n else 300
        lr = int(nn * 0.7) + i
        lq = nn - lr + int(nn * 0.45)
        c = LC.make_edge_case("n", 80 + i, members=(kr, kq), length=(lr, lq), thr=1.0)
        cases.append(c)
        paths.append(_path_of(rng, lr, lq, n) if n else np.zeros(0, np.int8))
    seqs, pairs, ids = _level(cases, store_all=True)
    p = twl.make_params(LC.matrix_of("n"))
    if level == "pitch_65536":
        twl.set_knob(api.KNOB_FAIL_ROW_ALLOCS, 1)          # the generous pitch fails: the store starts at the pitch its sequences need
    try:
        st = L.Store(seqs, "n")
    finally:
        twl.set_knob(api.KNOB_FAIL_ROW_ALLOCS, 0)
    st.prepare(p, pairs, gappy_threshold=1.0)
    stride = max(len(x) for x in paths)
    assert (stride % 16 == 0) == (level == "pitch_65536")
    st.commit(paths)
    rows = st.rows()
    for i, (c, path) in enumerate(zip(cases, paths)):
        if len(path) == 0:
            for sid in ids[i][0] + ids[i][1]:
                assert rows[sid] == seqs[sid], f"pair {i}: row {sid} of a pair left out changed"
            continue
        for sd in range(2):
            for m, sid in enumerate(ids[i][sd]):
                assert rows[sid] == LO.apply_path(c.sides[sd].rows[m], path, 2 - sd), f"pair {i} side {sd}: row of member {m} after write-back"
    for i in (0, 1, 2) if level == "pitch_140001" else (0, 3):          # merged caches of paths beyond / at one scan round
        c = cases[i]
        caches = [LO.cache_from_profile(LC.side_profile(c, sd), c.sides[sd].group_weight, len(c.sides[sd].rows)) for sd in range(2)]
        m = LO.update_frequency(caches[0], caches[1], paths[i], c.sides[0].group_weight, c.sides[1].group_weight)
        assert np.array_equal(_bits(st.cache(2 * i)), _bits(m)), f"pair {i}: merged cache along a path of {len(paths[i])}"
    st.close()


def _restore_level(twl, seq_type, cases, specs, thr=0.95, out_stride=None, select=None, store_all=False, keep=None):
    """prepare -> align_in_hbm -> restore -> read_final -> (write_final for handed-back pairs) -> commit_from_dp(restored=...), every step
    against the checker.  specs[i] is None for an ordinary pair: it must not be handed back.  keep: a dict that receives what the run left
    (rows, the DP lengths, the committed lengths and, with store_all, the cached profile under every reference side's id) for tests that
    hold another flow to this one (tests/test_gpu_level_exchange.py)."""
    from twilight_amd import level as L

    seqs, pairs, ids = _level(cases, store_all=store_all)
    p = twl.make_params(LC.matrix_of(seq_type))
    st = L.Store(seqs, seq_type)
    lens, info = st.prepare(p, pairs, gappy_threshold=thr)
    n, err = st.align_in_hbm(p)
    assert not err.any()
    stride = out_stride or max(len(c.sides[0].rows[0]) + len(c.sides[1].rows[0]) for c in cases)
    lost = [i for i, c in enumerate(cases) if tuple(lens[i]) != (len(c.sides[0].rows[0]), len(c.sides[1].rows[0]))]
    sel = [i for i in lost if select is None or select(i)]
    fin = st.restore(p, sel, stride)
    exps, plen, written = {}, [int(x) for x in n], []
    for t, i in enumerate(sel):
        path = st.read_path(i, int(n[i]))
        e = exps[i] = LC.expected(cases[i], path_wo_gc=path)
        hb = False
        if specs[i] is not None:
            LC.check_spec(specs[i], LC.classify(cases[i], path, e))       # the device's own path reaches the branch the case exists for
            hb = specs[i].hand_back
        if hb:
            assert fin[t] == -1, f"pair {i} ({specs[i].name}): final_len {fin[t]}, the device must hand it back"
            written.append(i)
        else:
            assert fin[t] == len(e["path_full"]), f"pair {i}: final_len {fin[t]}, want {len(e['path_full'])}"
            assert np.array_equal(st.read_final(i, int(fin[t])), e["path_full"]), f"pair {i}: restored path"
        plen[i] = len(e["path_full"])
    for i in written:
        st.write_final(i, exps[i]["path_full"])
    for i in lost:
        if i not in exps:                                   # removed columns, not selected: left out of the commit like a deferred pair
            plen[i] = 0
    st.commit_from_dp([None] * len(cases), plen, stride=stride, restored=sel)
    rows = st.rows()
    for i, c in enumerate(cases):
        flat = ids[i][0] + ids[i][1]
        if i in exps:
            want = exps[i]["rows_after"]
        elif plen[i] == 0:
            want = [seqs[s] for s in flat]
        else:                                               # nothing removed: the DP path is the final path
            continue
        for sid, w in zip(flat, want):
            assert rows[sid] == w, f"pair {i}: row {sid} after write-back"
    if keep is not None:
        keep.update(rows=rows, dp_len=[int(x) for x in n], plen=list(plen), caches=[st.cache(2 * i) for i in range(len(cases))] if store_all else None)
    st.close()
    return sel, fin


@pytest.mark.parametrize("group", ["scan", "runs"])
@pytest.mark.parametrize("seq_type", ["n", "p"])
def test_restore_scan_rounds_tiers_and_queued_segments(gpu, seq_type, group):
    """restore_index / runs / count / write kernels at 1 023-1 025, 8 191-8 193 and 20 000 path elements with runs throughout (group scan);
    leads and trails on one and both sides, 3 x 3 ... 31 x 127 and 2 047 x 1 in LDS and global scratch, one-sided runs of 32-5 000 columns
    (group runs).  No pair may be handed back."""
    specs = LC.restore_specs(seq_type, group)
    sel, fin = _restore_level(gpu, seq_type, [s.case for s in specs], specs)
    assert len(sel) == len(specs) and (fin > 0).all(), fin


@pytest.mark.parametrize("seq_type", ["n", "p"])
def test_hand_back_between_ordinary_pairs(gpu, seq_type):
    """32 x 127, 1 x 128 and 150 x 150 are handed back (-1) and no other pair of the call; after the caller has written their final paths
    (twl_level_write_final) the commit leaves the checker's rows for all of them."""
    specs = LC.restore_specs(seq_type, "hand_back")
    sel, fin = _restore_level(gpu, seq_type, [s.case for s in specs], specs)
    assert [i for t, i in enumerate(sel) if fin[t] == -1] == [i for i, s in enumerate(specs) if s.hand_back]


def test_mixed_level_selects_a_subset_in_ascending_order(gpu):
    """>= 300 ordinary pairs with the edge pairs scattered among them; only a subset is restored, so slot indices differ from pair indices."""
    specs_e = LC.restore_specs("n", "runs")[::2] + LC.restore_specs("n", "scan")[:3]
    cases, specs = [], []
    for seed in range(300):
        cases.append(LC.make_case("n", seed, cached=0, length=70 + (seed % 13) * 11, thr=0.6))
        specs.append(None)
        if seed % 20 == 7 and specs_e:
            s = specs_e.pop()
            s.case.thr = 0.6                                # (the level's threshold; a single-member side has gap fractions 0 and 1 only)
            cases.append(s.case)
            specs.append(s)
    assert not specs_e
    sel, fin = _restore_level(gpu, "n", cases, specs, thr=0.6, select=lambda i: specs[i] is not None or i % 3 != 1)
    assert len(sel) >= 150 and sel == sorted(sel) and sel != list(range(len(sel))) and (fin > 0).all()


def test_out_stride_one_byte_short(gpu):
    """restore_write_kernel: a final path that does not fit out_stride is not written and reports -1; its neighbours are intact."""
    import twilight_amd as twl
    from twilight_amd import level as L

    specs = [s for s in LC.restore_specs("n", "runs") if s.name in ("lead31x31", "long_one_sided", "mid5x32", "trail3x3")]
    cases = [s.case for s in specs]
    seqs, pairs, ids = _level(cases)
    p = twl.make_params(LC.matrix_of("n"))
    st = L.Store(seqs, "n")
    st.prepare(p, pairs, gappy_threshold=0.95)
    n, err = st.align_in_hbm(p)
    assert not err.any()
    exps = [LC.expected(c, path_wo_gc=st.read_path(i, int(n[i]))) for i, c in enumerate(cases)]
    final = [len(e["path_full"]) for e in exps]
    longest = int(np.argmax(final))
    assert sorted(final)[-1] > sorted(final)[-2] and specs[longest].name == "long_one_sided"
    fin = st.restore(p, list(range(len(cases))), final[longest] - 1)
    for i, e in enumerate(exps):
        if i == longest:
            assert fin[i] == -1, fin
        else:
            assert fin[i] == final[i] and np.array_equal(st.read_final(i, final[i]), e["path_full"]), f"pair {i}: neighbour of the path that did not fit"
    st.close()


def test_more_pairs_than_one_restore_batch(gpu):
    """twl_level_restore works in batches of 4 096 pairs: 4 100 tiny pairs, the first and last pair of each batch and a sample in between."""
    import twilight_amd as twl
    from twilight_amd import level as L

    N = 4100
    cases = [LC.make_edge_case("n", 9000 + i, length=30 + i % 11, identical=True, lead=(i % 3, (i // 3) % 2), trail=((i // 5) % 2, i % 4 == 0), runs=([(9, 1 + i % 2)], [(9 + i % 2, 1)]))
             for i in range(N)]
    seqs, pairs, ids = _level(cases)
    p = twl.make_params(LC.matrix_of("n"))
    st = L.Store(seqs, "n")
    lens, info = st.prepare(p, pairs, gappy_threshold=0.95)
    n, err = st.align_in_hbm(p)
    assert not err.any()
    stride = max(len(c.sides[0].rows[0]) + len(c.sides[1].rows[0]) for c in cases)
    fin = st.restore(p, list(range(N)), stride)
    assert (fin > 0).all()
    for i in sorted({0, 1, 4094, 4095, 4096, 4097, N - 1} | set(range(0, N, 131))):
        e = LC.expected(cases[i], path_wo_gc=st.read_path(i, int(n[i])))
        assert fin[i] == len(e["path_full"]) and np.array_equal(st.read_final(i, int(fin[i])), e["path_full"]), f"pair {i}"
    st.close()
