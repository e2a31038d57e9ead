"""A level's final paths between ranks without leaving HBM (include/twl_level.h: twl_level_paths_to_block / rows_to_block_kernel,
twl_level_paths_from_block / block_to_rows_kernel, and the commit of path-buffer rows that came out of a block), with several ranks on
ONE device: W stores of the same sequences each play one rank of a sharded run, the test moves the blocks between them (device -> host
-> every rank's receive buffer) where a run on W devices has its all-gather.

Everything is bytes: a rank's block against the restatement of the layout (tests/exchange_cases.py, held to the host's function by
tests/test_exchange_plan_cpu.py) over a buffer full of a sentinel, the unpacked rows against the owner's final path followed by the
sentinel, the rows and merged profiles after the commit against the single-store flow of tests/test_gpu_level_edges.py and the level
oracle.  No tolerance anywhere.  What the levels contain is asserted on the checker's paths by tests/test_exchange_inputs_cpu.py and
here again on the device's own."""
import os
import sys
from collections import Counter

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import exchange_cases as EC  # noqa: E402
import level_cases as LC  # noqa: E402
import level_oracle as LO  # noqa: E402
from test_gpu_level import _bits, _level  # noqa: E402
from test_gpu_level_edges import _restore_level  # noqa: E402

pytestmark = pytest.mark.gpu
SENT = bytes([EC.SENTINEL])


def _words(r, level_no):
    """The four header words of rank r's block: any numbers, different per rank."""
    return (10 ** 12 + 17 * r, r, 0.5 * (r + 1), level_no)


def _sentinel_row(n):
    return np.full(n, EC.SENTINEL, dtype=np.uint8).view(np.int8)


def _exchange_level(twl, stores, seq_type, cases, pairs, owner, takes_part, descending=(), thr=0.95, level_no=1, hand_back=(), gaps=None):
    """The rank flow of one level on stores[r] for r in range(W), all W levels prepared at once.  Per rank: prepare, align_in_hbm of the
    owned pairs, restore of the owned pairs that lost columns, write_final of the ones handed back, exchange_buffers, sentinel fill of
    send, header upload, paths_to_block; then the gather; then per rank: the headers back, sentinel fill of the foreign rows of the path
    buffer, paths_from_block, commit_from_dp (owned pairs 1 or 2, foreign pairs 2).  Returns what the level left."""
    from twilight_amd import api

    W, n = len(stores), len(cases)
    p = twl.make_params(LC.matrix_of(seq_type), **(gaps or {}))
    orig = [(len(c.sides[0].rows[0]), len(c.sides[1].rows[0])) for c in cases]
    pl = EC.plan(owner, takes_part, [a + b for a, b in orig], W, descending)
    assert sorted(i for m in pl.mine for i in m) == [i for i in range(n) if takes_part[i]]
    exps, final, where, dp_len, lost_of = {}, {}, {}, {}, {}
    for r, st in enumerate(stores):
        lens, _ = st.prepare(p, pairs, gappy_threshold=thr)
        mask = np.array([bool(takes_part[i]) and owner[i] == r for i in range(n)])
        dl, err = st.align_in_hbm(p, run_mask=mask)
        assert not err.any() and not dl[~mask].any() and (dl[mask] > 0).all()
        lost_of[r] = [i for i in range(n) if mask[i] and tuple(lens[i]) != orig[i]]
        for i in np.flatnonzero(mask):
            path = st.read_path(int(i), int(dl[i]))
            e = exps[int(i)] = LC.expected(cases[i], path_wo_gc=path)
            final[int(i)], where[int(i)], dp_len[int(i)] = len(e["path_full"]), (2 if int(i) in lost_of[r] else 1), int(dl[i])
            assert where[int(i)] == 2 or np.array_equal(e["path_full"], path)
    stride = max(final.values())                       # the longest final path of the level, exactly
    blocks, ptrs, sent = [], [], []
    for r, st in enumerate(stores):
        send, recv = st.exchange_buffers(pl.block_max, pl.block_max * W)
        assert send and recv and send != recv
        with pytest.raises(api.TwlError, match="twl_level_restore first"):      # the row pitch of the path buffer is not fixed yet (and the pitch of an earlier level is gone)
            st.paths_to_block([0], [1], [2], send, [64])
        fin = st.restore(p, lost_of[r], stride)
        for t, i in enumerate(lost_of[r]):
            if i in hand_back:
                assert fin[t] == -1, f"rank {r} pair {i}: final_len {fin[t]}, the device must hand it back"
                st.write_final(i, exps[i]["path_full"])
            else:
                assert fin[t] == final[i], f"rank {r} pair {i}: final_len {fin[t]}, want {final[i]}"
        api.copy_to_device(send, SENT * pl.block_max)
        mine = pl.mine[r]
        lens_r, errs_r = [final[i] for i in mine], [0] * len(mine)
        api.copy_to_device(send, EC.header_bytes(pl, r, _words(r, level_no), lens_r, errs_r))
        off, end = EC.row_offsets(pl, r, lens_r)
        assert end <= pl.block_max
        st.paths_to_block(mine, lens_r, [where[i] for i in mine], send, off)
        blk = api.copy_from_device(send, pl.block_max)
        want = EC.block_bytes(pl, r, _words(r, level_no), lens_r, errs_r, [exps[i]["path_full"] for i in mine])
        if blk != want:
            at = next(k for k in range(pl.block_max) if blk[k] != want[k])
            raise AssertionError(f"rank {r}: block differs from byte {at} on (header {pl.hdr[r]}, offsets {off}, lengths {lens_r}, kinds {[where[i] for i in mine]})")
        blocks.append(blk)
        ptrs.append((send, recv))
        sent.append(Counter(where[i] for i in mine))
    for _, recv in ptrs:                               # the all-gather
        for r in range(W):
            api.copy_to_device(recv + pl.block_max * r, blocks[r])
    rows, unpacked = [], []
    for q, st in enumerate(stores):
        recv = ptrs[q][1]
        hb = api.copy_rows_from_device(recv, pl.block_max, pl.hdr_max, W)
        foreign, lens_f, off_f = [], [], []
        for r in range(W):
            lens_r = [final[i] for i in pl.mine[r]]
            assert hb[pl.hdr_max * r: pl.hdr_max * r + pl.hdr[r]] == EC.header_bytes(pl, r, _words(r, level_no), lens_r, [0] * len(lens_r)), f"rank {q}: header of rank {r}"
            if r != q:
                off, _ = EC.row_offsets(pl, r, lens_r)
                foreign += pl.mine[r]; lens_f += lens_r; off_f += [pl.block_max * r + o for o in off]
        for i in foreign:
            st.write_final(i, _sentinel_row(stride))
        before = [st.read_final(i, stride).tobytes() for i in range(n)]
        st.paths_from_block(foreign, lens_f, recv, off_f)
        for i in range(n):
            got = st.read_final(i, stride).tobytes()
            if i in foreign:
                assert got == exps[i]["path_full"].tobytes() + SENT * (stride - final[i]), f"rank {q}: received row of pair {i} ({final[i]} codes, kind {where[i]} at its owner)"
            else:
                assert got == before[i], f"rank {q}: row of pair {i} changed though nothing was unpacked into it"
        plen = [final.get(i, 0) for i in range(n)]
        st.commit_from_dp([None] * n, plen, stride=stride, restored=set(foreign) | {i for i in pl.mine[q] if where[i] == 2})
        rows.append(st.rows())
        unpacked.append(len(foreign))
    return dict(plan=pl, exps=exps, final=final, where=where, dp_len=dp_len, stride=stride, rows=rows, sent=sent, unpacked=unpacked, ptrs=ptrs)


def _after_commit(res, cases, ids, seqs_before, stores, caches=True):
    """Every rank's rows (and merged profiles) against the level oracle; pairs that took no part keep their rows."""
    for q, rows in enumerate(res["rows"]):
        for i, c in enumerate(cases):
            flat = ids[i][0] + ids[i][1]
            want = res["exps"][i]["rows_after"] if i in res["exps"] else [seqs_before[s] for s in flat]
            for sid, w in zip(flat, want):
                assert rows[sid] == w, f"rank {q} pair {i}: row {sid} after the commit"


@pytest.fixture(scope="module")
def main_n(gpu):
    """The nucleotide level and its single-store run (prepare -> align -> restore -> commit on one store that owns every pair)."""
    lv = EC.main_level("n")
    specs = [LC.EdgeSpec(x.name, x.case, frozenset({"hand_back"}), hand_back=True) if x.hand_back else None for x in lv.pairs]
    ref = {}
    _restore_level(gpu, "n", lv.cases, specs, thr=lv.thr, select=lambda i: lv.pairs[i].where != 0, store_all=True, keep=ref)
    return lv, ref


def _check_level_one(lv, res, ref, ids, seqs, stores):
    """What a level-1 run of lv must have met and left, whatever the ownership."""
    hand_back = {i for i, x in enumerate(lv.pairs) if x.hand_back}
    for i, x in enumerate(lv.pairs):                   # the device's own paths are of the kind and length the pair exists for
        if x.where:
            assert res["where"][i] == x.where and (x.final_len is None or res["final"][i] == x.final_len), f"{x.name}: kind {res['where'][i]}, {res['final'][i]} codes"
            assert res["dp_len"][i] == ref["dp_len"][i] and res["final"][i] == ref["plen"][i]
        else:
            assert i not in res["final"] and ref["plen"][i] == 0
    assert res["stride"] == 600 == max(res["final"][i] for i in res["final"] if res["where"][i] == 2)
    _after_commit(res, lv.cases, ids, seqs, stores)
    for q, st in enumerate(stores):
        assert res["rows"][q] == ref["rows"], f"rank {q}: rows differ from the single-store run"
        for i, x in enumerate(lv.pairs):
            if x.where:
                got = _bits(st.cache(2 * i))
                assert np.array_equal(got, _bits(ref["caches"][i])), f"rank {q} pair {i}: merged profile differs from the single-store run"
                assert np.array_equal(got, _bits(EC.node_side(x, res["exps"][i]).cache)), f"rank {q} pair {i}: merged profile"
    return hand_back


@pytest.mark.parametrize("ownership", [o.name for o in EC.main_level("n").ownerships])
def test_ranks_exchange_a_level(gpu, main_n, ownership):
    """W = 2, 3 and 8; round robin, a rank that owns nothing (and one that packs in descending pair order), a rank that owns all; blocks with
    rows of both kinds interleaved and blocks of one kind; paths of 1, 7, 8, 9, 255, 256, 257 and 513 codes of both kinds, a restored path
    of exactly out_stride, a pair handed back and written by its owner, a pair that takes no part."""
    from twilight_amd import level as L

    lv, ref = main_n
    own = next(o for o in lv.ownerships if o.name == ownership)
    seqs, pairs, ids = _level(lv.cases, store_all=True)
    stores = [L.Store(seqs, "n") for _ in range(own.world)]
    try:
        res = _exchange_level(gpu, stores, "n", lv.cases, pairs, own.owner, lv.takes_part, own.descending, thr=lv.thr,
                              hand_back={i for i, x in enumerate(lv.pairs) if x.hand_back})
        _check_level_one(lv, res, ref, ids, seqs, stores)
        # the rows the helper sent, per kind: both kernels ran, and the two-launch path of one call did
        n_part = sum(lv.takes_part)
        assert sum(sum(c.values()) for c in res["sent"]) == n_part
        for q in range(own.world):
            assert res["unpacked"][q] == n_part - sum(res["sent"][q].values())
            assert res["unpacked"][q] >= 1 or sum(res["sent"][q].values()) == n_part, f"rank {q} unpacked nothing"
        assert sum(res["unpacked"]) >= 1
        both = [q for q in range(own.world) if res["sent"][q][1] >= 2 and res["sent"][q][2] >= 2]
        one = [q for q in range(own.world) if len(res["sent"][q]) == 1]
        if ownership == "w8_round_robin":
            assert one and not both
        else:
            assert both
        assert [dict(c) for c in res["sent"]] == [dict(Counter(k)) for _, k in sorted(EC.kinds_per_rank(lv, own).items())]
    finally:
        for st in stores:
            st.close()


def test_two_levels_on_the_same_stores(gpu, main_n):
    """Level 2 aligns merged nodes of level 1 with other owners, a smaller out_stride (the row pitch of level 1 must not survive its
    commit) and smaller blocks in the grow-only exchange buffers, which still hold level 1's bytes behind the new ones."""
    from twilight_amd import level as L

    lv, ref = main_n
    own = lv.ownerships[0]
    seqs, pairs, ids = _level(lv.cases, store_all=True)
    stores = [L.Store(seqs, "n") for _ in range(own.world)]
    try:
        res1 = _exchange_level(gpu, stores, "n", lv.cases, pairs, own.owner, lv.takes_part, thr=lv.thr, hand_back={i for i, x in enumerate(lv.pairs) if x.hand_back})
        _check_level_one(lv, res1, ref, ids, seqs, stores)
        cases2 = EC.second_level(lv, [res1["exps"].get(i) for i in range(len(lv.pairs))])
        pairs2, ids2 = [], []
        for c, ab in zip(cases2, EC.second_level_pairs(lv)):
            sides = []
            for s, i in zip(c.sides, ab):
                members = ids[i][0] + ids[i][1]
                sides.append(L.Side(members=members, member_weight=LO.member_weights(s.seq_weights, s.group_weight, len(members)), len=len(s.rows[0]), num=len(members),
                                    weight=s.group_weight, cache_id=2 * i))
            pairs2.append(sides)
            ids2.append([sd.members for sd in sides])
        own2 = EC.second_level_owner(lv, own)
        rows1 = res1["rows"][0]
        res2 = _exchange_level(gpu, stores, "n", cases2, pairs2, own2, [1] * len(cases2), thr=lv.thr, level_no=2)
        assert res2["stride"] < res1["stride"] and res2["plan"].block_max < res1["plan"].block_max
        assert {s for s, _ in res2["ptrs"]} <= {s for s, _ in res1["ptrs"]} and {r for _, r in res2["ptrs"]} <= {r for _, r in res1["ptrs"]}      # the buffers of level 1, not new ones
        assert all(u >= 1 for u in res2["unpacked"])
        _after_commit(res2, cases2, ids2, rows1, stores)
        touched = {s for pr in ids2 for sd in pr for s in sd}
        for q, st in enumerate(stores):
            assert res2["rows"][q] == res2["rows"][0]
            for sid in set(range(len(seqs))) - touched:
                assert res2["rows"][q][sid] == rows1[sid], f"rank {q}: row {sid} of a node outside level 2 changed"
            for k, (a, b) in enumerate(EC.second_level_pairs(lv)):
                assert np.array_equal(_bits(st.cache(2 * a)), _bits(res2["exps"][k]["merged"])), f"rank {q}: merged profile of level-2 pair {k}"
    finally:
        for st in stores:
            st.close()


def test_dp_row_one_code_short_of_its_pitch(gpu):
    """A where == 1 path of 2 * seq_len - 1 codes, the longest a DP path can be (one match, gaps otherwise; gaps cost less than mismatches in
    this level): packed from a DP output row that is full but for one code, alone in its rank's block, unpacked and committed by the other."""
    from twilight_amd import level as L

    lv = EC.gap_only_level()
    own = lv.ownerships[0]
    seqs, pairs, ids = _level(lv.cases)
    stores = [L.Store(seqs, "n") for _ in range(own.world)]
    try:
        res = _exchange_level(gpu, stores, "n", lv.cases, pairs, own.owner, lv.takes_part, thr=lv.thr, gaps=EC.GAP_ONLY)
        assert [res["final"][i] for i in range(3)] == [x.final_len for x in lv.pairs] and set(res["where"].values()) == {1}
        assert res["final"][1] == 2 * stores[0]._seq_len - 1 == res["stride"] and Counter(res["exps"][1]["path_full"].tolist())[0] == 1
        _after_commit(res, lv.cases, ids, seqs, stores)
        assert res["rows"][0] == res["rows"][1] and res["unpacked"] == [1, 2]
    finally:
        for st in stores:
            st.close()


def test_protein_ranks_exchange_a_level(gpu):
    from twilight_amd import level as L

    lv = EC.main_level("p", small=True)
    own = lv.ownerships[0]
    seqs, pairs, ids = _level(lv.cases, store_all=True)
    specs = [LC.EdgeSpec(x.name, x.case, frozenset({"hand_back"}), hand_back=True) if x.hand_back else None for x in lv.pairs]
    ref = {}
    _restore_level(gpu, "p", lv.cases, specs, thr=lv.thr, select=lambda i: lv.pairs[i].where != 0, store_all=True, keep=ref)
    stores = [L.Store(seqs, "p") for _ in range(own.world)]
    try:
        res = _exchange_level(gpu, stores, "p", lv.cases, pairs, own.owner, lv.takes_part, thr=lv.thr, hand_back={i for i, x in enumerate(lv.pairs) if x.hand_back})
        for i, x in enumerate(lv.pairs):
            assert (res["where"].get(i, 0), res["final"].get(i, 0)) == (x.where, ref["plen"][i]) and (x.final_len is None or res["final"][i] == x.final_len), x.name
        _after_commit(res, lv.cases, ids, seqs, stores)
        assert all(c[1] >= 2 and c[2] >= 2 for c in res["sent"]) and all(u >= 1 for u in res["unpacked"])
        for q, st in enumerate(stores):
            assert res["rows"][q] == ref["rows"]
            for i, x in enumerate(lv.pairs):
                if x.where:
                    assert np.array_equal(_bits(st.cache(2 * i)), _bits(ref["caches"][i])), f"rank {q} pair {i}: merged profile"
    finally:
        for st in stores:
            st.close()


def test_refused_calls_change_nothing(gpu):
    """Everything the two block calls refuse on the host, each followed by a look at the block, the receive buffer and every row of the
    path buffer; then a good call, an unpack of the same block and the commit.  Only arguments the library judges before a launch are
    sent: tables, pair numbers, lengths, kinds, and offsets into the level's OWN exchange buffers (whose end the library knows)."""
    from twilight_amd import api, level as L

    lv = EC.main_level("n", small=True)
    cases, n = lv.cases, len(lv.pairs)
    seqs, pairs, ids = _level(cases)
    p = gpu.make_params(LC.matrix_of("n"))
    st = L.Store(seqs, "n")
    try:
        lens, _ = st.prepare(p, pairs, gappy_threshold=lv.thr)
        part = [i for i in range(n) if lv.takes_part[i]]
        dl, err = st.align_in_hbm(p, run_mask=np.array(lv.takes_part, dtype=np.uint8))
        assert not err.any()
        exps = {i: LC.expected(cases[i], path_wo_gc=st.read_path(i, int(dl[i]))) for i in part}
        final = {i: len(exps[i]["path_full"]) for i in part}
        where = {i: lv.pairs[i].where for i in part}
        stride, sl2 = max(final.values()), 2 * st._seq_len
        pl = EC.plan([0] * n, lv.takes_part, [len(c.sides[0].rows[0]) + len(c.sides[1].rows[0]) for c in cases], 1)
        send, recv = st.exchange_buffers(pl.block_max, pl.block_max)
        api.copy_to_device(send, SENT * pl.block_max)
        api.copy_to_device(recv, SENT * pl.block_max)
        for call in (lambda: st.paths_to_block([part[0]], [1], [1], send, [64]), lambda: st.paths_from_block([part[0]], [1], recv, [64])):
            with pytest.raises(api.TwlError, match="twl_level_restore first"):      # before twl_level_restore
                call()
        lost = [i for i in part if where[i] == 2]
        fin = st.restore(p, lost, stride)
        for t, i in enumerate(lost):
            if lv.pairs[i].hand_back:
                assert fin[t] == -1
                st.write_final(i, exps[i]["path_full"])
        k1 = [i for i in part if where[i] == 1]

        def state():
            return api.copy_from_device(send, pl.block_max), api.copy_from_device(recv, pl.block_max), [st.read_final(i, stride).tobytes() for i in range(n)]

        s0 = state()
        assert s0[0] == s0[1] == SENT * pl.block_max
        refused = {
            "pair n to a block": lambda: st.paths_to_block([lost[0], n], [1, 1], [2, 2], send, [64, 72]),
            "pair -1 to a block": lambda: st.paths_to_block([-1], [1], [1], send, [64]),
            "pair n from a block": lambda: st.paths_from_block([n], [1], recv, [64]),
            "one code more than a DP row": lambda: st.paths_to_block([k1[0]], [sl2 + 1], [1], send, [64]),
            "one code more than a path row": lambda: st.paths_to_block([lost[0]], [stride + 1], [2], send, [64]),
            "one code more into a path row": lambda: st.paths_from_block([lost[0]], [stride + 1], recv, [64]),
            "bad path row behind good DP rows": lambda: st.paths_to_block([k1[0], k1[1], lost[0]], [final[k1[0]], final[k1[1]], stride + 1], [1, 1, 2], send, [64, 512, 1024]),
            "kind 3": lambda: st.paths_to_block([k1[0]], [1], [3], send, [64]),
            "null tables to a block": lambda: st.paths_to_block(None, None, None, send, None, n_sel=2),
            "null tables from a block": lambda: st.paths_from_block(None, None, recv, None, n_sel=2),
            "null block": lambda: st.paths_to_block([k1[0]], [1], [1], 0, [64]),
            "row behind the send buffer": lambda: st.paths_to_block([k1[0]], [1], [1], send, [1 << 40]),
            "row in front of the send buffer": lambda: st.paths_to_block([k1[0]], [1], [1], send, [-8]),
            "row behind the receive buffer": lambda: st.paths_from_block([lost[0]], [1], recv, [1 << 40]),
            "row in front of the receive buffer": lambda: st.paths_from_block([lost[0]], [1], recv + 64, [-128]),
        }
        for name, call in refused.items():
            with pytest.raises(api.TwlError, match="bad (row selection|argument)"):
                call()
            assert state() == s0, f"{name}: refused, but something changed"
        st.paths_to_block([], [], [], send, [])               # n_sel == 0 is accepted, with and without tables
        st.paths_to_block(None, None, None, send, None, n_sel=0)
        st.paths_from_block(None, None, recv, None, n_sel=0)
        assert state() == s0
        # a good call after all that: pack every pair, hand the block to the receive buffer, unpack it into rows full of the sentinel
        lens_r = [final[i] for i in part]
        off, _ = EC.row_offsets(pl, 0, lens_r)
        api.copy_to_device(send, EC.header_bytes(pl, 0, _words(0, 1), lens_r, [0] * len(part)))
        st.paths_to_block(part, lens_r, [where[i] for i in part], send, off)
        blk = api.copy_from_device(send, pl.block_max)
        assert blk == EC.block_bytes(pl, 0, _words(0, 1), lens_r, [0] * len(part), [exps[i]["path_full"] for i in part])
        api.copy_to_device(recv, blk)
        for i in part:
            st.write_final(i, _sentinel_row(stride))
        st.paths_from_block(part, lens_r, recv, off)
        for i in part:
            assert st.read_final(i, stride).tobytes() == exps[i]["path_full"].tobytes() + SENT * (stride - final[i]), f"pair {i}"
        st.commit_from_dp([None] * n, [final.get(i, 0) for i in range(n)], stride=stride, restored=part)
        rows = st.rows()
        for i in range(n):
            flat = ids[i][0] + ids[i][1]
            for sid, w in zip(flat, exps[i]["rows_after"] if i in exps else [seqs[s] for s in flat]):
                assert rows[sid] == w, f"pair {i}: row {sid}"
    finally:
        st.close()
