"""Restatements of the host plan and of the two small kernels of a tile-parallel level, in numpy.  Test infrastructure only.

Written from DESIGN.md section 3.3 and the comments of twilight_amd/csrc/talco_mt.hip.h (the block "tile-parallel alignment", "anchored scouts") and of
twl_policy.inc.hip (plan_tile_level), one definition at a time; the DP itself is not restated here -- tiles come from the oracle (oracle_lib.tile_from).

  launch_order   the pairs that run, longest first
  plan           slots, tiles per pair, the scout and tile job lists, the dims twl_mt_tables reports
  true_starts    the start cell of every tile of a pair, from the oracle's exit hook
  anchor_table   mt_anchor_kernel: 128 + the trusted offset of q - r at every tile boundary, or -1 -- with what decided each entry
  chain          mt_chain_kernel: predicted starts from a row of scout path samples
"""
from __future__ import annotations

import numpy as np

import oracle_lib as O

K_MAX_MARKER = 1024          # TWL_MAX_MARKER: a scout's own marker is clamped to it
REC_WORDS = 12               # TWL_MT_REC_WORDS
ANCHOR_HALF, ANCHOR_OFFSETS = 32, 256            # 64 columns, offsets -128 .. 127
ANCHOR_SHIFTS = (0, 24, -24, 48, -48, 72, -72, 96, -96)      # the nine windows, in the order they are tried
ANCHOR_MIN_MATCHES, ANCHOR_MIN_GAP = 36, 8


def launch_order(lens):
    """Pairs with both sides non-empty, longest (R + Q) first, ties in pair order (run_device, step 1)."""
    lens = np.asarray(lens)
    live = [int(i) for i in range(lens.shape[0]) if lens[i, 0] > 0 and lens[i, 1] > 0]
    return sorted(live, key=lambda i: -(int(lens[i, 0]) + int(lens[i, 1])))      # (sorted is stable)


def tiles_of(R, Q, slots, marker):
    """Tiles of a pair as the plan counts them: tile 0, and one for every boundary s in [1, slots) whose first reported anti-diagonal
    (marker - 1) * s - 1 still lies in the pair (<= R + Q - 2)."""
    return 1 + sum(1 for s in range(1, slots) if (marker - 1) * s - 1 <= R + Q - 2)


def plan(lens, order, seq_len, marker, *, rounds=2, thr_jobs=256, anchor=1, lead2=None, marg=None):
    """The plan of a tile-parallel level on the narrow geometries (not the wide re-run, not the 512-row tiles).  lead2 / marg None: the defaults, which
    depend on the level (128 / 64 on levels of at most 2048 tile jobs, 96 / 40 beyond); a knob value sets both kinds of level."""
    lens = np.asarray(lens)
    slots = (2 * seq_len) // (marker - 1) + 2
    T = [tiles_of(int(lens[p, 0]), int(lens[p, 1]), slots, marker) for p in order]
    maxT = max(T) if T else 0
    scouts = [(int(order[row]), s, row) for s in range(1, maxT) for row in range(len(order)) if s < T[row]]
    tiles = [(int(order[row]), s, row) for s in range(0, maxT) for row in range(len(order)) if s < T[row]]
    long_scouts = len(tiles) <= 2048
    dims = dict(n_run=len(order), slots=slots, sp_pitch=2 * seq_len + 8, segcap=2 * marker + 16, n_scout=len(scouts), n_tile=len(tiles),
                rounds=max(1, min(int(rounds), 7)), lead2=(128 if long_scouts else 96) if lead2 is None else max(16, int(lead2)),
                marg=(64 if long_scouts else 40) if marg is None else max(2, int(marg)), anchors=1 if (anchor and scouts) else 0,
                thr=1 if len(tiles) > thr_jobs else 0, small_tiles=0, marker=marker)
    return dict(dims=dims, order=[int(p) for p in order], T=T, scouts=scouts, tiles=tiles)


def takes_the_path(lens, order, marker, cus=256):
    """The policy's own condition for the tile-parallel path on a level of few pairs: sumLen >= 3 * marker * n_run and 2 * n_run <= CUs."""
    lens = np.asarray(lens)
    s = sum(int(lens[p, 0]) + int(lens[p, 1]) for p in order)
    return len(order) > 0 and s >= 3 * marker * len(order) and 2 * len(order) <= cus


def true_starts(params, pv):
    """(starts, tiles, errorType, band cells, path): starts[t] is the cell tile t of the pair starts from -- (0, 0), then where every tile's exit left the pair
    (the oracle's exit hook).  A tile that fails has a start (the exit of the one before) and no exit: len(starts) == tiles either way."""
    aln, err, st, rows = O.pair_exits(params, pv)
    starts = [(0, 0)] + [(r, q) for (_t, _kind, _state, r, q) in rows]
    return starts[: st.tiles], int(st.tiles), int(err), int(st.cells), aln


# ---- anchors ----
def consensus(freq_side, n, side, P):
    """Consensus letter of columns 0 .. n-1 of one side: the most frequent of the first P - 2 letters (the first of equals) when its count is positive and at
    least the gap letter's (entry P - 1); else 100 + side, which equals nothing -- not even the same verdict on the other side."""
    f = np.asarray(freq_side[:n], dtype=np.float32)
    if n <= 0:
        return np.zeros(0, dtype=np.int16)
    best = np.argmax(f[:, : P - 2], axis=1)
    bc = f[np.arange(n), best]
    ok = (bc > np.float32(0.0)) & (bc >= f[:, P - 1])
    return np.where(ok, best, 100 + side).astype(np.int16)


def line_cell(d0, R, Q):
    """The cell of anti-diagonal d0 on the straight line between the corners, with its two clamps: (r, q, clamp_q, clamp_r) or None when no cell of the pair
    lies there.  For 0 <= d0 <= R + Q - 2 the first clamp cannot fire: floor(d0 * Q / (R + Q)) <= floor(Q - 2Q / (R + Q)) <= Q - 1; the second one fires only
    where Q > R and d0 > R + Q - 2 - Q / R (r = ceil(d0 * R / (R + Q)) reaches R)."""
    q = (d0 * Q) // (R + Q)
    clamp_q = q > Q - 1
    q = min(q, Q - 1)
    r = d0 - q
    clamp_r = r > R - 1
    if clamp_r:
        r = R - 1
        q = d0 - r
    if q > Q - 1 or r < 0:
        return None
    return r, q, clamp_q, clamp_r


def _rank(o):
    """Place of offset o in the order 0, -1, 1, -2, 2, ... in which ties are decided."""
    return 0 if o == 0 else (-2 * o - 1 if o < 0 else 2 * o)


def anchor_boundary(cr, cq, R, Q, marker, slot, lead2):
    """One entry of the table with what decided it: dict(value, window, why, tie, left) --
    value 128 + offset or -1; window 0..8 the window that was trusted (-1 none); why "early" (R < 2, Q < 2, boundary beyond the pair, no line cell), "trusted",
    "few" (the last window's best count below 36) or "close" (... its runner-up within 8); tie: the trusted window's best count is shared by another offset within
    2 of it (the tie order decided), tied: those offsets; left: set of "r-", "r+", "q-", "q+" -- a window that was examined reached past that end of that side;
    clamps: which clamps of the line cell fired."""
    sp_lo = (marker - 1) * slot - 1
    d0 = max(sp_lo - lead2, 0)
    out = dict(value=-1, window=-1, why="early", tie=False, tied=[], left=set(), clamps=(False, False), d0=d0, clamped_d0=sp_lo - lead2 < 0)
    if sp_lo > R + Q - 2 or R < 2 or Q < 2:
        return out
    cell = line_cell(d0, R, Q)
    if cell is None:
        return out
    r0, q0, cq_, cr_ = cell
    out["clamps"] = (cq_, cr_)
    offs = np.arange(-ANCHOR_OFFSETS // 2, ANCHOR_OFFSETS // 2)
    ranks = np.array([_rank(int(o)) for o in offs])
    for w, shift in enumerate(ANCHOR_SHIFTS):
        ri = r0 - ANCHOR_HALF + shift + np.arange(2 * ANCHOR_HALF)                    # the 64 reference columns
        qi = (q0 - ANCHOR_HALF + shift + np.arange(2 * ANCHOR_HALF))[:, None] + offs[None, :]      # the query column of each at every offset
        if ri[0] < 0: out["left"].add("r-")
        if ri[-1] >= R: out["left"].add("r+")
        if qi.min() < 0: out["left"].add("q-")
        if qi.max() >= Q: out["left"].add("q+")
        lr = np.where((ri >= 0) & (ri < R), cr[np.clip(ri, 0, R - 1)], 100)
        lq = np.where((qi >= 0) & (qi < Q), cq[np.clip(qi, 0, Q - 1)], 101)
        cnt = (lr[:, None] == lq).sum(axis=0)
        bc = int(cnt.max())
        bo = int(offs[np.flatnonzero(cnt == bc)[np.argmin(ranks[cnt == bc])]])
        far = np.abs(offs - bo) > 2
        second = int(cnt[far].max())
        if bc >= ANCHOR_MIN_MATCHES and bc - second >= ANCHOR_MIN_GAP:
            near = (~far) & (offs != bo)
            out.update(value=128 + bo, window=w, why="trusted", tie=bool(np.any(cnt[near] == bc)), tied=[int(o) for o in offs[near & (cnt == bc)]])
            return out
        out["why"] = "few" if bc < ANCHOR_MIN_MATCHES else "close"
    return out


def anchor_table(batch, pl, marker, lead2, detail=False):
    """anchor[n_run][slots] of a level (int32, -1 where nothing is trusted or no scout exists); detail=True: also {(row, slot): anchor_boundary(...)}."""
    d = pl["dims"]
    table = np.full((d["n_run"], d["slots"]), -1, dtype=np.int32)
    info = {}
    cons = {}
    for pair, slot, row in pl["scouts"]:
        R, Q = int(batch.len[pair, 0]), int(batch.len[pair, 1])
        if pair not in cons:
            cons[pair] = (consensus(batch.freq[pair, 0], R, 0, batch.P), consensus(batch.freq[pair, 1], Q, 1, batch.P))
        b = anchor_boundary(cons[pair][0], cons[pair][1], R, Q, marker, slot, lead2)
        table[row, slot] = b["value"]
        info[(row, slot)] = b
    return (table, info) if detail else table


# ---- chain ----
def chain(spath_row, R, Q, slots, marker, perturb=0, front=None, prev=None):
    """Predicted starts [slots][2] of one pair from its row of scout path samples (sp[d] = query row of the path on anti-diagonal d, -1 = the path steps over
    d, below -1 = nobody knows).  From (0, 0), or -- front = a row of the stitch front in state 1 -- from the true cell the stitch stopped at; a front in state 2
    leaves the row as it was (prev).  A tile that starts on anti-diagonal s hands over on s + marker, or on s + marker - 1 when the path steps over that one;
    the walk ends at a missing sample, beyond anti-diagonal R + Q - 2 or at a cell outside the pair, and every slot behind it is unknown (-1)."""
    sp = np.asarray(spath_row)
    ch = np.full((slots, 2), -1, dtype=np.int32) if prev is None else np.array(prev, dtype=np.int32).copy()
    if front is not None and int(front[0]) == 2:
        return ch
    if front is not None and int(front[0]) == 1:
        t = int(front[1])
        if t >= slots:
            return ch
        ch[t] = (int(front[2]), int(front[3]))
        s = int(front[2]) + int(front[3])
    else:
        t = 0
        ch[0] = (0, 0)
        s = 0
    ch[t + 1:] = -1
    for t in range(t + 1, slots):
        d = s + marker
        if d > R + Q - 2:
            break
        if sp[d] >= 0:
            s, q = d, int(sp[d])
        elif sp[d] == -1 and d - 1 > s and sp[d - 1] >= 0:
            s, q = d - 1, int(sp[d - 1])
        else:
            break
        r = s - q
        if perturb > 0 and t % perturb == 0:      # the test aid: every perturb-th prediction moved by one cell along its anti-diagonal
            if q > 0 and r + 1 < R:
                r, q = r + 1, q - 1
            elif r > 0 and q + 1 < Q:
                r, q = r - 1, q + 1
        if r < 0 or r >= R or q >= Q:
            break
        ch[t] = (r, q)
    return ch


# ---- the checks of the tables read back from a level (tests/test_gpu_mt_edges.py, tools/fuzz_mt.py) ----
class Tiles:
    """oracle_lib.tile_from over the pairs of one batch with one set of parameters, remembered by (pair, start, first): most starts repeat from run to run."""

    def __init__(self, params, batch):
        self.params, self.batch, self.views, self.memo = params, batch, {}, {}

    def view(self, pair):
        if pair not in self.views:
            self.views[pair] = O.PairView(self.batch, pair)
        return self.views[pair]

    def __call__(self, pair, start, first):
        key = (pair, int(start[0]), int(start[1]), bool(first))
        if key not in self.memo:
            self.memo[key] = O.tile_from(self.params, self.view(pair), start, first)
        return self.memo[key]


def check_chain(tables, lens, marker, perturb):
    """(d): after ONE round the chain table is `chain` of the scout path samples read back from the device, in every slot of every row."""
    d = tables["dims"]
    assert d["rounds"] == 1, "the chain of a later round starts from a front the last stitch launch has overwritten"
    for row, pair in enumerate(tables["order"]):
        R, Q = int(lens[pair, 0]), int(lens[pair, 1])
        want = chain(tables["spath"][row], R, Q, d["slots"], marker, perturb)
        got = tables["chain"][row]
        bad = np.flatnonzero(np.any(want != got, axis=1))
        assert bad.size == 0, f"row {row} (pair {pair}): chain differs in slots {bad.tolist()[:8]}: device {got[bad[:4]].tolist()} restated {want[bad[:4]].tolist()}"


def check_records(tables, tiles: Tiles):
    """(e): every record is the tile function of the start it names.  Returns (records in state 1, in state 2 with an errorType, in state 2 with an internal
    re-run code -- the only ones that are not compared)."""
    d = tables["dims"]
    ok = failed = internal = 0
    for row, pair in enumerate(tables["order"]):
        pair = int(pair)
        pv = tiles.view(pair)
        for slot in range(d["slots"]):
            rc = tables["rec"][row, slot]
            tag = f"row {row} (pair {pair}) slot {slot} record {rc.tolist()}"
            if rc[0] == 0:
                continue
            assert rc[0] in (1, 2), tag
            start = (int(rc[1]), int(rc[2]))
            assert 0 <= start[0] < pv.R and 0 <= start[1] < pv.Q, f"{tag}: start outside the pair"
            assert slot > 0 or start == (0, 0), f"{tag}: tile 0 starts at the corner"
            if rc[0] == 2 and not 1 <= rc[10] <= 3:
                internal += 1
                continue
            nxt, last, err, cells, seg = tiles(pair, start, slot == 0)
            if rc[0] == 2:
                assert err == rc[10], f"{tag}: the oracle's tile from {start} ends with errorType {err}"
                assert cells == int(np.uint32(rc[9])), f"{tag}: band cells of the failed tile, oracle {cells}"
                failed += 1
                continue
            assert err == 0, f"{tag}: the oracle's tile from {start} fails with errorType {err}"
            assert nxt == (int(rc[3]), int(rc[4])), f"{tag}: next start, oracle {nxt}"
            assert bool(rc[5]) == last, f"{tag}: last flag, oracle {last}"
            assert cells == int(np.uint32(rc[9])), f"{tag}: band cells, oracle {cells}"
            cnt, tail_dir, tail_len = int(rc[6]), int(rc[7]), int(rc[8])
            assert 0 <= cnt <= d["segcap"] and tail_len >= 0, tag
            got = np.concatenate([tables["seg"][row, slot, :cnt], np.full(tail_len, tail_dir, dtype=np.int8)])
            assert got.shape == seg.shape and np.array_equal(got, seg), f"{tag}: forward segment differs (device {got.shape[0]} bytes, oracle {seg.shape[0]})"
            ok += 1
    return ok, failed, internal
