"""Inputs for the tile-parallel kernels, each listed with the branch it is for.  tests/test_mt_edge_inputs_cpu.py proves every claim with the oracle and the
restatements of tests/mt_oracle.py alone (no GPU); tests/test_gpu_mt_edges.py runs them on the device and reads the level's tables back.

Every case is a small synth.LevelBatch, the alignment parameters and the knobs of the run.  TWL_KNOB_MT_MIN_MARKER is 64 everywhere, the marker 128 or 250, a
level has 1 to 6 pairs of 600 to 2500 columns (the one case that needs many slots apart), and every level meets the policy's own condition for the path.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from twilight_amd import api, synth

M = synth.nucleotide_matrix()
PM = synth.protein_matrix()
BASE_KNOBS = {api.KNOB_MT_MIN_MARKER: 64}


@dataclasses.dataclass
class Case:
    name: str
    branch: str                 # what the case is for (the CPU file proves it)
    batch: synth.LevelBatch
    pk: dict                    # alignment parameters (marker, xdrop, flen)
    knobs: dict                 # twl_set_knob values on top of BASE_KNOBS
    matrix: np.ndarray = None
    notes: dict = dataclasses.field(default_factory=dict)      # what the builder engineered: {(pair, slot): class}

    @property
    def marker(self):
        return self.pk["marker"]

    def knob(self, key, default=None):
        return self.knobs.get(key, default)


def _with_len(b, ln):
    return synth.LevelBatch(P=b.P, seq_len=b.seq_len, freq=b.freq, gap_open=b.gap_open, gap_extend=b.gap_extend, len=np.asarray(ln, dtype=np.int32), num=b.num)


def _take(b, idx):
    idx = np.asarray(idx)
    return synth.LevelBatch(P=b.P, seq_len=b.seq_len, freq=b.freq[idx].copy(), gap_open=b.gap_open[idx].copy(), gap_extend=b.gap_extend[idx].copy(),
                            len=b.len[idx].copy(), num=b.num[idx].copy())


# ---- boundary arithmetic ----
def boundary_case():
    """One pair three times, truncated so that R + Q - 2 is one below, on and one above (marker - 1) * 10 - 1 = 1269: T is 10, 11, 11."""
    b = _take(synth.make_level_batch(1, 700, members=((1, 5), (1, 5)), seed=201), [0, 0, 0])
    edge = (128 - 1) * 10 - 1
    ln = [[636, edge + 2 - 1 - 636], [636, edge + 2 - 636], [636, edge + 2 + 1 - 636]]
    assert all(x[1] <= b.len[0, 1] for x in ln) and b.len[0, 0] >= 636
    return Case("boundary", "R + Q - 2 one below / on / one above a boundary's first anti-diagonal: T switches between s and s + 1", _with_len(b, ln), dict(marker=128), {})


# ---- stepped-over and landed boundaries ----
def stepped_case():
    b = synth.make_level_batch(2, 1500, members=((1, 6), (1, 6)), seed=5, indel=0.01)
    return Case("stepped", "true starts advance by marker - 1 at some boundaries (the path steps over the marker diagonal) and by marker at others", b, dict(marker=128), {})


# ---- tails and ends ----
def tails_case():
    b = synth.make_level_batch(3, 1500, members=((1, 4), (1, 4)), seed=203)
    ln = b.len.copy()
    ln[0, 0] = int(ln[0, 0] * 0.4)       # the reference ends first: the last record carries a run of 1 (query columns)
    ln[1, 1] = int(ln[1, 1] * 0.4)       # the query ends first: a run of 2
    return Case("tails", "the last record of a pair carries tailDir 1, tailDir 2, no tail", _with_len(b, ln), dict(marker=128), {})


# ---- degenerate pairs beside long ones ----
def degenerate_case():
    b = synth.make_level_batch(6, 1500, members=((1, 4), (1, 4)), seed=204)
    ln = b.len.copy()
    ln[1, 0] = 1          # R = 1
    ln[2, 1] = 1          # Q = 1
    ln[3, 0] = 0          # R = 0: the pair does not run
    ln[4] = (50, 60)      # R + Q < marker: one tile, no scout
    return Case("degenerate", "R = 1, Q = 1, R = 0 and R + Q < marker beside long pairs in one level", _with_len(b, ln), dict(marker=128), {})


# ---- scout start clamps ----
def clamps_case():
    """Slots whose scout would start before anti-diagonal 0; a pair with R >= 8 Q and its mirror -- and, with the shortest lead (16), the mirror's last boundary on
    the pair's last anti-diagonal, where the straight line's reference row reaches R and is clamped (mt_oracle.line_cell says when that can happen)."""
    b = synth.make_level_batch(3, 2500, members=((1, 4), (1, 4)), seed=205, length_jitter=0.0)
    ln = b.len.copy()
    total = (128 - 1) * 20 + 1           # boundary 20 reports from the last anti-diagonal: 127 * 20 - 1 = R + Q - 2
    ln[0] = (total - 100, 100)
    ln[1] = (100, total - 100)
    assert ln[0, 0] <= b.len[0, 0] and ln[1, 1] <= b.len[1, 1]
    return Case("clamps", "scout start clamped to anti-diagonal 0; the line cell's clamps on R >= 8 Q and its mirror", _with_len(b, ln), dict(marker=128),
                {api.KNOB_MT_LEAD2: 16, api.KNOB_MT_LEAD: 16})


# ---- scout marker clamp, overlapping report ranges ----
def long_case():
    b = synth.make_level_batch(1, 8200, members=((1, 4), (1, 4)), seed=206)
    return Case("long", "scouts whose own marker is clamped to kMaxMarker; report ranges of neighbouring scouts overlap in mt_spath (slots >= marker - 3)", b,
                dict(marker=128), {api.KNOB_MT_ANCHOR: 0, api.KNOB_MT_LEAD: 900, api.KNOB_MT_MARGIN: 64})


# ---- anchor classes ----
def _gap_out(b, pair, side, lo, hi):
    lo, hi = max(lo, 0), min(hi, int(b.len[pair, side]))
    if hi > lo:
        b.freq[pair, side, lo:hi, :] = 0.0
        b.freq[pair, side, lo:hi, b.P - 1] = float(b.num[pair, side])


def _put(b, pair, side, lo, letters):
    for i, c in enumerate(letters):
        if 0 <= lo + i < int(b.len[pair, side]):
            b.freq[pair, side, lo + i, :] = 0.0
            b.freq[pair, side, lo + i, int(c)] = float(b.num[pair, side])


def _line(d0, R, Q):
    q = (d0 * Q) // (R + Q)
    return d0 - q, q


def anchor_case(name, members, gap_col_rate, seed, P=6, length=1500, marker=128):
    """Boundaries engineered around the straight line's cell (r0, q0) of the anchor kernel (lead2 128: anti-diagonal (marker - 1) * slot - 1 - 128):
      "w1".."w8"  aimed at window 1..8 (shift +24, -24, ... -96): the reference columns of the windows tried before it are gap-dominated, the window
                  itself keeps 44 of its 64 columns.  Substitutions and the drawn gap columns move some of them a window or two on; what counts is
                  that the level as a whole reaches all nine, which the CPU file asserts from the restated table
      "few"       every window gap-dominated: rejected for fewer than 36 matches
      "close"     a tandem repeat of period 4 on both sides, longer than window plus offsets: every fourth offset matches all 64 columns, the runner-up ties
      "tie"       both sides doubled letters, the query with one column inserted in the middle of the window: offsets 0 and 1 match 48 columns each, 0 wins
      "tie_neg"   offsets -1 and +1 match 48 columns each, offset 0 none: the negative one wins
    Everything else is left as drawn (window 0 decides, or not)."""
    b = synth.make_level_batch(4, length, P=P, members=members, seed=seed, sub=0.02, indel=0.002, gap_col_rate=gap_col_rate)
    lead2 = 128
    nL = P - 2
    notes = {}
    shifts = (0, 24, -24, 48, -48, 72, -72, 96, -96)
    plan_ = {0: {5: "w1", 11: "w2", 17: "w3"}, 1: {5: "w4", 11: "w5", 17: "w6"}, 2: {5: "w7", 11: "w8", 16: "close"}, 3: {5: "few", 11: "tie", 17: "tie_neg", -1: "few"}}
    rng = np.random.default_rng(seed + 1)
    for pair, slots in plan_.items():
        R, Q = int(b.len[pair, 0]), int(b.len[pair, 1])
        last = (R + Q - 1) // (marker - 1)            # the last boundary of the pair
        while (marker - 1) * last - 1 > R + Q - 2:
            last -= 1
        for slot, cls in slots.items():
            slot = last if slot < 0 else slot
            r0, q0 = _line(max((marker - 1) * slot - 1 - lead2, 0), R, Q)
            if cls.startswith("w"):
                S = shifts[int(cls[1:])]
                if S > 0:
                    _gap_out(b, pair, 0, r0 - 130, r0 + S - 12)
                else:
                    _gap_out(b, pair, 0, r0 + S + 12, r0 + 130)
            elif cls == "few":
                _gap_out(b, pair, 0, r0 - 130, r0 + 130)
            elif cls == "close":
                _put(b, pair, 0, r0 - 200, [(r0 - 200 + i) % 4 for i in range(400)])
                _put(b, pair, 1, q0 - 400, [(q0 - 400 + i) % 4 for i in range(800)])
            elif cls == "tie":
                c = [int(rng.integers(0, nL))]
                while len(c) < 40:
                    x = int(rng.integers(0, nL))
                    if x != c[-1]:
                        c.append(x)
                a = [c[i // 2] for i in range(64)]                    # doubled letters: a[i] == a[i + 1] for even i
                _put(b, pair, 0, r0 - 32, a)
                ins = (a[31] + 1) % nL if (a[31] + 1) % nL != a[32] else (a[31] + 2) % nL
                _put(b, pair, 1, q0 - 32, a[:32] + [ins] + a[32:])
            elif cls == "tie_neg":
                # blocks x y x y of two letters, the next block of the other two: a[i] == a[i + 2] inside a block, a[i] != a[i + 1] everywhere.  The query holds the
                # first half of the window one column to the left and the second half one to the right: offsets -1 and +1 match 32 + 16 columns each, offset 0 none
                a = []
                for k in range(16):
                    x, y = ((0, 1), (2, 3))[k % 2][:: 1 if rng.random() < 0.5 else -1]
                    a += [x, y, x, y]
                _put(b, pair, 0, r0 - 32, a)
                _put(b, pair, 1, q0 - 33, a[:32] + [a[31], a[30]] + a[32:])      # (the two fillers match neither neighbour at either offset)
            notes[(pair, slot)] = cls
    return Case(name, "anchor classes: the nine windows, both rejections, a tie the order decides, windows past the ends, the early outs", b, dict(marker=marker, xdrop=1500), {}, notes=notes)      # (X-drop 1500: gap-dominated stretches widen the band; it has to fit the 768-row window of the throughput geometry)


def anchors_leaf_case():
    return anchor_case("anchors_leaf", (1, 1), 0.0, 207)


def anchors_profile_case():
    return anchor_case("anchors_profile", ((2, 6), (2, 6)), 0.2, 208)


# ---- protein ----
def protein_case():
    b = synth.make_level_batch(4, 1500, P=22, members=((1, 6), (1, 6)), seed=209, sub=0.15)
    return Case("protein", "P = 22: twenty letters in the anchor kernel, records on the precomputed-score path", b, dict(marker=250, xdrop=2500), {}, matrix=PM)      # (X-drop 2500: bands of ~270 rows fit the 512-row window of the protein throughput geometry)


# ---- errors ----
def err1_case():
    """250 columns of A against 250 columns of C in the middle of one pair: no offset matches, every cell of tile 10 falls more than the X-drop below the tile's
    best score and the band empties.  The pairs beside it end well."""
    b = synth.make_level_batch(3, 1500, members=(1, 1), seed=210)
    for side, letter in ((0, 0), (1, 1)):
        b.freq[1, side, 700:950, :] = 0.0
        b.freq[1, side, 700:950, letter] = 1.0
    return Case("err1", "a tile fails from its true start with errorType 1 (a small X-drop empties the band)", b, dict(marker=128, xdrop=300), {})


def err2_case():
    """fLen 128 with an X-drop under which the band reaches 129 rows in tile 7 of one pair, tile 5 of another and tile 0 of the third."""
    b = synth.make_level_batch(3, 1500, members=(1, 1), seed=9)
    return Case("err2", "a tile fails from its true start with errorType 2 (band wider than fLen 128)", b, dict(marker=128, flen=128, xdrop=1400), {})


BUILDERS = (boundary_case, stepped_case, tails_case, degenerate_case, clamps_case, long_case, anchors_leaf_case, anchors_profile_case, protein_case, err1_case, err2_case)
NAMES = tuple(f.__name__[: -len("_case")] for f in BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name) -> Case:
    c = BUILDERS[NAMES.index(name)]()
    if c.matrix is None:
        c.matrix = M
    c.knobs = {**BASE_KNOBS, **c.knobs}
    return c
