"""Directed cases for the tile exit and the traceback walk of the DP kernels (talco_nuc.hip.h, talco_kernel.hip.h, talco_global.hip.h).

The reference's tile exit (TALCO-XDrop.cpp:615-682) and the steps of its traceback (:134-231) are written once (talco_exit.hip.h: tile_exit, pair_advance,
walk_step, the guarded append, the border fill, the segment copy; tests/test_exit_fn_cpu.py holds them on the CPU) for talco_kernel.hip.h and talco_global.hip.h,
which keep how they fetch CS[last_k][0] and a pointer nibble and their walk loops; talco_nuc.hip.h restates the same lines.  The oracle's exit hook
(oracle/talco_oracle.h, twlo_exit_fn) says, per tile that reaches its traceback, which exit it took: kind 0 converged, 1 the pair ended
before the marker, 2 it ended at or behind the marker unconverged; the state the walk starts in (0 S, 1 I, 2 D, 3 the S cell one diagonal
in front of the marker), the diagonal the tile stopped on and where the pair stands behind it.  `records` turns those and the final path
into one TileExit per tile: its segment of the path, the trailing run behind the last tile, the longest runs of each code inside the
walked segment and, for tile 0, the codes the border fill added.  `tags_of` is the predicate of every class, written out: a case carries
the tags its pairs have, tests/test_exit_edge_inputs_cpu.py recomputes records and tags on the oracle and holds them to the constants
below, and REQUIRED is what the cases must reach between them.  tests/test_gpu_exit_edges.py sends every pool down every route.

A case is generator arguments (synth.make_level_batch), the pairs kept, per pair an optional trim (R, Q: the sides cut to these lengths)
and an optional cut (side, at, count: `count` columns removed from `side` at `at`, which the path answers with a run of the other
side's gap code; the X-drop of the pools does not prune these runs, so no per-column gap penalty is lowered), and the parameters.  All of it was searched on the CPU (tools/find_exit_cases.py) and is constant
here.  Every pair's band stays inside the smallest row window of the routes it is sent to (span < NV of dp_cases.PairTrace), so the
first launch's kernel is the one that makes the path.

Classes declared NOT REACHED (2000 generated pairs per marker 16, 33 and 128 and per family with one side shortened to 0.6; no test
depends on them): a trailing run behind a converged exit, a border fill of more than 64 codes, errorType-3 exits.  See NOT_REACHED at
the end of the module."""
from __future__ import annotations

import os
import sys
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dp_cases as D  # noqa: E402
import oracle_lib as O  # noqa: E402
from twilight_amd import synth  # noqa: E402

F_MARKERS = (2, 3, 7, 8, 9, 1023, 1024)


@dataclass(frozen=True)
class TileExit:
    tile: int
    last_k: int
    kind: int            # 0 converged, 1 ended before the marker, 2 ended at or behind the marker unconverged
    state: int           # tb_state 0..3
    conv_r: int
    conv_q: int
    ridx: int            # the pair's reference_idx / query_idx after the advance
    qidx: int
    last: bool           # no tile follows
    seg: int             # codes of its segment of the final path
    tail_dir: int        # the trailing run behind the last tile (0: none)
    tail_len: int
    run: Tuple[int, int, int]      # longest run of code 0, 1, 2 inside the WALKED segment (tile 0: without the border fill)
    border: bool         # tile 0: the walk left through the border (ridx < 0 || qidx < 0)
    fill: int            # ... and the fill added this many codes

    @property
    def key(self) -> Tuple[int, int, int]:
        return (self.kind, self.state, self.last_k)


def _longest_runs(seg: np.ndarray) -> Tuple[int, int, int]:
    best = [0, 0, 0]
    if seg.size:
        cut = np.flatnonzero(np.diff(seg)) + 1
        starts = np.concatenate(([0], cut))
        ends = np.concatenate((cut, [seg.size]))
        for s, e in zip(starts, ends):
            c = int(seg[s])
            best[c] = max(best[c], int(e - s))
    return tuple(best)


def records(raw, path: np.ndarray, R: int, Q: int) -> List[TileExit]:
    """One TileExit per raw hook record (tile, last_k, kind, state, conv_r, conv_q, ridx, qidx), from the final path (forward order)."""
    path = np.asarray(path, dtype=np.int8)
    cr = np.cumsum(path != 1)      # reference columns consumed by the prefix ending here
    cq = np.cumsum(path != 2)
    out, begin = [], 0
    for n, (tile, last_k, kind, state, conv_r, conv_q, ridx, qidx) in enumerate(raw):
        assert tile == n
        # the prefix that consumes ridx + 1 and qidx + 1 columns ends the tile
        hit = np.flatnonzero((cr == ridx + 1) & (cq == qidx + 1))
        assert hit.size == 1, (tile, ridx, qidx, hit)
        end = int(hit[0]) + 1
        last = n == len(raw) - 1
        seg = path[begin:end]
        tail = path[end:] if last else path[:0]
        tail_dir, tail_len = (int(tail[0]), int(tail.size)) if tail.size else (0, 0)
        assert not tail.size or (tail == tail[0]).all()
        # what the exit itself says of the trailing run (:671-678)
        want = (1, Q - qidx - 1) if (ridx == R - 1 and qidx < Q - 1) else (2, R - ridx - 1) if (qidx == Q - 1 and ridx < R - 1) else (0, 0)
        assert not last or want == (tail_dir, tail_len), (want, tail_dir, tail_len)
        border, fill = False, 0
        if tile == 0 and seg.size and seg[0] != 0:      # a walk that reaches cell (0, 0) ends with code 0 there; the fill's codes differ from the code of the cell it left through
            border = True
            fill = int(np.argmax(seg != seg[0])) if (seg != seg[0]).any() else int(seg.size)
        out.append(TileExit(tile, last_k, kind, state, conv_r, conv_q, ridx, qidx, last, int(seg.size), tail_dir, tail_len,
                            _longest_runs(seg[fill:]), border, fill))
        begin = end
    if raw:
        assert begin + out[-1].tail_len == path.size
    return out


def exits_of_pair(batch, i: int, matrix: np.ndarray, **pk):
    """(path, errorType, [TileExit]) of pair `i` of `batch` from the oracle with its exit hook."""
    R, Q = int(batch.len[i, 0]), int(batch.len[i, 1])
    P = batch.P
    raw = []
    path, err, _ = O.align_pair_exits(O.make_params(matrix, **pk), batch.freq[i, 0, :R, :P], batch.freq[i, 1, :Q, :P], batch.gap_open[i, 0, :R],
                                      batch.gap_extend[i, 0, :R], batch.gap_open[i, 1, :Q], batch.gap_extend[i, 1, :Q], int(batch.num[i, 0]),
                                      int(batch.num[i, 1]), exits=lambda _u, *rec: raw.append(tuple(int(v) for v in rec)))
    return path, err, (records(raw, path, R, Q) if err == 0 else [])


def tags_of(marker: int, R: int, Q: int, recs: List[TileExit], path: np.ndarray) -> set:
    """The classes a pair is in: every predicate written out."""
    t = set()
    for e in recs:
        d = e.last_k - marker
        where = "t0" if e.tile == 0 else "later"
        if e.kind == 0:                                           # A: converged
            t.add(f"conv.s{e.state}.{where}")
        elif e.kind == 1:                                         # B: ended before the marker (the end cell, state 0, the flush of a partial group of 8)
            assert e.last_k < marker and e.state == 0 and e.last
            t.add(f"before.mod{e.last_k % 8}")
            if d in (-1, -2):
                t.add(f"before.m{d}")
            if e.tile > 0 and e.last_k <= 8:
                t.add("before.later.small")
            if e.tile > 0 and e.last_k == 2:
                t.add("before.later.k2")
        else:                                                     # C: ended at or behind the marker, unconverged
            assert e.last_k >= marker
            t.add(f"unconv.s{e.state}")
            if 0 <= d <= 2:
                t.add(f"unconv.m+{d}")
            if not e.last:
                t.add("unconv.followed")
        if len(recs) == 1 and e.last_k == R + Q - 2 and -2 <= d <= 2:      # the ends of the lean kernel's phases A / B / C
            t.add(f"single.m{d:+d}")
        if e.tail_len:                                            # D: trailing runs
            t.add(f"tail{e.tail_dir}.{'long' if e.tail_len > 64 else 'short'}.{'conv' if e.kind == 0 else 'unconv'}")
        if e.border:                                              # E: the first tile's border exit and fill
            t.add(f"start{int(path[0])}")
            if e.fill > 64:
                t.add("fill>64")
        if marker in F_MARKERS:                                   # F
            t.add(f"marker{marker}.kind{e.kind}")
            t.add(f"marker{marker}.s{e.state}")
        if e.run[1] >= 64:                                        # G: the walk leaves the 64-row patch through its rows ...
            t.add("run1>=64")
        if e.run[2] >= 128:                                       # ... through the 16 groups of 8 diagonals ...
            t.add("run2>=128")
        if e.run[0] > 64 and marker >= 256:                       # ... and the ordinary refetch: matches across more than 128 diagonals
            t.add("match>128diag")
    return t


@dataclass(frozen=True)
class ExitCase:
    name: str
    P: int
    length: int
    n: int                                                         # synth.make_level_batch(n, length, seed=..., **gen), one batch per seed named in `pairs`
    marker: int
    gen: Tuple[Tuple[str, object], ...]
    pairs: Tuple[Tuple[int, int], ...]                             # (seed, pair of that seed's batch)
    trim: Optional[Tuple[Optional[Tuple[int, int]], ...]] = None
    cut: Optional[Tuple[Optional[Tuple[int, int, int]], ...]] = None
    xdrop: Optional[int] = None
    flen: int = 4096
    exits: Tuple[Tuple[Tuple[int, int, int], ...], ...] = ()      # per pair, per tile: (kind, tb_state, last_k)
    shapes: Tuple[Tuple[int, int, int, int, int], ...] = ()        # per pair: (tailDir, tailLen, border fill, longest walked run of code 1, of code 2)
    tags: Tuple[str, ...] = ()                                     # the classes the pool is in (sorted)
    mt: bool = False                                               # long enough for the tile-parallel plan (sumLen >= 3 * marker * n)

    def batch(self):
        pad = int(self.length * 1.1) + 16      # one pitch for the batches of every seed
        made = {seed: synth.make_level_batch(self.n, self.length, P=self.P, seed=seed, pad_to=pad, **dict(self.gen)) for seed in sorted({s for s, _ in self.pairs})}
        pick = lambda f: np.stack([getattr(made[seed], f)[i] for seed, i in self.pairs])      # noqa: E731
        b = synth.LevelBatch(P=self.P, seq_len=pad, freq=pick("freq"), gap_open=pick("gap_open"), gap_extend=pick("gap_extend"), len=pick("len"), num=pick("num"))
        freq, go, ge, ln = b.freq, b.gap_open, b.gap_extend, b.len
        for i in range(len(self.pairs)):
            c = self.cut[i] if self.cut is not None else None
            if c is not None:
                side, at, count = c
                L = int(ln[i, side])
                assert 0 < at and at + count < L
                for a in (freq, go, ge):
                    a[i, side, at:L - count] = a[i, side, at + count:L].copy()
                    a[i, side, L - count:L] = 0
                ln[i, side] = L - count
            tr = self.trim[i] if self.trim is not None else None
            if tr is not None:
                for side in range(2):
                    assert 1 <= tr[side] <= ln[i, side]
                    for a in (freq, go, ge):
                        a[i, side, tr[side]:] = 0
                    ln[i, side] = tr[side]
        return synth.LevelBatch(P=b.P, seq_len=b.seq_len, freq=freq, gap_open=go, gap_extend=ge, len=ln, num=b.num)

    def params(self) -> dict:
        pk = dict(marker=self.marker, flen=self.flen)
        if self.xdrop is not None:
            pk["xdrop"] = self.xdrop
        return pk

    def compute(self, batch=None):
        """Per pair (path, errorType, [TileExit], tags, PairTrace) from the oracle."""
        b = self.batch() if batch is None else batch
        M = D.matrix_of(self.P)

        def one(i):
            path, err, recs = exits_of_pair(b, i, M, **self.params())
            tg = tags_of(self.marker, int(b.len[i, 0]), int(b.len[i, 1]), recs, path) if err == 0 else set()
            return path, err, recs, tg, D.trace_pair(b, i, M, **self.params())

        with ThreadPoolExecutor(max_workers=4) as ex:
            return list(ex.map(one, range(b.n_pairs)))


def shape_of(recs: List[TileExit]) -> Tuple[int, int, int, int, int]:
    return (recs[-1].tail_dir, recs[-1].tail_len, recs[0].fill, max(e.run[1] for e in recs), max(e.run[2] for e in recs))


def check_case(case: ExitCase, res, batch) -> None:
    """The case is what it claims to be: raises AssertionError otherwise."""
    got_exits = tuple(tuple(e.key for e in recs) for _p, _e, recs, _t, _tr in res)
    tag = f"{case.name}: exits {got_exits}"
    assert 2 <= len(res) <= 6, tag
    assert all(err == 0 for _p, err, _r, _t, _tr in res), tag
    assert case.length <= (700 if case.P == 6 else 400) and int(batch.len.max()) <= 1.06 * case.length, (tag, batch.len.tolist())      # (the generator's jitter and indels)
    assert got_exits == case.exits, tag
    got_shapes = tuple(shape_of(recs) for _p, _e, recs, _t, _tr in res)
    assert got_shapes == case.shapes, f"{case.name}: shapes {got_shapes}"
    tags = tuple(sorted(set().union(*[t for _p, _e, _r, t, _tr in res])))
    assert tags == case.tags, f"{case.name}: tags {tags}"
    if case.mt:
        assert case.marker >= 64 and int(batch.len.sum()) >= 3 * case.marker * batch.n_pairs, tag


REQUIRED = tuple(
    [f"conv.s{s}.{w}" for s in range(4) for w in ("t0", "later")] +                                   # A
    ["before.m-1", "before.m-2"] + [f"before.mod{r}" for r in range(8)] + ["before.later.small"] +    # B
    [f"single.m{d:+d}" for d in (-2, -1, 0, 1, 2)] +
    [f"unconv.s{s}" for s in range(4)] + ["unconv.m+0", "unconv.m+1", "unconv.m+2", "unconv.followed"] +      # C
    [f"tail{d}.{ln}.unconv" for d in (1, 2) for ln in ("short", "long")] +                            # D
    ["start2", "start1"] +                                                                            # E (a path that starts with code 1 may be declared not reached: it was reached)
    [f"marker{m}.{x}" for m in (2, 3, 7, 8, 9) for x in ("kind0", "kind2", "s0", "s3")] +             # F (1023, 1024: every pool of that marker is a case; see the CPU test)
    ["run1>=64", "run2>=128", "match>128diag"])                                                       # G


def _c(**kw):
    return ExitCase(**kw)


GEN = (("members", ((1, 4), (1, 4))), ("indel", 0.02), ("sub", 0.1))      # (the survey's generator: tools/find_exit_cases.py)


CASES: List[ExitCase] = [
    # ---- nucleotide ----
    _c(name='nuc_m128_0', P=6, length=700, n=6, marker=128, gen=GEN, pairs=((0, 0), (0, 1), (0, 3), (0, 4), (1, 2), (2, 1)), xdrop=3000, mt=True, 
       exits=(((0, 0, 596), (0, 3, 452), (0, 0, 493), (0, 0, 480), (0, 3, 553), (0, 0, 436), (0, 3, 388), (0, 0, 334), (0, 0, 277), (0, 3, 212), (1, 0, 122)), ((0, 0, 481), (0, 0, 478), (0, 0, 529), (0, 0, 637), (0, 0, 511), (0, 3, 442), (0, 3, 402), (0, 0, 334), (0, 2, 263), (0, 3, 179), (1, 0, 83)), ((0, 3, 483), (0, 0, 487), (0, 0, 693), (0, 3, 479), (0, 0, 469), (0, 0, 440), (0, 3, 380), (0, 0, 307), (0, 3, 243), (0, 0, 191), (1, 0, 93)), ((0, 0, 617), (0, 0, 531), (0, 3, 518), (0, 0, 517), (0, 0, 509), (0, 3, 460), (0, 0, 446), (0, 0, 330), (0, 3, 313), (0, 3, 208), (2, 3, 142), (1, 0, 15)), ((0, 0, 469), (0, 0, 541), (0, 0, 535), (0, 3, 554), (0, 0, 552), (0, 0, 468), (0, 3, 444), (0, 3, 386), (0, 3, 333), (0, 0, 208), (2, 0, 140), (1, 0, 12)), ((0, 3, 447), (0, 3, 418), (0, 3, 435), (0, 0, 469), (0, 3, 437), (0, 1, 498), (0, 3, 380), (0, 2, 342), (0, 3, 249), (0, 0, 194), (1, 0, 96))), 
       shapes=((0, 0, 0, 13, 7), (0, 0, 0, 9, 9), (0, 0, 0, 6, 12), (0, 0, 0, 12, 12), (0, 0, 0, 11, 4), (0, 0, 0, 7, 7)), 
       tags=('before.mod0', 'before.mod2', 'before.mod3', 'before.mod4', 'before.mod5', 'before.mod7', 'conv.s0.later', 'conv.s0.t0', 'conv.s1.later', 'conv.s2.later', 'conv.s3.later', 'conv.s3.t0', 'unconv.followed', 'unconv.s0', 'unconv.s3')),
    _c(name='nuc_m128_1', P=6, length=700, n=6, marker=128, gen=GEN, pairs=((2, 3), (3, 5), (4, 0), (9, 5), (11, 3), (12, 3)), xdrop=3000, mt=True, 
       exits=(((0, 3, 512), (0, 0, 560), (0, 2, 511), (0, 3, 437), (0, 3, 449), (0, 3, 435), (0, 0, 391), (0, 3, 346), (0, 0, 263), (0, 3, 200), (1, 0, 126)), ((0, 1, 549), (0, 3, 461), (0, 0, 437), (0, 0, 466), (0, 3, 463), (0, 3, 440), (0, 3, 415), (0, 0, 318), (0, 3, 286), (0, 3, 189), (1, 0, 109)), ((0, 3, 680), (0, 1, 582), (0, 0, 470), (0, 3, 598), (0, 3, 547), (0, 3, 472), (0, 3, 395), (0, 0, 354), (0, 0, 272), (0, 0, 197), (2, 3, 129), (1, 0, 2)), ((0, 2, 497), (0, 3, 459), (0, 0, 450), (0, 0, 459), (0, 0, 440), (0, 1, 505), (0, 0, 416), (0, 0, 355), (0, 0, 286), (0, 3, 222), (2, 1, 153), (1, 0, 25)), ((0, 3, 498), (0, 3, 617), (0, 0, 526), (0, 0, 493), (0, 0, 494), (0, 0, 473), (0, 0, 447), (0, 0, 331), (0, 0, 285), (0, 3, 200), (2, 2, 135), (1, 0, 7)), ((0, 3, 457), (0, 0, 488), (0, 0, 476), (0, 0, 472), (0, 3, 570), (0, 3, 469), (0, 3, 398), (0, 3, 345), (0, 0, 263), (0, 0, 203), (1, 0, 127))), 
       shapes=((0, 0, 0, 7, 5), (0, 0, 0, 8, 13), (0, 0, 0, 4, 12), (0, 0, 0, 10, 9), (0, 0, 0, 8, 8), (0, 0, 0, 8, 11)), 
       tags=('before.later.k2', 'before.later.small', 'before.m-1', 'before.m-2', 'before.mod1', 'before.mod2', 'before.mod5', 'before.mod6', 'before.mod7', 'conv.s0.later', 'conv.s1.later', 'conv.s1.t0', 'conv.s2.later', 'conv.s2.t0', 'conv.s3.later', 'conv.s3.t0', 'unconv.followed', 'unconv.m+1', 'unconv.s1', 'unconv.s2', 'unconv.s3')),
    _c(name='nuc_m128_2', P=6, length=700, n=6, marker=128, gen=GEN, pairs=((14, 3), (20, 4)), xdrop=3000, mt=True, 
       exits=(((0, 0, 486), (0, 0, 440), (0, 3, 424), (0, 0, 521), (0, 3, 442), (0, 0, 484), (0, 3, 414), (0, 3, 332), (0, 0, 264), (0, 0, 196), (2, 0, 130), (1, 0, 2)), ((0, 3, 466), (0, 3, 517), (0, 0, 484), (0, 0, 495), (0, 0, 471), (0, 0, 454), (0, 3, 399), (0, 3, 354), (0, 3, 271), (0, 0, 204), (2, 0, 128))), 
       shapes=((0, 0, 0, 8, 10), (0, 0, 1, 4, 6)), 
       tags=('before.later.k2', 'before.later.small', 'before.mod2', 'conv.s0.later', 'conv.s0.t0', 'conv.s3.later', 'conv.s3.t0', 'start2', 'unconv.followed', 'unconv.m+0', 'unconv.m+2', 'unconv.s0')),
    _c(name='nuc_single0_m128', P=6, length=70, n=6, marker=128, gen=GEN, pairs=((0, 0), (0, 1), (0, 2), (0, 3), (0, 4), (0, 5)), trim=((61, 61), (62, 61), (62, 62), (63, 62), (63, 63), (64, 63)), mt=False, 
       exits=(((1, 0, 120),), ((1, 0, 121),), ((1, 0, 122),), ((1, 0, 123),), ((1, 0, 124),), ((1, 0, 125),)), 
       shapes=((0, 0, 0, 11, 6), (0, 0, 0, 0, 1), (0, 0, 0, 6, 6), (0, 0, 0, 3, 6), (0, 0, 0, 1, 1), (0, 0, 0, 0, 1)), 
       tags=('before.mod0', 'before.mod1', 'before.mod2', 'before.mod3', 'before.mod4', 'before.mod5')),
    _c(name='nuc_single1_m128', P=6, length=70, n=5, marker=128, gen=GEN, pairs=((6, 0), (6, 1), (6, 2), (6, 3), (6, 4)), trim=((64, 64), (65, 64), (65, 65), (66, 65), (66, 66)), mt=False, 
       exits=(((1, 0, 126),), ((1, 0, 127),), ((2, 0, 128),), ((2, 0, 129),), ((2, 1, 130),)), 
       shapes=((0, 0, 0, 2, 2), (0, 0, 0, 2, 5), (0, 0, 0, 3, 3), (1, 1, 0, 0, 2), (1, 2, 0, 2, 2)), 
       tags=('before.m-1', 'before.m-2', 'before.mod6', 'before.mod7', 'single.m+0', 'single.m+1', 'single.m+2', 'single.m-1', 'single.m-2', 'tail1.short.unconv', 'unconv.m+0', 'unconv.m+1', 'unconv.m+2', 'unconv.s0', 'unconv.s1')),
    _c(name='nuc_later_m128', P=6, length=700, n=3, marker=128, gen=GEN, pairs=((0, 0), (0, 1)), trim=((372, 398), (690, 672)), xdrop=3000, mt=True, 
       exits=(((0, 0, 521), (0, 3, 393), (0, 0, 341), (0, 0, 279), (0, 3, 239), (2, 0, 130), (1, 0, 2)), ((0, 0, 481), (0, 0, 478), (0, 0, 529), (0, 0, 637), (0, 0, 511), (0, 3, 442), (0, 3, 402), (0, 0, 334), (0, 2, 263), (0, 3, 179), (1, 0, 83))), 
       shapes=((0, 0, 0, 13, 7), (0, 0, 0, 9, 9)), 
       tags=('before.later.k2', 'before.later.small', 'before.mod2', 'before.mod3', 'conv.s0.later', 'conv.s0.t0', 'conv.s2.later', 'conv.s3.later', 'unconv.followed', 'unconv.m+2', 'unconv.s0')),
    _c(name='nuc_tails_m128', P=6, length=700, n=6, marker=128, gen=GEN, pairs=((0, 0), (8, 1), (36, 0), (0, 0), (0, 5), (5, 5)), trim=((412, 712), (418, 704), (416, 680), (688, 427), (708, 703), (720, 701)), xdrop=3000, mt=True, 
       exits=(((0, 0, 562), (0, 3, 440), (0, 0, 455), (2, 0, 739), (2, 3, 611), (2, 0, 484), (2, 1, 356)), ((0, 0, 463), (0, 3, 519), (0, 0, 515), (2, 0, 737), (2, 0, 609), (2, 3, 481), (2, 1, 354), (2, 1, 226)), ((0, 3, 419), (0, 3, 472), (0, 3, 432), (2, 0, 713), (2, 0, 585), (2, 1, 457), (2, 1, 329), (2, 3, 201), (1, 0, 74)), ((0, 0, 596), (0, 3, 452), (0, 0, 493), (2, 0, 730), (2, 3, 602), (2, 0, 475), (2, 2, 347), (2, 2, 219)), ((0, 0, 431), (0, 0, 451), (0, 0, 447), (0, 3, 438), (0, 0, 453), (0, 0, 502), (0, 3, 416), (0, 0, 330), (0, 3, 275), (0, 0, 211), (2, 1, 132)), ((0, 0, 463), (0, 0, 457), (0, 3, 508), (0, 3, 473), (0, 3, 470), (0, 3, 457), (0, 0, 428), (0, 0, 354), (0, 0, 281), (0, 0, 233), (2, 2, 143))), 
       shapes=((1, 228, 0, 49, 7), (1, 98, 1, 83, 5), (0, 0, 3, 95, 2), (2, 91, 0, 13, 79), (1, 4, 0, 16, 7), (2, 15, 0, 10, 7)), 
       tags=('before.mod2', 'conv.s0.later', 'conv.s0.t0', 'conv.s3.later', 'conv.s3.t0', 'run1>=64', 'start1', 'start2', 'tail1.long.unconv', 'tail1.short.unconv', 'tail2.long.unconv', 'tail2.short.unconv', 'unconv.followed', 'unconv.s0', 'unconv.s1', 'unconv.s2', 'unconv.s3')),
    _c(name='nuc_m2', P=6, length=120, n=6, marker=2, gen=GEN, pairs=((0, 0), (0, 1), (0, 2)), mt=False, 
       exits=(((0, 0, 143), (0, 0, 133), (0, 0, 129), (0, 0, 127), (0, 0, 125), (0, 0, 123), (0, 0, 129), (0, 0, 125), (0, 0, 125), (0, 0, 123), (0, 0, 119), (0, 0, 119), (0, 0, 117), (0, 0, 115), (0, 0, 115), (0, 0, 113), (0, 0, 113), (0, 0, 113), (0, 0, 111), (0, 0, 109), (0, 0, 109), (0, 0, 109), (0, 0, 107), (0, 0, 105), (0, 0, 109), (0, 0, 109), (0, 0, 103), (0, 0, 105), (0, 0, 103), (0, 0, 109), (0, 0, 97), (0, 0, 101), (0, 0, 95), (0, 0, 97), (0, 0, 95), (0, 0, 93), (0, 0, 91), (0, 0, 91), (0, 0, 89), (0, 0, 89), (0, 0, 87), (0, 0, 87), (0, 0, 85), (0, 0, 85), (0, 0, 89), (0, 0, 103), (0, 0, 101), (0, 0, 83), (0, 0, 97), (0, 0, 95), (0, 3, 101), (0, 0, 78), (0, 0, 88), (0, 0, 78), (0, 0, 76), (0, 0, 82), (0, 0, 76), (0, 0, 88), (0, 0, 86), (0, 0, 74), (0, 0, 78), (0, 0, 70), (0, 0, 74), (0, 0, 68), (0, 0, 66), (0, 0, 64), (0, 0, 62), (0, 0, 62), (0, 0, 62), (0, 0, 64), (0, 0, 58), (0, 0, 60), (0, 0, 58), (0, 0, 56), (0, 0, 54), (0, 0, 62), (0, 0, 60), (0, 0, 58), (0, 0, 56), (0, 0, 54), (0, 0, 52), (0, 0, 50), (0, 0, 48), (0, 0, 46), (0, 0, 44), (0, 0, 44), (0, 0, 46), (0, 0, 44), (0, 0, 42), (0, 0, 42), (0, 0, 42), (0, 0, 38), (0, 0, 38), (0, 0, 36), (0, 0, 34), (0, 0, 34), (0, 0, 32), (0, 0, 32), (0, 0, 32), (0, 0, 34), (0, 0, 32), (0, 0, 30), (0, 0, 26), (0, 0, 24), (0, 0, 24), (0, 0, 26), (0, 0, 24), (0, 0, 22), (0, 0, 26), (0, 0, 24), (0, 0, 18), (0, 0, 16), (0, 0, 18), (0, 0, 16), (2, 0, 17), (2, 0, 15), (2, 0, 13), (2, 0, 11), (2, 0, 9), (2, 0, 7), (2, 0, 5)), ((0, 0, 128), (0, 0, 126), (0, 0, 124), (0, 0, 122), (0, 0, 120), (0, 0, 118), (0, 0, 116), (0, 0, 114), (0, 0, 112), (0, 0, 112), (0, 0, 110), (0, 0, 110), (0, 0, 118), (0, 0, 116), (0, 0, 114), (0, 0, 112), (0, 0, 110), (0, 0, 108), (0, 0, 106), (0, 0, 104), (0, 0, 102), (0, 0, 104), (0, 0, 102), (0, 0, 100), (0, 0, 106), (0, 0, 98), (0, 0, 94), (0, 0, 94), (0, 0, 98), (0, 0, 96), (0, 0, 94), (0, 0, 92), (0, 0, 90), (0, 0, 88), (0, 0, 86), (0, 0, 90), (0, 0, 92), (0, 0, 86), (0, 0, 84), (0, 0, 88), (0, 0, 86), (0, 0, 84), (0, 0, 82), (0, 0, 80), (0, 0, 78), (0, 0, 76), (0, 0, 74), (0, 0, 74), (0, 0, 74), (0, 0, 72), (0, 0, 70), (0, 0, 72), (0, 0, 86), (0, 0, 84), (0, 0, 70), (0, 0, 82), (0, 0, 66), (0, 0, 78), (0, 0, 76), (0, 0, 74), (0, 0, 60), (0, 0, 68), (0, 0, 66), (0, 0, 64), (0, 0, 62), (0, 0, 64), (0, 0, 82), (0, 0, 56), (0, 0, 78), (0, 0, 52), (0, 0, 74), (0, 0, 72), (0, 0, 70), (0, 0, 68), (0, 0, 66), (0, 0, 64), (0, 0, 62), (0, 0, 60), (0, 0, 58), (0, 0, 56), (0, 0, 54), (0, 0, 52), (0, 0, 50), (0, 0, 48), (0, 0, 46), (0, 0, 44), (0, 0, 42), (0, 0, 40), (0, 0, 38), (0, 0, 36), (0, 0, 36), (0, 0, 34), (0, 0, 36), (0, 0, 28), (0, 0, 26), (0, 0, 30), (0, 0, 28), (0, 0, 26), (0, 1, 32), (0, 1, 28), (0, 0, 26), (0, 0, 24), (0, 0, 18), (0, 0, 16), (0, 0, 14), (0, 0, 14), (0, 0, 12), (0, 0, 10), (0, 0, 10), (0, 0, 8), (0, 0, 8), (2, 0, 6), (2, 0, 4), (2, 0, 2)), ((0, 0, 127), (0, 0, 125), (0, 0, 125), (0, 0, 123), (0, 0, 121), (0, 0, 123), (0, 0, 121), (0, 0, 119), (0, 0, 117), (0, 0, 115), (0, 0, 119), (0, 0, 117), (0, 0, 115), (0, 0, 113), (0, 0, 113), (0, 0, 111), (0, 0, 109), (0, 0, 113), (0, 2, 159), (0, 3, 121), (0, 0, 108), (0, 0, 106), (0, 0, 104), (0, 0, 102), (0, 0, 100), (0, 0, 112), (0, 0, 98), (0, 0, 100), (0, 0, 98), (0, 0, 96), (0, 0, 112), (0, 2, 134), (0, 0, 94), (0, 0, 92), (0, 0, 96), (0, 0, 94), (0, 0, 120), (0, 0, 88), (0, 0, 86), (0, 0, 84), (0, 0, 82), (0, 2, 110), (0, 2, 100), (0, 2, 98), (0, 2, 88), (0, 0, 86), (0, 0, 72), (0, 0, 70), (0, 0, 70), (0, 0, 70), (0, 0, 68), (0, 0, 66), (0, 0, 68), (0, 0, 66), (0, 0, 64), (0, 0, 84), (0, 0, 64), (0, 0, 66), (0, 0, 60), (0, 0, 60), (0, 0, 68), (0, 0, 66), (0, 0, 56), (0, 0, 54), (0, 0, 56), (0, 0, 60), (0, 0, 58), (0, 0, 62), (0, 0, 54), (0, 0, 58), (0, 0, 56), (0, 0, 54), (0, 0, 50), (0, 0, 48), (0, 0, 46), (0, 0, 46), (0, 0, 42), (0, 0, 40), (0, 0, 40), (0, 0, 38), (0, 0, 40), (0, 0, 38), (0, 0, 36), (0, 0, 42), (0, 0, 40), (0, 0, 38), (0, 0, 36), (0, 0, 30), (0, 0, 32), (0, 0, 30), (0, 0, 28), (0, 0, 26), (0, 0, 26), (0, 0, 24), (0, 0, 24), (0, 0, 22), (0, 0, 24), (0, 0, 22), (0, 0, 20), (0, 0, 18), (0, 0, 20), (0, 0, 18), (0, 0, 16), (0, 0, 14), (0, 0, 16), (0, 0, 14), (0, 0, 12), (0, 0, 10), (2, 0, 12), (2, 0, 10), (2, 0, 8), (0, 0, 6), (2, 0, 4), (2, 0, 2))), 
       shapes=((2, 3, 0, 1, 2), (0, 0, 0, 2, 0), (0, 0, 0, 0, 2)), 
       tags=('conv.s0.later', 'conv.s0.t0', 'conv.s1.later', 'conv.s2.later', 'conv.s3.later', 'marker2.kind0', 'marker2.kind2', 'marker2.s0', 'marker2.s1', 'marker2.s2', 'marker2.s3', 'tail2.short.unconv', 'unconv.followed', 'unconv.m+0', 'unconv.m+2', 'unconv.s0')),
    _c(name='nuc_m3', P=6, length=120, n=6, marker=3, gen=GEN, pairs=((0, 0), (0, 1)), mt=False, 
       exits=(((0, 3, 143), (0, 3, 133), (0, 3, 129), (0, 3, 127), (0, 3, 125), (0, 3, 131), (0, 3, 129), (0, 3, 127), (0, 3, 125), (0, 3, 123), (0, 3, 121), (0, 3, 119), (0, 3, 117), (0, 3, 117), (0, 3, 115), (0, 3, 115), (0, 3, 115), (0, 3, 113), (0, 3, 111), (0, 3, 111), (0, 3, 111), (0, 3, 109), (0, 3, 107), (0, 3, 111), (0, 3, 111), (0, 3, 109), (0, 3, 107), (0, 3, 105), (0, 2, 109), (0, 0, 108), (0, 3, 101), (0, 3, 99), (0, 3, 97), (0, 3, 95), (0, 3, 93), (0, 3, 93), (0, 3, 91), (0, 3, 91), (0, 3, 89), (0, 3, 89), (0, 3, 87), (0, 3, 87), (0, 3, 91), (0, 3, 105), (0, 3, 103), (0, 3, 101), (0, 3, 99), (0, 3, 97), (0, 0, 103), (0, 3, 90), (0, 3, 88), (0, 3, 78), (0, 3, 84), (0, 3, 82), (0, 3, 90), (0, 3, 88), (0, 3, 86), (0, 3, 80), (0, 3, 78), (0, 3, 76), (0, 3, 74), (0, 3, 68), (0, 3, 66), (0, 3, 64), (0, 3, 64), (0, 3, 64), (0, 3, 66), (0, 3, 64), (0, 3, 62), (0, 3, 60), (0, 3, 58), (0, 3, 56), (0, 3, 64), (0, 3, 62), (0, 3, 60), (0, 3, 58), (0, 3, 56), (0, 3, 54), (0, 3, 52), (0, 3, 50), (0, 3, 48), (0, 3, 46), (0, 3, 46), (0, 3, 48), (0, 3, 46), (0, 3, 44), (0, 3, 44), (0, 3, 44), (0, 3, 42), (0, 3, 40), (0, 3, 38), (0, 3, 36), (0, 3, 36), (0, 3, 34), (0, 3, 34), (0, 3, 34), (0, 3, 36), (0, 3, 34), (0, 2, 32), (0, 0, 29), (0, 3, 26), (0, 3, 28), (0, 3, 26), (0, 3, 24), (0, 3, 28), (0, 3, 26), (0, 3, 24), (0, 3, 18), (0, 3, 20), (0, 3, 18), (2, 3, 19), (2, 3, 17), (2, 3, 15), (2, 3, 13), (2, 3, 11), (2, 3, 9), (2, 3, 7), (2, 2, 5)), ((0, 3, 128), (0, 3, 126), (0, 3, 124), (0, 3, 122), (0, 3, 120), (0, 3, 118), (0, 3, 116), (0, 3, 114), (0, 3, 114), (0, 3, 112), (0, 3, 112), (0, 3, 120), (0, 3, 118), (0, 3, 116), (0, 3, 114), (0, 3, 112), (0, 3, 110), (0, 3, 108), (0, 3, 106), (0, 3, 104), (0, 3, 106), (0, 3, 104), (0, 3, 102), (0, 3, 108), (0, 3, 106), (0, 3, 98), (0, 3, 96), (0, 3, 100), (0, 3, 98), (0, 3, 96), (0, 3, 94), (0, 3, 92), (0, 3, 90), (0, 3, 88), (0, 3, 92), (0, 3, 94), (0, 3, 92), (0, 3, 86), (0, 3, 90), (0, 3, 88), (0, 3, 86), (0, 3, 84), (0, 3, 82), (0, 3, 80), (0, 3, 78), (0, 3, 76), (0, 3, 76), (0, 3, 76), (0, 3, 74), (0, 3, 72), (0, 3, 74), (0, 3, 88), (0, 3, 86), (0, 3, 84), (0, 3, 84), (0, 3, 82), (0, 3, 80), (0, 3, 78), (0, 3, 76), (0, 3, 74), (0, 3, 70), (0, 3, 68), (0, 3, 66), (0, 3, 64), (0, 3, 66), (0, 3, 84), (0, 3, 82), (0, 3, 80), (0, 3, 78), (0, 3, 76), (0, 3, 74), (0, 3, 72), (0, 3, 70), (0, 3, 68), (0, 3, 66), (0, 3, 64), (0, 3, 62), (0, 3, 60), (0, 3, 58), (0, 3, 56), (0, 3, 54), (0, 3, 52), (0, 3, 50), (0, 3, 48), (0, 3, 46), (0, 3, 44), (0, 3, 42), (0, 3, 40), (0, 3, 38), (0, 3, 38), (0, 3, 36), (0, 3, 38), (0, 3, 36), (0, 3, 28), (0, 3, 32), (0, 3, 30), (0, 3, 28), (0, 1, 34), (0, 1, 31), (0, 1, 26), (0, 0, 23), (0, 3, 16), (0, 3, 16), (0, 3, 14), (0, 3, 12), (0, 3, 12), (0, 3, 10), (0, 3, 10), (2, 3, 8), (2, 3, 6), (2, 3, 4), (1, 0, 2))), 
       shapes=((2, 2, 0, 1, 1), (0, 0, 0, 3, 0)), 
       tags=('before.later.k2', 'before.later.small', 'before.m-1', 'before.mod2', 'conv.s0.later', 'conv.s1.later', 'conv.s2.later', 'conv.s3.later', 'conv.s3.t0', 'marker3.kind0', 'marker3.kind1', 'marker3.kind2', 'marker3.s0', 'marker3.s1', 'marker3.s2', 'marker3.s3', 'tail2.short.unconv', 'unconv.followed', 'unconv.m+1', 'unconv.m+2', 'unconv.s2', 'unconv.s3')),
    _c(name='nuc_m7', P=6, length=120, n=6, marker=7, gen=GEN, pairs=((0, 0), (0, 1)), mt=False, 
       exits=(((0, 3, 143), (0, 3, 135), (0, 3, 129), (0, 3, 123), (0, 3, 119), (0, 3, 117), (0, 3, 115), (0, 3, 115), (0, 3, 111), (0, 3, 113), (0, 3, 103), (0, 3, 97), (0, 3, 95), (0, 3, 91), (0, 3, 109), (0, 3, 103), (0, 0, 105), (0, 3, 88), (0, 3, 92), (0, 3, 86), (0, 3, 76), (0, 3, 68), (0, 3, 68), (0, 3, 62), (0, 3, 66), (0, 3, 60), (0, 3, 54), (0, 3, 50), (0, 3, 48), (0, 3, 46), (0, 3, 40), (0, 3, 38), (0, 3, 38), (0, 3, 32), (0, 3, 30), (0, 3, 30), (0, 3, 24), (2, 3, 21), (2, 3, 15), (2, 2, 9)), ((0, 3, 128), (0, 3, 122), (0, 3, 118), (0, 3, 124), (0, 3, 118), (0, 3, 112), (0, 3, 110), (0, 3, 112), (0, 3, 106), (0, 3, 100), (0, 3, 100), (0, 3, 98), (0, 3, 94), (0, 3, 88), (0, 3, 82), (0, 3, 80), (0, 3, 78), (0, 3, 88), (0, 3, 84), (0, 3, 78), (0, 3, 70), (0, 3, 88), (0, 3, 82), (0, 3, 76), (0, 3, 70), (0, 3, 64), (0, 3, 58), (0, 3, 52), (0, 3, 46), (0, 3, 42), (0, 3, 40), (0, 3, 34), (0, 1, 36), (0, 0, 27), (0, 3, 18), (0, 3, 14), (2, 3, 10), (1, 0, 4))), 
       shapes=((2, 2, 0, 1, 2), (0, 0, 0, 3, 0)), 
       tags=('before.later.small', 'before.mod4', 'conv.s0.later', 'conv.s1.later', 'conv.s3.later', 'conv.s3.t0', 'marker7.kind0', 'marker7.kind1', 'marker7.kind2', 'marker7.s0', 'marker7.s1', 'marker7.s2', 'marker7.s3', 'tail2.short.unconv', 'unconv.followed', 'unconv.m+2', 'unconv.s2', 'unconv.s3')),
    _c(name='nuc_m8', P=6, length=120, n=6, marker=8, gen=GEN, pairs=((0, 0), (0, 1), (0, 2)), mt=False, 
       exits=(((0, 0, 143), (0, 0, 133), (0, 0, 125), (0, 0, 119), (0, 0, 115), (0, 0, 111), (0, 0, 111), (0, 0, 111), (0, 0, 99), (0, 0, 95), (0, 0, 91), (0, 0, 105), (0, 3, 105), (0, 0, 88), (0, 0, 90), (0, 0, 78), (0, 0, 68), (0, 0, 66), (0, 0, 68), (0, 0, 60), (0, 0, 52), (0, 0, 50), (0, 0, 46), (0, 0, 40), (0, 0, 40), (0, 0, 32), (0, 0, 28), (0, 0, 26), (2, 0, 21), (2, 0, 13), (1, 0, 5)), ((0, 0, 128), (0, 0, 120), (0, 0, 116), (0, 0, 118), (0, 0, 110), (0, 0, 106), (0, 0, 106), (0, 0, 98), (0, 0, 96), (0, 0, 94), (0, 0, 86), (0, 0, 80), (0, 0, 78), (0, 0, 88), (0, 0, 80), (0, 0, 70), (0, 0, 86), (0, 0, 78), (0, 0, 70), (0, 0, 62), (0, 0, 54), (0, 0, 46), (0, 0, 40), (0, 0, 36), (0, 1, 36), (0, 0, 26), (0, 0, 16), (2, 0, 12), (1, 0, 4)), ((0, 0, 129), (0, 0, 125), (0, 0, 123), (0, 0, 117), (0, 3, 163), (0, 0, 108), (0, 0, 114), (0, 2, 140), (0, 0, 100), (0, 0, 120), (0, 2, 112), (0, 0, 88), (0, 0, 72), (0, 0, 90), (0, 0, 68), (0, 0, 68), (0, 0, 68), (0, 0, 60), (0, 0, 52), (0, 0, 44), (0, 0, 48), (0, 0, 40), (0, 0, 32), (0, 0, 28), (0, 0, 24), (0, 0, 20), (0, 0, 16), (2, 0, 12), (1, 0, 4))), 
       shapes=((0, 0, 0, 1, 3), (0, 0, 0, 4, 0), (0, 0, 0, 0, 6)), 
       tags=('before.later.small', 'before.mod4', 'before.mod5', 'conv.s0.later', 'conv.s0.t0', 'conv.s1.later', 'conv.s2.later', 'conv.s3.later', 'marker8.kind0', 'marker8.kind1', 'marker8.kind2', 'marker8.s0', 'marker8.s1', 'marker8.s2', 'marker8.s3', 'unconv.followed', 'unconv.s0')),
    _c(name='nuc_m9', P=6, length=120, n=6, marker=9, gen=GEN, pairs=((0, 0), (0, 1)), mt=False, 
       exits=(((0, 3, 143), (0, 3, 133), (0, 3, 125), (0, 3, 121), (0, 3, 117), (0, 3, 117), (0, 3, 111), (0, 3, 111), (0, 3, 99), (0, 3, 95), (0, 3, 97), (0, 3, 105), (0, 0, 105), (0, 3, 96), (0, 3, 88), (0, 3, 76), (0, 3, 72), (0, 3, 64), (0, 3, 66), (0, 3, 58), (0, 3, 52), (0, 3, 50), (0, 3, 44), (0, 3, 40), (0, 2, 38), (0, 0, 33), (0, 3, 30), (0, 3, 22), (2, 3, 17), (2, 0, 9)), ((0, 3, 128), (0, 3, 120), (0, 3, 126), (0, 3, 118), (0, 3, 110), (0, 3, 114), (0, 3, 106), (0, 3, 98), (0, 3, 100), (0, 3, 94), (0, 3, 86), (0, 3, 82), (0, 3, 94), (0, 3, 88), (0, 3, 80), (0, 3, 70), (0, 3, 86), (0, 3, 78), (0, 3, 70), (0, 3, 62), (0, 3, 54), (0, 3, 46), (0, 3, 44), (0, 3, 36), (0, 1, 36), (0, 0, 25), (0, 3, 16), (2, 3, 10), (1, 0, 2))), 
       shapes=((0, 0, 0, 1, 3), (0, 0, 0, 5, 0)), 
       tags=('before.later.k2', 'before.later.small', 'before.mod2', 'conv.s0.later', 'conv.s1.later', 'conv.s2.later', 'conv.s3.later', 'conv.s3.t0', 'marker9.kind0', 'marker9.kind1', 'marker9.kind2', 'marker9.s0', 'marker9.s1', 'marker9.s2', 'marker9.s3', 'unconv.followed', 'unconv.m+0', 'unconv.m+1', 'unconv.s0', 'unconv.s3')),
    _c(name='nuc_m1023', P=6, length=700, n=6, marker=1023, gen=GEN, pairs=((0, 0), (0, 1)), xdrop=3000, mt=False, 
       exits=(((0, 0, 1227), (1, 0, 375)), ((0, 3, 1228), (1, 0, 338))), 
       shapes=((0, 0, 0, 13, 7), (0, 0, 0, 9, 9)), 
       tags=('before.mod2', 'before.mod7', 'conv.s0.t0', 'conv.s3.t0', 'marker1023.kind0', 'marker1023.kind1', 'marker1023.s0', 'marker1023.s3', 'match>128diag')),
    _c(name='nuc_m1024', P=6, length=700, n=6, marker=1024, gen=GEN, pairs=((0, 0), (0, 1)), xdrop=3000, mt=False, 
       exits=(((0, 3, 1227), (1, 0, 375)), ((0, 0, 1228), (1, 0, 336))), 
       shapes=((0, 0, 0, 13, 7), (0, 0, 0, 9, 9)), 
       tags=('before.mod0', 'before.mod7', 'conv.s0.t0', 'conv.s3.t0', 'marker1024.kind0', 'marker1024.kind1', 'marker1024.s0', 'marker1024.s3', 'match>128diag')),
    _c(name='nuc_runs_m512', P=6, length=700, n=3, marker=512, gen=GEN, pairs=((7, 0), (7, 1), (7, 2)), cut=((1, 150, 140), (0, 150, 72), (0, 120, 200)), xdrop=3000, mt=False, 
       exits=(((0, 3, 1123), (0, 0, 632), (1, 0, 218)), ((0, 3, 1133), (0, 3, 693), (1, 0, 335)), ((0, 0, 1071), (0, 3, 616), (1, 0, 172))), 
       shapes=((0, 0, 0, 4, 132), (0, 0, 0, 46, 10), (0, 0, 0, 217, 8)), 
       tags=('before.mod2', 'before.mod4', 'before.mod7', 'conv.s0.later', 'conv.s0.t0', 'conv.s3.later', 'conv.s3.t0', 'match>128diag', 'run1>=64', 'run2>=128')),
    # ---- protein ----
    _c(name='prot_m128_0', P=22, length=400, n=6, marker=128, gen=GEN, pairs=((0, 0), (0, 1), (0, 2), (1, 4), (2, 3), (3, 4)), xdrop=3000, mt=True, 
       exits=(((0, 0, 392), (0, 0, 380), (0, 0, 358), (0, 0, 294), (0, 0, 229), (0, 0, 163), (1, 0, 66)), ((0, 3, 399), (0, 3, 382), (0, 3, 346), (0, 0, 280), (0, 3, 224), (0, 0, 152), (1, 0, 41)), ((0, 0, 350), (0, 0, 391), (0, 0, 343), (0, 3, 295), (0, 0, 218), (2, 3, 166), (1, 0, 39)), ((0, 0, 386), (0, 3, 406), (0, 3, 343), (0, 0, 276), (0, 0, 209), (2, 0, 151), (1, 0, 23)), ((0, 3, 388), (0, 1, 407), (0, 3, 333), (0, 0, 276), (0, 0, 207), (0, 3, 141), (1, 0, 18)), ((0, 0, 407), (0, 3, 420), (0, 2, 354), (0, 0, 276), (0, 0, 206), (0, 0, 142), (1, 0, 22))), 
       shapes=((0, 0, 0, 6, 9), (0, 0, 0, 11, 6), (0, 0, 0, 8, 4), (0, 0, 0, 11, 11), (0, 0, 0, 3, 5), (0, 0, 0, 10, 9)), 
       tags=('before.mod1', 'before.mod2', 'before.mod6', 'before.mod7', 'conv.s0.later', 'conv.s0.t0', 'conv.s1.later', 'conv.s2.later', 'conv.s3.later', 'conv.s3.t0', 'unconv.followed', 'unconv.s0', 'unconv.s3')),
    _c(name='prot_m128_1', P=22, length=400, n=6, marker=128, gen=GEN, pairs=((6, 2), (12, 1), (24, 0), (26, 1), (28, 1), (29, 2)), xdrop=3000, mt=True, 
       exits=(((0, 0, 392), (0, 3, 366), (0, 3, 337), (0, 0, 271), (0, 3, 205), (2, 3, 129), (1, 0, 2)), ((0, 0, 373), (0, 0, 331), (0, 3, 325), (0, 0, 261), (0, 3, 197), (1, 0, 127)), ((0, 0, 374), (0, 0, 389), (0, 0, 326), (0, 3, 260), (0, 3, 197), (2, 2, 129)), ((0, 0, 409), (0, 3, 395), (0, 0, 327), (0, 0, 269), (0, 0, 202), (2, 2, 130)), ((0, 0, 429), (0, 3, 400), (0, 0, 341), (0, 3, 275), (0, 0, 206), (2, 1, 136), (1, 0, 8)), ((0, 0, 355), (0, 0, 343), (0, 3, 325), (0, 0, 259), (0, 3, 195), (2, 0, 128))), 
       shapes=((0, 0, 0, 8, 13), (0, 0, 0, 6, 4), (2, 1, 0, 11, 5), (2, 2, 0, 4, 3), (0, 0, 0, 12, 11), (0, 0, 0, 8, 5)), 
       tags=('before.later.k2', 'before.later.small', 'before.m-1', 'before.mod0', 'before.mod2', 'before.mod7', 'conv.s0.later', 'conv.s0.t0', 'conv.s3.later', 'tail2.short.unconv', 'unconv.followed', 'unconv.m+0', 'unconv.m+1', 'unconv.m+2', 'unconv.s0', 'unconv.s1', 'unconv.s2', 'unconv.s3')),
    _c(name='prot_m128_2', P=22, length=400, n=6, marker=128, gen=GEN, pairs=((36, 3), (51, 0), (62, 4)), xdrop=3000, mt=True, 
       exits=(((0, 1, 410), (0, 3, 453), (0, 3, 352), (0, 1, 297), (0, 0, 219), (0, 3, 155), (1, 0, 50)), ((0, 2, 420), (0, 0, 390), (0, 0, 337), (0, 0, 278), (0, 0, 206), (2, 0, 149), (1, 0, 21)), ((0, 0, 389), (0, 0, 388), (0, 3, 328), (0, 3, 278), (0, 0, 193), (1, 0, 126))), 
       shapes=((0, 0, 0, 6, 6), (0, 0, 0, 5, 7), (0, 0, 0, 6, 15)), 
       tags=('before.m-2', 'before.mod2', 'before.mod5', 'before.mod6', 'conv.s0.later', 'conv.s0.t0', 'conv.s1.later', 'conv.s1.t0', 'conv.s2.t0', 'conv.s3.later', 'unconv.followed', 'unconv.s0')),
    _c(name='prot_single0_m128', P=22, length=70, n=6, marker=128, gen=GEN, pairs=((0, 0), (0, 1), (0, 2), (0, 3), (0, 4), (0, 5)), trim=((61, 61), (62, 61), (62, 62), (63, 62), (63, 63), (64, 63)), mt=False, 
       exits=(((1, 0, 120),), ((1, 0, 121),), ((1, 0, 122),), ((1, 0, 123),), ((1, 0, 124),), ((1, 0, 125),)), 
       shapes=((0, 0, 0, 0, 0), (0, 0, 0, 3, 4), (0, 0, 1, 6, 5), (0, 0, 0, 3, 5), (0, 0, 0, 3, 5), (0, 0, 0, 1, 2)), 
       tags=('before.mod0', 'before.mod1', 'before.mod2', 'before.mod3', 'before.mod4', 'before.mod5', 'start2')),
    _c(name='prot_single1_m128', P=22, length=70, n=5, marker=128, gen=GEN, pairs=((2, 0), (2, 1), (2, 2), (2, 3), (2, 4)), trim=((64, 64), (65, 64), (65, 65), (66, 65), (66, 66)), mt=False, 
       exits=(((1, 0, 126),), ((1, 0, 127),), ((2, 0, 128),), ((2, 2, 129),), ((2, 0, 130),)), 
       shapes=((0, 0, 0, 6, 8), (0, 0, 0, 3, 4), (0, 0, 0, 7, 9), (2, 1, 0, 2, 2), (1, 2, 0, 1, 2)), 
       tags=('before.m-1', 'before.m-2', 'before.mod6', 'before.mod7', 'single.m+0', 'single.m+1', 'single.m+2', 'single.m-1', 'single.m-2', 'tail1.short.unconv', 'tail2.short.unconv', 'unconv.m+0', 'unconv.m+1', 'unconv.m+2', 'unconv.s0', 'unconv.s2')),
    _c(name='prot_later_m128', P=22, length=400, n=3, marker=128, gen=GEN, pairs=((0, 0), (0, 1)), trim=((258, 258), (402, 405)), xdrop=3000, mt=True, 
       exits=(((0, 0, 342), (0, 0, 262), (0, 0, 200), (2, 0, 130), (1, 0, 2)), ((0, 3, 399), (0, 3, 382), (0, 3, 346), (0, 0, 280), (0, 3, 224), (0, 0, 152), (1, 0, 41))), 
       shapes=((0, 0, 0, 5, 9), (0, 0, 0, 11, 6)), 
       tags=('before.later.k2', 'before.later.small', 'before.mod1', 'before.mod2', 'conv.s0.later', 'conv.s0.t0', 'conv.s3.later', 'conv.s3.t0', 'unconv.followed', 'unconv.m+2', 'unconv.s0')),
    _c(name='prot_tails_m128', P=22, length=400, n=6, marker=128, gen=GEN, pairs=((1, 1), (6, 3), (7, 2), (0, 0), (1, 2), (1, 2)), trim=((250, 415), (235, 397), (237, 394), (415, 252), (381, 388), (393, 376)), xdrop=3000, mt=True, 
       exits=(((0, 0, 374), (2, 3, 535), (2, 3, 408), (2, 1, 281)), ((0, 0, 370), (2, 0, 502), (2, 0, 374), (2, 3, 246), (1, 0, 119)), ((0, 3, 360), (2, 3, 502), (2, 0, 375), (2, 1, 247), (1, 0, 119)), ((0, 0, 378), (2, 0, 537), (2, 0, 409), (2, 2, 281)), ((0, 3, 388), (0, 0, 347), (0, 3, 333), (0, 0, 266), (0, 0, 201), (2, 1, 129)), ((0, 3, 388), (0, 0, 347), (0, 3, 329), (0, 0, 270), (0, 0, 201), (2, 2, 129))), 
       shapes=((1, 153, 0, 11, 5), (0, 0, 6, 90, 2), (0, 0, 1, 109, 7), (2, 153, 0, 5, 10), (1, 1, 0, 11, 7), (2, 1, 0, 6, 11)), 
       tags=('before.mod7', 'conv.s0.later', 'conv.s0.t0', 'conv.s3.later', 'conv.s3.t0', 'run1>=64', 'start1', 'start2', 'tail1.long.unconv', 'tail1.short.unconv', 'tail2.long.unconv', 'tail2.short.unconv', 'unconv.followed', 'unconv.m+1', 'unconv.s0', 'unconv.s1', 'unconv.s2', 'unconv.s3')),
    _c(name='prot_m2', P=22, length=120, n=6, marker=2, gen=GEN, pairs=((0, 0), (0, 1)), mt=False, 
       exits=(((0, 2, 135), (0, 3, 131), (0, 0, 126), (0, 0, 126), (0, 0, 124), (0, 0, 124), (0, 0, 122), (0, 0, 122), (0, 0, 130), (0, 0, 128), (0, 0, 126), (0, 0, 124), (0, 0, 122), (0, 0, 120), (0, 0, 118), (0, 0, 116), (0, 0, 114), (0, 0, 112), (0, 0, 110), (0, 0, 112), (0, 0, 110), (0, 0, 108), (0, 0, 106), (0, 0, 111), (0, 0, 109), (0, 0, 107), (0, 0, 105), (0, 0, 103), (0, 0, 101), (0, 0, 101), (0, 0, 99), (0, 0, 99), (0, 0, 97), (0, 0, 95), (0, 0, 95), (0, 0, 93), (0, 0, 93), (0, 0, 91), (0, 0, 93), (0, 0, 91), (0, 0, 103), (0, 0, 97), (0, 0, 97), (0, 2, 95), (0, 2, 93), (0, 0, 89), (0, 0, 87), (0, 0, 85), (0, 0, 83), (0, 0, 81), (0, 0, 81), (0, 0, 79), (0, 0, 79), (0, 0, 77), (0, 0, 77), (0, 0, 75), (0, 0, 77), (0, 0, 75), (0, 0, 75), (0, 0, 71), (0, 0, 71), (0, 0, 69), (0, 0, 69), (0, 0, 67), (0, 0, 67), (0, 0, 65), (0, 0, 74), (0, 0, 72), (0, 0, 70), (0, 0, 68), (0, 0, 66), (0, 0, 64), (0, 0, 62), (0, 0, 60), (0, 0, 60), (0, 3, 58), (0, 0, 55), (0, 0, 53), (0, 0, 53), (0, 0, 51), (0, 0, 51), (0, 0, 49), (0, 0, 51), (0, 0, 49), (0, 0, 47), (0, 0, 45), (0, 0, 45), (0, 0, 45), (0, 0, 45), (0, 0, 41), (0, 0, 41), (0, 0, 39), (0, 0, 41), (0, 0, 39), (0, 0, 37), (0, 0, 35), (0, 0, 35), (0, 0, 33), (0, 3, 39), (0, 0, 38), (0, 0, 36), (0, 0, 34), (0, 0, 32), (0, 0, 30), (0, 0, 28), (0, 0, 26), (0, 0, 26), (0, 0, 24), (0, 0, 22), (0, 0, 22), (0, 0, 20), (2, 0, 25), (2, 0, 23), (2, 0, 21), (2, 0, 19), (2, 0, 17), (2, 0, 15), (2, 0, 13), (2, 0, 11), (2, 0, 9), (2, 1, 7), (2, 1, 5), (2, 3, 3), (2, 0, 2)), ((0, 0, 125), (0, 0, 123), (0, 0, 123), (0, 0, 121), (0, 0, 121), (0, 0, 119), (0, 0, 119), (0, 0, 117), (0, 0, 119), (0, 0, 117), (0, 0, 123), (0, 0, 121), (0, 0, 115), (0, 0, 113), (0, 0, 111), (0, 0, 113), (0, 0, 111), (0, 0, 109), (0, 0, 107), (0, 0, 105), (0, 0, 107), (0, 0, 105), (0, 0, 103), (0, 0, 101), (0, 0, 103), (0, 0, 99), (0, 0, 105), (0, 0, 99), (0, 0, 97), (0, 0, 99), (0, 3, 117), (0, 0, 96), (0, 0, 114), (0, 0, 112), (0, 0, 110), (0, 0, 108), (0, 0, 106), (0, 0, 104), (0, 0, 102), (0, 0, 100), (0, 0, 98), (0, 0, 96), (0, 0, 94), (0, 0, 92), (0, 0, 90), (0, 0, 88), (0, 0, 86), (0, 0, 84), (0, 0, 82), (0, 0, 80), (0, 0, 78), (0, 0, 76), (0, 0, 82), (0, 0, 74), (0, 0, 72), (0, 0, 76), (0, 0, 70), (0, 0, 72), (0, 0, 70), (0, 0, 68), (0, 0, 66), (0, 0, 66), (0, 0, 64), (0, 0, 78), (0, 0, 76), (0, 0, 74), (0, 0, 72), (0, 0, 70), (0, 0, 68), (0, 0, 66), (0, 0, 64), (0, 0, 62), (0, 0, 60), (0, 0, 58), (0, 0, 56), (0, 0, 54), (0, 0, 52), (0, 0, 50), (0, 0, 48), (0, 0, 50), (0, 0, 50), (0, 1, 52), (0, 0, 48), (0, 0, 44), (0, 0, 42), (0, 0, 40), (0, 0, 40), (0, 0, 38), (0, 0, 36), (0, 0, 36), (0, 0, 34), (0, 0, 36), (0, 0, 32), (0, 0, 32), (0, 0, 44), (0, 1, 42), (0, 0, 40), (0, 0, 26), (0, 0, 36), (0, 0, 34), (0, 0, 32), (0, 0, 30), (0, 0, 28), (0, 0, 26), (0, 0, 24), (0, 0, 22), (0, 0, 20), (0, 0, 18), (0, 0, 16), (0, 0, 16), (0, 0, 18), (0, 0, 12), (0, 0, 14), (0, 0, 12), (0, 0, 10), (0, 0, 8), (0, 0, 6), (2, 0, 4), (2, 0, 2))), 
       shapes=((0, 0, 0, 2, 2), (0, 0, 0, 2, 2)), 
       tags=('conv.s0.later', 'conv.s0.t0', 'conv.s1.later', 'conv.s2.later', 'conv.s2.t0', 'conv.s3.later', 'marker2.kind0', 'marker2.kind2', 'marker2.s0', 'marker2.s1', 'marker2.s2', 'marker2.s3', 'unconv.followed', 'unconv.m+0', 'unconv.m+1', 'unconv.m+2', 'unconv.s0', 'unconv.s1', 'unconv.s3')),
    _c(name='prot_m3', P=22, length=120, n=6, marker=3, gen=GEN, pairs=((0, 0), (0, 1)), mt=False, 
       exits=(((0, 0, 135), (0, 3, 128), (0, 3, 126), (0, 3, 126), (0, 3, 124), (0, 3, 124), (0, 3, 132), (0, 3, 130), (0, 3, 128), (0, 3, 126), (0, 3, 124), (0, 3, 122), (0, 3, 120), (0, 3, 118), (0, 3, 116), (0, 3, 114), (0, 3, 112), (0, 3, 114), (0, 3, 112), (0, 3, 110), (0, 3, 108), (0, 3, 113), (0, 3, 111), (0, 3, 109), (0, 3, 107), (0, 3, 105), (0, 3, 103), (0, 3, 103), (0, 3, 101), (0, 3, 101), (0, 3, 99), (0, 3, 97), (0, 3, 97), (0, 3, 95), (0, 3, 95), (0, 3, 93), (0, 3, 95), (0, 3, 93), (0, 1, 105), (0, 3, 98), (0, 3, 96), (0, 2, 98), (0, 2, 93), (0, 0, 88), (0, 3, 85), (0, 3, 83), (0, 3, 83), (0, 3, 81), (0, 3, 81), (0, 3, 79), (0, 3, 79), (0, 3, 77), (0, 3, 79), (0, 3, 77), (0, 3, 77), (0, 3, 75), (0, 3, 73), (0, 3, 71), (0, 3, 71), (0, 3, 69), (0, 3, 69), (0, 3, 67), (0, 3, 76), (0, 3, 74), (0, 3, 72), (0, 3, 70), (0, 3, 68), (0, 3, 66), (0, 3, 64), (0, 3, 62), (0, 3, 60), (0, 0, 60), (0, 3, 55), (0, 3, 55), (0, 3, 53), (0, 3, 53), (0, 3, 51), (0, 3, 53), (0, 3, 51), (0, 3, 49), (0, 3, 47), (0, 3, 47), (0, 3, 47), (0, 3, 47), (0, 3, 45), (0, 3, 43), (0, 3, 41), (0, 3, 43), (0, 3, 41), (0, 3, 39), (0, 3, 37), (0, 3, 37), (0, 3, 35), (0, 0, 41), (0, 3, 38), (0, 3, 36), (0, 3, 34), (0, 3, 32), (0, 3, 30), (0, 3, 28), (0, 3, 28), (0, 3, 26), (0, 3, 24), (0, 3, 24), (0, 3, 22), (2, 3, 27), (2, 3, 25), (2, 3, 23), (2, 1, 21), (2, 0, 18), (2, 3, 15), (2, 3, 13), (2, 3, 11), (2, 1, 9), (2, 1, 6)), ((0, 3, 125), (0, 3, 125), (0, 3, 123), (0, 3, 123), (0, 3, 121), (0, 3, 121), (0, 3, 119), (0, 3, 121), (0, 3, 119), (0, 3, 125), (0, 3, 123), (0, 3, 121), (0, 3, 115), (0, 3, 113), (0, 3, 115), (0, 3, 113), (0, 3, 111), (0, 3, 109), (0, 3, 107), (0, 3, 109), (0, 3, 107), (0, 3, 105), (0, 3, 103), (0, 3, 105), (0, 3, 103), (0, 2, 107), (0, 0, 104), (0, 3, 101), (0, 0, 119), (0, 3, 116), (0, 3, 114), (0, 3, 112), (0, 3, 110), (0, 3, 108), (0, 3, 106), (0, 3, 104), (0, 3, 102), (0, 3, 100), (0, 3, 98), (0, 3, 96), (0, 3, 94), (0, 3, 92), (0, 3, 90), (0, 3, 88), (0, 3, 86), (0, 3, 84), (0, 3, 82), (0, 3, 80), (0, 3, 78), (0, 3, 84), (0, 3, 82), (0, 3, 74), (0, 3, 78), (0, 3, 76), (0, 3, 74), (0, 3, 72), (0, 3, 70), (0, 3, 68), (0, 3, 68), (0, 3, 66), (0, 3, 80), (0, 3, 78), (0, 3, 76), (0, 3, 74), (0, 3, 72), (0, 3, 70), (0, 3, 68), (0, 3, 66), (0, 3, 64), (0, 3, 62), (0, 3, 60), (0, 3, 58), (0, 3, 56), (0, 3, 54), (0, 3, 52), (0, 3, 50), (0, 3, 52), (0, 3, 52), (0, 1, 54), (0, 0, 49), (0, 3, 44), (0, 3, 42), (0, 3, 42), (0, 3, 40), (0, 3, 38), (0, 3, 38), (0, 3, 36), (0, 3, 38), (0, 3, 36), (0, 3, 34), (0, 3, 46), (0, 1, 44), (0, 0, 41), (0, 3, 38), (0, 3, 36), (0, 3, 34), (0, 3, 32), (0, 3, 30), (0, 3, 28), (0, 3, 26), (0, 3, 24), (0, 3, 22), (0, 3, 20), (0, 3, 18), (0, 3, 18), (0, 3, 20), (0, 3, 18), (0, 3, 16), (0, 3, 14), (0, 3, 12), (0, 3, 10), (0, 3, 8), (2, 3, 6), (2, 3, 4), (1, 0, 2))), 
       shapes=((1, 3, 0, 1, 3), (0, 0, 0, 3, 1)), 
       tags=('before.later.k2', 'before.later.small', 'before.m-1', 'before.mod2', 'conv.s0.later', 'conv.s0.t0', 'conv.s1.later', 'conv.s2.later', 'conv.s3.later', 'conv.s3.t0', 'marker3.kind0', 'marker3.kind1', 'marker3.kind2', 'marker3.s0', 'marker3.s1', 'marker3.s2', 'marker3.s3', 'tail1.short.unconv', 'unconv.followed', 'unconv.m+1', 'unconv.s0', 'unconv.s1', 'unconv.s3')),
    _c(name='prot_m7', P=22, length=120, n=6, marker=7, gen=GEN, pairs=((0, 0), (0, 1)), mt=False, 
       exits=(((0, 0, 135), (0, 3, 128), (0, 3, 132), (0, 3, 126), (0, 3, 120), (0, 3, 118), (0, 3, 112), (0, 3, 113), (0, 3, 107), (0, 3, 105), (0, 3, 101), (0, 3, 97), (0, 1, 109), (0, 2, 102), (0, 3, 93), (0, 3, 87), (0, 3, 83), (0, 3, 83), (0, 3, 79), (0, 3, 75), (0, 3, 71), (0, 3, 76), (0, 3, 70), (0, 3, 64), (0, 0, 60), (0, 3, 55), (0, 3, 53), (0, 3, 51), (0, 3, 47), (0, 3, 45), (0, 3, 41), (0, 0, 43), (0, 3, 36), (0, 3, 32), (0, 3, 28), (2, 3, 29), (2, 3, 23), (2, 3, 17), (2, 1, 11), (1, 0, 4)), ((0, 3, 127), (0, 3, 125), (0, 3, 123), (0, 3, 125), (0, 3, 119), (0, 3, 113), (0, 3, 111), (0, 3, 109), (0, 3, 109), (0, 0, 123), (0, 3, 116), (0, 3, 110), (0, 3, 104), (0, 3, 98), (0, 3, 92), (0, 3, 86), (0, 3, 88), (0, 3, 82), (0, 3, 76), (0, 3, 72), (0, 3, 82), (0, 3, 76), (0, 3, 70), (0, 3, 64), (0, 3, 58), (0, 3, 56), (0, 1, 56), (0, 0, 45), (0, 3, 42), (0, 3, 40), (0, 1, 48), (0, 0, 41), (0, 3, 34), (0, 3, 28), (0, 3, 22), (0, 3, 22), (0, 3, 16), (2, 3, 10), (1, 0, 4))), 
       shapes=((0, 0, 0, 3, 4), (0, 0, 0, 3, 2)), 
       tags=('before.later.small', 'before.mod4', 'conv.s0.later', 'conv.s0.t0', 'conv.s1.later', 'conv.s2.later', 'conv.s3.later', 'conv.s3.t0', 'marker7.kind0', 'marker7.kind1', 'marker7.kind2', 'marker7.s0', 'marker7.s1', 'marker7.s2', 'marker7.s3', 'unconv.followed', 'unconv.s1', 'unconv.s3')),
    _c(name='prot_m8', P=22, length=120, n=6, marker=8, gen=GEN, pairs=((0, 0), (0, 1)), mt=False, 
       exits=(((0, 3, 135), (0, 0, 128), (0, 0, 130), (0, 0, 122), (0, 0, 118), (0, 0, 117), (0, 0, 109), (0, 0, 105), (0, 0, 99), (0, 0, 97), (0, 2, 103), (0, 0, 93), (0, 0, 85), (0, 0, 81), (0, 0, 79), (0, 0, 73), (0, 0, 78), (0, 0, 70), (0, 3, 64), (0, 0, 57), (0, 0, 55), (0, 0, 51), (0, 0, 45), (0, 0, 41), (0, 3, 43), (0, 0, 36), (0, 0, 30), (2, 0, 31), (2, 0, 23), (2, 0, 15), (1, 0, 7)), ((0, 0, 127), (0, 0, 123), (0, 0, 127), (0, 0, 119), (0, 0, 111), (0, 0, 107), (0, 0, 109), (0, 3, 121), (0, 0, 114), (0, 0, 106), (0, 0, 98), (0, 0, 90), (0, 0, 82), (0, 0, 82), (0, 0, 74), (0, 0, 84), (0, 0, 76), (0, 0, 68), (0, 0, 60), (0, 0, 56), (0, 0, 54), (0, 0, 44), (0, 0, 42), (0, 1, 48), (0, 0, 40), (0, 0, 32), (0, 0, 24), (0, 0, 22), (0, 0, 14), (1, 0, 6))), 
       shapes=((0, 0, 0, 5, 4), (0, 0, 0, 4, 2)), 
       tags=('before.later.small', 'before.m-1', 'before.m-2', 'before.mod6', 'before.mod7', 'conv.s0.later', 'conv.s0.t0', 'conv.s1.later', 'conv.s2.later', 'conv.s3.later', 'conv.s3.t0', 'marker8.kind0', 'marker8.kind1', 'marker8.kind2', 'marker8.s0', 'marker8.s1', 'marker8.s2', 'marker8.s3', 'unconv.followed', 'unconv.s0')),
    _c(name='prot_m9', P=22, length=120, n=6, marker=9, gen=GEN, pairs=((0, 0), (0, 1)), mt=False, 
       exits=(((0, 0, 135), (0, 3, 136), (0, 3, 128), (0, 3, 120), (0, 3, 116), (0, 3, 115), (0, 3, 109), (0, 3, 103), (0, 3, 99), (0, 3, 109), (0, 2, 99), (0, 0, 88), (0, 3, 85), (0, 3, 83), (0, 3, 77), (0, 3, 82), (0, 3, 74), (0, 3, 68), (0, 0, 60), (0, 3, 57), (0, 3, 53), (0, 3, 47), (0, 3, 43), (0, 0, 45), (0, 3, 36), (0, 3, 30), (2, 3, 31), (2, 3, 23), (2, 1, 15), (1, 0, 6)), ((0, 3, 129), (0, 3, 127), (0, 3, 127), (0, 3, 119), (0, 3, 115), (0, 3, 111), (0, 3, 109), (0, 0, 121), (0, 3, 112), (0, 3, 104), (0, 3, 96), (0, 3, 88), (0, 3, 88), (0, 3, 80), (0, 3, 74), (0, 3, 82), (0, 3, 74), (0, 3, 66), (0, 3, 58), (0, 1, 60), (0, 0, 49), (0, 3, 42), (0, 3, 52), (0, 3, 44), (0, 3, 36), (0, 3, 28), (0, 3, 26), (0, 3, 18), (2, 3, 10), (1, 0, 2))), 
       shapes=((0, 0, 0, 4, 5), (0, 0, 0, 4, 2)), 
       tags=('before.later.k2', 'before.later.small', 'before.mod2', 'before.mod6', 'conv.s0.later', 'conv.s0.t0', 'conv.s1.later', 'conv.s2.later', 'conv.s3.later', 'conv.s3.t0', 'marker9.kind0', 'marker9.kind1', 'marker9.kind2', 'marker9.s0', 'marker9.s1', 'marker9.s2', 'marker9.s3', 'unconv.followed', 'unconv.m+1', 'unconv.s1', 'unconv.s3')),
    _c(name='prot_m1023', P=22, length=400, n=6, marker=1023, gen=GEN, pairs=((0, 0), (0, 1)), xdrop=3000, mt=False, 
       exits=(((1, 0, 834),), ((1, 0, 805),)), 
       shapes=((0, 0, 0, 6, 9), (0, 0, 0, 11, 6)), 
       tags=('before.mod2', 'before.mod5', 'marker1023.kind1', 'marker1023.s0', 'match>128diag')),
    _c(name='prot_m1024', P=22, length=400, n=6, marker=1024, gen=GEN, pairs=((0, 0), (0, 1)), xdrop=3000, mt=False, 
       exits=(((1, 0, 834),), ((1, 0, 805),)), 
       shapes=((0, 0, 0, 6, 9), (0, 0, 0, 11, 6)), 
       tags=('before.mod2', 'before.mod5', 'marker1024.kind1', 'marker1024.s0', 'match>128diag')),
    _c(name='prot_runs_m512', P=22, length=400, n=3, marker=512, gen=GEN, pairs=((7, 0), (7, 1), (7, 2)), cut=((1, 150, 140), (0, 150, 72), (0, 120, 200)), xdrop=3000, mt=False, 
       exits=(((0, 3, 601), (1, 0, 147)), ((0, 3, 630), (1, 0, 213)), ((0, 3, 557), (1, 0, 76))), 
       shapes=((0, 0, 0, 5, 154), (0, 0, 0, 70, 6), (0, 0, 1, 161, 0)), 
       tags=('before.mod3', 'before.mod4', 'before.mod5', 'conv.s3.t0', 'match>128diag', 'run1>=64', 'run2>=128', 'start1')),
]
BY_NAME = {c.name: c for c in CASES}

# Classes searched for and NOT REACHED: tools/find_exit_cases.py rare / err3, 2000 generated pairs per marker (16, 33, 128) and per family
# with one side shortened to 0.6 of its length, 12 000 pairs in all.  A trailing run only ever followed an unconverged exit (kind 2),
# never a converged one, in either direction; no border fill was longer than 64 codes (a walk leaves through the border within a few
# columns of the corner); and no pair ended with errorType 3, whatever the err3_reason (the reason 2 that tools/classify_err3.py finds
# needs the random matrices of the fuzz campaign, not this generator).  A path that starts with code 1 WAS reached (255 of the 12 000 pairs)
# and is in the pools ("start1").  No test depends on the classes below; a case that reaches one fails test_exit_edge_inputs_cpu.py, so that it gets named.
NOT_REACHED: Tuple[str, ...] = ("tail1.short.conv", "tail1.long.conv", "tail2.short.conv", "tail2.long.conv", "fill>64")
