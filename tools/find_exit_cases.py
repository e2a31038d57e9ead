#!/usr/bin/env python3
"""Search for the pools of tests/exit_cases.py on the CPU oracle and print them as constants.  Not part of the suite.

    python tools/find_exit_cases.py survey  [--P 6]      greedy cover of the converged / unconverged classes over seeds at one marker
    python tools/find_exit_cases.py singles [--P 6]      single-tile pairs with R + Q - 2 around the marker, every residue of last_k mod 8
    python tools/find_exit_cases.py tails   [--P 6]      one side shortened: trailing runs, paths that start with a gap code
    python tools/find_exit_cases.py later   [--P 6]      a later tile with a tiny remainder
    python tools/find_exit_cases.py small   [--P 6]      markers 2, 3, 7, 8, 9 on 120-column pairs, 1023 / 1024 on long ones
    python tools/find_exit_cases.py runs    [--P 6]      a block of columns cut from one side: long runs of a gap code inside one tile
    python tools/find_exit_cases.py rare    [--P 6]      the classes that may be declared not reached (2000 pairs per marker 16, 33, 128)
    python tools/find_exit_cases.py err3    [--P 6]      ... and errorType 3 by err3_reason over the same pairs

Every line printed is an `_c(...)` of exit_cases.CASES with the oracle's exits, shapes and tags.  The committed pools were made with
`--xdrop 3000` (the pools of long pairs: at the default X-drop of 5000 their bands outgrow 512 rows) and 40 seeds; the protein survey
needed `--seeds 160` for a converged exit in state 2 on tile 0."""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import exit_cases as E  # noqa: E402

GEN = E.GEN
NV_MIN = 8      # the smallest window of the routes (512 rows)


def complete(case: E.ExitCase):
    """The case with the oracle's constants filled in, or None when a pair fails, leaves the smallest window or is too long."""
    b = case.batch()
    res = case.compute(b)
    if any(err != 0 or tr.span >= NV_MIN for _p, err, _r, _t, tr in res) or int(b.len.max()) > 1.06 * case.length:
        return None
    kw = dict(case.__dict__)
    kw["exits"] = tuple(tuple(e.key for e in recs) for _p, _e, recs, _t, _tr in res)
    kw["shapes"] = tuple(E.shape_of(recs) for _p, _e, recs, _t, _tr in res)
    kw["tags"] = tuple(sorted(set().union(*[t for _p, _e, _r, t, _tr in res])))
    kw["mt"] = case.marker >= 64 and int(b.len.sum()) >= 3 * case.marker * b.n_pairs
    return E.ExitCase(**kw)


def show(case: E.ExitCase):
    f = [f"name={case.name!r}", f"P={case.P}", f"length={case.length}", f"n={case.n}", f"marker={case.marker}",
         "gen=GEN", f"pairs={case.pairs!r}"]
    for k in ("trim", "cut", "xdrop"):
        if getattr(case, k) is not None:
            f.append(f"{k}={getattr(case, k)!r}")
    f += [f"mt={case.mt!r}", f"\n       exits={case.exits!r}", f"\n       shapes={case.shapes!r}", f"\n       tags={case.tags!r}"]
    print("    _c(" + ", ".join(f) + "),", flush=True)


XDROP = None      # --xdrop: the X-drop of the pools of long pairs (the default's band outgrows 512 rows at these mutation rates)


def base(name, P, length, n, marker, pairs, gen=GEN, **kw):
    if length > 200 and XDROP is not None:
        kw.setdefault("xdrop", XDROP)
    return E.ExitCase(name=name, P=P, length=length, n=n, marker=marker, gen=gen, pairs=tuple(pairs), **kw)


def per_pair_tags(case):
    """[(pair index in the case, tags, span, err)]"""
    res = case.compute()
    return [(i, t, tr.span, err) for i, (_p, err, _r, t, tr) in enumerate(res)]


def cover(name, P, length, marker, seeds, want, n=6, gen=GEN, trims=None):
    """Greedy: pairs over `seeds` until every tag of `want` is held.  Returns the picks [((seed, pair), trim)]."""
    want = set(want)
    picks = []
    for seed in seeds:
        if not want:
            break
        tr = trims(seed, n, P, length, gen) if trims else None
        c = base(name, P, length, n, marker, [(seed, i) for i in range(n)], gen=gen, trim=tr)
        for i, t, span, err in per_pair_tags(c):
            if err == 0 and span < NV_MIN and (t & want):
                picks.append(((seed, i), tr[i] if tr else None))
                print(f"# {name} seed {seed} pair {i}: {sorted(t & want)}", file=sys.stderr, flush=True)
                want -= t
    print(f"# {name}: not found {sorted(want)}", file=sys.stderr, flush=True)
    return picks


def pools(name, P, length, marker, picks, n=6, gen=GEN):
    """The picks as pools of 2 to 6 pairs."""
    chunks = [picks[i:i + 6] for i in range(0, len(picks), 6)]
    if chunks and len(chunks[-1]) == 1:
        if len(chunks) > 1:
            chunks[-1].insert(0, chunks[-2].pop())
        else:
            (seed, i), tr = chunks[-1][0]
            chunks[-1].append(((seed, (i + 1) % n), tr))
    for k, ch in enumerate(chunks):
        trim = tuple(tr for _p, tr in ch)
        c = complete(base(f"{name}_{k}" if len(chunks) > 1 else name, P, length, n, marker, [p for p, _tr in ch], gen=gen,
                          trim=trim if any(t is not None for t in trim) else None))
        assert c is not None, (name, ch)
        show(c)


def lens_of(P, length, n, seed, gen):
    from twilight_amd import synth
    return synth.make_level_batch(n, length, P=P, seed=seed, **dict(gen)).len


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what")
    ap.add_argument("--P", type=int, default=6)
    ap.add_argument("--marker", type=int, default=128)
    ap.add_argument("--seeds", type=int, default=40)
    ap.add_argument("--xdrop", type=int, default=None)
    a = ap.parse_args()
    global XDROP
    XDROP = a.xdrop
    P, m = a.P, a.marker
    fam = "nuc" if P == 6 else "prot"
    length = 700 if P == 6 else 400
    if a.what == "survey":
        want = [f"conv.s{s}.{w}" for s in range(4) for w in ("t0", "later")] + [f"unconv.s{s}" for s in range(4)] + \
               ["unconv.m+0", "unconv.m+1", "unconv.m+2", "unconv.followed", "before.m-1", "before.m-2"]
        pools(f"{fam}_m{m}", P, length, m, cover(f"{fam}_m{m}", P, length, m, range(a.seeds), want))
    elif a.what == "singles":
        # R + Q - 2 = last_k for a pair of one tile: every residue below the marker, and the five ends of the phases
        ks = list(range(m - 8, m + 3))
        for part, chunk in enumerate((ks[:6], ks[6:])):
            half = (m + 4) // 2 + 4
            for seed in range(a.seeds):
                ln = lens_of(P, half, len(chunk), seed, GEN)
                trim = tuple(((k + 2 + 1) // 2, (k + 2) // 2) for k in chunk)
                if any(t[0] > ln[i, 0] or t[1] > ln[i, 1] for i, t in enumerate(trim)):
                    continue
                c = complete(base(f"{fam}_single{part}_m{m}", P, half, len(chunk), m, [(seed, i) for i in range(len(chunk))], trim=trim))
                if c is not None and all(len(x) == 1 and x[0][2] == k for x, k in zip(c.exits, chunk)):
                    show(c)
                    break
    elif a.what == "tails":
        picks = []
        for frac, label in ((0.6, "long"), (0.97, "short")):
            for side in (0, 1):
                def trims(seed, n, P_, length_, gen, side=side, frac=frac):
                    ln = lens_of(P_, length_, n, seed, gen)
                    return tuple((int(l[0] * frac), int(l[1])) if side == 0 else (int(l[0]), int(l[1] * frac)) for l in ln)
                # (a shortened reference leaves query columns behind the last tile: code 1)
                want = [f"tail{side + 1}.{label}.unconv"] + (["start2", "start1"] if (frac, side) == (0.6, 0) else [])
                picks += cover(f"{fam}_tail_{label}{side}_m{m}", P, length, m, range(a.seeds), want, trims=trims)
        pools(f"{fam}_tails_m{m}", P, length, m, picks)
    elif a.what == "later":
        # a multi-tile pair trimmed to end a few cells behind a tile's end cell
        best = None
        for seed in range(a.seeds):
            res = base("x", P, length, 3, m, [(seed, i) for i in range(3)]).compute()
            ln = lens_of(P, length, 3, seed, GEN)
            for i, (_p, err, recs, _t, tr) in enumerate(res):
                if err or tr.span >= NV_MIN or len(recs) < 3:
                    continue
                e = recs[len(recs) // 2]
                for dr, dq in ((2, 2), (2, 3), (3, 2), (3, 3)):
                    j = (i + 1) % 3
                    c = complete(base(f"{fam}_later_m{m}", P, length, 3, m, [(seed, i), (seed, j)],
                                      trim=((e.ridx + dr, e.qidx + dq), (int(ln[j, 0]), int(ln[j, 1])))))
                    if c is not None and "before.later.small" in c.tags:
                        if "before.later.k2" in c.tags:
                            show(c)
                            return
                        best = best or c
        if best is not None:
            show(best)
    elif a.what == "small":
        for mk in (2, 3, 7, 8, 9):
            pools(f"{fam}_m{mk}", P, 120, mk, cover(f"{fam}_m{mk}", P, 120, mk, range(a.seeds), [f"marker{mk}.{x}" for x in ("kind0", "kind2", "s0", "s3", "s1", "s2", "kind1")]))
        for mk in (1023, 1024):
            pools(f"{fam}_m{mk}", P, length, mk, cover(f"{fam}_m{mk}", P, length, mk, range(min(a.seeds, 10)), [f"marker{mk}.{x}" for x in ("kind0", "kind2", "kind1", "s0", "s3")]))
    elif a.what == "runs":
        mk = 512
        for seed in range(a.seeds):
            cut = ((1, 150, 140), (0, 150, 72), (0, 120, 200))
            c = complete(base(f"{fam}_runs_m{mk}", P, length, 3, mk, [(seed, i) for i in range(3)], cut=cut))
            if c is not None and {"run1>=64", "run2>=128", "match>128diag"} <= set(c.tags):
                show(c)
                return
    elif a.what == "rare":
        # 2000 generated pairs per marker with one side shortened to 0.6 of its length
        want = {"tail1.short.conv", "tail1.long.conv", "tail2.short.conv", "tail2.long.conv", "start1", "fill>64"}
        seen = set()
        for mk in (16, 33, 128):
            pairs = 0
            seed = 0
            while pairs < 2000:
                side = seed & 1
                ln = lens_of(P, length, 8, seed, GEN)
                trim = tuple((int(l[0] * 0.6), int(l[1])) if side == 0 else (int(l[0]), int(l[1] * 0.6)) for l in ln)
                case = base("rare", P, length, 8, mk, [(seed, j) for j in range(8)], trim=trim)
                b = case.batch()
                for i in range(8):      # (the exit records alone: no band trace, these pairs go to no route)
                    path, err, recs = E.exits_of_pair(b, i, E.D.matrix_of(P), **case.params())
                    t = E.tags_of(mk, int(b.len[i, 0]), int(b.len[i, 1]), recs, path) if err == 0 else set()
                    if err == 0 and (t & want):
                        seen |= t & want
                        print(f"# marker {mk} seed {seed} pair {i} (side {side}): {sorted(t & want)}", flush=True)
                pairs += 8
                seed += 1
            print(f"# marker {mk}: {pairs} pairs, reached so far {sorted(seen)}", flush=True)
        print(f"# not reached: {sorted(want - seen)}")
    elif a.what == "err3":
        # the same 2000 pairs per marker through the batch form: errorType 3 by err3_reason (0: none ended that way)
        import oracle_lib as O
        for mk in (16, 33, 128):
            reasons = {}
            for seed in range(250):
                side = seed & 1
                ln = lens_of(P, length, 8, seed, GEN)
                trim = tuple((int(l[0] * 0.6), int(l[1])) if side == 0 else (int(l[0]), int(l[1] * 0.6)) for l in ln)
                case = base("err3", P, length, 8, mk, [(seed, j) for j in range(8)], trim=trim)
                _a, _n, err, st = O.align_batch(O.make_params(E.D.matrix_of(P), **case.params()), case.batch(), threads=8)
                if (err == 3).any():
                    reasons[int(st.err3_reason)] = reasons.get(int(st.err3_reason), 0) + int((err == 3).sum())
                    print(f"# marker {mk} seed {seed}: errorType {err.tolist()} reason {st.err3_reason}", flush=True)
            print(f"# marker {mk}: 2000 pairs, errorType 3 by reason {reasons}", flush=True)
    else:
        raise SystemExit(a.what)


if __name__ == "__main__":
    main()
