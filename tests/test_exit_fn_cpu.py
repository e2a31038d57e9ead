"""The tile exit and the walk steps that the three DP kernels share (twilight_amd/csrc/talco_exit.hip.h), on the CPU: the header is compiled by g++ into
a small program (tests/exit_kats.cpp) that prints what its functions return; the expected answers are here.  No GPU, no library.

walk_step is held to a table written out from the reference's Traceback (TALCO-XDrop.cpp:134-231), every state and every nibble; tile_exit and
pair_advance to every tile record the oracle's exit hook gives for every pool of exit_cases.CASES; the code-3 exits and the trailing run behind a
converged exit, which no pool reaches (exit_cases.NOT_REACHED), are called directly; border fill, guarded append and the segment copy on small buffers."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dp_cases as D  # noqa: E402
import exit_cases as E  # noqa: E402

K_IB, K_DB = -2, -3      # I_BOUNDARY, D_BOUNDARY (TALCO-XDrop.cpp:33-34)


@pytest.fixture(scope="module")
def kats(tmp_path_factory):
    exe = tmp_path_factory.mktemp("exit_kats") / "exit_kats"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "exit_kats.cpp")])

    def run(*args, stdin=""):
        r = subprocess.run([str(exe)] + [str(a) for a in args], input=stdin, capture_output=True, text=True)
        assert r.returncode == 0, (args, r.stdout, r.stderr)
        return r.stdout.splitlines()
    return run


# (state, nibble) -> (code, next state, d kk, d ii, d qi, d ri), from TALCO-XDrop.cpp:161-217.  In state M the nibble's low two bits choose the move
# (:162-184; 3 falls into the `else` of :176 like 2), and the move's own extend bit (4 for I, 8 for D) the next state; in state I (:186-192) and D
# (:193-200) the move is given and only its extend bit is read.  A match steps two diagonals back (:203-207), I one diagonal and one row (:209-212),
# D one diagonal (:214-216).
WALK = [
    (0, 0, 0, 0, -2, -1, -1, -1), (0, 1, 1, 0, -1, -1, -1, 0), (0, 2, 2, 0, -1, 0, 0, -1), (0, 3, 2, 0, -1, 0, 0, -1), (0, 4, 0, 0, -2, -1, -1, -1), (0, 5, 1, 1, -1, -1, -1, 0), (0, 6, 2, 0, -1, 0, 0, -1), (0, 7, 2, 0, -1, 0, 0, -1),
    (0, 8, 0, 0, -2, -1, -1, -1), (0, 9, 1, 0, -1, -1, -1, 0), (0, 10, 2, 2, -1, 0, 0, -1), (0, 11, 2, 2, -1, 0, 0, -1), (0, 12, 0, 0, -2, -1, -1, -1), (0, 13, 1, 1, -1, -1, -1, 0), (0, 14, 2, 2, -1, 0, 0, -1), (0, 15, 2, 2, -1, 0, 0, -1),
    (1, 0, 1, 0, -1, -1, -1, 0), (1, 1, 1, 0, -1, -1, -1, 0), (1, 2, 1, 0, -1, -1, -1, 0), (1, 3, 1, 0, -1, -1, -1, 0), (1, 4, 1, 1, -1, -1, -1, 0), (1, 5, 1, 1, -1, -1, -1, 0), (1, 6, 1, 1, -1, -1, -1, 0), (1, 7, 1, 1, -1, -1, -1, 0),
    (1, 8, 1, 0, -1, -1, -1, 0), (1, 9, 1, 0, -1, -1, -1, 0), (1, 10, 1, 0, -1, -1, -1, 0), (1, 11, 1, 0, -1, -1, -1, 0), (1, 12, 1, 1, -1, -1, -1, 0), (1, 13, 1, 1, -1, -1, -1, 0), (1, 14, 1, 1, -1, -1, -1, 0), (1, 15, 1, 1, -1, -1, -1, 0),
    (2, 0, 2, 0, -1, 0, 0, -1), (2, 1, 2, 0, -1, 0, 0, -1), (2, 2, 2, 0, -1, 0, 0, -1), (2, 3, 2, 0, -1, 0, 0, -1), (2, 4, 2, 0, -1, 0, 0, -1), (2, 5, 2, 0, -1, 0, 0, -1), (2, 6, 2, 0, -1, 0, 0, -1), (2, 7, 2, 0, -1, 0, 0, -1),
    (2, 8, 2, 2, -1, 0, 0, -1), (2, 9, 2, 2, -1, 0, 0, -1), (2, 10, 2, 2, -1, 0, 0, -1), (2, 11, 2, 2, -1, 0, 0, -1), (2, 12, 2, 2, -1, 0, 0, -1), (2, 13, 2, 2, -1, 0, 0, -1), (2, 14, 2, 2, -1, 0, 0, -1), (2, 15, 2, 2, -1, 0, 0, -1),
]


def test_walk_step_on_every_state_and_nibble(kats):
    got = [tuple(int(x) for x in l.split()) for l in kats("walk")]
    assert len(WALK) == 48 and {(r[0], r[1]) for r in WALK} == {(s, v) for s in range(3) for v in range(16)}
    assert got == WALK


def _exit(kats, *rows):
    """tile_exit + pair_advance per row (conv_logic, last_k, marker, conv_value, refLen, qLen, R, Q, ref_idx, qry_idx) -> dicts."""
    names = ("bad", "conv_r", "conv_q", "tb_state", "start_k", "ended", "adv_bad", "ref_idx", "qry_idx", "last", "tail_dir", "tail_len")
    out = kats("exits", stdin="".join(" ".join(str(int(v)) for v in r) + "\n" for r in rows))
    assert len(out) == len(rows)
    return [dict(zip(names, (int(x) for x in l.split()))) for l in out]


@pytest.mark.parametrize("P", [6, 22])
def test_exit_and_advance_against_every_record_of_every_pool(kats, P):
    cases = [c for c in E.CASES if c.P == P]
    M = D.matrix_of(P)
    jobs = []
    for c in cases:
        b = c.batch()
        jobs += [(c, b, i) for i in range(b.n_pairs)]
    with ThreadPoolExecutor(max_workers=4) as ex:
        res = list(ex.map(lambda j: E.exits_of_pair(j[1], j[2], M, **j[0].params()), jobs))
    rows, want = [], []
    for (c, b, i), (_path, err, recs) in zip(jobs, res):
        assert err == 0 and len(recs) == len(c.exits[i]), (c.name, i)
        R, Q = int(b.len[i, 0]), int(b.len[i, 1])
        ref_idx = qry_idx = 0
        for e in recs:
            conv_value = 0 if e.kind == 1 else (e.state << 16) | e.conv_q      # kind 1 never reads it
            rows.append((e.kind == 0, e.last_k, c.marker, conv_value, R - ref_idx, Q - qry_idx, R, Q, ref_idx, qry_idx))
            start_k = e.last_k if e.kind == 1 else (c.marker - 1 if e.state == 3 else c.marker)      # :625-632, :636-653
            want.append((c.name, i, e.tile, dict(bad=0, conv_r=e.conv_r, conv_q=e.conv_q, tb_state=e.state, start_k=start_k, ended=int(e.kind == 1), adv_bad=0,
                                                 ref_idx=e.ridx, qry_idx=e.qidx, last=int(e.last), tail_dir=e.tail_dir, tail_len=e.tail_len)))
            ref_idx, qry_idx = e.ridx, e.qidx
    got = _exit(kats, *rows)
    wrong = [(w[:3], w[3], g) for w, g in zip(want, got) if w[3] != g]
    assert not wrong, wrong[:5]
    assert len(got) == sum(len(t) for c in cases for t in c.exits) > 0      # the oracle's tile count of the pools: nothing skipped
    assert {0, 1, 2} == {r.kind for _p, _e, recs in res for r in recs} and {0, 1, 2, 3} == {r.state for _p, _e, recs in res for r in recs}


def test_the_code_3_exits(kats):
    """What no pool reaches (exit_cases.NOT_REACHED: errorType-3 exits): a pointer that is unset or a boundary sentinel, a cell in front of the tile,
    an advance that leaves the pair.  Marker 8; the pair 40 x 40 at (10, 10) unless said."""
    row = lambda logic, last_k, value, **kw: (logic, last_k, kw.get("marker", 8), value, 30, 30, kw.get("R", 40), kw.get("Q", 40), kw.get("ref", 10), kw.get("qry", 10))      # noqa: E731
    sentinels = [row(logic, last_k, v) for v in (-1, K_IB, K_DB) for logic, last_k in ((1, 20), (0, 8), (0, 20))]
    for g in _exit(kats, *sentinels):
        assert g["bad"] == 1 and g["tb_state"] > 3, g
    assert _exit(kats, row(1, 20, (4 << 16) | 2))[0]["bad"] == 1      # the first state that is none
    # conv_q beyond the marker: conv_r < 0.  State 3 starts one diagonal earlier, so its limit is one lower.
    g = _exit(kats, row(1, 20, 8), row(1, 20, 9), row(1, 20, (3 << 16) | 7), row(1, 20, (3 << 16) | 8), row(0, 9, (1 << 16) | 9), row(0, 9, (2 << 16) | 8))
    assert [(x["bad"], x["conv_r"]) for x in g] == [(0, 0), (1, -1), (0, 0), (1, -1), (1, -1), (0, 0)]
    assert all(x["adv_bad"] == 0 for x in g if not x["bad"])
    # an advance past R or past Q (conv_r 5, conv_q 3 from (10, 10)): the first position outside is R + 1 / Q + 1
    g = _exit(kats, row(1, 20, 3, R=15), row(1, 20, 3, R=14), row(1, 20, 3, Q=13), row(1, 20, 3, Q=12), row(1, 20, 3, R=14, Q=12))
    assert [(x["bad"], x["adv_bad"]) for x in g] == [(0, 0), (0, 1), (0, 0), (0, 1), (0, 1)]
    assert (g[1]["ref_idx"], g[1]["qry_idx"]) == (15, 13)      # the advance itself is made (the kernels' debug record shows it)
    # before the marker the pair ends in this tile and conv_value is not read
    (g,) = _exit(kats, row(0, 7, -1))
    assert g == dict(bad=0, conv_r=29, conv_q=29, tb_state=0, start_k=7, ended=1, adv_bad=0, ref_idx=39, qry_idx=39, last=1, tail_dir=0, tail_len=0)


def test_a_trailing_run_behind_a_converged_exit(kats):
    """exit_cases.NOT_REACHED tail*.conv: a converged tile (state 0 and 3) whose end cell lies on the pair's last row or column (:671-679)."""
    rows, want = [], []
    for value, conv_r in ((3, 5), ((3 << 16) | 3, 4)):
        ref, qry = 10 + conv_r, 13
        for R, Q, w in ((ref + 1, 33, (1, 1, 33 - qry - 1)), (ref + 1, qry + 2, (1, 1, 1)), (40, qry + 1, (1, 2, 40 - ref - 1)), (ref + 2, qry + 1, (1, 2, 1)),
                        (ref + 1, qry + 1, (1, 0, 0)), (ref + 2, qry + 2, (0, 0, 0)), (40, 33, (0, 0, 0))):
            rows.append((1, 20, 8, value, R - 10, Q - 10, R, Q, 10, 10))
            want.append((0, 0, 0, ref, qry) + w)
    got = _exit(kats, *rows)
    assert [(g["bad"], g["adv_bad"], g["ended"], g["ref_idx"], g["qry_idx"], g["last"], g["tail_dir"], g["tail_len"]) for g in got] == want


CAP = 2 * 1024 + 16      # the kernels' reverse buffer: 2 * kMaxMarker + 16 codes


@pytest.mark.parametrize("ri,qi,codes", [(-1, -1, ""), (0, -1, "2"), (-1, 0, "1"), (29, 39, "2" * 30 + "1" * 40), (69, -1, "2" * 70), (-5, 69, "1" * 70)])
def test_border_fill(kats, ri, qi, codes):
    """:221-230: the reference columns left first (code 2), then the query's (code 1)."""
    n, buf = kats("fill", CAP, ri, qi)
    assert int(n) == len(codes) and buf == codes + "7" * (CAP + 4 - len(codes))


def test_the_guarded_append_and_a_fill_across_the_cap(kats):
    for n0, wrote in ((6, True), (7, True), (8, False), (9, False)):      # cap 8: the last slot is n == cap - 1; at and past the cap nothing is written, and it still counts
        n, buf = kats("append", 8, n0, 1)
        assert int(n) == n0 + 1 and buf == "".join("1" if (wrote and t == n0) else "7" for t in range(12)), (n0, n, buf)
    n, buf = kats("append", 8, 5, 6)
    assert int(n) == 11 and buf == "77777111" + "7777"
    n, buf = kats("fill", 5, 3, 3)
    assert int(n) == 8 and buf == "22221" + "7777"      # n > cap: the kernels end the pair with code 3


@pytest.mark.parametrize("stride", [1, 64, 1024])
def test_emit_segment(kats, stride):
    """The codes reversed, without the first of them for later tiles (:98-102), then the trailing run; whatever the thread count."""
    rev = [t % 3 for t in range(70)]
    for n, skip, tdir, tlen in ((70, 0, 0, 0), (70, 1, 0, 0), (70, 1, 2, 67), (1, 1, 1, 3), (1, 0, 0, 0), (0, 0, 0, 0)):
        pos, out = kats("emit", n, skip, tdir, tlen, stride)
        seg = rev[:n][::-1][skip:]
        want = [9, 9, 9] + seg + [tdir] * tlen
        assert int(pos) == len(want) and out == "".join(str(c) for c in want) + "9" * (n + tlen + 8 - len(want)), (n, skip, tdir, tlen)
