"""`--adjust-direction` where it needs no device: the restatement (tests/strand_oracle.py) against its own definition and against the planted
strands of the three fixtures, the host steps and the pure checks against their known answers (g++ alone), the calls and the command line
where they refuse before any device work, and the build.  Every test fails on a tree without the feature.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import guide_oracle as G
import strand_cases as SC
import strand_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "twilight_amd", "csrc")
EXE = os.path.join(ROOT, "twilight_amd", "twilight-mi355x")


# ---- the restatement ----

def test_rc_bin_is_the_code_of_the_reverse_complement():
    letters = "ACGT"
    rng = np.random.default_rng(1)
    for b in [0, 1, 4095, 1234] + [int(x) for x in rng.integers(0, 4096, 40)]:
        kmer = "".join(letters[(b // 4 ** (5 - k)) % 4] for k in range(6))
        rc = SO.reverse_complement(kmer.encode()).decode()
        assert SO.rc_bin(b) == sum(letters.index(c) * 4 ** (5 - k) for k, c in enumerate(rc)), kmer
    p = SO.perm()
    assert sorted(p.tolist()) == list(range(4096)) and (p[p] == np.arange(4096)).all()
    assert SO.rc_bin(-1) == -1 and SO.rc_bin(4096) == -1


@pytest.mark.parametrize("case", ["random", "with_N", "short", "empty", "homopolymer", "lower_and_iupac", "rna"])
def test_the_counts_of_a_reverse_complement_are_the_permuted_counts(case):
    rng = np.random.default_rng(7)
    rnd = bytes(rng.choice(list(b"ACGT"), 500).tolist())
    seq = {"random": rnd, "with_N": rnd[:100] + b"NNN" + rnd[100:200] + b"N" + rnd[200:207] + b"RY" + rnd[207:], "short": b"ACGTA", "empty": b"",
           "homopolymer": b"A" * 70000 + rnd[:50], "lower_and_iupac": rnd[:200].lower() + b"KMBVDHSW" + rnd[200:300], "rna": rnd.replace(b"T", b"U")}[case]
    fwd, rev = G.kmer_counts(seq, "n"), G.kmer_counts(SO.reverse_complement(seq), "n")
    assert (rev == fwd[SO.perm()]).all()
    if case == "homopolymer":
        assert fwd.max() == 65535 and rev[4095] == 65535      # saturation is symmetric under the permutation
    if case in ("short", "empty"):
        assert fwd.sum() == 0
    assert SO.reverse_complement(SO.reverse_complement(seq)) == seq


def test_the_text_reverse_complement():
    rc = SO.reverse_complement
    assert rc(b"AACG") == b"CGTT" and rc(b"RYKMBVDH") == b"DHBVKMRY" and rc(b"SWN-.*X") == b"X*.-NWS" and rc(b"acgtRyKm") == b"kMrYacgt"
    assert rc(b"AACGU") == b"ACGUU" and rc(b"aacgu") == b"acguu" and rc(b"AUT") == b"AUT" and rc(b"AAN") == b"NTT"


def test_the_default_number_of_seeds():
    assert [SO.default_seeds(n, n) for n in (1, 2, 20, 200, 1 << 20)] == [1, 2, 9, 29, 2048]
    assert SO.default_seeds(579, 479) == 49 and SO.default_seeds(1 << 20, 100) == 100 and SO.default_seeds(1 << 40, 1 << 40) == 16384


def test_opposite_counts_are_the_cross_block_of_the_doubled_family():
    rng = np.random.default_rng(3)
    seqs = [bytes(rng.choice(list(b"ACGT"), int(rng.integers(50, 300))).tolist()) for _ in range(12)] + [b"ACG", b"ACGTNNACGTACGTAAC"]
    counts = G.counts_matrix(seqs, "n")
    both = G.shared_counts(G.counts_matrix(seqs + [SO.reverse_complement(s) for s in seqs], "n"))
    n = len(seqs)
    Ox = SO.opposite_counts(counts)
    assert (Ox == both[:n, n:]).all() and (Ox == Ox.T).all()


# ---- the fixtures: the oracle's directions are the planted ones ----

@pytest.mark.parametrize("s", [None, 8, 200])
def test_rnasim_200_planted_directions(s):
    _, _, planted, want = SC.rnasim200()
    assert s is not None or SO.default_seeds(200, 200) == 29
    assert int((SO.directions(planted, s) != want).sum()) == 0


def test_sars_20_planted_directions():
    _, _, planted, want = SC.sars20()
    assert SO.default_seeds(20, 20) == 9
    assert int((SO.directions(planted) != want).sum()) == 0


def test_placement_fixture_planted_directions():
    backbone, _, _, planted, want = SC.placement()
    assert SO.default_seeds(479 + 100, 479) == 49
    assert int((SO.directions_on_backbone(SC.degapped(backbone), planted) != want).sum()) == 0


def test_an_unplanted_family_stays_forward():
    _, seqs, _, _ = SC.rnasim200()
    assert int(SO.directions(seqs).sum()) == 0


# ---- the host steps and the pure checks, g++ alone ----

def _kats(tmp_path, name, flags=()):
    exe = tmp_path / name
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *flags, "-o", str(exe), os.path.join(ROOT, "tests", name + ".cpp")])
    return str(exe)


def _lines(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.splitlines()


def test_host_steps_known_answers(tmp_path):
    lines = _lines(_kats(tmp_path, "strand_kats"))
    assert not [l for l in lines if l.startswith("FAIL")] and len([l for l in lines if l.startswith("OK")]) == 24, lines


def test_the_one_link_per_seed_form_is_the_naive_form(tmp_path):
    """300 matrices of numbers below 4, full of ties: strand::seedFlips (one best link per outside seed) against the walk over all links."""
    x = [12345]

    def draw(mod):
        x[0] = (x[0] * 1103515245 + 12345) & 0x7FFFFFFF
        return (x[0] >> 16) % mod

    want = []
    for k in range(300):
        S = 2 + k % 9
        F, R = np.zeros((S, S), dtype=np.int64), np.zeros((S, S), dtype=np.int64)
        for u in range(S):
            for v in range(u, S):
                F[u][v] = F[v][u] = draw(4) * 2 if u == v else draw(4)
                R[u][v] = R[v][u] = draw(4)
        want.append("R " + "".join(str(int(f)) for f in SO.seed_flips(F, R)))
    got = _lines(_kats(tmp_path, "strand_kats"), "random")
    assert got == want
    assert len({l for l in got}) > 50


def test_plan_known_answers(tmp_path):
    lines = _lines(_kats(tmp_path, "strand_plan_kats"))
    assert not [l for l in lines if l.startswith("FAIL")] and len([l for l in lines if l.startswith("OK")]) == 28, lines


def test_every_refusal_is_written_in_the_plan_file():
    host = open(os.path.join(CSRC, "twl_strand.inc.hip")).read()
    plan = open(os.path.join(CSRC, "twl_strand_plan.inc.hip")).read()
    for message in ("the strand calls work on a set of nucleotide sequences", "the number of ids must be between 1 and 16384", "id out of range", "the same sequence is listed twice",
                    "the number of seeds must be between 1 and 16384", "seed id out of range", "the same sequence is a seed twice", "a seed's flip must be 0 or 1"):
        assert message in plan and message not in host, message
    for call in ("hipMalloc", "hipMemcpy", "hipLaunch", "<<<"):
        assert call not in plan, call


# ---- the library and its binding ----

def test_rc_bin_of_the_library_needs_no_device(built):
    from twilight_amd import strand

    assert [strand.rc_bin(b) for b in range(4096)] == SO.perm().tolist()
    assert strand.rc_bin(-1) == -1 and strand.rc_bin(4096) == -1


def test_the_calls_refuse_a_null_set_before_any_device_work(built):
    import twilight_amd as twl
    from twilight_amd import strand

    lib = strand._lib()
    a = np.zeros(4, dtype=np.int32)
    p = lambda v: v.ctypes.data_as(C.c_void_p)
    for rc in (lib.twl_guide_set_opposite(None, C.c_int32(1), p(a), p(a)), lib.twl_guide_set_strand_assign(None, C.c_int32(1), p(a), p(a), p(a), p(a), None),
               lib.twl_guide_set_strand_timing(None, None, None, None, None)):
        with pytest.raises(twl.TwlError, match="bad argument"):
            twl.api._check(rc)


def test_header_binding_and_library_name_the_same_symbols(built):
    from twilight_amd import api, strand

    header = open(os.path.join(ROOT, "include", "twl_strand.h")).read()
    lib = api.load_library()
    for name in strand.exported_symbols():
        assert name + "(" in header and hasattr(lib, name), name
    assert len(strand.exported_symbols()) == 4


def test_the_new_files_are_kernel_sources_and_built():
    import __graft_entry__ as g

    for f in ("strand_kernels.hip.h", "twl_strand.inc.hip", "twl_strand_plan.inc.hip"):
        assert f in g.KERNEL_SOURCES
    assert '#include "twl_strand.inc.hip"' in open(os.path.join(CSRC, "twl_align.hip")).read()
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert '"strand.cpp"' in entry and '"strand_orient.hpp"' in entry and '"twl_strand.h"' in entry


def test_the_guide_kernels_are_untouched():
    """The strand kernels sit in a file of their own; the guide kernels' files carry no word of them."""
    for f in ("guide_kernels.hip.h", "guide_stage_kernels.hip.h"):
        assert "strand" not in open(os.path.join(CSRC, f)).read()


# ---- the command line, before a device is opened ----

def _cli(*args, timeout=60):
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=timeout)


def _refused(r, *words):
    assert r.returncode == 1, r.stderr
    for w in words:
        assert w in r.stderr, (w, r.stderr)
    assert "twl_init" not in r.stderr and "usage:" not in r.stderr and "unsupported option" not in r.stderr, r.stderr


def _fasta(tmp_path, n=5, name="s.fa"):
    fa = tmp_path / name
    fa.write_text("".join(">s%d\nACGTACGTACGGTCA%s\n" % (i, "ACGT"[i % 4] * 3) for i in range(n)))
    return str(fa)


def test_usage_names_the_flags(built):
    r = _cli()
    assert r.returncode == 1 and "--adjust-direction [--direction-seeds S] [--write-directions <file>]" in r.stderr and "_R_<name>" in r.stderr


@pytest.mark.parametrize("value", ["0", "x", "16385", "-4", "12x", ""])
def test_refuses_a_bad_number_of_seeds_at_parse_time(built, tmp_path, value):
    r = _cli("-i", str(tmp_path / "none.fa"), "-o", str(tmp_path / "o.aln"), "--adjust-direction", "--direction-seeds", value)
    _refused(r, "--direction-seeds needs a number of seeds from 1 to 16384", "(got %s)" % value)
    assert "open" not in r.stderr


@pytest.mark.parametrize("flags", [("--direction-seeds", "4"), ("--write-directions", "d.tsv")])
def test_refuses_the_companions_without_the_flag(built, tmp_path, flags):
    r = _cli("-i", _fasta(tmp_path), "-o", str(tmp_path / "o.aln"), "--type", "n", *flags)
    _refused(r, "apply to a run with --adjust-direction")


def test_refuses_the_modes_it_does_not_cover(built, tmp_path):
    fa, o = _fasta(tmp_path), str(tmp_path / "o.aln")
    _refused(_cli("-f", str(tmp_path), "-o", o, "--adjust-direction"), "--adjust-direction cannot be combined with -f")
    _refused(_cli("-t", "x.nwk", "-a", "x.aln", "-i", fa, "-o", o, "--place-on-tree", "--adjust-direction"), "not available with --place-on-tree")
    _refused(_cli("-t", "x.nwk", "-i", fa, "-o", o, "--host-staged", "--adjust-direction"), "--host-staged is not available with --adjust-direction")
    _refused(_cli("-t", "x.nwk", "-i", fa, "-o", o, "--gpu-index", "0,1", "--adjust-direction"), "--adjust-direction runs on one GPU")
    assert not os.path.exists(o)


def test_refuses_proteins_given_or_detected(built, tmp_path):
    fa, o = _fasta(tmp_path), str(tmp_path / "o.aln")
    _refused(_cli("-i", fa, "-o", o, "--type", "p", "--adjust-direction"), "applies to nucleotide sequences")
    prot = tmp_path / "p.fa"
    prot.write_text(">a\nMKVLEEFQIL\n>b\nMKVLEEFQIP\n")
    _refused(_cli("-i", str(prot), "-o", o, "--adjust-direction"), "reads as protein")
    assert not os.path.exists(o)


def test_refuses_more_seeds_than_sequences_after_reading(built, tmp_path):
    fa = _fasta(tmp_path, 5)
    _refused(_cli("-i", fa, "-o", str(tmp_path / "o.aln"), "--type", "n", "--adjust-direction", "--direction-seeds", "6"), "--direction-seeds 6 is more than the 5 sequences")
    bb = tmp_path / "bb.aln"
    bb.write_text(">b0\nACGT-ACGTACGGTCA\n>b1\nACGTTACGTACGGTCA\n")
    _refused(_cli("-a", str(bb), "-i", fa, "-o", str(tmp_path / "o.aln"), "--type", "n", "--adjust-direction", "--direction-seeds", "3"),
             "--direction-seeds 3 is more than the 2 rows of the backbone")
    assert not (tmp_path / "o.aln").exists()


def test_refuses_more_than_two_to_the_twentieth_sequences(built, tmp_path):
    fa = tmp_path / "many.fa"
    fa.write_text("".join(">%x\nA\n" % i for i in range((1 << 20) + 1)))
    _refused(_cli("-i", str(fa), "-o", str(tmp_path / "o.aln"), "--type", "n", "--adjust-direction"), "at most 1048576 sequences", "holds 1048577")
    assert not (tmp_path / "o.aln").exists()


def test_checker_binary_rejects_the_option(built, tmp_path):
    exe = os.path.join(ROOT, "oracle", "twilight-cpucheck")
    r = subprocess.run([exe, "-t", "x.nwk", "-i", "x.fa", "-o", str(tmp_path / "o.aln"), "--adjust-direction"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "unsupported option --adjust-direction" in r.stderr
