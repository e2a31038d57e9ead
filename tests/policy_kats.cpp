// tests/policy_kats.cpp -- known answers of the re-run ladder (next_rung), of the pass memory (PassMemory::update) and of a tile-parallel level's plan (plan_tile_level),
// which are pure functions in twilight_amd/csrc/twl_policy.inc.hip (no HIP call: this program includes the file directly).  Every expected answer restates the dispatch of
// commit 4533235, twilight_amd/csrc/twl_align.hip (run_device, lines 549-629), read as the specification -- for the tile level, launch_mt of commit 610317e,
// twilight_amd/csrc/twl_launch.inc.hip (lines 209-331); the line it restates is named.  Prints "OK <name>" / "FAIL <name>".
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../twilight_amd/csrc/twl_policy.inc.hip"

static int g_fail = 0;
#define CHECK(name, cond) do { if (cond) printf("OK %s\n", name); else { printf("FAIL %s\n", name); ++g_fail; } } while (0)

static Knobs knobs(int mt_wide = 1) { return Knobs{1024, 512, 70, mt_wide, 0, 0, 0, ProtMode::Auto, 448, 256, 2, 1, 320, 40, 64, 96, 128}; }      // the library's defaults (twl_knobs.inc.hip)

// The rungs a set of `count` pairs of summed length `sumLen` takes when it outgrows every window in turn, after an optional guard round on the first round.
static std::string climb(const Ran &ran, int count, long long sumLen, bool guardFirst, int mt_wide = 1)
{
    std::string s;
    const RedoFacts f{count, sumLen, 1024, false};
    Level at = ran.start;
    if (guardFirst) { const Step g = next_rung(ran, at, RedoKind::Guard, f, knobs(mt_wide)); s += rung_name(g.rung); s += " > "; at = g.next; }
    for (int guard = 0; at != Level::Global && guard < 16; ++guard) {
        const Step st = next_rung(ran, at, RedoKind::Overflow, f, knobs(mt_wide));
        s += rung_name(st.rung); s += " > ";
        at = st.next;
    }
    return s + rung_name(next_rung(ran, at, RedoKind::Overflow, f, knobs(mt_wide)).rung);
}
static Ran nuc(Level start, bool leanMid = true, int mode = 2) { Ran r; r.start = start; r.leanMid = leanMid; r.mode = mode; return r; }

// The plan and the job table of a tile-parallel level at marker 128, sequence capacity 300 (slots = 600 / 127 + 2 = 6: line 228), 12-word tile records (kMtRec, talco_mt.hip.h).
struct Tiles { TilePlan pl; std::vector<int32_t> jobs; };
static Tiles tiles(const std::vector<int32_t> &order, const std::vector<int32_t> &len, const Knobs &k, bool wide = false, bool can_small = false, bool small_tiles = false)
{
    TileFacts f;
    f.wide = wide; f.can_small = can_small; f.small_tiles = small_tiles;
    f.n_run = (int)order.size(); f.marker = 128; f.seq_len = 300; f.rec_words = 12; f.order = order.data(); f.h_len = len.data();
    Tiles t;
    t.pl = plan_tile_level(f, k, t.jobs);
    return t;
}
// n pairs of one tile each (R = Q = 1: line 241 stops at n = 1), in their own order
static Tiles one_tile_pairs(int n, const Knobs &k, bool wide = false)
{
    std::vector<int32_t> order((size_t)n), len(2 * (size_t)n, 1);
    for (int t = 0; t < n; ++t) order[t] = t;
    return tiles(order, len, k, wide);
}
static std::string tile_name(int P, int mm, int tw, int trpl, int stitch_rpl, bool thr, bool smallT)
{
    TileFacts f; f.P = P; f.mm = mm; f.tw = tw; f.trpl = trpl; f.stitch_rpl = stitch_rpl;
    TilePlan pl; pl.thr = thr; pl.smallT = smallT;
    char s[160];      // (Device::kname)
    tile_level_name(s, sizeof s, f, pl);
    return s;
}

int main()
{
    // "few long pairs": 4 pairs of 2 x 10 000 columns at marker 1024 (sumLen 80 000 >= 8 * 1024 * 4: lines 572, 596); "many short": 2000 pairs of 2 x 1600 (more than mt_max_pairs)
    const int FEW = 4, MANY = 2000; const long long FEWLEN = 80000, MANYLEN = 6400000;
    // ---- throughput 512 (thr512, lines 566-582): few long pairs go tile-parallel on the 1024-row stitch (viaMt, 572-576), then the middle rung (593-600), then 4608 (602), then global (639-661)
    CHECK("from512_few_long", climb(nuc(Level::From512), FEW, FEWLEN, false) == "tile-parallel 1024 > tile-parallel 3072 > wide 4608 > global");
    // ... many short pairs: 768 throughput (578-580), then from768 -> 1024 lean (583-587), then the middle rung: too many pairs for tiles -> lean 2048 (599)
    CHECK("from512_many_short", climb(nuc(Level::From512), MANY, MANYLEN, false) == "throughput 768 > lean 1024 > lean 2048 > wide 4608 > global");
    // a guard round first leaves the state as it was (557: --stage; 564-565: from512 / from768 need !guardRound; 588)
    CHECK("from512_guard_first", climb(nuc(Level::From512), MANY, MANYLEN, true) == "guard (IEEE division) > throughput 768 > lean 1024 > lean 2048 > wide 4608 > global");
    CHECK("from512_few_guard_first", climb(nuc(Level::From512), FEW, FEWLEN, true) == "guard (IEEE division) > tile-parallel 1024 > tile-parallel 3072 > wide 4608 > global");
    // TWL_KNOB_MT_WIDE 0 (596: wideMt needs g_mt_wide): the middle rung is the lean 2048-row kernel; the 1024-row stitch of 572 does not ask the knob
    CHECK("from512_few_long_mt_wide_0", climb(nuc(Level::From512), FEW, FEWLEN, false, 0) == "tile-parallel 1024 > lean 2048 > wide 4608 > global");
    // ---- throughput 768 (thr768, 583-587)
    CHECK("from768_few_long", climb(nuc(Level::From768), FEW, FEWLEN, false) == "lean 1024 > tile-parallel 3072 > wide 4608 > global");
    CHECK("from768_many_short", climb(nuc(Level::From768), MANY, MANYLEN, false) == "lean 1024 > lean 2048 > wide 4608 > global");
    CHECK("from768_guard_first_mt_wide_0", climb(nuc(Level::From768), FEW, FEWLEN, true, 0) == "guard (IEEE division) > lean 1024 > lean 2048 > wide 4608 > global");
    // ... of a matrix without the default structure in its one-letter form (mode 5 over mm 1: leanMid false, 405): the middle rung is the 16 x 2 IEEE kernel (601)
    CHECK("from768_mode5_over_mm1", climb(nuc(Level::From768, false, 5), MANY, MANYLEN, false) == "lean 1024 > 16 x 2 IEEE > wide 4608 > global");
    // ---- 1024 lean first launches (16-wave, speculative, throughput of modes 0 / 1) and the tile-parallel first launch: stage 1 is the middle rung (560, 593-601)
    CHECK("mid_few_long", climb(nuc(Level::Mid), FEW, FEWLEN, false) == "tile-parallel 3072 > wide 4608 > global");
    CHECK("mid_many_short", climb(nuc(Level::Mid), MANY, MANYLEN, false) == "lean 2048 > wide 4608 > global");
    CHECK("mid_few_long_mt_wide_0", climb(nuc(Level::Mid), FEW, FEWLEN, false, 0) == "lean 2048 > wide 4608 > global");
    CHECK("mid_guard_first", climb(nuc(Level::Mid), FEW, FEWLEN, true) == "guard (IEEE division) > tile-parallel 3072 > wide 4608 > global");
    // few pairs too short for tiles (596: redoLen >= 3 * marker * n): 4 pairs of 2 x 1000
    CHECK("mid_few_short", climb(nuc(Level::Mid), FEW, 8000, false) == "lean 2048 > wide 4608 > global");
    // ---- wide tile-parallel first (startedWide, 560: "a call that started on the 3072-row geometry goes on to the widest kernel")
    { Ran r = nuc(Level::Wide); r.startedWide = true;
      CHECK("wide_first_few_long", climb(r, FEW, FEWLEN, false) == "wide 4608 > global");
      CHECK("wide_first_many_short_guard_first", climb(r, MANY, MANYLEN, true, 0) == "guard (IEEE division) > wide 4608 > global"); }
    // ---- IEEE general first launch (nucleotide, !lean: leanMid false): 16 x 2 IEEE (601), then 4608
    CHECK("ieee_general_few_long", climb(nuc(Level::Mid, false, 0), FEW, FEWLEN, false) == "16 x 2 IEEE > wide 4608 > global");
    CHECK("ieee_general_many_short_mt_wide_0", climb(nuc(Level::Mid, false, 0), MANY, MANYLEN, false, 0) == "16 x 2 IEEE > wide 4608 > global");
    // ---- protein: the 512-row geometries (protSmall, 376 / 388) have the 16-wave kernel ahead (590); everything else goes straight to 4608 (560: mid needs protSmall)
    { Ran p; p.prot = true; p.mode = 3; p.start = Level::Mid;
      CHECK("protein_512_few_long", climb(p, FEW, FEWLEN, false) == "protein 16-wave > wide 4608 > global");
      CHECK("protein_512_many_short_guard_first", climb(p, MANY, MANYLEN, true) == "guard (IEEE division) > protein 16-wave > wide 4608 > global");
      p.start = Level::Wide;
      CHECK("protein_16wave_few_long", climb(p, FEW, FEWLEN, false, 0) == "wide 4608 > global");
      CHECK("protein_16wave_many_short_guard_first", climb(p, MANY, MANYLEN, true) == "guard (IEEE division) > wide 4608 > global"); }
    // a guard round never moves the ladder (557, 612), wherever it stands
    { bool ok = true; const RedoFacts f{3, 60000, 1024, false};
      for (Level at : {Level::From512, Level::From768, Level::Mid, Level::Wide}) { const Step g = next_rung(nuc(at), at, RedoKind::Guard, f, knobs()); ok = ok && g.rung == Rung::Guard && g.next == at; }
      CHECK("guard_round_keeps_the_level", ok); }
    // the 512-row sample's dump exception (572: !d->dump_on)
    CHECK("from512_dump_no_tiles", next_rung(nuc(Level::From512), Level::From512, RedoKind::Overflow, RedoFacts{FEW, FEWLEN, 1024, true}, knobs()).rung == Rung::Thr768);

    // ---- PassMemory::update (lines 556, 615-629), one case each side of each threshold ----
    const Knobs k = knobs();
    { // rule 1 (615): calls of up to 8 pairs -- the streak goes on when the call started wide or every pair was re-run tile-parallel; else it ends
      PassMemory m; m.wide_streak = 2; Ran r = nuc(Level::Mid); LadderOutcome o; o.redoMt = true; o.relaunched = 8; o.widePairs = 8;
      m.update(r, o, 8, 20000, k); CHECK("streak_goes_on_all_pairs_wide", m.wide_streak == 3);
      o.relaunched = 7; m.update(r, o, 8, 20000, k); CHECK("streak_ends_one_pair_fitted", m.wide_streak == 0);
      m.wide_streak = 2; o.relaunched = 9; m.update(r, o, 9, 20000, k); CHECK("streak_untouched_above_8_pairs", m.wide_streak == 2);
      Ran w = nuc(Level::Wide); w.startedWide = true; m.update(w, LadderOutcome{}, 1, 20000, k); CHECK("streak_goes_on_started_wide", m.wide_streak == 3);
      Ran g = nuc(Level::Mid, false); m.update(g, LadderOutcome{}, 1, 20000, k); CHECK("streak_untouched_other_matrix", m.wide_streak == 3); }
    { // rule 2 (616-619): share of a narrow-first call's pairs that went wide; calls started wide since.  75 % is plan_nucleotide's threshold: 75 / 100 against 74 / 100
      PassMemory m; m.wide_calls = 3; Ran r = nuc(Level::Mid); LadderOutcome o; o.widePairs = 75;
      m.update(r, o, 100, 20000, k); CHECK("wide_share_75", m.last_wide_pct == 75 && m.wide_calls == 0);
      o.widePairs = 74; m.update(r, o, 100, 20000, k); CHECK("wide_share_74", m.last_wide_pct == 74);
      Ran w = nuc(Level::Wide); w.startedWide = true; m.last_wide_pct = 80;
      for (int t = 0; t < 5; ++t) m.update(w, LadderOutcome{}, 100, 20000, k);
      CHECK("wide_calls_count_to_the_6th", m.wide_calls == 5 && m.last_wide_pct == 80); }      // (plan_nucleotide: wide_calls % 6 == 5 probes)
    { // rule 3 (622): any tile computed in line after small tiles takes the pass off the 512-row window
      PassMemory m; m.small_state = 1; Ran r = nuc(Level::Mid); r.smallTiles = true; LadderOutcome o;
      m.update(r, o, 100, 20000, k); CHECK("small_tiles_none_inline", m.small_state == 1);
      o.firstInline = 1; m.update(r, o, 100, 20000, k); CHECK("small_tiles_one_inline", m.small_state == -1);
      PassMemory n; n.small_state = 1; r.smallTiles = false; n.update(r, o, 100, 20000, k); CHECK("inline_without_small_tiles", n.small_state == 1); }
    { // rule 4 (625-629): more than 1 % of a level of short pairs (longestRun <= 4096) outgrew 512 rows, 5 % of long ones
      PassMemory m; Ran r = nuc(Level::From512); LadderOutcome o;
      o.from512Pairs = 10; m.update(r, o, 1000, 3200, k); CHECK("small_1pct_short_fits", m.small_state == 1);
      o.from512Pairs = 11; m.update(r, o, 1000, 3200, k); CHECK("small_above_1pct_short_lost", m.small_state == -1);
      o.from512Pairs = 11; m.update(r, o, 1000, 4096, k); CHECK("small_longest_4096_is_short", m.small_state == -1);
      o.from512Pairs = 11; m.update(r, o, 1000, 4097, k); CHECK("small_longest_4097_is_long", m.small_state == 1);
      o.from512Pairs = 50; m.update(r, o, 1000, 20000, k); CHECK("small_5pct_long_fits", m.small_state == 1);
      o.from512Pairs = 51; m.update(r, o, 1000, 20000, k); CHECK("small_above_5pct_long_lost", m.small_state == -1);
      o.from512Pairs = -1; m.update(r, o, 1000, 3200, k); CHECK("small_nothing_outgrew", m.small_state == 1);
      Ran p = r; p.probed = true; m.small_state = -1; m.update(p, o, 1000, 3200, k); CHECK("small_sample_said_no_keeps_its_verdict", m.small_state == -1);      // (625: probed)
      Knobs k2 = k; k2.thr_small = 2; m.update(r, o, 1000, 3200, k2); CHECK("small_knob_set_nothing_learnt", m.small_state == -1);
      m.update(nuc(Level::From768), o, 1000, 3200, k); CHECK("small_untouched_by_768_levels", m.small_state == -1); }
    { // a level larger than the last forgets (399, 401, 361-362)
      PassMemory m; m.small_state = -1; m.small_last_n = 1000; m.corridor_lost = true; m.corridor_last_n = 50;
      CHECK("small_for_same_or_smaller", m.small_for(1000) == -1 && m.small_for(10) == -1);
      CHECK("small_for_larger_forgets", m.small_for(1001) == 0);
      m.begin_small_level(1001); CHECK("begin_small_level_larger", m.small_state == 0 && m.small_last_n == 1001);
      m.small_state = 1; m.begin_small_level(500); CHECK("begin_small_level_smaller", m.small_state == 1 && m.small_last_n == 500);
      CHECK("corridor_for", m.corridor_lost_for(50) && !m.corridor_lost_for(51));
      m.begin_corridor_level(51); CHECK("begin_corridor_level_larger", !m.corridor_lost && m.corridor_last_n == 51);
      // a guard round after a corridor loses it (556); without a corridor it does not
      Ran p; p.prot = true; p.usedCorridor = true; LadderOutcome o; o.guardRound = true;
      m.update(p, o, 40, 4000, k); CHECK("corridor_lost_by_a_guard_round", m.corridor_lost);
      m.forget_corridor(); p.usedCorridor = false; m.update(p, o, 40, 4000, k); CHECK("no_corridor_nothing_lost", !m.corridor_lost && m.corridor_last_n == 0);
      m.small_state = 1; m.small_last_n = 9; m.forget_small(); CHECK("forget_small", m.small_state == 0 && m.small_last_n == 0); }
    { // the memory as twl_plan_describe's argument carries it
      PassMemory a = memory_from_code(3), b = memory_from_code(1051), c = memory_from_code(100000 * 31 + 1000);
      CHECK("memory_from_code", a.wide_streak == 3 && b.wide_streak == 0 && b.last_wide_pct == 100 && b.wide_calls == 5 && c.small_for(1 << 30) == -1 && c.last_wide_pct == 0); }

    // ---- plan_tile_level (launch_mt of commit 610317e, twl_launch.inc.hip) ----
    { // the job table (232-247): scouts for every boundary s >= 1, then tiles for s >= 0, tile-major over `order`; the third word is the POSITION in `order` (231), not the pair id.
      // pair 5 = (300, 300): 127 n - 1 <= 598 up to n = 4, so 5 tiles; pair 2 = (100, 150): 126 <= 248 but 253 > 248, so 2 (241)
      std::vector<int32_t> len(12, 0); len[10] = len[11] = 300; len[4] = 100; len[5] = 150;
      const Tiles t = tiles({5, 2}, len, k);
      const std::vector<int32_t> want = {5,1,0, 2,1,1, 5,2,0, 5,3,0, 5,4,0,   5,0,0, 2,0,1, 5,1,0, 2,1,1, 5,2,0, 5,3,0, 5,4,0};
      CHECK("tile_slots_segcap_pitch", t.pl.slots == 6 && t.pl.segcap == 272 && t.pl.sp_pitch == 608);      // 228-230
      CHECK("tile_counts_per_pair", t.pl.T == std::vector<int>({5, 2}) && t.pl.maxT == 5 && t.pl.maxRQ == 600);      // 237-243, 294
      CHECK("tile_jobs_tile_major_row_is_position", t.jobs == want && t.pl.nScout == 5 && t.pl.nTile == 7);      // 244-247
      // 249-254, 257: chain [2][6][2] ints, records [2][6][12], segments [2][6][272] bytes, scout paths [2][608], 4 counters + [2][8] ints of frontier, 12 jobs x 3, anchors [2][6]
      CHECK("tile_table_sizes", t.pl.chain_ints == 24 && t.pl.rec_ints == 144 && t.pl.seg_bytes == 3264 && t.pl.spath_ints == 1216 && t.pl.stat_bytes == 32 + 64 &&
                                t.pl.jobs_ints == 36 && t.pl.anchor_ints == 12);
      CHECK("tile_defaults_of_a_small_level", !t.pl.thr && !t.pl.smallT && t.pl.longScouts && t.pl.anchors && t.pl.rounds == 2 && t.pl.tb_groups == 0);      // 277, 216, 279, 256, 263
      // the wide geometry (288-299): no anchors (256), the pair scout keeps (600 >> 3) + 2 groups of the longest pair (298), the shorter margin and lead (279-281)
      const Tiles w = tiles({2, 5}, len, k, true);
      CHECK("tile_wide_pair_scout", w.pl.tb_groups == 77 && !w.pl.anchors && w.pl.anchor_ints == 0 && !w.pl.thr && w.pl.marg == 40 && w.pl.lead2 == 96 &&
                                    w.pl.T == std::vector<int>({2, 5}) && w.jobs[0] == 2 && w.jobs[2] == 0 && w.jobs[3] == 5 && w.jobs[5] == 1); }      // (the rows follow `order`: pair 2 is row 0 here)
    { // the tile count's boundary (241: 127 n - 1 <= R + Q - 2): R + Q = 255 has 253 <= 253 and a third tile, 254 has not; R = Q = 1 is one tile and no scout
      const Tiles a = tiles({0}, {128, 127}, k), b = tiles({0}, {127, 127}, k), c = tiles({0}, {1, 1}, k);
      CHECK("tile_count_255", a.pl.T[0] == 3 && a.pl.nScout == 2 && a.pl.nTile == 3);
      CHECK("tile_count_254", b.pl.T[0] == 2 && b.pl.nScout == 1 && b.pl.nTile == 2);
      CHECK("tile_count_one_no_scout_no_anchors", c.pl.T[0] == 1 && c.pl.nScout == 0 && c.pl.nTile == 1 && k.mt_anchor == 1 && !c.pl.anchors && c.pl.anchor_ints == 0);      // 256: nScout > 0
      Knobs k0 = k; k0.mt_anchor = 0;
      CHECK("tile_anchor_knob_off", !tiles({0}, {128, 127}, k0).pl.anchors && a.pl.anchors); }
    { // the throughput geometry (277: !WIDE && nTile > g_mt_thr_jobs, 256)
      Knobs k0 = k; k0.mt_thr_jobs = 0;
      CHECK("tile_thr_at_the_knob", !one_tile_pairs(256, k).pl.thr);
      CHECK("tile_thr_above_the_knob", one_tile_pairs(257, k).pl.thr);
      CHECK("tile_thr_knob_0", one_tile_pairs(1, k0).pl.thr);
      CHECK("tile_thr_never_wide", !one_tile_pairs(257, k, true).pl.thr && !one_tile_pairs(1, k0, true).pl.thr); }
    { // the longer scouts (279-281: !WIDE && nTile <= 2048 takes the _lat values 64 / 128, else 40 / 96)
      const Tiles a = one_tile_pairs(2048, k), b = one_tile_pairs(2049, k), w = one_tile_pairs(2048, k, true);
      CHECK("tile_long_scouts_2048", a.pl.longScouts && a.pl.marg == 64 && a.pl.lead2 == 128);
      CHECK("tile_long_scouts_2049", !b.pl.longScouts && b.pl.marg == 40 && b.pl.lead2 == 96);
      CHECK("tile_long_scouts_never_wide", !w.pl.longScouts && w.pl.marg == 40 && w.pl.lead2 == 96);
      Knobs ke = k; ke.mt_marg = ke.mt_marg_lat = 50; ke.mt_lead2 = ke.mt_lead2_lat = 100;      // (TWL_KNOB_MT_MARGIN / TWL_KNOB_MT_LEAD2 set both kinds)
      const Tiles c = one_tile_pairs(2048, ke), e = one_tile_pairs(2049, ke);
      CHECK("tile_long_scouts_knob_set_both", c.pl.marg == 50 && e.pl.marg == 50 && c.pl.lead2 == 100 && e.pl.lead2 == 100); }
    { // rounds (263: clamped to [1, 7]: 1 + 2 * 7 launches on 16 work counters)
      Knobs k0 = k, k9 = k; k0.mt_rounds = 0; k9.mt_rounds = 9;
      CHECK("tile_rounds_clamped", one_tile_pairs(1, k0).pl.rounds == 1 && one_tile_pairs(1, k).pl.rounds == 2 && one_tile_pairs(1, k9).pl.rounds == 7); }
    { // tiles on the 512-row window (215-216: kCanSmall && small_tiles; kCanSmall is P == 6 && TW == 4 && !WIDE, so the protein instantiation passes false whatever the caller says)
      CHECK("tile_small_needs_both", tiles({0}, {1, 1}, k, false, true, true).pl.smallT && !tiles({0}, {1, 1}, k, false, true, false).pl.smallT &&
                                     !tiles({0}, {1, 1}, k, false, false, true).pl.smallT); }
    // the kernel name (284-286), literally: throughput with small tiles (nucleotide, mode 5), throughput (protein 8 x 1, mode 4), and the 16-wave geometries (wide: 3 blocks per wave)
    CHECK("tile_name_thr_small", tile_name(6, 5, 4, 3, 1, true, true) == "talco_lean_kernel<6, 4, 2, 5, 5, false, false, 2 / 1> + <6, 16, 1, 5, 1, false, false, 3> (tile-parallel: scouts, tiles, stitch)");
    CHECK("tile_name_thr", tile_name(22, 4, 8, 1, 1, true, false) == "talco_lean_kernel<22, 8, 1, 4, 4, false, false, 2 / 1> + <22, 16, 1, 4, 1, false, false, 3> (tile-parallel: scouts, tiles, stitch)");
    CHECK("tile_name_16_waves", tile_name(6, 2, 4, 3, 3, false, true) == "talco_lean_kernel<6, 16, 3, 2, 1, false, false, 2 / 1 / 3> (tile-parallel: scouts, tiles, stitch)");
    return g_fail ? 1 : 0;
}
