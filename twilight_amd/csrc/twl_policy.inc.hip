// twilight_amd/csrc/twl_policy.inc.hip -- the launch policy of a DP call as PURE functions of the call's facts: the first launch (plan_nucleotide, plan_protein), the rung a set of
// outgrown pairs takes next (next_rung), what a device remembers of a pass (PassMemory) and what a tile-parallel level launches on which tables (plan_tile_level).  No HIP call
// in this file: twl_plan_describe prints the plans without a device (tests/test_policy_cpu.py), tests/policy_kats.cpp includes the file directly for the ladder, the memory and
// the tile level.  Included by twl_align.hip (one translation unit).
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

// TWL_KNOB_PROT_MODE: auto | dense | sparse | presim | r1 (round-1 kernels) | lean_sparse | lean_presim
enum class ProtMode { Auto, Dense, Sparse, Presim, R1, LeanSparse, LeanPresim };
struct Knobs {
    int mt_max_pairs, mt_min_marker, mt_tail_pct, mt_wide, assume_onehot_query, no_spec, thr_small; ProtMode prot_mode; int prot_corridor;
    int mt_thr_jobs, mt_rounds, mt_anchor, mt_lead, mt_marg, mt_marg_lat, mt_lead2, mt_lead2_lat;      // of a tile-parallel level (plan_tile_level)
};
// fast_div's guard (talco_div.hip.h): non-zero scores within [2^-10, 2^10]; anything else takes the IEEE-division kernel
inline bool fast_div_in_range(const float *M, int n, float gap_char)
{
    auto inRange = [](float x) { const float ax = std::fabs(x); return x == 0.0f || (ax >= 0.0009765625f && ax <= 1024.0f); };
    bool ok = inRange(gap_char);
    for (int t = 0; t < n; ++t) ok = ok && inRange(M[t]);
    return ok;
}

// ---- what ran first (the steps of run_device share it), and what a device remembers of a pass ----
enum class Level { From512, From768, Mid, Wide, Global };      // where the re-run ladder stands: the window class of what ran last
struct Ran {
    bool prot = false;
    Level start = Level::Wide;            // window class of the first launch: 512- / 768-row throughput, a 1024-row geometry (protein: 512) with the middle rungs ahead, or straight on to the widest kernel
    int mode = -1, spec = 0;              // twl_stats: matrix_mode (5: one-letter query rows), speculative (1 teams of 16 waves, 2 shared teams, 3 tile-parallel)
    bool leanMid = false;                 // nucleotide, round-2 kernels, default matrix structure: the middle rung is tile-parallel 3072 / lean 2048
    bool startedWide = false;             // the first launch was the 3072-row tile-parallel geometry
    bool ranMt = false;                   // a tile-parallel launch was part of the first launch (its counters are collected)
    bool smallTiles = false;              // the tile jobs of a tile-parallel launch of this call ran on the 512-row window
    bool probed = false;                  // the level's own sample kept the level off the 512-row window (and set the memory of it)
    bool usedCorridor = false;            // protein: the scores of this call were precomputed in a corridor only
};
struct LadderOutcome {
    int relaunched = 0, widePairs = 0;    // pairs re-run by the ladder (all rungs); pairs that went on to the wide window (middle rung)
    int from512Pairs = -1;                // pairs of a 512-row throughput launch that outgrew it (-1: no such launch)
    bool redoMt = false, guardRound = false;      // a re-run went through the tile-parallel path; a guard round was needed
    unsigned long long firstInline = 0;   // tiles the FIRST launch's stitch kernel computed in line (mt_stat[1])
};
struct PassMemory {
    int wide_streak = 0;                            // consecutive small calls whose pairs all outgrew the fast window (plan_nucleotide: wideFirst)
    int last_wide_pct = 0, wide_calls = 0;          // share of the last narrow-first call's pairs that went on to the wide window; calls started wide since
    int small_state = 0, small_last_n = 0;          // what the levels of short pairs of this pass found of the 512-row throughput window (1 fits, -1 outgrown), and the pairs of the last such level
    bool corridor_lost = false; int corridor_last_n = 0;      // protein: a pair of an earlier level of this pass left the corridor of the precomputed scores (the later levels score the whole matrix)
    void forget_small() { small_state = small_last_n = 0; }
    void forget_corridor() { corridor_lost = false; corridor_last_n = 0; }
    // a level LARGER than the one before it is another pass or family and starts afresh: nothing is known again
    int small_for(int n_run) const { return n_run > small_last_n ? 0 : small_state; }
    void begin_small_level(int n_run) { small_state = small_for(n_run); small_last_n = n_run; }
    bool corridor_lost_for(int n_run) const { return n_run > corridor_last_n ? false : corridor_lost; }
    void begin_corridor_level(int n_run) { corridor_lost = corridor_lost_for(n_run); corridor_last_n = n_run; }
    void update(const Ran &ran, const LadderOutcome &o, int n_run, long long longestRun, const Knobs &k)
    {
        // (the lean kernels check what they read.  A pair that leaves the corridor is re-run by the kernel that scores in line, at a hundred times what the corridor saved
        //  on it: the first such pair takes the rest of the pass off the corridor -- bands widen and paths wander up the tree)
        if (o.guardRound && ran.usedCorridor) corridor_lost = true;
        const bool nucMid = !ran.prot && ran.leanMid && n_run > 0;
        // how the fast window fared (see wideFirst): every pair of a small call outgrew it / the call started wide -> the streak goes on
        if (nucMid && n_run <= 8) wide_streak = (ran.startedWide || (o.redoMt && o.relaunched >= n_run)) ? wide_streak + 1 : 0;
        if (nucMid && ran.startedWide) wide_calls += 1;
        else if (nucMid) { last_wide_pct = (int)(100ll * o.widePairs / n_run); wide_calls = 0; }
        // tiles that outgrew the 512-row window were computed in line by the stitch launch, one after the other per pair -- the expensive way to lose (10 000 x 10 kbp:
        // its levels 6 and 7, where tiles begin to outgrow 512 rows, took 34 and 33 ms instead of 23 and 16 with a 2 % allowance): ANY tile in line takes the pass off it
        if (ran.smallTiles && k.thr_small == 0 && o.firstInline > 0ull) small_state = -1;
        // how the 512-row throughput window fared (plan_nucleotide, small): a level that sent more than 1 % of its pairs on (5 % when they are long) keeps the rest
        // of the pass off it, one that fitted lets the next level start on it.  (longestRun: the longest pair, or one of the sample's: lengths of a level are alike;
        // long pairs re-run tile-parallel: the bet is lost later.)  A level whose own sample said no has set the memory already.
        if (!ran.probed && k.thr_small == 0 && ran.start == Level::From512)
            small_state = (std::max(o.from512Pairs, 0) * 100ll > (longestRun <= 4096 ? 1ll : 5ll) * n_run) ? -1 : 1;
    }
};
// twl_plan_describe's `wide_streak` argument carries the whole memory: below 1000 the streak itself; 1000 + 10 * calls started wide + (1 if three quarters of the last
// narrow-first call went wide); + 100000 * (32 + small_state: -1 / 1) when the pass remembers something of the 512-row throughput window
inline PassMemory memory_from_code(int code)
{
    PassMemory m;
    if (code >= 100000) { m.small_state = code / 100000 - 32; m.small_last_n = INT_MAX; }
    code %= 100000;
    if (code < 1000) m.wide_streak = code;
    else { m.last_wide_pct = ((code - 1000) % 10) ? 100 : 0; m.wide_calls = (code - 1000) / 10; }
    return m;
}

// ---- launch policy of the nucleotide path ----
struct NucFacts {
    int n_run = 0, num_cu = 0, marker = 0;
    const float *M = nullptr;             // 5 x 5 matrix
    float gap_char = 0;
    bool qry_onehot = false, dump = false;
    int shape = 0;                        // what the caller knows about every pair: 0 nothing, 2 leaf x leaf (single sequences on both sides)
    int wide_streak = 0, last_wide_pct = 0, wide_calls = 0;      // copies of PassMemory's
    int small_state = 0;                  // PassMemory::small_for(n_run): the 512-row throughput window (NucPlan::small) on the earlier levels of this pass: 1 they fitted it, -1 one outgrew it, 0 nothing known
    void remember(const PassMemory &m) { wide_streak = m.wide_streak; last_wide_pct = m.last_wide_pct; wide_calls = m.wide_calls; small_state = m.small_for(n_run); }
    const int32_t *h_len = nullptr;       // [pair][2]
    const int32_t *order = nullptr;       // the pairs that run, longest first
};
enum class NucFirst { Dump, WideMt, Mt, SpecShared, Spec16, Few16, Throughput, General };
struct NucPlan {
    NucFirst first = NucFirst::General;
    int mm = 0;                           // matrix mode 0 general / 1 zero N row and column / 2 match-transition-transversion
    bool mm5 = false;                     // ... in its one-letter-query form (mode 5)
    bool lean = false;                    // the round-2 kernels (scores within fast_div's range)
    bool four = false;                    // throughput launch on 4 waves x 3 blocks, four workgroups per CU (768-row window)
    bool small = false;                   // ... on 4 waves x 2 blocks, FIVE workgroups per CU (512-row window): levels of short pairs
    bool probe = false;                   // ... to be decided by a sample of the level's pairs (run_device): levels of 8+ rounds with nothing remembered
    bool held_back = false;               // ... not taken because a recent level outgrew it
    int bulk = 0, tail = 0;               // throughput: pairs in full rounds / remainder through the tile-parallel path
    int sp = 0;                           // the specialised step of the throughput geometries (talco_lean_kernel, SP): 1 leaf x leaf
};
NucPlan plan_nucleotide(const NucFacts &f, const Knobs &k)
{
    NucPlan pl;
    const float *M = f.M;
    // matrix mode (see talco_kernel): 2 = default match/transition/transversion structure with a zero N row/column
    bool nz = true, st3 = true;
    for (int t = 0; t < 5; ++t) nz = nz && M[20 + t] == 0.0f && M[5 * t + 4] == 0.0f;
    for (int l = 0; l < 4; ++l)
        for (int m = 0; m < 4; ++m) st3 = st3 && M[5 * l + m] == ((l == m) ? M[0] : (((l ^ m) == 2) ? M[2] : M[1]));
    pl.mm = nz ? (st3 ? 2 : 1) : 0;
    pl.lean = fast_div_in_range(M, 25, f.gap_char);
    const int mm = pl.mm, n_run = f.n_run;
    // few pairs: one 64-row block per wave (16 waves) for the shortest diagonal step
    const bool few = n_run <= f.num_cu;
    int32_t maxLen = 0;
    long long sumLen = 0;
    for (int32_t t = 0; t < n_run; ++t) {
        const int32_t R = f.h_len[2 * f.order[t]], Q = f.h_len[2 * f.order[t] + 1];
        maxLen = std::max(maxLen, std::max(R, Q)); sumLen += (long long)R + Q;
    }
    // single-sequence query sides and no score for N: matrix mode 5 (the one-letter form of modes 1 and 2)
    pl.mm5 = pl.lean && mm >= 1 && (f.qry_onehot || k.assume_onehot_query);
    // the step without the per-block tests (talco_lean_kernel, SP 1): leaf x leaf, on the one-letter-query score
    pl.sp = (pl.lean && mm == 2 && f.shape == 2 && pl.mm5) ? 1 : 0;
    // very few pairs: two workgroups per pair take the tiles in turn (the mailbox words of that start carry absolute positions in 16 bits each)
    const bool spec = pl.lean && few && (mm == 2 || pl.mm5) && 2 * n_run <= f.num_cu && maxLen <= 65535 && !k.no_spec;
    // Tile-parallel path: always for levels of up to CUs/2 pairs (a pair's tile chain is what they wait for); beyond that when the pairs fill the
    // ONE round of the throughput kernel badly -- tiles spread evenly, at the price of the scouts (~1.2x the work).  Levels of several rounds: the remainder rule below.
    pl.four = pl.lean && (pl.mm5 || mm == 2);
    // With X-drop 5000 a band is ~440 rows wide whatever the length of the pair: most pairs fit a 512-row window, and at 29 KB of LDS and 96 registers FIVE
    // workgroups of 4 waves x 2 blocks share a CU -- five independent anti-diagonal chains per SIMD instead of four (16 384 pairs of 1.6 kbp: 95.7 -> 82.6 ms,
    // leaf x leaf 76.2 -> 65.3 ms, tools/exp_thr.py).  A level whose pairs outgrow the window pays for it twice (they re-run on the 768-row geometry), so the
    // outcome is remembered for the rest of the pass (run_device keeps small_state; bands widen up the tree, and a level LARGER than the one before it is the
    // start of another pass or family: nothing is known again): after a level that fitted the next ones start there, after one that sent more than 1 % of its
    // pairs on the rest of the pass stays off it (the window is worth ~16 % of a level's time; the pairs that outgrow it run twice AND their re-run is a launch
    // of its own that takes a pair's full latency, ~3.5 ms for 1.6 kbp pairs, however few they are: on 100 000 x 1.6 kbp levels of 3-5 % lost 2-11 %), and a
    // level that finds nothing remembered asks ITS OWN pairs when it is large -- eight or more rounds: one pair per CU, spread over the cost order, runs on the
    // small window first (they are part of the level: nothing is computed twice but what outgrows the window; ~3 ms) and the share of them that outgrew it
    // decides for the rest -- and simply tries when it is small.
    const long long longest = n_run > 0 ? (long long)f.h_len[2 * f.order[0]] + f.h_len[2 * f.order[0] + 1] : 0;
    // LONG pairs are eligible too (late round 4: on 10 000 x 10 kbp no pair of any level outgrows 512 rows, and the five workgroups are worth 97.8 against 110 ms
    // on its leaf level, 442 against 469 ms per pass): what made a lost bet expensive there -- the re-run of a FEW 10 kbp pairs, one after the other, a pair's
    // full latency of ~18 ms -- goes through the tile-parallel path instead (run_device: ~3 ms).  They are not sampled (a sample would cost that latency): the
    // first level of a pass pairs sibling leaves, the most similar sequences of the family, and simply tries; the levels above it do as it fared.
    const bool eligible = pl.four && n_run > f.num_cu && k.thr_small == 0;
    pl.probe = eligible && f.small_state == 0 && n_run >= 8 * f.num_cu && longest <= 4096;
    pl.small = (pl.four && n_run > f.num_cu && k.thr_small == 2) || (eligible && f.small_state >= 0);
    pl.held_back = eligible && f.small_state < 0;
    const int perRound = (pl.small ? 5 : (pl.four ? 4 : 2)) * f.num_cu;
    const double roundsThr = (double)n_run / (double)perRound;
    const bool mtOk = pl.lean && mm == 2 && !pl.mm5 && !f.dump && n_run <= k.mt_max_pairs && f.marker >= k.mt_min_marker &&
                      sumLen >= 3ll * f.marker * n_run && (2 * n_run <= f.num_cu || (roundsThr <= 1.0 && std::ceil(roundsThr) >= 1.2 * roundsThr));
    // the last calls' pairs all outgrew the fast window (the deferred pass: one pair per level against the same growing root): no point in finding
    // that out again -- straight to the 3072-row geometry; every 8th such call tries the fast window again
    // ... and so for a level of up to CUs pairs when three quarters of the previous narrow-first level's pairs went on to the wide window (the upper levels
    // of a family whose pairs outgrow the fast window: their narrow attempts cost 40-80 ms each in tiles computed in line up to the overflow); every 6th probes
    const bool wideFirst = k.mt_wide && (n_run <= 8 ? (f.wide_streak >= 2 && (f.wide_streak & 7) != 7)
                                                    : (n_run <= f.num_cu && f.last_wide_pct >= 75 && (f.wide_calls % 6) != 5));
    if (f.dump) pl.first = NucFirst::Dump;
    else if (mtOk && wideFirst) pl.first = NucFirst::WideMt;
    else if (mtOk) pl.first = NucFirst::Mt;
    // CUs/2 < pairs <= CUs: two workgroups per pair taking the tiles in turn, of the 8-wave geometry, two to a CU (all 2n resident at once, as the teams
    // wait for each other).  250 pairs of 10 kbp: 27.6 -> 20.1 ms against one 16-wave workgroup per pair
    else if (pl.lean && mm == 2 && n_run <= f.num_cu && 2 * n_run > f.num_cu && maxLen <= 65535 && !k.no_spec) pl.first = NucFirst::SpecShared;
    else if (spec) pl.first = NucFirst::Spec16;
    else if (pl.lean && few) pl.first = NucFirst::Few16;
    else if (pl.lean) {
        // Many pairs: persistent workgroups take them in rounds.  A last round that is badly filled costs a whole round: when the remainder is small enough
        // its pairs (the shortest ones, the order is longest first) go through the tile-parallel path instead, where they spread over all CUs.
        pl.first = NucFirst::Throughput;
        int tail = n_run % perRound;
        long long tailLen = 0;
        for (int32_t t = n_run - tail; t < n_run; ++t) tailLen += (long long)f.h_len[2 * f.order[t]] + f.h_len[2 * f.order[t] + 1];
        // (pairs of 8+ tiles: with fewer the scouts and extra launches cost more than the idle workgroups)
        if (!(n_run > perRound && tail > 0 && tail * 100 <= k.mt_tail_pct * perRound && tail <= k.mt_max_pairs && pl.four && f.marker >= k.mt_min_marker && tailLen >= 8ll * f.marker * tail)) tail = 0;
        pl.tail = tail; pl.bulk = n_run - tail;
    }
    else pl.first = NucFirst::General;
    if (pl.first != NucFirst::Throughput) pl.small = pl.probe = pl.held_back = false;
    return pl;
}
const char *nuc_first_name(NucFirst f)
{
    switch (f) {
    case NucFirst::Dump: return "dump";
    case NucFirst::WideMt: return "tile-parallel, 3072-row window";
    case NucFirst::Mt: return "tile-parallel";
    case NucFirst::SpecShared: return "speculative teams, 8 waves x 2 blocks";
    case NucFirst::Spec16: return "speculative teams, 16 waves";
    case NucFirst::Few16: return "16 waves x 1 block";
    case NucFirst::Throughput: return "throughput";
    default: return "general (IEEE division)";
    }
}

// ---- a tile-parallel level (launch_mt): its jobs, the sizes of its tables, the geometry class of its launches ----
constexpr int kMtMaxRounds = 7, kMtCounters = 16;      // 1 + 2 * rounds launches, each with its own work counter (the count is clamped wherever it is set)
static_assert(1 + 2 * kMtMaxRounds <= kMtCounters, "scouts + rounds x (tiles, stitch): every launch of a tile-parallel level has a work counter of its own");
struct TileFacts {
    int P = 6, mm = 2, tw = 8, trpl = 1, stitch_rpl = 1;      // launch_mt's template arguments and the 64-row blocks per wave of its stitch launch, as the kernel name carries them
    bool wide = false;                    // the 3072-row geometry (launch_mt, WIDE)
    bool can_small = false;               // the instantiation has the 512-row throughput geometry (nucleotide, 4-wave throughput geometry, not wide) ...
    bool small_tiles = false;             // ... and the earlier levels of this pass fitted it
    int n_run = 0, marker = 0, seq_len = 0;
    int rec_words = 0;                    // words of a tile's record (talco_mt.hip.h, kMtRec)
    const int32_t *order = nullptr;       // the pairs that run
    const int32_t *h_len = nullptr;       // [pair][2]
};
struct TilePlan {
    int slots = 0, segcap = 0, sp_pitch = 0;      // tile boundaries of the longest pair the call may hold, bytes of a tile's path segment, words of a pair's scout path
    std::vector<int> T;                   // tiles of every pair, by its position in `order`
    int maxT = 0, nScout = 0, nTile = 0;  // jobs {pair, slot, row}: nScout scouts, then nTile tiles
    long long maxRQ = 0;                  // R + Q of the longest pair
    size_t chain_ints = 0, rec_ints = 0, seg_bytes = 0, spath_ints = 0, stat_bytes = 0, jobs_ints = 0, anchor_ints = 0;      // the device tables; rows are positions in `order` (not pair ids)
    bool thr = false;                     // scouts and tiles on the throughput geometry: more tile jobs than fit the device at once
    bool smallT = false;                  // ... the tiles too on its 512-row form
    bool longScouts = false;              // the longer margin and anchored lead (twl_knobs.inc.hip: levels of at most a round or two of tile jobs)
    bool anchors = false;                 // mt_anchor_kernel runs in front of the scouts
    int lead2 = 0, marg = 0, rounds = 1;
    size_t tb_groups = 0;                 // wide: groups of 8 anti-diagonals the pair scout (MT 4) keeps of the longest pair
};
// `jobs` is the caller's: the upload of it is asynchronous, so it has to outlive the call.
TilePlan plan_tile_level(const TileFacts &f, const Knobs &k, std::vector<int32_t> &jobs)
{
    TilePlan pl;
    pl.slots = (2 * f.seq_len) / (f.marker - 1) + 2;
    pl.segcap = 2 * f.marker + 16;
    pl.sp_pitch = 2 * f.seq_len + 8;
    pl.T.resize((size_t)f.n_run);
    for (int t = 0; t < f.n_run; ++t) {
        const long long RQ = (long long)f.h_len[2 * f.order[t]] + f.h_len[2 * f.order[t] + 1];
        int n = 1;
        while (n < pl.slots && (long long)(f.marker - 1) * n - 1 <= RQ - 2) ++n;
        pl.T[t] = n; pl.maxT = std::max(pl.maxT, n); pl.maxRQ = std::max(pl.maxRQ, RQ);
    }
    // scouts for every tile boundary s >= 1 that exists, then tiles for s >= 0 (tile-major, so that the tiles of a pair spread over the launch)
    jobs.clear();
    for (int s = 1; s < pl.maxT; ++s) for (int t = 0; t < f.n_run; ++t) if (s < pl.T[t]) { jobs.push_back(f.order[t]); jobs.push_back(s); jobs.push_back(t); }
    pl.nScout = (int)(jobs.size() / 3);
    for (int s = 0; s < pl.maxT; ++s) for (int t = 0; t < f.n_run; ++t) if (s < pl.T[t]) { jobs.push_back(f.order[t]); jobs.push_back(s); jobs.push_back(t); }
    pl.nTile = (int)(jobs.size() / 3) - pl.nScout;
    const size_t np = (size_t)f.n_run;
    pl.chain_ints = np * pl.slots * 2;
    pl.rec_ints = np * pl.slots * f.rec_words;
    pl.seg_bytes = np * pl.slots * (size_t)pl.segcap;
    pl.spath_ints = np * (size_t)pl.sp_pitch;
    pl.stat_bytes = 4 * sizeof(unsigned long long) + np * 8 * sizeof(int32_t);      // counters, then the per-pair frontier
    pl.jobs_ints = jobs.size();
    // scouts of the narrow geometries start from an anchored cell where the profiles give one (talco_mt.hip.h, mt_anchor_kernel)
    pl.anchors = !f.wide && k.mt_anchor && pl.nScout > 0;
    pl.anchor_ints = pl.anchors ? np * pl.slots : 0;
    pl.thr = !f.wide && pl.nTile > k.mt_thr_jobs;
    // small tiles (nucleotide, throughput geometry): the tile jobs too run on 4 waves x 2 blocks, five workgroups per CU -- the earlier levels of this pass
    // fitted the 512-row window (plan_nucleotide, small).  A tile that outgrows it leaves a failed record of a window narrower than the stitch launch's, which
    // the stitch launch does not adopt: it computes that tile in line (run_device counts them and takes the pass off the small window when they are many).
    pl.smallT = f.can_small && f.small_tiles;
    // (see twl_knobs.inc.hip: longer scouts where the tile jobs are at most a round or two of the device's workgroups and a missed start a second round that lasts as long as the first)
    pl.longScouts = !f.wide && pl.nTile <= 2048;
    pl.lead2 = pl.longScouts ? k.mt_lead2_lat : k.mt_lead2;
    pl.marg = pl.longScouts ? k.mt_marg_lat : k.mt_marg;
    pl.rounds = std::max(1, std::min(k.mt_rounds, kMtMaxRounds));
    pl.tb_groups = f.wide ? (size_t)(pl.maxRQ >> 3) + 2 : 0;
    return pl;
}
// what twl_stats.kernel says of a level that started tile-parallel
inline void tile_level_name(char *s, size_t n, const TileFacts &f, const TilePlan &pl)
{
    if (pl.thr && pl.smallT) snprintf(s, n, "talco_lean_kernel<%d, 4, 2, %d, 5, false, false, 2 / 1> + <%d, 16, 1, %d, 1, false, false, 3> (tile-parallel: scouts, tiles, stitch)", f.P, f.mm, f.P, f.mm);
    else if (pl.thr) snprintf(s, n, "talco_lean_kernel<%d, %d, %d, %d, 4, false, false, 2 / 1> + <%d, 16, 1, %d, 1, false, false, 3> (tile-parallel: scouts, tiles, stitch)", f.P, f.tw, f.trpl, f.mm, f.P, f.mm);
    else snprintf(s, n, "talco_lean_kernel<%d, 16, %d, %d, 1, false, false, 2 / 1 / 3> (tile-parallel: scouts, tiles, stitch)", f.P, f.stitch_rpl, f.mm);
}

// ---- launch policy of the protein path ----
struct ProtFacts {
    int n_run = 0, n_pairs = 0, num_cu = 0, marker = 0;
    const float *M = nullptr;             // 21 x 21 matrix
    float gap_char = 0;
    bool dump = false;
    bool corridor_lost = false;           // PassMemory::corridor_lost_for(n_run)
    const int32_t *h_len = nullptr;       // [pair][2], all n_pairs of the call
    const int32_t *order = nullptr;       // the pairs that run, longest first
};
enum class ProtFirst { R1, Dense, MtPresim, SpecShared, Spec16, Plain16, Thr512, Sparse16, Ieee, Dump };
struct ProtPlan {
    ProtFirst first = ProtFirst::Ieee;
    int mm = -1;                          // matrix mode 3 sparse score loop in the kernel / 4 precomputed scores (-1: the round-1 kernels behind r1 / dense)
    bool lean = false;                    // the round-2 kernels (scores within fast_div's range)
    bool presim = false;                  // score_matrix_kernel runs first ...
    size_t simFloats = 0;                 // ... into this many floats ...
    int corridor = 0;                     // ... within this half-width of the diagonal (0: the whole R x Q matrix)
    int spec = 0;                         // twl_stats.speculative
    bool small = false;                   // a 512-row geometry: what outgrows it has the 16-wave kernel ahead
};
ProtPlan plan_protein(const ProtFacts &f, const Knobs &k)
{
    ProtPlan pl;
    const ProtMode pm = k.prot_mode;
    const int n_run = f.n_run;
    // default: sparse score loop over the non-zero letters of the reference column (matrix mode 3, bit-identical to the dense loop)
    pl.lean = fast_div_in_range(f.M, 441, f.gap_char) && (pm == ProtMode::Auto || pm == ProtMode::LeanSparse || pm == ProtMode::LeanPresim);
    if (pm == ProtMode::R1 || pm == ProtMode::Dense) { pl.first = pm == ProtMode::R1 ? ProtFirst::R1 : ProtFirst::Dense; return pl; }
    // Few pairs (upper tree levels): the serial diagonal chain of each pair is what costs, and most of its instructions are the
    // column score.  Scores do not depend on the DP state, so the otherwise idle CUs compute them for the whole R x Q matrix
    // first (score_matrix_kernel, same arithmetic) and the DP kernel only loads them (matrix mode 4).
    int32_t blocks = 0, maxLen = 0;
    long long sumLen = 0;
    for (int32_t t = 0; t < n_run; ++t) {
        const long long R = f.h_len[2 * f.order[t]], Q = f.h_len[2 * f.order[t] + 1];
        pl.simFloats += (size_t)((R + Q) * ((Q + 63) & ~63ll));
        blocks += (int32_t)(((R + Q - 1 + 63) / 64) * ((Q + 63) / 64));
        sumLen += R + Q;
    }
    for (int32_t t = 0; t < 2 * f.n_pairs; ++t) maxLen = std::max(maxLen, f.h_len[t]);
    const bool few = n_run <= std::max(1, f.num_cu / 2);      // measured break-even vs the sparse in-kernel path: ~150 pairs of 2 kaa
    const bool fits = pl.simFloats * sizeof(float) <= ((size_t)16 << 30) && blocks > 0;
    // very few pairs: two workgroups per pair take the tiles in turn (the mailbox words of that start carry absolute positions in 16 bits each)
    const bool spec16 = pl.lean && 2 * n_run <= f.num_cu && maxLen <= 65535 && !k.no_spec;
    // CUs/2 < pairs <= CUs: speculative teams of the 512-row geometry, two workgroups per CU, on precomputed scores (as the nucleotide
    // path does with its throughput geometry)
    const bool sharedSpec = pl.lean && pm == ProtMode::Auto && !few && n_run <= f.num_cu && maxLen <= 65535 && fits && !f.dump && !k.no_spec;
    pl.presim = (pm == ProtMode::Presim || pm == ProtMode::LeanPresim || (pm == ProtMode::Auto && few) || sharedSpec) && fits && !f.dump;
    pl.mm = pl.presim ? 4 : 3;
    // tile-parallel (talco_nuc.hip.h, MT kernels) on the precomputed scores: pairs of 2 kaa have 4-5 tiles each
    const bool mtOk = pl.lean && pm == ProtMode::Auto && n_run <= k.mt_max_pairs && n_run <= f.num_cu && f.marker >= k.mt_min_marker && sumLen >= 3ll * f.marker * n_run;
    if (pl.presim) {
        // (the round-1 kernel behind a matrix outside the range does not check what it reads: the corridor is for the lean kernels; a pass that lost it scores the whole matrix)
        pl.corridor = (pl.lean && !f.corridor_lost) ? k.prot_corridor : 0;
        pl.first = mtOk ? ProtFirst::MtPresim : sharedSpec ? ProtFirst::SpecShared : spec16 ? ProtFirst::Spec16 : pl.lean ? ProtFirst::Plain16 : ProtFirst::Ieee;
    }
    else if (f.dump) pl.first = ProtFirst::Dump;      // twl_dp_column_scores (one pair, lean: the launch step refuses anything else)
    // more pairs than CUs: the 512-row window (8 waves, one block each; protein bands of 2 kaa pairs are ~270 rows wide, ~400
    // at most) keeps the ring at 61 KB, so two workgroups share a CU like in the nucleotide throughput kernel; a pair
    // whose band outgrows it goes to the 16-wave kernel (1024 rows) by the ladder
    else if (pl.lean && n_run > f.num_cu) pl.first = ProtFirst::Thr512;
    else pl.first = pl.lean ? ProtFirst::Sparse16 : ProtFirst::Ieee;
    pl.spec = pl.first == ProtFirst::MtPresim ? 3 : pl.first == ProtFirst::SpecShared ? 2 : pl.first == ProtFirst::Spec16 ? 1 : 0;
    pl.small = pl.first == ProtFirst::SpecShared || pl.first == ProtFirst::Thr512;
    return pl;
}
const char *prot_first_name(ProtFirst f)
{
    switch (f) {
    case ProtFirst::R1: return "round-1 kernel, 8 waves x 1 block";
    case ProtFirst::Dense: return "dense, 8 waves x 2 blocks";
    case ProtFirst::MtPresim: return "tile-parallel on precomputed scores";
    case ProtFirst::SpecShared: return "speculative teams, 8 waves x 1 block";
    case ProtFirst::Spec16: return "speculative teams, 16 waves";
    case ProtFirst::Plain16: return "16 waves x 1 block on precomputed scores";
    case ProtFirst::Thr512: return "throughput, 8 waves x 1 block";
    case ProtFirst::Sparse16: return "16 waves x 1 block";
    case ProtFirst::Dump: return "dump";
    default: return "general (IEEE division)";
    }
}
inline int prot_first_window(ProtFirst f) { return (f == ProtFirst::R1 || f == ProtFirst::SpecShared || f == ProtFirst::Thr512) ? 512 : 1024; }

// ---- the re-run ladder: which rung a set of outgrown pairs takes, and where the next round stands ----
enum class Rung { Guard, Thr768, MtStitch1024, Lean1024, Prot16, Mt3072, Lean2048, Ieee16x2, Wide4608, Global };
enum class RedoKind { Guard, Overflow };      // pairs with an operand outside the fast division's range / pairs whose band outgrew the window
struct RedoFacts { int count = 0; long long sumLen = 0; int marker = 0; bool dump = false; };      // the pairs to re-run: how many, their summed R + Q
struct Step { Rung rung; Level next; };
Step next_rung(const Ran &ran, Level at, RedoKind kind, const RedoFacts &f, const Knobs &k)
{
    if (at == Level::Global) return {Rung::Global, Level::Global};      // no window, IEEE division: takes whatever is left, of either kind
    // the IEEE-division kernel of the same window; the window rungs follow once these are done
    if (kind == RedoKind::Guard) return {Rung::Guard, at};
    const bool tiles = f.count <= k.mt_max_pairs && f.marker >= k.mt_min_marker;
    switch (at) {
    case Level::From512:
        // the 512-row throughput window was outgrown: the 768-row throughput geometry takes these pairs -- unless they are a few LONG pairs (8+ tiles each): then all
        // their tiles at once (1024-row stitch window) instead of one pair after the other for a pair's full latency
        if (tiles && f.sumLen >= 8ll * f.marker * (long long)f.count && !f.dump) return {Rung::MtStitch1024, Level::Mid};
        return {Rung::Thr768, Level::From768};
    case Level::From768:      // the throughput launch's 768-row window was outgrown: first the 1024-row one (8 waves x 2 blocks)
        return {Rung::Lean1024, Level::Mid};
    case Level::Mid:
        if (ran.prot) return {Rung::Prot16, Level::Wide};
        if (!ran.leanMid) return {Rung::Ieee16x2, Level::Wide};
        // nucleotide, default matrix structure: every tile of these pairs at once on a 3072-row window (launch_mt, WIDE) when they have tiles
        // to spread; otherwise the lean kernel on a 2048-row window (8 waves x 4 blocks, reference ring still in LDS), tile after tile
        return {(k.mt_wide && tiles && f.sumLen >= 3ll * f.marker * (long long)f.count) ? Rung::Mt3072 : Rung::Lean2048, Level::Wide};
    default:                  // 4608-row window (8 waves x 9 blocks; covers flen = 4096; columns from L2/HBM)
        return {Rung::Wide4608, Level::Global};
    }
}
const char *rung_name(Rung r)
{
    static const char *const names[] = {"guard (IEEE division)", "throughput 768", "tile-parallel 1024", "lean 1024", "protein 16-wave", "tile-parallel 3072", "lean 2048", "16 x 2 IEEE", "wide 4608", "global"};
    return names[(int)r];
}
