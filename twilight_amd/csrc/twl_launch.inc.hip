// twilight_amd/csrc/twl_launch.inc.hip -- one function per kernel family that sizes the scratch, fills the kernel arguments and launches: round-1 kernels, the global-memory kernel, the lean kernels, the tile-parallel launches of a level.
// Included by twl_align.hip (one translation unit: it shares that file's Device bookkeeping, error string and fill queue).

// Traceback words of a workgroup: the groups of 8 anti-diagonals up to the marker, a window of rows each.
template <class CfgT>
size_t tb_words_for(int marker) { return ((size_t)(marker >> 3) + 1) * (size_t)CfgT::WINDOW; }
// ... `words` of them for each of `grid` workgroups in `b`, poisoned when the knob asks (tests: see g_poison_tb)
int ensure_tb(Buf &b, hipStream_t st, size_t words, int grid)
{
    const size_t bytes = words * sizeof(uint32_t) * (size_t)grid;
    if (const int rc = b.ensure(bytes)) return rc;
    if (g_poison_tb) HIP_TRY(hipMemsetAsync(b.p, 0xFF, bytes, st));
    return TWL_OK;
}
// Resident workgroups per CU of one kernel instantiation, queried once (the static is one per instantiation; device threads may race to fill it: same value).
template <auto Kernel, int THREADS>
int resident_per_cu(int *out)
{
    static std::atomic<int> cached{0};
    if (cached.load() == 0) {
        int nb = 0;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, Kernel, THREADS, 0));
        cached.store(std::max(1, nb));
    }
    *out = cached.load();
    return TWL_OK;
}
// What the lean kernels' arguments take over from the call's; the caller adds the traceback scratch, the items, the work counter and what is its own.
twl::NArgs lean_args(const Device *d, const twl::KArgs &base)
{
    twl::NArgs a{};
    a.cols = base.cols; a.len = base.len; a.num = base.num; a.aln = base.aln; a.aln_len = base.aln_len; a.err = base.err;
    a.cells = base.cells; a.seq_len = base.seq_len; a.n_pairs_total = base.n_pairs_total;
    a.step_slack = base.step_slack; a.gap_open = base.gap_open; a.gap_extend = base.gap_extend; a.gap_char = base.gap_char; a.gc_zero = base.gc_zero;
    a.xdrop = base.xdrop; a.flen = base.flen; a.marker = base.marker;
    for (int t = 0; t < 25; ++t) a.M[t] = base.M[t];
    a.M24 = (const float *)d->m24.p; a.sim = base.sim; a.sim_off = base.sim_off;
    return a;
}

template <int P, int W, int RPL, bool PRE, bool REFLDS, bool QREG = true, int MINW = 1, int MM = 0>
int launch_dp(Device *d, hipStream_t st, const twl::KArgs &base, const int32_t *d_items, int n_items, int blocks_per_cu, int *grid_out,
              int *window_out = nullptr)
{
    using CfgT = twl::Cfg<P, W, RPL, PRE, REFLDS, QREG>;
    int rc;
    if (blocks_per_cu <= 0 && (rc = resident_per_cu<twl::talco_kernel<P, W, RPL, PRE, REFLDS, QREG, MINW, MM>, CfgT::THREADS>(&blocks_per_cu))) return rc;
    if (window_out) *window_out = CfgT::WINDOW;
    int grid = std::min(n_items, d->num_cu * std::max(1, blocks_per_cu));
    if (grid < 1) grid = 1;
    const size_t tbw = tb_words_for<CfgT>(base.marker);
    if ((rc = ensure_tb(d->tb, st, tbw, grid))) return rc;
    twl::KArgs a = base;
    a.tb = (uint32_t *)d->tb.p;
    a.tb_words = (int32_t)tbw;
    a.items = d_items;
    a.n_items = n_items;
    FILL_TRY(queue_fill(d, st, d->queue.p, sizeof(int32_t), 0));
    int32_t *hb = nullptr;
#ifdef TWL_KERNEL_DEBUG
    if (dbg_on()) {
        HIP_TRY(hipHostMalloc((void **)&hb, 16 * sizeof(int32_t), hipHostMallocMapped));
        for (int i = 0; i < 16; ++i) hb[i] = -777;
        a.hb = hb;
    }
#endif
    TRACE("launch dp W=%d RPL=%d grid=%d threads=%d n_items=%d tb_words=%zu", W, RPL, grid, CfgT::THREADS, n_items, tbw);
    if (!d->kname[0]) snprintf(d->kname, sizeof d->kname, "talco_kernel<%d, %d, %d, %s, %s, %s, %d, %d>", P, W, RPL, PRE ? "true" : "false", REFLDS ? "true" : "false", QREG ? "true" : "false", MINW, MM);
    FILL_TRY(flush_fills(d, st));
    hipLaunchKernelGGL((twl::talco_kernel<P, W, RPL, PRE, REFLDS, QREG, MINW, MM>), dim3(grid), dim3(CfgT::THREADS), 0, st, a);
    HIP_TRY(hipGetLastError());
    if (hb) {   // debug only: poll the heartbeat until the kernel is done (or 20 s)
        for (int t = 0; t < 200; ++t) {
            if (hipStreamQuery(st) == hipSuccess) break;
            std::this_thread::sleep_for(std::chrono::milliseconds(100));
            if (t % 10 == 9)
                TRACE("hb: start %d item %d tile %d k %d preB %d postB %d preTB %d postTB %d n %d err %d done %d", hb[0], hb[1], hb[2], hb[3],
                      hb[4], hb[5], hb[6], hb[7], hb[8], hb[9], hb[10]);
        }
        TRACE("hb final: start %d item %d tile %d k %d preB %d postB %d preTB %d postTB %d n %d err %d done %d", hb[0], hb[1], hb[2], hb[3],
              hb[4], hb[5], hb[6], hb[7], hb[8], hb[9], hb[10]);
    }
    *grid_out = grid;
    return TWL_OK;
}

// The last stage of the re-run chain (talco_global.hip.h): DP rows in global scratch, any band width.  One workgroup of 1024 threads per pair; as many
// workgroups as the pairs need, within a scratch budget (a 30 kbp pair at marker 1024 takes ~33 MB: 14 rows of fLen + 2 words and (marker + 2) rows of pointer bytes).
template <int P>
int launch_global(Device *d, hipStream_t st, const twl::KArgs &base, const int32_t *d_items, int n_items, int32_t seq_len, int *grid_out, int *window_out)
{
    const size_t rowcap = (size_t)std::min(std::max(base.flen, 1), std::max(seq_len, 1)) + 2;
    const size_t words = 14 * rowcap + (((size_t)base.marker + 2) * rowcap + 3) / 4;
    const size_t budget = (size_t)4 << 30;
    // one pair's scratch may not be larger than the budget either: refused (the caller sees TWL_ERR_UNSUPPORTED), not silently pinned in HBM
    if (words * sizeof(uint32_t) > budget) { g_err = "a pair whose band needs more than 4 GiB of scratch in the global-memory kernel"; return TWL_ERR_UNSUPPORTED; }
    int grid = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_items, budget / (words * sizeof(uint32_t))));
    grid = std::min(grid, d->num_cu);
    // a buffer of its own, handed back after the stage (run_device: release_global_scratch): d->tb lives until twl_shutdown and a single retry of the deferred
    // pass would otherwise pin several GiB next to the resident store for the rest of the run
    const int rc = ensure_tb(d->gtb, st, words, grid);
    if (rc) return rc;
    twl::GArgs g;
    g.k = base;
    g.k.tb = (uint32_t *)d->gtb.p;
    g.k.tb_words = (int32_t)words;
    if ((size_t)g.k.tb_words != words) { g_err = "a pair too long for the global-memory kernel's scratch index"; return TWL_ERR_UNSUPPORTED; }
    g.k.items = d_items;
    g.k.n_items = n_items;
    g.rowcap = (int32_t)rowcap;
    FILL_TRY(queue_fill(d, st, d->queue.p, sizeof(int32_t), 0));
    FILL_TRY(flush_fills(d, st));
    TRACE("launch global P=%d grid=%d n_items=%d rowcap=%zu words=%zu", P, grid, n_items, rowcap, words);
    hipLaunchKernelGGL((twl::talco_global_kernel<P>), dim3(grid), dim3(1024), 0, st, g);
    HIP_TRY(hipGetLastError());
    *grid_out = grid;
    if (window_out) *window_out = (int)rowcap - 2;
    return TWL_OK;
}

// The round-2 nucleotide kernel (talco_nuc.hip.h): same launch protocol as launch_dp.
template <int P, int W, int RPL, int MM, int MINW, bool SPEC = false, bool DUMP = false, int SP = 0>
int launch_lean(Device *d, hipStream_t st, const twl::KArgs &base, const int32_t *d_items, int n_items, int *grid_out, int *window_out)
{
    using CfgT = twl::NCfg<W, RPL>;
    int rc, blocks_per_cu = 0;
    if ((rc = resident_per_cu<twl::talco_lean_kernel<P, W, RPL, MM, MINW, SPEC, DUMP, 0, SP>, CfgT::THREADS>(&blocks_per_cu))) return rc;
    if (window_out) *window_out = CfgT::WINDOW;
    int grid = std::min(n_items, d->num_cu * blocks_per_cu);
    if (grid < 1) grid = 1;
    if (SPEC) {      // two workgroups per pair that wait for each other: all of them must be resident at once
        grid = 2 * n_items;
        if (grid > d->num_cu * blocks_per_cu) { g_err = "speculative launch larger than the device"; return TWL_ERR_BAD_ARGUMENT; }
    }
    const size_t tbw = tb_words_for<CfgT>(base.marker);
    if ((rc = ensure_tb(d->tb, st, tbw, grid))) return rc;
    twl::NArgs a = lean_args(d, base);
    a.tb = (uint32_t *)d->tb.p; a.tb_words = (int32_t)tbw; a.queue = base.queue; a.items = d_items; a.n_items = n_items; a.dbg = base.dbg;
    FILL_TRY(queue_fill(d, st, d->queue.p, sizeof(int32_t), 0));
    if (SPEC) {
        if ((rc = d->team.ensure((size_t)n_items * twl::kTeamWords * sizeof(unsigned long long)))) return rc;
        FILL_TRY(queue_fill(d, st, d->team.p, (size_t)n_items * twl::kTeamWords * sizeof(unsigned long long), 0));
        FILL_TRY(queue_fill(d, st, a.cells, (size_t)base.n_pairs_total * sizeof(unsigned long long), 0));
        a.team = (unsigned long long *)d->team.p;
    }
    TRACE("launch lean P=%d W=%d RPL=%d MM=%d grid=%d threads=%d n_items=%d tb_words=%zu", P, W, RPL, MM, grid, CfgT::THREADS, n_items, tbw);
    if (!d->kname[0]) {
        if constexpr (SP != 0) snprintf(d->kname, sizeof d->kname, "talco_lean_kernel<%d, %d, %d, %d, %d, %s, %s, 0, %d>", P, W, RPL, MM, MINW, SPEC ? "true" : "false", DUMP ? "true" : "false", SP);
        else snprintf(d->kname, sizeof d->kname, "talco_lean_kernel<%d, %d, %d, %d, %d, %s, %s, 0>", P, W, RPL, MM, MINW, SPEC ? "true" : "false", DUMP ? "true" : "false");
    }
    a.simdump = DUMP ? (float *)d->simdump.p : nullptr;
    FILL_TRY(flush_fills(d, st));
    // (the bulk of a throughput level whose remainder runs beside it: that stream waits for what is in front of this kernel -- the order, the arguments' uploads, the
    // fills of the outputs -- and not for the kernel, behind which an event would complete only when the bulk has)
    if (d->fork_next) { d->fork_next = false; HIP_TRY(hipEventRecord(d->tail_ev[0], st)); }
    hipLaunchKernelGGL((twl::talco_lean_kernel<P, W, RPL, MM, MINW, SPEC, DUMP, 0, SP>), dim3(grid), dim3(CfgT::THREADS), 0, st, a);
    HIP_TRY(hipGetLastError());
    if (SPEC && dbg_on()) {      // development: how often the guessed tile start was the true one
        std::vector<unsigned long long> tw((size_t)n_items * twl::kTeamWords);
        HIP_TRY(hipMemcpyAsync(tw.data(), d->team.p, tw.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        unsigned long long g = 0, h = 0;
        for (int t = 0; t < n_items; ++t) { g += tw[(size_t)t * twl::kTeamWords + twl::kTeamStat]; h += tw[(size_t)t * twl::kTeamWords + twl::kTeamStat + 1]; }
        fprintf(stderr, "[twl spec] %d pairs: %llu tile starts guessed, %llu confirmed\n", n_items, g, h);
    }
    *grid_out = grid;
    return TWL_OK;
}

// What a tile-parallel level launched beside a running bulk launch (first_throughput, Device::tail_side) may not share with it: the traceback scratch, which
// ensure_tb may grow or poison, and the work counters -- a second block of kMtCounters behind the first in d->queue (run_device sizes the buffer for both
// before anything is launched; 64 bytes in, so that the block is zeroed by the fill queue like the first).
constexpr int kTailCounterBase = 16;
static_assert(kTailCounterBase >= kMtCounters && (kTailCounterBase * sizeof(int32_t)) % 16 == 0, "the remainder's counters start behind the level's, 16-byte aligned");
constexpr size_t kQueueBytes = (size_t)(kTailCounterBase + kMtCounters) * sizeof(int32_t);
Buf &mt_tb(Device *d) { return d->tail_side ? d->tb_tail : d->tb; }
int32_t *mt_counters(Device *d) { return (int32_t *)d->queue.p + (d->tail_side ? kTailCounterBase : 0); }

// One launch of a tile-parallel kernel (MT 1 tiles / 2 scouts / 3 stitch) of geometry <W, RPL>; the caller has filled the NArgs.
template <int P, int W, int RPL, int MM, int MINW, int MT, int SP = 0>
int launch_mt_kernel(Device *d, hipStream_t st, twl::NArgs a, int n_items, int *grid_out = nullptr, size_t tb_groups = 0)
{
    using CfgT = twl::NCfg<W, RPL>;
    int rc, blocks_per_cu = 0;
    if ((rc = resident_per_cu<twl::talco_lean_kernel<P, W, RPL, MM, MINW, false, false, MT, SP>, CfgT::THREADS>(&blocks_per_cu))) return rc;
    int grid = std::max(1, std::min(n_items, d->num_cu * blocks_per_cu));
    // traceback words of a workgroup: up to the marker, or (pair scouts, MT 4) the tb_groups groups of a whole pair
    // A scout (MT 2) keeps traceback words up to ITS marker, slot + 2 + mt_marg + lead anti-diagonals (talco_lean_kernel: spHi + mt_marg - scoutD0, at most kMaxMarker), which at a
    // small marker of the level is the larger of the two: sized by the level's marker alone its words ran over into the next workgroup's (what a scout found then depended on
    // its neighbours: predictions differed from run to run on the same level) and, behind the last workgroup, past the launch's share of the buffer.
    int tbMarker = a.marker;
    if constexpr (MT == 2) tbMarker = std::max(tbMarker, std::min(a.mt_slots + 2 + a.mt_marg + std::max(a.mt_lead, a.mt_lead2), twl::kMaxMarker));
    const size_t tbw = tb_groups ? tb_groups * (size_t)CfgT::WINDOW : tb_words_for<CfgT>(tbMarker);
    if (tb_groups) grid = (int)std::max<size_t>(1, std::min<size_t>((size_t)grid, ((size_t)8 << 30) / (tbw * sizeof(uint32_t))));      // (at most 8 GB of them: fewer workgroups take the pairs in turn)
    Buf &tb = mt_tb(d);
    if ((rc = ensure_tb(tb, st, tbw, grid))) return rc;
    a.tb = (uint32_t *)tb.p; a.tb_words = (int32_t)tbw; a.n_items = n_items;
    // (every launch of a tile-parallel level has its own work counter: launch_mt zeroed the 16 of them in one go)
    a.queue = mt_counters(d) + (d->mt_launch++ % kMtCounters);
    FILL_TRY(flush_fills(d, st));
    hipLaunchKernelGGL((twl::talco_lean_kernel<P, W, RPL, MM, MINW, false, false, MT, SP>), dim3(grid), dim3(CfgT::THREADS), 0, st, a);
    HIP_TRY(hipGetLastError());
    if (grid_out) *grid_out = grid;
    return TWL_OK;
}


// What the host knows about every pair of a nucleotide launch, taken out of the kernel's per-block tests (talco_lean_kernel, SP): 1 = leaf x leaf (needs the
// one-letter-query column score, MM 5).  Only the throughput geometries have the specialised step.
template <int W, int RPL, int MINW>
int launch_thr(Device *d, hipStream_t st, const twl::KArgs &a, const int32_t *items, int n, int *grid, int *window, bool mm5, int sp)
{
    if (mm5) {
        if (sp == 1) return launch_lean<6, W, RPL, 5, MINW, false, false, 1>(d, st, a, items, n, grid, window);
        return launch_lean<6, W, RPL, 5, MINW>(d, st, a, items, n, grid, window);
    }
    return launch_lean<6, W, RPL, 2, MINW>(d, st, a, items, n, grid, window);
}
template <int W, int RPL, int MM, int MINW, int MT>
int launch_mt_thr(Device *d, hipStream_t st, const twl::NArgs &a, int n_items, int *grid_out, int sp)
{
    if constexpr (MM == 5) { if (sp == 1) return launch_mt_kernel<6, W, RPL, MM, MINW, MT, 1>(d, st, a, n_items, grid_out); }
    return launch_mt_kernel<6, W, RPL, MM, MINW, MT>(d, st, a, n_items, grid_out);
}

// The tables of a tile-parallel level as its plan sizes them, the upload of its jobs (`jobs` outlives the call: Device::mt_jobs_host) and the fills, queued in front of its first kernel.
int prepare_mt_tables(Device *d, hipStream_t st, const TilePlan &pl, const std::vector<int32_t> &jobs)
{
    int rc;
    if ((rc = d->mt_chain.ensure(pl.chain_ints * sizeof(int32_t)))) return rc;
    if ((rc = d->mt_rec.ensure(pl.rec_ints * sizeof(int32_t)))) return rc;
    if ((rc = d->mt_seg.ensure(pl.seg_bytes))) return rc;
    if ((rc = d->mt_spath.ensure(pl.spath_ints * sizeof(int32_t)))) return rc;
    if ((rc = d->mt_stat.ensure(pl.stat_bytes))) return rc;
    if ((rc = d->mt_jobs.ensure(pl.jobs_ints * sizeof(int32_t)))) return rc;
    if (pl.anchors && (rc = d->mt_anchor.ensure(pl.anchor_ints * sizeof(int32_t)))) return rc;
    HIP_TRY(hipMemcpyAsync(d->mt_jobs.p, jobs.data(), pl.jobs_ints * sizeof(int32_t), hipMemcpyHostToDevice, st));
    FILL_TRY(queue_fill(d, st, d->mt_rec.p, pl.rec_ints * sizeof(int32_t), 0));
    FILL_TRY(queue_fill(d, st, d->mt_spath.p, pl.spath_ints * sizeof(int32_t), 0xFE));
    FILL_TRY(queue_fill(d, st, d->mt_stat.p, pl.stat_bytes, 0));
    if (pl.anchors) FILL_TRY(queue_fill(d, st, d->mt_anchor.p, pl.anchor_ints * sizeof(int32_t), 0xFF));
    FILL_TRY(queue_fill(d, st, mt_counters(d), kMtCounters * sizeof(int32_t), 0));      // one work counter per launch: scouts + rounds x (tiles, stitch); launch_mt_kernel hands them out
    d->mt_launch = 0;
    return TWL_OK;
}

// What twl_mt_tables reports of a tile-parallel level: the dims of its plan and the pair of every table row.  Host integers only.
static_assert(TWL_MT_REC_WORDS == twl::kMtRec, "include/twl_align.h states the words of a tile's record");
void remember_mt_plan(Device *d, const TilePlan &pl, const std::vector<int32_t> &order, int n_run, int marker)
{
    twl_mt_dims &m = d->mt_dims;
    m = twl_mt_dims{};
    m.n_run = n_run; m.slots = pl.slots; m.sp_pitch = pl.sp_pitch; m.segcap = pl.segcap; m.n_scout = pl.nScout; m.n_tile = pl.nTile; m.rounds = pl.rounds;
    m.lead2 = pl.lead2; m.marg = pl.marg; m.anchors = pl.anchors ? 1 : 0; m.thr = pl.thr ? 1 : 0; m.small_tiles = pl.smallT ? 1 : 0; m.marker = marker;
    d->mt_order.assign(order.begin(), order.begin() + n_run);
    d->mt_seen = true;
}
// twl_mt_tables: plain copies of the buffers the last tile-parallel level left behind, after the device's stream has drained.  No launch.
int read_mt_tables(Device *d, twl_mt_dims *dims, int32_t *order, int32_t *anchor, int32_t *spath, int32_t *chain, int32_t *rec, int8_t *seg, int32_t *front)
{
    if (!d->mt_seen) { g_err = "no tile-parallel level has run on this device since twl_init"; return TWL_ERR_BAD_ARGUMENT; }
    const twl_mt_dims &m = d->mt_dims;
    if (anchor && !m.anchors) { g_err = "the last tile-parallel level ran without anchors: there is no anchor table"; return TWL_ERR_BAD_ARGUMENT; }
    HIP_TRY(hipSetDevice(d->id));
    HIP_TRY(hipStreamSynchronize(d->stream));
    const size_t np = (size_t)m.n_run, ns = np * (size_t)m.slots;
    if (dims) *dims = m;
    if (order) std::copy(d->mt_order.begin(), d->mt_order.end(), order);
    if (np == 0) return TWL_OK;
    if (anchor) HIP_TRY(hipMemcpy(anchor, d->mt_anchor.p, ns * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (spath) HIP_TRY(hipMemcpy(spath, d->mt_spath.p, np * (size_t)m.sp_pitch * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (chain) HIP_TRY(hipMemcpy(chain, d->mt_chain.p, ns * 2 * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (rec) HIP_TRY(hipMemcpy(rec, d->mt_rec.p, ns * twl::kMtRec * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (seg) HIP_TRY(hipMemcpy(seg, d->mt_seg.p, ns * (size_t)m.segcap, hipMemcpyDeviceToHost));
    if (front) HIP_TRY(hipMemcpy(front, (const unsigned long long *)d->mt_stat.p + 4, np * 8 * sizeof(int32_t), hipMemcpyDeviceToHost));      // (behind the four counters: launch_mt, mt_front)
    return TWL_OK;
}

// Tile-parallel alignment of a level with few pairs (talco_nuc.hip.h, MT kernels): scouts, then rounds of chain -> tiles -> stitch, on `st`.
// `order` = the pairs that run, h_len their lengths on the host.  Scouts and tiles run on the 16-wave geometry (one workgroup per CU, the
// shortest diagonal step) while they fit the device at once (one workgroup per CU), on the throughput geometry (8 waves x 2 blocks, two per CU) beyond.

template <int P, int MM, int TRPL, bool WIDE = false, int TW = 8>      // TW x TRPL: waves and 64-row blocks per wave of the throughput geometry (nucleotide 4 x 3: 768 rows, four workgroups per CU; protein 8 x 1: 512 rows, two)
int launch_mt(Device *d, hipStream_t st, const twl::KArgs &base, const int32_t *d_items, const std::vector<int32_t> &order, int n_run,
              const int32_t *h_len, int *grid_out, int *window_out, bool small_tiles = false, int sp = 0)
{
    constexpr bool kCanSmall = (P == 6 && TW == 4 && !WIDE);
    // WIDE (nucleotide): the tiles and the stitch launch on 16 waves x 3 blocks, a 3072-row window -- for the pairs whose band outgrew the
    // 1024-row window of the fast geometries.  Until round 4 those ran their ~20 tiles one after the other on the 2048- and 4608-row kernels
    // (0.2-0.6 s per 10 kbp pair); their tiles are as independent as anybody's.  The scouts keep the narrow geometry: a scout's band opens
    // from one cell by a row per diagonal over the ~400 diagonals it runs.
    constexpr int SW = 16, SR = WIDE ? 3 : 1;       // geometry of the stitch launch and of tiles while they fit the device at once
    if (window_out) *window_out = twl::NCfg<SW, SR>::WINDOW;
    TileFacts f;
    f.P = P; f.mm = MM; f.tw = TW; f.trpl = TRPL; f.stitch_rpl = SR; f.wide = WIDE; f.can_small = kCanSmall; f.small_tiles = small_tiles;
    f.n_run = n_run; f.marker = base.marker; f.seq_len = base.seq_len; f.rec_words = twl::kMtRec; f.order = order.data(); f.h_len = h_len;
    const Knobs k = current_knobs();
    const TilePlan pl = plan_tile_level(f, k, d->mt_jobs_host);       // (the jobs are kept with the device: their upload is asynchronous)
    int rc;
    if ((rc = prepare_mt_tables(d, st, pl, d->mt_jobs_host))) return rc;
    remember_mt_plan(d, pl, order, n_run, base.marker);
    twl::NArgs a = lean_args(d, base);
    a.items = d_items;
    a.mt_chain = (int32_t *)d->mt_chain.p; a.mt_rec = (int32_t *)d->mt_rec.p; a.mt_seg = (int8_t *)d->mt_seg.p; a.mt_spath = (int32_t *)d->mt_spath.p;
    a.mt_stat = (unsigned long long *)d->mt_stat.p;
    a.mt_front = (int32_t *)((unsigned long long *)d->mt_stat.p + 4);
    a.mt_slots = pl.slots; a.mt_segcap = pl.segcap; a.mt_sp_pitch = pl.sp_pitch; a.mt_lead = k.mt_lead; a.mt_marg = pl.marg;
    TRACE("launch mt pairs=%d scouts=%d tiles=%d slots=%d geometry=%s", n_run, pl.nScout, pl.nTile, pl.slots, WIDE ? "16x3 (wide)" : (pl.thr ? "throughput geometry" : "16x1"));
    if (!d->kname[0]) tile_level_name(d->kname, sizeof d->kname, f, pl);
    if constexpr (WIDE) {
        // pairs that outgrew the fast window are, more often than not, pairs whose tiles converge late or never (diffuse profiles): a tile then runs
        // to the end of the pair and the next one starts where the path from the END cell crosses the marker diagonal -- nothing a scout that
        // starts 320 diagonals ahead can know.  One workgroup per pair runs the whole DP once with every traceback word kept (MT 4) and leaves the
        // global path's crossing of every anti-diagonal; its suffixes are what the tiles' own paths follow.
        if constexpr (P == 6) {
            twl::NArgs as = a;
            as.xdrop = (int32_t)((long long)a.xdrop * g_scout_xdrop_pct / 100);
            if ((rc = launch_mt_kernel<P, SW, SR, MM, 1, 4>(d, st, as, n_run, nullptr, pl.tb_groups))) return rc;
        }
    } else if (pl.nScout > 0) {
        a.mt_jobs = (const int32_t *)d->mt_jobs.p;
        if (pl.anchors) {
            FILL_TRY(flush_fills(d, st));
            hipLaunchKernelGGL(twl::mt_anchor_kernel<P>, dim3(pl.nScout), dim3(256), 0, st, base.cols, base.len, base.seq_len, a.mt_jobs, pl.nScout, (int32_t *)d->mt_anchor.p, pl.slots, base.marker, pl.lead2);
            HIP_TRY(hipGetLastError());
            a.mt_anchor = (const int32_t *)d->mt_anchor.p; a.mt_lead2 = pl.lead2;
        }
        // Nucleotide scouts of the throughput geometry take the 512-row window (4 waves x 2 blocks, FIVE workgroups per CU, see plan_nucleotide) whatever the
        // tiles need.  The scout of boundary `slot` runs min(slot + 2 + marg + lead, kMaxMarker) anti-diagonals from one cell (talco_lean_kernel, MT 2: its marker is
        // spHi + mt_marg - scoutD0, spHi - spLo = slot + 2, lead = mt_lead2 when it is anchored and mt_lead when not), and the premise is that its band opens by
        // about a row per diagonal.  With the knobs' defaults that is at most 320 + 40 + 2 + slot = 362 + slot rows, and 320 + 64 + 2 + slot = 386 + slot with the
        // longer margin of the levels of at most 2048 tile jobs: within 512 rows up to boundary 126 (pairs of ~129 000 columns at marker 1024), past it beyond.
        // A scout that outgrows the window predicts nothing, and the tile it was to start costs a tile in line or a second round.
        if constexpr (kCanSmall) rc = pl.thr ? launch_mt_thr<4, 2, MM, 5, 2>(d, st, a, pl.nScout, nullptr, sp) : launch_mt_kernel<P, SW, SR, MM, 1, 2>(d, st, a, pl.nScout);
        else rc = pl.thr ? launch_mt_kernel<P, TW, TRPL, MM, 4, 2>(d, st, a, pl.nScout) : launch_mt_kernel<P, SW, SR, MM, 1, 2>(d, st, a, pl.nScout);
        if (rc) return rc;
    }
    for (int r = 0; r < pl.rounds; ++r) {
        FILL_TRY(flush_fills(d, st));
        hipLaunchKernelGGL(twl::mt_chain_kernel, dim3((n_run + 63) / 64), dim3(64), 0, st, (const int32_t *)d->mt_spath.p, pl.sp_pitch, base.len, d_items, n_run,
                           (int32_t *)d->mt_chain.p, pl.slots, base.marker, g_mt_perturb, (const int32_t *)a.mt_front);
        HIP_TRY(hipGetLastError());
        a.mt_jobs = (const int32_t *)d->mt_jobs.p + 3 * (size_t)pl.nScout;
        if constexpr (kCanSmall) rc = pl.thr ? (pl.smallT ? launch_mt_thr<4, 2, MM, 5, 1>(d, st, a, pl.nTile, grid_out, sp) : launch_mt_thr<TW, TRPL, MM, 4, 1>(d, st, a, pl.nTile, grid_out, sp))
                                             : launch_mt_kernel<P, SW, SR, MM, 1, 1>(d, st, a, pl.nTile, grid_out);
        else rc = pl.thr ? launch_mt_kernel<P, TW, TRPL, MM, 4, 1>(d, st, a, pl.nTile, grid_out) : launch_mt_kernel<P, SW, SR, MM, 1, 1>(d, st, a, pl.nTile, grid_out);
        if (rc) return rc;
        a.mt_jobs = nullptr;
        a.mt_inline = (r == pl.rounds - 1) ? 1 : 0;
        a.dbg = a.mt_inline ? base.dbg : nullptr;
        if ((rc = launch_mt_kernel<P, SW, SR, MM, 1, 3>(d, st, a, n_run))) return rc;
    }
    return TWL_OK;
}
