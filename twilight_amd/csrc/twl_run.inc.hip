// twilight_amd/csrc/twl_run.inc.hip -- one DP call on a device (run_device): a short driver over named steps -- order the pairs, prepare the arguments, first launch (by plan),
// collect, re-run ladder (next_rung), global-memory stage, remember (PassMemory), fill twl_stats.  What the policy decides is in twl_policy.inc.hip, how a kernel family is launched in twl_launch.inc.hip.
// Included by twl_align.hip (one translation unit: it shares that file's Device bookkeeping, error string and fill queue).

// What every step of one call is given: the caller's arguments, the cost order and the kernel arguments made of them.
struct Call {
    Device *d; hipStream_t st; const twl_params *p;
    int32_t n_pairs, seq_len;
    const int32_t *d_len, *d_num; int32_t *d_alnlen; int16_t *d_err;
    const int32_t *h_len;                 // [pair][2] on the host: the caller's, or len_host
    std::vector<int32_t> len_host, order; // order: longest first, the pairs that do not run last
    int32_t n_run = 0;                    // the pairs that run (both sides non-empty): order[0 .. n_run)
    uint64_t nominal = 0;                 // sum of R x Q
    twl::KArgs a{};
    const int32_t *items() const { return (const int32_t *)d->items.p; }
    long long len_sum(int32_t pr) const { return (long long)h_len[2 * pr] + h_len[2 * pr + 1]; }
};
// The per-pair results as the host last read them, and the tile-parallel counters of the call.
struct Results { std::vector<int16_t> err; std::vector<unsigned long long> cells; unsigned long long mt[4] = {0, 0, 0, 0}; };

// A pinned host block of at least `bytes` (grown by half when it has to grow).
int pinned_at_least(void **h, size_t *cap, size_t bytes)
{
    if (bytes <= *cap) return TWL_OK;
    if (*h) (void)hipHostFree(*h);
    *h = nullptr; *cap = 0;
    HIP_TRY(hipHostMalloc(h, bytes + bytes / 2, hipHostMallocDefault));
    *cap = bytes + bytes / 2;
    return TWL_OK;
}

// The run-time matrix mode as a template argument, among the modes the launch site names and no other (nothing else is instantiated); the last one named is the default.
template <int MM0, int... MMs, class F>
int with_mm(int mode, F &&f)
{
    if constexpr (sizeof...(MMs) == 0) return f(std::integral_constant<int, MM0>{});
    else return mode == MM0 ? f(std::integral_constant<int, MM0>{}) : with_mm<MMs...>(mode, f);
}
#define MM_OF(x) decltype(x)::value

// Step 1: cost order, longest first (LPT) so the persistent workgroups finish together; the order goes up to d->items.
int order_pairs(Call &c)
{
    const int32_t n_pairs = c.n_pairs;
    if (!c.h_len) {      // len/num are needed on the host for cost ordering (they are tiny)
        c.len_host.resize((size_t)n_pairs * 2);
        HIP_TRY(hipMemcpyAsync(c.len_host.data(), c.d_len, c.len_host.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c.st));
        HIP_TRY(hipStreamSynchronize(c.st));
        c.h_len = c.len_host.data();
    }
    const int32_t *h_len = c.h_len;
    c.order.resize((size_t)n_pairs);
    std::iota(c.order.begin(), c.order.end(), 0);
    // (pairs with an empty side -- masked out by the caller, or really empty -- come last and are not launched at all: what the geometry
    // is chosen by is the number of pairs that run, e.g. a rank's share of a level)
    auto live = [h_len](int32_t x) { return h_len[2 * x] > 0 && h_len[2 * x + 1] > 0; };
    std::stable_sort(c.order.begin(), c.order.end(), [&](int32_t x, int32_t y) {
        if (live(x) != live(y)) return live(x);
        return (int64_t)h_len[2 * x] + h_len[2 * x + 1] > (int64_t)h_len[2 * y] + h_len[2 * y + 1];
    });
    for (int32_t n = 0; n < n_pairs; ++n) c.n_run += live(n) ? 1 : 0;
    for (int32_t n = 0; n < n_pairs; ++n) c.nominal += (uint64_t)std::max(0, h_len[2 * n]) * (uint64_t)std::max(0, h_len[2 * n + 1]);
    HIP_TRY(hipMemcpyAsync(c.d->items.p, c.order.data(), c.order.size() * sizeof(int32_t), hipMemcpyHostToDevice, c.st));
    return TWL_OK;
}

// Step 2: the packing launch (between ev[0] and ev[1]), the kernel arguments, the per-pair gap-character flags, the debug buffer and the fills of the outputs.
int prepare_args(Call &c, const float *d_freq, const float *d_gop, const float *d_gex, int8_t *d_aln, const float *d_packed, const uint8_t *h_gc_zero)
{
    Device *d = c.d; hipStream_t st = c.st; const twl_params *p = c.p; const int32_t n_pairs = c.n_pairs;
    int rc;
    TRACE("run_device n_pairs=%d seq_len=%d", n_pairs, c.seq_len);
    HIP_TRY(hipEventRecord(d->ev[0], st));
    if (!d_packed) {
        const size_t n_cols = (size_t)n_pairs * 2 * (size_t)c.seq_len;
        const int threads = 256;
        const int blocks = (int)std::min<size_t>((n_cols + threads - 1) / threads, (size_t)d->num_cu * 8);
        if (p->P == 22) hipLaunchKernelGGL(twl::pack_kernel<22>, dim3(std::max(blocks, 1)), dim3(threads), 0, st, d_freq, d_gop, d_gex, (float *)d->cols.p, n_cols);
        else hipLaunchKernelGGL(twl::pack_kernel<6>, dim3(std::max(blocks, 1)), dim3(threads), 0, st, d_freq, d_gop, d_gex, (float *)d->cols.p, n_cols);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(d->ev[1], st));
    if (dbg_on()) { HIP_TRY(hipStreamSynchronize(st)); TRACE("pack done"); }

    twl::KArgs &a = c.a;
    a.cols = d_packed ? d_packed : (const float *)d->cols.p;
    a.len = c.d_len; a.num = c.d_num;
    a.aln = d_aln; a.aln_len = c.d_alnlen; a.err = c.d_err;
    a.cells = (unsigned long long *)d->cells.p;
    a.queue = (int32_t *)d->queue.p;
    a.seq_len = c.seq_len;
    a.n_pairs_total = n_pairs;
    a.gap_open = p->gap_open; a.gap_extend = p->gap_extend; a.gap_char = p->gap_char;
    a.gc_zero = nullptr;
    if (h_gc_zero && p->gap_char != 0.0f && std::any_of(h_gc_zero, h_gc_zero + n_pairs, [](uint8_t z) { return z != 0; })) {
        if ((rc = d->gc_zero.ensure((size_t)n_pairs))) return rc;
        d->gc_zero_host.assign(h_gc_zero, h_gc_zero + n_pairs);       // (kept with the device: the upload is asynchronous)
        HIP_TRY(hipMemcpyAsync(d->gc_zero.p, d->gc_zero_host.data(), (size_t)n_pairs, hipMemcpyHostToDevice, st));
        a.gc_zero = (const uint8_t *)d->gc_zero.p;
    }
    a.xdrop = p->xdrop; a.flen = p->flen; a.marker = p->marker;
    a.step_slack = 1 << 16;
    a.dbg = nullptr;
    if (dbg_on()) {
        if ((rc = d->dbg.ensure((size_t)n_pairs * 16 * sizeof(int32_t) + 2048 + 16 * 192 * 32))) return rc;     // per-pair records, then the stamp build's sums and timeline
        HIP_TRY(hipMemsetAsync(d->dbg.p, 0xff, (size_t)n_pairs * 16 * sizeof(int32_t), st));
        a.dbg = (int32_t *)d->dbg.p;
    }
    { const int ms = p->P - 1; for (int l = 0; l < ms; ++l) for (int m = 0; m < ms; ++m) a.M[ms * l + m] = p->matrix[ms * l + m]; }
    // the pairs that do not run: path length 0, errorType 0, no cells
    FILL_TRY(queue_fill(d, st, c.d_alnlen, (size_t)n_pairs * sizeof(int32_t), 0));
    FILL_TRY(queue_fill(d, st, c.d_err, (size_t)n_pairs * sizeof(int16_t), 0));
    FILL_TRY(queue_fill(d, st, d->cells.p, (size_t)n_pairs * sizeof(unsigned long long), 0));
    return TWL_OK;
}

// Step 3, protein: the first launch plan_protein names.
int first_protein(Call &c, Ran &ran, int *grid, int *window)
{
    Device *d = c.d; hipStream_t st = c.st; twl::KArgs &a = c.a; const int32_t *items = c.items(), *h_len = c.h_len; const int32_t n_run = c.n_run, n_pairs = c.n_pairs;
    int rc;
    ProtFacts pf;
    pf.n_run = n_run; pf.n_pairs = n_pairs; pf.num_cu = d->num_cu; pf.marker = c.p->marker; pf.M = a.M; pf.gap_char = c.p->gap_char; pf.dump = d->dump_on;
    pf.corridor_lost = d->mem.corridor_lost_for(n_run); pf.h_len = h_len; pf.order = c.order.data();
    const ProtPlan pl = plan_protein(pf, current_knobs());
    TRACE("plan: %s, matrix mode %d", prot_first_name(pl.first), pl.mm);
    ran.mode = pl.mm; ran.spec = pl.spec; ran.ranMt = pl.first == ProtFirst::MtPresim;
    ran.start = pl.small ? Level::Mid : Level::Wide;      // (the 512-row geometries have the 16-wave kernel ahead; everything else goes on to the widest kernel)
    if (pl.first == ProtFirst::R1) return launch_dp<22, 8, 1, false, true, true>(d, st, a, items, n_run, 0, grid, window);
    if (pl.first == ProtFirst::Dense) return launch_dp<22, 8, 2, false, true, true>(d, st, a, items, n_run, 0, grid, window);
    if ((rc = d->m24.ensure(21 * 24 * sizeof(float)))) return rc;
    std::vector<float> m24(21 * 24, 0.0f);
    for (int l = 0; l < 21; ++l) for (int m = 0; m < 21; ++m) m24[24 * l + m] = a.M[21 * l + m];
    HIP_TRY(hipMemcpyAsync(d->m24.p, m24.data(), m24.size() * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));      // m24 goes out of scope
    if (pl.presim) {
        // Scores do not depend on the DP state, so the otherwise idle CUs compute them for the whole R x Q matrix (or a corridor of it) first
        // (score_matrix_kernel, same arithmetic) and the DP kernel only loads them (matrix mode 4).
        std::vector<long long> off((size_t)n_pairs, 0);
        std::vector<int32_t> blk((size_t)n_pairs + 1, 0);
        long long floats = 0;
        for (int32_t t = 0; t < n_run; ++t) {
            const long long R = h_len[2 * c.order[t]], Q = h_len[2 * c.order[t] + 1];
            off[c.order[t]] = floats;
            floats += (R + Q) * ((Q + 63) & ~63ll);
            blk[t + 1] = blk[t] + (int32_t)(((R + Q - 1 + 63) / 64) * ((Q + 63) / 64));
        }
        if ((rc = d->sim.ensure(pl.simFloats * sizeof(float)))) return rc;
        if ((rc = d->sim_off.ensure(off.size() * sizeof(long long)))) return rc;
        if ((rc = d->blk_off.ensure(blk.size() * sizeof(int32_t)))) return rc;
        HIP_TRY(hipMemcpyAsync(d->sim_off.p, off.data(), off.size() * sizeof(long long), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d->blk_off.p, blk.data(), blk.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));      // the host vectors above go out of scope
        twl::ScoreArgs sa{};
        sa.cols = a.cols; sa.len = c.d_len; sa.num = c.d_num; sa.items = items; sa.blk_off = (const int32_t *)d->blk_off.p;
        sa.n_items = n_run; sa.seq_len = c.seq_len; sa.gap_char = c.p->gap_char; sa.gc_zero = a.gc_zero; sa.M24 = (const float *)d->m24.p;
        sa.sim = (float *)d->sim.p; sa.sim_off = (const long long *)d->sim_off.p;
        d->mem.begin_corridor_level(n_run);
        sa.corridor = pl.corridor;
        ran.usedCorridor = sa.corridor > 0;
        FILL_TRY(flush_fills(d, st));
        hipLaunchKernelGGL(twl::score_matrix_kernel<22>, dim3((unsigned)blk[n_run]), dim3(256), 0, st, sa);
        HIP_TRY(hipGetLastError());
        a.sim = (const float *)d->sim.p;
        a.sim_off = (const long long *)d->sim_off.p;
        // what twl_dp_score_matrix reads back: host integers only
        d->sim_last_off.assign((size_t)n_pairs, -1);
        for (int32_t t = 0; t < n_run; ++t) d->sim_last_off[(size_t)c.order[t]] = off[(size_t)c.order[t]];
        d->sim_last_len.assign(h_len, h_len + 2 * (size_t)n_pairs);
        d->sim_last_corridor = sa.corridor;
    }
    switch (pl.first) {
    case ProtFirst::MtPresim: return launch_mt<22, 4, 1>(d, st, a, items, c.order, n_run, h_len, grid, window);
    case ProtFirst::SpecShared: return launch_lean<22, 8, 1, 4, 4, true>(d, st, a, items, n_run, grid, window);
    case ProtFirst::Spec16: return launch_lean<22, 16, 1, 4, 1, true>(d, st, a, items, n_run, grid, window);
    case ProtFirst::Plain16: return launch_lean<22, 16, 1, 4, 1>(d, st, a, items, n_run, grid, window);
    case ProtFirst::Dump:      // twl_dp_column_scores: the sparse in-kernel score loop, every visited cell written out
        if (!pl.lean || n_run != 1) { g_err = "score dump: one pair, matrix within the fast-division range"; return TWL_ERR_UNSUPPORTED; }
        return launch_lean<22, 16, 1, 3, 1, false, true>(d, st, a, items, n_run, grid, window);
    case ProtFirst::Thr512: return launch_lean<22, 8, 1, 3, 4>(d, st, a, items, n_run, grid, window);
    case ProtFirst::Sparse16: return launch_lean<22, 16, 1, 3, 1>(d, st, a, items, n_run, grid, window);
    default: return pl.presim ? launch_dp<22, 8, 2, false, true, true, 1, 4>(d, st, a, items, n_run, 0, grid, window)
                              : launch_dp<22, 8, 2, false, true, true, 1, 3>(d, st, a, items, n_run, 0, grid, window);
    }
}

// The sample of a throughput level with nothing remembered: one pair per CU, every (bulk / CUs)-th of the cost order, moved to the front of the launch order, runs on the
// 512-row window; *small = at most 1 % of them outgrew it.  *done = the pairs of the bulk the sample took.
int sample_small_window(Call &c, const NucPlan &pl, Ran &ran, int *grid, int *window, bool *small, int *done)
{
    Device *d = c.d; hipStream_t st = c.st; std::vector<int32_t> &order = c.order; const int bulk = pl.bulk;
    const int S = d->num_cu;
    std::vector<int32_t> front, rest;
    front.reserve((size_t)S); rest.reserve((size_t)bulk);
    for (int t = 0, nextPick = 0, j = 0; t < bulk; ++t) {
        if (j < S && t == nextPick) { front.push_back(order[t]); ++j; nextPick = (int)((long long)j * bulk / S); }
        else rest.push_back(order[t]);
    }
    std::copy(front.begin(), front.end(), order.begin());
    std::copy(rest.begin(), rest.end(), order.begin() + (std::ptrdiff_t)front.size());
    HIP_TRY(hipMemcpyAsync(d->items.p, order.data(), (size_t)bulk * sizeof(int32_t), hipMemcpyHostToDevice, st));
    *done = (int)front.size();
    FILL_TRY((launch_thr<4, 2, 5>(d, st, c.a, c.items(), *done, grid, window, pl.mm5, pl.sp)));
    FILL_TRY(pinned_at_least(&d->probe_h, &d->probe_cap, (size_t)c.n_pairs * sizeof(int16_t)));
    HIP_TRY(hipMemcpyAsync(d->probe_h, c.d_err, (size_t)c.n_pairs * sizeof(int16_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    int outgrew = 0;
    for (int32_t pr : front) outgrew += ((const int16_t *)d->probe_h)[pr] == twl::kErrOverflow ? 1 : 0;
    *small = outgrew * 100 <= 1 * *done;
    d->mem.small_state = *small ? 1 : -1;      // (the levels that follow in this pass do as this one did)
    ran.probed = !*small;                      // (a sample that said yes leaves the verdict to the whole level, PassMemory::update)
    TRACE("sample of %d pairs on the 512-row window: %d outgrew it -> the level runs on %d rows", *done, outgrew, *small ? 512 : 768);
    d->kname[0] = 0;                           // (the level's kernel is the one the rest runs on)
    return TWL_OK;
}

// The throughput launch of a nucleotide level: (sample,) bulk in rounds of persistent workgroups, remainder through the tile-parallel path.
int first_throughput(Call &c, const NucPlan &pl, Ran &ran, int *grid, int *window)
{
    // Default matrix structure (modes 2 and 5): 4 waves x 3 blocks, a 768-row window, FOUR workgroups per CU (round 4: the same 16 waves per CU as
    // 8 waves x 2 blocks twice, but four independent anti-diagonal chains per SIMD instead of two, a barrier of four waves instead of eight, and no
    // first products kept per row -- 2048 pairs of 10 kbp 120 -> 95 ms, a leaf level 96 -> 66 ms, tools/exp_thr.py); a pair whose band outgrows 640
    // rows re-runs on 8 waves x 2 blocks (1024 rows) by the ladder.
    Device *d = c.d; hipStream_t st = c.st; const int32_t *items = c.items(); const int bulk = pl.bulk, tail = pl.tail;
    bool small = pl.small;
    int done = 0, rc;
    if (pl.probe && bulk >= 8 * d->num_cu && (rc = sample_small_window(c, pl, ran, grid, window, &small, &done))) return rc;
    // The remainder beside the bulk (TWL_KNOB_TAIL_OVERLAP): the bulk's workgroups take one or two whole pairs each and end spread over the last milliseconds of the
    // launch; the remainder's scouts and tile jobs, 0.15-2.3 ms each and handed out by a counter, take the slots they free.  The bulk is enqueued first, on the
    // stream of higher priority; the remainder's stream starts from what is in front of the bulk kernel (launch_lean, fork_next) and the call's stream waits for its
    // last launch before anything reads a result.  What the two would share and the bulk still uses is the remainder's own: Device::tail_side.
    const bool beside = tail > 0 && g_tail_overlap != 0;
    d->fork_next = beside;
    if (pl.four) rc = small ? launch_thr<4, 2, 5>(d, st, c.a, items + done, bulk - done, grid, window, pl.mm5, pl.sp)
                            : launch_thr<4, 3, 4>(d, st, c.a, items + done, bulk - done, grid, window, pl.mm5, pl.sp);
    else rc = with_mm<1, 0>(pl.mm, [&](auto MM) { return launch_lean<6, 8, 2, MM_OF(MM), 2>(d, st, c.a, items, bulk, grid, window); });
    // (after a sample that said no, its own pairs that outgrew 512 rows go straight on to the 1024-row window with the rest's)
    ran.start = small ? Level::From512 : (pl.four ? Level::From768 : Level::Mid);
    const bool forked = beside && !d->fork_next;      // (the bulk kernel was launched with the fork event in front of it)
    d->fork_next = false;
    if (rc || tail <= 0) return rc;
    const std::vector<int32_t> tailOrder(c.order.begin() + bulk, c.order.begin() + c.n_run);
    int g2 = 0, w2 = 0;
    ran.smallTiles = small && !ran.probed;
    ran.ranMt = true;
    hipStream_t ts = forked ? d->tail_stream : st;
    if (forked) HIP_TRY(hipStreamWaitEvent(d->tail_stream, d->tail_ev[0], 0));
    d->tail_side = forked;
    // (one-letter query rows: the tiles too take the four-product form of the column score)
    rc = with_mm<5, 2>(ran.mode, [&](auto MM) { return launch_mt<6, MM_OF(MM), 3, false, 4>(d, ts, c.a, items + bulk, tailOrder, tail, c.h_len, &g2, &w2, ran.smallTiles, pl.sp); });
    d->tail_side = false;
    if (!forked) return rc;
    // the join, also behind a remainder that failed half way: what it did launch is waited for before the call returns its error and a buffer is touched again
    if (!rc) rc = flush_fills(d, ts);
    else d->fills.n = 0;
    if (hipEventRecord(d->tail_ev[1], ts) != hipSuccess || hipStreamWaitEvent(st, d->tail_ev[1], 0) != hipSuccess) {
        (void)hipStreamSynchronize(ts);
        if (!rc) { g_err = "the join of a level's remainder with its bulk launch failed"; rc = TWL_ERR_HIP; }
    }
    return rc;
}

// Step 3, nucleotide: the first launch plan_nucleotide names.
int first_nucleotide(Call &c, bool qry_onehot, int shape, Ran &ran, int *grid, int *window)
{
    Device *d = c.d; hipStream_t st = c.st; const twl::KArgs &a = c.a; const int32_t *items = c.items(); const int32_t n_run = c.n_run;
    NucFacts nf;
    nf.n_run = n_run; nf.num_cu = d->num_cu; nf.marker = c.p->marker; nf.M = a.M; nf.gap_char = c.p->gap_char; nf.qry_onehot = qry_onehot; nf.shape = shape; nf.dump = d->dump_on;
    nf.remember(d->mem); nf.h_len = c.h_len; nf.order = c.order.data();
    const NucPlan pl = plan_nucleotide(nf, current_knobs());
    if (pl.first == NucFirst::Throughput && (pl.small || pl.held_back)) d->mem.begin_small_level(n_run);
    const int mode = pl.mm5 ? 5 : pl.mm;
    ran.mode = mode;
    ran.leanMid = pl.lean && pl.mm == 2;
    ran.start = Level::Mid;
    TRACE("plan: %s%s, matrix mode %d%s", nuc_first_name(pl.first), pl.small ? " (512-row window, five workgroups per CU)" : "", pl.mm, pl.mm5 ? " (one-letter query rows)" : "");
    switch (pl.first) {
    case NucFirst::Dump:      // twl_dp_column_scores: the same kernel code with the score of every visited cell written out
        if (!pl.lean || n_run != 1) { g_err = "score dump: one pair, matrix within the fast-division range"; return TWL_ERR_UNSUPPORTED; }
        return with_mm<5, 2, 1, 0>(mode, [&](auto MM) { return launch_lean<6, 16, 1, MM_OF(MM), 1, false, true>(d, st, a, items, n_run, grid, window); });
    case NucFirst::WideMt:    // (a call that starts on the 3072-row geometry goes on to the widest kernel)
        ran.spec = 3; ran.ranMt = true; ran.startedWide = true; ran.start = Level::Wide;
        return launch_mt<6, 2, 3, true, 4>(d, st, a, items, c.order, n_run, c.h_len, grid, window);
    case NucFirst::Mt:        // few pairs of many tiles each: all tiles of all pairs side by side from predicted starts (talco_nuc.hip.h, MT kernels)
        ran.smallTiles = nf.small_state > 0;      // (the throughput levels of this pass fitted the 512-row window: so do the tiles of their pairs' descendants, until they do not)
        ran.spec = 3; ran.ranMt = true;
        return launch_mt<6, 2, 3, false, 4>(d, st, a, items, c.order, n_run, c.h_len, grid, window, ran.smallTiles, pl.sp);
    case NucFirst::SpecShared:
        ran.mode = 2; ran.spec = 2;
        return launch_lean<6, 8, 2, 2, 4, true>(d, st, a, items, n_run, grid, window);
    case NucFirst::Spec16:
        ran.spec = 1;
        return with_mm<5, 2>(mode, [&](auto MM) { return launch_lean<6, 16, 1, MM_OF(MM), 1, true>(d, st, a, items, n_run, grid, window); });
    case NucFirst::Few16:
        return with_mm<5, 2, 1, 0>(mode, [&](auto MM) { return launch_lean<6, 16, 1, MM_OF(MM), 1>(d, st, a, items, n_run, grid, window); });
    case NucFirst::Throughput:
        return first_throughput(c, pl, ran, grid, window);
    default:                  // scores outside the fast division's range: the round-1 kernels (IEEE division)
        return with_mm<2, 1, 0>(pl.mm, [&](auto MM) { return launch_dp<6, 8, 2, false, true, true, 4, MM_OF(MM)>(d, st, a, items, n_run, 0, grid, window); });
    }
}

// Step 4: error codes, path lengths, band cells and the tile-parallel counters come back in ONE synchronisation (one small kernel writes them into a pinned host
// block: three device-to-host copies into pageable memory before).  withCells: the band cells too; mt: where to put the four counters, or null.
int collect(Call &c, bool withMt, Results &res, bool withCells, unsigned long long *mt)
{
    Device *d = c.d; const int32_t n_pairs = c.n_pairs;
    hipLaunchKernelGGL(twl::collect_kernel, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, c.st, (int)n_pairs, (const int16_t *)c.d_err, (const int32_t *)c.d_alnlen,
                       (const unsigned long long *)d->cells.p, withMt ? (const unsigned long long *)d->mt_stat.p : nullptr, (unsigned long long *)d->res_h);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c.st));
    const unsigned long long *r = (const unsigned long long *)d->res_h;
    const int32_t *rl = (const int32_t *)(r + 4 + n_pairs);
    const int16_t *re = (const int16_t *)(rl + n_pairs);
    std::copy(re, re + n_pairs, res.err.begin());
    d->last_alnlen.assign(rl, rl + n_pairs);
    if (withCells) std::copy(r + 4, r + 4 + n_pairs, res.cells.begin());
    if (mt) for (int t = 0; t < 4; ++t) mt[t] = r[t];      // (zeros when no tile-parallel launch ran)
    return TWL_OK;
}

// One rung of the ladder on the pairs in `redo` (already in d->items).
int launch_rung(Call &c, const Ran &ran, Rung rung, const std::vector<int32_t> &redo, int *g, int *w)
{
    Device *d = c.d; hipStream_t st = c.st; const twl::KArgs &a = c.a; const int32_t *it = c.items(); const int n = (int)redo.size();
    switch (rung) {
    case Rung::Guard:        return ran.prot ? launch_dp<22, 8, 2, false, true, true, 1, 3>(d, st, a, it, n, 0, g, w) : launch_dp<6, 16, 2, false, true, true, 1, 0>(d, st, a, it, n, 0, g, w);
    case Rung::Thr768:       return with_mm<5, 2>(ran.mode, [&](auto MM) { return launch_lean<6, 4, 3, MM_OF(MM), 4>(d, st, a, it, n, g, w); });
    case Rung::MtStitch1024: return with_mm<5, 2>(ran.mode, [&](auto MM) { return launch_mt<6, MM_OF(MM), 3, false, 4>(d, st, a, it, redo, n, c.h_len, g, w); });
    case Rung::Lean1024:     return with_mm<5, 2>(ran.mode, [&](auto MM) { return launch_lean<6, 8, 2, MM_OF(MM), 4>(d, st, a, it, n, g, w); });
    case Rung::Prot16:       return launch_lean<22, 16, 1, 3, 1>(d, st, a, it, n, g, w);
    case Rung::Mt3072:       return launch_mt<6, 2, 3, true, 4>(d, st, a, it, redo, n, c.h_len, g, w);
    case Rung::Lean2048:     return launch_lean<6, 8, 4, 2, 2>(d, st, a, it, n, g, w);
    case Rung::Ieee16x2:     return launch_dp<6, 16, 2, false, true, true, 1, 0>(d, st, a, it, n, 0, g, w);
    case Rung::Wide4608:     return ran.prot ? launch_dp<22, 8, 9, false, false, false>(d, st, a, it, n, 1, g, w) : launch_dp<6, 8, 9, false, false, true>(d, st, a, it, n, 1, g, w);
    default:                 return ran.prot ? launch_global<22>(d, st, a, it, n, c.seq_len, g, w) : launch_global<6>(d, st, a, it, n, c.seq_len, g, w);
    }
}
// A timed re-run stage: the pairs go up, the rung runs between ev[3] and ev[4], the host waits, the milliseconds, the launch and the pairs are counted.
int timed_rerun(Call &c, const Ran &ran, Rung rung, const std::vector<int32_t> &redo, float *ms_redo, int *window)
{
    Device *d = c.d;
    HIP_TRY(hipMemcpyAsync(d->items.p, redo.data(), redo.size() * sizeof(int32_t), hipMemcpyHostToDevice, c.st));
    HIP_TRY(hipEventRecord(d->ev[3], c.st));
    int grid2 = 0;
    TRACE("re-run: %d pairs on %s", (int)redo.size(), rung_name(rung));
    FILL_TRY(launch_rung(c, ran, rung, redo, &grid2, window));
    HIP_TRY(hipEventRecord(d->ev[4], c.st));
    HIP_TRY(hipStreamSynchronize(c.st));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, d->ev[3], d->ev[4]));
    *ms_redo += ms;
    d->stats.n_launches += 1;
    d->stats.n_relaunched += (int32_t)redo.size();
    return TWL_OK;
}
std::vector<int32_t> pairs_with(const std::vector<int16_t> &err, int16_t code, int16_t code2)
{
    std::vector<int32_t> v;
    for (int32_t n = 0; n < (int32_t)err.size(); ++n) if (err[n] == code || err[n] == code2) v.push_back(n);
    return v;
}

// Step 5: pairs whose band outgrew a window are re-run, bit-identically, on the next rung (next_rung: 512 -> 768 -> 1024 -> 2048 / tile-parallel 3072 -> 4608 rows);
// first, on every round, the pairs with an operand outside the fast division's range (lean kernels only): the IEEE-division kernel.  When nothing has to be
// re-run -- the common case -- the first collect is the call's only synchronisation here.
int climb_ladder(Call &c, const Ran &ran, Results &res, LadderOutcome &o, float *ms_redo)
{
    const Knobs k = current_knobs();
    int rc, w2 = 0;
    if ((rc = collect(c, ran.ranMt, res, true, ran.ranMt ? res.mt : nullptr))) return rc;
    TRACE("dp kernel done");
    o.firstInline = res.mt[1];
    for (Level at = ran.start; at != Level::Global;) {
        std::vector<int32_t> redo = pairs_with(res.err, twl::kErrGuard, twl::kErrGuard);
        const RedoKind kind = redo.empty() ? RedoKind::Overflow : RedoKind::Guard;
        if (kind == RedoKind::Overflow) redo = pairs_with(res.err, twl::kErrOverflow, twl::kErrOverflow);
        if (redo.empty()) break;
        RedoFacts f;
        f.count = (int)redo.size(); f.marker = c.p->marker; f.dump = c.d->dump_on;
        for (int32_t n : redo) f.sumLen += c.len_sum(n);
        const Step s = next_rung(ran, at, kind, f, k);
        if (kind == RedoKind::Guard) o.guardRound = true;
        else if (at == Level::From512) o.from512Pairs = f.count;
        if (s.rung == Rung::Mt3072 || s.rung == Rung::Lean2048) o.widePairs += f.count;
        if (s.rung == Rung::Mt3072 || s.rung == Rung::MtStitch1024) o.redoMt = true;      // (what outgrows the 1024-row stitch goes on to the 3072-row rung)
        if ((rc = timed_rerun(c, ran, s.rung, redo, ms_redo, &w2))) return rc;
        o.relaunched += f.count;
        at = s.next;
        if (at != Level::Global && (rc = collect(c, ran.ranMt || o.redoMt, res, false, nullptr))) return rc;
    }
    if (o.relaunched > 0) {      // band cells of the re-run pairs; the counters of the first launch are kept and those of a tile-parallel re-run added
        unsigned long long now[4];
        if ((rc = collect(c, ran.ranMt || o.redoMt, res, true, now))) return rc;
        if (o.redoMt) for (int t = 0; t < 4; ++t) res.mt[t] += now[t];
    }
    return TWL_OK;
}

// Step 6: a band that outgrew even the 4608-row window (only possible with flen > 4608, i.e. in a retry of the deferred pass, alignment-cpu.cpp:116-129), or an
// operand outside the fast division's range that met such a band: the global-memory kernel, which has no window and divides the IEEE way (round 5;
// TWL_ERR_UNSUPPORTED ended the run here before).  Only this stage raises twl_stats.window.
int global_stage(Call &c, const Ran &ran, Results &res, bool anyMt, float *ms_redo)
{
    const std::vector<int32_t> redo = pairs_with(res.err, twl::kErrOverflow, twl::kErrGuard);
    int rc, w2 = 0;
    if (!redo.empty()) {
        if ((rc = timed_rerun(c, ran, Rung::Global, redo, ms_redo, &w2))) return rc;
        c.d->stats.window = std::max(c.d->stats.window, w2);
        if ((rc = collect(c, anyMt, res, true, nullptr))) return rc;
    }
    if (!pairs_with(res.err, twl::kErrOverflow, twl::kErrGuard).empty()) { g_err = "internal: a re-run code survived the global-memory kernel"; return TWL_ERR_HIP; }
    return TWL_OK;
}

// Device-resident core of every DP call (C ABI, device-resident level path, placement).
int run_device(Device *d, hipStream_t st, const twl_params *p, int32_t n_pairs, int32_t seq_len, const float *d_freq,
               const float *d_gop, const float *d_gex, const int32_t *d_len, const int32_t *d_num, int8_t *d_aln,
               int32_t *d_alnlen, int16_t *d_err, const int32_t *h_len, const float *d_packed = nullptr, bool qry_onehot = false,
               const uint8_t *h_gc_zero = nullptr, int shape = 0)
{
    // h_gc_zero: optional [n_pairs], 1 = the pair's gapCharScore is 0 whatever p->gap_char says (the reference decides it per pair,
    // alignment-cpu.cpp:88; one launch then takes the pairs of both kinds -- the top levels of a 100 000-leaf tree hold a few of each)
    // shape: what the caller knows about EVERY pair that runs: 2 = single sequences on both sides (no gap letters, denominators of 1): the throughput kernels
    // then run a step without the per-block tests (talco_lean_kernel, SP 1)
    // qry_onehot: every query row of every pair of this call has at most one non-zero letter (single sequences: the device-resident
    // level path knows, it built the profiles) -- the nucleotide kernels then take the four-product form of the column score
    // d_packed: the level's columns already in the packed [P+2] layout (device-resident level path); no packing pass then
    HIP_TRY(hipSetDevice(d->id));
    d->stats = twl_stats{};
    d->kname[0] = 0;
    d->fills.n = 0;
    d->last_err.clear();
    d->last_alnlen.clear();
    d->sim_last_off.clear(); d->sim_last_len.clear(); d->sim_last_corridor = 0;      // (twl_dp_score_matrix: first_protein fills them in when it precomputes)
    d->pair_cells.assign((size_t)n_pairs, 0);
    if (n_pairs == 0) return TWL_OK;

    int rc;
    if (!d_packed && (rc = d->cols.ensure((size_t)n_pairs * 2 * (size_t)seq_len * (size_t)(p->P + 2) * sizeof(float)))) return rc;
    if ((rc = d->cells.ensure((size_t)n_pairs * sizeof(unsigned long long)))) return rc;
    if ((rc = d->queue.ensure(kQueueBytes))) return rc;      // (both blocks of work counters, before anything is launched: never reallocated under a running kernel)
    if ((rc = d->items.ensure((size_t)n_pairs * sizeof(int32_t)))) return rc;
    Call c{d, st, p, n_pairs, seq_len, d_len, d_num, d_alnlen, d_err, h_len};
    if ((rc = order_pairs(c))) return rc;
    if ((rc = prepare_args(c, d_freq, d_gop, d_gex, d_aln, d_packed, h_gc_zero))) return rc;

    Ran ran;
    ran.prot = (p->P == 22);
    ran.start = ran.prot ? Level::Wide : Level::Mid;
    int grid = 0, window = 0;
    if (c.n_run == 0) rc = TWL_OK;      // nothing to align in this call
    else if (g_force_global) {
        rc = ran.prot ? launch_global<22>(d, st, c.a, c.items(), c.n_run, seq_len, &grid, &window) : launch_global<6>(d, st, c.a, c.items(), c.n_run, seq_len, &grid, &window);
        snprintf(d->kname, sizeof d->kname, "talco_global_kernel<%d>", ran.prot ? 22 : 6);
    }
    else rc = ran.prot ? first_protein(c, ran, &grid, &window) : first_nucleotide(c, qry_onehot, shape, ran, &grid, &window);
    if (rc) return rc;
    FILL_TRY(flush_fills(d, st));      // (nothing ran: the outputs are still to be zeroed)
    HIP_TRY(hipEventRecord(d->ev[2], st));
    d->stats.n_launches = 1;
    d->stats.grid = grid;
    d->stats.window = window;
    d->stats.matrix_mode = ran.mode;
    d->stats.speculative = ran.spec;
    memcpy(d->stats.kernel, d->kname, sizeof d->stats.kernel);

    Results res;
    res.err.resize((size_t)n_pairs); res.cells.resize((size_t)n_pairs);
    LadderOutcome o;
    float ms_redo = 0.f;
    FILL_TRY(pinned_at_least((void **)&d->res_h, &d->res_cap, 4 * sizeof(unsigned long long) + (size_t)n_pairs * (sizeof(unsigned long long) + sizeof(int32_t) + sizeof(int16_t))));
    if ((rc = climb_ladder(c, ran, res, o, &ms_redo))) return rc;
    d->mem.update(ran, o, c.n_run, c.n_run > 0 ? c.len_sum(c.order[0]) : 0, current_knobs());
    if ((rc = global_stage(c, ran, res, ran.ranMt || o.redoMt, &ms_redo))) return rc;

    // work done by the abandoned fast-window attempts is real GPU work but not algorithmic cells: not counted
    uint64_t total = 0;
    for (int32_t n = 0; n < n_pairs; ++n) { d->pair_cells[n] = res.cells[n]; total += res.cells[n]; }
    if (ran.ranMt || o.redoMt) { d->stats.mt_tiles_predicted = (int32_t)res.mt[0]; d->stats.mt_tiles_inline = (int32_t)res.mt[1]; d->stats.mt_scouts_failed = (int32_t)res.mt[2]; }
    d->last_err = res.err;      // (twl_level_align hands them to its caller without another copy)
    // the global-memory kernel's scratch does not stay next to a resident store for the rest of the run (every launch of the call has been waited for)
    if (d->gtb.cap > ((size_t)256 << 20)) d->gtb.release();
    if (dbg_on()) {
        d->dbg_host.resize((size_t)n_pairs * 16);
        HIP_TRY(hipMemcpy(d->dbg_host.data(), d->dbg.p, d->dbg_host.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int32_t n = 0; n < n_pairs && n < 64; ++n) {
            const int32_t *g = &d->dbg_host[(size_t)n * 16];
            fprintf(stderr, "[twl dbg] pair %d: tiles %d last_k %d conv 0x%x L %d U %d ref_idx %d qry_idx %d pos %d err %d steps_left %d R %d Q %d\n",
                    n, g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], g[8], g[9], g[10], g[11]);
        }
    }
    float ms_pack = 0.f, ms_k = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms_pack, d->ev[0], d->ev[1]));
    HIP_TRY(hipEventElapsedTime(&ms_k, d->ev[1], d->ev[2]));
    d->stats.band_cells = total;
    d->stats.nominal_cells = c.nominal;
    d->stats.pack_ms = ms_pack;
    d->stats.kernel_ms = ms_k + ms_redo;
    d->stats.total_ms = ms_pack + ms_k + ms_redo;
    return TWL_OK;
}
