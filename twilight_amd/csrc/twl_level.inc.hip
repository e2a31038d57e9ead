// twilight_amd/csrc/twl_level.inc.hip -- a level on the device-resident store (include/twl_level.h): prepare, align, the read-backs of a level,
// restore, the exchange of final paths, commit, timing.  Each of prepare / align / commit is a driver over named steps: what the call rejects
// and the tables its kernels read come from the pure functions of twl_level_plan.inc.hip, the steps here size buffers, upload the tables
// (one Arena copy per call), fill the kernels' arguments, launch, read back and apply the bookkeeping.
// Included at the end of twl_align.hip, behind twl_store.inc.hip (the store, its pools, Arena, DeviceCall).

namespace {

static_assert(sizeof(SideRow) == sizeof(twl::SideDesc) && offsetof(SideRow, weight) == offsetof(twl::SideDesc, weight) &&
              offsetof(SideRow, cache_slot) == offsetof(twl::SideDesc, cache_slot) && offsetof(SideRow, store_slot) == offsetof(twl::SideDesc, store_slot),
              "SideRow (twl_level_plan.inc.hip) is uploaded as twl::SideDesc");

// ---- steps of twl_level_prepare ----

// the profiles this level stores: every buffer is had before any is registered (a failure IN this step leaves the store's table as it was;
// a prepare that fails in a later step keeps them registered, as it always did)
int register_stored(twl_store *s, const PreparePlan &pp)
{
    std::vector<CacheEntry> fresh(pp.newIds.size());
    for (size_t k = 0; k < fresh.size(); ++k) {
        const int rc = fresh[k].take(s->d, pp.newLens[k], std::max<size_t>((size_t)pp.newLens[k] * (size_t)s->P * sizeof(float), 16));
        if (rc) return rc;
    }
    for (size_t k = 0; k < fresh.size(); ++k) s->cache[pp.newIds[k]] = std::move(fresh[k]);
    return TWL_OK;
}

int upload_prepare(twl_store *s, hipStream_t st, const PreparePlan &pp, const float *member_weight)
{
    LevelBufs *lv = s->lv;
    std::vector<float *> tab(pp.slotIds.size());
    for (size_t k = 0; k < tab.size(); ++k) tab[k] = (float *)s->cache.find(pp.slotIds[k])->second.buf.p;
    const size_t ns = pp.dsides.size();
    Arena &A = lv->up_prepare;
    int rc = A.begin(ns * (sizeof(SideRow) + sizeof(int32_t)) + pp.nm * (sizeof(int32_t) + sizeof(float) + 1) + tab.size() * sizeof(float *), 6);
    if (rc) return rc;
    A.put(lv->d_sides, pp.dsides);
    A.put(lv->d_mseq, s->members);
    A.put(lv->d_mw, member_weight, pp.nm);
    A.put(lv->d_mplane, pp.mplane);
    A.put(lv->d_tab, tab);
    A.put(lv->d_num, s->h_num);
    return A.flush(st);
}

int size_prepare(LevelBufs *lv, size_t ns, size_t sl, size_t P, size_t chunks)
{
    int rc;
    if ((rc = lv->d_raw.ensure(ns * sl * P * sizeof(float)))) return rc;
    if ((rc = lv->d_colinfo.ensure(ns * sl))) return rc;
    if ((rc = lv->d_cols.ensure(ns * sl * (P + 2) * sizeof(float)))) return rc;
    if ((rc = lv->d_len.ensure(ns * sizeof(int32_t)))) return rc;
    return lv->d_ccnt.ensure(ns * chunks * sizeof(int32_t));
}

twl::LevelArgs prepare_args(const twl_store *s, const twl_params *p, float gappy_threshold, int32_t chunks)
{
    const LevelBufs *lv = s->lv;
    twl::LevelArgs a{};
    a.sides = lv->d_sides.as<const twl::SideDesc>();
    a.member_seq = lv->d_mseq.as<const int32_t>();
    a.member_w = lv->d_mw.as<const float>();
    a.member_plane = lv->d_mplane.as<const uint8_t>();
    a.rows0 = (const char *)s->rows[0].p; a.rows1 = (const char *)s->rows[1].p;
    a.cap = s->cap;
    a.cache = lv->d_tab.as<float *const>();
    a.lut = (const uint8_t *)s->lut.p;
    a.raw = (float *)lv->d_raw.p;
    a.colinfo = (uint8_t *)lv->d_colinfo.p;
    a.cols = (float *)lv->d_cols.p;
    a.len_out = (int32_t *)lv->d_len.p;
    a.stride = s->seq_len;
    a.gappy_thr = gappy_threshold;
    a.remove = (gappy_threshold == 1.0) ? 0 : 1;                         // alignment-helper.cpp:77
    a.gap_open = p->gap_open; a.gap_extend = p->gap_extend;
    a.scale = (s->type == 'n') ? 0.5f : 1.0f;                            // :171
    a.min_gap_extend = p->gap_extend * 0.2;                              // :174  (double product narrowed to float)
    a.min_gap_open = p->gap_open * 0.1;                                  // :175
    a.chunk_cnt = (int32_t *)lv->d_ccnt.p;
    a.n_chunks = chunks;
    return a;
}

int launch_prepare(const twl_store *s, hipStream_t st, const twl::LevelArgs &a, dim3 grid)
{
    if (s->P == 6) {
        hipLaunchKernelGGL(twl::profile_kernel<6>, grid, dim3(256), 0, st, a);
        hipLaunchKernelGGL(twl::compact_kernel<6>, grid, dim3(256), 0, st, a);
    } else {
        hipLaunchKernelGGL(twl::profile_kernel<22>, grid, dim3(256), 0, st, a);
        hipLaunchKernelGGL(twl::compact_kernel<22>, grid, dim3(256), 0, st, a);
    }
    HIP_TRY(hipGetLastError());
    return TWL_OK;
}

// the lengths after gappy-column removal (and the column info, if asked for) come back: the one synchronisation of a prepare
int read_back_prepare(twl_store *s, hipStream_t st, size_t ns, int32_t *len_out, uint8_t *colinfo_out)
{
    LevelBufs *lv = s->lv;
    s->h_len.resize(ns);
    int rc;
    if ((rc = lv->back.ensure(ns * sizeof(int32_t)))) return rc;
    HIP_TRY(hipMemcpyAsync(lv->back.p, lv->d_len.p, ns * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (colinfo_out) HIP_TRY(hipMemcpyAsync(colinfo_out, lv->d_colinfo.p, ns * (size_t)s->seq_len, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    memcpy(s->h_len.data(), lv->back.p, ns * sizeof(int32_t));
    for (size_t i = 0; i < ns; ++i) len_out[i] = s->h_len[i];
    return TWL_OK;
}

// ---- steps of twl_level_align ----

int upload_align(LevelBufs *lv, hipStream_t st, const std::vector<int32_t> &lm)
{
    Arena &A = lv->up_align;
    int rc = A.begin(lm.size() * sizeof(int32_t), 1);
    if (rc) return rc;
    A.put(lv->d_lenmask, lm);
    return A.flush(st);
}

int size_align(LevelBufs *lv, size_t n, size_t sl)
{
    int rc;
    if ((rc = lv->d_aln.ensure(n * 2 * sl))) return rc;
    if ((rc = lv->d_alnlen.ensure(n * sizeof(int32_t)))) return rc;
    return lv->d_err.ensure(n * sizeof(int16_t));
}

// lengths and error codes (run_device has read them back in its one synchronisation, as a rule), then the paths the caller asked for
int read_back_align(twl_store *s, Device *d, hipStream_t st, int8_t *aln_out, int32_t *aln_len_out, int16_t *err_out)
{
    const int32_t n = s->n_pairs;
    const size_t sl = (size_t)s->seq_len;
    LevelBufs *lv = s->lv;
    if ((int32_t)d->last_err.size() == n && (int32_t)d->last_alnlen.size() == n) {
        std::copy(d->last_err.begin(), d->last_err.end(), err_out);
        std::copy(d->last_alnlen.begin(), d->last_alnlen.end(), aln_len_out);
        if (!aln_out) { d->stats.total_ms = d->stats.kernel_ms; return TWL_OK; }       // the paths stay in HBM (twl_level_read_path / twl_level_commit_from_dp)
    } else {
        HIP_TRY(hipMemcpyAsync(aln_len_out, lv->d_alnlen.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(err_out, lv->d_err.p, (size_t)n * sizeof(int16_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    // paths: bulk when most pairs ran, else one copy per pair that has a path
    int32_t ran = 0;
    for (int32_t i = 0; i < n; ++i) ran += aln_len_out[i] > 0;
    if (!aln_out) {}
    else if (ran * 2 >= n) HIP_TRY(hipMemcpyAsync(aln_out, lv->d_aln.p, (size_t)n * 2 * sl, hipMemcpyDeviceToHost, st));
    else
        for (int32_t i = 0; i < n; ++i)
            if (aln_len_out[i] > 0)
                HIP_TRY(hipMemcpyAsync(aln_out + (size_t)i * 2 * sl, (int8_t *)lv->d_aln.p + (size_t)i * 2 * sl, (size_t)aln_len_out[i], hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(d->ev[3], st));
    HIP_TRY(hipStreamSynchronize(st));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, d->ev[5], d->ev[3]));
    d->stats.total_ms = ms;
    return TWL_OK;
}

// ---- steps of twl_level_restore ----

// The work arrays of one batch.  rc of the first that cannot be had; soft: the batch is then handed back to the host instead of failing the call.
int size_restore(LevelBufs *lv, size_t ns, size_t n, size_t sl, unsigned nWch, unsigned nb, bool &soft)
{
    const size_t bstride = 2 * sl + 1;
    const struct { Buf *b; size_t bytes; bool soft; } want[] = {
        {&lv->r_oidx, 2 * ns * (sl + 1) * sizeof(int32_t), true},
        {&lv->r_run, ns * 4 * bstride * sizeof(int32_t), true},
        {&lv->r_seg, ns * bstride * sizeof(int32_t), true},
        {&lv->r_aoff, ns * bstride * sizeof(int32_t), true},
        {&lv->r_blist, ns * bstride * sizeof(int32_t), true},
        {&lv->r_nboth, ns * sizeof(int32_t), false},
        {&lv->r_wtot, ns * nWch * sizeof(int32_t), true},
        // (the arena's pitch does not follow out_stride: the two-sided runs of a pair add up to at most both sides' columns, however short the caller's rows are)
        {&lv->r_arena, ns * 2 * sl, true},
        {&lv->r_outlen, n * sizeof(int32_t), false},
        {&lv->r_tb, ns * nb * twl::kNwThreads * (size_t)twl::kNwCells, true},
        {&lv->r_rows, ns * nb * twl::kNwThreads * 6 * (size_t)twl::kNwRow * sizeof(float), true},
    };
    for (const auto &w : want)
        if (const int rc = w.b->ensure(w.bytes)) { soft = w.soft; return rc; }
    return TWL_OK;
}

twl::RestoreArgs restore_args(const twl_store *s, const twl_params *p, int32_t n_sel, int32_t out_stride, unsigned nWch)
{
    const LevelBufs *lv = s->lv;
    const size_t sl = (size_t)s->seq_len;
    twl::RestoreArgs a{};
    a.aln = (const int8_t *)lv->d_aln.p; a.aln_len = (const int32_t *)lv->d_alnlen.p; a.aln_stride = (int32_t)(2 * sl);
    a.colinfo = (const uint8_t *)lv->d_colinfo.p; a.stride = s->seq_len;
    a.sides = lv->d_sides.as<const twl::SideDesc>(); a.len_red = (const int32_t *)lv->d_len.p;
    a.sel = lv->r_sel.as<const int32_t>(); a.n_sel = n_sel;
    a.orig_idx = (int32_t *)lv->r_oidx.p; a.run = (int32_t *)lv->r_run.p; a.seg = (int32_t *)lv->r_seg.p; a.aoff = (int32_t *)lv->r_aoff.p;
    a.both_list = (int32_t *)lv->r_blist.p; a.n_both = (int32_t *)lv->r_nboth.p;
    a.wtot = (int32_t *)lv->r_wtot.p; a.n_wchunks = (int32_t)nWch;
    a.arena = (int8_t *)lv->r_arena.p; a.arena_stride = (int32_t)(2 * sl); a.bstride = (int32_t)(2 * sl + 1);
    a.out = (int8_t *)lv->d_paths.p; a.out_stride = out_stride; a.out_len = (int32_t *)lv->r_outlen.p;
    a.tbs = (int8_t *)lv->r_tb.p; a.rows = (float *)lv->r_rows.p;
    a.ms = p->P - 1;
    for (int t = 0; t < a.ms * a.ms; ++t) a.M[t] = p->matrix[t];
    a.gap_open = p->gap_open; a.gap_extend = p->gap_extend;
    return a;
}

// One batch of twl_level_restore (the caller holds the device's lock and has sized the path buffer).
int restore_batch(twl_store *s, const twl_params *p, int32_t n_sel, const int32_t *pairs, int32_t out_stride, int32_t *final_len_out)
{
    int rc;
    const int32_t n = s->n_pairs;
    hipStream_t st = s->d->stream;
    LevelBufs *lv = s->lv;
    const size_t bstride = 2 * (size_t)s->seq_len + 1;
    {
        Arena &A = lv->up_restore;
        if ((rc = A.begin((size_t)n_sel * sizeof(int32_t), 1))) return rc;
        A.put(lv->r_sel, pairs, (size_t)n_sel);
        if ((rc = A.flush(st))) return rc;
    }
    const unsigned nWch = (unsigned)((bstride + (size_t)twl::kRsThreads * twl::kWrItems - 1) / ((size_t)twl::kRsThreads * twl::kWrItems));      // chunks of boundaries of the longest possible path
    const unsigned nb = (unsigned)std::max(1, std::min(128, 4096 / n_sel));     // one-wave workgroups per pair of the small alignments (<= ~1.8 GB of scratch for the rare large ones)
    bool soft = false;
    if ((rc = size_restore(lv, (size_t)n_sel, (size_t)n, (size_t)s->seq_len, nWch, nb, soft))) {
        if (!soft) return rc;
        (void)hipGetLastError();                // out of device memory for this batch: its pairs go back to the host path
        for (int32_t t = 0; t < n_sel; ++t) final_len_out[t] = -1;
        return TWL_OK;
    }
    const twl::RestoreArgs a = restore_args(s, p, n_sel, out_stride, nWch);
    hipLaunchKernelGGL(twl::restore_index_kernel, dim3(2 * (unsigned)n_sel), dim3(twl::kRsThreads), 0, st, a);
    hipLaunchKernelGGL(twl::restore_runs_kernel, dim3((unsigned)n_sel), dim3(twl::kRsThreads), 0, st, a);
    hipLaunchKernelGGL(twl::restore_align_kernel, dim3((unsigned)n_sel, nb), dim3(twl::kNwThreads), 0, st, a);
    hipLaunchKernelGGL(twl::restore_count_kernel, dim3((unsigned)n_sel, nWch), dim3(twl::kRsThreads), 0, st, a);
    hipLaunchKernelGGL(twl::restore_write_kernel, dim3((unsigned)n_sel, nWch), dim3(twl::kRsThreads), 0, st, a);
    HIP_TRY(hipGetLastError());
    if ((rc = lv->back.ensure((size_t)n * sizeof(int32_t)))) return rc;
    HIP_TRY(hipMemcpyAsync(lv->back.p, lv->r_outlen.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int32_t *all = (const int32_t *)lv->back.p;
    for (int32_t t = 0; t < n_sel; ++t) final_len_out[t] = all[pairs[t]];
    return TWL_OK;
}

// ---- steps of twl_level_commit_from_dp ----

// the merged profile of every pair that gets one, out of the device's pool (they go back to it if the commit fails before it installs them)
int take_merged(twl_store *s, const int32_t *path_len, std::vector<CacheEntry> &merged)
{
    const CommitPlan &cp = s->commit;
    merged.resize(cp.nMerge());
    for (size_t k = 0; k < merged.size(); ++k) {
        const int32_t len = path_len[cp.merge[4 * k]];
        const int rc = merged[k].take(s->d, len, (size_t)len * (size_t)s->P * sizeof(float));
        if (rc) return rc;
    }
    return TWL_OK;
}

// The paths into the level's path buffer.  The DP output of this level stays where the DP kernel left it (the commit kernels read row i of that
// buffer for from_dp[i] == 1; until round 4 every run of such rows was copied into the path buffer: ~1700 small 2-D copies per pass of a
// 100 000-leaf tree); only the (few) rows the caller brought are uploaded.  (from_dp[i] == 2: twl_level_restore has put pair i's final path
// into its row already)
int stage_paths(twl_store *s, hipStream_t st, const int8_t *paths, const int32_t *path_len, int32_t path_stride, const uint8_t *from_dp)
{
    const size_t n = (size_t)s->n_pairs, ps = (size_t)path_stride;
    int rc;
    if ((rc = s->lv->d_paths.ensure(n * ps))) return rc;
    if (!from_dp) HIP_TRY(hipMemcpyAsync(s->lv->d_paths.p, paths, n * ps, hipMemcpyHostToDevice, st));
    else
        for (size_t i = 0; i < n; ++i)
            if (!from_dp[i] && path_len[i] > 0)
                HIP_TRY(hipMemcpyAsync((int8_t *)s->lv->d_paths.p + i * ps, paths + i * ps, (size_t)path_len[i], hipMemcpyHostToDevice, st));
    return s->lv->d_chunk.ensure(n * (size_t)s->commit.nChunks * 2 * sizeof(int32_t));
}

int upload_commit(twl_store *s, hipStream_t st, const std::vector<CacheEntry> &merged, const int32_t *path_len, const uint8_t *from_dp)
{
    const CommitPlan &cp = s->commit;
    LevelBufs *lv = s->lv;
    const size_t n = (size_t)s->n_pairs;
    std::vector<float *> &tab = s->h_tab;
    tab.clear();
    for (size_t k = 0; k < merged.size(); ++k)
        for (float *p : {(float *)s->cache.find(cp.mergeIds[2 * k])->second.buf.p, (float *)s->cache.find(cp.mergeIds[2 * k + 1])->second.buf.p, (float *)merged[k].buf.p})
            tab.push_back(p);
    Arena &A = lv->up_commit;
    int rc = A.begin((n + cp.work.size() + cp.merge.size()) * sizeof(int32_t) + cp.mergew.size() * sizeof(float) + tab.size() * sizeof(float *) + cp.mplane.size() + (from_dp ? n : 0), 7);
    if (rc) return rc;
    A.put(lv->d_pathlen, path_len, n);
    A.put(lv->d_work, cp.work);
    A.put(lv->d_merge, cp.merge);
    A.put(lv->d_mergew, cp.mergew);
    A.put(lv->d_tab, tab);
    A.put(lv->d_mplane, cp.mplane);
    if (from_dp) A.put(lv->d_fromdp, from_dp, n);
    return A.flush(st);
}

twl::CommitArgs commit_args(const twl_store *s, int32_t path_stride, bool fromDp)
{
    const LevelBufs *lv = s->lv;
    twl::CommitArgs a{};
    a.paths = (const int8_t *)lv->d_paths.p;
    if (fromDp) { a.from_dp = lv->d_fromdp.as<const uint8_t>(); a.paths_dp = (const int8_t *)lv->d_aln.p; a.dp_stride = (int32_t)(2 * (size_t)s->seq_len); }
    a.path_len = lv->d_pathlen.as<const int32_t>();
    a.path_stride = path_stride;
    a.chunk_base = (int32_t *)lv->d_chunk.p;
    a.n_chunks = s->commit.nChunks;
    a.sides = lv->d_sides.as<const twl::SideDesc>();
    a.member_seq = lv->d_mseq.as<const int32_t>();
    a.member_plane = lv->d_mplane.as<const uint8_t>();
    a.rows0 = (char *)s->rows[0].p; a.rows1 = (char *)s->rows[1].p;
    a.cap = s->cap;
    a.work = lv->d_work.as<const int32_t>();
    a.cache = lv->d_tab.as<float *const>();
    a.merge = lv->d_merge.as<const int32_t>();
    a.merge_w = lv->d_mergew.as<const float>();
    return a;
}

// The row rewrite (behind path_scan_kernel on the first stream).
// The row rewrite of a SMALL level (the top of a tree: a pair or a few, each with thousands of rows, 0.1-3 ms of HBM traffic) goes to
// the device's second stream: the next levels there align a few pairs on a few CUs from cached profiles and need no row, so the rewrite
// runs beside them.  Whatever reads or rewrites rows on the first stream waits for the event; the tables it reads belong to this level
// set, which acquire_level does not hand out again before the rewrite is done (a second set takes the next level).
int rewrite_rows(twl_store *s, Device *d, hipStream_t st, const twl::CommitArgs &a)
{
    const CommitPlan &cp = s->commit;
    const dim3 grid(cp.nWork(), (unsigned)((cp.nChunks + 3) / 4));
    s->commit_side = false;
    if (!cp.nWork()) return TWL_OK;
    if (!cp.side) {
        const int rc = wait_rows(s, st);
        if (rc) return rc;
        hipLaunchKernelGGL(twl::apply_path_kernel, grid, dim3(256), 0, st, a);
        return TWL_OK;
    }
    LevelBufs *lv = s->lv;
    if (!lv->ev_scan) { HIP_TRY(hipEventCreateWithFlags(&lv->ev_scan, hipEventDisableTiming)); HIP_TRY(hipEventCreateWithFlags(&lv->ev_apply, hipEventDisableTiming)); }
    HIP_TRY(hipEventRecord(lv->ev_scan, st));
    HIP_TRY(hipStreamWaitEvent(d->stream2, lv->ev_scan, 0));        // (rewrites on the second stream follow each other in order)
    HIP_TRY(hipEventRecord(d->ev2[0], d->stream2));
    hipLaunchKernelGGL(twl::apply_path_kernel, grid, dim3(256), 0, d->stream2, a);
    HIP_TRY(hipEventRecord(d->ev2[1], d->stream2));
    HIP_TRY(hipEventRecord(lv->ev_apply, d->stream2));
    lv->apply_pending = true;
    s->rows_event = lv->ev_apply;
    s->commit_side = true;
    return TWL_OK;
}

// bookkeeping: every member of a committed pair now lives in its other plane with the path's length; a merged profile replaces the
// reference node's cache, the query node's is dropped
void apply_commit(twl_store *s, std::vector<CacheEntry> &merged)
{
    const CommitPlan &cp = s->commit;
    for (size_t k = 0; k < cp.flips.size(); k += 2) { s->plane[cp.flips[k]] ^= 1; s->len[cp.flips[k]] = cp.flips[k + 1]; }
    for (size_t k = 0; k < merged.size(); ++k) {
        s->cache[cp.mergeIds[2 * k]] = std::move(merged[k]);      // (merge_cache_kernel may still read the two old ones: the pool hands them out on the same stream)
        s->cache.erase(cp.mergeIds[2 * k + 1]);
    }
}

// rows of the DP output (where[t] == 1; only as a source) and rows of the staged path buffer (2) to or from a device block, one launch per buffer
int level_rows_block(twl_store *s, bool toBlock, int32_t n_sel, const int32_t *pairs, const int32_t *lens, const uint8_t *where, void *blk_dev, const int64_t *blk_off)
{
    if (!s || !s->prepared || !s->lv || !s->staged_stride || n_sel < 0 || (n_sel > 0 && (!pairs || !lens || !blk_dev || !blk_off))) { g_err = "bad argument (twl_level_restore first)"; return TWL_ERR_BAD_ARGUMENT; }
    if (n_sel == 0) return TWL_OK;
    DEVICE_CALL(call, s->d);
    hipStream_t st = call.st;
    LevelBufs *lv = s->lv;
    // a block inside the level's own exchange buffers has a known end; the whole selection is judged before the first launch
    int64_t room = -1;
    for (const Buf *b : {&lv->x_send, &lv->x_recv})
        if (b->p && (const char *)blk_dev >= (const char *)b->p && (const char *)blk_dev < (const char *)b->p + b->cap) room = (int64_t)((const char *)b->p + b->cap - (const char *)blk_dev);
    if (const char *why = check_block_rows(toBlock, n_sel, pairs, lens, where, blk_off, s->n_pairs, s->seq_len, s->staged_stride, lv->d_aln.p != nullptr, room)) { g_err = why; return TWL_ERR_BAD_ARGUMENT; }
    const size_t sl2 = 2 * (size_t)s->seq_len, ps = (size_t)s->staged_stride;
    for (int which = 1; which <= 2; ++which) {
        std::vector<int64_t> ro, bo;
        std::vector<int32_t> ln;
        for (int32_t t = 0; t < n_sel; ++t) {
            const int w = where ? where[t] : 2;
            if (w != which || lens[t] <= 0) continue;
            ro.push_back((int64_t)pairs[t] * (int64_t)(which == 1 ? sl2 : ps)); bo.push_back(blk_off[t]); ln.push_back(lens[t]);
        }
        if (ro.empty()) continue;
        int rc;
        Ref rowoff, blkoff, len;
        Arena &A = lv->up_paths;
        if ((rc = A.begin(ro.size() * (2 * sizeof(int64_t) + sizeof(int32_t)), 3))) return rc;
        A.put(rowoff, ro);
        A.put(blkoff, bo);
        A.put(len, ln);
        if ((rc = A.flush(st))) return rc;
        int8_t *base = (int8_t *)(which == 1 ? lv->d_aln.p : lv->d_paths.p);
        if (toBlock) hipLaunchKernelGGL(twl::rows_to_block_kernel, dim3((unsigned)ro.size()), dim3(256), 0, st, (const int8_t *)base, rowoff.as<const int64_t>(), len.as<const int32_t>(), (int8_t *)blk_dev, blkoff.as<const int64_t>());
        else hipLaunchKernelGGL(twl::block_to_rows_kernel, dim3((unsigned)ro.size()), dim3(256), 0, st, base, rowoff.as<const int64_t>(), len.as<const int32_t>(), (const int8_t *)blk_dev, blkoff.as<const int64_t>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));      // (the arena is rewritten by the second launch; the caller hands the block to a collective next)
    }
    return TWL_OK;
}

}  // namespace

extern "C" {

int twl_level_prepare(twl_store *s, const twl_params *p, float gappy_threshold, int32_t n_pairs, const twl_side *sides, const int32_t *members,
                      const float *member_weight, int32_t seq_len, int32_t *len_out, uint8_t *colinfo_out)
{
    if (!s) { g_err = "store is null"; return TWL_ERR_BAD_ARGUMENT; }
    int rc = check_params(p);
    if (rc) return rc;
    if (p->P != s->P) { g_err = "params.P does not match the store's sequence type"; return TWL_ERR_BAD_ARGUMENT; }
    if (n_pairs < 0 || seq_len < 1 || (n_pairs > 0 && (!sides || !len_out))) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    s->prepared = false;
    s->n_pairs = n_pairs;
    s->seq_len = seq_len;
    if (n_pairs == 0) { s->prepared = true; return TWL_OK; }
    DEVICE_CALL(call, s->d);
    Device *d = call.d;
    hipStream_t st = call.st;
    if (!s->lv) s->lv = acquire_level(d);      // held until the commit (or the store's end)
    const char *why = check_sides(n_pairs, sides, seq_len, members, member_weight, s->n_seqs, s->len.data(), [&](int32_t id) {
        const auto it = s->cache.find(id);
        return it == s->cache.end() ? -1 : it->second.len;
    });
    if (why) { g_err = why; return TWL_ERR_BAD_ARGUMENT; }
    PreparePlan pp = plan_prepare(n_pairs, sides, members, s->plane.data());
    const size_t ns = (size_t)n_pairs * 2;
    s->sides.assign(sides, sides + ns);
    s->members.assign(members, members + pp.nm);
    s->h_num.swap(pp.h_num);
    if ((rc = register_stored(s, pp))) return rc;
    if (pp.readsRows && (rc = wait_rows(s, st))) return rc;      // sides that are built from rows read what a row rewrite on the second stream writes
    HIP_TRY(hipEventRecord(d->ev[0], st));
    if ((rc = upload_prepare(s, st, pp, member_weight))) return rc;
    const dim3 grid((unsigned)ns, (unsigned)((pp.maxLen + 1023) / 1024));
    if ((rc = size_prepare(s->lv, ns, (size_t)seq_len, (size_t)s->P, grid.y))) return rc;
    if ((rc = launch_prepare(s, st, prepare_args(s, p, gappy_threshold, (int32_t)grid.y), grid))) return rc;
    HIP_TRY(hipEventRecord(d->ev[1], st));
    if ((rc = read_back_prepare(s, st, ns, len_out, colinfo_out))) return rc;
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, d->ev[0], d->ev[1]));
    s->prepare_ms = ms;
    s->prepared = true;
    return TWL_OK;
}

int twl_level_read_colinfo(twl_store *s, int32_t pair, int32_t side, uint8_t *out)
{
    if (!s || !s->prepared || !out || pair >= s->n_pairs || side < 0 || side > 1) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    DEVICE_CALL(call, s->d);
    if (pair < 0) {      // the whole level: [n_pairs][2][seq_len]
        HIP_TRY(hipMemcpy(out, s->lv->d_colinfo.p, (size_t)s->n_pairs * 2 * (size_t)s->seq_len, hipMemcpyDeviceToHost));
        return TWL_OK;
    }
    const size_t idx = (size_t)pair * 2 + (size_t)side;
    const size_t len = (size_t)std::max(0, s->sides[idx].len);
    if (len) HIP_TRY(hipMemcpy(out, (const uint8_t *)s->lv->d_colinfo.p + idx * (size_t)s->seq_len, len, hipMemcpyDeviceToHost));
    return TWL_OK;
}

int twl_level_align(twl_store *s, const twl_params *p, const uint8_t *run_mask, int8_t *aln_out, int32_t *aln_len_out, int16_t *err_out)
{
    return twl_level_align_mixed(s, p, run_mask, nullptr, aln_out, aln_len_out, err_out);
}

// One call for the pairs of both gap-character kinds of a level (alignment-cpu.cpp:88 decides gapCharScore per pair): zero_gap[i] = 1 gives
// pair i gapCharScore 0, the others p->gap_char.
int twl_level_align_mixed(twl_store *s, const twl_params *p, const uint8_t *run_mask, const uint8_t *zero_gap, int8_t *aln_out, int32_t *aln_len_out, int16_t *err_out)
{
    if (!s || !s->prepared) { g_err = "twl_level_prepare has not been called"; return TWL_ERR_BAD_ARGUMENT; }
    int rc = check_params(p);
    if (rc) return rc;
    if (p->P != s->P) { g_err = "params.P does not match the store's sequence type"; return TWL_ERR_BAD_ARGUMENT; }
    const int32_t n = s->n_pairs;
    if (n == 0) return TWL_OK;
    if (!aln_len_out || !err_out) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    DEVICE_CALL(call, s->d);
    Device *d = call.d;
    hipStream_t st = call.st;
    LevelBufs *lv = s->lv;
    const AlignPlan ap = plan_align(n, s->h_len, s->sides.data(), run_mask, g_leaf_step);
    if ((rc = upload_align(lv, st, ap.lm))) return rc;
    if ((rc = size_align(lv, (size_t)n, (size_t)s->seq_len))) return rc;
    HIP_TRY(hipEventRecord(d->ev[5], st));
    rc = run_device(d, st, p, n, s->seq_len, nullptr, nullptr, nullptr, lv->d_lenmask.as<const int32_t>(), lv->d_num.as<const int32_t>(), (int8_t *)lv->d_aln.p,
                    (int32_t *)lv->d_alnlen.p, (int16_t *)lv->d_err.p, ap.lm.data(), (const float *)lv->d_cols.p, ap.qryOneHot, zero_gap, ap.shape);
    if (rc) return rc;
    return read_back_align(s, d, st, aln_out, aln_len_out, err_out);
}

int twl_level_read_path(twl_store *s, int32_t pair, int8_t *out, int32_t len)
{
    if (!s || !s->prepared || !out || pair < 0 || pair >= s->n_pairs || len < 0 || len > 2 * s->seq_len || !s->lv || !s->lv->d_aln.p) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    DEVICE_CALL(call, s->d);
    if (len) HIP_TRY(hipMemcpy(out, (const int8_t *)s->lv->d_aln.p + (size_t)pair * 2 * (size_t)s->seq_len, (size_t)len, hipMemcpyDeviceToHost));
    return TWL_OK;
}

int twl_level_read_colinfo_many(twl_store *s, int32_t n_sel, const int32_t *pairs, uint8_t *out)
{
    if (!s || !s->prepared || n_sel < 0 || (n_sel > 0 && (!pairs || !out || !s->lv))) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    DEVICE_CALL(call, s->d);
    const size_t sl = (size_t)s->seq_len;
    for (int32_t t = 0; t < n_sel; ++t) {
        if (pairs[t] < 0 || pairs[t] >= s->n_pairs) { g_err = "pair index out of range"; return TWL_ERR_BAD_ARGUMENT; }
        HIP_TRY(hipMemcpyAsync(out + (size_t)t * 2 * sl, (const uint8_t *)s->lv->d_colinfo.p + (size_t)pairs[t] * 2 * sl, 2 * sl, hipMemcpyDeviceToHost, call.st));
    }
    HIP_TRY(hipStreamSynchronize(call.st));
    return TWL_OK;
}

int twl_level_read_paths(twl_store *s, int32_t n_sel, const int32_t *pairs, const int32_t *lens, int8_t *out, int32_t out_stride)
{
    if (!s || !s->prepared || n_sel < 0 || (n_sel > 0 && (!pairs || !lens || !out || !s->lv || !s->lv->d_aln.p)) || out_stride < 0) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    DEVICE_CALL(call, s->d);
    const size_t sl = (size_t)s->seq_len;
    for (int32_t t = 0; t < n_sel; ++t) {
        if (pairs[t] < 0 || pairs[t] >= s->n_pairs || lens[t] < 0 || lens[t] > out_stride || (size_t)lens[t] > 2 * sl) { g_err = "bad selection"; return TWL_ERR_BAD_ARGUMENT; }
        if (lens[t]) HIP_TRY(hipMemcpyAsync(out + (size_t)t * (size_t)out_stride, (const int8_t *)s->lv->d_aln.p + (size_t)pairs[t] * 2 * sl, (size_t)lens[t], hipMemcpyDeviceToHost, call.st));
    }
    HIP_TRY(hipStreamSynchronize(call.st));
    return TWL_OK;
}

// addGappyColumnsBack for the pairs `pairs` of the prepared and aligned level, on the device (restore_kernels.hip.h): their final paths go
// into the level's path buffer (row pitch out_stride, the pitch the commit must then be given), final_len_out[t] = the final length of
// pairs[t], or -1 when that pair holds a two-sided run too large for the device (the caller restores it on the host, as before).
int twl_level_restore(twl_store *s, const twl_params *p, int32_t n_sel, const int32_t *pairs, int32_t out_stride, int32_t *final_len_out)
{
    if (!s || !s->prepared || !s->lv || (n_sel > 0 && !s->lv->d_aln.p)) { g_err = "twl_level_align has not been called"; return TWL_ERR_BAD_ARGUMENT; }
    int rc = check_params(p);
    if (rc) return rc;
    const int32_t n = s->n_pairs;
    if (n_sel < 0 || (n_sel > 0 && (!pairs || !final_len_out)) || out_stride < 1) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    for (int32_t t = 0; t < n_sel; ++t) if (pairs[t] < 0 || pairs[t] >= n) { g_err = "pair index out of range"; return TWL_ERR_BAD_ARGUMENT; }
    DEVICE_CALL(call, s->d);
    // the restored paths go straight into the rows of the level's path buffer (the commit leaves those rows alone); several calls per
    // level share the buffer and must agree on its pitch
    if (s->staged_stride && s->staged_stride != out_stride) { g_err = "twl_level_restore: one row pitch per level"; return TWL_ERR_BAD_ARGUMENT; }
    if ((rc = s->lv->d_paths.ensure((size_t)n * (size_t)out_stride))) return rc;
    s->staged_stride = out_stride;
    //  at most 4096 pairs per batch: the work arrays cost ~32 * (2 * seq_len + 1) bytes per pair plus the scratch of the small alignments
    // (~458 KB per pair once 4096 / n_sel floors at one workgroup); a wide level of a 100 000-leaf tree with a low -r would otherwise ask for tens of GB at
    // once.  A batch whose arrays cannot be had is handed back (-1: the caller restores those pairs on the host, a path that still exists).
    constexpr int32_t kBatch = 4096;
    for (int32_t at = 0; at < n_sel; at += kBatch)
        if ((rc = restore_batch(s, p, std::min(kBatch, n_sel - at), pairs + at, out_stride, final_len_out + at))) return rc;
    return TWL_OK;
}

// ---- the staged path buffer and contiguous device blocks (exchange of final paths between processes, include/twl_level.h) ----
int twl_level_exchange_buffers(twl_store *s, int64_t send_bytes, int64_t recv_bytes, void **send_dev, void **recv_dev)
{
    if (!s || !s->prepared || !s->lv || send_bytes < 0 || recv_bytes < 0 || !send_dev || !recv_dev) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    DEVICE_CALL(call, s->d);
    int rc;
    if ((rc = s->lv->x_send.ensure(std::max<size_t>((size_t)send_bytes, 64)))) return rc;
    if ((rc = s->lv->x_recv.ensure(std::max<size_t>((size_t)recv_bytes, 64)))) return rc;
    *send_dev = s->lv->x_send.p; *recv_dev = s->lv->x_recv.p;
    return TWL_OK;
}

int twl_level_paths_to_block(twl_store *s, int32_t n_sel, const int32_t *pairs, const int32_t *lens, const uint8_t *where, void *blk_dev, const int64_t *blk_off)
{
    return level_rows_block(s, true, n_sel, pairs, lens, where, blk_dev, blk_off);
}

int twl_level_paths_from_block(twl_store *s, int32_t n_sel, const int32_t *pairs, const int32_t *lens, const void *blk_dev, const int64_t *blk_off)
{
    return level_rows_block(s, false, n_sel, pairs, lens, nullptr, const_cast<void *>(blk_dev), blk_off);
}

int twl_level_write_final(twl_store *s, int32_t pair, const int8_t *path, int32_t len)
{
    if (!s || !s->prepared || !s->lv || !s->staged_stride || pair < 0 || pair >= s->n_pairs || len < 0 || len > s->staged_stride || (len > 0 && !path)) { g_err = "bad argument (twl_level_restore first)"; return TWL_ERR_BAD_ARGUMENT; }
    DEVICE_CALL(call, s->d);
    if (len) HIP_TRY(hipMemcpy((int8_t *)s->lv->d_paths.p + (size_t)pair * (size_t)s->staged_stride, path, (size_t)len, hipMemcpyHostToDevice));
    return TWL_OK;
}

int twl_level_read_final(twl_store *s, int32_t pair, int8_t *out, int32_t len)
{
    if (!s || !s->prepared || !out || pair < 0 || pair >= s->n_pairs || len < 0 || !s->lv || !s->staged_stride || len > s->staged_stride) { g_err = "bad argument (twl_level_restore first)"; return TWL_ERR_BAD_ARGUMENT; }
    DEVICE_CALL(call, s->d);
    if (len) HIP_TRY(hipMemcpy(out, (const int8_t *)s->lv->d_paths.p + (size_t)pair * (size_t)s->staged_stride, (size_t)len, hipMemcpyDeviceToHost));
    return TWL_OK;
}

int twl_level_commit(twl_store *s, const int8_t *paths, const int32_t *path_len, int32_t path_stride)
{
    return twl_level_commit_from_dp(s, paths, path_len, path_stride, nullptr);
}

int twl_level_commit_from_dp(twl_store *s, const int8_t *paths, const int32_t *path_len, int32_t path_stride, const uint8_t *from_dp)
{
    if (!s || !s->prepared) { g_err = "twl_level_prepare has not been called"; return TWL_ERR_BAD_ARGUMENT; }
    const int32_t n = s->n_pairs;
    // (the arguments are checked BEFORE the level's state is given up -- a rejected call leaves the level as it was, committable)
    if (const char *why = check_commit(n, s->seq_len, s->staged_stride, s->lv && s->lv->d_aln.p, paths != nullptr, path_len, path_stride, from_dp)) { g_err = why; return TWL_ERR_BAD_ARGUMENT; }
    DEVICE_CALL(call, s->d);
    Device *d = call.d;
    hipStream_t st = call.st;
    s->prepared = false;                       // the commit goes ahead: the level is over whatever happens from here on
    s->staged_stride = 0;
    struct GiveBack { twl_store *s; ~GiveBack() { release_level(s->lv); } } giveBack{s};      // the level's buffers return to the device's pool
    if (n == 0 || max_path(n, path_len) == 0) return TWL_OK;
    CommitPlan &cp = s->commit;
    plan_commit(cp, n, s->sides.data(), s->members, s->plane.data(), path_len, from_dp);
    int rc;
    if ((rc = grow_rows(s, cp.maxPath))) return rc;
    std::vector<CacheEntry> merged;
    if ((rc = take_merged(s, path_len, merged))) return rc;
    HIP_TRY(hipEventRecord(d->ev[6], st));
    if ((rc = stage_paths(s, st, paths, path_len, path_stride, from_dp))) return rc;
    if ((rc = upload_commit(s, st, merged, path_len, from_dp))) return rc;
    const twl::CommitArgs a = commit_args(s, path_stride, from_dp != nullptr);
    hipLaunchKernelGGL(twl::path_scan_kernel, dim3((unsigned)n), dim3(256), 0, st, a);
    if ((rc = rewrite_rows(s, d, st, a))) return rc;
    if (cp.nMerge()) {
        if (s->P == 6) hipLaunchKernelGGL(twl::merge_cache_kernel<6>, dim3(cp.nMerge(), (unsigned)cp.nChunks), dim3(256), 0, st, a);
        else hipLaunchKernelGGL(twl::merge_cache_kernel<22>, dim3(cp.nMerge(), (unsigned)cp.nChunks), dim3(256), 0, st, a);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(d->ev[7], st));
    s->commit_pending = true;
    // No wait for the kernels: whatever touches the rows, the caches or the level's buffers next is queued behind them on the device's
    // stream, and the host's share of the next level overlaps with the row rewrite.  (Only the caller's own `paths` must be consumed.)
    if (cp.hostRows) HIP_TRY(hipStreamSynchronize(st));
    apply_commit(s, merged);
    return TWL_OK;
}

int twl_level_read_columns(twl_store *s, int32_t pair, int32_t side, float *out, int32_t max_cols)
{
    if (!s || !s->prepared || pair < 0 || pair >= s->n_pairs || side < 0 || side > 1 || !out) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    const size_t CW = (size_t)s->P + 2;
    const int32_t n = std::min(max_cols, s->h_len[2 * (size_t)pair + side]);
    DEVICE_CALL(call, s->d);
    if (n > 0)
        HIP_TRY(hipMemcpy(out, (const float *)s->lv->d_cols.p + ((size_t)pair * 2 + side) * (size_t)s->seq_len * CW, (size_t)n * CW * sizeof(float), hipMemcpyDeviceToHost));
    return TWL_OK;
}

int twl_level_timing(twl_store *s, double *prepare_ms, double *commit_ms)
{
    if (!s) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    if (s->commit_pending) {
        DEVICE_CALL(call, s->d);
        HIP_TRY(hipEventSynchronize(s->d->ev[7]));
        float ms = 0.f, ms2 = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, s->d->ev[6], s->d->ev[7]));
        if (s->commit_side) { HIP_TRY(hipEventSynchronize(s->d->ev2[1])); HIP_TRY(hipEventElapsedTime(&ms2, s->d->ev2[0], s->d->ev2[1])); }
        s->commit_ms = ms + ms2;
        s->commit_pending = false;
    }
    if (prepare_ms) *prepare_ms = s->prepare_ms;
    if (commit_ms) *commit_ms = s->commit_ms;
    return TWL_OK;
}

}  // extern "C"
