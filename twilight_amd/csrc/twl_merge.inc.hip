// twilight_amd/csrc/twl_merge.inc.hip -- host side of the merge of existing alignments (include/twl_merge.h).
// Included at the end of twl_align.hip, behind twl_place.inc.hip: it works on the store's rows and on the level's path buffers.
// What a call rejects is decided in twl_merge_plan.inc.hip (pure); this file allocates, uploads and launches (kernels: merge_kernels.hip.h).
//
// HBM of a merge: the map arena pos (the L_g ints of every group back to back), per apply the rank tables rpos / qpos of every taking
// pair, and at the finish the inverse maps inv[n_groups][pitch].

#include "twl_merge_plan.inc.hip"

static_assert(sizeof(ComposeRow) == sizeof(twl::ComposeJob) && offsetof(ComposeRow, tab_off) == offsetof(twl::ComposeJob, tab_off) &&
              offsetof(ComposeRow, L) == offsetof(twl::ComposeJob, L) && offsetof(ComposeRow, tab_len) == offsetof(twl::ComposeJob, tab_len),
              "ComposeRow (twl_merge_plan.inc.hip) and twl::ComposeJob (merge_kernels.hip.h) must agree");

struct twl_merge {
    twl_store *s = nullptr;
    MergeGroups g;
    bool finished = false;
    Buf pos, ranks, counts, inv, hostRows;
    Ref rPosOff, rL;                 // the groups' tables, uploaded once (up_groups)
    Arena up_groups, up;             // up: the per-call tables of apply / finish: both synchronise the stream before they return
    PinBuf back;
    hipEvent_t ev[5] = {};           // apply: start, end; finish: start, rewrite start, end
    double apply_ms = 0, finish_ms = 0, rewrite_ms = 0;      // HIP-event times: every apply so far, the finish, its row rewrite alone
    void release()
    {
        for (Buf *b : {&pos, &ranks, &counts, &inv, &hostRows}) b->release();
        for (hipEvent_t &e : ev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
        up_groups.release(); up.release(); back.release();
    }
};

extern "C" {

int twl_merge_create(twl_store *s, int32_t n_groups, const int32_t *group_off, const int32_t *row_ids, twl_merge **out)
{
    if (!s || !out) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    auto mg = std::make_unique<twl_merge>();
    if (const char *why = check_merge_create(n_groups, group_off, row_ids, s->n_seqs, s->len.data(), mg->g)) { g_err = why; return TWL_ERR_BAD_ARGUMENT; }
    mg->s = s;
    struct Undo { twl_merge *m; ~Undo() { if (m) m->release(); } };      // (a create that fails gives back what it took)
    DEVICE_CALL(call, s->d);
    Undo undo{mg.get()};
    hipStream_t st = call.st;
    int rc;
    const MergeGroups &g = mg->g;
    for (hipEvent_t &e : mg->ev) HIP_TRY(hipEventCreate(&e));
    if ((rc = mg->pos.ensure((size_t)std::max<int64_t>(g.posInts, 4) * sizeof(int32_t)))) return rc;
    Arena &A = mg->up_groups;
    if ((rc = A.begin((size_t)n_groups * (sizeof(int64_t) + sizeof(int32_t)), 2))) return rc;
    A.put(mg->rPosOff, g.posOff); A.put(mg->rL, g.L);
    if ((rc = A.flush(st))) return rc;
    if (n_groups > 0) {
        hipLaunchKernelGGL(twl::merge_iota_kernel, dim3((unsigned)n_groups, (unsigned)((g.maxL + twl::kPlThreads - 1) / twl::kPlThreads)), dim3(twl::kPlThreads), 0, st,
                           mg->rPosOff.as<const int64_t>(), mg->rL.as<const int32_t>(), (int32_t *)mg->pos.p);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(st));
    undo.m = nullptr;
    *out = mg.release();
    return TWL_OK;
}

void twl_merge_destroy(twl_merge *mg)
{
    if (!mg) return;
    const std::unique_ptr<twl_merge> own(mg);
    {
        std::lock_guard<std::mutex> lk(mg->s->d->mu);
        (void)hipSetDevice(mg->s->d->id);
        (void)hipStreamSynchronize(mg->s->d->stream);
        mg->release();
    }
}

int twl_merge_apply(twl_merge *mg, twl_store *s, int32_t n_pairs, const int32_t *ref_off, const int32_t *ref_groups, const int32_t *qry_off,
                    const int32_t *qry_groups, const int8_t *paths, const int32_t *path_len, int32_t path_stride, const uint8_t *from_dp)
{
    if (!mg || !s || mg->s != s) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    MergeApplyPlan p;
    if (const char *why = check_merge_apply(mg->g, mg->finished, n_pairs, ref_off, ref_groups, qry_off, qry_groups, paths != nullptr, path_len, path_stride, from_dp, path_level_view(s), p)) {
        g_err = why;
        return TWL_ERR_BAD_ARGUMENT;
    }
    const int32_t m = (int32_t)p.pair.size();
    if (m == 0) return TWL_OK;
    DEVICE_CALL(call, s->d);
    hipStream_t st = call.st;
    int rc;
    if ((rc = upload_host_paths(mg->hostRows, paths, path_len, path_stride, p.src.hostRows, st))) return rc;
    Ref rWhich, rSrc, rPlen, rWr, rWq, rROff, rQOff, rJobs;
    Arena &A = mg->up;
    if ((rc = A.begin((size_t)m * (1 + 3 * sizeof(int64_t) + 3 * sizeof(int32_t)) + p.jobs.size() * sizeof(ComposeRow), 8))) return rc;
    A.put(rWhich, p.src.which); A.put(rSrc, p.src.srcOff); A.put(rPlen, p.plen); A.put(rWr, p.wr); A.put(rWq, p.wq); A.put(rROff, p.rOff); A.put(rQOff, p.qOff);
    A.put(rJobs, p.jobs);
    if ((rc = A.flush(st))) return rc;
    if ((rc = mg->ranks.ensure((size_t)std::max<int64_t>(p.rankInts, 4) * sizeof(int32_t)))) return rc;
    if ((rc = mg->counts.ensure((size_t)m * 3 * sizeof(int32_t)))) return rc;
    twl::RankArgs a{};
    a.from = path_src(s, from_dp, mg->hostRows, rWhich, rSrc, rPlen);
    a.wr = rWr.as<const int32_t>(); a.wq = rWq.as<const int32_t>();
    a.r_off = rROff.as<const int64_t>(); a.q_off = rQOff.as<const int64_t>();
    a.ranks = (int32_t *)mg->ranks.p;
    a.counts = (int32_t *)mg->counts.p;
    HIP_TRY(hipEventRecord(mg->ev[0], st));
    hipLaunchKernelGGL(twl::merge_ranks_kernel, dim3((unsigned)m), dim3(twl::kPlThreads), 0, st, a);
    HIP_TRY(hipGetLastError());
    if ((rc = mg->back.ensure((size_t)m * 3 * sizeof(int32_t)))) return rc;
    HIP_TRY(hipMemcpyAsync(mg->back.p, mg->counts.p, (size_t)m * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // a path of another shape: nothing has been composed, every map is as it was
    if (const char *why = check_merge_counts(p, (const int32_t *)mg->back.p)) { g_err = why; return TWL_ERR_BAD_ARGUMENT; }
    hipLaunchKernelGGL(twl::merge_compose_kernel, dim3((unsigned)p.jobs.size(), (unsigned)((p.maxL + twl::kPlThreads - 1) / twl::kPlThreads)), dim3(twl::kPlThreads), 0, st,
                       rJobs.as<const twl::ComposeJob>(), (const int32_t *)mg->ranks.p, (int32_t *)mg->pos.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(mg->ev[1], st));
    HIP_TRY(hipStreamSynchronize(st));
    float ms = 0;
    if (hipEventElapsedTime(&ms, mg->ev[0], mg->ev[1]) == hipSuccess) mg->apply_ms += ms;
    merge_apply_done(mg->g, p);
    return TWL_OK;
}

int twl_merge_finish(twl_merge *mg, int32_t *W_out)
{
    if (!mg || !W_out) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    twl_store *s = mg->s;
    const MergeGroups &g = mg->g;
    int32_t W = 0;
    if (const char *why = check_merge_finish(g, mg->finished, s->len.data(), &W)) { g_err = why; return TWL_ERR_BAD_ARGUMENT; }
    const int32_t nG = g.n(), nRows = (int32_t)g.rows.size();
    DEVICE_CALL(call, s->d);
    hipStream_t st = call.st;
    int rc;
    if (nG > 0 && W > 0) {
        if ((rc = wait_rows(s, st))) return rc;
        if ((rc = grow_rows(s, (int64_t)W + 1))) return rc;
        const int64_t pitch = ((int64_t)W + twl::kMgCols - 1) / twl::kMgCols * twl::kMgCols;
        const size_t invBytes = (size_t)nG * (size_t)pitch * sizeof(int32_t);
        if ((rc = mg->inv.ensure(invBytes))) return rc;
        HIP_TRY(hipEventRecord(mg->ev[2], st));
        HIP_TRY(hipMemsetAsync(mg->inv.p, 0xFF, invBytes, st));
        hipLaunchKernelGGL(twl::merge_inverse_kernel, dim3((unsigned)nG, (unsigned)((g.maxL + twl::kPlThreads - 1) / twl::kPlThreads)), dim3(twl::kPlThreads), 0, st,
                           mg->rPosOff.as<const int64_t>(), mg->rL.as<const int32_t>(), (const int32_t *)mg->pos.p, W, pitch, (int32_t *)mg->inv.p);
        std::vector<uint8_t> plane;
        std::vector<int32_t> sGroup, sFirst, sN;
        for (int32_t q : g.rows) plane.push_back(s->plane[q]);
        for (int32_t k = 0; k < nG; ++k)
            for (int32_t at = g.off[k]; at < g.off[k + 1]; at += twl::kMgRows) {
                sGroup.push_back(k); sFirst.push_back(at); sN.push_back(std::min<int32_t>(twl::kMgRows, g.off[k + 1] - at));
            }
        Ref rIds, rPlane, rSG, rSF, rSN;
        Arena &A = mg->up;
        if ((rc = A.begin((size_t)nRows * (1 + sizeof(int32_t)) + sGroup.size() * 3 * sizeof(int32_t), 5))) return rc;
        A.put(rIds, g.rows); A.put(rPlane, plane); A.put(rSG, sGroup); A.put(rSF, sFirst); A.put(rSN, sN);
        if ((rc = A.flush(st))) return rc;
        twl::RewriteArgs a{};
        fill_row_planes(s, a);
        a.ids = rIds.as<const int32_t>(); a.plane = rPlane.as<const uint8_t>();
        a.slice_group = rSG.as<const int32_t>(); a.slice_first = rSF.as<const int32_t>(); a.slice_n = rSN.as<const int32_t>();
        a.L = mg->rL.as<const int32_t>();
        a.inv = (const int32_t *)mg->inv.p;
        a.pitch = pitch;
        a.W = W;
        HIP_TRY(hipEventRecord(mg->ev[3], st));
        hipLaunchKernelGGL(twl::merge_rewrite_kernel, dim3((unsigned)((W + twl::kMgColTile - 1) / twl::kMgColTile), (unsigned)sGroup.size()), dim3(twl::kPlThreads), 0, st, a);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(mg->ev[4], st));
        HIP_TRY(hipStreamSynchronize(st));
        float ms = 0;
        if (hipEventElapsedTime(&ms, mg->ev[2], mg->ev[4]) == hipSuccess) mg->finish_ms = ms;
        if (hipEventElapsedTime(&ms, mg->ev[3], mg->ev[4]) == hipSuccess) mg->rewrite_ms = ms;
        rows_rewritten(s, g.rows, W);
    }
    mg->finished = true;
    *W_out = W;
    return TWL_OK;
}

int twl_merge_read_map(twl_merge *mg, int32_t group, int32_t *out)
{
    if (!mg || !out || group < 0 || group >= mg->g.n()) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    DEVICE_CALL(call, mg->s->d);
    if (mg->g.L[group] > 0)
        HIP_TRY(hipMemcpyAsync(out, (const int32_t *)mg->pos.p + mg->g.posOff[group], (size_t)mg->g.L[group] * sizeof(int32_t), hipMemcpyDeviceToHost, call.st));
    HIP_TRY(hipStreamSynchronize(call.st));
    return TWL_OK;
}

int twl_merge_timing(twl_merge *mg, double *apply_ms, double *finish_ms, double *rewrite_ms)
{
    if (!mg) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    if (apply_ms) *apply_ms = mg->apply_ms;
    if (finish_ms) *finish_ms = mg->finish_ms;
    if (rewrite_ms) *rewrite_ms = mg->rewrite_ms;
    return TWL_OK;
}

}  // extern "C"
