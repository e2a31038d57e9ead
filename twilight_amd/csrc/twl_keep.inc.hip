// twilight_amd/csrc/twl_keep.inc.hip -- host side of the placement finish that keeps the backbone's length (include/twl_keep.h).
// Included at the end of twl_align.hip, behind twl_place.inc.hip: it works on that file's twl_place (arena of final paths, upload arena,
// pinned read-back block) and on the store's two row planes.
//
// What a call rejects is decided in twl_keep_plan.inc.hip (pure); this file allocates, uploads, launches and reads back.  Kernels:
// keep_kernels.hip.h.

namespace {

// a kernel between two events of the call; the milliseconds are read behind the call's synchronisation
struct KeepTimer {
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int begin(hipStream_t st)
    {
        HIP_TRY(hipEventCreate(&ev0));
        HIP_TRY(hipEventCreate(&ev1));
        HIP_TRY(hipEventRecord(ev0, st));
        return TWL_OK;
    }
    int end(hipStream_t st) { HIP_TRY(hipEventRecord(ev1, st)); return TWL_OK; }
    int ms(double *out)
    {
        float v = 0;
        HIP_TRY(hipEventElapsedTime(&v, ev0, ev1));
        *out += v;
        return TWL_OK;
    }
    ~KeepTimer()
    {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
};

}  // namespace

extern "C" {

int twl_place_finish_keep(twl_place *pl, int64_t *runs_out, int64_t *letters_out)
{
    if (!pl) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    twl_store *s = pl->s;
    PlaceBook &b = pl->b;
    if (const char *why = check_keep_finish(b, pl->k, runs_out && letters_out, s->n_seqs, s->len.data())) { g_err = why; return TWL_ERR_BAD_ARGUMENT; }
    const int32_t L = b.L;
    DEVICE_CALL(call, s->d);
    hipStream_t st = call.st;
    int rc;
    if ((rc = wait_rows(s, st))) return rc;
    if ((rc = grow_rows(s, (int64_t)L + 1))) return rc;
    const int32_t nP = (int32_t)b.placed.size();
    std::vector<int32_t> pIds(b.placed), pQlen, pPlen;
    std::vector<uint8_t> pPlane;
    std::vector<int64_t> pOff;
    for (int32_t id : pIds) { pPlane.push_back(s->plane[id]); pQlen.push_back(b.qlen[id]); pPlen.push_back(b.plen[id]); pOff.push_back(b.slot[id]); }
    KeepTimer timer;
    if (nP > 0) {
        Ref rId, rPl, rQ, rOff, rLen;
        Arena &A = pl->up;
        if ((rc = A.begin((size_t)nP * (1 + sizeof(int64_t) + 3 * sizeof(int32_t)), 5))) return rc;
        A.put(rId, pIds); A.put(rPl, pPlane); A.put(rQ, pQlen); A.put(rOff, pOff); A.put(rLen, pPlen);
        if ((rc = A.flush(st))) return rc;
        if ((rc = pl->keepCnt.ensure(2 * (size_t)nP * sizeof(int32_t)))) return rc;
        twl::KeepRowsArgs a{};
        fill_row_planes(s, a);
        a.ids = rId.as<const int32_t>(); a.plane = rPl.as<const uint8_t>(); a.qlen = rQ.as<const int32_t>();
        a.path_off = rOff.as<const int64_t>(); a.plen = rLen.as<const int32_t>();
        a.arena = (const int8_t *)pl->arena.p;
        a.runs = (int32_t *)pl->keepCnt.p; a.letters = (int32_t *)pl->keepCnt.p + nP;
        a.L = L;
        if ((rc = timer.begin(st))) return rc;
        hipLaunchKernelGGL(twl::keep_rows_kernel, dim3((unsigned)nP), dim3(twl::kPlThreads), 0, st, a);
        HIP_TRY(hipGetLastError());
        if ((rc = timer.end(st))) return rc;
        if ((rc = pl->back.ensure(2 * (size_t)nP * sizeof(int32_t)))) return rc;
        HIP_TRY(hipMemcpyAsync(pl->back.p, pl->keepCnt.p, 2 * (size_t)nP * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (nP > 0 && (rc = timer.ms(&pl->keepRowsMs))) return rc;
    rows_rewritten(s, pIds, L);
    const int32_t *cnt = (const int32_t *)pl->back.p;
    keep_finish_done(b, pl->k, cnt, cnt + nP, runs_out, letters_out);
    return TWL_OK;
}

int twl_place_dropped_counts(twl_place *pl, int32_t n, const int32_t *seq_ids, int32_t *runs, int32_t *letters)
{
    if (!pl) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    if (const char *why = check_dropped_counts(pl->b, pl->k, n, seq_ids, runs && letters)) { g_err = why; return TWL_ERR_BAD_ARGUMENT; }
    for (int32_t i = 0; i < n; ++i) { runs[i] = pl->k.runs[seq_ids[i]]; letters[i] = pl->k.letters[seq_ids[i]]; }
    return TWL_OK;
}

int twl_place_dropped_runs(twl_place *pl, int32_t n, const int32_t *seq_ids, const int64_t *run_off, int32_t *col, int32_t *qpos, int32_t *len)
{
    if (!pl) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    KeepRunsPlan p;
    if (const char *why = check_dropped_runs(pl->b, pl->k, n, seq_ids, run_off, col && qpos && len, p)) { g_err = why; return TWL_ERR_BAD_ARGUMENT; }
    if (n == 0 || p.total == 0) return TWL_OK;                 // (no record is asked for: nothing is launched)
    twl_store *s = pl->s;
    DEVICE_CALL(call, s->d);
    hipStream_t st = call.st;
    int rc;
    const size_t total = (size_t)p.total;
    Ref rOff, rLen, rRun, rCnt;
    Arena &A = pl->up;
    if ((rc = A.begin((size_t)n * (2 * sizeof(int64_t) + 2 * sizeof(int32_t)), 4))) return rc;
    A.put(rOff, p.pathOff); A.put(rLen, p.plen); A.put(rRun, p.runOff); A.put(rCnt, p.nRuns);
    if ((rc = A.flush(st))) return rc;
    if ((rc = pl->keepRec.ensure(3 * total * sizeof(int32_t)))) return rc;
    HIP_TRY(hipMemsetAsync(pl->keepRec.p, 0xFF, 3 * total * sizeof(int32_t), st));
    twl::KeepRunsArgs a{};
    a.path_off = rOff.as<const int64_t>(); a.plen = rLen.as<const int32_t>(); a.run_off = rRun.as<const int64_t>(); a.n_runs = rCnt.as<const int32_t>();
    a.arena = (const int8_t *)pl->arena.p;
    a.col = (int32_t *)pl->keepRec.p; a.qpos = a.col + total; a.len = a.qpos + total;
    KeepTimer timer;
    if ((rc = timer.begin(st))) return rc;
    hipLaunchKernelGGL(twl::keep_runs_kernel, dim3((unsigned)n), dim3(twl::kPlThreads), 0, st, a);
    HIP_TRY(hipGetLastError());
    if ((rc = timer.end(st))) return rc;
    if ((rc = pl->back.ensure(3 * total * sizeof(int32_t)))) return rc;
    HIP_TRY(hipMemcpyAsync(pl->back.p, pl->keepRec.p, 3 * total * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if ((rc = timer.ms(&pl->keepRunsMs))) return rc;
    const int32_t *back = (const int32_t *)pl->back.p;
    memcpy(col, back, total * sizeof(int32_t));
    memcpy(qpos, back + total, total * sizeof(int32_t));
    memcpy(len, back + 2 * total, total * sizeof(int32_t));
    return TWL_OK;
}

int twl_place_keep_timing(twl_place *pl, double *rows_ms, double *runs_ms)
{
    if (!pl || !rows_ms || !runs_ms) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    *rows_ms = pl->keepRowsMs; *runs_ms = pl->keepRunsMs;
    return TWL_OK;
}

}  // extern "C"
