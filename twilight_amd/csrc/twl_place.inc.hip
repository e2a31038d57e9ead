// twilight_amd/csrc/twl_place.inc.hip -- host side of placement without a tree (include/twl_place.h).
// Included at the end of twl_align.hip, behind twl_store.inc.hip and twl_level.inc.hip: it works on their stores and level buffers.
//
// HBM of a placement: one arena of final paths (a slot of L + len bytes per sequence of the store), longest[L + 1], and at the finish
// ins[L + 1] and colsrc[W] (kernels: place_kernels.hip.h).

// What a call rejects, and the placement's bookkeeping, are decided in twl_place_plan.inc.hip (pure); this file allocates, uploads, launches
// and reads back.

#include "twl_place_plan.inc.hip"
#include "twl_keep_plan.inc.hip"

struct twl_place {
    twl_store *s = nullptr;
    PlaceBook b;
    KeepBook k;                      // the finish that keeps the backbone's length (twl_keep.inc.hip)
    Buf arena, longest, ins, colsrc, w, bad, hostRows, keepCnt, keepRec;
    double keepRowsMs = 0, keepRunsMs = 0;
    Arena up;                        // the small per-call tables of collect / finish: both synchronise the stream before they return
    PinBuf back;
    void release()
    {
        for (Buf *buf : {&arena, &longest, &ins, &colsrc, &w, &bad, &hostRows, &keepCnt, &keepRec}) buf->release();
        up.release(); back.release();
    }
};

extern "C" {

int twl_store_count_columns(twl_store *s, int32_t n_ids, const int32_t *ids, int32_t cache_id)
{
    if (!s) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    int32_t L = -1;
    if (const char *why = check_count_columns(n_ids, ids, cache_id, cache_id >= 0 && s->cache.count(cache_id), s->n_seqs, s->len.data(), &L)) { g_err = why; return TWL_ERR_BAD_ARGUMENT; }
    DEVICE_CALL(call, s->d);
    hipStream_t st = call.st;
    const size_t P = (size_t)s->P, cells = (size_t)L * P;
    CacheEntry e;
    int rc = e.take(call.d, L, std::max<size_t>(cells * sizeof(float), 16));
    if (rc) return rc;
    struct Scratch { Buf b; ~Scratch() { b.release(); } } scratch;      // the integer counts: freed behind the call's synchronisation
    Buf &counts = scratch.b;
    if ((rc = counts.ensure(std::max<size_t>(cells * sizeof(int32_t), 16)))) return rc;
    if ((rc = wait_rows(s, st))) return rc;
    RowRefs r;
    if ((rc = upload_row_tables(s, st, n_ids, ids, nullptr, nullptr, r))) return rc;
    if (cells) {
        HIP_TRY(hipMemsetAsync(counts.p, 0, cells * sizeof(int32_t), st));
        const dim3 grid((unsigned)((L + twl::kPlThreads - 1) / twl::kPlThreads), (unsigned)((n_ids + twl::kCountRows - 1) / twl::kCountRows));
        if (s->P == 6)
            hipLaunchKernelGGL(twl::count_columns_kernel<6>, grid, dim3(twl::kPlThreads), 0, st, (const char *)s->rows[0].p, (const char *)s->rows[1].p, s->cap,
                               r.plane.as<const uint8_t>(), r.ids.as<const int32_t>(), n_ids, L, (const uint8_t *)s->lut.p, (int32_t *)counts.p);
        else
            hipLaunchKernelGGL(twl::count_columns_kernel<22>, grid, dim3(twl::kPlThreads), 0, st, (const char *)s->rows[0].p, (const char *)s->rows[1].p, s->cap,
                               r.plane.as<const uint8_t>(), r.ids.as<const int32_t>(), n_ids, L, (const uint8_t *)s->lut.p, (int32_t *)counts.p);
        hipLaunchKernelGGL(twl::counts_to_cache_kernel, dim3((unsigned)((cells + twl::kPlThreads - 1) / twl::kPlThreads)), dim3(twl::kPlThreads), 0, st,
                           (const int32_t *)counts.p, (int64_t)cells, (float *)e.buf.p);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(st));
    s->cache[cache_id] = std::move(e);
    return TWL_OK;
}

int twl_place_create(twl_store *s, int32_t L, twl_place **out)
{
    if (!s || !out) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    auto pl = std::make_unique<twl_place>();
    int64_t total = 0;
    if (const char *why = check_place_create(L, s->n_seqs, s->len.data(), pl->b, &total)) { g_err = why; return TWL_ERR_BAD_ARGUMENT; }
    pl->s = s;
    struct Undo { twl_place *p; ~Undo() { if (p) p->release(); } };      // (a create that fails gives back what it took)
    DEVICE_CALL(call, s->d);
    Undo undo{pl.get()};
    hipStream_t st = call.st;
    int rc;
    if ((rc = pl->arena.ensure((size_t)std::max<int64_t>(total, 16)))) return rc;
    if ((rc = pl->longest.ensure(((size_t)L + 1) * sizeof(int32_t)))) return rc;
    HIP_TRY(hipMemsetAsync(pl->longest.p, 0, ((size_t)L + 1) * sizeof(int32_t), st));
    HIP_TRY(hipStreamSynchronize(st));
    undo.p = nullptr;
    *out = pl.release();
    return TWL_OK;
}

void twl_place_destroy(twl_place *pl)
{
    if (!pl) return;
    const std::unique_ptr<twl_place> own(pl);
    {
        std::lock_guard<std::mutex> lk(pl->s->d->mu);
        (void)hipSetDevice(pl->s->d->id);
        (void)hipStreamSynchronize(pl->s->d->stream);
        pl->release();
    }
}

int twl_place_collect(twl_place *pl, twl_store *s, int32_t n_pairs, const int32_t *seq_ids, const int8_t *paths, const int32_t *path_len,
                      int32_t path_stride, const uint8_t *from_dp)
{
    if (!pl || !s || pl->s != s) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    PlaceCollectPlan p;
    if (const char *why = check_place_collect(pl->b, n_pairs, seq_ids, paths != nullptr, path_len, path_stride, from_dp, s->n_seqs, s->len.data(), path_level_view(s), p)) {
        g_err = why;
        return TWL_ERR_BAD_ARGUMENT;
    }
    DEVICE_CALL(call, s->d);
    hipStream_t st = call.st;
    int rc;
    const int32_t m = (int32_t)p.ids.size();
    if (m > 0) {
        if ((rc = upload_host_paths(pl->hostRows, paths, path_len, path_stride, p.src.hostRows, st))) return rc;
        Ref rWhich, rSrc, rPlen, rQlen, rDst;
        Arena &A = pl->up;
        if ((rc = A.begin((size_t)m * (1 + 2 * sizeof(int64_t) + 2 * sizeof(int32_t)), 5))) return rc;
        A.put(rWhich, p.src.which); A.put(rSrc, p.src.srcOff); A.put(rPlen, p.plen); A.put(rQlen, p.qlen); A.put(rDst, p.dstOff);
        if ((rc = A.flush(st))) return rc;
        if ((rc = pl->bad.ensure((size_t)m * sizeof(int32_t)))) return rc;
        twl::CollectArgs a{};
        a.from = path_src(s, from_dp, pl->hostRows, rWhich, rSrc, rPlen);
        a.qlen = rQlen.as<const int32_t>();
        a.dst_off = rDst.as<const int64_t>();
        a.arena = (int8_t *)pl->arena.p;
        a.longest = (int32_t *)pl->longest.p;
        a.bad = (int32_t *)pl->bad.p;
        a.L = pl->b.L;
        hipLaunchKernelGGL(twl::place_collect_kernel, dim3((unsigned)m), dim3(twl::kPlThreads), 0, st, a);
        HIP_TRY(hipGetLastError());
        if ((rc = pl->back.ensure((size_t)m * sizeof(int32_t)))) return rc;
        HIP_TRY(hipMemcpyAsync(pl->back.p, pl->bad.p, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (from_dp) {                                 // the level is over: its buffers go back to the device's pool
        s->prepared = false;
        s->staged_stride = 0;
        release_level(s->lv);
    }
    if (const int32_t nBad = place_collect_done(pl->b, p, (const int32_t *)pl->back.p)) {
        g_err = std::string("a path does not cover the backbone's columns and its sequence's letters exactly (") + std::to_string(nBad) + " paths)";
        return TWL_ERR_BAD_ARGUMENT;
    }
    return TWL_OK;
}

int twl_place_finish(twl_place *pl, int32_t n_backbone, const int32_t *backbone_ids, int32_t *W_out)
{
    if (!pl || !W_out) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    twl_store *s = pl->s;
    PlaceBook &b = pl->b;
    if (const char *why = check_finish_after_keep(pl->k)) { g_err = why; return TWL_ERR_BAD_ARGUMENT; }
    if (const char *why = check_place_finish(b, n_backbone, backbone_ids, s->n_seqs, s->len.data())) { g_err = why; return TWL_ERR_BAD_ARGUMENT; }
    const int32_t L = b.L;
    DEVICE_CALL(call, s->d);
    hipStream_t st = call.st;
    int rc;
    if ((rc = pl->ins.ensure(((size_t)L + 1) * sizeof(int32_t)))) return rc;
    if ((rc = pl->w.ensure(sizeof(int32_t)))) return rc;
    hipLaunchKernelGGL(twl::place_scan_kernel, dim3(1), dim3(twl::kPlThreads), 0, st, (const int32_t *)pl->longest.p, L, (int32_t *)pl->ins.p, (int32_t *)pl->w.p);
    HIP_TRY(hipGetLastError());
    if ((rc = pl->back.ensure(sizeof(int32_t)))) return rc;
    HIP_TRY(hipMemcpyAsync(pl->back.p, pl->w.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int32_t W = *(const int32_t *)pl->back.p;
    if (const char *why = check_place_width(b, W)) { g_err = why; return TWL_ERR_HIP; }
    if ((rc = wait_rows(s, st))) return rc;
    if ((rc = grow_rows(s, (int64_t)W + 1))) return rc;
    if ((rc = pl->colsrc.ensure((size_t)std::max(W, 1) * sizeof(int32_t)))) return rc;
    HIP_TRY(hipMemsetAsync(pl->colsrc.p, 0xFF, (size_t)std::max(W, 1) * sizeof(int32_t), st));
    if (L > 0)
        hipLaunchKernelGGL(twl::place_colsrc_kernel, dim3((unsigned)((L + twl::kPlThreads - 1) / twl::kPlThreads)), dim3(twl::kPlThreads), 0, st,
                           (const int32_t *)pl->longest.p, (const int32_t *)pl->ins.p, L, (int32_t *)pl->colsrc.p);
    const int32_t nP = (int32_t)b.placed.size();
    std::vector<int32_t> pIds(b.placed), pQlen, pPlen, bIds(backbone_ids, backbone_ids + n_backbone);
    std::vector<uint8_t> pPlane, bPlane;
    std::vector<int64_t> pOff;
    for (int32_t id : pIds) { pPlane.push_back(s->plane[id]); pQlen.push_back(b.qlen[id]); pPlen.push_back(b.plen[id]); pOff.push_back(b.slot[id]); }
    for (int32_t id : bIds) bPlane.push_back(s->plane[id]);
    Ref rPId, rPPl, rPQ, rPOff, rPLen, rBId, rBPl;
    Arena &A = pl->up;
    if ((rc = A.begin((size_t)nP * (1 + sizeof(int64_t) + 3 * sizeof(int32_t)) + (size_t)n_backbone * (1 + sizeof(int32_t)), 7))) return rc;
    A.put(rPId, pIds); A.put(rPPl, pPlane); A.put(rPQ, pQlen); A.put(rPOff, pOff); A.put(rPLen, pPlen); A.put(rBId, bIds); A.put(rBPl, bPlane);
    if ((rc = A.flush(st))) return rc;
    twl::ExpandArgs a{};
    fill_row_planes(s, a);
    a.arena = (const int8_t *)pl->arena.p;
    a.longest = (const int32_t *)pl->longest.p; a.ins = (const int32_t *)pl->ins.p; a.colsrc = (const int32_t *)pl->colsrc.p;
    a.L = L; a.W = W;
    if (nP > 0) {
        twl::ExpandArgs ap = a;
        ap.ids = rPId.as<const int32_t>(); ap.plane = rPPl.as<const uint8_t>(); ap.qlen = rPQ.as<const int32_t>();
        ap.path_off = rPOff.as<const int64_t>(); ap.plen = rPLen.as<const int32_t>();
        hipLaunchKernelGGL(twl::place_expand_kernel, dim3((unsigned)nP), dim3(twl::kPlThreads), 0, st, ap);
    }
    if (n_backbone > 0 && W > 0) {
        twl::ExpandArgs ab = a;
        ab.ids = rBId.as<const int32_t>(); ab.plane = rBPl.as<const uint8_t>();
        hipLaunchKernelGGL(twl::backbone_expand_kernel, dim3((unsigned)n_backbone, (unsigned)((W + twl::kPlThreads - 1) / twl::kPlThreads)), dim3(twl::kPlThreads), 0, st, ab);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    rows_rewritten(s, pIds, W);
    rows_rewritten(s, bIds, W);
    b.finished = true;
    *W_out = W;
    return TWL_OK;
}

int twl_place_read_insertions(twl_place *pl, int32_t *out)
{
    if (!pl || !out) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    DEVICE_CALL(call, pl->s->d);
    HIP_TRY(hipMemcpyAsync(out, pl->longest.p, ((size_t)pl->b.L + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, call.st));
    HIP_TRY(hipStreamSynchronize(call.st));
    return TWL_OK;
}

}  // extern "C"
