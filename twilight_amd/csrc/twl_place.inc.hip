// twilight_amd/csrc/twl_place.inc.hip -- host side of placement without a tree (include/twl_place.h).
// Included at the end of twl_align.hip, behind twl_store.inc.hip and twl_level.inc.hip: it works on their stores and level buffers.
//
// HBM of a placement: one arena of final paths (a slot of L + len bytes per sequence of the store), longest[L + 1], and at the finish
// ins[L + 1] and colsrc[W] (kernels: place_kernels.hip.h).

#include <unordered_set>

struct twl_place {
    twl_store *s = nullptr;
    int32_t L = 0;
    bool finished = false;
    std::vector<int32_t> qlen;       // length of every store sequence when the placement began (its path covers that many letters)
    std::vector<int64_t> slot;       // its slot in the arena
    std::vector<int32_t> plen;       // collected path length, -1: not collected
    std::vector<int32_t> placed;     // collected ids, in order
    Buf arena, longest, ins, colsrc, w, bad, hostRows;
    Arena up;                        // the small per-call tables of collect / finish: both synchronise the stream before they return
    PinBuf back;
};

extern "C" {

int twl_store_count_columns(twl_store *s, int32_t n_ids, const int32_t *ids, int32_t cache_id)
{
    if (!s || n_ids < 1 || !ids || cache_id < 0) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    if (s->cache.count(cache_id)) { g_err = "cache id in use"; return TWL_ERR_BAD_ARGUMENT; }
    const int32_t L = (ids[0] >= 0 && ids[0] < s->n_seqs) ? s->len[ids[0]] : -1;
    for (int32_t t = 0; t < n_ids; ++t) {
        if (ids[t] < 0 || ids[t] >= s->n_seqs) { g_err = "sequence id out of range"; return TWL_ERR_BAD_ARGUMENT; }
        if (s->len[ids[t]] != L) { g_err = "the rows to count differ in length"; return TWL_ERR_BAD_ARGUMENT; }
    }
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
    if (!s || L < 0 || !out) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    DEVICE_CALL(call, s->d);
    Device *d = call.d;
    auto pl = std::make_unique<twl_place>();
    pl->s = s;
    pl->L = L;
    pl->qlen = s->len;
    pl->slot.resize((size_t)s->n_seqs);
    pl->plen.assign((size_t)s->n_seqs, -1);
    int64_t total = 0;
    for (int32_t i = 0; i < s->n_seqs; ++i) { pl->slot[i] = total; total += (int64_t)L + s->len[i]; }
    int rc;
    if ((rc = pl->arena.ensure((size_t)std::max<int64_t>(total, 16)))) return rc;
    if ((rc = pl->longest.ensure(((size_t)L + 1) * sizeof(int32_t)))) return rc;
    HIP_TRY(hipMemsetAsync(pl->longest.p, 0, ((size_t)L + 1) * sizeof(int32_t), d->stream));
    HIP_TRY(hipStreamSynchronize(d->stream));
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
        for (Buf *b : {&pl->arena, &pl->longest, &pl->ins, &pl->colsrc, &pl->w, &pl->bad, &pl->hostRows}) b->release();
        pl->up.release();
        pl->back.release();
    }
}

int twl_place_collect(twl_place *pl, twl_store *s, int32_t n_pairs, const int32_t *seq_ids, const int8_t *paths, const int32_t *path_len,
                      int32_t path_stride, const uint8_t *from_dp)
{
    if (!pl || !s || pl->s != s || n_pairs < 0 || (n_pairs > 0 && (!seq_ids || !path_len || path_stride < 1))) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    if (pl->finished) { g_err = "twl_place_collect after twl_place_finish"; return TWL_ERR_BAD_ARGUMENT; }
    if (from_dp && (!s->prepared || !s->lv || s->n_pairs != n_pairs)) { g_err = "from_dp needs the prepared and aligned level of these pairs"; return TWL_ERR_BAD_ARGUMENT; }
    const int64_t dpStride = 2 * (int64_t)s->seq_len;
    std::vector<int32_t> ids, plen, qlen;
    std::vector<uint8_t> which;
    std::vector<int64_t> srcOff, dstOff;
    std::vector<int32_t> hostRows;                 // pairs whose row comes from `paths`
    std::unordered_set<int32_t> seen;
    for (int32_t i = 0; i < n_pairs; ++i) {
        const int32_t id = seq_ids[i], n = path_len[i];
        if (n == 0) continue;
        if (id < 0 || id >= s->n_seqs) { g_err = "sequence id out of range"; return TWL_ERR_BAD_ARGUMENT; }
        if (pl->plen[id] >= 0 || !seen.insert(id).second) { g_err = "sequence collected twice"; return TWL_ERR_BAD_ARGUMENT; }
        if (s->len[id] != pl->qlen[id]) { g_err = "the sequence's row has been rewritten since the placement began"; return TWL_ERR_BAD_ARGUMENT; }
        if (n < 0 || n > path_stride || (int64_t)n > (int64_t)pl->L + pl->qlen[id]) { g_err = "path_len outside [0, min(path_stride, L + len)]"; return TWL_ERR_BAD_ARGUMENT; }
        const int w = from_dp ? from_dp[i] : 0;
        if (w == 1 && ((int64_t)n > dpStride || !s->lv->d_aln.p)) { g_err = "from_dp 1 without a DP output of that length"; return TWL_ERR_BAD_ARGUMENT; }
        if (w == 2 && (!s->staged_stride || s->staged_stride != path_stride)) { g_err = "from_dp 2: twl_level_restore first, with this row pitch"; return TWL_ERR_BAD_ARGUMENT; }
        if (w == 0 && !paths) { g_err = "host rows missing"; return TWL_ERR_BAD_ARGUMENT; }
        if (w > 2) { g_err = "from_dp must be 0, 1 or 2"; return TWL_ERR_BAD_ARGUMENT; }
        ids.push_back(id); plen.push_back(n); qlen.push_back(pl->qlen[id]); which.push_back((uint8_t)w); dstOff.push_back(pl->slot[id]);
        if (w == 0) { srcOff.push_back((int64_t)hostRows.size() * path_stride); hostRows.push_back(i); }
        else srcOff.push_back((int64_t)i * (w == 1 ? dpStride : (int64_t)path_stride));
    }
    DEVICE_CALL(call, s->d);
    hipStream_t st = call.st;
    int rc;
    const int32_t m = (int32_t)ids.size();
    if (m > 0) {
        if (!hostRows.empty()) {
            if ((rc = pl->hostRows.ensure(hostRows.size() * (size_t)path_stride))) return rc;
            for (size_t k = 0; k < hostRows.size(); ++k)
                HIP_TRY(hipMemcpyAsync((int8_t *)pl->hostRows.p + k * (size_t)path_stride, paths + (size_t)hostRows[k] * (size_t)path_stride,
                                       (size_t)path_len[hostRows[k]], hipMemcpyHostToDevice, st));
        }
        Ref rWhich, rSrc, rPlen, rQlen, rDst;
        Arena &A = pl->up;
        if ((rc = A.begin((size_t)m * (1 + 2 * sizeof(int64_t) + 2 * sizeof(int32_t)), 5))) return rc;
        A.put(rWhich, which); A.put(rSrc, srcOff); A.put(rPlen, plen); A.put(rQlen, qlen); A.put(rDst, dstOff);
        if ((rc = A.flush(st))) return rc;
        if ((rc = pl->bad.ensure((size_t)m * sizeof(int32_t)))) return rc;
        twl::CollectArgs a{};
        a.src[0] = (const int8_t *)pl->hostRows.p;
        a.src[1] = from_dp ? (const int8_t *)s->lv->d_aln.p : nullptr;
        a.src[2] = from_dp ? (const int8_t *)s->lv->d_paths.p : nullptr;
        a.which = rWhich.as<const uint8_t>();
        a.src_off = rSrc.as<const int64_t>();
        a.plen = rPlen.as<const int32_t>();
        a.qlen = rQlen.as<const int32_t>();
        a.dst_off = rDst.as<const int64_t>();
        a.arena = (int8_t *)pl->arena.p;
        a.longest = (int32_t *)pl->longest.p;
        a.bad = (int32_t *)pl->bad.p;
        a.L = pl->L;
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
    int32_t nBad = 0;
    for (int32_t k = 0; k < m; ++k) {
        if (((const int32_t *)pl->back.p)[k]) ++nBad;
        else { pl->plen[ids[k]] = plen[k]; pl->placed.push_back(ids[k]); }
    }
    if (nBad) { g_err = "a path does not cover the backbone's columns and its sequence's letters exactly (" + std::to_string(nBad) + " paths)"; return TWL_ERR_BAD_ARGUMENT; }
    return TWL_OK;
}

int twl_place_finish(twl_place *pl, int32_t n_backbone, const int32_t *backbone_ids, int32_t *W_out)
{
    if (!pl || n_backbone < 0 || (n_backbone > 0 && !backbone_ids) || !W_out) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    if (pl->finished) { g_err = "twl_place_finish called twice"; return TWL_ERR_BAD_ARGUMENT; }
    twl_store *s = pl->s;
    const int32_t L = pl->L;
    std::unordered_set<int32_t> seen(pl->placed.begin(), pl->placed.end());
    for (int32_t t = 0; t < n_backbone; ++t) {
        const int32_t id = backbone_ids[t];
        if (id < 0 || id >= s->n_seqs || s->len[id] != L) { g_err = "backbone id out of range or not of length L"; return TWL_ERR_BAD_ARGUMENT; }
        if (!seen.insert(id).second) { g_err = "a backbone id is listed twice or was collected"; return TWL_ERR_BAD_ARGUMENT; }
    }
    for (int32_t id : pl->placed)
        if (s->len[id] != pl->qlen[id]) { g_err = "a placed sequence's row has been rewritten since it was collected"; return TWL_ERR_BAD_ARGUMENT; }
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
    if (W < L) { g_err = "final width below the backbone's"; return TWL_ERR_HIP; }
    if ((rc = wait_rows(s, st))) return rc;
    if ((rc = grow_rows(s, (int64_t)W + 1))) return rc;
    if ((rc = pl->colsrc.ensure((size_t)std::max(W, 1) * sizeof(int32_t)))) return rc;
    HIP_TRY(hipMemsetAsync(pl->colsrc.p, 0xFF, (size_t)std::max(W, 1) * sizeof(int32_t), st));
    if (L > 0)
        hipLaunchKernelGGL(twl::place_colsrc_kernel, dim3((unsigned)((L + twl::kPlThreads - 1) / twl::kPlThreads)), dim3(twl::kPlThreads), 0, st,
                           (const int32_t *)pl->longest.p, (const int32_t *)pl->ins.p, L, (int32_t *)pl->colsrc.p);
    const int32_t nP = (int32_t)pl->placed.size();
    std::vector<int32_t> pIds(pl->placed), pQlen, pPlen, bIds(backbone_ids, backbone_ids + n_backbone);
    std::vector<uint8_t> pPlane, bPlane;
    std::vector<int64_t> pOff;
    for (int32_t id : pIds) { pPlane.push_back(s->plane[id]); pQlen.push_back(pl->qlen[id]); pPlen.push_back(pl->plen[id]); pOff.push_back(pl->slot[id]); }
    for (int32_t id : bIds) bPlane.push_back(s->plane[id]);
    Ref rPId, rPPl, rPQ, rPOff, rPLen, rBId, rBPl;
    Arena &A = pl->up;
    if ((rc = A.begin((size_t)nP * (1 + sizeof(int64_t) + 3 * sizeof(int32_t)) + (size_t)n_backbone * (1 + sizeof(int32_t)), 7))) return rc;
    A.put(rPId, pIds); A.put(rPPl, pPlane); A.put(rPQ, pQlen); A.put(rPOff, pOff); A.put(rPLen, pPlen); A.put(rBId, bIds); A.put(rBPl, bPlane);
    if ((rc = A.flush(st))) return rc;
    twl::ExpandArgs a{};
    a.rows0 = (const char *)s->rows[0].p; a.rows1 = (const char *)s->rows[1].p;
    a.out0 = (char *)s->rows[0].p; a.out1 = (char *)s->rows[1].p;
    a.cap = s->cap;
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
    for (int32_t id : pIds) { s->plane[id] ^= 1; s->len[id] = W; }
    for (int32_t id : bIds) { s->plane[id] ^= 1; s->len[id] = W; }
    pl->finished = true;
    *W_out = W;
    return TWL_OK;
}

int twl_place_read_insertions(twl_place *pl, int32_t *out)
{
    if (!pl || !out) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    DEVICE_CALL(call, pl->s->d);
    HIP_TRY(hipMemcpyAsync(out, pl->longest.p, ((size_t)pl->L + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, call.st));
    HIP_TRY(hipStreamSynchronize(call.st));
    return TWL_OK;
}

}  // extern "C"
