// twilight_amd/csrc/twl_trim.inc.hip -- host side of include/twl_trim.h: the gappy columns taken out of every listed row of the store.
// Included at the end of twl_align.hip, behind twl_store.inc.hip: it works on the store's rows.
//
// What a call rejects and the grids of its kernels are decided in twl_trim_plan.inc.hip (pure); this file allocates, uploads, launches and
// reads back.  A call in steps: check_trim_columns, plan_trim_grid, trim_upload (one copy of both tables), trim_launch (zeroed counts, then
// counts, keep bits, scan, column list, compaction: nothing waits in between), the read-back of the kept total, rows_rewritten.

#include "twl_trim_plan.inc.hip"

namespace {

// The device memory of one call that nobody reads afterwards: freed when the call returns, behind its synchronisation.  (The gap counts and the
// kept-column list belong to the store: twl_store_trim_read brings them back.)
struct TrimScratch {
    Buf flags, pre, kept;
    Arena up;
    PinBuf back;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    ~TrimScratch()
    {
        for (Buf *b : {&flags, &pre, &kept}) b->release();
        up.release(); back.release();
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
};

// both tables of the call in one copy, the call's buffers; the kernels' arguments point into them
int trim_upload(twl_store *s, hipStream_t st, const TrimRows &t, const TrimGrid &g, int32_t n_ids, const int32_t *ids, int32_t rule, int32_t arg, TrimScratch &m, twl::TrimArgs &a)
{
    std::vector<uint8_t> plane((size_t)n_ids);
    for (int32_t k = 0; k < n_ids; ++k) plane[k] = s->plane[ids[k]];
    Ref rIds, rPlane;
    int rc;
    if ((rc = m.up.begin((size_t)n_ids * (sizeof(int32_t) + 1), 2))) return rc;
    m.up.put(rIds, ids, (size_t)n_ids); m.up.put(rPlane, plane);
    if ((rc = m.up.flush(st))) return rc;
    const size_t W = (size_t)t.W;
    if ((rc = s->trim_gaps.ensure(std::max<size_t>(W * sizeof(uint32_t), 16)))) return rc;
    if ((rc = s->trim_cols.ensure(std::max<size_t>(W * sizeof(int32_t), 16)))) return rc;
    if ((rc = m.flags.ensure(std::max<size_t>((size_t)g.words * sizeof(uint32_t), 16)))) return rc;
    if ((rc = m.pre.ensure(((size_t)g.words + 1) * sizeof(int32_t)))) return rc;
    if ((rc = m.kept.ensure(16))) return rc;
    if (W) HIP_TRY(hipMemsetAsync(s->trim_gaps.p, 0, W * sizeof(uint32_t), st));
    fill_row_planes(s, a);
    a.ids = rIds.as<const int32_t>(); a.plane = rPlane.as<const uint8_t>();
    a.n = n_ids; a.W = t.W;
    a.rule = rule; a.arg = rule == TWL_TRIM_TO_ROW ? t.refIndex : arg;
    a.gaps = (uint32_t *)s->trim_gaps.p; a.flags = (uint32_t *)m.flags.p; a.pre = (int32_t *)m.pre.p; a.cols = (int32_t *)s->trim_cols.p; a.kept = (int32_t *)m.kept.p;
    return TWL_OK;
}

// the five launches, between the call's two events
int trim_launch(hipStream_t st, const TrimGrid &g, TrimScratch &m, const twl::TrimArgs &a)
{
    HIP_TRY(hipEventCreate(&m.ev0));
    HIP_TRY(hipEventCreate(&m.ev1));
    HIP_TRY(hipEventRecord(m.ev0, st));
    const dim3 block(twl::kTrThreads);
    if (a.W > 0) {
        hipLaunchKernelGGL(twl::trim_counts_kernel, dim3((unsigned)g.colTiles, (unsigned)g.rowSlices), block, 0, st, a);
        hipLaunchKernelGGL(twl::trim_bits_kernel, dim3((unsigned)g.colBlocks), block, 0, st, a);
    }
    hipLaunchKernelGGL(twl::trim_scan_kernel, dim3(1), block, 0, st, a);
    if (a.W > 0) {
        hipLaunchKernelGGL(twl::trim_list_kernel, dim3((unsigned)g.colBlocks), block, 0, st, a);
        hipLaunchKernelGGL(twl::trim_compact_kernel, dim3((unsigned)g.colTiles, (unsigned)g.rowsY, (unsigned)g.rowsZ), block, 0, st, a);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(m.ev1, st));
    return TWL_OK;
}

}  // namespace

extern "C" {

int twl_store_trim_columns(twl_store *s, int32_t n_ids, const int32_t *ids, int32_t rule, int32_t arg, int32_t *kept_out)
{
    TrimRows t;
    if (const char *why = check_trim_columns(s != nullptr, n_ids, ids, kept_out != nullptr, rule, arg, s ? s->n_seqs : 0, s ? s->len.data() : nullptr, s && s->prepared,
                                             twl::kTrColTile, t)) { g_err = why; return TWL_ERR_BAD_ARGUMENT; }
    TrimGrid g;
    if (const char *why = plan_trim_grid(t.W, n_ids, twl::kTrColTile, twl::kTrRowSlice, twl::kTrThreads, g)) { g_err = why; return TWL_ERR_BAD_ARGUMENT; }
    if (s->cap % twl::kTrCols != 0 || t.W > s->cap) { g_err = "the store's row pitch is no multiple of 16"; return TWL_ERR_HIP; }
    DEVICE_CALL(call, s->d);
    hipStream_t st = call.st;
    TrimScratch m;
    twl::TrimArgs a{};
    int rc;
    if ((rc = wait_rows(s, st))) return rc;
    s->trim_W = -1;                                                                    // (the store's buffers are rewritten from here on)
    if ((rc = trim_upload(s, st, t, g, n_ids, ids, rule, arg, m, a))) return rc;
    if ((rc = trim_launch(st, g, m, a))) return rc;
    if ((rc = m.back.ensure(sizeof(int32_t)))) return rc;
    HIP_TRY(hipMemcpyAsync(m.back.p, m.kept.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, m.ev0, m.ev1));
    s->trim_ms = ms;
    memcpy(kept_out, m.back.p, sizeof(int32_t));
    rows_rewritten(s, std::vector<int32_t>(ids, ids + n_ids), *kept_out);
    s->trim_W = t.W; s->trim_kept = *kept_out;
    return TWL_OK;
}

int twl_store_trim_read(twl_store *s, int32_t *cols_out, uint32_t *gaps_out)
{
    if (!s) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    if (s->trim_W < 0) { g_err = "no twl_store_trim_columns has run on this store"; return TWL_ERR_BAD_ARGUMENT; }
    DEVICE_CALL(call, s->d);
    if (cols_out && s->trim_kept > 0) HIP_TRY(hipMemcpyAsync(cols_out, s->trim_cols.p, (size_t)s->trim_kept * sizeof(int32_t), hipMemcpyDeviceToHost, call.st));
    if (gaps_out && s->trim_W > 0) HIP_TRY(hipMemcpyAsync(gaps_out, s->trim_gaps.p, (size_t)s->trim_W * sizeof(uint32_t), hipMemcpyDeviceToHost, call.st));
    HIP_TRY(hipStreamSynchronize(call.st));
    return TWL_OK;
}

int twl_store_trim_timing(twl_store *s, double *ms)
{
    if (!s || !ms) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    *ms = s->trim_ms;
    return TWL_OK;
}

int twl_trim_describe(int32_t out[4])
{
    if (!out) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    out[0] = twl::kTrColTile; out[1] = twl::kTrRowSlice; out[2] = twl::kTrScanChunk; out[3] = twl::kTrFlush;
    return TWL_OK;
}

}  // extern "C"
