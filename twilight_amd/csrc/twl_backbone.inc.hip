// twilight_amd/csrc/twl_backbone.inc.hip -- host side of include/twl_backbone.h: the all-gap columns taken out of every group of backbone rows.
// Included at the end of twl_align.hip, behind twl_store.inc.hip: it works on the store's rows.
//
// What a call rejects and the tile list of its first kernel are decided in twl_backbone_plan.inc.hip (pure); this file allocates, uploads,
// launches and reads back.  A call in steps: check_squeeze_groups, plan_squeeze_tiles, squeeze_upload (one copy of every table),
// squeeze_launch (flags, scan, compaction: three launches whatever the number of groups, nothing waits in between), the read-back of
// len_out, squeeze_book (plane flags and lengths of the rewritten rows).

#include "twl_backbone_plan.inc.hip"

static_assert(sizeof(SqueezeTilePlan) == sizeof(twl::SqueezeTile), "the planned tile list is what squeeze_flags_kernel reads");

namespace {

// The device memory of one call: freed when the call returns, behind its synchronisation.
struct SqueezeScratch {
    Buf flags, pre, lenOut;
    Arena up;
    PinBuf back;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    ~SqueezeScratch()
    {
        for (Buf *b : {&flags, &pre, &lenOut}) b->release();
        up.release(); back.release();
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
};

// every table of the call in one copy; the kernels' arguments point into it
int squeeze_upload(twl_store *s, hipStream_t st, const SqueezeGroups &g, const std::vector<SqueezeTilePlan> &tiles, int32_t n_rows, const int32_t *ids, SqueezeScratch &m,
                   twl::SqueezeArgs &a)
{
    std::vector<uint8_t> plane((size_t)n_rows);
    for (int32_t k = 0; k < n_rows; ++k) plane[k] = s->plane[ids[k]];
    Ref rIds, rPlane, rGroup, rLen, rFlagOff, rPreOff, rTiles;
    int rc;
    if ((rc = m.up.begin((size_t)n_rows * (2 * sizeof(int32_t) + 1) + g.len.size() * (sizeof(int32_t) + 2 * sizeof(int64_t)) + tiles.size() * sizeof(SqueezeTilePlan), 7))) return rc;
    m.up.put(rIds, ids, (size_t)n_rows); m.up.put(rPlane, plane); m.up.put(rGroup, g.rowGroup); m.up.put(rLen, g.len);
    m.up.put(rFlagOff, g.flagOff); m.up.put(rPreOff, g.preOff); m.up.put(rTiles, tiles);
    if ((rc = m.up.flush(st))) return rc;
    if ((rc = m.flags.ensure(std::max<size_t>((size_t)g.flagWords * sizeof(uint32_t), 16)))) return rc;
    if ((rc = m.pre.ensure((size_t)g.preInts * sizeof(int32_t)))) return rc;
    if ((rc = m.lenOut.ensure(g.len.size() * sizeof(int32_t)))) return rc;
    if (g.flagWords) HIP_TRY(hipMemsetAsync(m.flags.p, 0, (size_t)g.flagWords * sizeof(uint32_t), st));
    fill_row_planes(s, a);
    a.ids = rIds.as<const int32_t>(); a.plane = rPlane.as<const uint8_t>(); a.row_group = rGroup.as<const int32_t>();
    a.len = rLen.as<const int32_t>(); a.flag_off = rFlagOff.as<const int64_t>(); a.pre_off = rPreOff.as<const int64_t>();
    a.flags = (uint32_t *)m.flags.p; a.pre = (int32_t *)m.pre.p; a.len_out = (int32_t *)m.lenOut.p;
    a.tiles = rTiles.as<const twl::SqueezeTile>();
    return TWL_OK;
}

// the three launches, between the call's two events
int squeeze_launch(hipStream_t st, const SqueezeGroups &g, size_t nTiles, int32_t n_rows, SqueezeScratch &m, const twl::SqueezeArgs &a)
{
    HIP_TRY(hipEventCreate(&m.ev0));
    HIP_TRY(hipEventCreate(&m.ev1));
    HIP_TRY(hipEventRecord(m.ev0, st));
    if (nTiles) hipLaunchKernelGGL(twl::squeeze_flags_kernel, dim3((unsigned)nTiles), dim3(twl::kSqThreads), 0, st, a);
    hipLaunchKernelGGL(twl::squeeze_scan_kernel, dim3((unsigned)g.len.size()), dim3(twl::kSqThreads), 0, st, a);
    if (g.maxLen > 0)
        hipLaunchKernelGGL(twl::squeeze_compact_kernel, dim3((unsigned)n_rows, (unsigned)((g.maxLen + twl::kSqColTile - 1) / twl::kSqColTile)), dim3(twl::kSqThreads), 0, st, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(m.ev1, st));
    return TWL_OK;
}

// behind the kernels: every listed row lives on its other plane now, at its group's kept length
void squeeze_book(twl_store *s, int32_t n_groups, const int32_t *group_off, const int32_t *ids, const int32_t *kept)
{
    for (int32_t k = 0; k < n_groups; ++k)
        for (int32_t t = group_off[k]; t < group_off[k + 1]; ++t) { s->plane[ids[t]] ^= 1; s->len[ids[t]] = kept[k]; }
}

}  // namespace

extern "C" {

int twl_store_squeeze_groups(twl_store *s, int32_t n_groups, const int32_t *group_off, const int32_t *ids, int32_t *len_out)
{
    if (!s) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    SqueezeGroups g;
    if (const char *why = check_squeeze_groups(n_groups, group_off, ids, len_out != nullptr, s->n_seqs, s->len.data(), s->prepared, g)) { g_err = why; return TWL_ERR_BAD_ARGUMENT; }
    if (n_groups == 0) { s->squeeze_ms = 0; return TWL_OK; }
    if (s->cap % twl::kSqCols != 0) { g_err = "the store's row pitch is no multiple of 16"; return TWL_ERR_HIP; }
    if ((g.maxLen + twl::kSqColTile - 1) / twl::kSqColTile > 65535) { g_err = "rows too long for twl_store_squeeze_groups"; return TWL_ERR_BAD_ARGUMENT; }
    const int32_t n_rows = group_off[n_groups];
    const std::vector<SqueezeTilePlan> tiles = plan_squeeze_tiles(n_groups, group_off, g.len.data(), twl::kSqColTile, twl::kSqRowSlice);
    DEVICE_CALL(call, s->d);
    hipStream_t st = call.st;
    SqueezeScratch m;
    twl::SqueezeArgs a{};
    int rc;
    if ((rc = wait_rows(s, st))) return rc;
    if ((rc = squeeze_upload(s, st, g, tiles, n_rows, ids, m, a))) return rc;
    if ((rc = squeeze_launch(st, g, tiles.size(), n_rows, m, a))) return rc;
    if ((rc = m.back.ensure((size_t)n_groups * sizeof(int32_t)))) return rc;
    HIP_TRY(hipMemcpyAsync(m.back.p, m.lenOut.p, (size_t)n_groups * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, m.ev0, m.ev1));
    s->squeeze_ms = ms;
    memcpy(len_out, m.back.p, (size_t)n_groups * sizeof(int32_t));
    squeeze_book(s, n_groups, group_off, ids, len_out);
    return TWL_OK;
}

int twl_store_squeeze_timing(twl_store *s, double *ms)
{
    if (!s || !ms) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    *ms = s->squeeze_ms;
    return TWL_OK;
}

int twl_squeeze_describe(int32_t *col_tile, int32_t *row_slice, int32_t *scan_chunk)
{
    if (!col_tile || !row_slice || !scan_chunk) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    *col_tile = twl::kSqColTile; *row_slice = twl::kSqRowSlice; *scan_chunk = twl::kSqScanChunk;
    return TWL_OK;
}

}  // extern "C"
