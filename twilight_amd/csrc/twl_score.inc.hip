// twilight_amd/csrc/twl_score.inc.hip -- host side of include/twl_score.h: the exact integers of the affine sum-of-pairs score of the listed rows
// of the store.  Included at the end of twl_align.hip, behind twl_store.inc.hip: it works on the store's rows.
//
// What a call rejects, the grids, the plane padding, the tile-pair list and the terminal runs are decided in twl_score_plan.inc.hip (pure);
// this file allocates, uploads, launches and reads back.  A call in steps: check_score_rows, plan_score_grid, score_upload (one copy of the
// three tables), score_launch (zeroed sums, then pack, counts, products, pairs between four events: nothing waits in between), one
// read-back, score_terminals and the sums on the host.  Nothing of the store is written.

#include "twl_score_plan.inc.hip"

namespace {

// The device memory of one call: freed when the call returns, behind its synchronisation.
struct ScoreScratch {
    Buf present, first, last, cnt, let, gaps, sub, runs;
    Arena up;
    PinBuf back;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    ~ScoreScratch()
    {
        for (Buf *b : {&present, &first, &last, &cnt, &let, &gaps, &sub, &runs}) b->release();
        up.release(); back.release();
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    }
};

// an allocation that fails is refused with the bytes that were asked for
int score_alloc(Buf &b, size_t bytes, const char *what)
{
    const int rc = b.ensure(std::max<size_t>(bytes, 16));
    if (rc) {
        (void)hipGetLastError();
        g_err = std::string("twl_store_score_rows: no device memory for ") + what + ": " + std::to_string(bytes) + " bytes were asked for";
    }
    return rc;
}

// the tables of the call in one copy, the call's buffers, the sums zeroed; the kernels' arguments point into them
int score_upload(twl_store *s, hipStream_t st, const ScoreGrid &g, int32_t n_ids, const int32_t *ids, int32_t W, int32_t K, ScoreScratch &m, twl::SopArgs &a)
{
    std::vector<uint8_t> plane((size_t)n_ids);
    for (int32_t k = 0; k < n_ids; ++k) plane[k] = s->plane[ids[k]];
    std::vector<uint32_t> pairs;
    plan_score_tile_pairs(g.tiles, pairs);
    Ref rIds, rPlane, rPairs;
    int rc;
    const size_t tableBytes = (size_t)n_ids * (sizeof(int32_t) + 1) + pairs.size() * sizeof(uint32_t);
    if ((rc = m.up.begin(tableBytes, 3))) {
        (void)hipGetLastError();
        g_err = "twl_store_score_rows: no memory for the tables of the call: " + std::to_string(tableBytes) + " bytes were asked for";
        return rc;
    }
    m.up.put(rIds, ids, (size_t)n_ids); m.up.put(rPlane, plane); m.up.put(rPairs, pairs);
    if ((rc = m.up.flush(st))) return rc;
    const size_t n = (size_t)n_ids, w = (size_t)W, subN = (size_t)score_sub_entries(K);
    if ((rc = score_alloc(m.present, n * (size_t)g.wordsPad * sizeof(uint64_t), "the bit-planes"))) return rc;
    if ((rc = score_alloc(m.first, n * sizeof(int32_t), "the first letter columns"))) return rc;
    if ((rc = score_alloc(m.last, n * sizeof(int32_t), "the last letter columns"))) return rc;
    if ((rc = score_alloc(m.cnt, (size_t)(K + 1) * w * sizeof(uint32_t), "the class counts"))) return rc;
    if ((rc = score_alloc(m.let, w * sizeof(uint32_t), "the letter counts"))) return rc;
    if ((rc = score_alloc(m.gaps, w * sizeof(uint32_t), "the gap counts"))) return rc;
    if ((rc = score_alloc(m.sub, subN * sizeof(uint64_t), "the products"))) return rc;
    if ((rc = score_alloc(m.runs, n * sizeof(uint64_t), "the run counts"))) return rc;
    HIP_TRY(hipMemsetAsync(m.cnt.p, 0, (size_t)(K + 1) * w * sizeof(uint32_t), st));
    HIP_TRY(hipMemsetAsync(m.sub.p, 0, subN * sizeof(uint64_t), st));
    HIP_TRY(hipMemsetAsync(m.runs.p, 0, n * sizeof(uint64_t), st));
    fill_row_planes(s, a);
    a.ids = rIds.as<const int32_t>(); a.plane = rPlane.as<const uint8_t>(); a.tilePairs = rPairs.as<const uint32_t>();
    a.n = n_ids; a.W = W; a.K = K; a.wordsPad = g.wordsPad;
    a.present = (unsigned long long *)m.present.p; a.first = (int32_t *)m.first.p; a.last = (int32_t *)m.last.p;
    a.cnt = (uint32_t *)m.cnt.p; a.let = (uint32_t *)m.let.p; a.gaps = (uint32_t *)m.gaps.p;
    a.sub = (unsigned long long *)m.sub.p; a.runsRow = (unsigned long long *)m.runs.p;
    return TWL_OK;
}

// the four launches, an event in front of each and one behind the last
int score_launch(hipStream_t st, const ScoreGrid &g, ScoreScratch &m, const twl::SopArgs &a)
{
    for (hipEvent_t &e : m.ev) HIP_TRY(hipEventCreate(&e));
    const dim3 block(twl::kScThreads);
    HIP_TRY(hipEventRecord(m.ev[0], st));
    hipLaunchKernelGGL(twl::score_pack_kernel, dim3((unsigned)a.n), block, 0, st, a);
    HIP_TRY(hipEventRecord(m.ev[1], st));
    hipLaunchKernelGGL(twl::score_counts_kernel, dim3((unsigned)g.colTiles, (unsigned)g.rowSlices), block, 0, st, a);
    hipLaunchKernelGGL(twl::score_products_kernel, dim3((unsigned)g.prodBlocks), block, 0, st, a);
    HIP_TRY(hipEventRecord(m.ev[2], st));
    hipLaunchKernelGGL(twl::score_pairs_kernel, dim3((unsigned)g.tilePairs), block, 0, st, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(m.ev[3], st));
    return TWL_OK;
}

}  // namespace

extern "C" {

int twl_store_score_rows(twl_store *s, int32_t n_ids, const int32_t *ids, char type, uint64_t *sub_out, uint64_t *runs_row_out, uint64_t totals_out[5])
{
    int32_t W = 0;
    if (const char *why = check_score_rows(s != nullptr, n_ids, ids, type, sub_out != nullptr, runs_row_out != nullptr, totals_out != nullptr, s ? s->n_seqs : 0,
                                           s ? s->len.data() : nullptr, s && s->prepared, twl::kScColTile, W)) { g_err = why; return TWL_ERR_BAD_ARGUMENT; }
    ScoreGrid g;
    if (const char *why = plan_score_grid(W, n_ids, twl::kScSlice, twl::kScTile, twl::kScColTile, twl::kScRowSlice, twl::kScProdCols, g)) { g_err = why; return TWL_ERR_BAD_ARGUMENT; }
    if (s->cap % twl::kScCols != 0 || W > s->cap) { g_err = "the store's row pitch is no multiple of 4"; return TWL_ERR_HIP; }
    const int32_t K = score_classes(type);
    DEVICE_CALL(call, s->d);
    hipStream_t st = call.st;
    ScoreScratch m;
    twl::SopArgs a{};
    int rc;
    if ((rc = wait_rows(s, st))) return rc;
    if ((rc = score_upload(s, st, g, n_ids, ids, W, K, m, a))) return rc;
    if ((rc = score_launch(st, g, m, a))) return rc;
    // one read-back: sub, runs_row, first, last, let, each from an 8-byte boundary
    const size_t n = (size_t)n_ids, w = (size_t)W, subN = (size_t)score_sub_entries(K);
    const size_t oSub = 0, oRuns = oSub + subN * 8, oFirst = oRuns + n * 8, oLast = oFirst + (n * 4 + 7) / 8 * 8, oLet = oLast + (n * 4 + 7) / 8 * 8, total = oLet + w * 4;
    if ((rc = m.back.ensure(total))) {
        (void)hipGetLastError();
        g_err = "twl_store_score_rows: no pinned memory for the read-back: " + std::to_string(total) + " bytes were asked for";
        return rc;
    }
    char *back = (char *)m.back.p;
    HIP_TRY(hipMemcpyAsync(back + oSub, m.sub.p, subN * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(back + oRuns, m.runs.p, n * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(back + oFirst, m.first.p, n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(back + oLast, m.last.p, n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(back + oLet, m.let.p, w * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    float ms[3] = {0, 0, 0};
    for (int k = 0; k < 3; ++k) HIP_TRY(hipEventElapsedTime(&ms[k], m.ev[k], m.ev[k + 1]));
    for (int k = 0; k < 3; ++k) s->score_ms[k] = ms[k];
    memcpy(sub_out, back + oSub, subN * 8);
    memcpy(runs_row_out, back + oRuns, n * 8);
    const uint32_t *let = reinterpret_cast<const uint32_t *>(back + oLet);
    uint64_t R = 0, G = 0, letters = 0, RT = 0, GT = 0;
    for (size_t k = 0; k < n; ++k) R += runs_row_out[k];
    for (size_t c = 0; c < w; ++c) { letters += let[c]; G += (uint64_t)((uint32_t)n_ids - let[c]) * (uint64_t)let[c]; }
    score_terminals(n_ids, W, let, reinterpret_cast<const int32_t *>(back + oFirst), reinterpret_cast<const int32_t *>(back + oLast), RT, GT);
    totals_out[0] = R; totals_out[1] = G; totals_out[2] = RT; totals_out[3] = GT; totals_out[4] = letters;
    return TWL_OK;
}

int twl_store_score_timing(twl_store *s, double *pack_ms, double *columns_ms, double *pairs_ms)
{
    if (!s) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    if (pack_ms) *pack_ms = s->score_ms[0];
    if (columns_ms) *columns_ms = s->score_ms[1];
    if (pairs_ms) *pairs_ms = s->score_ms[2];
    return TWL_OK;
}

int twl_score_describe(int32_t out[4])
{
    if (!out) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    out[0] = twl::kScSlice; out[1] = twl::kScTile; out[2] = twl::kScRowSlice; out[3] = twl::kScFlush;
    return TWL_OK;
}

}  // extern "C"
