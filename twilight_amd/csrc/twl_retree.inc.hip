// twilight_amd/csrc/twl_retree.inc.hip -- host side of include/twl_retree.h: the gap counts of the columns and the pair counts of the rows of a
// finished alignment.  Included at the end of twl_align.hip, behind twl_guide.inc.hip (guide_now_ms).  What the calls reject is decided in
// twl_retree_plan.inc.hip (pure); this file allocates, uploads, launches and downloads, as named steps over one RetreeRun.

#include "twl_retree_plan.inc.hip"

namespace {

static_assert(kRetreeMaxSeqs == TWL_RETREE_MAX_SEQS, "the cap of the plan and of the header are one number");
static_assert(twl::kRetreeTile == 64 && twl::kRetreeThreads == 256 && twl::kRetreeWordCols == 64, "4 x 4 pairs per thread, one ballot per word");
static_assert(twl::kRetreeSlice % (twl::kRetreeThreads / 64) == 0, "the pack kernel's workgroups cover the padded words exactly");

struct RetreeTiming { double upload_ms = 0, gaps_ms = 0, pack_ms = 0, pairs_ms = 0, download_ms = 0; };
std::unordered_map<int, RetreeTiming> g_retree_timing;     // by device id
std::mutex g_retree_mu;                                    // ... guards the map

// The device memory of one call; freed when the call ends, however it ends.
struct RetreeRun {
    void *rows = nullptr, *gaps = nullptr, *planes = nullptr, *match = nullptr, *both = nullptr;
    int32_t n = 0, width = 0;
    int64_t words_pad = 0;
    char type = 'n';
    ~RetreeRun() { for (void *p : {rows, gaps, planes, match, both}) if (p) (void)hipFree(p); }
};

// step 0: the whole call must fit the free memory of the device (pairs false: rows and gap counts alone)
int retree_fits(const RetreeRun &g, bool pairs)
{
    size_t free_b = 0, all_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &all_b));
    const uint64_t need = pairs ? retree_device_bytes(g.type, g.n, g.width, g.words_pad) : (uint64_t)g.n * (uint64_t)g.width + (uint64_t)g.width * 4;
    if (need > free_b) {
        g_err = "out of device memory: " + std::to_string(g.n) + " rows of " + std::to_string(g.width) + " columns need " + std::to_string(need) + " bytes, " +
                std::to_string(free_b) + " are free";
        return TWL_ERR_HIP;
    }
    return TWL_OK;
}

// step 1: the rows back to back, n x width bytes, into device memory
int retree_upload(RetreeRun &g, hipStream_t st, const char *const *rows)
{
    std::vector<unsigned char> flat((size_t)g.n * (size_t)g.width);
    for (int32_t i = 0; i < g.n; ++i) memcpy(flat.data() + (size_t)i * (size_t)g.width, rows[i], (size_t)g.width);
    HIP_TRY(hipMalloc(&g.rows, flat.size()));
    HIP_TRY(hipMemcpyAsync(g.rows, flat.data(), flat.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));      // (the host block above ends with this function)
    return TWL_OK;
}

// step 2: gaps[width]
int retree_gaps(RetreeRun &g, hipStream_t st)
{
    HIP_TRY(hipMalloc(&g.gaps, (size_t)g.width * sizeof(uint32_t)));
    HIP_TRY(hipMemsetAsync(g.gaps, 0, (size_t)g.width * sizeof(uint32_t), st));
    const dim3 grid((unsigned)(((int64_t)g.width + twl::kRetreeThreads - 1) / twl::kRetreeThreads), (unsigned)((g.n + twl::kRetreeGapRows - 1) / twl::kRetreeGapRows));
    hipLaunchKernelGGL(twl::retree_gap_kernel, grid, dim3(twl::kRetreeThreads), 0, st, (const unsigned char *)g.rows, g.n, g.width, (uint32_t *)g.gaps);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return TWL_OK;
}

// step 3: planes[n][P][words_pad]
int retree_pack(RetreeRun &g, hipStream_t st, int32_t max_gaps)
{
    const int P = retree_planes(g.type);
    HIP_TRY(hipMalloc(&g.planes, (size_t)g.n * (size_t)P * (size_t)g.words_pad * sizeof(unsigned long long)));
    const dim3 grid((unsigned)(g.words_pad / (twl::kRetreeThreads / 64)), (unsigned)g.n), block(twl::kRetreeThreads);
    if (P == 3)
        hipLaunchKernelGGL(twl::retree_pack_kernel<3>, grid, block, 0, st, (const unsigned char *)g.rows, (const uint32_t *)g.gaps, g.width, (uint32_t)max_gaps, (long long)g.words_pad,
                           (unsigned long long *)g.planes);
    else
        hipLaunchKernelGGL(twl::retree_pack_kernel<6>, grid, block, 0, st, (const unsigned char *)g.rows, (const uint32_t *)g.gaps, g.width, (uint32_t)max_gaps, (long long)g.words_pad,
                           (unsigned long long *)g.planes);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return TWL_OK;
}

// step 4: match[n][n], both[n][n]
int retree_pairs(RetreeRun &g, hipStream_t st)
{
    HIP_TRY(hipMalloc(&g.match, (size_t)g.n * (size_t)g.n * sizeof(uint32_t)));
    HIP_TRY(hipMalloc(&g.both, (size_t)g.n * (size_t)g.n * sizeof(uint32_t)));
    const unsigned tiles = (unsigned)((g.n + twl::kRetreeTile - 1) / twl::kRetreeTile);
    const dim3 grid(tiles, tiles), block(twl::kRetreeThreads);
    if (retree_planes(g.type) == 3)
        hipLaunchKernelGGL(twl::retree_pair_kernel<3>, grid, block, 0, st, (const unsigned long long *)g.planes, g.n, (long long)g.words_pad, (uint32_t *)g.match, (uint32_t *)g.both);
    else
        hipLaunchKernelGGL(twl::retree_pair_kernel<6>, grid, block, 0, st, (const unsigned long long *)g.planes, g.n, (long long)g.words_pad, (uint32_t *)g.match, (uint32_t *)g.both);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return TWL_OK;
}

int retree_begin(RetreeRun &g, const char *why, char type, int32_t n, int32_t width, Device **d, int device)
{
    if (why) { g_err = why; return TWL_ERR_BAD_ARGUMENT; }
    if (!g_init) { g_err = "twl_init not called"; return TWL_ERR_NOT_INITIALIZED; }
    g.n = n; g.width = width; g.type = type;
    g.words_pad = retree_words_padded(width, twl::kRetreeWordCols, twl::kRetreeSlice);
    return find_dev(device, d);
}

}  // namespace

extern "C" {

int twl_retree_describe(int32_t out[4])
{
    if (!out) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    out[0] = twl::kRetreeWordCols; out[1] = twl::kRetreeTile; out[2] = twl::kRetreeSlice; out[3] = twl::kRetreeGapRows;
    return 4;
}

int twl_retree_column_gaps(int device, int32_t n, int32_t width, const char *const *rows, uint32_t *gaps_out)
{
    RetreeRun g;
    Device *d = nullptr;
    int rc = retree_begin(g, check_retree_gaps(n, width, rows, gaps_out), 'n', n, width, &d, device);
    if (rc) return rc;
    DEVICE_CALL(call, d);
    if ((rc = retree_fits(g, false))) return rc;
    if ((rc = retree_upload(g, call.st, rows))) return rc;
    if ((rc = retree_gaps(g, call.st))) return rc;
    HIP_TRY(hipMemcpy(gaps_out, g.gaps, (size_t)width * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return TWL_OK;
}

int twl_retree_pair_counts(int device, char type, int32_t n, int32_t width, const char *const *rows, int32_t max_gaps, uint32_t *match_out, uint32_t *both_out, int32_t *kept_out)
{
    RetreeRun g;
    Device *d = nullptr;
    int rc = retree_begin(g, check_retree_pairs(type, n, width, rows, max_gaps, match_out, both_out, kept_out), type, n, width, &d, device);
    if (rc) return rc;
    DEVICE_CALL(call, d);
    if ((rc = retree_fits(g, true))) return rc;
    RetreeTiming t;
    double t0 = guide_now_ms(), t1;
    if ((rc = retree_upload(g, call.st, rows))) return rc;
    t.upload_ms = (t1 = guide_now_ms()) - t0;
    if ((rc = retree_gaps(g, call.st))) return rc;
    t.gaps_ms = (t0 = guide_now_ms()) - t1;
    if ((rc = retree_pack(g, call.st, max_gaps))) return rc;
    t.pack_ms = (t1 = guide_now_ms()) - t0;
    if ((rc = retree_pairs(g, call.st))) return rc;
    t.pairs_ms = (t0 = guide_now_ms()) - t1;
    std::vector<uint32_t> gaps((size_t)width);
    HIP_TRY(hipMemcpy(gaps.data(), g.gaps, gaps.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(match_out, g.match, (size_t)n * (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(both_out, g.both, (size_t)n * (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    t.download_ms = guide_now_ms() - t0;
    int32_t kept = 0;
    for (uint32_t c : gaps) kept += c <= (uint32_t)max_gaps ? 1 : 0;
    *kept_out = kept;
    { std::lock_guard<std::mutex> tl(g_retree_mu); g_retree_timing[d->id] = t; }
    return TWL_OK;
}

int twl_retree_timing(int device, double *upload_ms, double *gaps_ms, double *pack_ms, double *pairs_ms, double *download_ms)
{
    if (!g_init) { g_err = "twl_init not called"; return TWL_ERR_NOT_INITIALIZED; }
    if (!upload_ms || !gaps_ms || !pack_ms || !pairs_ms || !download_ms) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    Device *d = nullptr;
    const int rc = find_dev(device, &d);
    if (rc) return rc;
    std::lock_guard<std::mutex> tl(g_retree_mu);
    const RetreeTiming t = g_retree_timing[d->id];
    *upload_ms = t.upload_ms; *gaps_ms = t.gaps_ms; *pack_ms = t.pack_ms; *pairs_ms = t.pairs_ms; *download_ms = t.download_ms;
    return TWL_OK;
}

}  // extern "C"
