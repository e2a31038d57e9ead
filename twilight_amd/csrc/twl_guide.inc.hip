// twilight_amd/csrc/twl_guide.inc.hip -- host side of include/twl_guide.h: k-mer counts and shared k-mer counts of a set of sequences.
// Included at the end of twl_align.hip, behind twl_store.inc.hip (DEVICE_CALL).  What the calls reject is decided in
// twl_guide_plan.inc.hip (pure); this file allocates, uploads, launches and downloads, as named steps over one GuideRun.

#include "twl_guide_plan.inc.hip"

namespace {

static_assert(kGuideMaxSeqs == TWL_GUIDE_MAX_SEQS, "the cap of the plan and of the header are one number");
static_assert(twl::kGuideSlice * 2 % 16 == 0 && twl::kGuideTile == 64, "the all-pairs kernel stages rows in 16-byte pieces, 4 x 4 pairs per thread");

struct GuideTiming { double count_ms = 0, pairs_ms = 0, download_ms = 0; };
std::unordered_map<int, GuideTiming> g_guide_timing;      // by device id
std::mutex g_guide_mu;                                    // ... guards the map

// The device memory of one call; freed when the call ends, however it ends.
struct GuideRun {
    void *letters = nullptr, *off = nullptr, *len = nullptr, *counts = nullptr, *w = nullptr, *shared = nullptr;
    int32_t n = 0, bins = 0, bins_pad = 0;
    char type = 'n';
    ~GuideRun() { for (void *p : {letters, off, len, counts, w, shared}) if (p) (void)hipFree(p); }
};

double guide_now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// step 1: the letters of all sequences back to back, their offsets and lengths, into device memory
int guide_upload(GuideRun &g, hipStream_t st, const char *const *seqs, const int32_t *lens, uint64_t total)
{
    std::vector<unsigned long long> off((size_t)g.n);
    std::vector<unsigned char> flat((size_t)std::max<uint64_t>(total, 1));
    uint64_t at = 0;
    for (int32_t i = 0; i < g.n; ++i) {
        off[i] = at;
        if (lens[i] > 0) memcpy(flat.data() + at, seqs[i], (size_t)lens[i]);
        at += (uint64_t)lens[i];
    }
    HIP_TRY(hipMalloc(&g.letters, flat.size()));
    HIP_TRY(hipMalloc(&g.off, off.size() * sizeof(unsigned long long)));
    HIP_TRY(hipMalloc(&g.len, (size_t)g.n * sizeof(int32_t)));
    HIP_TRY(hipMemcpyAsync(g.letters, flat.data(), flat.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(g.off, off.data(), off.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(g.len, lens, (size_t)g.n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));      // (the host blocks above end with this function)
    return TWL_OK;
}

// step 2: counts[n][bins_pad] (16 bit, saturated, padding bins zero) and w[n]
int guide_count(GuideRun &g, hipStream_t st)
{
    HIP_TRY(hipMalloc(&g.counts, (size_t)g.n * (size_t)g.bins_pad * sizeof(uint16_t)));
    HIP_TRY(hipMalloc(&g.w, (size_t)g.n * sizeof(uint32_t)));
    const dim3 grid((unsigned)g.n), block(twl::kGuideCountThreads);
    if (g.type == 'n')
        hipLaunchKernelGGL((twl::guide_count_kernel<4, 6, 4096>), grid, block, 0, st, (const unsigned char *)g.letters, (const unsigned long long *)g.off,
                           (const int32_t *)g.len, g.bins_pad, (uint16_t *)g.counts, (uint32_t *)g.w);
    else
        hipLaunchKernelGGL((twl::guide_count_kernel<6, 5, 7776>), grid, block, 0, st, (const unsigned char *)g.letters, (const unsigned long long *)g.off,
                           (const int32_t *)g.len, g.bins_pad, (uint16_t *)g.counts, (uint32_t *)g.w);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return TWL_OK;
}

// step 3: shared[n][n]
int guide_pairs(GuideRun &g, hipStream_t st)
{
    HIP_TRY(hipMalloc(&g.shared, (size_t)g.n * (size_t)g.n * sizeof(uint32_t)));
    const unsigned tiles = (unsigned)((g.n + twl::kGuideTile - 1) / twl::kGuideTile);
    hipLaunchKernelGGL(twl::guide_shared_kernel, dim3(tiles, tiles), dim3(256), 0, st, (const uint16_t *)g.counts, (const uint32_t *)g.w, g.n, g.bins_pad, (uint32_t *)g.shared);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return TWL_OK;
}

int guide_begin(GuideRun &g, char type, int32_t n, const char *const *seqs, const int32_t *lens, const void *out, uint64_t *total, Device **d, int device)
{
    if (const char *why = check_guide(type, n, seqs, lens, out, total)) { g_err = why; return TWL_ERR_BAD_ARGUMENT; }
    if (!g_init) { g_err = "twl_init not called"; return TWL_ERR_NOT_INITIALIZED; }
    g.n = n; g.type = type; g.bins = guide_bins(type); g.bins_pad = guide_bins_padded(g.bins, twl::kGuideSlice);
    return find_dev(device, d);
}

}  // namespace

extern "C" {

int twl_guide_bins(char type)
{
    const int32_t b = guide_bins(type);
    if (b == 0) { g_err = "the type must be 'n' or 'p'"; return TWL_ERR_BAD_ARGUMENT; }
    return b;
}

int twl_guide_describe(int32_t out[4])
{
    if (!out) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    out[0] = twl::kGuideChunk; out[1] = twl::kGuideRound; out[2] = twl::kGuideTile; out[3] = twl::kGuideSlice;
    return 4;
}

int twl_guide_kmer_counts(int device, char type, int32_t n, const char *const *seqs, const int32_t *lens, uint16_t *counts_out)
{
    GuideRun g;
    uint64_t total = 0;
    Device *d = nullptr;
    int rc = guide_begin(g, type, n, seqs, lens, counts_out, &total, &d, device);
    if (rc) return rc;
    DEVICE_CALL(call, d);
    if ((rc = guide_upload(g, call.st, seqs, lens, total))) return rc;
    if ((rc = guide_count(g, call.st))) return rc;
    HIP_TRY(hipMemcpy2D(counts_out, (size_t)g.bins * sizeof(uint16_t), g.counts, (size_t)g.bins_pad * sizeof(uint16_t), (size_t)g.bins * sizeof(uint16_t), (size_t)n,
                        hipMemcpyDeviceToHost));
    return TWL_OK;
}

int twl_guide_shared(int device, char type, int32_t n, const char *const *seqs, const int32_t *lens, uint32_t *shared_out)
{
    GuideRun g;
    uint64_t total = 0;
    Device *d = nullptr;
    int rc = guide_begin(g, type, n, seqs, lens, shared_out, &total, &d, device);
    if (rc) return rc;
    DEVICE_CALL(call, d);
    GuideTiming t;
    double t0 = guide_now_ms();
    if ((rc = guide_upload(g, call.st, seqs, lens, total))) return rc;
    if ((rc = guide_count(g, call.st))) return rc;
    double t1 = guide_now_ms();
    t.count_ms = t1 - t0;
    if ((rc = guide_pairs(g, call.st))) return rc;
    t0 = guide_now_ms();
    t.pairs_ms = t0 - t1;
    HIP_TRY(hipMemcpy(shared_out, g.shared, (size_t)n * (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    t.download_ms = guide_now_ms() - t0;
    { std::lock_guard<std::mutex> tl(g_guide_mu); g_guide_timing[d->id] = t; }
    return TWL_OK;
}

int twl_guide_timing(int device, double *count_ms, double *pairs_ms, double *download_ms)
{
    if (!g_init) { g_err = "twl_init not called"; return TWL_ERR_NOT_INITIALIZED; }
    if (!count_ms || !pairs_ms || !download_ms) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    Device *d = nullptr;
    const int rc = find_dev(device, &d);
    if (rc) return rc;
    std::lock_guard<std::mutex> tl(g_guide_mu);
    const GuideTiming t = g_guide_timing[d->id];
    *count_ms = t.count_ms; *pairs_ms = t.pairs_ms; *download_ms = t.download_ms;
    return TWL_OK;
}

}  // extern "C"
