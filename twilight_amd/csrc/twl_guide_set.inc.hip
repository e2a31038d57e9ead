// twilight_amd/csrc/twl_guide_set.inc.hip -- host side of the twl_guide_set_* calls of include/twl_guide.h: the count panels of up to 2^20 sequences
// kept in HBM, every sequence assigned to its closest seed, and the S-matrices of groups of sequences (the two-stage guide tree, DESIGN.md
// section 4g).  Included at the end of twl_align.hip, behind twl_guide.inc.hip, whose upload and count steps it runs.  What the calls reject is
// decided in twl_guide_set_plan.inc.hip (pure); this file allocates, uploads, launches and downloads.

#include "twl_guide_set_plan.inc.hip"
#include "guide_stage_kernels.hip.h"

struct twl_guide_set {
    Device *d = nullptr;
    GuideRun run;                                             // counts and w stay; letters, offsets and lengths leave after the count kernel
    double count_ms = 0, assign_ms = 0, groups_ms = 0, download_ms = 0;      // summed over the calls on this set
    double permute_ms = 0, strand_assign_ms = 0, opposite_ms = 0, strand_download_ms = 0;      // ... and over the calls of twl_strand.inc.hip
};

namespace {

static_assert(kGuideSetMaxSeqs == TWL_GUIDE_SET_MAX_SEQS, "the cap of the plan and of the header are one number");
static_assert(sizeof(twl::GuideGroupTile) == sizeof(GuideGroupTilePlan) && offsetof(twl::GuideGroupTile, block) == offsetof(GuideGroupTilePlan, block),
              "the tile list of the plan is uploaded as the kernel reads it");

// device memory of one call on a set; freed when the call ends, however it ends
struct GuideScratch {
    std::vector<void *> p;
    int get(void **out, size_t bytes) { HIP_TRY(hipMalloc(out, bytes ? bytes : 1)); p.push_back(*out); return TWL_OK; }
    ~GuideScratch() { for (void *q : p) (void)hipFree(q); }
};

}  // namespace

extern "C" {

int twl_guide_set_create(int device, char type, int32_t n, const char *const *seqs, const int32_t *lens, twl_guide_set **set)
{
    uint64_t total = 0;
    if (const char *why = check_guide_set_create(type, n, seqs, lens, set, &total)) { g_err = why; return TWL_ERR_BAD_ARGUMENT; }
    *set = nullptr;
    if (!g_init) { g_err = "twl_init not called"; return TWL_ERR_NOT_INITIALIZED; }
    Device *d = nullptr;
    int rc = find_dev(device, &d);
    if (rc) return rc;
    std::unique_ptr<twl_guide_set> s(new twl_guide_set);
    s->d = d;
    GuideRun &g = s->run;
    g.n = n; g.type = type; g.bins = guide_bins(type); g.bins_pad = guide_bins_padded(g.bins, twl::kGuideSlice);
    DEVICE_CALL(call, d);
    size_t free_b = 0, all_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &all_b));
    const uint64_t need = (uint64_t)n * (uint64_t)g.bins_pad * sizeof(uint16_t) + total + (uint64_t)n * 16;
    if (need > free_b) {
        g_err = "out of device memory: the count panels of " + std::to_string(n) + " sequences need " + std::to_string(need) + " bytes, " + std::to_string(free_b) + " are free";
        return TWL_ERR_HIP;
    }
    const double t0 = guide_now_ms();
    if ((rc = guide_upload(g, call.st, seqs, lens, total))) return rc;
    if ((rc = guide_count(g, call.st))) return rc;
    for (void **p : {&g.letters, &g.off, &g.len}) { (void)hipFree(*p); *p = nullptr; }
    s->count_ms = guide_now_ms() - t0;
    d->live_stores += 1;      // (a set holds the device as a store does: twl_shutdown waits for it)
    *set = s.release();
    return TWL_OK;
}

int twl_guide_set_destroy(twl_guide_set *set)
{
    if (!set) return TWL_OK;
    {
        DeviceCall call(set->d);      // (the memory is freed either way)
        set->d->live_stores -= 1;
        delete set;
    }
    return TWL_OK;
}

int twl_guide_set_weights(twl_guide_set *set, uint32_t *w_out)
{
    if (!set || !w_out) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    DEVICE_CALL(call, set->d);
    const double t0 = guide_now_ms();
    HIP_TRY(hipMemcpy(w_out, set->run.w, (size_t)set->run.n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    set->download_ms += guide_now_ms() - t0;
    return TWL_OK;
}

int twl_guide_set_assign(twl_guide_set *set, int32_t n_seeds, const int32_t *seed_ids, int32_t *seed_out, uint32_t *shared_out)
{
    if (const char *why = check_guide_set_assign(set != nullptr, set ? set->run.n : 0, n_seeds, seed_ids, seed_out)) { g_err = why; return TWL_ERR_BAD_ARGUMENT; }
    const GuideRun &g = set->run;
    DEVICE_CALL(call, set->d);
    GuideScratch mem;
    void *d_seeds = nullptr, *d_out = nullptr, *d_shared = nullptr;
    int rc;
    if ((rc = mem.get(&d_seeds, (size_t)n_seeds * sizeof(int32_t)))) return rc;
    if ((rc = mem.get(&d_out, (size_t)g.n * sizeof(int32_t)))) return rc;
    if (shared_out && (rc = mem.get(&d_shared, (size_t)g.n * sizeof(uint32_t)))) return rc;
    double t0 = guide_now_ms();
    HIP_TRY(hipMemcpyAsync(d_seeds, seed_ids, (size_t)n_seeds * sizeof(int32_t), hipMemcpyHostToDevice, call.st));
    const unsigned tiles = (unsigned)((g.n + twl::kGuideTile - 1) / twl::kGuideTile);
    hipLaunchKernelGGL(twl::guide_assign_kernel, dim3(tiles), dim3(256), 0, call.st, (const uint16_t *)g.counts, (const uint32_t *)g.w, g.n, g.bins_pad, (const int32_t *)d_seeds,
                       n_seeds, (int32_t *)d_out, (uint32_t *)d_shared);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(call.st));
    double t1 = guide_now_ms();
    set->assign_ms += t1 - t0;
    HIP_TRY(hipMemcpy(seed_out, d_out, (size_t)g.n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (shared_out) HIP_TRY(hipMemcpy(shared_out, d_shared, (size_t)g.n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    set->download_ms += guide_now_ms() - t1;
    return TWL_OK;
}

int twl_guide_set_shared_groups(twl_guide_set *set, int32_t n_groups, const int32_t *group_off, const int32_t *ids, uint32_t *out)
{
    uint64_t words = 0;
    if (const char *why = check_guide_set_groups(set != nullptr, set ? set->run.n : 0, n_groups, group_off, ids, out, &words)) { g_err = why; return TWL_ERR_BAD_ARGUMENT; }
    const GuideRun &g = set->run;
    const std::vector<GuideGroupTilePlan> tiles = plan_guide_groups(n_groups, group_off, twl::kGuideTile);
    DEVICE_CALL(call, set->d);
    GuideScratch mem;
    void *d_tiles = nullptr, *d_ids = nullptr, *d_out = nullptr;
    int rc;
    if ((rc = mem.get(&d_tiles, tiles.size() * sizeof(GuideGroupTilePlan)))) return rc;
    if ((rc = mem.get(&d_ids, (size_t)group_off[n_groups] * sizeof(int32_t)))) return rc;
    if ((rc = mem.get(&d_out, (size_t)words * sizeof(uint32_t)))) return rc;
    double t0 = guide_now_ms();
    HIP_TRY(hipMemcpyAsync(d_tiles, tiles.data(), tiles.size() * sizeof(GuideGroupTilePlan), hipMemcpyHostToDevice, call.st));
    HIP_TRY(hipMemcpyAsync(d_ids, ids, (size_t)group_off[n_groups] * sizeof(int32_t), hipMemcpyHostToDevice, call.st));
    hipLaunchKernelGGL(twl::guide_groups_kernel, dim3((unsigned)tiles.size()), dim3(256), 0, call.st, (const uint16_t *)g.counts, (const uint32_t *)g.w, g.bins_pad,
                       (const twl::GuideGroupTile *)d_tiles, (const int32_t *)d_ids, (uint32_t *)d_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(call.st));      // (the host blocks above are read until here)
    double t1 = guide_now_ms();
    set->groups_ms += t1 - t0;
    HIP_TRY(hipMemcpy(out, d_out, (size_t)words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    set->download_ms += guide_now_ms() - t1;
    return TWL_OK;
}

int twl_guide_set_timing(twl_guide_set *set, double *count_ms, double *assign_ms, double *groups_ms, double *download_ms)
{
    if (!set || !count_ms || !assign_ms || !groups_ms || !download_ms) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    std::lock_guard<std::mutex> lk(set->d->mu);
    *count_ms = set->count_ms; *assign_ms = set->assign_ms; *groups_ms = set->groups_ms; *download_ms = set->download_ms;
    return TWL_OK;
}

}  // extern "C"
