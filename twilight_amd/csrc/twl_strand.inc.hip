// twilight_amd/csrc/twl_strand.inc.hip -- host side of the calls of include/twl_strand.h: the opposite-strand counts of a list of rows and
// the direction of every sequence of a twl_guide_set against seeds of known direction (`--adjust-direction`).
// Included at the end of twl_align.hip, behind twl_guide_set.inc.hip, whose set it works on.  What the calls reject is decided in
// twl_strand_plan.inc.hip (pure); this file allocates, uploads, launches and downloads.

#include "twl_strand_plan.inc.hip"
#include "strand_kernels.hip.h"

namespace {

// perm[t][b] = counts[ids[t]][rc(b)] for the `count` rows of d_ids, into a fresh panel of the scratch; the time goes to the set's permute_ms
int strand_permute(twl_guide_set *set, hipStream_t st, GuideScratch &mem, const void *d_ids, int32_t count, void **d_perm)
{
    const GuideRun &g = set->run;
    int rc;
    if ((rc = mem.get(d_perm, (size_t)count * (size_t)g.bins_pad * sizeof(uint16_t)))) return rc;
    const double t0 = guide_now_ms();
    hipLaunchKernelGGL(twl::strand_permute_kernel, dim3((unsigned)count), dim3(256), 0, st, (const uint16_t *)g.counts, g.bins_pad, (const int32_t *)d_ids, (uint16_t *)*d_perm);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    set->permute_ms += guide_now_ms() - t0;
    return TWL_OK;
}

}  // namespace

extern "C" {

int32_t twl_strand_rc_bin(int32_t b) { return strand_rc_bin(b); }

int twl_guide_set_opposite(twl_guide_set *set, int32_t n_ids, const int32_t *ids, uint32_t *out)
{
    if (const char *why = check_strand_opposite(set != nullptr, set ? set->run.type : 0, set ? set->run.n : 0, n_ids, ids, out)) { g_err = why; return TWL_ERR_BAD_ARGUMENT; }
    const GuideRun &g = set->run;
    DEVICE_CALL(call, set->d);
    GuideScratch mem;
    void *d_ids = nullptr, *d_perm = nullptr, *d_out = nullptr;
    int rc;
    const size_t words = (size_t)n_ids * (size_t)n_ids;
    if ((rc = mem.get(&d_ids, (size_t)n_ids * sizeof(int32_t)))) return rc;
    if ((rc = mem.get(&d_out, words * sizeof(uint32_t)))) return rc;
    HIP_TRY(hipMemcpyAsync(d_ids, ids, (size_t)n_ids * sizeof(int32_t), hipMemcpyHostToDevice, call.st));
    if ((rc = strand_permute(set, call.st, mem, d_ids, n_ids, &d_perm))) return rc;
    const double t0 = guide_now_ms();
    const unsigned tiles = (unsigned)((n_ids + twl::kGuideTile - 1) / twl::kGuideTile);
    hipLaunchKernelGGL(twl::strand_opposite_kernel, dim3(tiles, tiles), dim3(256), 0, call.st, (const uint16_t *)g.counts, (const uint32_t *)g.w, g.bins_pad, (const int32_t *)d_ids,
                       (const uint16_t *)d_perm, n_ids, (uint32_t *)d_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(call.st));
    const double t1 = guide_now_ms();
    set->opposite_ms += t1 - t0;
    HIP_TRY(hipMemcpy(out, d_out, words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    set->strand_download_ms += guide_now_ms() - t1;
    return TWL_OK;
}

int twl_guide_set_strand_assign(twl_guide_set *set, int32_t n_seeds, const int32_t *seed_ids, const uint8_t *seed_flip, int32_t *seed_out, uint8_t *dir_out, uint32_t *shared_out)
{
    if (const char *why = check_strand_assign(set != nullptr, set ? set->run.type : 0, set ? set->run.n : 0, n_seeds, seed_ids, seed_flip, seed_out, dir_out)) {
        g_err = why;
        return TWL_ERR_BAD_ARGUMENT;
    }
    const GuideRun &g = set->run;
    DEVICE_CALL(call, set->d);
    GuideScratch mem;
    void *d_seeds = nullptr, *d_flip = nullptr, *d_perm = nullptr, *d_out = nullptr, *d_dir = nullptr, *d_shared = nullptr;
    int rc;
    if ((rc = mem.get(&d_seeds, (size_t)n_seeds * sizeof(int32_t)))) return rc;
    if ((rc = mem.get(&d_flip, (size_t)n_seeds))) return rc;
    if ((rc = mem.get(&d_out, (size_t)g.n * sizeof(int32_t)))) return rc;
    if ((rc = mem.get(&d_dir, (size_t)g.n))) return rc;
    if (shared_out && (rc = mem.get(&d_shared, (size_t)g.n * sizeof(uint32_t)))) return rc;
    HIP_TRY(hipMemcpyAsync(d_seeds, seed_ids, (size_t)n_seeds * sizeof(int32_t), hipMemcpyHostToDevice, call.st));
    HIP_TRY(hipMemcpyAsync(d_flip, seed_flip, (size_t)n_seeds, hipMemcpyHostToDevice, call.st));
    if ((rc = strand_permute(set, call.st, mem, d_seeds, n_seeds, &d_perm))) return rc;
    const double t0 = guide_now_ms();
    const unsigned tiles = (unsigned)((g.n + twl::kGuideTile - 1) / twl::kGuideTile);
    hipLaunchKernelGGL(twl::strand_assign_kernel, dim3(tiles), dim3(256), 0, call.st, (const uint16_t *)g.counts, (const uint32_t *)g.w, g.n, g.bins_pad, (const int32_t *)d_seeds,
                       (const unsigned char *)d_flip, (const uint16_t *)d_perm, n_seeds, (int32_t *)d_out, (unsigned char *)d_dir, (uint32_t *)d_shared);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(call.st));
    const double t1 = guide_now_ms();
    set->strand_assign_ms += t1 - t0;
    HIP_TRY(hipMemcpy(seed_out, d_out, (size_t)g.n * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(dir_out, d_dir, (size_t)g.n, hipMemcpyDeviceToHost));
    if (shared_out) HIP_TRY(hipMemcpy(shared_out, d_shared, (size_t)g.n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    set->strand_download_ms += guide_now_ms() - t1;
    return TWL_OK;
}

int twl_guide_set_strand_timing(twl_guide_set *set, double *permute_ms, double *assign_ms, double *opposite_ms, double *download_ms)
{
    if (!set || !permute_ms || !assign_ms || !opposite_ms || !download_ms) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    std::lock_guard<std::mutex> lk(set->d->mu);
    *permute_ms = set->permute_ms; *assign_ms = set->strand_assign_ms; *opposite_ms = set->opposite_ms; *download_ms = set->strand_download_ms;
    return TWL_OK;
}

}  // extern "C"
