// twilight_amd/csrc/twl_retree_set.inc.hip -- host side of include/twl_retree_set.h: the bit-planes of up to 2^20 rows of a finished alignment kept
// in HBM, every row assigned to its closest seed row, and the pair counts of groups of rows (the two-stage rebuilt guide tree, DESIGN.md
// section 4j).  Included at the end of twl_align.hip, behind twl_guide_set.inc.hip (GuideScratch) and twl_retree.inc.hip, whose gap and pack
// kernels it launches.  What the calls reject is decided in twl_retree_set_plan.inc.hip (pure); this file allocates, uploads, launches and
// downloads.

#include "twl_retree_set_plan.inc.hip"

struct twl_retree_set {
    Device *d = nullptr;
    void *rows = nullptr, *gaps = nullptr;                    // leave again before twl_retree_set_create returns
    void *planes = nullptr, *letters = nullptr;               // stay
    int32_t n = 0, width = 0;
    int64_t words_pad = 0;
    char type = 'n';
    double upload_ms = 0, gaps_ms = 0, pack_ms = 0, assign_ms = 0, groups_ms = 0, download_ms = 0;      // summed over the calls on this set
    ~twl_retree_set() { for (void *p : {rows, gaps, planes, letters}) if (p) (void)hipFree(p); }
};

namespace {

static_assert(kRetreeSetMaxSeqs == TWL_RETREE_SET_MAX_SEQS && kRetreeSetMaxSeeds == TWL_RETREE_MAX_SEQS, "the caps of the plan and of the headers are the same numbers");
static_assert(sizeof(twl::RetreeGroupTile) == sizeof(GuideGroupTilePlan) && offsetof(twl::RetreeGroupTile, block) == offsetof(GuideGroupTilePlan, block),
              "the tile list of the plan is uploaded as the kernel reads it");
static_assert(kRetreePackMaxRows <= 65535, "blockIdx.y of the pack kernel");
constexpr unsigned kRetreeMaxGridX = 65535;      // no launch of this file has a larger grid dimension

int retree_set_fits(uint64_t need, const char *what)
{
    size_t free_b = 0, all_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &all_b));
    if (need > free_b) {
        g_err = std::string("out of device memory: ") + what + " needs " + std::to_string(need) + " bytes, " + std::to_string(free_b) + " are free";
        return TWL_ERR_HIP;
    }
    return TWL_OK;
}

// step 1: the rows back to back, n x width bytes, into device memory, through one host block of at most kRetreeStageBytes (or one row)
int retree_set_upload(twl_retree_set &s, hipStream_t st, const char *const *rows)
{
    HIP_TRY(hipMalloc(&s.rows, (size_t)s.n * (size_t)s.width));
    const int32_t per = retree_stage_rows(s.n, s.width);
    std::vector<unsigned char> flat((size_t)per * (size_t)s.width);
    for (int32_t k = 0; k < retree_slabs(s.n, per); ++k) {
        int32_t first = 0, count = 0;
        retree_slab(s.n, per, k, &first, &count);
        for (int32_t i = 0; i < count; ++i) memcpy(flat.data() + (size_t)i * (size_t)s.width, rows[first + i], (size_t)s.width);
        HIP_TRY(hipMemcpyAsync((unsigned char *)s.rows + (size_t)first * (size_t)s.width, flat.data(), (size_t)count * (size_t)s.width, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));      // (the host block is filled again next)
    }
    return TWL_OK;
}

// step 2: gaps[width] over all rows; *kept = the columns the mask keeps
int retree_set_gaps(twl_retree_set &s, hipStream_t st, int32_t max_gaps, int32_t *kept)
{
    HIP_TRY(hipMalloc(&s.gaps, (size_t)s.width * sizeof(uint32_t)));
    HIP_TRY(hipMemsetAsync(s.gaps, 0, (size_t)s.width * sizeof(uint32_t), st));
    const dim3 grid((unsigned)(((int64_t)s.width + twl::kRetreeThreads - 1) / twl::kRetreeThreads), (unsigned)((s.n + twl::kRetreeGapRows - 1) / twl::kRetreeGapRows));
    hipLaunchKernelGGL(twl::retree_gap_kernel, grid, dim3(twl::kRetreeThreads), 0, st, (const unsigned char *)s.rows, s.n, s.width, (uint32_t *)s.gaps);
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> gaps((size_t)s.width);
    HIP_TRY(hipMemcpyAsync(gaps.data(), s.gaps, gaps.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *kept = 0;
    for (uint32_t c : gaps) *kept += c <= (uint32_t)max_gaps ? 1 : 0;
    return TWL_OK;
}

// step 3: planes[n][P][words_pad], one launch of the pack kernel per slab of rows (its blockIdx.y is the row of the slab), and letters[n]
template <int P> int retree_set_pack(twl_retree_set &s, hipStream_t st, int32_t max_gaps)
{
    HIP_TRY(hipMalloc(&s.planes, (size_t)s.n * P * (size_t)s.words_pad * sizeof(unsigned long long)));
    HIP_TRY(hipMalloc(&s.letters, (size_t)s.n * sizeof(uint32_t)));
    for (int32_t k = 0; k < retree_slabs(s.n, kRetreePackMaxRows); ++k) {
        int32_t first = 0, count = 0;
        retree_slab(s.n, kRetreePackMaxRows, k, &first, &count);
        const dim3 grid((unsigned)(s.words_pad / (twl::kRetreeThreads / 64)), (unsigned)count);
        hipLaunchKernelGGL(twl::retree_pack_kernel<P>, grid, dim3(twl::kRetreeThreads), 0, st, (const unsigned char *)s.rows + (size_t)first * (size_t)s.width, (const uint32_t *)s.gaps,
                           s.width, (uint32_t)max_gaps, (long long)s.words_pad, (unsigned long long *)s.planes + (size_t)first * P * (size_t)s.words_pad);
        HIP_TRY(hipGetLastError());
    }
    const unsigned blocks = (unsigned)std::min<int64_t>(((int64_t)s.n + twl::kRetreeThreads / 64 - 1) / (twl::kRetreeThreads / 64), kRetreeMaxGridX);
    hipLaunchKernelGGL(twl::retree_letters_kernel<P>, dim3(blocks), dim3(twl::kRetreeThreads), 0, st, (const unsigned long long *)s.planes, s.n, (long long)s.words_pad, (uint32_t *)s.letters);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return TWL_OK;
}

}  // namespace

extern "C" {

int twl_retree_set_describe(int32_t out[4])
{
    if (!out) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    out[0] = twl::kRetreeTile; out[1] = twl::kRetreeTile; out[2] = twl::kRetreeTile; out[3] = kRetreePackMaxRows;
    return 4;
}

int twl_retree_set_create(int device, char type, int32_t n, int32_t width, const char *const *rows, int32_t max_gaps, twl_retree_set **set, int32_t *kept_out)
{
    if (const char *why = check_retree_set_create(type, n, width, rows, max_gaps, set, kept_out)) { g_err = why; return TWL_ERR_BAD_ARGUMENT; }
    *set = nullptr;
    if (!g_init) { g_err = "twl_init not called"; return TWL_ERR_NOT_INITIALIZED; }
    Device *d = nullptr;
    int rc = find_dev(device, &d);
    if (rc) return rc;
    std::unique_ptr<twl_retree_set> s(new twl_retree_set);
    s->d = d; s->n = n; s->width = width; s->type = type;
    s->words_pad = retree_words_padded(width, twl::kRetreeWordCols, twl::kRetreeSlice);
    DEVICE_CALL(call, d);
    if ((rc = retree_set_fits(retree_set_create_bytes(type, n, width, s->words_pad), "a set of rows"))) return rc;
    double t0 = guide_now_ms(), t1;
    if ((rc = retree_set_upload(*s, call.st, rows))) return rc;
    s->upload_ms = (t1 = guide_now_ms()) - t0;
    if ((rc = retree_set_gaps(*s, call.st, max_gaps, kept_out))) return rc;
    s->gaps_ms = (t0 = guide_now_ms()) - t1;
    if ((rc = retree_planes(type) == 3 ? retree_set_pack<3>(*s, call.st, max_gaps) : retree_set_pack<6>(*s, call.st, max_gaps))) return rc;
    for (void **p : {&s->rows, &s->gaps}) { (void)hipFree(*p); *p = nullptr; }
    s->pack_ms = guide_now_ms() - t0;
    d->live_stores += 1;      // (a set holds the device as a store does: twl_shutdown waits for it)
    *set = s.release();
    return TWL_OK;
}

int twl_retree_set_destroy(twl_retree_set *set)
{
    if (!set) return TWL_OK;
    {
        DeviceCall call(set->d);      // (the memory is freed either way)
        set->d->live_stores -= 1;
        delete set;
    }
    return TWL_OK;
}

int twl_retree_set_letters(twl_retree_set *set, uint32_t *out)
{
    if (!set || !out) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    DEVICE_CALL(call, set->d);
    const double t0 = guide_now_ms();
    HIP_TRY(hipMemcpy(out, set->letters, (size_t)set->n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    set->download_ms += guide_now_ms() - t0;
    return TWL_OK;
}

int twl_retree_set_assign(twl_retree_set *set, int32_t n_seeds, const int32_t *seed_ids, int32_t *seed_out, uint32_t *match_out, uint32_t *both_out)
{
    if (const char *why = check_retree_set_assign(set != nullptr, set ? set->n : 0, n_seeds, seed_ids, seed_out)) { g_err = why; return TWL_ERR_BAD_ARGUMENT; }
    const twl_retree_set &s = *set;
    DEVICE_CALL(call, set->d);
    int rc;
    if ((rc = retree_set_fits((uint64_t)n_seeds * 4 + 3 * (uint64_t)s.n * 4, "an assignment"))) return rc;
    GuideScratch mem;
    void *d_seeds = nullptr, *d_out = nullptr, *d_match = nullptr, *d_both = nullptr;
    if ((rc = mem.get(&d_seeds, (size_t)n_seeds * sizeof(int32_t)))) return rc;
    if ((rc = mem.get(&d_out, (size_t)s.n * sizeof(int32_t)))) return rc;
    if (match_out && (rc = mem.get(&d_match, (size_t)s.n * sizeof(uint32_t)))) return rc;
    if (both_out && (rc = mem.get(&d_both, (size_t)s.n * sizeof(uint32_t)))) return rc;
    const double t0 = guide_now_ms();
    HIP_TRY(hipMemcpyAsync(d_seeds, seed_ids, (size_t)n_seeds * sizeof(int32_t), hipMemcpyHostToDevice, call.st));
    const dim3 grid((unsigned)((s.n + twl::kRetreeTile - 1) / twl::kRetreeTile)), block(twl::kRetreeThreads);      // at most 2^20 / 64 workgroups
    if (retree_planes(s.type) == 3)
        hipLaunchKernelGGL(twl::retree_assign_kernel<3>, grid, block, 0, call.st, (const unsigned long long *)s.planes, (const uint32_t *)s.letters, s.n, (long long)s.words_pad,
                           (const int32_t *)d_seeds, n_seeds, (int32_t *)d_out, (uint32_t *)d_match, (uint32_t *)d_both);
    else
        hipLaunchKernelGGL(twl::retree_assign_kernel<6>, grid, block, 0, call.st, (const unsigned long long *)s.planes, (const uint32_t *)s.letters, s.n, (long long)s.words_pad,
                           (const int32_t *)d_seeds, n_seeds, (int32_t *)d_out, (uint32_t *)d_match, (uint32_t *)d_both);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(call.st));
    const double t1 = guide_now_ms();
    set->assign_ms += t1 - t0;
    HIP_TRY(hipMemcpy(seed_out, d_out, (size_t)s.n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (match_out) HIP_TRY(hipMemcpy(match_out, d_match, (size_t)s.n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (both_out) HIP_TRY(hipMemcpy(both_out, d_both, (size_t)s.n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    set->download_ms += guide_now_ms() - t1;
    return TWL_OK;
}

int twl_retree_set_pair_groups(twl_retree_set *set, int32_t n_groups, const int32_t *group_off, const int32_t *ids, uint32_t *match_out, uint32_t *both_out)
{
    uint64_t words = 0;
    if (const char *why = check_retree_set_groups(set != nullptr, set ? set->n : 0, n_groups, group_off, ids, match_out, both_out, &words)) { g_err = why; return TWL_ERR_BAD_ARGUMENT; }
    const twl_retree_set &s = *set;
    const std::vector<GuideGroupTilePlan> tiles = plan_guide_groups(n_groups, group_off, twl::kRetreeTile);
    DEVICE_CALL(call, set->d);
    int rc;
    if ((rc = retree_set_fits(tiles.size() * sizeof(GuideGroupTilePlan) + (uint64_t)group_off[n_groups] * 4 + 2 * words * 4, "the groups' matrices"))) return rc;
    GuideScratch mem;
    void *d_tiles = nullptr, *d_ids = nullptr, *d_match = nullptr, *d_both = nullptr;
    if ((rc = mem.get(&d_tiles, tiles.size() * sizeof(GuideGroupTilePlan)))) return rc;
    if ((rc = mem.get(&d_ids, (size_t)group_off[n_groups] * sizeof(int32_t)))) return rc;
    if ((rc = mem.get(&d_match, (size_t)words * sizeof(uint32_t)))) return rc;
    if ((rc = mem.get(&d_both, (size_t)words * sizeof(uint32_t)))) return rc;
    const double t0 = guide_now_ms();
    HIP_TRY(hipMemcpyAsync(d_tiles, tiles.data(), tiles.size() * sizeof(GuideGroupTilePlan), hipMemcpyHostToDevice, call.st));
    HIP_TRY(hipMemcpyAsync(d_ids, ids, (size_t)group_off[n_groups] * sizeof(int32_t), hipMemcpyHostToDevice, call.st));
    for (size_t first = 0; first < tiles.size(); first += kRetreeMaxGridX) {
        const dim3 grid((unsigned)std::min<size_t>(tiles.size() - first, kRetreeMaxGridX)), block(twl::kRetreeThreads);
        const twl::RetreeGroupTile *list = (const twl::RetreeGroupTile *)d_tiles + first;
        if (retree_planes(s.type) == 3)
            hipLaunchKernelGGL(twl::retree_groups_kernel<3>, grid, block, 0, call.st, (const unsigned long long *)s.planes, (long long)s.words_pad, list, (const int32_t *)d_ids,
                               (uint32_t *)d_match, (uint32_t *)d_both);
        else
            hipLaunchKernelGGL(twl::retree_groups_kernel<6>, grid, block, 0, call.st, (const unsigned long long *)s.planes, (long long)s.words_pad, list, (const int32_t *)d_ids,
                               (uint32_t *)d_match, (uint32_t *)d_both);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(call.st));      // (the host blocks above are read until here)
    const double t1 = guide_now_ms();
    set->groups_ms += t1 - t0;
    HIP_TRY(hipMemcpy(match_out, d_match, (size_t)words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(both_out, d_both, (size_t)words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    set->download_ms += guide_now_ms() - t1;
    return TWL_OK;
}

int twl_retree_set_timing(twl_retree_set *set, double *upload_ms, double *gaps_ms, double *pack_ms, double *assign_ms, double *groups_ms, double *download_ms)
{
    if (!set || !upload_ms || !gaps_ms || !pack_ms || !assign_ms || !groups_ms || !download_ms) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    std::lock_guard<std::mutex> lk(set->d->mu);
    *upload_ms = set->upload_ms; *gaps_ms = set->gaps_ms; *pack_ms = set->pack_ms; *assign_ms = set->assign_ms; *groups_ms = set->groups_ms; *download_ms = set->download_ms;
    return TWL_OK;
}

}  // extern "C"
