// twilight_amd/csrc/twl_compare.inc.hip -- host side of include/twl_compare.h: an alignment compared with a reference alignment of the same
// sequences.  Included at the end of twl_align.hip, behind twl_trim.inc.hip.
//
// What a call rejects from its arguments, the pitches and the byte counts are decided in twl_compare_plan.inc.hip (pure); this file allocates,
// uploads, launches and reads back.  twl_compare_create in steps: plan_compare, compare_upload (both alignments, padded with '-' to their
// pitch, through one host block), compare_build_keys (zeroed counts, the reference positions, the keys; the one read-back is the bad-row word),
// then the reference positions are freed.  twl_compare_columns: one launch and the copies back.

#include "twl_compare_plan.inc.hip"

struct twl_compare {
    Device *d = nullptr;
    ComparePlan p;
    void *est = nullptr, *ref = nullptr, *pos = nullptr;           // est, ref and pos leave again before twl_compare_create returns
    void *keys = nullptr, *ref_letters = nullptr, *row_letters = nullptr, *bad = nullptr;
    void *shared = nullptr, *letters = nullptr, *distinct = nullptr, *recovered = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    double upload_ms = 0, keys_ms = 0, columns_ms = 0, download_ms = 0;
    ~twl_compare()
    {
        for (void *q : {est, ref, pos, keys, ref_letters, row_letters, bad, shared, letters, distinct, recovered}) if (q) (void)hipFree(q);
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    }
};

namespace {

constexpr int64_t kCompareStageBytes = 64ll << 20;      // the host block both alignments are uploaded through

int compare_alloc(void **out, uint64_t bytes, const char *what)
{
    const size_t want = (size_t)std::max<uint64_t>(bytes, 256);
    if (hipMalloc(out, want) != hipSuccess) {
        (void)hipGetLastError();
        *out = nullptr;
        g_err = std::string("out of device memory: ") + what + " of a comparison need " + std::to_string(want) + " bytes";
        return TWL_ERR_HIP;
    }
    return TWL_OK;
}

// n rows of w bytes into [n][pitch], '-' behind every row
int compare_upload_rows(hipStream_t st, void *dst, int32_t n, int32_t w, int64_t pitch, const char *const *rows)
{
    if (pitch == 0) return TWL_OK;
    const int32_t per = compare_stage_rows(n, pitch, kCompareStageBytes);
    std::vector<char> flat;
    try { flat.resize((size_t)per * (size_t)pitch); }      // (no exception crosses the C ABI)
    catch (const std::bad_alloc &) { g_err = "out of host memory: the upload block of a comparison needs " + std::to_string((size_t)per * (size_t)pitch) + " bytes"; return TWL_ERR_HIP; }
    for (int32_t first = 0; first < n; first += per) {
        const int32_t count = std::min(per, n - first);
        memset(flat.data(), '-', (size_t)count * (size_t)pitch);
        for (int32_t i = 0; i < count; ++i) memcpy(flat.data() + compare_row_at(pitch, i), rows[first + i], (size_t)w);
        HIP_TRY(hipMemcpyAsync((char *)dst + compare_row_at(pitch, first), flat.data(), (size_t)count * (size_t)pitch, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));      // (the host block is filled again next)
    }
    return TWL_OK;
}

twl::CompareArgs compare_args(const twl_compare &c)
{
    twl::CompareArgs a{};
    a.est = (const unsigned char *)c.est; a.ref = (const unsigned char *)c.ref;
    a.pe = c.p.pe; a.pr = c.p.pr;
    a.n = c.p.n; a.we = c.p.we; a.wr = c.p.wr;
    a.pos = (int32_t *)c.pos; a.keys = (int32_t *)c.keys;
    a.ref_letters = (uint32_t *)c.ref_letters; a.row_letters = (uint32_t *)c.row_letters; a.bad = (int32_t *)c.bad;
    a.shared = (unsigned long long *)c.shared; a.letters = (uint32_t *)c.letters; a.distinct = (uint32_t *)c.distinct; a.recovered = (uint8_t *)c.recovered;
    return a;
}

// the reference positions and the keys between the object's two events; *bad = the bad-row word (INT32_MAX: every row matches)
int compare_build_keys(twl_compare &c, hipStream_t st, int32_t *bad)
{
    const int32_t none = INT32_MAX;
    HIP_TRY(hipMemsetAsync(c.ref_letters, 0, std::max<size_t>((size_t)c.p.wr * sizeof(uint32_t), 4), st));
    HIP_TRY(hipMemcpyAsync(c.bad, &none, sizeof none, hipMemcpyHostToDevice, st));
    const twl::CompareArgs a = compare_args(c);
    HIP_TRY(hipEventRecord(c.ev[0], st));
    hipLaunchKernelGGL(twl::compare_refpos_kernel, dim3((unsigned)c.p.n), dim3(twl::kCmpThreads), 0, st, a);
    hipLaunchKernelGGL(twl::compare_keys_kernel, dim3((unsigned)c.p.n), dim3(twl::kCmpThreads), 0, st, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c.ev[1], st));
    HIP_TRY(hipMemcpyAsync(bad, c.bad, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c.ev[0], c.ev[1]));
    c.keys_ms = ms;
    return TWL_OK;
}

}  // namespace

extern "C" {

int twl_compare_describe(int32_t out[4])
{
    if (!out) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    out[0] = twl::kCmpWindow; out[1] = twl::kCmpColTile; out[2] = twl::kCmpRowStep; out[3] = twl::kCmpScanChunk;
    return TWL_OK;
}

int twl_compare_create(int device, int32_t n, int32_t w_est, const char *const *est_rows, int32_t w_ref, const char *const *ref_rows, twl_compare **cmp, int32_t *bad_row)
{
    if (cmp) *cmp = nullptr;
    if (bad_row) *bad_row = -1;
    ComparePlan p;
    if (const char *why = plan_compare(n, w_est, est_rows != nullptr, w_ref, ref_rows != nullptr, cmp != nullptr, bad_row != nullptr, twl::kCmpColTile, twl::kCmpScanChunk, p)) {
        g_err = why; return TWL_ERR_BAD_ARGUMENT;
    }
    for (int32_t k = 0; k < n; ++k)
        if ((w_est > 0 && !est_rows[k]) || (w_ref > 0 && !ref_rows[k])) { g_err = "bad argument: a null row"; return TWL_ERR_BAD_ARGUMENT; }
    if (!g_init) { g_err = "twl_init not called"; return TWL_ERR_NOT_INITIALIZED; }
    Device *d = nullptr;
    int rc = find_dev(device, &d);
    if (rc) return rc;
    DEVICE_CALL(call, d);
    std::unique_ptr<twl_compare> c(new (std::nothrow) twl_compare);      // (behind the call's hold on the device: whatever it holds is freed under it on every early return)
    if (!c) { g_err = "out of host memory"; return TWL_ERR_HIP; }
    c->d = d; c->p = p;
    hipStream_t st = call.st;
    if ((rc = compare_alloc(&c->est, p.estBytes, "the rows of the estimate"))) return rc;
    if ((rc = compare_alloc(&c->ref, p.refBytes, "the rows of the reference"))) return rc;
    if ((rc = compare_alloc(&c->pos, p.posBytes, "the reference positions"))) return rc;
    if ((rc = compare_alloc(&c->keys, p.keyBytes, "the residue keys"))) return rc;
    if ((rc = compare_alloc(&c->ref_letters, (uint64_t)p.wr * 4u, "the reference's column counts"))) return rc;
    if ((rc = compare_alloc(&c->row_letters, (uint64_t)p.n * 4u, "the rows' letter counts"))) return rc;
    if ((rc = compare_alloc(&c->bad, 16, "the bad-row word"))) return rc;
    if ((rc = compare_alloc(&c->shared, (uint64_t)p.we * 8u, "the column results"))) return rc;
    if ((rc = compare_alloc(&c->letters, (uint64_t)p.we * 4u, "the column results"))) return rc;
    if ((rc = compare_alloc(&c->distinct, (uint64_t)p.we * 4u, "the column results"))) return rc;
    if ((rc = compare_alloc(&c->recovered, (uint64_t)p.we, "the column results"))) return rc;
    HIP_TRY(hipEventCreate(&c->ev[0]));
    HIP_TRY(hipEventCreate(&c->ev[1]));
    const double t0 = guide_now_ms();
    if ((rc = compare_upload_rows(st, c->est, n, w_est, p.pe, est_rows))) return rc;
    if ((rc = compare_upload_rows(st, c->ref, n, w_ref, p.pr, ref_rows))) return rc;
    c->upload_ms = guide_now_ms() - t0;
    int32_t bad = INT32_MAX;
    if ((rc = compare_build_keys(*c, st, &bad))) return rc;
    if (bad != INT32_MAX) {
        *bad_row = bad >> 1;
        g_err = std::string("row ") + std::to_string(bad >> 1) + ((bad & 1) ? ": the letters differ between the estimate and the reference (after folding a-z to A-Z)"
                                                                             : ": the letter count differs between the estimate and the reference");
        return TWL_ERR_BAD_ARGUMENT;
    }
    for (void **q : {&c->est, &c->ref, &c->pos}) { (void)hipFree(*q); *q = nullptr; }
    d->live_stores += 1;      // (a compare object holds the device as a store does: twl_shutdown waits for it)
    *cmp = c.release();
    return TWL_OK;
}

int twl_compare_columns(twl_compare *c, uint64_t *shared_out, uint32_t *letters_out, uint32_t *distinct_out, uint8_t *recovered_out, uint32_t *ref_letters_out)
{
    if (!c) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    DEVICE_CALL(call, c->d);
    hipStream_t st = call.st;
    HIP_TRY(hipEventRecord(c->ev[0], st));
    if (c->p.colTiles > 0) {
        hipLaunchKernelGGL(twl::compare_columns_kernel, dim3((unsigned)c->p.colTiles), dim3(twl::kCmpThreads), 0, st, compare_args(*c));
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(c->ev[1], st));
    HIP_TRY(hipStreamSynchronize(st));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    c->columns_ms = ms;
    const double t0 = guide_now_ms();
    const size_t we = (size_t)c->p.we, wr = (size_t)c->p.wr;
    if (shared_out && we) HIP_TRY(hipMemcpyAsync(shared_out, c->shared, we * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (letters_out && we) HIP_TRY(hipMemcpyAsync(letters_out, c->letters, we * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (distinct_out && we) HIP_TRY(hipMemcpyAsync(distinct_out, c->distinct, we * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (recovered_out && we) HIP_TRY(hipMemcpyAsync(recovered_out, c->recovered, we, hipMemcpyDeviceToHost, st));
    if (ref_letters_out && wr) HIP_TRY(hipMemcpyAsync(ref_letters_out, c->ref_letters, wr * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    c->download_ms = guide_now_ms() - t0;
    return TWL_OK;
}

int twl_compare_timing(twl_compare *c, double *upload_ms, double *keys_ms, double *columns_ms, double *download_ms)
{
    if (!c) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    if (upload_ms) *upload_ms = c->upload_ms;
    if (keys_ms) *keys_ms = c->keys_ms;
    if (columns_ms) *columns_ms = c->columns_ms;
    if (download_ms) *download_ms = c->download_ms;
    return TWL_OK;
}

int twl_compare_destroy(twl_compare *c)
{
    if (!c) return TWL_OK;
    {
        DeviceCall call(c->d);      // (the memory is freed either way)
        c->d->live_stores -= 1;
        delete c;
    }
    return TWL_OK;
}

}  // extern "C"
