// twilight_amd/csrc/twl_subtree.inc.hip -- host side of include/twl_subtree.h: the weighted profile of a finished subtree.
// Included at the end of twl_align.hip, behind twl_store.inc.hip: it works on that file's stores and cached profiles.
// What the call rejects is decided in twl_subtree_plan.inc.hip (pure); this file allocates, uploads, launches.

#include "twl_subtree_plan.inc.hip"

extern "C" {

int twl_store_weighted_columns(twl_store *s, int32_t n_ids, const int32_t *ids, const float *weights, int32_t cache_id)
{
    if (!s) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    int32_t L = -1;
    if (const char *why = check_weighted_columns(n_ids, ids, weights, cache_id, cache_id >= 0 && s->cache.count(cache_id), s->n_seqs, s->len.data(), &L)) {
        g_err = why;
        return TWL_ERR_BAD_ARGUMENT;
    }
    DEVICE_CALL(call, s->d);
    hipStream_t st = call.st;
    CacheEntry e;
    int rc = e.take(call.d, L, (size_t)L * (size_t)s->P * sizeof(float));
    if (rc) return rc;
    if ((rc = wait_rows(s, st))) return rc;
    // the planes of all sequences, the ids and the weights in one upload (the store's row arena: the call synchronises before it returns)
    Arena &A = s->up_rows;
    Ref d_plane, d_ids, d_w;
    if ((rc = A.begin(s->plane.size() + (size_t)n_ids * (sizeof(int32_t) + sizeof(float)), 3))) return rc;
    A.put(d_plane, s->plane);
    A.put(d_ids, ids, (size_t)n_ids);
    A.put(d_w, weights, (size_t)n_ids);
    if ((rc = A.flush(st))) return rc;
    const dim3 grid((unsigned)((L + twl::kWcThreads - 1) / twl::kWcThreads));
    if (s->P == 6)
        hipLaunchKernelGGL(twl::weighted_columns_kernel<6>, grid, dim3(twl::kWcThreads), 0, st, (const char *)s->rows[0].p, (const char *)s->rows[1].p, s->cap,
                           d_plane.as<const uint8_t>(), d_ids.as<const int32_t>(), d_w.as<const float>(), n_ids, L, (const uint8_t *)s->lut.p, (float *)e.buf.p);
    else
        hipLaunchKernelGGL(twl::weighted_columns_kernel<22>, grid, dim3(twl::kWcThreads), 0, st, (const char *)s->rows[0].p, (const char *)s->rows[1].p, s->cap,
                           d_plane.as<const uint8_t>(), d_ids.as<const int32_t>(), d_w.as<const float>(), n_ids, L, (const uint8_t *)s->lut.p, (float *)e.buf.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    s->cache[cache_id] = std::move(e);
    return TWL_OK;
}

}  // extern "C"
