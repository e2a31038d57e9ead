// twilight_amd/csrc/twl_store.inc.hip -- the device-resident store of include/twl_level.h: the table upload (Arena), the device's pools of level
// buffers and cache buffers, the store itself, its rows (one mover for every transfer of rows) and its cached profiles.
// Included at the end of twl_align.hip, in front of twl_level.inc.hip: it shares that file's Device bookkeeping.
//
// HBM layout of a store (one device):
//   rows[2]    two planes of [n_seqs][cap] bytes; plane[i] says which one holds sequence i's current row.  A commit writes the row of every
//              touched sequence into its other plane and flips the flag (SequenceInfo::changeStorage, sequencedb.cpp:51-55).
//   caches     one float[len][P] buffer per cached node profile (Node::msaFreq), addressed by the caller's ids.
//   level      raw[2n][stride][P] -> cols[2n][stride][P+2] (what the DP kernel reads), colinfo[2n][stride], lens, paths.
#include <cstdlib>
#include "twl_path_source.inc.hip"

namespace {

// One call's hold on a device: the device's lock for the whole call, the device made current.  rc != 0: it could not be (g_err says why).
// (dev->stream is read before the lock is taken: it is fixed from twl_init to twl_shutdown.)  DEVICE_CALL is two statements, a declaration
// and a test: use it as a statement of its own inside braces, never as the body of an unbraced if / else.
struct DeviceCall {
    Device *d;
    hipStream_t st;
    std::lock_guard<std::mutex> lk;
    int rc;
    explicit DeviceCall(Device *dev) : d(dev), st(dev->stream), lk(dev->mu), rc(make_current()) {}
    int make_current() { HIP_TRY(hipSetDevice(d->id)); return TWL_OK; }
};
#define DEVICE_CALL(name, dev) DeviceCall name(dev); if (name.rc) return name.rc

}  // namespace

// The small tables a call hands to its kernels (side descriptors, member lists, work lists ...) travel as ONE copy: they are laid out
// back to back in a pinned host block and land in a device block of the same layout.  One arena per kind of call (prepare / align /
// restore / commit, the path rows of a level, the rows of a store, a placement): a call rewrites its host block only after an earlier
// synchronisation of the same store has seen the previous copy out of it complete, and the device block is rewritten in stream order
// behind the kernels that read the old content.  (A call that fails between its flush and its synchronisation returns with the copy
// possibly still in flight: after a HIP error the rule is not kept.)
struct Ref {                            // a table inside an arena
    void *p = nullptr;
    template <class T> T *as() const { return static_cast<T *>(p); }
};
struct PinBuf {                         // pinned host memory a device-to-host copy lands in (no staging through pageable memory)
    void *p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes)
    {
        if (bytes <= cap) return TWL_OK;
        if (p) (void)hipHostFree(p);
        p = nullptr; cap = 0;
        HIP_TRY(hipHostMalloc(&p, bytes + bytes / 2 + 256, hipHostMallocDefault));
        cap = bytes + bytes / 2 + 256;
        return TWL_OK;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
};
struct Arena {
    char *h = nullptr;
    size_t hcap = 0, used = 0;
    Buf d;
    int begin(size_t bytes, size_t tables)      // room for `bytes` of payload in `tables` tables
    {
        const size_t want = bytes + 256 * (tables + 1);
        if (want > hcap) {
            if (h) (void)hipHostFree(h);
            h = nullptr; hcap = 0;
            const size_t cap = want + want / 2;
            HIP_TRY(hipHostMalloc((void **)&h, cap, hipHostMallocDefault));
            hcap = cap;
        }
        used = 0;
        return d.ensure(hcap);
    }
    template <class T>
    void put(Ref &r, const T *src, size_t n)
    {
        used = (used + 255) & ~(size_t)255;
        if (n) memcpy(h + used, src, n * sizeof(T));
        r.p = (char *)d.p + used;
        used += std::max<size_t>(n * sizeof(T), 16);
    }
    template <class T> void put(Ref &r, const std::vector<T> &v) { put(r, v.data(), v.size()); }
    int flush(hipStream_t st)
    {
        if (used) HIP_TRY(hipMemcpyAsync(d.p, h, used, hipMemcpyHostToDevice, st));
        return TWL_OK;
    }
    void release() { if (h) (void)hipHostFree(h); h = nullptr; hcap = 0; d.release(); }
};

// The device buffers of one prepared level (raw and packed columns are GBs at the leaf level).  They belong to the DEVICE, not to the
// store: a store takes a set at twl_level_prepare and gives it back at twl_level_commit, so the runs of a process that align one after
// the other work in the same, already mapped memory (device memory a process has not touched before costs tens of ms per GB:
// tools/micro/alloc_cost.hip), and a run holds only its rows while it waits.  Stores that are between prepare and commit at the same
// time (device replicas of a test) get a set each.
struct LevelBufs {
    Arena up_prepare, up_align, up_restore, up_commit;
    Arena up_paths;                                          // path rows to and from a block: every launch over it is followed by a synchronisation (level_rows_block)
    PinBuf back;                                             // lengths coming back from prepare / restore
    Ref d_sides, d_mseq, d_mw, d_mplane, d_tab, d_num;       // up_prepare (d_mplane, d_tab: up_commit after the commit's upload)
    Ref d_lenmask;                                           // up_align
    Ref r_sel;                                               // up_restore
    Ref d_pathlen, d_work, d_merge, d_mergew, d_fromdp;      // up_commit
    Buf d_raw, d_colinfo, d_cols, d_len, d_aln, d_alnlen, d_err;
    Buf d_paths, d_chunk, d_ccnt;
    Buf r_oidx, r_run, r_seg, r_aoff, r_blist, r_nboth, r_wtot, r_arena, r_outlen, r_tb, r_rows;      // twl_level_restore (restore_kernels.hip.h)
    Buf x_send, x_recv;                                      // exchange of final paths between processes (device blocks)
    bool busy = false;
    hipEvent_t ev_scan = nullptr, ev_apply = nullptr;        // a small level's row rewrite runs on the device's second stream: path_scan done / rewrite done
    bool apply_pending = false;                              // ... and may still read this set's tables
    void release_all()
    {
        if (ev_scan) (void)hipEventDestroy(ev_scan);
        if (ev_apply) (void)hipEventDestroy(ev_apply);
        ev_scan = ev_apply = nullptr; apply_pending = false;
        for (Buf *b : {&d_raw, &d_colinfo, &d_cols, &d_len, &d_aln, &d_alnlen, &d_err,
                       &d_paths, &d_chunk, &d_ccnt, &r_oidx, &r_run, &r_seg, &r_aoff, &r_blist, &r_nboth, &r_wtot, &r_arena, &r_outlen, &r_tb, &r_rows, &x_send, &x_recv})
            b->release();
        for (Arena *a : {&up_prepare, &up_align, &up_restore, &up_commit, &up_paths}) a->release();
        back.release();
    }
};

namespace {
std::vector<std::unique_ptr<LevelBufs>> &level_pool(Device *d)
{
    static std::mutex mu;
    static std::unordered_map<Device *, std::vector<std::unique_ptr<LevelBufs>>> pools;
    std::lock_guard<std::mutex> lk(mu);
    return pools[d];
}
// (callers hold d->mu)
LevelBufs *acquire_level(Device *d)
{
    auto &pool = level_pool(d);
    LevelBufs *waiting = nullptr;        // free, but the row rewrite of its last level may still read its tables
    for (const auto &own : pool) {
        LevelBufs *b = own.get();
        if (b->busy) continue;
        if (b->apply_pending && hipEventQuery(b->ev_apply) != hipSuccess) { (void)hipGetLastError(); if (!waiting) waiting = b; continue; }
        b->apply_pending = false;
        b->busy = true;
        return b;
    }
    if (waiting && pool.size() >= 3) {   // (two sets alternate at the top of a tree; never more than three)
        (void)hipStreamWaitEvent(d->stream, waiting->ev_apply, 0);
        waiting->apply_pending = false;
        waiting->busy = true;
        return waiting;
    }
    pool.push_back(std::make_unique<LevelBufs>());
    pool.back()->busy = true;
    return pool.back().get();
}
void release_level(LevelBufs *&lv) { if (lv) { lv->busy = false; lv = nullptr; } }

// Cached node profiles come and go with every level near the top of a tree (a merged profile replaces its two parts): their buffers are
// recycled through the device instead of hipMalloc / hipFree (which waits for the device) in the middle of a level.  Everything that
// touches them runs on the device's one stream, so a buffer may be handed out again while the kernel that last read it is still queued.
std::vector<Buf> &cache_pool(Device *d)
{
    static std::mutex mu;
    static std::unordered_map<Device *, std::vector<Buf>> pools;
    std::lock_guard<std::mutex> lk(mu);
    return pools[d];
}
// (callers hold d->mu)
int cache_buf_get(Device *d, Buf &b, size_t bytes)
{
    auto &pool = cache_pool(d);
    size_t best = pool.size();
    for (size_t k = 0; k < pool.size(); ++k)
        if (pool[k].cap >= bytes && (best == pool.size() || pool[k].cap < pool[best].cap)) best = k;
    if (best != pool.size()) { b = pool[best]; pool[best] = pool.back(); pool.pop_back(); return TWL_OK; }
    b = Buf{};
    return b.ensure(bytes + bytes / 4);      // (the next profile up the tree is a little longer)
}
void cache_buf_put(Device *d, Buf &b)
{
    if (!b.p) return;
    auto &pool = cache_pool(d);
    if (pool.size() >= 4096) {               // keep the larger ones (hipFree waits for the device -- for the row rewrite that is still running: a 64-entry pool
                                             // made every top-level commit of a 100 000-leaf tree wait 1-2.6 ms here)
        size_t small = 0;
        for (size_t k = 1; k < pool.size(); ++k) if (pool[k].cap < pool[small].cap) small = k;
        if (pool[small].cap < b.cap) std::swap(pool[small], b);
        b.release();
        return;
    }
    pool.push_back(b);
    b = Buf{};
}

// A cached profile and its buffer out of the device's pool.  The buffer goes back to the pool with its owner, wherever that dies: in the
// store's table, or in a call that failed before it could install it.  (Whoever creates, moves or destroys one holds d->mu.)
struct CacheEntry {
    Device *d = nullptr;
    Buf buf;
    int32_t len = 0;
    CacheEntry() = default;
    CacheEntry(CacheEntry &&o) noexcept : d(o.d), buf(o.buf), len(o.len) { o.buf = Buf{}; }
    CacheEntry &operator=(CacheEntry &&o) noexcept
    {
        if (this != &o) { cache_buf_put(d, buf); d = o.d; buf = o.buf; len = o.len; o.buf = Buf{}; }
        return *this;
    }
    ~CacheEntry() { cache_buf_put(d, buf); }
    int take(Device *dev, int32_t n, size_t bytes) { d = dev; len = n; return cache_buf_get(dev, buf, bytes); }
};
}  // namespace

static void twl_level_pool_release(Device *d)
{
    auto &pool = level_pool(d);
    for (const auto &b : pool) b->release_all();
    pool.clear();
    for (Buf &b : cache_pool(d)) b.release();
    cache_pool(d).clear();
}

struct twl_store {
    Device *d = nullptr;
    int P = 6;
    char type = 'n';
    int32_t n_seqs = 0;
    int64_t cap = 0;
    Buf rows[2];
    std::vector<uint8_t> plane;
    std::vector<int32_t> len;
    std::unordered_map<int32_t, CacheEntry> cache;
    Buf lut;
    // state of the level between prepare / align / commit
    int32_t n_pairs = 0, seq_len = 0;
    bool prepared = false;
    std::vector<twl_side> sides;
    std::vector<int32_t> members;
    std::vector<int32_t> h_len, h_num;
    CommitPlan commit;                       // scratch of the commit (kept for its capacity)
    std::vector<float *> h_tab;
    bool commit_pending = false;             // the last commit's kernels may still run (its events are d->ev[6], d->ev[7])
    bool commit_side = false;                // ... its row rewrite on the second stream (timed by d->ev2)
    hipEvent_t rows_event = nullptr;         // != nullptr: a row rewrite on the second stream may still run; whoever reads or rewrites rows on the first stream waits for it
    LevelBufs *lv = nullptr;     // the level's device buffers, held from prepare to commit (from the device's pool, see LevelBufs)
    int32_t staged_stride = 0;   // > 0: twl_level_restore put this level's DP paths (and the restored ones) into lv->d_paths at this row pitch
    Arena up_rows;               // tables of a row transfer (move_rows, twl_store_count_columns): each of those calls synchronises the stream before it returns
    Buf d_gather;                // rows packed back to back, on their way to or from the host
    Buf x_send, x_recv;          // device blocks of the subtree exchange of a sharded run (twl_store_exchange_buffers)
    double prepare_ms = 0, commit_ms = 0;
    double squeeze_ms = 0;       // HIP-event time of the kernels of the last twl_store_squeeze_groups (twl_backbone.inc.hip)
    Buf trim_gaps, trim_cols;    // of the last twl_store_trim_columns (twl_trim.inc.hip): gaps of its trim_W columns, the trim_kept columns it kept
    int32_t trim_W = -1, trim_kept = 0;      // trim_W < 0: no trim has run
    double trim_ms = 0;          // HIP-event time of its kernels
    double score_ms[3] = {0, 0, 0};      // of the last twl_store_score_rows (twl_score.inc.hip): pack, column and pair kernels, HIP-event times
};

namespace {

// letterIdx(type, toupper(c)) -- reference src/scoring-matrix.cpp:26-79
void build_lut(char type, uint8_t *lut)
{
    for (int c = 0; c < 256; ++c) {
        const int u = (c >= 'a' && c <= 'z') ? c - 32 : c;
        int v;
        if (type == 'n') {
            switch (u) {
            case 'A': v = 0; break;
            case 'C': v = 1; break;
            case 'G': v = 2; break;
            case 'T': case 'U': v = 3; break;
            case '-': case '.': v = 5; break;
            default: v = 4; break;
            }
        } else {
            static const char acids[] = "ACDEFGHIKLMNPQRSTVWY";
            v = 20;
            for (int k = 0; k < 20; ++k) if (u == acids[k]) v = k;
            if (u == '-' || u == '.') v = 21;
        }
        lut[c] = (uint8_t)v;
    }
}

// Room for the rows.  The final alignment is several times longer than the sequences (6.6x at 10 000 x 10 kbp, 22x on the synthetic
// 100 000 x 1.6 kbp family), and re-pitching costs more than its copy: device memory the process has not touched before comes at tens of
// ms per GB (tools/micro/alloc_cost.hip: a first 16 GB allocation 1.3 s, recycled ones < 1 ms), which a pass must not pay in its middle.
// So the planes start at 8x-48x the longest sequence (more for more sequences, see twl_store_create) and grow by half when they have to -- within a budget of a sixth of the device memory
// for both planes (288 GB of HBM are there to be used), never below what is needed.
int64_t rows_budget_cap(twl_store *s)
{
    size_t freeB = 0, totalB = 0;
    if (hipMemGetInfo(&freeB, &totalB) != hipSuccess) { (void)hipGetLastError(); return INT64_MAX; }
    const int64_t budget = (int64_t)(totalB / 6);
    return std::max<int64_t>(256, budget / (2 * std::max<int64_t>(1, s->n_seqs)));
}

int g_fail_next_row_allocs = 0;      // twl_set_knob(TWL_KNOB_FAIL_ROW_ALLOCS, n): the next n allocations of grow_rows fail (test of its fallback)

int grow_rows(twl_store *s, int64_t need, int64_t want = 0)
{
    if (need <= s->cap) return TWL_OK;
    Device *d = s->d;
    HIP_TRY(hipStreamSynchronize(d->stream2));      // (a row rewrite of the previous level may still run there)
    s->rows_event = nullptr;
    const int64_t minCap = (need + 255) & ~(int64_t)255;
    int64_t ncap = std::max(need, std::min(std::max(want, need + need / 2), rows_budget_cap(s)));
    ncap = (ncap + 255) & ~(int64_t)255;
    // Both planes must end up with ONE pitch: both buffers are allocated before either plane is touched; if either allocation
    // fails at the generous pitch, both are given back and both are retried at the pitch that is needed.
    Buf nb[2];
    auto alloc_both = [&](int64_t cap) {
        for (int pl = 0; pl < 2; ++pl) {
            int rc = TWL_ERR_HIP;
            if (g_fail_next_row_allocs > 0) { --g_fail_next_row_allocs; g_err = "row allocation failed (test knob)"; }
            else rc = nb[pl].ensure((size_t)s->n_seqs * (size_t)cap);
            if (rc) { nb[0].release(); nb[1].release(); (void)hipGetLastError(); return rc; }      // (the failed hipMalloc's error is not left behind)
        }
        return (int)TWL_OK;
    };
    int rc = alloc_both(ncap);
    if (rc && ncap > minCap) { ncap = minCap; rc = alloc_both(ncap); }
    if (rc) return rc;
    for (int pl = 0; pl < 2; ++pl)
        if (s->rows[pl].p)
            HIP_TRY(hipMemcpy2DAsync(nb[pl].p, (size_t)ncap, s->rows[pl].p, (size_t)s->cap, (size_t)s->cap, (size_t)s->n_seqs, hipMemcpyDeviceToDevice, d->stream));
    HIP_TRY(hipStreamSynchronize(d->stream));
    for (int pl = 0; pl < 2; ++pl) { s->rows[pl].release(); s->rows[pl] = nb[pl]; }
    s->cap = ncap;
    return TWL_OK;
}

// The end of a store, whoever ends it: twl_store_destroy, or a twl_store_create that could not finish.  (callers hold s->d->mu)
struct StoreEnd {
    void operator()(twl_store *raw) const
    {
        std::unique_ptr<twl_store> s(raw);
        (void)hipSetDevice(s->d->id);
        (void)hipStreamSynchronize(s->d->stream);        // (a commit does not wait for its kernels)
        (void)hipStreamSynchronize(s->d->stream2);
        s->cache.clear();                                // (the profiles' buffers go back to the device's pool)
        release_level(s->lv);
        for (Buf *b : {&s->rows[0], &s->rows[1], &s->lut, &s->d_gather, &s->x_send, &s->x_recv, &s->trim_gaps, &s->trim_cols}) b->release();
        s->up_rows.release();
        s->d->live_stores -= 1;
    }
};

// a row rewrite on the second stream may still run: whoever reads or rewrites rows on the first stream waits for it
int wait_rows(twl_store *s, hipStream_t st)
{
    if (s->rows_event) { HIP_TRY(hipStreamWaitEvent(st, s->rows_event, 0)); s->rows_event = nullptr; }
    return TWL_OK;
}

// The two ends of a kernel that rewrites whole rows into their other plane (the finish of a placement, of a merge): both planes as the
// kernel's arguments name them, and behind the kernel the flag and the length of every rewritten row.
template <class Args>
void fill_row_planes(const twl_store *s, Args &a)
{
    a.rows0 = (const char *)s->rows[0].p; a.rows1 = (const char *)s->rows[1].p;
    a.out0 = (char *)s->rows[0].p; a.out1 = (char *)s->rows[1].p;
    a.cap = s->cap;
}
void rows_rewritten(twl_store *s, const std::vector<int32_t> &ids, int32_t W) { for (int32_t id : ids) { s->plane[id] ^= 1; s->len[id] = W; } }

// ---- the store's level as the source of the final paths a call takes (twl_place_collect, twl_merge_apply; twl_path_source.inc.hip) ----
PathLevelView path_level_view(const twl_store *s)
{
    const bool prepared = s->prepared && s->lv;
    return PathLevelView{prepared, s->n_pairs, 2 * (int64_t)s->seq_len, prepared && s->lv->d_aln.p, s->staged_stride};
}
// the host rows of a call, packed at the call's pitch into `buf` in upload order
int upload_host_paths(Buf &buf, const int8_t *paths, const int32_t *path_len, int32_t path_stride, const std::vector<int32_t> &hostRows, hipStream_t st)
{
    const size_t pitch = (size_t)path_stride;
    if (!hostRows.empty()) { const int rc = buf.ensure(hostRows.size() * pitch); if (rc) return rc; }
    for (size_t k = 0; k < hostRows.size(); ++k)
        HIP_TRY(hipMemcpyAsync((int8_t *)buf.p + k * pitch, paths + (size_t)hostRows[k] * pitch, (size_t)path_len[hostRows[k]], hipMemcpyHostToDevice, st));
    return TWL_OK;
}
// what the taking kernel reads: the three sources and the uploaded tables of the taking pairs
twl::PathSrc path_src(const twl_store *s, const uint8_t *from_dp, const Buf &hostRows, const Ref &which, const Ref &srcOff, const Ref &plen)
{
    return twl::PathSrc{{(const int8_t *)hostRows.p, from_dp ? (const int8_t *)s->lv->d_aln.p : nullptr, from_dp ? (const int8_t *)s->lv->d_paths.p : nullptr},
                        which.as<const uint8_t>(), srcOff.as<const int64_t>(), plen.as<const int32_t>()};
}

// ---- the one mover of rows: between the planes and a packed block of rows (row t at off[t]) on the host or on the device ----
struct RowTables { std::vector<int64_t> off; int64_t total = 0; int32_t maxLen = 1; };
RowTables row_offsets(int32_t n, const int32_t *lens)
{
    RowTables t;
    t.off.resize((size_t)n);
    for (int32_t k = 0; k < n; ++k) { t.off[k] = t.total; t.total += lens[k]; t.maxLen = std::max(t.maxLen, lens[k]); }
    return t;
}

// the table step of a row transfer: the planes of all sequences and, as far as given, ids / lengths / offsets of the rows, in one upload
struct RowRefs { Ref plane, ids, len, off; };
int upload_row_tables(twl_store *s, hipStream_t st, int32_t n, const int32_t *ids, const int32_t *lens, const int64_t *off, RowRefs &r)
{
    Arena &A = s->up_rows;
    int rc = A.begin(s->plane.size() + (size_t)n * ((ids ? sizeof(int32_t) : 0) + (lens ? sizeof(int32_t) : 0) + (off ? sizeof(int64_t) : 0)), 4);
    if (rc) return rc;
    A.put(r.plane, s->plane);
    if (ids) A.put(r.ids, ids, (size_t)n);
    if (lens) A.put(r.len, lens, (size_t)n);
    if (off) A.put(r.off, off, (size_t)n);
    return A.flush(st);
}

struct RowMove {
    bool write = false;             // the rows arrive (scatter into the sequences' current planes) instead of leaving (gather)
    int32_t n = 0;
    const int32_t *ids = nullptr;   // nullptr: every sequence of the store in order (gather_rows_kernel, the read-back at the end of a run)
    const int32_t *lens = nullptr;  // [n] lengths of the rows: the current ones of a read, the arriving ones of a write
    char *host = nullptr;           // the packed rows on the host (they pass through d_gather; only read by a write) ...
    void *block = nullptr;          // ... or in a device block of the caller's
};

int move_rows(twl_store *s, hipStream_t st, const RowMove &m, const RowTables &t)
{
    int rc;
    if ((rc = wait_rows(s, st))) return rc;
    if (m.write && (rc = grow_rows(s, (int64_t)t.maxLen + 1))) return rc;
    char *packed = (char *)m.block;
    if (!packed) {
        if ((rc = s->d_gather.ensure((size_t)std::max<int64_t>(t.total, 16)))) return rc;
        packed = (char *)s->d_gather.p;
    }
    RowRefs r;
    if ((rc = upload_row_tables(s, st, m.n, m.ids, m.lens, t.off.data(), r))) return rc;
    if (m.write && m.host && t.total) HIP_TRY(hipMemcpyAsync(packed, m.host, (size_t)t.total, hipMemcpyHostToDevice, st));
    const dim3 grid((unsigned)m.n, (unsigned)((t.maxLen + 255) / 256));
    if (m.write)
        hipLaunchKernelGGL(twl::scatter_rows_of_kernel, grid, dim3(256), 0, st, (char *)s->rows[0].p, (char *)s->rows[1].p, s->cap, r.plane.as<const uint8_t>(),
                           r.ids.as<const int32_t>(), r.len.as<const int32_t>(), r.off.as<const int64_t>(), (const char *)packed);
    else if (m.ids)
        hipLaunchKernelGGL(twl::gather_rows_of_kernel, grid, dim3(256), 0, st, (const char *)s->rows[0].p, (const char *)s->rows[1].p, s->cap, r.plane.as<const uint8_t>(),
                           r.ids.as<const int32_t>(), r.len.as<const int32_t>(), r.off.as<const int64_t>(), packed);
    else
        hipLaunchKernelGGL(twl::gather_rows_kernel, grid, dim3(256), 0, st, (const char *)s->rows[0].p, (const char *)s->rows[1].p, s->cap, r.plane.as<const uint8_t>(),
                           r.len.as<const int32_t>(), r.off.as<const int64_t>(), packed);
    HIP_TRY(hipGetLastError());
    if (!m.write && m.host && t.total) HIP_TRY(hipMemcpyAsync(m.host, packed, (size_t)t.total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (m.write) for (int32_t k = 0; k < m.n; ++k) s->len[m.ids[k]] = m.lens[k];
    return TWL_OK;
}

// host memory that is written before it is read (uninitialised on purpose: hundreds of MB at the end of a large run)
using HostBytes = std::unique_ptr<char, decltype(&std::free)>;
HostBytes host_bytes(size_t n) { return HostBytes((char *)std::malloc(std::max<size_t>(n, 1)), &std::free); }

// ids[t] names a sequence of the store (and lens[t], if given, is a length)
bool rows_in_range(const twl_store *s, int32_t n_ids, const int32_t *ids, const int32_t *lens)
{
    for (int32_t t = 0; t < n_ids; ++t) if (ids[t] < 0 || ids[t] >= s->n_seqs || (lens && lens[t] < 0)) return false;
    return true;
}

}  // namespace

extern "C" {

int twl_store_create(int device, char type, int32_t n_seqs, const char *const *seqs, const int32_t *lens, twl_store **out)
{
    if (!g_init) { g_err = "twl_init not called"; return TWL_ERR_NOT_INITIALIZED; }
    if (!out || n_seqs < 0 || (n_seqs > 0 && (!seqs || !lens)) || (type != 'n' && type != 'p')) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    Device *d = nullptr;
    int rc = find_dev(device, &d);
    if (rc) return rc;
    DEVICE_CALL(call, d);
    std::unique_ptr<twl_store, StoreEnd> s(std::make_unique<twl_store>().release());      // (every return below but the last ends the store again)
    d->live_stores += 1;
    s->d = d;
    s->type = type;
    s->P = (type == 'n') ? 6 : 22;
    s->n_seqs = n_seqs;
    s->plane.assign((size_t)n_seqs, 0);
    s->len.assign(lens, lens + n_seqs);
    int64_t maxLen = 1;
    for (int32_t i = 0; i < n_seqs; ++i) {
        if (lens[i] < 0) { g_err = "negative sequence length"; return TWL_ERR_BAD_ARGUMENT; }
        maxLen = std::max<int64_t>(maxLen, lens[i]);
    }
    // room for the alignment to grow (see grow_rows); the sequences go up through a tight host image with its own pitch
    // (how much longer than its sequences an alignment gets grows with the number of sequences: 6.6x at 10 000, 22x at 100 000 on the
    // synthetic families; 8 x log10(n) - 16, between 8x and 48x, within grow_rows' budget)
    const double lg = std::log10((double)std::max<int32_t>(n_seqs, 10));
    const int64_t factor = (int64_t)std::min(48.0, std::max(8.0, 8.0 * lg - 16.0));
    if ((rc = grow_rows(s.get(), maxLen + 1, factor * maxLen + 256))) return rc;
    if (n_seqs > 0) {
        const size_t hp = (size_t)maxLen;
        const HostBytes img = host_bytes((size_t)n_seqs * hp);
        if (!img) { g_err = "out of host memory"; return TWL_ERR_HIP; }
        for (int32_t i = 0; i < n_seqs; ++i) { memcpy(img.get() + (size_t)i * hp, seqs[i], (size_t)lens[i]); memset(img.get() + (size_t)i * hp + (size_t)lens[i], '-', hp - (size_t)lens[i]); }
        HIP_TRY(hipMemcpy2D(s->rows[0].p, (size_t)s->cap, img.get(), hp, hp, (size_t)n_seqs, hipMemcpyHostToDevice));
    }
    uint8_t lut[256];
    build_lut(type, lut);
    if ((rc = s->lut.ensure(256))) return rc;
    HIP_TRY(hipMemcpy(s->lut.p, lut, 256, hipMemcpyHostToDevice));
    *out = s.release();
    return TWL_OK;
}

void twl_store_destroy(twl_store *s)
{
    if (!s) return;
    std::lock_guard<std::mutex> lk(s->d->mu);      // (the level-buffer pool and the store count belong to the device)
    StoreEnd()(s);
}

int twl_store_read_rows(twl_store *s, char *const *rows_out, int32_t *lens_out)
{
    if (!s || !lens_out) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    for (int32_t i = 0; i < s->n_seqs; ++i) lens_out[i] = s->len[i];
    if (!rows_out || s->n_seqs == 0) return TWL_OK;
    DEVICE_CALL(call, s->d);
    const RowTables t = row_offsets(s->n_seqs, s->len.data());
    RowMove m;
    m.n = s->n_seqs; m.lens = s->len.data();
    // rows laid out back to back by the caller (row i at the prefix sum of the lengths): one transfer, straight into them
    bool packed = true;
    for (int32_t i = 0; i < s->n_seqs && packed; ++i) packed = (s->len[i] == 0) || (rows_out[i] == rows_out[0] + (t.off[i] - t.off[0]) && rows_out[0] != nullptr);
    if (packed && s->len[0] > 0) { m.host = rows_out[0]; return move_rows(s, call.st, m, t); }
    const HostBytes host = host_bytes((size_t)t.total);
    if (!host) { g_err = "out of host memory"; return TWL_ERR_HIP; }
    m.host = host.get();
    const int rc = move_rows(s, call.st, m, t);
    if (rc) return rc;
    // scatter into the caller's rows on a few threads (hundreds of MB at the end of a large run)
    const int nt = (int)std::min<size_t>(8, std::max<size_t>(1, (size_t)t.total >> 24));
    std::vector<std::thread> th;
    for (int k = 0; k < nt; ++k)
        th.emplace_back([&, k] {
            for (int32_t i = k; i < s->n_seqs; i += nt)
                if (rows_out[i] && s->len[i] > 0) memcpy(rows_out[i], host.get() + t.off[i], (size_t)s->len[i]);
        });
    for (auto &x : th) x.join();
    return TWL_OK;
}

// rows of a list of sequences: out = their current rows back to back (row t at the prefix sum of lens_out), lens_out[t] their lengths; out NULL: lengths only
int twl_store_read_rows_of(twl_store *s, int32_t n_ids, const int32_t *ids, char *out, int32_t *lens_out)
{
    if (!s || n_ids < 0 || (n_ids > 0 && (!ids || !lens_out))) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    if (!rows_in_range(s, n_ids, ids, nullptr)) { g_err = "sequence id out of range"; return TWL_ERR_BAD_ARGUMENT; }
    for (int32_t t = 0; t < n_ids; ++t) lens_out[t] = s->len[ids[t]];
    const RowTables t = row_offsets(n_ids, lens_out);
    if (!out || n_ids == 0 || t.total == 0) return TWL_OK;
    DEVICE_CALL(call, s->d);
    RowMove m;
    m.n = n_ids; m.ids = ids; m.lens = lens_out; m.host = out;
    return move_rows(s, call.st, m, t);
}

// the inverse: rows (back to back in `in`, lengths lens) become the current rows of these sequences
int twl_store_write_rows(twl_store *s, int32_t n_ids, const int32_t *ids, const char *in, const int32_t *lens)
{
    if (!s || n_ids < 0 || (n_ids > 0 && (!ids || !lens || !in))) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    if (n_ids == 0) return TWL_OK;
    if (!rows_in_range(s, n_ids, ids, lens)) { g_err = "sequence id or length out of range"; return TWL_ERR_BAD_ARGUMENT; }
    DEVICE_CALL(call, s->d);
    RowMove m;
    m.write = true; m.n = n_ids; m.ids = ids; m.lens = lens; m.host = const_cast<char *>(in);
    return move_rows(s, call.st, m, row_offsets(n_ids, lens));
}

// The same two on DEVICE blocks (the rows of a sharded run's subtrees travel HBM to HBM): rows_to_block packs the current rows of `ids` back to back at
// dev_block (lens_out their lengths), rows_from_block makes the rows found there the current rows.  twl_store_exchange_buffers: two device buffers of the store.
int twl_store_rows_to_block(twl_store *s, int32_t n_ids, const int32_t *ids, void *dev_block, int32_t *lens_out)
{
    if (!s || n_ids < 0 || (n_ids > 0 && (!ids || !lens_out || !dev_block))) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    if (!rows_in_range(s, n_ids, ids, nullptr)) { g_err = "sequence id out of range"; return TWL_ERR_BAD_ARGUMENT; }
    for (int32_t t = 0; t < n_ids; ++t) lens_out[t] = s->len[ids[t]];
    if (n_ids == 0) return TWL_OK;
    DEVICE_CALL(call, s->d);
    RowMove m;
    m.n = n_ids; m.ids = ids; m.lens = lens_out; m.block = dev_block;
    return move_rows(s, call.st, m, row_offsets(n_ids, lens_out));
}
int twl_store_rows_from_block(twl_store *s, int32_t n_ids, const int32_t *ids, const int32_t *lens, const void *dev_block)
{
    if (!s || n_ids < 0 || (n_ids > 0 && (!ids || !lens || !dev_block))) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    if (!rows_in_range(s, n_ids, ids, lens)) { g_err = "sequence id or length out of range"; return TWL_ERR_BAD_ARGUMENT; }
    if (n_ids == 0) return TWL_OK;
    DEVICE_CALL(call, s->d);
    RowMove m;
    m.write = true; m.n = n_ids; m.ids = ids; m.lens = lens; m.block = const_cast<void *>(dev_block);
    return move_rows(s, call.st, m, row_offsets(n_ids, lens));
}
int twl_store_exchange_buffers(twl_store *s, int64_t send_bytes, int64_t recv_bytes, void **send_dev, void **recv_dev)
{
    if (!s || send_bytes < 0 || recv_bytes < 0 || !send_dev || !recv_dev) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    DEVICE_CALL(call, s->d);
    int rc;
    if ((rc = s->x_send.ensure((size_t)std::max<int64_t>(send_bytes, 16)))) return rc;
    if ((rc = s->x_recv.ensure((size_t)std::max<int64_t>(recv_bytes, 16)))) return rc;
    *send_dev = s->x_send.p; *recv_dev = s->x_recv.p;
    return TWL_OK;
}

// a cached profile arriving from another rank: float[len][P] under an id this store does not hold yet
int twl_store_write_cache(twl_store *s, int32_t id, const float *data, int32_t len)
{
    if (!s || !data || len < 0 || id < 0) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    if (s->cache.count(id)) { g_err = "cache id in use"; return TWL_ERR_BAD_ARGUMENT; }
    DEVICE_CALL(call, s->d);
    CacheEntry e;
    const size_t bytes = (size_t)len * s->P * sizeof(float);
    int rc = e.take(call.d, len, std::max<size_t>(bytes, 16));
    if (rc) return rc;
    if (bytes) HIP_TRY(hipMemcpyAsync(e.buf.p, data, bytes, hipMemcpyHostToDevice, call.st));
    HIP_TRY(hipStreamSynchronize(call.st));
    s->cache[id] = std::move(e);
    return TWL_OK;
}

int twl_store_read_cache(twl_store *s, int32_t id, float *out, int32_t *len_out)
{
    if (!s) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    auto it = s->cache.find(id);
    if (it == s->cache.end()) { g_err = "unknown cache id"; return TWL_ERR_BAD_ARGUMENT; }
    if (len_out) *len_out = it->second.len;
    if (!out) return TWL_OK;
    DEVICE_CALL(call, s->d);
    HIP_TRY(hipStreamSynchronize(call.st));     // (a commit does not wait for its kernels)
    HIP_TRY(hipMemcpy(out, it->second.buf.p, (size_t)it->second.len * s->P * sizeof(float), hipMemcpyDeviceToHost));
    return TWL_OK;
}

int twl_store_drop_cache(twl_store *s, int32_t id)
{
    if (!s) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    auto it = s->cache.find(id);
    if (it == s->cache.end()) return TWL_OK;
    std::lock_guard<std::mutex> lk(s->d->mu);
    (void)hipSetDevice(s->d->id);
    (void)hipStreamSynchronize(s->d->stream);
    s->cache.erase(it);
    return TWL_OK;
}

}  // extern "C"
