// twilight_amd/csrc/twl_align.hip -- host side of libtwl_align (C ABI in include/twl_align.h).
//
// Owns device buffers, streams and the launch policy.  There is no CPU fallback: without a HIP
// device every entry point fails with TWL_ERR_HIP / TWL_ERR_NOT_INITIALIZED.
#include "../../include/twl_align.h"
#include "../../include/twl_level.h"
#include "../../include/twl_place.h"
#include "../../include/twl_keep.h"
#include "../../include/twl_merge.h"
#include "../../include/twl_subtree.h"
#include "../../include/twl_guide.h"
#include "../../include/twl_strand.h"
#include "../../include/twl_retree.h"
#include "../../include/twl_retree_set.h"
#include "../../include/twl_backbone.h"
#include "../../include/twl_trim.h"
#include "../../include/twl_compare.h"
#include "../../include/twl_score.h"
#include "level_kernels.hip.h"
#include "restore_kernels.hip.h"
#include "place_kernels.hip.h"
#include "keep_kernels.hip.h"
#include "merge_kernels.hip.h"
#include "subtree_kernels.hip.h"
#include "guide_kernels.hip.h"
#include "retree_kernels.hip.h"
#include "retree_stage_kernels.hip.h"
#include "backbone_kernels.hip.h"
#include "trim_kernels.hip.h"
#include "compare_kernels.hip.h"
#include "score_kernels.hip.h"
#include "talco_kernel.hip.h"
#include "talco_nuc.hip.h"
#include "talco_global.hip.h"

#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <numeric>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

namespace twl {
// Several byte fills in one launch (a level's DP call zeroes its outputs, work counters and tile tables: seven hipMemsetAsync before).
struct FillJob { void *p; unsigned long long bytes; unsigned int val; };
struct FillArgs { FillJob j[8]; int n; };
__global__ void __launch_bounds__(256) fill_kernel(FillArgs a)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, nt = (size_t)gridDim.x * 256;
    for (int r = 0; r < a.n; ++r) {
        const size_t nw = a.j[r].bytes >> 4;
        uint4 *w = reinterpret_cast<uint4 *>(a.j[r].p);
        const unsigned v = a.j[r].val;
        for (size_t i = t; i < nw; i += nt) w[i] = make_uint4(v, v, v, v);
        const size_t tail = a.j[r].bytes & 15;
        if (t < tail) reinterpret_cast<unsigned char *>(a.j[r].p)[(nw << 4) + t] = (unsigned char)v;
    }
}
// The per-pair results of a DP call (and the tile-parallel counters) into one host-visible block: [4 counters][n cells][n lengths][n codes]
__global__ void __launch_bounds__(256) collect_kernel(int n, const int16_t *err, const int32_t *aln_len, const unsigned long long *cells,
                                                      const unsigned long long *mt_stat, unsigned long long *out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    unsigned long long *oc = out + 4;
    int32_t *ol = reinterpret_cast<int32_t *>(oc + n);
    int16_t *oe = reinterpret_cast<int16_t *>(ol + n);
    if (i < 4) out[i] = mt_stat ? mt_stat[i] : 0ull;
    if (i < n) { oc[i] = cells[i]; ol[i] = aln_len[i]; oe[i] = err[i]; }
    __threadfence_system();
}
}  // namespace twl

namespace {

thread_local std::string g_err;
std::mutex g_mu;

static bool dbg_on() { static const bool v = getenv("TWL_DEBUG") != nullptr; return v; }
#define TRACE(...) do { if (dbg_on()) { fprintf(stderr, "[twl trace] " __VA_ARGS__); fputc('\n', stderr); fflush(stderr); } } while (0)

#define HIP_TRY(expr)                                                                                          \
    do {                                                                                                       \
        hipError_t e_ = (expr);                                                                                \
        if (e_ != hipSuccess) {                                                                                \
            g_err = std::string(#expr) + ": " + hipGetErrorString(e_);                                         \
            return TWL_ERR_HIP;                                                                                \
        }                                                                                                      \
    } while (0)

// Fast path: 8 waves x 2 row blocks per lane     -> 1024-row window (bands up to 961 wide), ref ring in LDS, 2 workgroups/CU.
// Wide path: 8 waves x 9 blocks                   -> 4608-row window (covers flen = 4096), ref columns from L2/HBM.
// Protein (P = 22): 8 waves x 1 block (512-row window, 96-byte columns in the LDS ring); wide path re-reads both columns per cell.

#include "twl_policy.inc.hip"

struct Buf {
    void *p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes)
    {
        if (bytes <= cap) return TWL_OK;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        size_t want = bytes + bytes / 8 + 256;
        HIP_TRY(hipMalloc(&p, want));
        cap = want;
        return TWL_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

struct Device {
    int id = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;                                               // row rewrites of small levels (twl_level_commit), beside the next level's work on `stream`
    hipEvent_t ev2[2] = {};                                                      // ... timed
    hipStream_t tail_stream = nullptr;                                           // the tile-parallel remainder of a throughput level, beside its bulk launch on the call's stream (first_throughput); lowest priority
    hipEvent_t tail_ev[2] = {};                                                  // ... fork (in front of the bulk kernel) and join (behind the remainder's last launch)
    Buf tb_tail;                                                                 // ... its traceback scratch: d->tb is the running bulk's
    bool tail_side = false;                                                      // launch_mt is running for that remainder: tb_tail and the second block of work counters (kTailCounterBase)
    bool fork_next = false;                                                      // launch_lean records tail_ev[0] between its fills and its kernel
    hipEvent_t ev[8] = {};                                                       // [6], [7]: the write-back of a level (twl_level_commit, read later by twl_level_timing)
    int num_cu = 0;
    Buf cols, tb, cells, queue, items, errs, dbg;
    Buf gtb;                                                                     // scratch of the global-memory kernel (DP rows + pointer bytes of its pairs): its own buffer, handed back after the stage when large
    Buf sim, sim_off, blk_off, m24;                                              // precomputed protein scores (matrix mode 4)
    std::vector<long long> sim_last_off;                                         // twl_dp_score_matrix: per pair of the last call that precomputed, the first float of its block in `sim` (-1: the pair did not run) ...
    std::vector<int32_t> sim_last_len;                                           // ... its {R, Q} ...
    int sim_last_corridor = 0;                                                   // ... and the corridor score_matrix_kernel was given.  Empty vectors: the last call did not precompute
    Buf team;                                                                    // mailboxes of the speculative tile start
    Buf mt_chain, mt_rec, mt_seg, mt_spath, mt_stat, mt_jobs, mt_anchor;                    // tile-parallel alignment (talco_nuc.hip.h, MT kernels)
    Buf simdump;                                                                 // twl_dp_column_scores: [Q][R] scores written by the DUMP kernels
    bool dump_on = false;
    std::vector<int32_t> dbg_host;
    std::vector<int32_t> mt_jobs_host;
    twl_mt_dims mt_dims{};                                                       // twl_mt_tables: the plan of the last tile-parallel level (launch_mt) ...
    std::vector<int32_t> mt_order;                                               // ... the pair of every table row ...
    bool mt_seen = false;                                                        // ... and whether one has run since twl_init
    Buf gc_zero;                         // [pair] flags of a call with pairs of both gap-character kinds (run_device)
    std::vector<uint8_t> gc_zero_host;
    std::vector<int16_t> last_err;                                               // error codes of the last run_device call, as read back by it
    void *probe_h = nullptr; size_t probe_cap = 0;                               // pinned: error codes of a level's sample (run_device, Throughput)
    PassMemory mem;                                                              // what the earlier calls of this pass found (twl_policy.inc.hip)
    int live_stores = 0;                                                         // twl_store handles alive on this device (twl_level.h); guarded by mu
    void *comm = nullptr;                                                        // ncclComm_t of a sharded run (twl_comm_init)
    int comm_world = 0, comm_rank = 0;
    Buf comm_send, comm_recv;                                                    // staging of twl_comm_all_gather_host
    int mt_launch = 0;                                                           // launches of the tile-parallel level in flight (work counter index)
    char kname[160] = {0};                                                       // the kernel of the first DP launch of the call in flight
    Buf h2d_freq, h2d_gop, h2d_gex, h2d_len, h2d_num, d_aln, d_alnlen, d_err;   // staging for the host form
    twl_stats stats{};
    std::vector<uint64_t> pair_cells;
    twl::FillArgs fills{};                                                        // byte fills queued for ONE launch in front of the next kernel (queue_fill / flush_fills)
    char *res_h = nullptr; size_t res_cap = 0;                                   // pinned host block the results of a call come back in (collect_kernel writes it)
    std::vector<int32_t> last_alnlen;                                            // path lengths of the last run_device call, as read back by it
    std::mutex mu;
};

std::vector<Device *> g_devs;
bool g_init = false;

int find_dev(int device, Device **out)
{
    for (auto *d : g_devs) if (d->id == device) { *out = d; return TWL_OK; }
    g_err = "device not selected in twl_init";
    return TWL_ERR_BAD_ARGUMENT;
}

// Byte fills queued in front of the next kernel of the device's stream: one launch for all of them (16-byte aligned pointers).
int flush_fills(Device *d, hipStream_t st)
{
    if (d->fills.n == 0) return TWL_OK;
    unsigned long long most = 0;
    for (int r = 0; r < d->fills.n; ++r) most = std::max(most, d->fills.j[r].bytes);
    const unsigned blocks = (unsigned)std::max<unsigned long long>(1, std::min<unsigned long long>((most / 16 + 255) / 256, (unsigned long long)d->num_cu * 8));
    hipLaunchKernelGGL(twl::fill_kernel, dim3(blocks), dim3(256), 0, st, d->fills);
    d->fills.n = 0;
    HIP_TRY(hipGetLastError());
    return TWL_OK;
}
int queue_fill(Device *d, hipStream_t st, void *p, size_t bytes, unsigned char v)
{
    if (!bytes) return TWL_OK;
    if (((size_t)p & 15) != 0) { HIP_TRY(hipMemsetAsync(p, v, bytes, st)); return TWL_OK; }
    if (d->fills.n == 8) { const int rc = flush_fills(d, st); if (rc) return rc; }
    d->fills.j[d->fills.n++] = twl::FillJob{p, (unsigned long long)bytes, 0x01010101u * v};
    return TWL_OK;
}
#define FILL_TRY(expr) do { const int rc_ = (expr); if (rc_) return rc_; } while (0)

int check_params(const twl_params *p)
{
    if (!p) { g_err = "params is null"; return TWL_ERR_BAD_ARGUMENT; }
    if (p->P != 6 && p->P != 22) { g_err = "profile width P must be 6 (nucleotide) or 22 (protein)"; return TWL_ERR_UNSUPPORTED; }
    if (p->marker < 2 || p->marker > TWL_MAX_MARKER) { g_err = "marker outside [2, TWL_MAX_MARKER]"; return TWL_ERR_UNSUPPORTED; }
    // flen is only a cap on the anti-diagonal width (TALCO-XDrop.cpp:258,331-338): the deferred pass raises it to min(R, Q)
    // (alignment-cpu.cpp:116-129).  Any value is accepted; what is limited is the band the widest kernel can hold (4608 rows).
    if (p->flen < 1) { g_err = "flen < 1"; return TWL_ERR_UNSUPPORTED; }
    if (p->xdrop < 0) { g_err = "xdrop < 0"; return TWL_ERR_BAD_ARGUMENT; }
    return TWL_OK;
}

#include "twl_knobs.inc.hip"
#include "twl_launch.inc.hip"
#include "twl_run.inc.hip"

}  // namespace

static void twl_level_pool_release(Device *d);      // twl_store.inc.hip: the level buffers the device lent to its stores
namespace { extern int g_fail_next_row_allocs; void comm_destroy_raw(void *comm); }

extern "C" {

const char *twl_last_error(void) { return g_err.c_str(); }
#ifndef TWL_SOURCE_HASH
#define TWL_SOURCE_HASH "unstamped"
#endif
#ifndef TWL_BUILD_STAMP
#define TWL_BUILD_STAMP "unstamped"
#endif
// digest of every source, header and flag of this build: __graft_entry__.build() looks for it in the file and rebuilds when it is another
__attribute__((used)) static const char twl_build_stamp[] = "TWLSTAMP:" TWL_BUILD_STAMP ";";
const char *twl_version(void) { return "twilight_amd 0.5 (gfx950) src " TWL_SOURCE_HASH; }      // (the hash of the kernel sources: __graft_entry__.source_hash)

int twl_init(const int *device_ids, int n_devices)
{
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_init) return TWL_OK;
    int count = 0;
    HIP_TRY(hipGetDeviceCount(&count));
    if (count < 1) { g_err = "no HIP device"; return TWL_ERR_HIP; }
    std::vector<int> ids;
    if (!device_ids || n_devices <= 0) ids.push_back(0);
    else ids.assign(device_ids, device_ids + n_devices);
    std::vector<Device *> devs;      // committed to g_devs only when every device came up
    auto fail = [&](int rc) {
        for (auto *d : devs) {
            for (auto &e : d->ev) if (e) (void)hipEventDestroy(e);
            if (d->stream) (void)hipStreamDestroy(d->stream);
            if (d->stream2) (void)hipStreamDestroy(d->stream2);
            if (d->tail_stream) (void)hipStreamDestroy(d->tail_stream);
            for (auto &e : d->ev2) if (e) (void)hipEventDestroy(e);
            for (auto &e : d->tail_ev) if (e) (void)hipEventDestroy(e);
            delete d;
        }
        return rc;
    };
    for (int id : ids) {
        if (id < 0 || id >= count) { g_err = "device id out of range"; return fail(TWL_ERR_BAD_ARGUMENT); }
        auto *d = new Device();
        d->id = id;
        devs.push_back(d);
        hipDeviceProp_t prop;
        hipError_t e = hipSetDevice(id);
        if (e == hipSuccess) e = hipGetDeviceProperties(&prop, id);
        if (e == hipSuccess) { d->num_cu = prop.multiProcessorCount; e = hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking); if (e == hipSuccess) { int least = 0, greatest = 0; (void)hipDeviceGetStreamPriorityRange(&least, &greatest); e = hipStreamCreateWithPriority(&d->stream2, hipStreamNonBlocking, least); if (e == hipSuccess) e = hipStreamCreateWithPriority(&d->tail_stream, hipStreamNonBlocking, least); } }      // (the row rewrites there give way to the DP kernels of the first stream, and so does the remainder of a throughput level on its own stream)
        for (auto &ev : d->ev2) if (e == hipSuccess) e = hipEventCreate(&ev);
        for (auto &ev : d->tail_ev) if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        for (auto &ev : d->ev) if (e == hipSuccess) e = hipEventCreate(&ev);
        if (e != hipSuccess) { g_err = std::string("twl_init: ") + hipGetErrorString(e); return fail(TWL_ERR_HIP); }
    }
    g_devs = devs;
    g_init = true;
#ifdef TWL_DEV      // development builds (__graft_entry__.build() with TWL_DEV_BUILD=1): the knobs of twl_set_knob from the environment, through its clamps
    static const struct { const char *env; int knob; } kEnvKnobs[] = {{"TWL_MT_MAX_PAIRS", TWL_KNOB_MT_MAX_PAIRS}, {"TWL_MT_LEAD", TWL_KNOB_MT_LEAD}, {"TWL_MT_MARGIN", TWL_KNOB_MT_MARGIN},
        {"TWL_MT_PERTURB", TWL_KNOB_MT_PERTURB}, {"TWL_MT_ROUNDS", TWL_KNOB_MT_ROUNDS}, {"TWL_MT_THR_JOBS", TWL_KNOB_MT_THR_JOBS}, {"TWL_MT_TAIL_PCT", TWL_KNOB_MT_TAIL_PCT}};
    for (const auto &k : kEnvKnobs) if (const char *v = getenv(k.env)) (void)twl_set_knob(k.knob, atoi(v));
#endif
    return TWL_OK;
}

void twl_shutdown(void)
{
    std::lock_guard<std::mutex> lk(g_mu);
    // stores (twl_level.h) point into their device's state and pool: with any of them alive the library stays up (destroy them first)
    for (auto *d : g_devs) {
        std::lock_guard<std::mutex> dl(d->mu);
        if (d->live_stores > 0) {
            fprintf(stderr, "twl_shutdown: %d store(s) still alive on device %d; the library stays initialised (twl_store_destroy them first)\n", d->live_stores, d->id);
            return;
        }
    }
    for (auto *d : g_devs) {
        (void)hipSetDevice(d->id);
        (void)hipStreamSynchronize(d->stream);
        (void)hipStreamSynchronize(d->stream2);
        (void)hipStreamSynchronize(d->tail_stream);
        twl_level_pool_release(d);
        if (d->comm) { comm_destroy_raw(d->comm); d->comm = nullptr; }
        d->comm_send.release(); d->comm_recv.release();
        for (Buf *b : {&d->cols, &d->tb, &d->tb_tail, &d->gtb, &d->cells, &d->queue, &d->items, &d->errs, &d->dbg, &d->sim, &d->sim_off, &d->blk_off, &d->m24, &d->team, &d->simdump, &d->mt_chain, &d->mt_rec, &d->mt_seg, &d->mt_spath, &d->mt_stat, &d->mt_jobs, &d->mt_anchor, &d->gc_zero,
                       &d->h2d_freq, &d->h2d_gop, &d->h2d_gex, &d->h2d_len, &d->h2d_num, &d->d_aln, &d->d_alnlen, &d->d_err})
            b->release();
        for (auto &e : d->ev) if (e) (void)hipEventDestroy(e);
        if (d->stream) (void)hipStreamDestroy(d->stream);
        if (d->stream2) (void)hipStreamDestroy(d->stream2);
        if (d->tail_stream) (void)hipStreamDestroy(d->tail_stream);
        for (auto &e : d->ev2) if (e) (void)hipEventDestroy(e);
        for (auto &e : d->tail_ev) if (e) (void)hipEventDestroy(e);
        if (d->res_h) (void)hipHostFree(d->res_h);
        if (d->probe_h) (void)hipHostFree(d->probe_h);
        delete d;
    }
    g_devs.clear();
    g_init = false;
}

int twl_align_batch_device(int device, void *stream, const twl_params *p, int32_t n_pairs, int32_t seq_len, const float *d_freq,
                           const float *d_gap_open, const float *d_gap_extend, const int32_t *d_len, const int32_t *d_num,
                           int8_t *d_aln_out, int32_t *d_aln_len_out, int16_t *d_err_out)
{
    if (!g_init) { g_err = "twl_init not called"; return TWL_ERR_NOT_INITIALIZED; }
    int rc = check_params(p);
    if (rc) return rc;
    if (n_pairs < 0 || seq_len < 1) { g_err = "bad n_pairs/seq_len"; return TWL_ERR_BAD_ARGUMENT; }
    Device *d = nullptr;
    if ((rc = find_dev(device, &d))) return rc;
    std::lock_guard<std::mutex> lk(d->mu);
    hipStream_t st = stream ? (hipStream_t)stream : d->stream;
    return run_device(d, st, p, n_pairs, seq_len, d_freq, d_gap_open, d_gap_extend, d_len, d_num, d_aln_out, d_aln_len_out,
                      d_err_out, nullptr);
}

static int run_host_slice(Device *d, const twl_params *p, const std::vector<int32_t> &ids, int32_t seq_len, const float *freq,
                          const float *gop, const float *gex, const int32_t *len, const int32_t *num, int8_t *aln_out,
                          int32_t *aln_len_out, int16_t *err_out)
{
    std::lock_guard<std::mutex> lk(d->mu);
    HIP_TRY(hipSetDevice(d->id));
    const int32_t n = (int32_t)ids.size();
    d->stats = twl_stats{};          // a device that gets no pairs of this call must not report the previous call's counters
    d->pair_cells.clear();
    if (n == 0) return TWL_OK;
    const size_t P = (size_t)p->P, sl = (size_t)seq_len;
    int rc;
    if ((rc = d->h2d_freq.ensure((size_t)n * 2 * sl * P * sizeof(float)))) return rc;
    if ((rc = d->h2d_gop.ensure((size_t)n * 2 * sl * sizeof(float)))) return rc;
    if ((rc = d->h2d_gex.ensure((size_t)n * 2 * sl * sizeof(float)))) return rc;
    if ((rc = d->h2d_len.ensure((size_t)n * 2 * sizeof(int32_t)))) return rc;
    if ((rc = d->h2d_num.ensure((size_t)n * 2 * sizeof(int32_t)))) return rc;
    if ((rc = d->d_aln.ensure((size_t)n * 2 * sl))) return rc;
    if ((rc = d->d_alnlen.ensure((size_t)n * sizeof(int32_t)))) return rc;
    if ((rc = d->d_err.ensure((size_t)n * sizeof(int16_t)))) return rc;
    hipStream_t st = d->stream;
    std::vector<int32_t> hl((size_t)n * 2), hn((size_t)n * 2);
    HIP_TRY(hipEventRecord(d->ev[5], st));
    bool contiguous = true;
    for (int32_t t = 0; t < n; ++t) contiguous = contiguous && ids[t] == ids[0] + t;
    for (int32_t t = 0; t < n; ++t) {
        const size_t s = (size_t)ids[t];
        hl[2 * t] = len[2 * s]; hl[2 * t + 1] = len[2 * s + 1];
        hn[2 * t] = num[2 * s]; hn[2 * t + 1] = num[2 * s + 1];
    }
    if (contiguous) {      // one transfer per array instead of three per pair
        const size_t s0 = (size_t)ids[0];
        HIP_TRY(hipMemcpyAsync(d->h2d_freq.p, freq + s0 * 2 * sl * P, (size_t)n * 2 * sl * P * sizeof(float), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d->h2d_gop.p, gop + s0 * 2 * sl, (size_t)n * 2 * sl * sizeof(float), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d->h2d_gex.p, gex + s0 * 2 * sl, (size_t)n * 2 * sl * sizeof(float), hipMemcpyHostToDevice, st));
    } else {
        for (int32_t t = 0; t < n; ++t) {
            const size_t s = (size_t)ids[t];
            HIP_TRY(hipMemcpyAsync((float *)d->h2d_freq.p + (size_t)t * 2 * sl * P, freq + s * 2 * sl * P, 2 * sl * P * sizeof(float), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync((float *)d->h2d_gop.p + (size_t)t * 2 * sl, gop + s * 2 * sl, 2 * sl * sizeof(float), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync((float *)d->h2d_gex.p + (size_t)t * 2 * sl, gex + s * 2 * sl, 2 * sl * sizeof(float), hipMemcpyHostToDevice, st));
        }
    }
    HIP_TRY(hipMemcpyAsync(d->h2d_len.p, hl.data(), hl.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d->h2d_num.p, hn.data(), hn.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    rc = run_device(d, st, p, n, seq_len, (const float *)d->h2d_freq.p, (const float *)d->h2d_gop.p, (const float *)d->h2d_gex.p,
                    (const int32_t *)d->h2d_len.p, (const int32_t *)d->h2d_num.p, (int8_t *)d->d_aln.p, (int32_t *)d->d_alnlen.p,
                    (int16_t *)d->d_err.p, hl.data());
    if (rc) return rc;
    std::vector<int32_t> alen((size_t)n);
    std::vector<int16_t> aerr((size_t)n);
    HIP_TRY(hipMemcpyAsync(alen.data(), d->d_alnlen.p, alen.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(aerr.data(), d->d_err.p, aerr.size() * sizeof(int16_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    size_t path_bytes = 0;
    for (int32_t t = 0; t < n; ++t) path_bytes += (size_t)std::max(alen[t], 0);
    // paths: one transfer of the whole [n][2*seq_len] block when the slice is contiguous and reasonably full, else one per pair
    const bool bulk = contiguous && path_bytes * 8 >= (size_t)n * 2 * sl;
    if (bulk) HIP_TRY(hipMemcpyAsync(aln_out + (size_t)ids[0] * 2 * sl, d->d_aln.p, (size_t)n * 2 * sl, hipMemcpyDeviceToHost, st));
    for (int32_t t = 0; t < n; ++t) {
        const size_t s = (size_t)ids[t];
        aln_len_out[s] = alen[t];
        err_out[s] = aerr[t];
        if (!bulk && alen[t] > 0)
            HIP_TRY(hipMemcpyAsync(aln_out + s * 2 * sl, (int8_t *)d->d_aln.p + (size_t)t * 2 * sl, (size_t)alen[t], hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipEventRecord(d->ev[3], st));
    HIP_TRY(hipStreamSynchronize(st));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, d->ev[5], d->ev[3]));
    d->stats.total_ms = ms;
    return TWL_OK;
}

int twl_align_batch(const twl_params *p, int32_t n_pairs, int32_t seq_len, const float *freq, const float *gap_open,
                    const float *gap_extend, const int32_t *len, const int32_t *num, int8_t *aln_out, int32_t *aln_len_out,
                    int16_t *err_out)
{
    if (!g_init) { g_err = "twl_init not called"; return TWL_ERR_NOT_INITIALIZED; }
    int rc = check_params(p);
    if (rc) return rc;
    if (n_pairs < 0 || seq_len < 1 || (n_pairs > 0 && (!freq || !gap_open || !gap_extend || !len || !num || !aln_out || !aln_len_out || !err_out))) {
        g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT;
    }
    const size_t nd = g_devs.size();
    // deal pairs to devices in descending cost order (independent units, no collective)
    std::vector<int32_t> order((size_t)n_pairs);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) {
        return (int64_t)len[2 * x] + len[2 * x + 1] > (int64_t)len[2 * y] + len[2 * y + 1];
    });
    std::vector<std::vector<int32_t>> slices(nd);
    if (nd == 1) { slices[0].resize((size_t)n_pairs); std::iota(slices[0].begin(), slices[0].end(), 0); }   // bulk copies; the device orders by cost itself
    else for (size_t t = 0; t < order.size(); ++t) slices[t % nd].push_back(order[t]);
    if (nd == 1) return run_host_slice(g_devs[0], p, slices[0], seq_len, freq, gap_open, gap_extend, len, num, aln_out, aln_len_out, err_out);
    std::vector<int> rcs(nd, 0);
    std::vector<std::string> errs(nd);
    std::vector<std::thread> th;
    for (size_t i = 0; i < nd; ++i)
        th.emplace_back([&, i] {
            rcs[i] = run_host_slice(g_devs[i], p, slices[i], seq_len, freq, gap_open, gap_extend, len, num, aln_out, aln_len_out, err_out);
            errs[i] = g_err;
        });
    for (auto &t : th) t.join();
    for (size_t i = 0; i < nd; ++i) if (rcs[i]) { g_err = errs[i]; return rcs[i]; }
    return TWL_OK;
}

int twl_get_stats(int device, twl_stats *out)
{
    if (!g_init) { g_err = "twl_init not called"; return TWL_ERR_NOT_INITIALIZED; }
    if (!out) { g_err = "out is null"; return TWL_ERR_BAD_ARGUMENT; }
    Device *d = nullptr;
    int rc = find_dev(device, &d);
    if (rc) return rc;
    *out = d->stats;
    return TWL_OK;
}

// Diagnostics: similarScore(i, j) (TALCO-XDrop.cpp:444) of one pair for every (query row i, reference column j), row-major
// out[Q][R], computed by score_matrix_kernel -- the arithmetic the DP kernels use (for nucleotides the general 5x5 order).
int twl_column_scores(const twl_params *p, int32_t seq_len, const float *freq, const int32_t *len, const int32_t *num, float *out)
{
    if (!g_init) { g_err = "twl_init not called"; return TWL_ERR_NOT_INITIALIZED; }
    int rc = check_params(p);
    if (rc) return rc;
    if (seq_len < 1 || !freq || !len || !num || !out || len[0] < 1 || len[1] < 1 || len[0] > seq_len || len[1] > seq_len) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    Device *d = g_devs[0];
    std::lock_guard<std::mutex> lk(d->mu);
    HIP_TRY(hipSetDevice(d->id));
    hipStream_t st = d->stream;
    const size_t P = (size_t)p->P, sl = (size_t)seq_len, CW = P + 2;
    const int R = len[0], Q = len[1];
    const size_t pitch = ((size_t)Q + 63) & ~(size_t)63, simFloats = (size_t)(R + Q) * pitch;
    if ((rc = d->h2d_freq.ensure(2 * sl * P * sizeof(float)))) return rc;
    if ((rc = d->h2d_gop.ensure(2 * sl * sizeof(float)))) return rc;
    if ((rc = d->cols.ensure(2 * sl * CW * sizeof(float)))) return rc;
    if ((rc = d->h2d_len.ensure(2 * sizeof(int32_t)))) return rc;
    if ((rc = d->h2d_num.ensure(2 * sizeof(int32_t)))) return rc;
    if ((rc = d->items.ensure(sizeof(int32_t)))) return rc;
    d->sim_last_off.clear(); d->sim_last_len.clear(); d->sim_last_corridor = 0;      // (the buffer twl_dp_score_matrix reads is overwritten here)
    if ((rc = d->sim.ensure(simFloats * sizeof(float)))) return rc;
    if ((rc = d->sim_off.ensure(sizeof(long long)))) return rc;
    if ((rc = d->blk_off.ensure(2 * sizeof(int32_t)))) return rc;
    if ((rc = d->m24.ensure(21 * 24 * sizeof(float)))) return rc;
    std::vector<float> m24(21 * 24, 0.0f);
    const int ms = p->P - 1;
    for (int l = 0; l < ms; ++l) for (int m = 0; m < ms; ++m) m24[(ms == 21 ? 24 : 5) * l + m] = p->matrix[ms * l + m];
    const int32_t item = 0, blk[2] = {0, (int32_t)(((R + Q - 1 + 63) / 64) * ((Q + 63) / 64))};
    const long long off = 0;
    HIP_TRY(hipMemcpyAsync(d->h2d_freq.p, freq, 2 * sl * P * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d->h2d_gop.p, 0, 2 * sl * sizeof(float), st));
    HIP_TRY(hipMemcpyAsync(d->h2d_len.p, len, 2 * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d->h2d_num.p, num, 2 * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d->items.p, &item, sizeof item, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d->sim_off.p, &off, sizeof off, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d->blk_off.p, blk, sizeof blk, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d->m24.p, m24.data(), m24.size() * sizeof(float), hipMemcpyHostToDevice, st));
    const size_t n_cols = 2 * sl;
    const int blocks = (int)((n_cols + 255) / 256);
    if (p->P == 22) hipLaunchKernelGGL(twl::pack_kernel<22>, dim3(blocks), dim3(256), 0, st, (const float *)d->h2d_freq.p, (const float *)d->h2d_gop.p, (const float *)d->h2d_gop.p, (float *)d->cols.p, n_cols);
    else hipLaunchKernelGGL(twl::pack_kernel<6>, dim3(blocks), dim3(256), 0, st, (const float *)d->h2d_freq.p, (const float *)d->h2d_gop.p, (const float *)d->h2d_gop.p, (float *)d->cols.p, n_cols);
    twl::ScoreArgs sa{};
    sa.cols = (const float *)d->cols.p; sa.len = (const int32_t *)d->h2d_len.p; sa.num = (const int32_t *)d->h2d_num.p;
    sa.items = (const int32_t *)d->items.p; sa.blk_off = (const int32_t *)d->blk_off.p; sa.n_items = 1; sa.seq_len = seq_len;
    sa.gap_char = p->gap_char; sa.M24 = (const float *)d->m24.p; sa.sim = (float *)d->sim.p; sa.sim_off = (const long long *)d->sim_off.p;
    if (p->P == 22) hipLaunchKernelGGL(twl::score_matrix_kernel<22>, dim3((unsigned)blk[1]), dim3(256), 0, st, sa);
    else hipLaunchKernelGGL(twl::score_matrix_kernel<6>, dim3((unsigned)blk[1]), dim3(256), 0, st, sa);
    HIP_TRY(hipGetLastError());
    std::vector<float> diag(simFloats);
    HIP_TRY(hipMemcpyAsync(diag.data(), d->sim.p, simFloats * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int i = 0; i < Q; ++i)
        for (int j = 0; j < R; ++j) out[(size_t)i * R + j] = diag[(size_t)(i + j) * pitch + i];
    return TWL_OK;
}

int twl_dp_column_scores(const twl_params *p, int32_t seq_len, const float *freq, const float *gap_open, const float *gap_extend,
                         const int32_t *len, const int32_t *num, float *out)
{
    if (!g_init) { g_err = "twl_init not called"; return TWL_ERR_NOT_INITIALIZED; }
    int rc = check_params(p);
    if (rc) return rc;
    if (seq_len < 1 || !freq || !gap_open || !gap_extend || !len || !num || !out || len[0] < 1 || len[1] < 1 || len[0] > seq_len || len[1] > seq_len) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    Device *d = g_devs[0];
    const size_t cells = (size_t)len[0] * (size_t)len[1];
    {
        std::lock_guard<std::mutex> lk(d->mu);
        HIP_TRY(hipSetDevice(d->id));
        if ((rc = d->simdump.ensure(cells * sizeof(float)))) return rc;
        HIP_TRY(hipMemset(d->simdump.p, 0xff, cells * sizeof(float)));      // NaN: a cell the band never visited
        d->dump_on = true;
    }
    std::vector<int8_t> aln(2 * (size_t)seq_len);
    int32_t alen = 0;
    int16_t aerr = 0;
    rc = twl_align_batch(p, 1, seq_len, freq, gap_open, gap_extend, len, num, aln.data(), &alen, &aerr);
    std::lock_guard<std::mutex> lk(d->mu);
    d->dump_on = false;
    if (rc) return rc;
    HIP_TRY(hipSetDevice(d->id));
    HIP_TRY(hipMemcpy(out, d->simdump.p, cells * sizeof(float), hipMemcpyDeviceToHost));
    return TWL_OK;
}

// debug aid (not in the public header): first `n` 64-bit words of the last call's debug record (TWL_DEBUG=1)
int twl_debug_read(int device, long long *out, int32_t n)
{
    Device *d = nullptr;
    if (find_dev(device, &d)) return TWL_ERR_BAD_ARGUMENT;
    // the stamp record (TWL_KERNEL_STAMPS builds) sits after the per-pair records
    const size_t base = d->pair_cells.size() * 16 * sizeof(int32_t);
    if (!d->dbg.p || base + (size_t)n * 8 > d->dbg.cap) return TWL_ERR_BAD_ARGUMENT;
    return hipMemcpy(out, (const char *)d->dbg.p + base, (size_t)n * 8, hipMemcpyDeviceToHost) == hipSuccess ? TWL_OK : TWL_ERR_HIP;
}

void *twl_host_alloc(uint64_t bytes)
{
    void *p = nullptr;
    if (!g_init || bytes == 0) return nullptr;
    if (hipHostMalloc(&p, (size_t)bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}

void twl_host_free(void *p)
{
    if (p) (void)hipHostFree(p);
}

int twl_copy_to_device(int device, void *dst_dev, const void *src, uint64_t bytes)
{
    if (!g_init) { g_err = "twl_init not called"; return TWL_ERR_NOT_INITIALIZED; }
    Device *d = nullptr;
    int rc = find_dev(device, &d);
    if (rc) return rc;
    if (bytes == 0) return TWL_OK;
    if (!dst_dev || !src) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    HIP_TRY(hipSetDevice(d->id));
    HIP_TRY(hipMemcpy(dst_dev, src, (size_t)bytes, hipMemcpyHostToDevice));
    return TWL_OK;
}

int twl_copy_from_device(int device, void *dst, const void *src_dev, uint64_t bytes)
{
    if (!g_init) { g_err = "twl_init not called"; return TWL_ERR_NOT_INITIALIZED; }
    Device *d = nullptr;
    int rc = find_dev(device, &d);
    if (rc) return rc;
    if (bytes == 0) return TWL_OK;
    if (!dst || !src_dev) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    HIP_TRY(hipSetDevice(d->id));
    HIP_TRY(hipMemcpy(dst, src_dev, (size_t)bytes, hipMemcpyDeviceToHost));
    return TWL_OK;
}

int twl_copy_rows_from_device(int device, void *dst, uint64_t dst_pitch, const void *src_dev, uint64_t src_pitch, uint64_t width, uint64_t rows)
{
    if (!g_init) { g_err = "twl_init not called"; return TWL_ERR_NOT_INITIALIZED; }
    Device *d = nullptr;
    int rc = find_dev(device, &d);
    if (rc) return rc;
    if (width == 0 || rows == 0) return TWL_OK;
    if (!dst || !src_dev || dst_pitch < width || src_pitch < width) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    HIP_TRY(hipSetDevice(d->id));
    HIP_TRY(hipMemcpy2D(dst, (size_t)dst_pitch, src_dev, (size_t)src_pitch, (size_t)width, (size_t)rows, hipMemcpyDeviceToHost));
    return TWL_OK;
}

int twl_set_knob(int key, int value)
{
    std::lock_guard<std::mutex> lk(g_mu);
    switch (key) {
    case TWL_KNOB_MT_PERTURB: g_mt_perturb = std::max(0, value); return TWL_OK;
    case TWL_KNOB_MT_MAX_PAIRS: g_mt_max_pairs = std::max(0, value); return TWL_OK;
    case TWL_KNOB_MT_MIN_MARKER: g_mt_min_marker = std::max(2, value); return TWL_OK;
    case TWL_KNOB_MT_LEAD: g_mt_lead = std::max(16, value); return TWL_OK;
    case TWL_KNOB_MT_MARGIN: if (value < 0) { g_mt_marg = 40; g_mt_marg_lat = 64; } else g_mt_marg = g_mt_marg_lat = std::max(2, value); return TWL_OK;      // (negative: the defaults of both kinds of level)
    case TWL_KNOB_MT_ROUNDS: g_mt_rounds = std::max(1, std::min(7, value)); return TWL_OK;
    case TWL_KNOB_MT_THR_JOBS: g_mt_thr_jobs = std::max(0, value); return TWL_OK;
    case TWL_KNOB_FAIL_ROW_ALLOCS: g_fail_next_row_allocs = std::max(0, value); return TWL_OK;
    case TWL_KNOB_PROT_MODE: if (value < 0 || value > 6) { g_err = "protein mode 0..6"; return TWL_ERR_BAD_ARGUMENT; } g_prot_mode = value; return TWL_OK;
    case TWL_KNOB_ASSUME_ONEHOT_QUERY: g_assume_onehot_query = value ? 1 : 0; return TWL_OK;
    case TWL_KNOB_MT_TAIL_PCT: g_mt_tail_pct = std::max(0, std::min(100, value)); return TWL_OK;
    case TWL_KNOB_MT_WIDE: g_mt_wide = value ? 1 : 0; return TWL_OK;
    case TWL_KNOB_NO_SPEC: g_no_spec = value ? 1 : 0; return TWL_OK;
    case TWL_KNOB_FORCE_GLOBAL: g_force_global = value ? 1 : 0; return TWL_OK;
    case TWL_KNOB_LEAF_STEP: g_leaf_step = value ? 1 : 0; return TWL_OK;
    case TWL_KNOB_POISON_TB: g_poison_tb = value ? 1 : 0; return TWL_OK;
    case TWL_KNOB_MT_ANCHOR: g_mt_anchor = value ? 1 : 0; return TWL_OK;
    case TWL_KNOB_MT_LEAD2: if (value < 0) { g_mt_lead2 = 96; g_mt_lead2_lat = 128; } else g_mt_lead2 = g_mt_lead2_lat = std::max(16, value); return TWL_OK;
    case TWL_KNOB_PROT_CORRIDOR: g_prot_corridor = std::max(0, value); for (auto *d : g_devs) d->mem.forget_corridor(); return TWL_OK;      // (and forgets what earlier levels found)
    case TWL_KNOB_SCOUT_XDROP_PCT: g_scout_xdrop_pct = std::max(10, std::min(100, value)); return TWL_OK;
    case TWL_KNOB_TAIL_OVERLAP: g_tail_overlap = value ? 1 : 0; return TWL_OK;
    case TWL_KNOB_THR_SMALL: g_thr_small = std::max(0, std::min(2, value)); for (auto *d : g_devs) d->mem.forget_small(); return TWL_OK;      // (and forgets what earlier levels found)
    default: g_err = "unknown knob"; return TWL_ERR_BAD_ARGUMENT;
    }
}

#include "twl_comm.inc.hip"

// The launch plan of a call, as run_device would make it, in words: no device is touched (unit tests of the policy on a CPU-only box).
int twl_plan_describe(const twl_params *p, int32_t n_pairs, const int32_t *len, int32_t num_cu, int32_t qry_onehot, int32_t wide_streak, char *out, int32_t cap)
{
    if (!p || (p->P != 6 && p->P != 22) || n_pairs < 0 || (n_pairs > 0 && !len) || num_cu < 1 || !out || cap < 64) { g_err = "bad argument (nucleotide or protein parameters, a buffer of 64+ bytes)"; return TWL_ERR_BAD_ARGUMENT; }
    const PassMemory mem = memory_from_code(wide_streak);
    std::vector<int32_t> order;
    for (int32_t n = 0; n < n_pairs; ++n) if (len[2 * n] > 0 && len[2 * n + 1] > 0) order.push_back(n);
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return (int64_t)len[2 * x] + len[2 * x + 1] > (int64_t)len[2 * y] + len[2 * y + 1]; });
    const int ms = p->P - 1;
    std::vector<float> M(p->matrix, p->matrix + ms * ms);
    if (p->P == 22) {
        ProtFacts pf;
        pf.n_run = (int)order.size(); pf.n_pairs = n_pairs; pf.num_cu = num_cu; pf.marker = p->marker; pf.M = M.data(); pf.gap_char = p->gap_char;
        pf.corridor_lost = mem.corridor_lost; pf.h_len = len; pf.order = order.data();
        const ProtPlan pl = plan_protein(pf, current_knobs());
        const int w = snprintf(out, (size_t)cap, "%s; mode %d; window %d", prot_first_name(pl.first), pl.mm, prot_first_window(pl.first));
        if (pl.presim && w > 0 && w < cap) snprintf(out + w, (size_t)(cap - w), "; %zu scores precomputed, corridor %d", pl.simFloats, pl.corridor);
        return TWL_OK;
    }
    NucFacts nf;
    nf.n_run = (int)order.size(); nf.num_cu = num_cu; nf.marker = p->marker; nf.M = M.data(); nf.gap_char = p->gap_char; nf.qry_onehot = qry_onehot != 0;
    nf.remember(mem); nf.h_len = len; nf.order = order.data();
    const NucPlan pl = plan_nucleotide(nf, current_knobs());
    snprintf(out, (size_t)cap, "%s; mode %d; window %d%s; bulk %d tail %d", nuc_first_name(pl.first), pl.mm5 ? 5 : pl.mm,
             pl.first == NucFirst::WideMt ? 3072 : ((pl.first == NucFirst::Throughput && pl.small) ? 512 : ((pl.first == NucFirst::Throughput && pl.four) ? 768 : 1024)), pl.probe ? " or 768 (a sample of the level decides)" : "", pl.bulk, pl.tail);
    return TWL_OK;
}

int twl_get_pair_cells(int device, uint64_t *cells_out, int32_t n)
{
    if (!g_init) { g_err = "twl_init not called"; return TWL_ERR_NOT_INITIALIZED; }
    Device *d = nullptr;
    int rc = find_dev(device, &d);
    if (rc) return rc;
    if (!cells_out || n < 0 || (size_t)n > d->pair_cells.size()) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    for (int32_t i = 0; i < n; ++i) cells_out[i] = d->pair_cells[i];
    return TWL_OK;
}

int twl_mt_tables(int device, twl_mt_dims *dims, int32_t *order, int32_t *anchor, int32_t *spath, int32_t *chain, int32_t *rec, int8_t *seg, int32_t *front)
{
    if (!g_init) { g_err = "twl_init not called"; return TWL_ERR_NOT_INITIALIZED; }
    Device *d = nullptr;
    int rc = find_dev(device, &d);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(d->mu);
    return read_mt_tables(d, dims, order, anchor, spath, chain, rec, seg, front);
}

// twl_dp_score_matrix: a plain copy of one pair's block of the scores score_matrix_kernel left behind, after the device's stream has drained.  No launch.
int twl_dp_score_matrix(int device, int32_t pair, twl_score_dims *dims, float *out)
{
    if (!g_init) { g_err = "twl_init not called"; return TWL_ERR_NOT_INITIALIZED; }
    Device *d = nullptr;
    int rc = find_dev(device, &d);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(d->mu);
    if (d->sim_last_off.empty()) { g_err = "the last call on this device did not precompute its column scores"; return TWL_ERR_UNSUPPORTED; }
    if (pair < 0 || (size_t)pair >= d->sim_last_off.size()) { g_err = "bad argument"; return TWL_ERR_BAD_ARGUMENT; }
    if (d->sim_last_off[(size_t)pair] < 0) { g_err = "the pair did not run in the last call"; return TWL_ERR_UNSUPPORTED; }
    const int32_t R = d->sim_last_len[2 * (size_t)pair], Q = d->sim_last_len[2 * (size_t)pair + 1];
    const size_t pitch = ((size_t)Q + 63) & ~(size_t)63, floats = (size_t)(R + Q) * pitch;
    if (dims) { *dims = twl_score_dims{}; dims->R = R; dims->Q = Q; dims->pitch = (int32_t)pitch; dims->corridor = d->sim_last_corridor; }
    if (!out) return TWL_OK;
    if (((size_t)d->sim_last_off[(size_t)pair] + floats) * sizeof(float) > d->sim.cap) { g_err = "internal: the pair's block lies outside the score buffer"; return TWL_ERR_HIP; }
    HIP_TRY(hipSetDevice(d->id));
    HIP_TRY(hipStreamSynchronize(d->stream));
    HIP_TRY(hipMemcpy(out, (const float *)d->sim.p + d->sim_last_off[(size_t)pair], floats * sizeof(float), hipMemcpyDeviceToHost));
    return TWL_OK;
}

}  // extern "C"

#include "twl_level_plan.inc.hip"
#include "twl_store.inc.hip"
#include "twl_level.inc.hip"
#include "twl_place.inc.hip"
#include "twl_keep.inc.hip"
#include "twl_merge.inc.hip"
#include "twl_subtree.inc.hip"
#include "twl_guide.inc.hip"
#include "twl_guide_set.inc.hip"
#include "twl_strand.inc.hip"
#include "twl_retree.inc.hip"
#include "twl_retree_set.inc.hip"
#include "twl_backbone.inc.hip"
#include "twl_trim.inc.hip"
#include "twl_compare.inc.hip"
#include "twl_score.inc.hip"
