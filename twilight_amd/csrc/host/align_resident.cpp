// twilight_amd/csrc/host/align_resident.cpp -- msa::progressive::gpu::alignmentKernel_Resident: the level kernel with the
// sequences resident in HBM (include/twl_level.h).  Same phases and policy as cpu::alignmentKernel_CPU
// (/root/reference/src/alignment-cpu.cpp:32-183); what moves to the device besides the DP is calculateProfile,
// getConsensus, removeGappyColumns, calculatePSGP (before) and updateFrequency + the row rewriting of updateAlignment (after).
// The host keeps the policy: empty sides, low-quality singletons, retry/defer, addGappyColumnsBack, Node bookkeeping.
//
// Differences from the host-staged kernel that do not change the result:
//  * groups of > 1000 sequences are not compressed into one negative id (alignment-helper.cpp:479-500): that device only saves the
//    reference per-level row rewriting, which here is a sub-millisecond kernel; every row is simply kept up to date.
//  * the deferred pass (currentTask 1, /root/reference/src/progressive.cpp:270-298) runs here too since round 4: the rows and the cached
//    profiles of the root and of the deferred nodes stay in HBM, every pair takes gapCharScore 0 and a failed pair is retried with the
//    larger X-drop / band limit of /root/reference/src/alignment-cpu.cpp:116-129 (per pair: twl_level_align with a one-pair mask).  Its
//    profiles cannot be batched: each is aligned to the root the previous one has just been merged into (:283-285).  Rows come back to
//    the host after it (progressive.cpp of this directory); currentTask 2 and a run whose rows are on the host already take alignmentKernel_GPU.
//
// Several devices (phase 2) without any collective: every device holds a replica of the store.  Profile building and the
// write-back are ~1 % of a level's device time, so EVERY device runs them for ALL pairs of the level (the replicas stay identical by
// construction, cached profiles included); only the DP -- the 99 % -- is sharded: each device aligns its share of the pairs
// (twl_level_align with a mask, longest-processing-time deal), the paths meet on the host, and every device commits all of them.
// Per level only paths cross PCIe, nothing crosses xGMI.  --test-virtual-devices k (tests) runs k replicas on the first device.
//
// A level in steps (alignmentKernel_Resident at the end of the file drives them): describeLevel, prepareOnReplicas, fetchColumnInfo, planDp,
// alignShare per replica, mergeShares, joinHandedBack, exchange, judgeFailures, finalPathsOnHost, commitAndBookkeep, closeLevel.
#include "align_gpu.hpp"

#include <cstring>
#include <omp.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <thread>

namespace msa {
namespace progressive {
namespace gpu {

namespace {

// the per-run state (store replicas, cache ids, totals) lives in RunCtx (align_gpu.hpp), reached through the SequenceDB
inline twl_store *firstStore(const RunCtx &ctx) { return ctx.stores.empty() ? nullptr : ctx.stores[0]; }

// Grow-only, never zero-filled staging shared by the runs of a process (one run aligns at a time): a level of 3 000 pairs x 10 kbp
// moves ~70 MB per array and first-touch page faults cost more than the copies.
std::vector<RunCtx::Raw> g_alnStage;      // per replica: paths as the DP wrote them
RunCtx::Raw g_finalStage, g_infoStage;    // final paths as the commit reads them; column info

void createStore(RunCtx &ctx, SequenceDB *db, Option *option)
{
    const int n = (int)db->sequences.size();
    std::vector<const char *> rows(n);
    std::vector<int32_t> lens(n);
    for (int i = 0; i < n; ++i) {
        auto *s = db->sequences[i];
        if (s->id != i) { std::cerr << "ERROR: sequence ids are not dense.\n"; exit(1); }
        rows[i] = s->alnStorage[s->storage];
        lens[i] = s->len;
    }
    ctx.storeDev = selectedDevices();
    if (option->testVirtualDevices > 0) ctx.storeDev.assign((size_t)option->testVirtualDevices, selectedDevices()[0]);
    ctx.stores.assign(ctx.storeDev.size(), nullptr);
    std::vector<std::thread> th;
    std::vector<std::pair<int, std::string>> res(ctx.storeDev.size(), {TWL_OK, ""});
    for (size_t d = 0; d < ctx.storeDev.size(); ++d)
        th.emplace_back([&, d] {
            const int rc = twl_store_create(ctx.storeDev[d], option->type, n, rows.data(), lens.data(), &ctx.stores[d]);
            if (rc != TWL_OK) res[d] = {rc, twl_last_error()};
        });
    for (auto &t : th) t.join();
    for (auto &r : res)
        if (r.first != TWL_OK) { std::cerr << "ERROR: twl_store_create failed (" << r.first << "): " << r.second << '\n'; exit(1); }
    if (ctx.onStoreCreated) {
        const std::function<void(twl_store *)> hook = std::move(ctx.onStoreCreated);
        ctx.onStoreCreated = nullptr;
        for (twl_store *st : ctx.stores) hook(st);
    }
}

// Runs fn(replica index) for every replica on its own host thread; stops the run on the first library error.
template <class F>
void onAllStores(RunCtx &ctx, const char *what, F fn)
{
    const size_t nd = ctx.stores.size();
    std::vector<std::pair<int, std::string>> res(nd, {TWL_OK, ""});
    if (nd == 1) { const int rc = fn(0); if (rc != TWL_OK) res[0] = {rc, twl_last_error()}; }
    else {
        std::vector<std::thread> th;
        for (size_t d = 0; d < nd; ++d)
            th.emplace_back([&, d] { const int rc = fn((int)d); if (rc != TWL_OK) res[d] = {rc, twl_last_error()}; });
        for (auto &t : th) t.join();
    }
    for (auto &r : res)
        if (r.first != TWL_OK) { std::cerr << "ERROR: " << what << " failed (" << r.first << "): " << r.second << '\n'; exit(1); }
}

// End of the main pass: current rows back into SequenceInfo::alnStorage, cached profiles of the nodes that go on (the root and the
// deferred nodes) back into Node::msaFreq, store released.
void materialise(Tree *T, SequenceDB *db, Option *option)
{
    RunCtx &ctx = ctxOf(db);
    if (!firstStore(ctx)) return;
    const double t0 = nowMs();
    const int n = (int)db->sequences.size();
    // A run whose output is trimmed (--trim-gappy, --trim-to): in the download that is the run's last the rows lose their columns here, on the
    // device, so that only kept columns come back -- unless the host still needs whole rows (--check reads them, a compressed group's members
    // wait for updateAlignment) or there are several replicas; the driver then trims an uploaded copy of the final rows.
    std::function<void()> trimmedRowsAreBack;
    if (db->trimRequested && db->lastDownload && option->trimResidentRows && ctx.stores.size() == 1 && !option->debug) {
        bool whole = true;
        for (const auto *s : db->sequences) whole = whole && s->subtreeIdx >= -1;
        if (whole) trimmedRowsAreBack = option->trimResidentRows(db, option, firstStore(ctx));
    }
    std::vector<int32_t> lens(n);
    int rc = twl_store_read_rows(firstStore(ctx), nullptr, lens.data());
    if (rc != TWL_OK) die("twl_store_read_rows", rc);
    // One block for all rows, laid out like the device's gathered buffer (row i at the prefix sum of the lengths), so the library
    // copies straight into it; the second half backs the sequences' other buffer (untouched until a later pass writes there).
    std::vector<char *> rows(n);
    size_t total = 0;
    for (int i = 0; i < n; ++i) total += (size_t)lens[i];
    free(db->rowArena);
    db->rowArena = static_cast<char *>(malloc(2 * total + 1));
    if (!db->rowArena) { std::cerr << "ERROR: out of host memory for the final rows.\n"; exit(1); }
    size_t at = 0;
    for (int i = 0; i < n; ++i) {
        auto *s = db->sequences[i];
        if (!s->borrowed) { free(s->alnStorage[0]); free(s->alnStorage[1]); }
        s->borrowed = true;
        s->alnStorage[s->storage] = db->rowArena + at;
        s->alnStorage[!s->storage] = db->rowArena + total + at;
        s->memLen = lens[i];
        rows[i] = s->alnStorage[s->storage];
        at += (size_t)lens[i];
    }
    rc = twl_store_read_rows(firstStore(ctx), rows.data(), lens.data());
    if (rc != TWL_OK) die("twl_store_read_rows", rc);
    for (int i = 0; i < n; ++i) db->sequences[i]->len = lens[i];
    if (trimmedRowsAreBack) trimmedRowsAreBack();
    const int P = (option->type == 'n') ? 6 : 22;
    std::vector<Node *> keep{T->root};
    keep.insert(keep.end(), db->fallback_nodes.begin(), db->fallback_nodes.end());
    for (Node *nd : keep) {
        if (nd->cacheId < 0) continue;
        int32_t len = 0;
        if ((rc = twl_store_read_cache(firstStore(ctx), nd->cacheId, nullptr, &len)) != TWL_OK) die("twl_store_read_cache", rc);
        std::vector<float> flat((size_t)len * P);
        if ((rc = twl_store_read_cache(firstStore(ctx), nd->cacheId, flat.data(), &len)) != TWL_OK) die("twl_store_read_cache", rc);
        nd->msaFreq.assign(len, std::vector<float>(P));
        for (int t = 0; t < len; ++t) std::copy(&flat[(size_t)t * P], &flat[(size_t)t * P] + P, nd->msaFreq[t].begin());
        nd->cacheId = -1;
    }
    for (twl_store *st : ctx.stores) twl_store_destroy(st);
    ctx.stores.clear();
    ctx.finished = true;
    if (option->printDetail) std::cerr << "Rows back on the host in " << nowMs() - t0 << " ms\n";
}

// How the paths of a level travel, from the shard and the replica count.  inPlace and devX hold for ONE replica only (nd == 1 in every
// term): twl_level_restore, the pairs it hands back and the HBM-to-HBM exchange never meet a second replica thread.
struct PathRoute { bool procs, devX, inPlace; };
PathRoute routeOf(const Shard &sh, int nd)
{
    PathRoute r;
    // One device, one process: the paths never leave HBM -- pairs that lost no column commit their DP path as it is, the others get their
    // columns back on the device (twl_level_restore); the column info comes to the host only for a pair the device hands back (below).
    r.procs = sh.world > 1;
    // ... and so it is with several processes when they can all-gather device blocks (Shard::exchangeDev): each rank restores its own
    // pairs on its device, the final paths travel HBM to HBM (exchangeFinalPaths below), every rank commits all of them from HBM.
    r.devX = (nd == 1 && (sh.exchangeDev != nullptr || sh.rccl));
    r.inPlace = (nd == 1 && ((!r.procs && !sh.exchange && !sh.rccl) || r.devX));
    return r;
}

// One level.  The steps below fill it in turn on the calling thread (each group of members names its step); the replica threads of
// alignShare get it const.  Steps that change the run or the nodes take RunCtx / NodePairVec as an argument of their own.
struct Level {
    const RunCtx &ctx;
    const NodePairVec &nodes;
    SequenceDB *database;
    Option *option;
    Params &param;
    int task, n, nd;                              // nd: device replicas of this process
    const char *letters;                          // consensus letter of a column-info code
    bool removal;
    PathRoute route;
    twl_params tp, tz;                            // tz: gapCharScore 0
    // describeLevel
    std::vector<twl_side> sides;
    std::vector<PairShape> ps;
    std::vector<int32_t> members;
    std::vector<float> weights;
    int stride = 1;                               // row pitch of the profiles: the longest side
    int pathStride = 1;                           // row pitch of the final paths: refLen + qryLen before removal bounds every path
    // prepareOnReplicas
    std::vector<int> needInfo;                    // pairs that lost a column
    std::vector<char> needsHost;                  // ... as a flag per pair
    // planDp
    std::vector<uint8_t> maskZero;                // pairs of the DP that take gapCharScore 0
    std::vector<char> takesPart;                  // pairs of the DP
    std::vector<int> owner;
    int meBase = 0;                               // replica d of this process aligns the pairs of owner meBase + d
    Level(const RunCtx &c, const NodePairVec &nv, SequenceDB *db, Option *o, Params &p)
        : ctx(c), nodes(nv), database(db), option(o), param(p), task(db->currentTask), n((int)nv.size()), nd((int)c.stores.size()),
          letters(consensusLetters(o->type)), removal(!(o->gappyVertical == 1.0)), route(routeOf(c.shard, nd)), tp(baseParams(p)), tz(tp)
    {
        tz.gap_char = 0;
    }
};

// What the DP and the steps after it leave per pair.  While the replicas run (alignShare), row i of paths / errs / fromDp / dpLen is
// written in place by the replica that owns pair i and by nobody else; before and after that only the calling thread touches the rows.
struct PairRows {
    std::vector<alnPath> paths;
    std::vector<int16_t> errs;
    std::vector<uint8_t> fromDp;                  // 1: the DP path is the final path; 2: twl_level_restore made the final path, in HBM
    std::vector<int32_t> dpLen;
    std::vector<ColumnInfo> cols;                 // calling thread only
    explicit PairRows(int n) : paths(n), errs(n, 0), fromDp(n, 0), dpLen(n, 0), cols(n) {}
};

// What one replica reports besides the rows of its pairs; merged into the level on the calling thread (mergeShares).
struct ReplicaShare {
    double callMs = 0, totMs = 0;
    LevelRecord part;                             // its cells, relaunched pairs, kernel time and kernel identity
    uint64_t nominalCells = 0;
    std::vector<int32_t> handedBack, handedBackLen;      // in-place mode: pairs twl_level_restore handed back to the host, and their DP path lengths
};

// ---- side descriptors (what calculateProfile reads from the two nodes, alignment-helper.cpp:8-40) ----
void describeLevel(Level &lv, RunCtx &ctx, NodePairVec &nodes)
{
    const int n = lv.n;
    SequenceDB *database = lv.database;
    Option *option = lv.option;
    std::vector<twl_side> &sides = lv.sides;
    sides.resize(2 * (size_t)n);
    lv.ps.resize(n);
    size_t nMembers = 0;
    // (what is read from the nodes and sequences of a pair -- cache misses, mostly -- in parallel; the running member offsets and the
    // ids of newly cached profiles, which depend on the order of the pairs, in a serial pass behind it)
#pragma omp parallel for schedule(static) if (n >= 512)
    for (int i = 0; i < n; ++i) {
        Node *nd[2] = {nodes[i].first, nodes[i].second};
        PairShape &s = lv.ps[i];
        s.refLen = nd[0]->getAlnLen(0); s.qryLen = nd[1]->getAlnLen(0);
        s.refNum = nd[0]->getAlnNum(0); s.qryNum = nd[1]->getAlnNum(0);
        for (int sd = 0; sd < 2; ++sd) {
            twl_side &x = sides[2 * (size_t)i + sd];
            x.n_members = (int32_t)nd[sd]->seqsIncluded.size();
            x.len = sd ? s.qryLen : s.refLen;
            x.num = sd ? s.qryNum : s.refNum;
            x.weight = nd[sd]->alnWeight;
            x.cache_id = nd[sd]->cacheId;
            x.store_id = -1;
            x.reserved = 0;
        }
        s.lowQ_r = lowQualitySide(option->alnMode == MERGE_MSA, s.refNum, firstSeqLowQuality(nd[0], database));
        s.lowQ_q = lowQualitySide(option->alnMode == MERGE_MSA, s.qryNum, firstSeqLowQuality(nd[1], database));
    }
    for (int i = 0; i < n; ++i) {
        const PairShape &s = lv.ps[i];
        Node *nd[2] = {nodes[i].first, nodes[i].second};
        const bool storeFreq = (s.refNum >= option->calProfileTh || s.qryNum >= option->calProfileTh) || (sides[2 * (size_t)i].cache_id >= 0 || sides[2 * (size_t)i + 1].cache_id >= 0);
        for (int sd = 0; sd < 2; ++sd) {
            twl_side &x = sides[2 * (size_t)i + sd];
            x.member_off = (int32_t)nMembers;
            if (storeFreq && x.cache_id < 0) x.store_id = nd[sd]->cacheId = ctx.nextCacheId++;
            nMembers += (size_t)x.n_members;
            lv.stride = std::max(lv.stride, x.len);
        }
        lv.pathStride = std::max(lv.pathStride, s.refLen + s.qryLen);
    }
    lv.members.resize(nMembers);
    lv.weights.resize(nMembers);
    // (levels of a few pairs stay on this thread: a parallel region of one iteration wakes every worker, and their spinning at its end
    // slowed the serial stretches that follow -- 1.3 ms against 0.3 ms for the 100 000 members of a top level)
#pragma omp parallel for schedule(dynamic, 16) if (n >= 64)
    for (int i = 0; i < n; ++i) {
        Node *nd[2] = {nodes[i].first, nodes[i].second};
        for (int sd = 0; sd < 2; ++sd) {
            const twl_side &x = sides[2 * (size_t)i + sd];
            const float groupWeight = nd[sd]->alnWeight;
            for (int m = 0; m < x.n_members; ++m) {
                const int sIdx = nd[sd]->seqsIncluded[m];
                if (sIdx < 0) { std::cerr << "ERROR: compressed sequence group in device-resident mode.\n"; exit(1); }
                lv.members[x.member_off + m] = sIdx;
                lv.weights[x.member_off + m] = database->sequences[sIdx]->weight / groupWeight * x.num;     // alignment-helper.cpp:27
            }
        }
    }
}

// ---- device: profiles, consensus, gappy-column removal, gap penalties ----
void prepareOnReplicas(Level &lv, RunCtx &ctx)
{
    const int n = lv.n;
    std::vector<int32_t> lens(2 * (size_t)n);
    std::vector<std::vector<int32_t>> lensOf(lv.nd);
    onAllStores(ctx, "twl_level_prepare", [&](int d) {
        lensOf[d].resize(2 * (size_t)n);       // every replica prepares the whole level; column info is fetched from the first only
        return twl_level_prepare(ctx.stores[d], &lv.tp, lv.option->gappyVertical, n, lv.sides.data(), lv.members.data(), lv.weights.data(), lv.stride,
                                 d == 0 ? lens.data() : lensOf[d].data(), nullptr);
    });
    for (int d = 1; d < lv.nd; ++d)
        if (lensOf[d] != lens) { std::cerr << "ERROR: device replicas disagree on the prepared level.\n"; exit(1); }
    // The column info (consensus letter + gappy flag per original column) only matters for addGappyColumnsBack, i.e. for pairs in
    // which some column was removed: fetch it for those (at the leaf level none: single sequences have no gap columns).
    lv.needsHost.assign(n, 0);
    for (int i = 0; i < n; ++i) {
        PairShape &s = lv.ps[i];
        s.lens = {lens[2 * i], lens[2 * i + 1]};
        if (s.lens.first != s.refLen || s.lens.second != s.qryLen) { lv.needInfo.push_back(i); lv.needsHost[i] = 1; }
    }
}

// Consensus + removed runs of the pairs `which` into cols, one synchronisation: the level's whole block (most pairs need it) or their
// blocks only.  Calling thread only: the stage is process-wide.
void fetchColumnInfo(const Level &lv, const std::vector<int> &which, bool wholeBlock, std::vector<ColumnInfo> &cols)
{
    if (which.empty()) return;
    const size_t stride = (size_t)lv.stride;
    uint8_t *info = reinterpret_cast<uint8_t *>(g_infoStage.get(2 * (wholeBlock ? (size_t)lv.n : which.size()) * stride));
    const int rc = wholeBlock ? twl_level_read_colinfo(firstStore(lv.ctx), -1, 0, info)
                              : twl_level_read_colinfo_many(firstStore(lv.ctx), (int32_t)which.size(), which.data(), info);
    if (rc != TWL_OK) die(wholeBlock ? "twl_level_read_colinfo" : "twl_level_read_colinfo_many", rc);
#pragma omp parallel for schedule(dynamic, 4)
    for (int t = 0; t < (int)which.size(); ++t) {
        const int i = which[t];
        const size_t slot = wholeBlock ? (size_t)i : (size_t)t;
        runsAndConsensus(&info[2 * slot * stride], lv.ps[i].refLen, lv.removal, lv.letters, cols[i].gappy.first, cols[i].consensus.first);
        runsAndConsensus(&info[(2 * slot + 1) * stride], lv.ps[i].qryLen, lv.removal, lv.letters, cols[i].gappy.second, cols[i].consensus.second);
    }
}

// ---- DP with the reference's grouping and retry/defer policy (level_policy.hpp) ----
void planDp(Level &lv, PairRows &rows)
{
    const int n = lv.n;
    lv.maskZero.assign(n, 0);
    lv.takesPart.assign(n, 0);
    std::vector<long long> cost(n, 0);
    for (int i = 0; i < n; ++i) {
        const PairShape &s = lv.ps[i];
        rows.paths[i] = trivialPath(s);
        cost[i] = (long long)s.lens.first + s.lens.second;
        if (!goesToDp(s)) continue;
        lv.takesPart[i] = 1;
        lv.maskZero[i] = zeroGapChar(lv.task, s) ? 1 : 0;
    }
    // deal the pairs, longest first (cost ~ R + Q after gappy-column removal), to the device replicas of this process or, with several
    // processes (one device each), to the ranks; everybody aligns its share
    lv.owner = dealPairs(cost, lv.takesPart, lv.route.procs ? lv.ctx.shard.world : lv.nd);
    lv.meBase = lv.route.procs ? lv.ctx.shard.rank : 0;
}

// The counters of the DP call replica d has just made, into its share.
void addStats(const Level &lv, int d, bool firstCall, ReplicaShare &mine)
{
    // per-device counters (virtual replicas share one device, whose counters describe the last call of any of them: left out)
    const bool ownDevice = lv.nd == 1 || lv.ctx.storeDev[d] != lv.ctx.storeDev[(d + 1) % lv.nd];
    const bool nominal = firstCall && d == 0;      // (R*Q of the level's pairs, once: the classic GCUPS figure of bench.py)
    twl_stats st{};
    if ((!ownDevice && !nominal) || twl_get_stats(lv.ctx.storeDev[d], &st) != TWL_OK) return;
    if (ownDevice) { foldStats(mine.part, st); mine.part.kernel_ms += st.kernel_ms; mine.totMs += st.total_ms; }
    if (nominal) mine.nominalCells += st.nominal_cells;
}

// In the deferred pass a failed pair is retried, by whoever owns it, with a larger X-drop / band limit until it passes.
int retryDeferredPair(const Level &lv, int d, const std::vector<uint8_t> &mask, int8_t *aln, std::vector<int32_t> &alnLen, std::vector<int16_t> &err, ReplicaShare &mine)
{
    // a retry is a call of the whole level with a one-pair mask, and a DP call zero-fills the outputs of ALL the level's pairs: with more
    // than one pair it would wipe what the others have just produced.  The deferred pass aligns one profile per level
    // (progressive.cpp:283-291); a task-1 level of several pairs is refused up front -- whether or not a pair fails -- rather than silently
    // wrong or dependent on the data (the limit is part of the contract: include/twl_msa.h)
    if (lv.n != 1) { std::cerr << "ERROR: a deferred-pass (task 1) level must hold exactly one pair; this one has " << lv.n << ".\n"; return (int)TWL_ERR_UNSUPPORTED; }
    if (!mask[0]) return (int)TWL_OK;
    twl_params tr = lv.maskZero[0] ? lv.tz : lv.tp;
    const uint8_t one = 1;
    int rc = TWL_OK;
    retryUntilPassed(tr, err[0], std::min(lv.ps[0].lens.first, lv.ps[0].lens.second), [&](const twl_params &grown) {
        if (lv.option->printDetail) std::cout << "Retry pair No. " << 0 << "\txdrop " << grown.xdrop << " flen " << grown.flen << '\n';
        const double tRetry = nowMs();
        rc = twl_level_align(lv.ctx.stores[d], &grown, &one, aln, alnLen.data(), err.data());
        if (rc != TWL_OK) return (int16_t)0;      // (ends the loop; the caller stops the run on rc)
        mine.callMs += nowMs() - tRetry;
        addStats(lv, d, false, mine);
        return err[0];
    });
    return rc;
}

// The results of replica d's pairs, sorted into: final in HBM as the DP wrote it / columns restored on the device / handed back to the host
// (in-place mode), or copied out of the replica's staging (otherwise).
int sortResults(const Level &lv, int d, const std::vector<uint8_t> &mask, const int8_t *aln, const std::vector<int32_t> &alnLen, const std::vector<int16_t> &err,
                PairRows &rows, ReplicaShare &mine)
{
    const size_t pitch = (size_t)2 * lv.stride;
    std::vector<int32_t> restore, restoreLen;
    for (int i = 0; i < lv.n; ++i) {
        if (!mask[i]) continue;
        rows.errs[i] = err[i];
        const int32_t len = (err[i] == 0) ? alnLen[i] : 0;
        if (!lv.route.inPlace) rows.paths[i].assign(&aln[i * pitch], &aln[i * pitch] + len);
        else if (lv.needsHost[i]) {
            // (a low-quality singleton is deferred in finalPathsOnHost: its path is dropped)
            if (len > 0 && !deferredLowQuality(lv.task, lv.ps[i])) { restore.push_back(i); restoreLen.push_back(len); } else rows.paths[i].clear();
        }
        else if (len > 0) { rows.fromDp[i] = 1; rows.dpLen[i] = len; }
    }
    if (restore.empty()) return (int)TWL_OK;
    std::vector<int32_t> fin(restore.size(), -1);      // gappy columns back on the device: these paths never leave HBM either
    const int rc = twl_level_restore(lv.ctx.stores[d], &lv.tp, (int32_t)restore.size(), restore.data(), lv.pathStride, fin.data());
    if (rc != TWL_OK) return rc;
    for (size_t t = 0; t < restore.size(); ++t) {
        if (fin[t] > 0) { rows.fromDp[restore[t]] = 2; rows.dpLen[restore[t]] = fin[t]; }
        else { mine.handedBack.push_back(restore[t]); mine.handedBackLen.push_back(restoreLen[t]); }      // a two-sided run too large for the device: on the host, as before
    }
    return (int)TWL_OK;
}

// The share of replica d, on its own thread: launch, deferred-pass retry, results into the rows of its pairs.
int alignShare(const Level &lv, int d, PairRows &rows, ReplicaShare &mine)
{
    // ONE launch for the pairs of both gap-character kinds (alignment-cpu.cpp:88 decides per pair; until round 4 one call per kind, which
    // doubled the latency of the top levels of a 100 000-leaf tree, where a few pairs of each kind meet)
    const int n = lv.n;
    std::vector<uint8_t> mask(n, 0);
    int cnt = 0, cntZero = 0;
    for (int i = 0; i < n; ++i) if (lv.takesPart[i] && lv.owner[i] == lv.meBase + d) { mask[i] = 1; ++cnt; cntZero += lv.maskZero[i]; }
    if (!cnt) return (int)TWL_OK;
    int8_t *aln = lv.route.inPlace ? nullptr : reinterpret_cast<int8_t *>(g_alnStage[d].get((size_t)n * 2 * lv.stride));
    std::vector<int32_t> alnLen(n);
    std::vector<int16_t> err(n);
    const double tCall = nowMs();
    const int rc = (cntZero == cnt) ? twl_level_align(lv.ctx.stores[d], &lv.tz, mask.data(), aln, alnLen.data(), err.data())
                                    : twl_level_align_mixed(lv.ctx.stores[d], &lv.tp, mask.data(), cntZero ? lv.maskZero.data() : nullptr, aln, alnLen.data(), err.data());
    if (rc != TWL_OK) return rc;
    mine.callMs += nowMs() - tCall;
    addStats(lv, d, true, mine);
    if (lv.task == 1) {
        const int rr = retryDeferredPair(lv, d, mask, aln, alnLen, err, mine);
        if (rr != TWL_OK) return rr;
    }
    return sortResults(lv, d, mask, aln, alnLen, err, rows, mine);
}

#ifdef TWL_DEV      // development builds: one line per pair for tools/sim_schedule.py
void dumpSchedule(const Level &lv, const PairRows &rows)
{
    const char *dump = getenv("TWL_DUMP_SCHEDULE");
    FILE *f = dump ? fopen(dump, "a") : nullptr;
    if (!f) return;
    std::vector<uint64_t> pc(lv.n, 0);
    if (lv.nd == 1) (void)twl_get_pair_cells(lv.ctx.storeDev[0], pc.data(), lv.n);
    for (int i = 0; i < lv.n; ++i)
        fprintf(f, "%d %d %d %d %d %d %d %llu\n", (int)lv.ctx.levels.size(), i, lv.nodes[i].first->seqsIncluded.empty() ? -1 : lv.nodes[i].first->seqsIncluded[0],
                lv.nodes[i].second->seqsIncluded.empty() ? -1 : lv.nodes[i].second->seqsIncluded[0], lv.ps[i].lens.first, lv.ps[i].lens.second, (int)rows.errs[i], (unsigned long long)pc[i]);
    fclose(f);
}
#endif

// The replicas ran concurrently: times combine by max, counts add up; the kernel's identity and the tile counts are replica 0's.
void mergeShares(const std::vector<ReplicaShare> &shares, RunCtx &ctx, LevelRecord &rec)
{
    double callMs = 0, totMs = 0;
    for (const ReplicaShare &s : shares) {
        callMs = std::max(callMs, s.callMs); totMs = std::max(totMs, s.totMs);
        rec.kernel_ms = std::max(rec.kernel_ms, s.part.kernel_ms);
        rec.band_cells += s.part.band_cells;
        rec.relaunched += s.part.relaunched;
    }
    const LevelRecord &p0 = shares[0].part;
    rec.matrix_mode = p0.matrix_mode; rec.speculative = p0.speculative; memcpy(rec.kernel, p0.kernel, sizeof rec.kernel);
    rec.mt_predicted += p0.mt_predicted; rec.mt_inline += p0.mt_inline;
    ctx.totals.call_ms += callMs;
    ctx.totals.total_ms += totMs;
    ctx.totals.nominal_cells += shares[0].nominalCells;
}

// what restoreOnHost made of pair i must cover both of its sides
void postCheck(const Level &lv, int i, int alnRef, int alnQry)
{
    const PairShape &s = lv.ps[i];
    if (alnRef != s.refLen) std::cout << "R: Post " << lv.nodes[i].first->identifier << "(" << alnRef << "/" << s.refLen << ")\n";
    if (alnQry != s.qryLen) std::cout << "Q: Post " << lv.nodes[i].second->identifier << "(" << alnQry << "/" << s.qryLen << ")\n";
}

// The pairs the device handed back: the host's result joins the others in HBM.  In-place mode only, hence one replica: share 0.
void joinHandedBack(const Level &lv, const ReplicaShare &share, PairRows &rows)
{
    const std::vector<int32_t> &fetch = share.handedBack;
    if (fetch.empty()) return;
    if (!lv.route.inPlace) { std::cerr << "ERROR: pairs handed back to the host outside the in-place mode.\n"; exit(1); }
    std::vector<int32_t> sideLen(2 * (size_t)lv.n);
    for (int i = 0; i < lv.n; ++i) { sideLen[2 * i] = lv.ps[i].refLen; sideLen[2 * i + 1] = lv.ps[i].qryLen; }
    const AlignedLevel al{lv.n, sideLen.data(), nullptr, nullptr, nullptr, lv.stride, lv.pathStride};
    const std::vector<int32_t> fin = restoreHandedBack(firstStore(lv.ctx), lv.param, *lv.option, al, fetch, share.handedBackLen,
                                                       [&](int i, int alnRef, int alnQry) { postCheck(lv, i, alnRef, alnQry); });
    for (size_t t = 0; t < fetch.size(); ++t) {
        rows.fromDp[fetch[t]] = 2; rows.dpLen[fetch[t]] = fin[t];
        rows.paths[fetch[t]].clear();
    }
}

// Several processes: everybody gets every path -- HBM to HBM when the ranks can all-gather device blocks, through the host otherwise.
void exchange(const Level &lv, RunCtx &ctx, PairRows &rows, LevelRecord &rec)
{
    if (!lv.route.devX) { exchangePaths(ctx, lv.owner, lv.takesPart, 2 * lv.stride, rows.paths, rows.errs, rec); return; }
    std::vector<int32_t> bound(lv.n);
    for (int i = 0; i < lv.n; ++i) bound[i] = lv.ps[i].refLen + lv.ps[i].qryLen;
    exchangeFinalPaths(ctx, firstStore(ctx), ctx.storeDev[0], lv.tp, lv.owner, lv.takesPart, bound, lv.pathStride, rows.fromDp, rows.dpLen, rows.errs, rec);
}

// A failed pair of the main pass is deferred; anywhere else it ends the run (the deferred pass retried until errorType 0).
std::vector<int> judgeFailures(const Level &lv, PairRows &rows)
{
    std::vector<int> fallbackPairs;
    for (int i = 0; i < lv.n; ++i) {
        if (!deferFailedPair(lv.task, rows.errs[i])) continue;
        rows.paths[i].clear();
        rows.fromDp[i] = 0;
        fallbackPairs.push_back(i);
    }
    return fallbackPairs;
}

// ---- gappy columns back for the paths that are on the host; returns the level's final-path block (row pitch pathStride) ----
int8_t *finalPathsOnHost(const Level &lv, PairRows &rows, std::vector<int32_t> &finalLen, std::vector<char> &deferred)
{
    const int n = lv.n, pathStride = lv.pathStride;
    int8_t *finalPaths = reinterpret_cast<int8_t *>(g_finalStage.get((size_t)n * pathStride));
    std::vector<int> onHost;                 // pairs whose final path the host still has to make (none in the in-place mode: their paths are in HBM)
    for (int i = 0; i < n; ++i) {
        deferred[i] = deferredLowQuality(lv.task, lv.ps[i]) ? 1 : 0;
        if (deferred[i]) { rows.paths[i].clear(); rows.fromDp[i] = 0; }
        if (rows.fromDp[i]) { finalLen[i] = rows.dpLen[i]; continue; }      // no column was removed: the DP path is the final path, and it is in HBM
        if (!rows.paths[i].empty()) onHost.push_back(i);
    }
#pragma omp parallel for schedule(dynamic, 1) if (onHost.size() > 1)
    for (int t = 0; t < (int)onHost.size(); ++t) {
        const int i = onHost[t];
        ColumnInfo &c = rows.cols[i];
        if (c.gappy.first.empty() && c.gappy.second.empty()) {      // nothing was removed: the DP path is the final path (addGappyColumnsBack would copy it)
            if ((int)rows.paths[i].size() > pathStride) { std::cerr << "ERROR: path longer than both profiles together.\n"; exit(1); }
            std::copy(rows.paths[i].begin(), rows.paths[i].end(), &finalPaths[(size_t)i * pathStride]);
            finalLen[i] = (int32_t)rows.paths[i].size();
            continue;
        }
        alnPath full;
        const IntPair covers = restoreOnHost(rows.paths[i], c, lv.param, pathStride, full);
        postCheck(lv, i, covers.first, covers.second);
        std::copy(full.begin(), full.end(), &finalPaths[(size_t)i * pathStride]);
        finalLen[i] = (int32_t)full.size();
    }
    return finalPaths;
}

// ---- the write-back on every replica, then the Node bookkeeping ----
void commitAndBookkeep(const Level &lv, RunCtx &ctx, NodePairVec &nodes, const int8_t *finalPaths, const std::vector<int32_t> &finalLen, const PairRows &rows)
{
    onAllStores(ctx, "twl_level_commit", [&](int d) { return twl_level_commit_from_dp(ctx.stores[d], finalPaths, finalLen.data(), lv.pathStride, lv.route.inPlace ? rows.fromDp.data() : nullptr); });
#pragma omp parallel for schedule(static) if (lv.n >= 512)
    for (int i = 0; i < lv.n; ++i) {            // Node bookkeeping of updateFrequency / updateAlignment (alignment-helper.cpp:474-478,536-538); the pairs of a level share no node
        if (finalLen[i] == 0) continue;
        Node *a = nodes[i].first, *b = nodes[i].second;
        if (a->cacheId >= 0 && b->cacheId >= 0) b->cacheId = -1;       // merged into a's cache by the commit
        a->alnNum += b->alnNum;
        a->alnLen = finalLen[i];
        a->alnWeight += b->alnWeight;
        a->seqsIncluded.insert(a->seqsIncluded.end(), b->seqsIncluded.begin(), b->seqsIncluded.end());
        b->seqsIncluded.clear();
    }
}

}  // namespace

const char *consensusLetters(char type)
{
    static const char bases[] = {'A', 'C', 'G', 'T', 'N'};
    static const char acids[] = {'A', 'C', 'D', 'E', 'F', 'G', 'H', 'I', 'K', 'L', 'M', 'N', 'P', 'Q', 'R', 'S', 'T', 'V', 'W', 'Y', 'X'};
    return type == 'n' ? bases : acids;
}

IntPair restoreOnHost(alnPath &dp, ColumnInfo &cols, Params &param, int pathStride, alnPath &full)
{
    auto covers = [](const alnPath &p) { IntPair c{0, 0}; for (auto a : p) { c.first += a != 1; c.second += a != 2; } return c; };
    alignment_helper::addGappyColumnsBack(dp, full, cols.gappy, param, covers(dp), cols.consensus);
    if ((int)full.size() > pathStride) { std::cerr << "ERROR: path longer than both profiles together.\n"; exit(1); }
    return covers(full);
}

std::vector<int32_t> restoreHandedBack(twl_store *st, Params &param, const Option &option, const AlignedLevel &lv, const std::vector<int32_t> &pairs,
                                       const std::vector<int32_t> &dpLen, const std::function<void(int, int, int)> &post)
{
    const size_t sl = (size_t)lv.stride, m = pairs.size();
    const bool removal = !(option.gappyVertical == 1.0f);
    const char *letters = consensusLetters(option.type);
    std::vector<uint8_t> info(m * 2 * sl);
    std::vector<int8_t> raw(m * 2 * sl);
    int rc = twl_level_read_colinfo_many(st, (int32_t)m, pairs.data(), info.data());
    if (rc != TWL_OK) die("twl_level_read_colinfo_many", rc);
    if ((rc = twl_level_read_paths(st, (int32_t)m, pairs.data(), dpLen.data(), raw.data(), (int32_t)(2 * sl))) != TWL_OK) die("twl_level_read_paths", rc);
    std::vector<int32_t> fin(m);
    for (size_t k = 0; k < m; ++k) {
        const int32_t i = pairs[k];
        ColumnInfo c;
        runsAndConsensus(&info[2 * k * sl], lv.sideLen[2 * i], removal, letters, c.gappy.first, c.consensus.first);
        runsAndConsensus(&info[(2 * k + 1) * sl], lv.sideLen[2 * i + 1], removal, letters, c.gappy.second, c.consensus.second);
        alnPath dp(&raw[2 * k * sl], &raw[2 * k * sl] + dpLen[k]), full;
        const IntPair covers = restoreOnHost(dp, c, param, lv.pathStride, full);
        if (post) post(i, covers.first, covers.second);
        if ((rc = twl_level_write_final(st, i, full.data(), (int32_t)full.size())) != TWL_OK) die("twl_level_write_final", rc);
        fin[k] = (int32_t)full.size();
    }
    return fin;
}

FinalPaths finalPathsOfLevel(twl_store *st, const twl_params &tp, Params &param, const Option &option, const AlignedLevel &lv)
{
    FinalPaths f;
    f.fromDp.assign((size_t)lv.n, 0);
    f.pathLen.assign((size_t)lv.n, 0);
    std::vector<int32_t> sel;                     // the pairs that lost a column; the others are final as the DP left them
    for (int32_t i = 0; i < lv.n; ++i) {
        if (lv.err[i] != 0) continue;
        f.pathLen[i] = lv.alnLen[i];
        f.fromDp[i] = 1;
        if (lv.lenOut[2 * i] < lv.sideLen[2 * i] || lv.lenOut[2 * i + 1] < lv.sideLen[2 * i + 1]) sel.push_back(i);
    }
    if (sel.empty()) return f;
    std::vector<int32_t> fin(sel.size(), -1), host, hostLen;
    const int rc = twl_level_restore(st, &tp, (int32_t)sel.size(), sel.data(), lv.pathStride, fin.data());
    if (rc != TWL_OK) die("twl_level_restore", rc);
    for (size_t k = 0; k < sel.size(); ++k) {
        f.fromDp[sel[k]] = 2;
        if (fin[k] > 0) f.pathLen[sel[k]] = fin[k];
        else { host.push_back(sel[k]); hostLen.push_back(lv.alnLen[sel[k]]); }
    }
    if (!host.empty()) {
        const std::vector<int32_t> full = restoreHandedBack(st, param, option, lv, host, hostLen);
        for (size_t k = 0; k < host.size(); ++k) f.pathLen[host[k]] = full[k];
        f.restoredOnHost = (int)host.size();
    }
    return f;
}

void alignWithRetry(twl_store *st, int device, const twl_params &prm, const Option &option, const std::string *retryWhat, const int16_t *knownErr, int32_t minLen,
                    int32_t *alnLen, int16_t *err, DpTotals &tot)
{
    auto runOnce = [&](const twl_params &p) {
        const int rc = twl_level_align(st, &p, nullptr, nullptr, alnLen, err);
        if (rc != TWL_OK) die("twl_level_align", rc);
        twl_stats ss{};
        if (twl_get_stats(device, &ss) == TWL_OK) { tot.cells += ss.band_cells; tot.kernel += ss.kernel_ms; }
        return err[0];
    };
    const int16_t first = knownErr ? *knownErr : runOnce(prm);
    if (!retryWhat) return;
    twl_params tr = prm;
    retryUntilPassed(tr, first, minLen, [&](const twl_params &grown) {
        ++tot.retries;
        if (option.printDetail) std::cout << "Retry " << *retryWhat << "\txdrop " << grown.xdrop << " flen " << grown.flen << '\n';
        return runOnce(grown);
    });
}

void runsAndConsensus(const uint8_t *info, int len, bool removal, const char *letters, IntPairVec &runs, std::string &cons)
{
    cons.resize(len);
    int start = -1;
    for (int t = 0; t < len; ++t) {
        cons[t] = letters[info[t] & 0x7f];
        if (!removal) continue;
        if (info[t] & 0x80) { if (start < 0) start = t; }
        else if (start >= 0) { runs.push_back({start, t - start}); start = -1; }
    }
    if (removal && start >= 0) runs.push_back({start, len - start});
}

void uploadSequences(SequenceDB *database, Option *option)
{
    RunCtx &ctx = ctxOf(database);
    if (firstStore(ctx) || ctx.finished) return;
    ensureInit(option);
    const double t0 = nowMs();
    createStore(ctx, database, option);
    // the rows live in HBM from here on; the host copies (two buffers per sequence) come back as one arena when something on the host
    // needs them (materialise): a resident run that waits for its turn holds names and lengths only
    for (auto *s : database->sequences) {
        if (!s->borrowed) { free(s->alnStorage[0]); free(s->alnStorage[1]); }
        s->alnStorage[0] = s->alnStorage[1] = nullptr;
        s->borrowed = true;
        s->memLen = 0;
    }
    if (option->printDetail) std::cerr << "Sequences resident on " << ctx.stores.size() << " device replica(s) in " << nowMs() - t0 << " ms\n";
    database->afterMainPass = [database, option](Tree *tree) { materialise(tree, database, option); };
    database->residentDeferred = true;      // the level kernel that set this up also takes the deferred pass with the rows in HBM
}

void downloadRows(SequenceDB *database, Tree *T)
{
    if (database->afterMainPass) { database->afterMainPass(T); database->afterMainPass = nullptr; }
}

void alignmentKernel_Resident(Tree *T, NodePairVec &nodes, SequenceDB *database, Option *option, Params &param)
{
    RunCtx &ctx = ctxOf(database);
    const int task = database->currentTask;
    if ((task != 0 && task != 1) || ctx.finished) {      // merging sub-alignments, or the rows are on the host already: host-staged kernel
        if (firstStore(ctx)) materialise(T, database, option);
        alignmentKernel_GPU(T, nodes, database, option, param);
        return;
    }
    refuseCpuOnly(option);
    ensureInit(option);
    uploadSequences(database, option);
    if (ctx.shard.world > 1 && ctx.stores.size() > 1) { std::cerr << "ERROR: several processes with several device replicas each are not supported.\n"; exit(1); }
    LevelRecord rec;
    rec.pairs = (int32_t)nodes.size();
    rec.task = task;
    const LevelTotals before = ctx.totals;
    const double tPrep = nowMs();
    const int n = (int)nodes.size(), nd = (int)ctx.stores.size();
    Level level(ctx, nodes, database, option, param);
    describeLevel(level, ctx, nodes);
    prepareOnReplicas(level, ctx);
    const Level &lv = level;
    PairRows rows(n);
    // the column info comes to the host up front unless the paths stay in HBM: most pairs -> one transfer of the level's block; a few -> their blocks only
    if (!lv.route.inPlace) fetchColumnInfo(lv, lv.needInfo, lv.needInfo.size() * 8 > (size_t)n, rows.cols);
    ctx.totals.prepare_ms += nowMs() - tPrep;

    planDp(level, rows);
    std::vector<ReplicaShare> shares(nd);
    if (g_alnStage.size() < (size_t)nd) g_alnStage.resize((size_t)nd);
    onAllStores(ctx, "twl_level_align", [&](int d) { return alignShare(lv, d, rows, shares[d]); });
#ifdef TWL_DEV
    dumpSchedule(lv, rows);
#endif
    mergeShares(shares, ctx, rec);
    joinHandedBack(lv, shares[0], rows);
    exchange(lv, ctx, rows, rec);
    std::vector<int> fallbackPairs = judgeFailures(lv, rows);

    const double tFin = nowMs();
    std::vector<int32_t> finalLen(n, 0);
    std::vector<char> deferred(n, 0);
    const int8_t *finalPaths = finalPathsOnHost(lv, rows, finalLen, deferred);
    const double tGappy = nowMs() - tFin;
    commitAndBookkeep(lv, ctx, nodes, finalPaths, finalLen, rows);
    ctx.totals.finish_ms += nowMs() - tFin;
    double devPrep = 0, devCommit = 0;
    if (option->printDetail) twl_level_timing(firstStore(ctx), &devPrep, &devCommit);      // (waits for the write-back kernels, which the next level would otherwise overlap with)
    ctx.totals.dev_prepare_ms += devPrep;
    ctx.totals.dev_commit_ms += devCommit;
    closeLevel(ctx, rec, tPrep, deferred, fallbackPairs, nodes, database, option);
    if (option->printDetail)
        std::cerr << "  phases (ms): prepare " << ctx.totals.prepare_ms - before.prepare_ms << " (device " << devPrep << ") call " << ctx.totals.call_ms - before.call_ms
                  << " (kernel " << rec.kernel_ms << ", exchange " << rec.exchange_ms << ") finish " << ctx.totals.finish_ms - before.finish_ms << " (device " << devCommit
                  << ") whole " << nowMs() - tPrep << "; relaunched pairs " << ctx.totals.relaunched - before.relaunched << "; pairs with removed columns " << lv.needInfo.size() << "; restored on the host " << shares[0].handedBack.size() << "; gappy columns back " << tGappy << " ms\n";
}

}  // namespace gpu
}  // namespace progressive
}  // namespace msa
