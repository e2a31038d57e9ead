// twilight_amd/csrc/host/level_policy.hpp -- the level policy of cpu::alignmentKernel_CPU (reference src/alignment-cpu.cpp:88-144),
// stated once: which pairs of a level go to the DP, with which gap-character score, what happens to a pair whose DP failed and which
// pairs are deferred whatever the DP said.  Pure functions over plain structs: no Node, no SequenceDB, no device call; the only output is
// the message before the exit of bugExit().  The level kernels (align_gpu.cpp, align_resident.cpp), the placement (place.cpp) and
// preparePair / finishPair (helpers.cpp) call these; tests/host_kats.cpp checks them against answers worked out from the reference.
#ifndef TWL_HOST_LEVEL_POLICY_HPP      // (a guard, not #pragma once: the header also compiles on its own, as a main file)
#define TWL_HOST_LEVEL_POLICY_HPP
#include "../../../include/twl_align.h"

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <iostream>
#include <utility>
#include <vector>

namespace msa {
namespace progressive {

// What the policy reads of one pair (alignment-cpu.cpp:50-66,91-92).
struct PairShape {
    int32_t refLen = 0, qryLen = 0, refNum = 0, qryNum = 0;      // columns and sequences of the two sides
    std::pair<int, int> lens{0, 0};                              // columns after gappy-column removal
    bool lowQ_r = false, lowQ_q = false;
};

// :91-92  a side is low-quality when it is a single sequence that was flagged on reading; never when sub-alignments are merged
inline bool lowQualitySide(bool mergeMsa, int32_t num, bool firstSeqLowQuality) { return mergeMsa ? false : (num > 1 ? false : firstSeqLowQuality); }

// :89-90  an empty side: the path is all gaps (1 = query only, 2 = reference only), no DP.  Empty when both sides have columns.
inline std::vector<int8_t> trivialPath(const PairShape &s)
{
    std::vector<int8_t> path;
    if (s.refLen == 0) path.assign((size_t)s.qryLen, 1);
    if (s.qryLen == 0) path.insert(path.end(), (size_t)s.refLen, 2);
    return path;
}

// :93,95  the DP runs while the path is empty (two empty sides leave it empty too), and only for sides that are not low-quality
inline bool goesToDp(const PairShape &s)
{
    const bool allGaps = (s.refLen == 0 && s.qryLen > 0) || (s.qryLen == 0 && s.refLen > 0);
    return !allGaps && !s.lowQ_r && !s.lowQ_q;
}

// :88  gapCharScore is 0 in the tasks after the main pass and for a side of more than 10000 sequences
inline bool zeroGapChar(int task, const PairShape &s) { return task != 0 || s.refNum > 10000 || s.qryNum > 10000; }

// :136-144  in the main pass a pair with a single-sequence side and a low-quality side is deferred whatever the DP said
inline bool deferredLowQuality(int task, const PairShape &s) { return task == 0 && (s.refNum == 1 || s.qryNum == 1) && (s.lowQ_r || s.lowQ_q); }

// :121-124  errorType 3, or a failure the policy has no answer to
[[noreturn]] inline void bugExit()
{
    std::cout << "There might be some bugs in the code!\n";
    exit(1);
}

// :108-115  a pair whose DP ended with errorType err: the main pass defers it; the later tasks retry until errorType 0 (below), so a
// failure that is left there ends the run, as errorType 3 does in every task (the level kernels judge after the retries; the reference
// would defer an errorType 3 of the main pass, which the DP here never reports there)
enum class FailedPair { Pass, Defer, Fatal };
inline FailedPair failedPairVerdict(int task, int16_t err)
{
    if (err == 0) return FailedPair::Pass;
    return (err == 3 || task != 0) ? FailedPair::Fatal : FailedPair::Defer;
}
// true: defer the pair; false: it passed; does not return for a fatal one
inline bool deferFailedPair(int task, int16_t err)
{
    const FailedPair v = failedPairVerdict(task, err);
    if (v == FailedPair::Fatal) bugExit();
    return v == FailedPair::Defer;
}

// :116-129 (tasks other than 0 retry a failed pair until it passes): the X-drop and band limit of the next attempt after a DP that ended
// with errorType err (1: xdrop doubles, 2: the band limit grows), minLen = the shorter side after gappy-column removal.
// errorType 3 ends the run, as it does there.
inline void nextRetryParams(int16_t err, int32_t minLen, twl_params &tr)
{
    if (err == 3) bugExit();
    if (err == 2) tr.flen = std::min(static_cast<int32_t>(tr.flen * 1.2) << 1, minLen);
    else { tr.xdrop = static_cast<int32_t>(tr.xdrop * 2); tr.flen = std::min(static_cast<int32_t>(tr.xdrop * 4) << 1, minLen); }
}

// :95-129  the retry loop: runOnce(tr) performs one DP attempt with the grown parameters and returns its errorType
template <class RunOnce>
void retryUntilPassed(twl_params &tr, int16_t err, int32_t minLen, RunOnce runOnce)
{
    while (err != 0) {
        nextRetryParams(err, minLen, tr);
        err = runOnce(tr);
    }
}

// Longest-processing-time deal of a level's pairs to `parts` owners (deterministic: every rank computes the same answer).
inline std::vector<int> dealPairs(const std::vector<long long> &cost, const std::vector<char> &takesPart, int parts)
{
    const int n = (int)cost.size();
    std::vector<int> owner(n, 0);
    if (parts <= 1) return owner;
    std::vector<int> order;
    for (int i = 0; i < n; ++i) if (takesPart[i]) order.push_back(i);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return cost[x] > cost[y]; });
    std::vector<long long> load(parts, 0);
    for (int i : order) {
        const int d = (int)(std::min_element(load.begin(), load.end()) - load.begin());
        owner[i] = d;
        load[d] += std::max<long long>(cost[i], 1);
    }
    return owner;
}

}  // namespace progressive
}  // namespace msa

#endif
