// twilight_amd/csrc/talco_team.hip.h -- the mailbox of the speculative tile start (the SPEC instantiations of talco_lean_kernel, talco_nuc.hip.h):
// two workgroups work on one pair and tell each other where tiles start through 8-byte words in global memory.
#pragma once
#include <hip/hip_runtime.h>

namespace twl {

// ---- speculative tile start (SPEC = true) ----
// A tile runs ~1450 diagonals: 1024 up to the marker and ~420 more until every surviving cell agrees on the cell of the marker
// diagonal all paths run through (TALCO-XDrop.cpp:585-612); the next tile starts there with scores at zero (:615-655, :77-106), so it
// depends on the POSITION of that cell only.  With fewer pairs than compute units, two workgroups work on one pair: they take the tiles
// in turn, and the one whose turn is next starts as soon as the other reaches its marker, from the best-scoring cell of the marker
// diagonals (the guess).  When the running tile has converged its workgroup publishes the true position: the partner carries on if the
// guess was right and restarts from the true position otherwise -- a wrong guess costs nothing but the idle workgroup's time, and
// the result is the same either way.  Mailbox words (global memory, one 8-byte agent-scope atomic each, tag = tile + 1):
//   guess[t & 3], truth[t & 3] = tag:16 | flags:16 | ref_idx:16 | qry_idx:16      pos[t & 3] = tag:16 | 0:16 | output offset:32
constexpr unsigned kTeamLast = 1u, kTeamErr = 2u;
constexpr int kTeamWords = 16, kTeamGuess = 0, kTeamTruth = 4, kTeamPos = 8, kTeamStat = 12;
__device__ __forceinline__ unsigned long long team_word(unsigned tag, unsigned flags, unsigned hi, unsigned lo)
{
    return ((unsigned long long)(tag & 0xFFFFu) << 48) | ((unsigned long long)(flags & 0xFFFFu) << 32) | ((unsigned long long)(hi & 0xFFFFu) << 16) | (lo & 0xFFFFu);
}
__device__ __forceinline__ unsigned long long team_load(const unsigned long long *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void team_store(unsigned long long *p, unsigned long long v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// one lane waits (bounded: ~2 s) until the word carries the tag; 0 = gave up: the partner is not co-resident or far too slow (a GPU
// shared with another process, a profiler serialising the workgroups).  That is a scheduling condition, not an alignment error: the
// caller reports the internal re-run code (kErrOverflow), the host re-runs the pair on the plain kernel of the next stage
__device__ __forceinline__ unsigned long long team_wait(const unsigned long long *p, unsigned tag, const unsigned long long *alt = nullptr)
{
    for (int spin = 0; spin < (1 << 21); ++spin) {
        const unsigned long long v = team_load(p);
        if ((unsigned)(v >> 48) == tag) return v;
        if (alt) { const unsigned long long u = team_load(alt); if ((unsigned)(u >> 48) == tag) return u | (1ull << 47); }      // bit 47: "this is the guess"
        __builtin_amdgcn_s_sleep(16);
    }
    return 0ull;
}
// order-preserving key of a score for an integer maximum (the guess only: never part of a result)
__device__ __forceinline__ unsigned score_key(float f)
{
    const unsigned b = (unsigned)__float_as_int(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

}  // namespace twl
