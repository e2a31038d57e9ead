// twilight_amd/csrc/host/exchange_plan.hpp -- the layout of the device blocks in which the ranks of a sharded run exchange a level's final
// paths (exchangeFinalPaths, align_gpu.cpp), stated once.  Pure functions over plain vectors: no Node, no store, no device call;
// tests/exchange_plan_kats.cpp includes this file alone and tests/exchange_cases.py restates it for the GPU tests.
//
// Block of rank r (every rank's block has blockMax bytes, rank r's lies at blockMax * r of the gathered buffer):
//   [0, 32)                      four 64-bit words: band cells, relaunched pairs, kernel ms (a double), magic | level number
//   [32, 32 + 8 * |mine[r]|)     {int32 length, int32 errorType} per pair of mine[r], in that order
//   [hdr[r], ...)                the paths of the pairs with length > 0, in that order, each starting at a multiple of 8 from hdr[r] on
// The bytes between a path's end and the next multiple of 8, and behind the last path, are not written.
#ifndef TWL_HOST_EXCHANGE_PLAN_HPP      // (a guard, not #pragma once: the header also compiles on its own, as a main file)
#define TWL_HOST_EXCHANGE_PLAN_HPP

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace msa {
namespace progressive {

constexpr uint64_t kPathBlockMagic = 0x54574C44ull << 32;      // "TWLD"
constexpr size_t kPathBlockHead = 32;

inline size_t pad8(size_t x) { return (x + 7) & ~(size_t)7; }

struct ExchangePlan {
    std::vector<std::vector<int>> mine;      // mine[r]: the pairs rank r owns that take part, ascending
    std::vector<size_t> hdr;                 // hdr[r]: bytes in front of rank r's first path
    size_t hdrMax = 0;                       // the longest header: what a receiver reads back of every block
    size_t blockMax = 0;                     // bytes of every rank's block: the largest header + padded bounds, rounded up to 256
};

// owner[i]: the rank that aligns pair i; takesPart[i]: pair i has a path on this level; bound[i]: the longest final path pair i can have
// (read only where takesPart[i]).  A pair that takes no part appears in no block.
inline ExchangePlan planExchange(const std::vector<int> &owner, const std::vector<char> &takesPart, const std::vector<int32_t> &bound, int world)
{
    ExchangePlan xp;
    xp.mine.resize((size_t)world);
    xp.hdr.resize((size_t)world);
    for (size_t i = 0; i < owner.size(); ++i) if (takesPart[i]) xp.mine[(size_t)owner[i]].push_back((int)i);
    for (int r = 0; r < world; ++r) {
        xp.hdr[r] = kPathBlockHead + 8 * xp.mine[r].size();
        size_t cap = xp.hdr[r];
        for (int i : xp.mine[r]) cap += pad8((size_t)bound[i]);
        xp.blockMax = std::max(xp.blockMax, cap); xp.hdrMax = std::max(xp.hdrMax, xp.hdr[r]);
    }
    xp.blockMax = (xp.blockMax + 255) & ~(size_t)255;
    return xp;
}

// Where the paths of rank r's pairs start in r's block once their lengths are known: off[t] for the t-th pair of mine[r], lens[t] its length
// (0: no path, it takes no room).  Returns the end of the last path's padded room; the caller holds it against blockMax.
inline size_t exchangeRowOffsets(const ExchangePlan &xp, int r, const std::vector<int32_t> &lens, std::vector<int64_t> &off)
{
    size_t at = xp.hdr[r];
    off.resize(lens.size());
    for (size_t t = 0; t < lens.size(); ++t) { off[t] = (int64_t)at; at += pad8((size_t)std::max(0, lens[t])); }
    return at;
}

// The header of rank r's block: the four words, then {length, errorType} of the t-th pair of mine[r].
inline std::vector<char> exchangeHeader(const ExchangePlan &xp, int r, uint64_t bandCells, uint64_t relaunched, double kernelMs, uint32_t level,
                                        const std::vector<int32_t> &lens, const std::vector<int32_t> &errs)
{
    std::vector<char> h(xp.hdr[r]);
    uint64_t h4[4] = {bandCells, relaunched, 0, kPathBlockMagic | (uint64_t)level};
    memcpy(&h4[2], &kernelMs, sizeof(double));
    memcpy(h.data(), h4, sizeof h4);
    for (size_t t = 0; t < lens.size(); ++t) { memcpy(&h[kPathBlockHead + 8 * t], &lens[t], 4); memcpy(&h[kPathBlockHead + 8 * t + 4], &errs[t], 4); }
    return h;
}

}  // namespace progressive
}  // namespace msa
#endif
