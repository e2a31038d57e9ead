// twilight_amd/csrc/host/strand_orient.hpp -- the host steps of `--adjust-direction` that need no device, as pure
// functions: the default number of seeds, the directions of the seeds from their same-strand and opposite-strand counts, and the reverse
// complement of a record's text.  tests/strand_kats.cpp includes this file directly; seqdb_io.cpp applies reverseComplement to the records
// of -i that the run found reversed.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace msa {
namespace strand {

// the smallest S with S * S >= 4 * total, clipped to [1, min(cap, 16384)]: `total` sequences in the set, `cap` of them may be seeds
inline int32_t defaultSeeds(int64_t total, int64_t cap)
{
    int64_t s = 1;
    while (s * s < 4 * total) ++s;
    if (s > cap) s = cap;
    if (s > 16384) s = 16384;
    if (s < 1) s = 1;
    return (int32_t)s;
}

// A link of the spanning tree: the outside seed joins the inside seed v on the same strand (kind 0) or on the opposite one (kind 1); its
// ratio is num / den.  before(a, b): the larger ratio (exactly: num, den < 2^29), then kind 0, then the smaller v.
struct Link { uint32_t num = 0, den = 1; int32_t kind = 0, v = 0; };
inline bool before(const Link &a, const Link &b)
{
    const uint64_t l = (uint64_t)a.num * b.den, r = (uint64_t)b.num * a.den;
    if (l != r) return l > r;
    if (a.kind != b.kind) return a.kind < b.kind;
    return a.v < b.v;
}

// flip[t] of the S seeds from F[u][v] = S(seed u, seed v) (w on the diagonal) and R[u][v] = O(seed u, seed v), both S x S row-major: seed 0 is
// forward; a maximum spanning tree is grown from it, Prim's way, the next link being the first in the order of before(), then the smaller
// outside seed u; flip[u] = flip[v] XOR kind.  One best link is kept per outside seed: S^2 steps.
inline std::vector<uint8_t> seedFlips(int32_t S, const uint32_t *F, const uint32_t *R)
{
    std::vector<uint8_t> flip((size_t)S, 0), inside((size_t)S, 0);
    std::vector<Link> best((size_t)S);
    auto link = [&](int32_t u, int32_t v, int32_t kind) {
        const uint32_t wu = F[(size_t)u * S + u], wv = F[(size_t)v * S + v], m = wu < wv ? wu : wv;
        Link k;
        k.kind = kind; k.v = v;
        if (m != 0) { k.num = (kind ? R : F)[(size_t)u * S + v]; k.den = m; }
        return k;
    };
    auto join = [&](int32_t v, bool first) {      // v goes inside: every outside seed sees its two links to v
        inside[(size_t)v] = 1;
        for (int32_t u = 0; u < S; ++u) {
            if (inside[(size_t)u]) continue;
            for (int32_t kind = 0; kind < 2; ++kind) {
                const Link k = link(u, v, kind);
                if ((first && kind == 0) || before(k, best[(size_t)u])) best[(size_t)u] = k;
            }
        }
    };
    if (S > 0) join(0, true);
    for (int32_t step = 1; step < S; ++step) {
        int32_t pick = -1;
        for (int32_t u = 0; u < S; ++u)
            if (!inside[(size_t)u] && (pick < 0 || before(best[(size_t)u], best[(size_t)pick]))) pick = u;
        flip[(size_t)pick] = (uint8_t)(flip[(size_t)best[(size_t)pick].v] ^ best[(size_t)pick].kind);
        join(pick, false);
    }
    return flip;
}

// The complement of a letter over the IUPAC table, case kept: A<->T, C<->G, R<->Y, K<->M, B<->V, D<->H; S, W, N and every other byte stay.
// rna: the record holds a U/u and no T/t; then A -> U and U -> A.
inline char complement(char c, bool rna)
{
    switch (c) {
    case 'A': return rna ? 'U' : 'T';   case 'a': return rna ? 'u' : 't';
    case 'T': return 'A';               case 't': return 'a';
    case 'U': return rna ? 'A' : 'U';   case 'u': return rna ? 'a' : 'u';
    case 'C': return 'G';               case 'c': return 'g';
    case 'G': return 'C';               case 'g': return 'c';
    case 'R': return 'Y';               case 'r': return 'y';
    case 'Y': return 'R';               case 'y': return 'r';
    case 'K': return 'M';               case 'k': return 'm';
    case 'M': return 'K';               case 'm': return 'k';
    case 'B': return 'V';               case 'b': return 'v';
    case 'V': return 'B';               case 'v': return 'b';
    case 'D': return 'H';               case 'd': return 'h';
    case 'H': return 'D';               case 'h': return 'd';
    default: return c;
    }
}

// the record's text reversed and complemented, in place
inline void reverseComplement(std::string &seq)
{
    bool hasU = false, hasT = false;
    for (char c : seq) { hasU |= (c == 'U' || c == 'u'); hasT |= (c == 'T' || c == 't'); }
    const bool rna = hasU && !hasT;
    const size_t n = seq.size();
    for (size_t i = 0; i < n / 2; ++i) {
        const char a = complement(seq[i], rna), b = complement(seq[n - 1 - i], rna);
        seq[i] = b; seq[n - 1 - i] = a;
    }
    if (n & 1) seq[n / 2] = complement(seq[n / 2], rna);
}

}  // namespace strand
}  // namespace msa
