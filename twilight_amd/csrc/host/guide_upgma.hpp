// twilight_amd/csrc/host/guide_upgma.hpp -- the clustering and the text of the guide tree that guide.cpp builds, as pure
// functions of a distance matrix: no device, no file.  tests/guide_kats.cpp includes this file directly.
//
// UPGMA (average linkage) as the naive algorithm defines it:
//   clusters start as the sequences in input order, slots 0 .. N-1, size 1, height 0; N-1 times: among the live slots the pair a < b with
//   the smallest d(a, b), ties to the smaller a, then the smaller b; the new cluster takes slot a, slot b dies; height d(a, b) / 2, size
//   n_a + n_b; for every other live c   d(a, c) = (n_a * d(a, c) + n_b * d(b, c)) / (n_a + n_b)   in double, evaluated as written.
// What is cached here (every row's smallest entry) changes the cost, not the tree: a row is searched again whenever its cached entry
// died or changed, and a changed entry replaces the cached one only when it is smaller, or equal with a smaller column.
// The translation unit that includes this file is built with -ffp-contract=off: a fused n_a * d + n_b * d changes the ties.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

namespace msa {
namespace guide {

// The upper triangle of a symmetric N x N matrix, row by row: entry (a, b), a < b.
struct Triangle {
    int n = 0;
    std::vector<double> v;
    explicit Triangle(int n_) : n(n_), v((size_t)n_ * (size_t)(n_ > 0 ? n_ - 1 : 0) / 2) {}
    size_t rowStart(int a) const { return (size_t)a * (size_t)(n - 1) - (size_t)a * (size_t)(a > 0 ? a - 1 : 0) / 2; }
    double &at(int a, int b) { return v[rowStart(a) + (size_t)(b - a - 1)]; }
    double &sym(int a, int b) { return a < b ? at(a, b) : at(b, a); }
};

// d(i, j) = 1 - S(i, j) / min(w_i, w_j) in double, 1 where the smaller w is 0; shared: N x N with w on the diagonal
inline Triangle distances(int n, const uint32_t *shared)
{
    Triangle d(n);
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 16) if (n >= 2048)
#endif
    for (int a = 0; a < n; ++a) {
        const uint32_t wa = shared[(size_t)a * n + a];
        for (int b = a + 1; b < n; ++b) {
            const uint32_t wb = shared[(size_t)b * n + b], m = wa < wb ? wa : wb;
            d.at(a, b) = m == 0 ? 1.0 : 1.0 - (double)shared[(size_t)a * n + b] / (double)m;
        }
    }
    return d;
}

// d(i, j) = 1 - match(i, j) / both(i, j) in double, 1 where both is 0; match, both: N x N
inline Triangle distancesFromCounts(int n, const uint32_t *match, const uint32_t *both)
{
    Triangle d(n);
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 16) if (n >= 2048)
#endif
    for (int a = 0; a < n; ++a)
        for (int b = a + 1; b < n; ++b) {
            const uint32_t m = match[(size_t)a * n + b], c = both[(size_t)a * n + b];
            d.at(a, b) = c == 0 ? 1.0 : 1.0 - (double)m / (double)c;
        }
    return d;
}

struct Merge { int left, right; double height; };      // nodes: leaves 0 .. N-1, the cluster of step s is N + s

// The N-1 merges of the definition above, in order.  d is consumed.
inline std::vector<Merge> upgma(Triangle &d)
{
    const int n = d.n;
    std::vector<Merge> merges;
    if (n < 2) return merges;
    std::vector<char> live((size_t)n, 1);
    std::vector<int> size((size_t)n, 1), node((size_t)n), nn((size_t)n, -1);
    std::vector<double> mv((size_t)n, 0.0);
    for (int i = 0; i < n; ++i) node[i] = i;
    auto rescan = [&](int c) {      // the smallest live entry of row c, the smallest column among equals
        nn[c] = -1;
        const size_t base = d.rowStart(c);      // d(c, x) = v[base + x - c - 1], x > c
        for (int x = c + 1; x < n; ++x) {
            const double v = d.v[base + (size_t)(x - c - 1)];
            if (live[x] && (nn[c] < 0 || v < mv[c])) { nn[c] = x; mv[c] = v; }
        }
    };
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 64) if (n >= 2048)
#endif
    for (int c = 0; c < n; ++c) rescan(c);
    for (int step = 0; step < n - 1; ++step) {
        int a = -1;
        for (int c = 0; c < n; ++c)
            if (live[c] && nn[c] >= 0 && (a < 0 || mv[c] < mv[a])) a = c;
        const int b = nn[a];
        const double dab = mv[a], na = (double)size[a], nb = (double)size[b];
        merges.push_back(Merge{node[a], node[b], dab / 2});
        live[b] = 0;
        // every iteration touches the entries (a, c) / (c, a) and the cache of row c alone, and reads column / row b, which nobody writes
#ifdef _OPENMP
#pragma omp parallel for schedule(static) if (n >= 2048)
#endif
        for (int c = 0; c < n; ++c) {
            if (!live[c] || c == a) continue;
            double &dac = d.sym(a, c);
            const double nd = (na * dac + nb * d.sym(b, c)) / (na + nb);
            dac = nd;
            if (c < a) {                      // row c holds column a (changed) and column b (dead)
                if (nn[c] == a || nn[c] == b) rescan(c);
                else if (nd < mv[c] || (nd == mv[c] && a < nn[c])) { nn[c] = a; mv[c] = nd; }
            } else if (c < b && nn[c] == b) rescan(c);      // row c holds column b (dead); a row behind b holds neither
        }
        size[a] += size[b];
        node[a] = n + step;
        rescan(a);
    }
    return merges;
}

// Recursive (X:lx,Y:ly) with X the cluster that held slot a: a leaf is its name, a branch length is the parent's height less the child's
// as %.6f (a negative one as 0.000000); no names on internal nodes, no root length; ';' and a newline at the end.
inline std::string newick(const std::vector<std::string> &names, const std::vector<Merge> &merges)
{
    const int n = (int)names.size();
    std::string out;
    if (n == 1) return names[0] + ";\n";
    auto height = [&](int v) { return v < n ? 0.0 : merges[(size_t)(v - n)].height; };
    struct Frame { int v, parent, state; };      // state 0: open, 1: between the children, 2: close
    std::vector<Frame> stack{{n + (int)merges.size() - 1, -1, 0}};
    char num[64];
    while (!stack.empty()) {
        Frame &f = stack.back();
        if (f.v < n) out += names[(size_t)f.v];
        else if (f.state == 0) { out += '('; f.state = 1; stack.push_back(Frame{merges[(size_t)(f.v - n)].left, f.v, 0}); continue; }
        else if (f.state == 1) { out += ','; f.state = 2; stack.push_back(Frame{merges[(size_t)(f.v - n)].right, f.v, 0}); continue; }
        else out += ')';
        if (f.parent >= 0) {
            double len = height(f.parent) - height(f.v);
            if (len < 0) len = 0.0;
            snprintf(num, sizeof num, ":%.6f", len);
            out += num;
        }
        stack.pop_back();
    }
    out += ";\n";
    return out;
}

}  // namespace guide
}  // namespace msa
