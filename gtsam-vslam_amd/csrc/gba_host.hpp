// Host-only part of vslam_global_ba (no HIP: tests/native/gba_host.cpp builds it alone under the sanitizers).  From the
// flattened problem's index arrays it derives, before anything is launched:
//   presence    a landmark is PRESENT iff it has at least two factors (set bits 0 / 1 of its pairs' flags); the others are thin
//   free set    a keyframe is FREE iff it is not fixed and has a factor on a present landmark or an edge; other non-fixed
//               keyframes are isolated
//   block graph two free keyframes are neighbours iff they share a present landmark or an edge; a component that neither a
//               present landmark shared with a fixed keyframe nor an edge to one ties down is a free gauge (refused)
//   reordering  reverse Cuthill-McKee of that graph (pgo_order_host.hpp): pos[keyframe] = block column, b = half-bandwidth
//   lists (CSR) lmStart / lmPairs: a present landmark's pairs that carry a factor, ascending pair index
//               rowStart / inc: a column's edges (edge << 1 | side), ascending edge index - the pose-graph solve's incidence
//               blkC / blkD / blkStart / list: per structurally non-zero block (c + d, c) of the band that a shared landmark
//               fills, the (pair on c + d, pair on c) entries in ascending landmark index (then ascending pair indices); the
//               diagonal block of a column holds every ordered combination of the column's pairs on one landmark
// Limits are checked before the array they bound is sized.
#pragma once
#include "pgo_order_host.hpp"
#include <cstdio>
#include <cstdlib>
#include <string>

namespace vslam {

constexpr int GBA_MAX_KF = 16384, GBA_MAX_EDGES = 262144, GBA_MAX_BLOCKS = 262144;     // the pose-graph call's limits
constexpr int GBA_MAX_PAIRS = 2097152, GBA_MAX_LM = 1048576;
constexpr long long GBA_MAX_LIST = 16777216;                                          // summed length of the block lists
enum { GBA_HOST_OK = 0, GBA_HOST_INVALID = 1, GBA_HOST_CAPACITY = 4 };               // (the values of vslam_status)

struct GbaIndex {           // the index arrays of a problem; edge ends as two arrays
    int n_kf = 0; const uint8_t* kf_fixed = nullptr;
    int n_lm = 0;
    int n_pairs = 0; const int32_t* pair_kf = nullptr; const int32_t* pair_lm = nullptr; const uint8_t* pair_flags = nullptr;
    int n_edges = 0; const int32_t* edge_i = nullptr; const int32_t* edge_j = nullptr;
};

struct GbaPlan {
    int nf = 0, nIso = 0, nPresent = 0, nThin = 0, nFactors = 0, b = 0, nBlk = 0;
    std::vector<uint8_t> lmPresent;                 // [n_lm]
    std::vector<int> pos;                           // [n_kf]: block column or -1
    std::vector<int> lmStart, lmPairs;              // [n_lm + 1], pairs
    std::vector<int> rowStart, inc;                 // [nf + 1], edge << 1 | side
    std::vector<int> blkC, blkD, blkStart, list;    // [nBlk], [nBlk], [nBlk + 1], 2 ints per entry (row pair, column pair)
    std::string err;
};

inline int gba_fail(GbaPlan& G, int status, const char* fmt, long long a = 0, long long b = 0, long long c = 0) {
    char buf[256];
    snprintf(buf, sizeof buf, fmt, a, b, c);
    G.err = buf;
    return status;
}

inline int gba_check_sizes(const GbaIndex& I, GbaPlan& G) {
    if (I.n_kf < 1 || I.n_lm < 0 || I.n_pairs < 0 || I.n_edges < 0 || !I.kf_fixed || (I.n_pairs > 0 && (!I.pair_kf || !I.pair_lm || !I.pair_flags)) ||
        (I.n_edges > 0 && (!I.edge_i || !I.edge_j)))
        return gba_fail(G, GBA_HOST_INVALID, "invalid arguments");
    if (I.n_kf > GBA_MAX_KF || I.n_edges > GBA_MAX_EDGES)
        return gba_fail(G, GBA_HOST_CAPACITY, "%lld keyframes / %lld edges exceed the limits (16384 / 262144)", I.n_kf, I.n_edges);
    if (I.n_pairs > GBA_MAX_PAIRS || I.n_lm > GBA_MAX_LM)
        return gba_fail(G, GBA_HOST_CAPACITY, "%lld pairs / %lld landmarks exceed the limits (2097152 / 1048576)", I.n_pairs, I.n_lm);
    return GBA_HOST_OK;
}

inline int gba_plan(const GbaIndex& I, GbaPlan& G) {
    G = GbaPlan{};
    if (const int st = gba_check_sizes(I, G)) return st;
    const int K = I.n_kf, L = I.n_lm, P = I.n_pairs, M = I.n_edges;
    for (int p = 0; p < P; p++)
        if (I.pair_kf[p] < 0 || I.pair_kf[p] >= K || I.pair_lm[p] < 0 || I.pair_lm[p] >= L)
            return gba_fail(G, GBA_HOST_INVALID, "pair %lld names keyframe %lld / landmark %lld", p, I.pair_kf[p], I.pair_lm[p]);
    for (int e = 0; e < M; e++)
        if (I.edge_i[e] < 0 || I.edge_j[e] < 0 || I.edge_i[e] >= K || I.edge_j[e] >= K || I.edge_i[e] == I.edge_j[e])
            return gba_fail(G, GBA_HOST_INVALID, "edge %lld joins keyframes %lld and %lld", e, I.edge_i[e], I.edge_j[e]);
    auto nfac = [&](int p) { return (I.pair_flags[p] & 1) + ((I.pair_flags[p] >> 1) & 1); };
    // presence
    std::vector<int> fac(L, 0);
    for (int p = 0; p < P; p++) fac[I.pair_lm[p]] += nfac(p);
    G.lmPresent.assign(L, 0);
    for (int l = 0; l < L; l++) { G.lmPresent[l] = fac[l] >= 2; if (fac[l] >= 2) { G.nPresent++; G.nFactors += fac[l]; } else G.nThin++; }
    // a present landmark's pairs
    G.lmStart.assign(L + 1, 0);
    for (int p = 0; p < P; p++) if (nfac(p) && G.lmPresent[I.pair_lm[p]]) G.lmStart[I.pair_lm[p] + 1]++;
    for (int l = 0; l < L; l++) G.lmStart[l + 1] += G.lmStart[l];
    G.lmPairs.assign(std::max(G.lmStart[L], 1), 0);
    {
        std::vector<int> fill(G.lmStart.begin(), G.lmStart.end() - 1);
        for (int p = 0; p < P; p++) if (nfac(p) && G.lmPresent[I.pair_lm[p]]) G.lmPairs[fill[I.pair_lm[p]]++] = p;
    }
    // the free set, numbered in ascending keyframe index
    std::vector<uint8_t> tied(K, 0);
    for (int k = 0; k < G.lmStart[L]; k++) tied[I.pair_kf[G.lmPairs[k]]] = 1;
    for (int e = 0; e < M; e++) tied[I.edge_i[e]] = tied[I.edge_j[e]] = 1;
    std::vector<int> fidx(K, -1), fkf;
    for (int k = 0; k < K; k++) {
        if (I.kf_fixed[k]) continue;
        if (!tied[k]) { G.nIso++; continue; }
        fidx[k] = (int)fkf.size(); fkf.push_back(k);
    }
    const int nf = (int)fkf.size();
    // the block lists' summed length, before the adjacency (of the same size) is built
    long long nList = 0;
    for (int l = 0; l < L; l++) {
        long long k = 0;
        for (int q = G.lmStart[l]; q < G.lmStart[l + 1]; q++) k += fidx[I.pair_kf[G.lmPairs[q]]] >= 0;
        nList += k * k;         // (an upper bound, k (k + 1) / 2 on distinct keyframes; reached when all of them sit on one keyframe)
        if (nList > GBA_MAX_LIST) return gba_fail(G, GBA_HOST_CAPACITY, "the block lists need more than %lld entries (reached at landmark %lld)", GBA_MAX_LIST, l);
    }
    std::vector<std::vector<int>> adj(nf);
    std::vector<uint8_t> anchored(nf, 0);
    std::vector<int> fs;
    for (int l = 0; l < L; l++) {
        fs.clear();
        bool fixedSeen = false;
        for (int q = G.lmStart[l]; q < G.lmStart[l + 1]; q++) {
            const int kf = I.pair_kf[G.lmPairs[q]];
            if (fidx[kf] >= 0) fs.push_back(fidx[kf]); else if (I.kf_fixed[kf]) fixedSeen = true;
        }
        for (size_t a = 0; a < fs.size(); a++) {
            if (fixedSeen) anchored[fs[a]] = 1;
            for (size_t c = 0; c < fs.size(); c++) if (fs[a] != fs[c]) adj[fs[a]].push_back(fs[c]);
        }
    }
    for (int e = 0; e < M; e++) {
        const int a = fidx[I.edge_i[e]], c = fidx[I.edge_j[e]];
        if (a >= 0 && c >= 0) { adj[a].push_back(c); adj[c].push_back(a); }
        else if (a >= 0) anchored[a] = 1;
        else if (c >= 0) anchored[c] = 1;
    }
    for (auto& v : adj) { std::sort(v.begin(), v.end()); v.erase(std::unique(v.begin(), v.end()), v.end()); }
    {   // every component of free keyframes needs a tie to a fixed one
        std::vector<uint8_t> seen(nf, 0);
        std::vector<int> comp;
        for (int s0 = 0; s0 < nf; s0++) {
            if (seen[s0]) continue;
            comp.clear(); comp.push_back(s0); seen[s0] = 1;
            bool anc = false;
            for (size_t h = 0; h < comp.size(); h++) {
                anc = anc || anchored[comp[h]];
                for (int v : adj[comp[h]]) if (!seen[v]) { seen[v] = 1; comp.push_back(v); }
            }
            if (!anc) return gba_fail(G, GBA_HOST_INVALID, "the free keyframes connected to keyframe %lld share no landmark and no edge with a fixed keyframe (free gauge)", fkf[s0]);
        }
    }
    std::vector<int> order;
    pgo_rcm(nf, adj, order);
    G.pos.assign(K, -1);
    for (int c = 0; c < nf; c++) G.pos[fkf[order[c]]] = c;
    int b = 0;
    for (int a = 0; a < nf; a++) for (int c : adj[a]) b = std::max(b, std::abs(G.pos[fkf[a]] - G.pos[fkf[c]]));
    if ((long long)(b + 1) * nf > GBA_MAX_BLOCKS) return gba_fail(G, GBA_HOST_CAPACITY, "the band needs %lld blocks (limit %lld)", (long long)(b + 1) * nf, GBA_MAX_BLOCKS);
    G.nf = nf; G.b = b;
    // the edges' incidence lists by column, ascending edge index
    const std::vector<int>& pos = G.pos;
    G.rowStart.assign(nf + 1, 0);
    for (int e = 0; e < M; e++) { if (pos[I.edge_i[e]] >= 0) G.rowStart[pos[I.edge_i[e]] + 1]++; if (pos[I.edge_j[e]] >= 0) G.rowStart[pos[I.edge_j[e]] + 1]++; }
    for (int c = 0; c < nf; c++) G.rowStart[c + 1] += G.rowStart[c];
    G.inc.assign(std::max(G.rowStart[nf], 1), 0);
    {
        std::vector<int> fill(G.rowStart.begin(), G.rowStart.end() - 1);
        for (int e = 0; e < M; e++) {
            if (pos[I.edge_i[e]] >= 0) G.inc[fill[pos[I.edge_i[e]]]++] = e << 1;
            if (pos[I.edge_j[e]] >= 0) G.inc[fill[pos[I.edge_j[e]]]++] = e << 1 | 1;
        }
    }
    // the landmarks' block lists: count per band slot, number the non-empty slots by (column, offset), fill in landmark order
    std::vector<int> slot((size_t)(b + 1) * std::max(nf, 1), 0);
    auto each_entry = [&](auto&& fn) {
        for (int l = 0; l < L; l++)
            for (int q1 = G.lmStart[l]; q1 < G.lmStart[l + 1]; q1++) {
                const int p1 = G.lmPairs[q1], r = pos[I.pair_kf[p1]];
                if (r < 0) continue;
                for (int q2 = G.lmStart[l]; q2 < G.lmStart[l + 1]; q2++) {
                    const int p2 = G.lmPairs[q2], c = pos[I.pair_kf[p2]];
                    if (c < 0 || c > r) continue;
                    fn((size_t)c * (b + 1) + (r - c), p1, p2);
                }
            }
    };
    each_entry([&](size_t s, int, int) { slot[s]++; });
    G.blkStart.assign(1, 0);
    for (int c = 0; c < nf; c++)
        for (int d = 0; d <= b; d++) {
            int& s = slot[(size_t)c * (b + 1) + d];
            if (!s) { s = -1; continue; }
            G.blkC.push_back(c); G.blkD.push_back(d);
            G.blkStart.push_back(G.blkStart.back() + s);
            s = (int)G.blkC.size() - 1;
        }
    G.nBlk = (int)G.blkC.size();
    G.list.assign(std::max<size_t>((size_t)G.blkStart.back() * 2, 2), 0);
    {
        std::vector<int> fill(G.blkStart.begin(), G.blkStart.end() - 1);
        each_entry([&](size_t s, int p1, int p2) { const int at = fill[slot[s]]++; G.list[2 * (size_t)at] = p1; G.list[2 * (size_t)at + 1] = p2; });
    }
    return GBA_HOST_OK;
}

}  // namespace vslam
