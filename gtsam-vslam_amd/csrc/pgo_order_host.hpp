// Host-only (no HIP): the reordering of the block-banded solves (pgo.hip, gba.hip).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace vslam {

// Reverse Cuthill-McKee over the free-free graph (adjacency lists sorted, duplicates removed).  Components are taken in ascending
// order of their lowest pose; a component starts at its pose of smallest degree (the lowest index on a tie); a pose's unvisited
// neighbours join the queue in ascending (degree, index); the whole sequence is reversed at the end.
inline void pgo_rcm(int nf, const std::vector<std::vector<int>>& adj, std::vector<int>& order) {
    std::vector<uint8_t> seen(nf, 0);
    std::vector<int> comp, nb;
    order.clear();
    for (int s0 = 0; s0 < nf; s0++) {
        if (seen[s0]) continue;
        comp.clear(); comp.push_back(s0); seen[s0] = 1;
        for (size_t h = 0; h < comp.size(); h++) for (int v : adj[comp[h]]) if (!seen[v]) { seen[v] = 1; comp.push_back(v); }
        int start = comp[0];
        for (int v : comp) if (adj[v].size() < adj[start].size() || (adj[v].size() == adj[start].size() && v < start)) start = v;
        for (int v : comp) seen[v] = 2;            // 2: in the component, not queued
        const size_t base = order.size();
        order.push_back(start); seen[start] = 1;
        for (size_t h = base; h < order.size(); h++) {
            nb.clear();
            for (int v : adj[order[h]]) if (seen[v] == 2) { seen[v] = 1; nb.push_back(v); }
            std::sort(nb.begin(), nb.end(), [&](int a, int b) { return adj[a].size() != adj[b].size() ? adj[a].size() < adj[b].size() : a < b; });
            order.insert(order.end(), nb.begin(), nb.end());
        }
    }
    std::reverse(order.begin(), order.end());
}

}  // namespace vslam
