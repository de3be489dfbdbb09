// Host-only lane packing of vslam_global_ba_batch (no HIP: tests/native/gba_pack.cpp builds it alone under the sanitizers).
// The lanes' arrays are concatenated; a lane's table entry holds its sizes, its camera and where its parts begin.  Every offset
// is an ELEMENT count in int (the kernels multiply by the record size in size_t); indices inside a lane's arrays stay lane-local.
// The sums over all lanes are limited so that every offset fits int32.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace vslam {

constexpr int GBA_MAX_LANES = 1024;                     // (k_gba_decide_b is ONE workgroup with a thread per lane)
// sums over the lanes of one call (the pose-graph batch's figures for keyframes, edges and band blocks)
constexpr long long GBA_SUM_KF = 262144, GBA_SUM_EDGES = 1048576, GBA_SUM_BLOCKS = 1048576;
constexpr long long GBA_SUM_PAIRS = 8388608, GBA_SUM_LM = 4194304, GBA_SUM_LIST = 67108864;

// what the packing needs of one lane: the problem's sizes and its plan's (gba_host.hpp)
struct GbaLaneShape {
    int K = 0, L = 0, P = 0, M = 0;                     // keyframes, landmarks, pairs, edges
    int nf = 0, b = 0, nBlk = 0;                        // block columns, half-bandwidth, blocks with a list
    int nInc = 0, nLmPairs = 0, nList = 0;              // incidence entries, entries of the landmarks' pair lists, block-list entries
    int hasUnknowns = 0;
    double fx = 0, fy = 0, cx = 0, cy = 0, bl = 0;
};

// a lane's table entry on the device
struct GbaLane {
    int K, L, P, M, nf, b, nBlk, hasUnknowns;
    int kf0;        // first keyframe: poses (x 12), pos, kf_local
    int lm0;        // first landmark: values (x 3), presence, Hinv (x 9), gl (x 3); the lane's L + 1 list starts begin at lm0 + lane
    int pair0;      // first pair: its index arrays, uv (x 4), whitening and thresholds (x 2), Jp (x 24), Jl (x 12), res (x 4), W, Y (x 18), flags
    int edge0;      // first edge: edges, res (x 6), Ji, Jj (x 36); the lane's 2 P + M cost terms begin at 2 pair0 + edge0
    int free0;      // first block column: diagH, g, rhs (x 6); the lane's nf + 1 row starts begin at free0 + lane; its
                    // 6 nf + 3 L steps begin at 6 free0 + 3 lm0
    int inc0, lp0;  // first incidence entry, first entry of the landmarks' pair lists
    int band0;      // first band block (x 36)
    int blk0;       // first listed block: blkC, blkD; the lane's nBlk + 1 list starts begin at blk0 + lane
    int list0;      // first block-list entry (x 2 ints)
    int lane, pad;
    double fx, fy, cx, cy, bl;
};

struct GbaPackSums { long long K = 0, L = 0, P = 0, M = 0, nf = 0, inc = 0, lp = 0, band = 0, blk = 0, list = 0; };

// the sums a call is refused for before any lane is planned; 0 or GBA_HOST_CAPACITY's value (4) with *err set
inline int gba_pack_check_sizes(const GbaLaneShape* s, int n, std::string* err) {
    long long K = 0, L = 0, P = 0, M = 0;
    for (int l = 0; l < n; l++) { K += s[l].K; L += s[l].L; P += s[l].P; M += s[l].M; }
    char buf[256];
    if (K > GBA_SUM_KF || M > GBA_SUM_EDGES) {
        snprintf(buf, sizeof buf, "%lld keyframes / %lld edges in all exceed the limits (%lld / %lld)", K, M, GBA_SUM_KF, GBA_SUM_EDGES);
        *err = buf; return 4;
    }
    if (P > GBA_SUM_PAIRS || L > GBA_SUM_LM) {
        snprintf(buf, sizeof buf, "%lld pairs / %lld landmarks in all exceed the limits (%lld / %lld)", P, L, GBA_SUM_PAIRS, GBA_SUM_LM);
        *err = buf; return 4;
    }
    return 0;
}

// the table of n planned lanes, in order; 0 or 4 (a sum of band blocks or block-list entries beyond its limit) with *err set
inline int gba_pack(const GbaLaneShape* s, int n, std::vector<GbaLane>& tab, GbaPackSums& S, std::string* err) {
    if (const int st = gba_pack_check_sizes(s, n, err)) return st;
    tab.assign(n > 0 ? n : 1, GbaLane{});
    S = GbaPackSums{};
    char buf[256];
    for (int l = 0; l < n; l++) {
        const GbaLaneShape& Q = s[l];
        const long long band = (long long)(Q.b + 1) * Q.nf;
        if (S.band + band > GBA_SUM_BLOCKS) {
            snprintf(buf, sizeof buf, "the lanes' bands need more than %lld blocks in all (reached at lane %d of those that hold a problem)", GBA_SUM_BLOCKS, l);
            *err = buf; return 4;
        }
        if (S.list + Q.nList > GBA_SUM_LIST) {
            snprintf(buf, sizeof buf, "the lanes' block lists need more than %lld entries in all (reached at lane %d of those that hold a problem)", GBA_SUM_LIST, l);
            *err = buf; return 4;
        }
        GbaLane& T = tab[l];
        T.K = Q.K; T.L = Q.L; T.P = Q.P; T.M = Q.M; T.nf = Q.nf; T.b = Q.b; T.nBlk = Q.nBlk; T.hasUnknowns = Q.hasUnknowns;
        T.kf0 = (int)S.K; T.lm0 = (int)S.L; T.pair0 = (int)S.P; T.edge0 = (int)S.M; T.free0 = (int)S.nf;
        T.inc0 = (int)S.inc; T.lp0 = (int)S.lp; T.band0 = (int)S.band; T.blk0 = (int)S.blk; T.list0 = (int)S.list;
        T.lane = l; T.pad = 0;
        T.fx = Q.fx; T.fy = Q.fy; T.cx = Q.cx; T.cy = Q.cy; T.bl = Q.bl;
        S.K += Q.K; S.L += Q.L; S.P += Q.P; S.M += Q.M; S.nf += Q.nf; S.inc += Q.nInc; S.lp += Q.nLmPairs;
        S.band += band; S.blk += Q.nBlk; S.list += Q.nList;
    }
    return 0;
}

}  // namespace vslam
