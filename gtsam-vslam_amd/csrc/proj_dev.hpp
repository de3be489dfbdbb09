// Device helpers shared by the projection-matching kernels (proj.hip) and the new-point pipeline (newpts.hip):
// candidate keys and the wave-wide window scan of getMatchIdxs (reference src/FeatureMatcher.cpp:13-64).
#pragma once
#include "matcher.hpp"

namespace vslam {

__device__ __forceinline__ int p_cvFloor(float v) { int i = (int)v; return i - (i > v); }
__device__ __forceinline__ int p_cvCeil(float v) { int i = (int)v; return i + (i < v); }

constexpr unsigned long long KEY_NONE = ~0ull;
// key = dist | cell | idx | octave at the KEY_*_SHIFT positions of matcher.hpp   (idx unique => octave never decides order)
__device__ __forceinline__ unsigned long long make_key(int dist, int cell, int idx, int oct) {
    return ((unsigned long long)dist << KEY_DIST_SHIFT) | ((unsigned long long)cell << KEY_CELL_SHIFT) |
           ((unsigned long long)idx << KEY_IDX_SHIFT) | (unsigned long long)(oct & ((1 << KEY_OCT_BITS) - 1));
}
__device__ __forceinline__ int key_dist(unsigned long long k) { return (int)(k >> KEY_DIST_SHIFT); }
__device__ __forceinline__ int key_idx(unsigned long long k) { return (int)((k >> KEY_IDX_SHIFT) & ((1 << KEY_IDX_BITS) - 1)); }
__device__ __forceinline__ int key_oct(unsigned long long k) { return (int)(k & ((1 << KEY_OCT_BITS) - 1)); }
// (cell, idx) of a key = its position in the reference's visit order (rows, columns, then the order within a cell)
constexpr unsigned long long KEY_POS_MASK = ((1ull << KEY_DIST_SHIFT) - 1ull) & ~((1ull << KEY_IDX_SHIFT) - 1ull);

template <int K>
__device__ __forceinline__ void insert_sorted(unsigned long long (&a)[K], unsigned long long key) {
#pragma unroll
    for (int j = 0; j < K; j++) {
        if (key < a[j]) { const unsigned long long t = a[j]; a[j] = key; key = t; }
    }
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d);
        v = o < v ? o : v;
    }
    return v;
}

// v of lane `src` (wave-uniform): two v_readlane into SGPRs, no LDS crossbar
__device__ __forceinline__ unsigned long long wave_read_u64(unsigned long long v, int src) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, src);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}

// lane form of a selection result: lane r < K holds out[r]
template <int K>
__device__ __forceinline__ unsigned long long sel_from_array(const unsigned long long (&out)[K], int lane) {
    unsigned long long v = KEY_NONE;
#pragma unroll
    for (int j = 0; j < K; j++) v = lane == j ? out[j] : v;
    return v;
}

// Every lane holds at most one key (KEY_NONE = none; valid keys are unique).  Returns, in lane r < K, the key of rank r in
// ascending order, KEY_NONE in every other lane and for ranks past the last valid key.  The valid lanes are walked as the set
// bits of their ballot: a lane's key is read into SGPRs and every lane counts the keys below its own, then the lanes of rank
// < K hand their key to lane `rank` the same way - a few VALU instructions per key that exists, none for the empty lanes.
template <int K>
__device__ __forceinline__ unsigned long long rank_select(unsigned long long key, int lane) {
    const bool valid = key != KEY_NONE;
    int rank = 0;
    for (unsigned long long m = __ballot(valid); m; m &= m - 1) rank += wave_read_u64(key, __builtin_ctzll(m)) < key;
    unsigned long long res = KEY_NONE;
    for (unsigned long long m = __ballot(valid && rank < K); m; m &= m - 1) {
        const int b = __builtin_ctzll(m);
        const int rb = __builtin_amdgcn_readlane(rank, b);
        const unsigned long long kb = wave_read_u64(key, b);
        res = lane == rb ? kb : res;
    }
    return res;
}

#ifdef VSLAM_PROJ_HIST
// -DVSLAM_PROJ_HIST (tools/proj_rate.py --hist): window entries visited / Hamming tests per PROJ_K-wide job, clamped to 64+
static __device__ unsigned long long g_projHist[2][66];
__device__ __forceinline__ void proj_hist_add(int visited, int tests) {
    if ((threadIdx.x & 63) != 0) return;
    atomicAdd(&g_projHist[0][min(visited, 65)], 1ull);
    atomicAdd(&g_projHist[1][min(tests, 65)], 1ull);
}
#endif

// Scan one side for one map point; lane r < K of `sel` receives the r-th smallest key (KEY_NONE past the last one) - read a
// rank wave-wide with wave_read_u64(sel, r).  `claimed` (may be null) = claim table to respect.  Returns the number of Hamming
// tests (wave-uniform).  `sparse` = false keeps every window on the general path (VSLAM_PROJ_SELECT=0: A/B and tests).
// `visited` (may be null; the VSLAM_PROJ_HIST build) receives the number of keys the scan walked over.
template <int K>
__device__ int scan_side(const ProjArgs& A, int side, const uint32_t (&md)[8], float px, float py,
                         int predScale, const int* claimed, unsigned long long& sel, bool sparse = true, int* visited = nullptr) {
    const int lane = threadIdx.x & 63;
    sel = KEY_NONE;
    const float radius = A.scalePyr[predScale] * A.rad;
    const int minX = max(0, p_cvFloor((px - radius) * A.xMult));
    const int maxX = min(A.xGrids - 1, p_cvCeil((px + radius) * A.xMult));
    const int minY = max(0, p_cvFloor((py - radius) * A.yMult));
    const int maxY = min(A.yGrids - 1, p_cvCeil((py + radius) * A.yMult));
    const bool any = !(minX >= A.xGrids || minY >= A.yGrids || maxX < 0 || maxY < 0);
    const vslam_keypoint* kps = A.kps[side];
    const uint8_t* desc = A.desc[side];
    // the tests of one candidate keypoint (every path below applies exactly these, in this order): its key, or KEY_NONE if a
    // filter rejects it before the Hamming test
    auto consider = [&](int idx) -> unsigned long long {
        const float kx = kps[idx].x, ky = kps[idx].y;
        int cx = __float2int_rn(kx * A.xMult), cy = __float2int_rn(ky * A.yMult);
        cx = cx < 0 ? 0 : (cx >= A.xGrids ? A.xGrids - 1 : cx);
        cy = cy < 0 ? 0 : (cy >= A.yGrids ? A.yGrids - 1 : cy);
        if (cx < minX || cx > maxX || cy < minY || cy > maxY) return KEY_NONE;
        const int oct = kps[idx].octave;
        if (oct > predScale + 1 || oct < predScale - 1) return KEY_NONE;
        if (!(fabsf(kx - px) < radius && fabsf(ky - py) < radius)) return KEY_NONE;
        if (claimed && claimed[idx] >= 0) return KEY_NONE;
        if (A.mode == PROJ_RADIUS) {      // Converter::checkPixelParallax (include/Conversions.h:25,140-144)
            const double dx = (double)kx - (double)px, dy = (double)ky - (double)py;
            if (!(sqrt(dx * dx + dy * dy) > 10.0)) return KEY_NONE;
        }
        const uint4* pr = (const uint4*)(desc + (size_t)idx * 32);
        const uint4 r0 = pr[0], r1 = pr[1];
        const int dist = __popc(md[0] ^ r0.x) + __popc(md[1] ^ r0.y) + __popc(md[2] ^ r0.z) +
                         __popc(md[3] ^ r0.w) + __popc(md[4] ^ r1.x) + __popc(md[5] ^ r1.y) +
                         __popc(md[6] ^ r1.z) + __popc(md[7] ^ r1.w);
        return make_key(dist, cy * A.xGrids + cx, idx, oct);
    };
    if (!any) return 0;
    const int nrows = __builtin_amdgcn_readfirstlane(maxY - minY + 1);      // (the window is wave-uniform)
    const bool bucketed = A.cellStart[side] && nrows <= 64;
    int rbeg = 0, rlen = 0;
    if (bucketed) {
        // bucketed keys: the window is nrows runs of consecutive cells = nrows contiguous slices of cellIdx (lane r holds slice r).
        // The keys carry (cell, index), so the visit order does not matter.
        const int* cs = A.cellStart[side];
        const unsigned short* ci = A.cellIdx[side];
        if (lane < nrows) {
            const int c0 = (minY + lane) * A.xGrids;
            rbeg = cs[c0 + minX];
            rlen = cs[c0 + maxX + 1] - rbeg;
        }
        if (sparse) {
            // entry `lane` of the concatenated slices, found with the slices' bounds in SGPRs (one short scalar loop over the rows
            // instead of a 64-lane prefix scan and per-lane lookups through the LDS crossbar)
            int total = 0, src = -1;
            for (int q = 0; q < nrows; q++) {
                const int lq = __builtin_amdgcn_readlane(rlen, q), bq = __builtin_amdgcn_readlane(rbeg, q);
                const int o = lane - total;
                if ((unsigned)o < (unsigned)lq) src = bq + o;
                total += lq;
            }
            if (total <= 64) {
                // at most one key per lane: no per-lane sorted list, no wave-wide merge
                unsigned long long key = KEY_NONE;
                if (src >= 0) key = consider((int)ci[src]);
                sel = rank_select<K>(key, lane);
                if (visited) *visited = total;
                return __popcll(__ballot(key != KEY_NONE));
            }
        }
    }
    // general path: a sorted list of the K smallest keys per lane, merged by K rounds of a wave-wide minimum
    unsigned long long top[K];
#pragma unroll
    for (int j = 0; j < K; j++) top[j] = KEY_NONE;
    int tests = 0;
    auto take = [&](unsigned long long key) {
        if (key == KEY_NONE) return;
        tests++;
        insert_sorted<K>(top, key);
    };
    if (bucketed) {
        // the slices are concatenated (inclusive scan of the lengths) and walked 64 entries at a time
        const unsigned short* ci = A.cellIdx[side];
        int incl = rlen;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(incl, d); if (lane >= d) incl += t; }
        const int total = __shfl(incl, 63);
        if (visited) *visited = total;
        for (int base = 0; base < total; base += 64) {
            const int p = base + lane;
            int r = 0;
            for (int q = 0; q < nrows; q++) r += (p >= __shfl(incl, q));
            r = r < nrows ? r : nrows - 1;
            const int re = __shfl(incl, r), rl = __shfl(rlen, r), rb = __shfl(rbeg, r);
            if (p < total) take(consider((int)ci[rb + (p - (re - rl))]));
        }
    } else {
        const int n = A.n[side];
        if (visited) *visited = n;
        for (int idx = lane; idx < n; idx += 64) take(consider(idx));
    }
    unsigned long long out[K];
#pragma unroll
    for (int j = 0; j < K; j++) out[j] = KEY_NONE;
#pragma unroll
    for (int r = 0; r < K; r++) {
        const unsigned long long head = top[0];
        const unsigned long long m = wave_min_u64(head);
        if (m == KEY_NONE) break;      // (wave-uniform) no key left: the remaining ranks stay KEY_NONE
        out[r] = m;
        if (head == m) {
#pragma unroll
            for (int j = 0; j + 1 < K; j++) top[j] = top[j + 1];
            top[K - 1] = KEY_NONE;
        }
    }
    sel = sel_from_array<K>(out, lane);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) tests += __shfl_xor(tests, d);
    return tests;
}


}  // namespace vslam
