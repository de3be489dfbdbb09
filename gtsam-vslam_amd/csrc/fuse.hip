// Duplicate search between two copies of a place (no reference counterpart; vslam_hip.h, DESIGN.md section 6 item 26, restated by
// tests/fuse_ref.py): set A (the new copy) against set B (the old copy) under ONE camera - a geometric gate on the projections, then
// the best 256-bit Hamming distance among the gated targets, then one proposer per target.
// There is ONE path (fuse_run): several lanes at once, one launch per stage for all of them, each kernel on a lane's part of
// concatenated arrays.  vslam_fuse_search is its one-lane case, so a lane's bytes are the single call's by construction.
//   k_fuse_project_b   one thread per point of either set: the 16-byte record (u, v, z, pad), (NaN, NaN, -1) for a point outside the image;
//                      the winner word of the point's slot is reset beside it
//   k_fuse_match_b     one thread per A point (descriptor and record in registers); the workgroup stages B through LDS in tiles of
//                      FUSE_TILE targets, record and descriptor together.  Every lane reads the SAME LDS address (a broadcast).
//                      The gate is tested from the record alone, eight targets per wave vote; a target's descriptor is read and
//                      counted only when some lane of the wave passed its gate (wave-uniform: results cannot depend on it).  A
//                      proposal is a 64-bit atomicMin.
//   k_fuse_resolve_b   one thread per A point reads winner[b1] back and writes match; workgroup 0 of a lane counts the four figures
//                      of its report (integer sums)
#include "common.hpp"
#include "dmath.hpp"
#include <cmath>

using namespace vslam;

namespace {

constexpr int FUSE_TILE = 1024;               // B targets staged per LDS tile: 16 + 32 bytes each = 48 KB, three workgroups a CU
constexpr int FUSE_GROUP = 8;                 // targets gated per wave vote (divides FUSE_TILE)
static_assert(FUSE_TILE % FUSE_GROUP == 0 && (FUSE_GROUP & (FUSE_GROUP - 1)) == 0 && FUSE_GROUP <= 32, "a padded group stays inside the tile");
constexpr int FUSE_MAX_POINTS = 65536;        // per set
constexpr int FUSE_MAX_LANES = 256;
constexpr int FUSE_SUM_POINTS = 1048576;      // both sets, all lanes

// one lane of a call.  Points are numbered over the whole call: the lane's A points from p0, its B points right behind them (p0 + nA);
// the per-A outputs from a0.
struct FuseLane {
    int nA, nB, p0, a0;
    int w, h;
    double fx, fy, cx, cy;
    double R[9], t[3];
};

__device__ __forceinline__ int fuse_hamming(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
           __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// The record of a point outside the image: z = -1 and NaN for the pixel.  du, dv and their squares are then NaN and `<= radius^2` is
// false whatever the other record holds, so an invisible point gates nothing at ANY depth_ratio (the depth compares alone would let two
// records with z = -1 pass each other at depth_ratio = 1).  The padding of a partial group of k_fuse_match_b is this record too.
__device__ __forceinline__ float4 fuse_invisible() { return make_float4(__builtin_nanf(""), __builtin_nanf(""), -1.f, 0.f); }

// grid (ceil(max (nA + nB) / 256), lanes)
__global__ __launch_bounds__(256) void k_fuse_project_b(const FuseLane* __restrict__ lanes, const double* __restrict__ xyz,
                                                        float4* __restrict__ rec, unsigned long long* __restrict__ winner) {
    const FuseLane& L = *lane_entry(lanes, blockIdx.y);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= L.nA + L.nB) return;
    const size_t p = (size_t)L.p0 + i;
    const double X[3] = {xyz[3 * p], xyz[3 * p + 1], xyz[3 * p + 2]};
    double Xc[3];
    mat3_vec(L.R, X, Xc);
#pragma unroll
    for (int k = 0; k < 3; k++) Xc[k] += L.t[k];
    float4 r = fuse_invisible();
    if (Xc[2] > 0.0) {
        const double invZ = 1.0 / Xc[2];
        const double u = L.fx * Xc[0] * invZ + L.cx, v = L.fy * Xc[1] * invZ + L.cy;
        if (!(u < 0 || v < 0 || u >= L.w || v >= L.h)) r = make_float4((float)u, (float)v, (float)Xc[2], 0.f);
    }
    rec[p] = r;
    winner[p] = ~0ull;
}

// grid (ceil(max nA / 256), lanes).  A workgroup wholly past its lane's nA leaves before the first barrier; threads past nA inside a
// workgroup take part in every barrier and every wave vote with an invisible record, which passes no gate.
template <bool SKIP>
__global__ __launch_bounds__(256) void k_fuse_match_b(const FuseLane* __restrict__ lanes, const float4* __restrict__ rec,
                                                      const uint4* __restrict__ desc, float r2, float ratio, int maxHamming,
                                                      int4* __restrict__ best, unsigned long long* __restrict__ winner) {
    __shared__ float4 sRec[FUSE_TILE];
    __shared__ uint4 sDesc[2 * FUSE_TILE];
    const FuseLane& L = *lane_entry(lanes, blockIdx.y);
    const int nA = L.nA, nB = L.nB;
    if ((int)(blockIdx.x * 256) >= nA) return;
    const int a = blockIdx.x * 256 + threadIdx.x;
    const size_t pB = (size_t)L.p0 + nA;
    float4 ra = fuse_invisible();
    uint4 a0 = make_uint4(0, 0, 0, 0), a1 = a0;
    if (a < nA) {
        const size_t p = (size_t)L.p0 + a;
        ra = rec[p]; a0 = desc[2 * p]; a1 = desc[2 * p + 1];
    }
    const float zaHi = ratio * ra.z;
    int d1 = 257, d2 = 257, b1 = -1, nG = 0;
    for (int base = 0; base < nB; base += FUSE_TILE) {
        const int cnt = min(FUSE_TILE, nB - base);
        __syncthreads();                          // the previous tile has been consumed
        const int cnt8 = (cnt + FUSE_GROUP - 1) & ~(FUSE_GROUP - 1);      // a partial last group is padded with invisible records
        for (int q = threadIdx.x; q < cnt8; q += 256) sRec[q] = q < cnt ? rec[pB + base + q] : fuse_invisible();
        for (int q = threadIdx.x; q < 2 * cnt; q += 256) sDesc[q] = desc[2 * (pB + base) + q];
        __syncthreads();
        // The gates of FUSE_GROUP targets at a time, as a bit mask: their record reads are in flight together and the wave votes once
        // per group (a workgroup has one wave per SIMD and nothing else hides an LDS read's latency; one vote and one branch per
        // target made the scan 0.10 us per target).  A group in which some lane passed some gate is then
        // walked target by target in ascending index, each under its own vote.
        for (int k0 = 0; k0 < cnt8; k0 += FUSE_GROUP) {
            unsigned m = 0;
#pragma unroll
            for (int j = 0; j < FUSE_GROUP; j++) {
                const float4 rb = sRec[k0 + j];
                const float du = ra.x - rb.x, dv = ra.y - rb.y;
                const bool pass = du * du + dv * dv <= r2 && rb.z <= zaHi && ra.z <= ratio * rb.z;
                m |= (pass ? 1u : 0u) << j;
            }
            if (SKIP && !__any(m != 0)) continue;         // (wave-uniform)
#pragma unroll
            for (int j = 0; j < FUSE_GROUP; j++) {
                const bool pass = (m >> j) & 1u;
                if (!SKIP || __any(pass)) {               // (wave-uniform)
                    const int d = fuse_hamming(a0, a1, sDesc[2 * (k0 + j)], sDesc[2 * (k0 + j) + 1]);
                    if (pass) {
                        nG++;
                        if (d < d1) { d2 = d1; d1 = d; b1 = base + k0 + j; }
                        else if (d < d2) d2 = d;
                    }
                }
            }
        }
    }
    if (a >= nA) return;
    best[(size_t)L.a0 + a] = make_int4(d1, b1, d2, nG);
    if (nG > 0 && d1 <= maxHamming) atomicMin(&winner[pB + b1], ((unsigned long long)d1 << 32) | (unsigned)a);
}

// grid (max(ceil(max nA / 256), 1), lanes)
__global__ __launch_bounds__(256) void k_fuse_resolve_b(const FuseLane* __restrict__ lanes, const float4* __restrict__ rec,
                                                        const int4* __restrict__ best, const unsigned long long* __restrict__ winner,
                                                        int maxHamming, int* __restrict__ match, int* __restrict__ report) {
    __shared__ int sCnt[4][4];
    const FuseLane& L = *lane_entry(lanes, blockIdx.y);
    const int nA = L.nA, nB = L.nB;
    const size_t pB = (size_t)L.p0 + nA;
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a < nA) {
        const int4 q = best[(size_t)L.a0 + a];
        int m = -1;
        if (q.w > 0 && q.x <= maxHamming && (unsigned)(winner[pB + q.y] & 0xFFFFFFFFull) == (unsigned)a) m = q.y;
        match[(size_t)L.a0 + a] = m;
    }
    if (blockIdx.x != 0) return;
    int c[4] = {0, 0, 0, 0};                      // visible A, visible B, proposals, pairs
    for (int i = threadIdx.x; i < nA; i += 256) {
        const int4 q = best[(size_t)L.a0 + i];
        c[0] += rec[(size_t)L.p0 + i].z > 0.f;
        if (q.w > 0 && q.x <= maxHamming) {
            c[2]++;
            c[3] += (unsigned)(winner[pB + q.y] & 0xFFFFFFFFull) == (unsigned)i;
        }
    }
    for (int i = threadIdx.x; i < nB; i += 256) c[1] += rec[pB + i].z > 0.f;
#pragma unroll
    for (int k = 0; k < 4; k++) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) c[k] += __shfl_down(c[k], off);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++) sCnt[threadIdx.x >> 6][k] = c[k];
    }
    __syncthreads();
    if (threadIdx.x < 4) report[4 * blockIdx.y + threadIdx.x] = sCnt[0][threadIdx.x] + sCnt[1][threadIdx.x] + sCnt[2][threadIdx.x] + sCnt[3][threadIdx.x];
}

inline bool fuse_finite(const double* p, size_t n) { for (size_t k = 0; k < n; k++) if (!std::isfinite(p[k])) return false; return true; }

thread_local std::vector<std::pair<const char*, float>> g_fuseTimes;
thread_local bool g_fuseTimingOn = false;

// VSLAM_FUSE_SKIP=0: k_fuse_match_b counts every target's descriptor, gated or not - the worth of the wave-uniform skip can be
// measured, and both settings are pinned to the same bytes (read per call)
bool fuse_skip() {
    const char* e = getenv("VSLAM_FUSE_SKIP");
    return !(e && e[0] == '0');
}

struct FuseLayout {
    size_t bytes = 0;
    size_t section(size_t n) { const size_t at = bytes; bytes = align_up_sz(bytes + std::max<size_t>(n, 8), 256); return at; }
};

// the defaults and ranges of vslam_fuse_params
vslam_status fuse_check_params(const char* who, const vslam_fuse_params* prm, vslam_fuse_params& P) {
    P = prm ? *prm : vslam_fuse_params{};
    if (!std::isfinite(P.radius) || !std::isfinite(P.depth_ratio)) { set_error("%s: non-finite parameter", who); return VSLAM_ERR_INVALID; }
    if (P.radius < 0 || P.depth_ratio < 0 || P.max_hamming < 0) { set_error("%s: negative parameter", who); return VSLAM_ERR_INVALID; }
    if (P.depth_ratio > 0 && P.depth_ratio < 1) { set_error("%s: depth_ratio %g lies inside (0, 1)", who, (double)P.depth_ratio); return VSLAM_ERR_INVALID; }
    if (P.radius == 0) P.radius = 4.0f;
    if (P.depth_ratio == 0) P.depth_ratio = 1.25f;
    if (P.max_hamming == 0) P.max_hamming = 50;
    return VSLAM_OK;
}

// THE search, behind both entry points: `n` lanes, the checked parameters.  Every lane is validated before anything is launched or
// written; `who` starts every error text, with the lane where `nameLane` says so.
vslam_status fuse_run(const char* who, bool nameLane, const vslam_fuse_lane* lanes, int n, const vslam_fuse_params& P, int device,
                      vslam_fuse_report* reports) {
    char lw[96];
    auto lane_text = [&](int g) { if (nameLane) snprintf(lw, sizeof lw, "%s: lane %d", who, g); else snprintf(lw, sizeof lw, "%s", who); return lw; };
    std::vector<int> live;
    std::vector<FuseLane> tab;
    long long sumP = 0, sumA = 0;
    int maxA = 0, maxP = 0;
    for (int g = 0; g < n; g++) {
        const vslam_fuse_lane& Q = lanes[g];
        if (Q.n_a < 0 || Q.n_b < 0) { set_error("%s: negative count", lane_text(g)); return VSLAM_ERR_INVALID; }
        if (Q.n_a == 0 && Q.n_b == 0) continue;
        if (!Q.T_cw || (Q.n_a > 0 && (!Q.a_xyz || !Q.a_desc || !Q.match || !Q.best)) || (Q.n_b > 0 && (!Q.b_xyz || !Q.b_desc))) {
            set_error("%s: invalid arguments", lane_text(g)); return VSLAM_ERR_INVALID;
        }
        if (Q.w < 1 || Q.h < 1) { set_error("%s: image size %d x %d", lane_text(g), Q.w, Q.h); return VSLAM_ERR_INVALID; }
        const double K[4] = {Q.fx, Q.fy, Q.cx, Q.cy};
        if (!fuse_finite(K, 4) || !fuse_finite(Q.T_cw, 16)) { set_error("%s: non-finite pose or intrinsic", lane_text(g)); return VSLAM_ERR_INVALID; }
        if (Q.n_a > FUSE_MAX_POINTS || Q.n_b > FUSE_MAX_POINTS) {
            set_error("%s: %d / %d points exceed the limit (%d per set)", lane_text(g), Q.n_a, Q.n_b, FUSE_MAX_POINTS); return VSLAM_ERR_CAPACITY;
        }
        if (!fuse_finite(Q.a_xyz, 3 * (size_t)Q.n_a) || !fuse_finite(Q.b_xyz, 3 * (size_t)Q.n_b)) {
            set_error("%s: non-finite coordinate", lane_text(g)); return VSLAM_ERR_INVALID;
        }
        FuseLane L{};
        L.nA = Q.n_a; L.nB = Q.n_b; L.p0 = (int)sumP; L.a0 = (int)sumA; L.w = Q.w; L.h = Q.h;
        L.fx = Q.fx; L.fy = Q.fy; L.cx = Q.cx; L.cy = Q.cy;
        for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) L.R[3 * r + c] = Q.T_cw[4 * r + c]; L.t[r] = Q.T_cw[4 * r + 3]; }
        tab.push_back(L); live.push_back(g);
        sumP += (long long)Q.n_a + Q.n_b; sumA += Q.n_a;
        maxA = std::max(maxA, Q.n_a); maxP = std::max(maxP, Q.n_a + Q.n_b);
        if (sumP > FUSE_SUM_POINTS) { set_error("%s: more than %d points over all lanes (reached at lane %d)", who, FUSE_SUM_POINTS, g); return VSLAM_ERR_CAPACITY; }
    }
    const int nl = (int)live.size();
    if (nl == 0) return VSLAM_OK;                 // (every lane idle: nothing to search, nothing written)
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available (no CPU fallback)"); return VSLAM_ERR_NO_DEVICE; }
    if (device < 0 || device >= ndev) { set_error("%s: device %d of %d", who, device, ndev); return VSLAM_ERR_INVALID; }
    VS_HIP(hipSetDevice(device));
    DevPool* pool = thread_pool(device);
    if (!pool) { set_error("no device pool"); return VSLAM_ERR_HIP; }
    pool->pending.clear();
    hipStream_t st = pool->stream;

    FuseLayout up, wk, dn;                        // the upload block, the work block, the download part of the work block
    const size_t oTab = up.section(nl * sizeof(FuseLane)), oXyz = up.section((size_t)sumP * 24), oDesc = up.section((size_t)sumP * 32);
    const size_t oBest = dn.section((size_t)sumA * 16), oMatch = dn.section((size_t)sumA * 4), oRep = dn.section((size_t)nl * 16);
    const size_t oDn = wk.section(dn.bytes), oRec = wk.section((size_t)sumP * 16), oWin = wk.section((size_t)sumP * 8);
    // The lanes' arrays are packed ONCE, straight into the pool's pinned arena (up to 59 MB: a pageable block first and the arena
    // behind it would copy them twice).  A call the arena cannot hold yet packs into a pageable block; the arena grows at the sync.
    // The bytes between two sections are never read.
    PoolBuf<uint8_t> dUp(pool), dWk(pool);
    VS_HIP(dUp.alloc(up.bytes)); VS_HIP(dWk.alloc(wk.bytes));
    std::vector<uint8_t> hPage;
    uint8_t* hUp = pool->stage(up.bytes);
    if (!hUp) { hPage.resize(up.bytes); hUp = hPage.data(); }
    memcpy(hUp + oTab, tab.data(), nl * sizeof(FuseLane));
    for (int l = 0; l < nl; l++) {
        const vslam_fuse_lane& Q = lanes[live[l]];
        const size_t p0 = (size_t)tab[l].p0, pB = p0 + Q.n_a;
        if (Q.n_a) { memcpy(hUp + oXyz + p0 * 24, Q.a_xyz, (size_t)Q.n_a * 24); memcpy(hUp + oDesc + p0 * 32, Q.a_desc, (size_t)Q.n_a * 32); }
        if (Q.n_b) { memcpy(hUp + oXyz + pB * 24, Q.b_xyz, (size_t)Q.n_b * 24); memcpy(hUp + oDesc + pB * 32, Q.b_desc, (size_t)Q.n_b * 32); }
    }
    VS_HIP(hipMemcpyAsync(dUp.p, hUp, up.bytes, hipMemcpyHostToDevice, st));
    const FuseLane* dTab = (const FuseLane*)(dUp.p + oTab);
    const double* dXyz = (const double*)(dUp.p + oXyz);
    const uint4* dDesc = (const uint4*)(dUp.p + oDesc);
    int4* dBest = (int4*)(dWk.p + oDn + oBest);
    int* dMatch = (int*)(dWk.p + oDn + oMatch);
    int* dRep = (int*)(dWk.p + oDn + oRep);
    float4* dRec = (float4*)(dWk.p + oRec);
    unsigned long long* dWin = (unsigned long long*)(dWk.p + oWin);

    struct TimerOwner { StageTimer t; ~TimerOwner() { t.destroy(); } } timerOwner;
    StageTimer& timer = timerOwner.t;
    timer.stream = st; timer.multi = true; timer.enabled = g_fuseTimingOn;
    const float r2 = P.radius * P.radius;
    const unsigned gA = (unsigned)((maxA + 255) / 256);
    int t = timer.begin("fuse_project");
    hipLaunchKernelGGL(k_fuse_project_b, dim3((maxP + 255) / 256, nl), dim3(256), 0, st, dTab, dXyz, dRec, dWin);
    timer.end(t);
    t = timer.begin("fuse_match");
    if (gA) {
        if (fuse_skip()) hipLaunchKernelGGL(k_fuse_match_b<true>, dim3(gA, nl), dim3(256), 0, st, dTab, dRec, dDesc, r2, P.depth_ratio, P.max_hamming, dBest, dWin);
        else hipLaunchKernelGGL(k_fuse_match_b<false>, dim3(gA, nl), dim3(256), 0, st, dTab, dRec, dDesc, r2, P.depth_ratio, P.max_hamming, dBest, dWin);
    }
    timer.end(t);
    t = timer.begin("fuse_resolve");
    hipLaunchKernelGGL(k_fuse_resolve_b, dim3(std::max(gA, 1u), nl), dim3(256), 0, st, dTab, dRec, dBest, dWin, P.max_hamming, dMatch, dRep);
    timer.end(t);
    VS_HIP(hipGetLastError());
    std::vector<uint8_t> hDn(dn.bytes);
    VS_HIP(pool->d2h(hDn.data(), dWk.p + oDn, dn.bytes));
    VS_HIP(pool->sync());
    if (timer.enabled) {
        const char* names[4]; float ms[4];
        const int k = timer.read(names, ms, 4);
        g_fuseTimes.clear();
        for (int q = 0; q < k; q++) g_fuseTimes.push_back({names[q], ms[q]});
    }
    for (int l = 0; l < nl; l++) {
        const vslam_fuse_lane& Q = lanes[live[l]];
        if (Q.n_a) {
            memcpy(Q.best, hDn.data() + oBest + (size_t)tab[l].a0 * 16, (size_t)Q.n_a * 16);
            memcpy(Q.match, hDn.data() + oMatch + (size_t)tab[l].a0 * 4, (size_t)Q.n_a * 4);
        }
        const int* r = (const int*)(hDn.data() + oRep) + 4 * l;
        reports[live[l]] = vslam_fuse_report{r[0], r[1], r[2], r[3]};
    }
    return VSLAM_OK;
}

}  // namespace

extern "C" vslam_status vslam_fuse_set_timing(int32_t on) {
    g_fuseTimingOn = on != 0;
    g_fuseTimes.clear();
    return VSLAM_OK;
}

extern "C" vslam_status vslam_fuse_timings(const char** names, float* ms, int32_t cap, int32_t* n_out) {
    if (!n_out || cap < 0 || (cap > 0 && (!names || !ms))) return VSLAM_ERR_INVALID;
    int n = 0;
    for (const auto& t : g_fuseTimes) { if (n >= cap) break; names[n] = t.first; ms[n] = t.second; n++; }
    *n_out = n;
    return VSLAM_OK;
}

// the one-lane case of fuse_run (its error texts name no lane)
extern "C" vslam_status vslam_fuse_search(const double* T_cw, double fx, double fy, double cx, double cy, int32_t w, int32_t h,
                                          const double* a_xyz, const uint8_t* a_desc, int32_t n_a,
                                          const double* b_xyz, const uint8_t* b_desc, int32_t n_b,
                                          const vslam_fuse_params* params, int32_t device, int32_t* match, int32_t* best, vslam_fuse_report* report) {
    static const char* const who = "vslam_fuse_search";
    if (!report || !T_cw) { set_error("%s: invalid arguments", who); return VSLAM_ERR_INVALID; }
    vslam_fuse_params P;
    VS_CHECK(fuse_check_params(who, params, P));
    const vslam_fuse_lane lane{T_cw, fx, fy, cx, cy, w, h, a_xyz, a_desc, n_a, b_xyz, b_desc, n_b, match, best};
    return fuse_run(who, false, &lane, 1, P, device, report);
}

extern "C" vslam_status vslam_fuse_search_batch(const vslam_fuse_lane* lanes, int32_t n_lanes, const vslam_fuse_params* params, int32_t device,
                                                vslam_fuse_report* reports) {
    static const char* const who = "vslam_fuse_search_batch";
    if (!lanes || !reports || n_lanes < 1) { set_error("%s: invalid arguments", who); return VSLAM_ERR_INVALID; }
    if (n_lanes > FUSE_MAX_LANES) { set_error("%s: %d lanes exceed the limit (%d)", who, n_lanes, FUSE_MAX_LANES); return VSLAM_ERR_CAPACITY; }
    vslam_fuse_params P;
    VS_CHECK(fuse_check_params(who, params, P));
    return fuse_run(who, true, lanes, n_lanes, P, device, reports);
}
