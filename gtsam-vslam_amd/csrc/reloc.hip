// Relocalisation on gfx950: recover the pose of the matcher's current stereo frame from a map WITHOUT a pose prior.
// This stage has no counterpart in the reference; its definition is the one in include/vslam_hip.h,
// restated on the CPU by tests/reloc_ref.py.
// Every call runs the same kernels over a RelocLane table, the lane as a grid dimension: vslam_relocalize, a session's call and a
// loop detection are the one-lane case of vslam_relocalize_batch / vslam_batch_relocalize (one driver: reloc_batch_run).
//   k_reloc_match_b    brute-force 256-bit Hamming search of every map point against every left key: one lane owns one map
//                      point (eight descriptor dwords in registers), a workgroup stages the frame's descriptors through LDS in
//                      tiles of 2048 (64 KB: two workgroups per CU), every lane reads the same LDS address (a broadcast);
//                      best / second-best distance, the acceptance tests, one 64-bit atomicMin per proposal
//   k_reloc_pairs_b    one workgroup: winning pairs whose key has stereo depth, compacted in ascending key index
//   k_reloc_ransac_b   one wave per hypothesis: three sampled correspondences -> rigid pose (fp64), scored over all records
//   k_reloc_best_b     one wave: the winning hypothesis and its inlier flags
//   k_reloc_problem_b  the refinement problem (the winner's inliers) built on the device, no wait before step D; refined by the
//                      motion-only LM (k_pose_lm_b, pose.hip) behind a gate
//   k_reloc_inframe_b  the lane's results into the download block; the left-image test of the map under the refined pose
// vslam_reloc_params::mode = 1 (hypotheses from 2D-3D correspondences, restated by tests/reloc_p3p_ref.py): the same bodies with
// MODE = 1 behind k_reloc_pairs_p3p_b (every winning pair, the key's unit bearing in the X_c slot), k_reloc_ransac_p3p_b (a P3P solver
// in fp64: up to four poses per hypothesis, all scored in one pass over the records) and k_reloc_best_p3p_b; k_reloc_match_b is shared.
// Stereo + IMU sessions (vslam_system_relocalize_imu, vslam_batch_relocalize_imu; restated by tests/reloc_imu_ref.py): the second of two
// relocalised poses re-initialises the velocity - the bucket between the poses through k_imu_preintegrate_b (pose_imu.hip) ahead of the
// stages, then
//   k_reloc_velocity_b  one wave per lane: the start velocity for which the IMU prediction lands on the new pose
#include "pose_dev.hpp"
#include "track_dev.hpp"
#include "imu_dev.hpp"

namespace vslam {

constexpr int RELOC_TILE = 2048;              // left keys staged per LDS tile (32 B each)
constexpr int RELOC_MAX_POINTS = 65536;
constexpr int RELOC_MAX_KEYS = 7680;          // the matcher's left-key limit (stereo staging)
constexpr int RELOC_MAX_HYP = 1024;
constexpr int RELOC_DRAWS = 16;               // sample indices tried per hypothesis

struct RelocRec {            // one correspondence: map point p <-> left key i
    double Xw[3], Xc[3];     // world position of p; key i back-projected with its depth (camera frame).  Mode 1: Xc = the key's unit bearing
    float kx, ky, kxr;       // left keypoint, x of the matched right keypoint (mode 1: 0 without the stereo flag)
    int octave, p, i;        // mode 1: octave + RELOC_STEREO_BIT with the stereo flag (estimatedDepth > 0 && rightIdxs >= 0)
};
constexpr int RELOC_STEREO_BIT = 256;
static_assert(sizeof(RelocRec) == 72, "records are downloaded as plain bytes");

__device__ __forceinline__ int hamming256(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
           __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// The rules are the bodies below; the kernels (k_*_b) hand them the arguments of a RelocLane entry, the lane being a grid dimension.
__device__ __forceinline__ void reloc_match_body(int nP, const uint4* __restrict__ descP, int nL, const uint4* __restrict__ descL,
                                                 int maxHamming, int ratioPct, int* __restrict__ dOut,
                                                 unsigned long long* __restrict__ keyWin) {
    __shared__ uint4 tile[RELOC_TILE * 2];
    const int p = blockIdx.x * 256 + threadIdx.x;
    uint4 a0 = make_uint4(0, 0, 0, 0), a1 = a0;
    if (p < nP) { a0 = descP[2 * (size_t)p]; a1 = descP[2 * (size_t)p + 1]; }
    int d1 = 257, d2 = 257, i1 = -1;
    for (int base = 0; base < nL; base += RELOC_TILE) {
        const int cnt = min(RELOC_TILE, nL - base);
        __syncthreads();                          // the previous tile has been consumed
        for (int q = threadIdx.x; q < 2 * cnt; q += 256) tile[q] = descL[2 * (size_t)base + q];
        __syncthreads();
        // ascending key index: the first key attaining d1 keeps it, a tie goes to d2.  Eight keys per trip: sixteen 16-byte LDS
        // reads are in flight before the first is consumed (a workgroup has one wave per SIMD, nothing else hides their latency)
#pragma unroll 8
        for (int k = 0; k < cnt; k++) {
            const int d = hamming256(a0, a1, tile[2 * k], tile[2 * k + 1]);
            if (d < d1) { d2 = d1; d1 = d; i1 = base + k; }
            else if (d < d2) d2 = d;
        }
    }
    if (p >= nP) return;
    dOut[3 * (size_t)p] = d1; dOut[3 * (size_t)p + 1] = i1; dOut[3 * (size_t)p + 2] = d2;
    if (i1 >= 0 && d1 <= maxHamming && 100 * d1 < ratioPct * d2)
        atomicMin(&keyWin[i1], ((unsigned long long)d1 << 32) | (unsigned)p);
}

// grid (ceil(max nP / 256), lanes).  A workgroup past its lane's points leaves as a whole, before the body's first barrier.
__global__ __launch_bounds__(256) void k_reloc_match_b(const RelocLane* __restrict__ lanes) {
    const RelocLane& L = *lane_entry(lanes, blockIdx.y);
    if ((int)(blockIdx.x * 256) >= L.nP) return;
    reloc_match_body(L.nP, L.descP, L.nL, L.descL, L.maxHamming, L.ratioPct, L.dOut, L.keyWin);
}

template <int MODE>
__device__ __forceinline__ void reloc_pairs_body(int nL, const unsigned long long* __restrict__ keyWin,
                                                 const vslam_keypoint* __restrict__ kpsL, const vslam_keypoint* __restrict__ kpsR,
                                                 const float* __restrict__ depth, const int* __restrict__ rightIdxs,
                                                 const double* __restrict__ pts, double fx, double fy, double cx, double cy,
                                                 RelocRec* __restrict__ rec, int* __restrict__ pairs, int* __restrict__ keyWinner,
                                                 int* __restrict__ out) {
    __shared__ int wsum[16];
    int run = 0;
    for (int base = 0; base < nL; base += 1024) {
        const int i = base + threadIdx.x;
        int p = -1, ri = -1;
        float z = 0.f;
        if (i < nL) {
            const unsigned long long w = keyWin[i];
            if (w != ~0ull) p = (int)(unsigned)(w & 0xFFFFFFFFull);
            keyWinner[i] = p;
            z = depth[i]; ri = rightIdxs[i];
        }
        const bool stereo = z > 0 && ri >= 0;
        const bool keep = p >= 0 && (MODE == 1 || stereo);  // mode 0: a winner on a key without depth is dropped; the key stays lost to the loser
        int tot;
        const int pos = run + block_excl_scan_1024(keep, wsum, tot);
        if (keep) {
            const vslam_keypoint k = kpsL[i];
            RelocRec r;
            r.Xw[0] = pts[3 * (size_t)p]; r.Xw[1] = pts[3 * (size_t)p + 1]; r.Xw[2] = pts[3 * (size_t)p + 2];
            if constexpr (MODE == 0) {
                const double zp = (double)z;                // back-projection exactly as k_init_map
                r.Xc[0] = ((double)k.x - cx) * zp / fx;
                r.Xc[1] = ((double)k.y - cy) * zp / fy;
                r.Xc[2] = zp;
                r.kx = k.x; r.ky = k.y; r.kxr = kpsR[ri].x;
                r.octave = k.octave; r.p = p; r.i = i;
            } else {                                        // the unit bearing of the key: ((kx - cx) / fx, (ky - cy) / fy, 1) / its norm
                const double bx = ((double)k.x - cx) / fx, by = ((double)k.y - cy) / fy;
                const double nb = sqrt((bx * bx + by * by) + 1.0);
                r.Xc[0] = bx / nb; r.Xc[1] = by / nb; r.Xc[2] = 1.0 / nb;
                r.kx = k.x; r.ky = k.y; r.kxr = stereo ? kpsR[ri].x : 0.f;
                r.octave = k.octave + (stereo ? RELOC_STEREO_BIT : 0); r.p = p; r.i = i;
            }
            rec[pos] = r;
            pairs[p] = i;
        }
        run += tot;
    }
    if (threadIdx.x == 0) out[0] = run;
}

// one workgroup per lane
__global__ __launch_bounds__(1024) void k_reloc_pairs_b(const RelocLane* __restrict__ lanes) {
    const RelocLane& L = *lane_entry(lanes, blockIdx.x);
    reloc_pairs_body<0>(L.nL, L.keyWin, L.kpsL, L.kpsR, L.depth, L.rightIdxs, L.pts, L.A.fx, L.A.fy, L.A.cx, L.A.cy, L.rec, L.pairs, L.keyWinner,
                        (int*)(L.out + 16));
}
__global__ __launch_bounds__(1024) void k_reloc_pairs_p3p_b(const RelocLane* __restrict__ lanes) {
    const RelocLane& L = *lane_entry(lanes, blockIdx.x);
    reloc_pairs_body<1>(L.nL, L.keyWin, L.kpsL, L.kpsR, L.depth, L.rightIdxs, L.pts, L.A.fx, L.A.fy, L.A.cx, L.A.cy, L.rec, L.pairs, L.keyWinner,
                        (int*)(L.out + 16));
}

__device__ __forceinline__ unsigned reloc_mix(unsigned s, unsigned h, unsigned j) {
    unsigned x = s ^ (h * 0x9E3779B9u) ^ (j * 0x85EBCA6Bu);
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return x;
}

// right-handed orthonormal frame of a point triple: e1 along P1 - P0, e3 along e1 x (P2 - P0), e2 = e3 x e1
__device__ __forceinline__ bool reloc_frame(const double* P0, const double* P1, const double* P2, double* e1, double* e2, double* e3) {
    const double a[3] = {P1[0] - P0[0], P1[1] - P0[1], P1[2] - P0[2]};
    const double na2 = a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
    if (na2 < 1e-12) return false;
    const double na = sqrt(na2);
    e1[0] = a[0] / na; e1[1] = a[1] / na; e1[2] = a[2] / na;
    const double c[3] = {P2[0] - P0[0], P2[1] - P0[1], P2[2] - P0[2]};
    const double n[3] = {e1[1] * c[2] - e1[2] * c[1], e1[2] * c[0] - e1[0] * c[2], e1[0] * c[1] - e1[1] * c[0]};
    const double nn2 = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
    if (nn2 < 1e-12) return false;
    const double nn = sqrt(nn2);
    e3[0] = n[0] / nn; e3[1] = n[1] / nn; e3[2] = n[2] / nn;
    e2[0] = e3[1] * e1[2] - e3[2] * e1[1]; e2[1] = e3[2] * e1[0] - e3[0] * e1[2]; e2[2] = e3[0] * e1[1] - e3[1] * e1[0];
    return true;
}

// hypothesis h: camera <- world pose from three sampled correspondences; false = void
__device__ __forceinline__ bool reloc_hypothesis(const RelocRec* __restrict__ rec, int C, unsigned seed, int h, DPose& T) {
    if (C < 3) return false;
    int idx[3] = {-1, -1, -1};
    int got = 0;
#pragma unroll
    for (int j = 0; j < RELOC_DRAWS; j++) {
        const int v = (int)(((unsigned long long)reloc_mix(seed, (unsigned)h, (unsigned)j) * (unsigned long long)C) >> 32);
        const bool fresh = got < 3 && v != idx[0] && v != idx[1];
        if (fresh) {                              // (written without a dynamic index: idx stays in registers)
            if (got == 0) idx[0] = v; else if (got == 1) idx[1] = v; else idx[2] = v;
            got++;
        }
    }
    if (got < 3) return false;
    const RelocRec &r0 = rec[idx[0]], &r1 = rec[idx[1]], &r2 = rec[idx[2]];
    double e1[3], e2[3], e3[3], f1[3], f2[3], f3[3];
    if (!reloc_frame(r0.Xw, r1.Xw, r2.Xw, e1, e2, e3)) return false;
    if (!reloc_frame(r0.Xc, r1.Xc, r2.Xc, f1, f2, f3)) return false;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) T.R[3 * r + c] = f1[r] * e1[c] + f2[r] * e2[c] + f3[r] * e3[c];
    double ra[3];
    mat3_vec(T.R, r0.Xw, ra);
#pragma unroll
    for (int r = 0; r < 3; r++) T.t[r] = r0.Xc[r] - ra[r];
    return true;
}

// stereo chi2 test of one correspondence under T (camera <- world): left u, left v, right u
__device__ __forceinline__ bool reloc_inlier(const RelocRec& r, const DPose& T, const PoseArgs& A, const float* lvl) {
    double pc[3];
    mat3_vec(T.R, r.Xw, pc);
#pragma unroll
    for (int k = 0; k < 3; k++) pc[k] += T.t[k];
    if (!(pc[2] > 0)) return false;
    const double pr[3] = {pc[0] - A.b, pc[1], pc[2]};
    double eu, ev, eur, evr;
    reproj_residual(pc, r.kx, r.ky, A, eu, ev);
    reproj_residual(pr, r.kxr, r.ky, A, eur, evr);
    return !((eu * eu + ev * ev + eur * eur) * (double)lvl[r.octave] > A.thres);
}

// ---- mode 1: poses from three (world point, unit bearing) pairs -------------------------------------------------------------------
// The solver of tests/reloc_p3p_ref.py, operation for operation (fp64 + - * / and sqrt, every sum and product associated as there;
// the library is built with -ffp-contract=off): the depths l along the bearings obey l^T M12 l = a12, l^T M13 l = a13,
// l^T M23 l = a23; D1 = a23 M12 - a12 M23 and D2 = a23 M13 - a13 M23 are homogeneous, a real root g of det(D1 + g D2) makes
// D0 = D1 + g D2 a pair of planes, each plane and the other conic of the pencil give a quadratic in l3 / l2.  Everything is
// wave-uniform; nothing is indexed dynamically (slots and selections are written out).
constexpr int P3P_CUBIC_STEPS = 16, P3P_REFINE_STEPS = 3;

// the sampling rule of reloc_hypothesis (that function keeps its own copy: its code object is held to the one before mode 1 existed)
__device__ __forceinline__ bool reloc_sample(int C, unsigned seed, int h, int* idx) {
    if (C < 3) return false;
    idx[0] = idx[1] = idx[2] = -1;
    int got = 0;
#pragma unroll
    for (int j = 0; j < RELOC_DRAWS; j++) {
        const int v = (int)(((unsigned long long)reloc_mix(seed, (unsigned)h, (unsigned)j) * (unsigned long long)C) >> 32);
        const bool fresh = got < 3 && v != idx[0] && v != idx[1];
        if (fresh) {
            if (got == 0) idx[0] = v; else if (got == 1) idx[1] = v; else idx[2] = v;
            got++;
        }
    }
    return got == 3;
}

struct Sym3 { double m00, m01, m02, m11, m12, m22; };

__device__ __forceinline__ Sym3 sym3_adj(const Sym3& a) {
    Sym3 r;
    r.m00 = a.m11 * a.m22 - a.m12 * a.m12; r.m01 = a.m02 * a.m12 - a.m01 * a.m22; r.m02 = a.m01 * a.m12 - a.m02 * a.m11;
    r.m11 = a.m00 * a.m22 - a.m02 * a.m02; r.m12 = a.m01 * a.m02 - a.m00 * a.m12; r.m22 = a.m00 * a.m11 - a.m01 * a.m01;
    return r;
}
__device__ __forceinline__ double sym3_tr(const Sym3& a, const Sym3& b) {      // trace(a b)
    return ((a.m00 * b.m00 + a.m11 * b.m11) + a.m22 * b.m22) + 2.0 * ((a.m01 * b.m01 + a.m02 * b.m02) + a.m12 * b.m12);
}
__device__ __forceinline__ double sq3(double x, double y, double z) { return (x * x + y * y) + z * z; }
__device__ __forceinline__ int first_max3(double a, double b, double c) {
    int k = 0; double m = a;
    if (b > m) { k = 1; m = b; }
    if (c > m) k = 2;
    return k;
}
__device__ __forceinline__ double sel3(int k, double a, double b, double c) { return k == 0 ? a : k == 1 ? b : c; }

// a real root of x^3 + b x^2 + c x + d: a start outside the stationary points, then a fixed number of Newton steps
__device__ __forceinline__ double p3p_cubic_root(double b, double c, double d) {
    const double bb = b * b, tc = 3.0 * c;
    double r;
    if (bb >= tc) {
        const double v = sqrt(bb - tc);
        const double t1 = (-b - v) / 3.0;
        double k = ((t1 + b) * t1 + c) * t1 + d;
        if (k > 0) r = t1 - sqrt(-k / (3.0 * t1 + b));
        else {
            const double t2 = (-b + v) / 3.0;
            k = ((t2 + b) * t2 + c) * t2 + d;
            r = t2 + sqrt(-k / (3.0 * t2 + b));
        }
    } else {
        r = -b / 3.0;
        const double s = (3.0 * r + 2.0 * b) * r + c;
        if ((s < 0 ? -s : s) < 1e-4) r = r + 1.0;
    }
#pragma unroll 1
    for (int it = 0; it < P3P_CUBIC_STEPS; it++) {
        const double fx = ((r + b) * r + c) * r + d;
        const double fp = (3.0 * r + 2.0 * b) * r + c;
        r = r - fx / fp;
    }
    return r;
}

struct P3PCoef { double a12, a13, a23, c12, c13, c23; };

// one root tau = l3 / l2 on the plane l1 = w0 l2 + w1 l3: the depths, polished on the three original equations; false = void
__device__ __forceinline__ bool p3p_depths(const P3PCoef& q, double w0, double w1, double tau, double& l1, double& l2, double& l3) {
    const double den = tau * (tau - 2.0 * q.c23) + 1.0;
    l2 = sqrt(q.a23 / den);
    l3 = tau * l2;
    l1 = w0 * l2 + w1 * l3;
    if (!(tau > 0 && l1 > 0)) return false;
#pragma unroll 1
    for (int it = 0; it < P3P_REFINE_STEPS; it++) {
        const double h1 = 0.5 * (((l1 * l1 + l2 * l2) - ((2.0 * q.c12) * l1) * l2) - q.a12);
        const double h2 = 0.5 * (((l1 * l1 + l3 * l3) - ((2.0 * q.c13) * l1) * l3) - q.a13);
        const double h3 = 0.5 * (((l2 * l2 + l3 * l3) - ((2.0 * q.c23) * l2) * l3) - q.a23);
        const double j11 = l1 - q.c12 * l2, j12 = l2 - q.c12 * l1;
        const double j21 = l1 - q.c13 * l3, j23 = l3 - q.c13 * l1;
        const double j32 = l2 - q.c23 * l3, j33 = l3 - q.c23 * l2;
        const double det = -((j11 * j23) * j32) - (j12 * j21) * j33;
        const double u = h2 * j33 - j23 * h3;
        const double d1 = (-(h1 * (j23 * j32)) - j12 * u) / det;
        const double d2 = (j11 * u - h1 * (j21 * j33)) / det;
        const double d3 = ((h1 * (j21 * j32) - j11 * (h2 * j32)) - j12 * (j21 * h3)) / det;
        l1 = l1 - d1; l2 = l2 - d2; l3 = l3 - d3;
    }
    const double inf = __builtin_huge_val();
    return l1 > 0 && l1 < inf && l2 > 0 && l2 < inf && l3 > 0 && l3 < inf;
}

// the pose between the world triple's frame (e1, e2, e3) and the frame of the camera points l_k y_k; false = void
__device__ __forceinline__ bool p3p_pose(const double* X0, const double* y0, const double* y1, const double* y2, const double* e1, const double* e2,
                                         const double* e3, double l1, double l2, double l3, DPose& T) {
    const double Y0[3] = {l1 * y0[0], l1 * y0[1], l1 * y0[2]}, Y1[3] = {l2 * y1[0], l2 * y1[1], l2 * y1[2]}, Y2[3] = {l3 * y2[0], l3 * y2[1], l3 * y2[2]};
    double f1[3], f2[3], f3[3];
    if (!reloc_frame(Y0, Y1, Y2, f1, f2, f3)) return false;
    const double inf = __builtin_huge_val();
    bool fin = true;
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double v = f1[r] * e1[c] + f2[r] * e2[c] + f3[r] * e3[c];
            T.R[3 * r + c] = v;
            fin = fin && v > -inf && v < inf;
        }
    }
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const double v = Y0[r] - (T.R[3 * r] * X0[0] + T.R[3 * r + 1] * X0[1] + T.R[3 * r + 2] * X0[2]);
        T.t[r] = v;
        fin = fin && v > -inf && v < inf;
    }
    return fin;
}

// the two solution slots of one plane (normal n): smaller tau first
__device__ __forceinline__ void p3p_plane(const P3PCoef& q, const Sym3& E, double n0, double n1, double n2, const double* X0, const double* y0,
                                          const double* y1, const double* y2, const double* e1, const double* e2, const double* e3,
                                          DPose& Ta, bool& oka, DPose& Tb, bool& okb) {
    oka = okb = false;
    const double w0 = -(n1 / n0), w1 = -(n2 / n0);
    const double qa = ((E.m00 * w1) * w1 + (2.0 * E.m02) * w1) + E.m22;
    const double hb = ((E.m00 * w0) * w1 + E.m01 * w1) + (E.m02 * w0 + E.m12);
    const double qc = ((E.m00 * w0) * w0 + (2.0 * E.m01) * w0) + E.m11;
    const double disc = hb * hb - qa * qc;
    if (!(disc >= 0)) return;
    const double sq = sqrt(disc);
    double l1, l2, l3;
    if (p3p_depths(q, w0, w1, (-hb - sq) / qa, l1, l2, l3)) oka = p3p_pose(X0, y0, y1, y2, e1, e2, e3, l1, l2, l3, Ta);
    if (p3p_depths(q, w0, w1, (-hb + sq) / qa, l1, l2, l3)) okb = p3p_pose(X0, y0, y1, y2, e1, e2, e3, l1, l2, l3, Tb);
}

// hypothesis h in mode 1: up to four camera <- world poses in slots 0 .. 3 (ok[s] false = void)
__device__ __forceinline__ void reloc_hypothesis_p3p(const RelocRec* __restrict__ rec, int C, unsigned seed, int h, DPose& T0, DPose& T1, DPose& T2,
                                                     DPose& T3, bool& ok0, bool& ok1, bool& ok2, bool& ok3) {
    ok0 = ok1 = ok2 = ok3 = false;
    int idx[3];
    if (!reloc_sample(C, seed, h, idx)) return;
    const RelocRec &r0 = rec[idx[0]], &r1 = rec[idx[1]], &r2 = rec[idx[2]];
    const double X0[3] = {r0.Xw[0], r0.Xw[1], r0.Xw[2]}, X1[3] = {r1.Xw[0], r1.Xw[1], r1.Xw[2]}, X2[3] = {r2.Xw[0], r2.Xw[1], r2.Xw[2]};
    const double y0[3] = {r0.Xc[0], r0.Xc[1], r0.Xc[2]}, y1[3] = {r1.Xc[0], r1.Xc[1], r1.Xc[2]}, y2[3] = {r2.Xc[0], r2.Xc[1], r2.Xc[2]};
    double e1[3], e2[3], e3[3];
    if (!reloc_frame(X0, X1, X2, e1, e2, e3)) return;                       // coincident or collinear world points
    // coincident bearings
    if (sq3(y0[1] * y1[2] - y0[2] * y1[1], y0[2] * y1[0] - y0[0] * y1[2], y0[0] * y1[1] - y0[1] * y1[0]) < 1e-12) return;
    if (sq3(y0[1] * y2[2] - y0[2] * y2[1], y0[2] * y2[0] - y0[0] * y2[2], y0[0] * y2[1] - y0[1] * y2[0]) < 1e-12) return;
    if (sq3(y1[1] * y2[2] - y1[2] * y2[1], y1[2] * y2[0] - y1[0] * y2[2], y1[0] * y2[1] - y1[1] * y2[0]) < 1e-12) return;
    P3PCoef q;
    q.a12 = sq3(X0[0] - X1[0], X0[1] - X1[1], X0[2] - X1[2]);
    q.a13 = sq3(X0[0] - X2[0], X0[1] - X2[1], X0[2] - X2[2]);
    q.a23 = sq3(X1[0] - X2[0], X1[1] - X2[1], X1[2] - X2[2]);
    q.c12 = (y0[0] * y1[0] + y0[1] * y1[1]) + y0[2] * y1[2];
    q.c13 = (y0[0] * y2[0] + y0[1] * y2[1]) + y0[2] * y2[2];
    q.c23 = (y1[0] * y2[0] + y1[1] * y2[1]) + y1[2] * y2[2];
    Sym3 D1, D2;
    D1.m00 = q.a23; D1.m01 = -(q.a23 * q.c12); D1.m02 = 0.0; D1.m11 = q.a23 - q.a12; D1.m12 = q.a12 * q.c23; D1.m22 = -q.a12;
    D2.m00 = q.a23; D2.m01 = 0.0; D2.m02 = -(q.a23 * q.c13); D2.m11 = -q.a13; D2.m12 = q.a13 * q.c23; D2.m22 = q.a23 - q.a13;
    const Sym3 A1 = sym3_adj(D1), A2 = sym3_adj(D2);
    const double k0 = (D1.m00 * A1.m00 + D1.m01 * A1.m01) + D1.m02 * A1.m02;
    const double k3 = (D2.m00 * A2.m00 + D2.m01 * A2.m01) + D2.m02 * A2.m02;
    const double k1 = sym3_tr(A1, D2), k2 = sym3_tr(A2, D1);
    const double g = p3p_cubic_root(k2 / k3, k1 / k3, k0 / k3);
    Sym3 D0;
    D0.m00 = D1.m00 + g * D2.m00; D0.m01 = D1.m01 + g * D2.m01; D0.m02 = D1.m02 + g * D2.m02;
    D0.m11 = D1.m11 + g * D2.m11; D0.m12 = D1.m12 + g * D2.m12; D0.m22 = D1.m22 + g * D2.m22;
    const Sym3 B = sym3_adj(D0);
    // adj(D0) = -p p^T: the column of the most negative diagonal entry
    const int k = first_max3(-B.m00, -B.m11, -B.m22);
    const double bm = sel3(k, B.m00, B.m11, B.m22);
    if (!(bm < 0)) return;
    const double s = sqrt(-bm);
    const double p0 = sel3(k, B.m00, B.m01, B.m02) / s, p1 = sel3(k, B.m01, B.m11, B.m12) / s, p2 = sel3(k, B.m02, B.m12, B.m22) / s;
    // N = D0 + [p]x has rank one: its rows are multiples of one plane's normal, its columns of the other's
    const double N00 = D0.m00, N01 = D0.m01 - p2, N02 = D0.m02 + p1;
    const double N10 = D0.m01 + p2, N11 = D0.m11, N12 = D0.m12 - p0;
    const double N20 = D0.m02 - p1, N21 = D0.m12 + p0, N22 = D0.m22;
    const int kr = first_max3(sq3(N00, N01, N02), sq3(N10, N11, N12), sq3(N20, N21, N22));
    const int kc = first_max3(sq3(N00, N10, N20), sq3(N01, N11, N21), sq3(N02, N12, N22));
    const double ag = g < 0 ? -g : g;
    const bool useD2 = ag <= 1.0;                                           // the conic of the pencil farther from D0
    Sym3 E;
    E.m00 = useD2 ? D2.m00 : D1.m00; E.m01 = useD2 ? D2.m01 : D1.m01; E.m02 = useD2 ? D2.m02 : D1.m02;
    E.m11 = useD2 ? D2.m11 : D1.m11; E.m12 = useD2 ? D2.m12 : D1.m12; E.m22 = useD2 ? D2.m22 : D1.m22;
    p3p_plane(q, E, sel3(kr, N00, N10, N20), sel3(kr, N01, N11, N21), sel3(kr, N02, N12, N22), X0, y0, y1, y2, e1, e2, e3, T0, ok0, T1, ok1);
    p3p_plane(q, E, sel3(kc, N00, N01, N02), sel3(kc, N10, N11, N12), sel3(kc, N20, N21, N22), X0, y0, y1, y2, e1, e2, e3, T2, ok2, T3, ok3);
}

// mode-1 chi2 test of one correspondence under T: left u, left v and, with the stereo flag, right u - against the same bound
__device__ __forceinline__ bool reloc_inlier_p3p(const double* Xw, float kx, float ky, float kxr, bool stereo, double w, const DPose& T,
                                                 const PoseArgs& A) {
    double pc[3];
    mat3_vec(T.R, Xw, pc);
#pragma unroll
    for (int k = 0; k < 3; k++) pc[k] += T.t[k];
    if (!(pc[2] > 0)) return false;
    const double pr[3] = {pc[0] - A.b, pc[1], pc[2]};
    double eu, ev, eur, evr;
    reproj_residual(pc, kx, ky, A, eu, ev);
    reproj_residual(pr, kxr, ky, A, eur, evr);
    const double val = stereo ? (eu * eu + ev * ev + eur * eur) * w : (eu * eu + ev * ev) * w;
    return !(val > A.thres);
}

template <int MODE>
__device__ __forceinline__ void reloc_ransac_body(const PoseArgs& A, const RelocRec* __restrict__ rec, const int* __restrict__ nRec,
                                                  unsigned seed, int* __restrict__ counts, double* __restrict__ poses) {
    __shared__ float sLvl[MAX_LEVELS];
    pose_stage_levels(A, sLvl);
    const int h = blockIdx.x, lane = threadIdx.x;
    const int C = *nRec;
    DPose T;
    int count = 0;
    bool valid;
    if constexpr (MODE == 0) {
        valid = reloc_hypothesis(rec, C, seed, h, T);             // (the same value in every lane)
        if (valid) {
            for (int base = 0; base < C; base += 64) {
                const int c = base + lane;
                const bool in = c < C && reloc_inlier(rec[c], T, A, sLvl);
                count += __popcll(__ballot(in));
            }
        }
    } else {
        // up to four poses, scored in ONE pass: a lane loads its record once and tests it against every valid slot
        DPose T1, T2, T3;
        bool ok0, ok1, ok2, ok3;
        reloc_hypothesis_p3p(rec, C, seed, h, T, T1, T2, T3, ok0, ok1, ok2, ok3);
        valid = ok0 || ok1 || ok2 || ok3;
        int n0 = 0, n1 = 0, n2 = 0, n3 = 0;
        if (valid) {
            for (int base = 0; base < C; base += 64) {
                const int c = base + lane;
                const bool live = c < C;
                const RelocRec& r = rec[live ? c : 0];
                const double Xw[3] = {r.Xw[0], r.Xw[1], r.Xw[2]};
                const float kx = r.kx, ky = r.ky, kxr = r.kxr;
                const int oct = r.octave;
                const bool stereo = (oct & RELOC_STEREO_BIT) != 0;
                const double w = (double)sLvl[oct & (RELOC_STEREO_BIT - 1)];
                if (ok0) n0 += __popcll(__ballot(live && reloc_inlier_p3p(Xw, kx, ky, kxr, stereo, w, T, A)));
                if (ok1) n1 += __popcll(__ballot(live && reloc_inlier_p3p(Xw, kx, ky, kxr, stereo, w, T1, A)));
                if (ok2) n2 += __popcll(__ballot(live && reloc_inlier_p3p(Xw, kx, ky, kxr, stereo, w, T2, A)));
                if (ok3) n3 += __popcll(__ballot(live && reloc_inlier_p3p(Xw, kx, ky, kxr, stereo, w, T3, A)));
            }
        }
        // the largest count over the valid slots, the lowest slot on a tie; its pose is the hypothesis's
        int bs = -1;
        count = -1;
        if (ok0 && n0 > count) { count = n0; bs = 0; }
        if (ok1 && n1 > count) { count = n1; bs = 1; }
        if (ok2 && n2 > count) { count = n2; bs = 2; }
        if (ok3 && n3 > count) { count = n3; bs = 3; }
        if (bs < 0) count = 0;
#pragma unroll
        for (int k = 0; k < 9; k++) T.R[k] = bs == 1 ? T1.R[k] : bs == 2 ? T2.R[k] : bs == 3 ? T3.R[k] : T.R[k];
#pragma unroll
        for (int k = 0; k < 3; k++) T.t[k] = bs == 1 ? T1.t[k] : bs == 2 ? T2.t[k] : bs == 3 ? T3.t[k] : T.t[k];
    }
    if (lane == 0) {
        counts[h] = count;
        double* o = poses + 12 * (size_t)h;
        for (int k = 0; k < 9; k++) o[k] = valid ? T.R[k] : 0.0;
        for (int k = 0; k < 3; k++) o[9 + k] = valid ? T.t[k] : 0.0;
    }
}

// grid (hypotheses, lanes)
__global__ __launch_bounds__(64) void k_reloc_ransac_b(const RelocLane* __restrict__ lanes) {
    const RelocLane& L = *lane_entry(lanes, blockIdx.y);
    reloc_ransac_body<0>(L.A, L.rec, (const int*)(L.out + 16), L.seed, L.counts, L.poses);
}
__global__ __launch_bounds__(64) void k_reloc_ransac_p3p_b(const RelocLane* __restrict__ lanes) {
    const RelocLane& L = *lane_entry(lanes, blockIdx.y);
    reloc_ransac_body<1>(L.A, L.rec, (const int*)(L.out + 16), L.seed, L.counts, L.poses);
}

template <int MODE>
__device__ __forceinline__ void reloc_best_body(const PoseArgs& A, const RelocRec* __restrict__ rec, int nHyp, const int* __restrict__ counts,
                                                const double* __restrict__ poses, double* __restrict__ out, uint8_t* __restrict__ flags) {
    __shared__ float sLvl[MAX_LEVELS];
    pose_stage_levels(A, sLvl);
    const int lane = threadIdx.x;
    int* outI = (int*)(out + 16);
    const int C = outI[0];
    unsigned long long best = 0;                  // (count << 32 | 0xFFFFFFFF - h): the lowest h wins a tie
    for (int h = lane; h < nHyp; h += 64) {
        const unsigned long long v = ((unsigned long long)(unsigned)counts[h] << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)h);
        best = v > best ? v : best;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(best, d);
        best = o > best ? o : best;
    }
    const int bh = (int)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull));
    const int bc = (int)(best >> 32);
    DPose T;
    const double* o = poses + 12 * (size_t)bh;
#pragma unroll
    for (int k = 0; k < 9; k++) T.R[k] = o[k];
#pragma unroll
    for (int k = 0; k < 3; k++) T.t[k] = o[9 + k];
    for (int c = lane; c < C; c += 64) {
        if constexpr (MODE == 0) flags[c] = bc > 0 && reloc_inlier(rec[c], T, A, sLvl) ? 1 : 0;
        else {
            const RelocRec& r = rec[c];
            const int oct = r.octave;
            flags[c] = bc > 0 && reloc_inlier_p3p(r.Xw, r.kx, r.ky, r.kxr, (oct & RELOC_STEREO_BIT) != 0, (double)sLvl[oct & (RELOC_STEREO_BIT - 1)], T, A) ? 1 : 0;
        }
    }
    if (lane == 0) {
        pose_to_rm16(T, out);
        outI[1] = bh; outI[2] = bc;
    }
}

// one wave per lane
__global__ __launch_bounds__(64) void k_reloc_best_b(const RelocLane* __restrict__ lanes) {
    const RelocLane& L = *lane_entry(lanes, blockIdx.x);
    reloc_best_body<0>(L.A, L.rec, L.nHyp, L.counts, L.poses, L.out, L.flags);
}
__global__ __launch_bounds__(64) void k_reloc_best_p3p_b(const RelocLane* __restrict__ lanes) {
    const RelocLane& L = *lane_entry(lanes, blockIdx.x);
    reloc_best_body<1>(L.A, L.rec, L.nHyp, L.counts, L.poses, L.out, L.flags);
}

// The refinement problem of a lane: the winner's inlier correspondences, in correspondence order, into the lane's matcher's pose buffers - points = X_w, matches = (i, rightIdxs[i]), both in-frame flags 1,
// both outlier flags 0, poseIO = the winning hypothesis - and the two words the pose kernel reads on the device: the problem size
// (PoseArgs::Mdev) and the gate (0: fewer than three correspondences or no inlier, the lane is not refined).  One workgroup per lane.
__global__ __launch_bounds__(1024) void k_reloc_problem_b(const RelocLane* __restrict__ lanes) {
    __shared__ int wsum[16];
    const RelocLane& L = *lane_entry(lanes, blockIdx.x);
    int* outI = (int*)(L.out + 16);
    const int C = outI[0];
    const bool go = !(C < 3 || outI[2] <= 0);
    int run = 0;
    if (go) {
        const size_t fs = L.flagStride;
        for (int base = 0; base < C; base += 1024) {
            const int c = base + threadIdx.x;
            const bool keep = c < C && L.flags[c];
            int tot;
            const int pos = run + block_excl_scan_1024(keep, wsum, tot);
            if (keep) {
                const RelocRec& r = L.rec[c];
                L.probPoints[3 * (size_t)pos] = r.Xw[0]; L.probPoints[3 * (size_t)pos + 1] = r.Xw[1]; L.probPoints[3 * (size_t)pos + 2] = r.Xw[2];
                L.A.matches[2 * pos] = r.i; L.A.matches[2 * pos + 1] = L.rightIdxs[r.i];
                L.probFlags[pos] = 1; L.probFlags[fs + pos] = 1; L.probFlags[2 * fs + pos] = 0; L.probFlags[3 * fs + pos] = 0;
            }
            run += tot;
        }
    }
    if (threadIdx.x < 16 && go) L.A.poseIO[threadIdx.x] = L.out[threadIdx.x];
    if (threadIdx.x == 0) { outI[3] = run; outI[4] = go ? 1 : 0; }
}

// Grid (ceil(max nP / 256), lanes).  The lane's results go to its summary slice (workgroup 0); for a lane whose refined inlier count
// reaches min_inliers, the left-camera worldToFrame test of every uploaded map point under the refined pose: one byte per point.
__global__ __launch_bounds__(256) void k_reloc_inframe_b(const RelocLane* __restrict__ lanes) {
    const RelocLane& L = *lane_entry(lanes, blockIdx.y);
    const int* outI = (const int*)(L.out + 16);
    const int gate = outI[4];
    const int nIn = gate ? L.A.out[0] : 0;
    const bool success = gate && nIn >= L.minInliers;
    if (blockIdx.x == 0) {
        const int t = threadIdx.x;
        if (t < 16) L.summary[t] = gate ? L.A.poseIO[t] : L.out[t];
        else if (t < 19) L.summary[t] = gate ? L.A.poseIO[t] : 0.0;
        else if (t == 19) {
            int* sI = (int*)(L.summary + RELOC_SUM_INTS);
            sI[0] = outI[0]; sI[1] = outI[1]; sI[2] = outI[2]; sI[3] = outI[3]; sI[4] = gate;
            sI[5] = nIn; sI[6] = gate ? L.A.out[1] : 0; sI[7] = gate ? L.A.out[2] : 0; sI[8] = gate ? L.A.out[3] : 0; sI[9] = success ? 1 : 0;
        }
    }
    if (!success || !L.inF) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= L.nP) return;
    DPose T;
    pose_from_rm16(L.A.poseIO, T);
    const double p[3] = {L.pts[3 * (size_t)i], L.pts[3 * (size_t)i + 1], L.pts[3 * (size_t)i + 2]};
    double pc[3];
    mat3_vec(T.R, p, pc);
#pragma unroll
    for (int k = 0; k < 3; k++) pc[k] += T.t[k];
    float uo, vo; int lvl;
    L.inF[i] = world_to_frame_cam(pc[0], pc[1], pc[2], L.A.fx, L.A.fy, L.A.cx, L.A.cy, L.w, L.h, L.msd + i, L.logScale, L.nLev, uo, vo, lvl) ? 1 : 0;
}

// Phase 2 of an IMU relocalisation (restated by tests/reloc_imu_ref.py): the velocity from two relocalised
// poses.  Tcw: the refined camera <- world pose (row-major 4x4); pim / pred: the bucket between the poses, pre-integrated with biasGood
// and predicted from (T_prev, v = 0, biasGood) by k_imu_preintegrate_b.  One wave; every value is formed by one lane in a written order:
//   T_new = (R^T, -R^T t):   t_new[i] = -((R[0][i] t[0] + R[1][i] t[1]) + R[2][i] t[2])
//   lane i < 3:   velocity_prev[i] = (t_new[i] - pred.t[i]) / dt,   velocity[i] = pred.v[i] + velocity_prev[i]
//   lane 3:       rot_residual = sqrt of the sum, in row-major order, of (pred.R[r][c] - R[c][r])^2
// out[8]: dt, velocity_prev, velocity, rot_residual.
__device__ __forceinline__ void reloc_velocity_body(const double* __restrict__ Tcw, const double* __restrict__ pim, const double* __restrict__ pred,
                                                    double* __restrict__ out) {
    const int i = threadIdx.x;
    const double dt = pim[0];
    if (i < 3) {
        const double tn = -((Tcw[i] * Tcw[3] + Tcw[4 + i] * Tcw[7]) + Tcw[8 + i] * Tcw[11]);
        const double vp = (tn - pred[9 + i]) / dt;
        out[1 + i] = vp;
        out[4 + i] = pred[12 + i] + vp;
    } else if (i == 3) {
        double s = 0.0;
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const double d = pred[3 * r + c] - Tcw[4 * c + r];
                s = s + d * d;
            }
        out[7] = sqrt(s);
        out[0] = dt;
    }
}

// One wave per lane, after k_reloc_inframe_b.  A lane without a pre-integrated bucket (phase 1) leaves at once; the pre-integration's
// status goes to the summary whatever the relocalisation gave; the rule runs behind the success word k_reloc_inframe_b tests.
__global__ __launch_bounds__(64) void k_reloc_velocity_b(const RelocLane* __restrict__ lanes) {
    const RelocLane& L = *lane_entry(lanes, blockIdx.x);
    if (!L.velPim) return;
    if (threadIdx.x == 0) ((int*)(L.summary + RELOC_SUM_INTS))[10] = *L.velStatus != 0.0 ? 1 : 0;
    const int* outI = (const int*)(L.out + 16);
    const int gate = outI[4];
    const int nIn = gate ? L.A.out[0] : 0;
    if (!(gate && nIn >= L.minInliers)) return;
    reloc_velocity_body(L.A.poseIO, L.velPim, L.velPred, L.summary + RELOC_SUM_VEL);
}

}  // namespace vslam

using namespace vslam;

vslam_status vslam_matcher::ensure_reloc_cap(int n) {
    if (!d_rlKeyWinner) {
        VS_HIP(poison_malloc(&d_rlKeyWinner, (size_t)RELOC_MAX_KEYS * sizeof(int)));
        VS_HIP(poison_malloc(&d_rlRec, (size_t)RELOC_MAX_KEYS * sizeof(RelocRec)));
        VS_HIP(poison_malloc(&d_rlFlags, (size_t)RELOC_MAX_KEYS));
        VS_HIP(poison_malloc(&d_rlCounts, (size_t)RELOC_MAX_HYP * sizeof(int)));
        VS_HIP(poison_malloc(&d_rlPoses, (size_t)RELOC_MAX_HYP * 12 * sizeof(double)));
        VS_HIP(poison_malloc(&d_rlOut, 20 * sizeof(double)));
    }
    if (n > rlDCap) {                                  // (map points, pairs and key winners live in the call's upload / download blocks)
        hipFree(d_rlD);
        d_rlD = nullptr; rlDCap = 0;
        const int cap2 = vslam::align_up(std::max(n, 1), 1024);
        VS_HIP(poison_malloc(&d_rlD, (size_t)cap2 * 3 * sizeof(int)));
        rlDCap = cap2;
    }
    return VSLAM_OK;
}

// a zero field takes its default; the ranges of vslam_hip.h
vslam_status vslam::reloc_resolve_params(const vslam_reloc_params* prm, vslam_reloc_params& P) {
    P = prm ? *prm : vslam_reloc_params{};
    if (!P.max_hamming) P.max_hamming = 50;
    if (!P.ratio_pct) P.ratio_pct = 80;
    if (!P.n_hypotheses) P.n_hypotheses = 256;
    if (!P.seed) P.seed = 0x52454C4Fu;
    if (!P.min_inliers) P.min_inliers = 50;
    if (P.max_hamming < 0 || P.max_hamming > 256 || P.ratio_pct < 0 || P.ratio_pct > 100 || P.n_hypotheses < 1 || P.n_hypotheses > RELOC_MAX_HYP ||
        P.min_inliers < 0) {
        set_error("relocalize: parameters out of range (max_hamming 0..256, ratio_pct 0..100, n_hypotheses 1..%d, min_inliers >= 0)", RELOC_MAX_HYP);
        return VSLAM_ERR_INVALID;
    }
    if (P.mode != 0 && P.mode != 1) {
        set_error("relocalize: mode %d (0: hypotheses from stereo-triangulated keys, 1: from 2D-3D correspondences)", P.mode);
        return VSLAM_ERR_INVALID;
    }
    return VSLAM_OK;
}

vslam_status vslam_matcher::relocalize_debug(int32_t* d3, int capPoints, int32_t* keyWinner, int capKeys, int32_t* counts, int capHyp,
                                             uint8_t* flags, int capPairs, int32_t* sizes4) {
    const int n = rlLast[0], nL = rlLast[1], H = rlLast[2], C = rlLast[3];
    if (sizes4) for (int k = 0; k < 4; k++) sizes4[k] = rlLast[k];
    if ((d3 && capPoints < n) || (keyWinner && capKeys < nL) || (counts && capHyp < H) || (flags && capPairs < C)) {
        set_error("relocalize_debug: capacity"); return VSLAM_ERR_CAPACITY;
    }
    if (!d_rlKeyWinner) return VSLAM_OK;                    // no call yet: all sizes 0
    VS_HIP(hipSetDevice(device));
    if (d3 && n) VS_HIP(hipMemcpyAsync(d3, d_rlD, (size_t)n * 12, hipMemcpyDeviceToHost, stream));
    if (keyWinner && nL) VS_HIP(hipMemcpyAsync(keyWinner, d_rlKeyWinner, (size_t)nL * 4, hipMemcpyDeviceToHost, stream));
    if (counts && H) VS_HIP(hipMemcpyAsync(counts, d_rlCounts, (size_t)H * 4, hipMemcpyDeviceToHost, stream));
    if (flags && C) VS_HIP(hipMemcpyAsync(flags, d_rlFlags, (size_t)C, hipMemcpyDeviceToHost, stream));
    VS_HIP(hipStreamSynchronize(stream));
    return VSLAM_OK;
}

// ---- the driver of every call: checks, block layout, the stages once for all lanes ------------------------------------------------------
namespace vslam {
void launch_pose_batch(hipStream_t s, const PoseLane* dLanes, int B);
void launch_imu_batch(hipStream_t s, const ImuLane* dLanes, int B);
}

namespace {
inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// the subject of a refusal, in the wording of vslam_system::reloc_imu_check: a call of several lanes names the lane, a single call none
struct RelocWho {
    char s[48];
    RelocWho(bool nameLanes, int lane) {
        if (nameLanes) snprintf(s, sizeof(s), "relocalize_batch: lane %d: ", lane);
        else snprintf(s, sizeof(s), "relocalize: ");
    }
};
}

vslam_status vslam::reloc_batch_check(const RelocBatchLane* lanes, int B, int device, bool nameLanes) {
    for (int b = 0; b < B; b++) {
        const vslam_matcher* m = lanes[b].m;
        if (!m) continue;
        const RelocWho who(nameLanes, b);
        if (m->mono) { set_error("%sa mono matcher", who.s); return VSLAM_ERR_INVALID; }
        if (m->device != device) { set_error("%sthe matcher is on device %d, the first lane's on %d", who.s, m->device, device); return VSLAM_ERR_INVALID; }
        if (!m->stereoDone) { set_error("%sa completed stereo match is needed", who.s); return VSLAM_ERR_INVALID; }
        if (lanes[b].n < 0) { set_error("%sinvalid arguments", who.s); return VSLAM_ERR_INVALID; }
        for (int a = 0; a < b; a++)
            if (lanes[a].m == m) { set_error("relocalize_batch: lanes %d and %d are the same matcher", a, b); return VSLAM_ERR_INVALID; }
    }
    for (int b = 0; b < B; b++)
        if (lanes[b].m && lanes[b].n > RELOC_MAX_POINTS) {
            set_error("%s%d map points exceed the limit (%d)", RelocWho(nameLanes, b).s, lanes[b].n, RELOC_MAX_POINTS);
            return VSLAM_ERR_CAPACITY;
        }
    return VSLAM_OK;
}

void vslam::reloc_batch_plan(RelocBatchLane* lanes, int B, RelocBatchPlan& plan) {
    plan = RelocBatchPlan{};
    size_t up = up256((size_t)B * sizeof(RelocLane));
    plan.oPose = up;
    up = up256(up + (size_t)B * sizeof(PoseLane));
    for (int b = 0; b < B; b++) if (lanes[b].m && lanes[b].imu) plan.nImu++;
    if (plan.nImu) { plan.oImuTab = up; up = up256(up + (size_t)B * sizeof(ImuLane)); }
    size_t dn = 0;
    for (int b = 0; b < B; b++) {
        RelocBatchLane& q = lanes[b];
        if (!q.m) continue;
        plan.nOn++;
        plan.maxN = std::max(plan.maxN, q.n);
        if (q.imu) { q.oImu = up; up += up256((size_t)(7 * std::max(q.imu->n_samples, 0) + 6) * sizeof(double)); }
        q.oXyz = up; up += up256((size_t)q.n * 24);
        q.oDesc = up; up += up256((size_t)q.n * 32);
        q.oMsd = up; if (q.wantInFrame) up += up256((size_t)q.n * 4);
        q.oSum = dn; dn += up256(RELOC_SUM_DOUBLES * sizeof(double));
        q.oPairs = dn; dn += up256((size_t)q.n * 4);
        q.oInF = dn; if (q.wantInFrame) dn += up256((size_t)q.n);
    }
    plan.upCopyBytes = up;
    for (int b = 0; b < B; b++) if (lanes[b].m) { lanes[b].oKeyWin = up; up += up256((size_t)RELOC_MAX_KEYS * sizeof(unsigned long long)); }
    plan.upBytes = up; plan.dnBytes = dn;
}

vslam_status vslam::reloc_batch_run(RelocBatchLane* lanes, int B, const RelocBatchPlan& plan, const RelocBlocks& blk, hipStream_t stream,
                                    const vslam_reloc_params& P, double logScale, StageTimer* tm, double* T_cw_out, vslam_reloc_report* reps,
                                    vslam_reloc_imu_report* imuReps, bool nameLanes) {
    if (!plan.nOn) return VSLAM_OK;
    if (plan.nImu && !imuReps) { set_error("relocalize_batch: a lane carries an IMU bucket but no report array was given"); return VSLAM_ERR_INVALID; }
    const int H = P.n_hypotheses, nOn = plan.nOn;
    // ---- the frames' keys: this stream after the extractors' last run; limits; capacities (all before the first launch) ----------
    std::vector<vslam_extractor*> seen;
    for (int b = 0; b < B; b++) {
        vslam_matcher* m = lanes[b].m;
        if (!m) continue;
        for (vslam_extractor* fe : {m->feL, m->feR}) {
            if (!fe || std::find(seen.begin(), seen.end(), fe) != seen.end()) continue;
            seen.push_back(fe);
            if (fe->evDone) VS_HIP(hipStreamWaitEvent(stream, fe->evDone, 0));
        }
        VS_CHECK(m->refresh_keys(false));
        lanes[b].nL = m->nKeys[0];
        if (lanes[b].nL > RELOC_MAX_KEYS) {
            set_error("%s%d left keypoints exceed the limit (%d)", RelocWho(nameLanes, b).s, lanes[b].nL, RELOC_MAX_KEYS);
            return VSLAM_ERR_CAPACITY;
        }
    }
    for (int b = 0; b < B; b++) {
        vslam_matcher* m = lanes[b].m;
        if (!m) continue;
        VS_CHECK(m->ensure_reloc_cap(lanes[b].n));
        VS_CHECK(m->ensure_pose_cap(std::max(lanes[b].nL, 1)));      // the refinement: at most one factor per left key
        VS_CHECK(m->ensure_proj_cap(std::max(lanes[b].nL, 1)));
    }
    // ---- lane tables (active lanes only: entry k of both tables is the k-th active lane) -----------------------------------------
    RelocLane* hT = (RelocLane*)blk.h_up;
    PoseLane* hP = (PoseLane*)(blk.h_up + plan.oPose);
    const RelocLane* dT = (const RelocLane*)blk.d_up;
    const PoseLane* dP = (const PoseLane*)(blk.d_up + plan.oPose);
    ImuLane* hI = (ImuLane*)(blk.h_up + plan.oImuTab);      // (read only when a lane carries a bucket)
    const ImuLane* dI = (const ImuLane*)(blk.d_up + plan.oImuTab);
    int k = 0;
    for (int b = 0; b < B; b++) {
        const RelocBatchLane& q = lanes[b];
        vslam_matcher* m = q.m;
        if (!m) continue;
        RelocLane& L = hT[k];
        L = RelocLane{};
        L.nP = q.n; L.nL = q.nL;
        L.descP = (const uint4*)(blk.d_up + q.oDesc); L.descL = (const uint4*)m->d_desc[0];
        L.pts = (const double*)(blk.d_up + q.oXyz); L.msd = q.wantInFrame ? (const float*)(blk.d_up + q.oMsd) : nullptr;
        L.maxHamming = P.max_hamming; L.ratioPct = P.ratio_pct; L.nHyp = H; L.minInliers = P.min_inliers; L.seed = P.seed;
        L.dOut = m->d_rlD; L.keyWin = (unsigned long long*)(blk.d_up + q.oKeyWin); L.keyWinner = m->d_rlKeyWinner;
        L.pairs = (int*)(blk.d_dn + q.oPairs);
        L.kpsL = m->d_kps[0]; L.kpsR = m->d_kps[1]; L.depth = m->d_depth; L.rightIdxs = m->d_rightIdxs;
        L.rec = (RelocRec*)m->d_rlRec; L.flags = m->d_rlFlags; L.counts = m->d_rlCounts; L.poses = m->d_rlPoses; L.out = m->d_rlOut;
        int* outI = (int*)(m->d_rlOut + 16);
        m->pose_lane(L.A, std::max(q.nL, 1), outI + 3, outI + 4, 1, 0, 0);      // problem size and gate: written by k_reloc_problem_b
        L.probPoints = m->d_points; L.probFlags = m->d_flags; L.flagStride = (size_t)m->poseCap;
        L.w = m->rig.width; L.h = m->rig.height; L.nLev = m->feL->nLevels; L.logScale = logScale;
        L.inF = q.wantInFrame ? blk.d_dn + q.oInF : nullptr;
        L.summary = (double*)(blk.d_dn + q.oSum);
        hP[k] = PoseLane{};
        hP[k].A = L.A;
        if (plan.nImu) {
            // the pre-integration's entry of this lane: idle (n = 0) without a bucket; with one, staged as a tracked IMU step stages it
            // (dt rule, dt0 = 1 / hz, integration bias = bias_prev) and predicted from (T_wc_prev, v = 0).  Its outputs live in the
            // matcher's IMU scratch; the status word in the spare slot behind the prediction.
            ImuLane& I = hI[k];
            I = ImuLane{};
            if (q.imu) {
                VS_CHECK(m->imu_stage(q.imu, 0.0, (double*)(blk.h_up + q.oImu), (double*)(blk.d_up + q.oImu), I));
                for (int c = 0; c < 3; c++) I.si.v[c] = 0.0;
                I.takeFrom = nullptr;
                I.status = m->imuPred + sizeof(DNav) / sizeof(double);
                L.velPim = (const double*)I.pim; L.velPred = (const double*)I.pred; L.velStatus = I.status;
                // (the staged views point into the caller's upload block: nothing may run on them after this call)
                m->imuSamplesDev = nullptr; m->imuBiasDev = nullptr; m->imuN = 0;
            }
        }
        m->rlLast[0] = q.n; m->rlLast[1] = q.nL; m->rlLast[2] = H; m->rlLast[3] = 0;
        k++;
    }
    // ---- one upload, the stages once for all lanes, one download, one wait ---------------------------------------------------------
    VS_HIP(hipMemcpyAsync(blk.d_up, blk.h_up, plan.upCopyBytes, hipMemcpyHostToDevice, stream));
    VS_HIP(hipMemsetAsync(blk.d_up + plan.upCopyBytes, 0xFF, plan.upBytes - plan.upCopyBytes, stream));      // key winners: none
    VS_HIP(hipMemsetAsync(blk.d_dn, 0xFF, plan.dnBytes, stream));                                              // pairs: -1
    const int gx = (plan.maxN + 255) / 256;
    StageTimer off; off.enabled = false;
    StageTimer& T = tm ? *tm : off;
    int t;
    if (plan.nImu) {                                // the phase-2 lanes' buckets: independent of the stages below, ahead of them
        t = T.begin("reloc_preintegrate");
        launch_imu_batch(stream, dI, nOn);
        T.end(t);
    }
    t = T.begin("reloc_match");
    if (gx) hipLaunchKernelGGL(k_reloc_match_b, dim3(gx, nOn), dim3(256), 0, stream, dT);
    T.end(t);
    t = T.begin("reloc_pairs");
    hipLaunchKernelGGL(P.mode ? k_reloc_pairs_p3p_b : k_reloc_pairs_b, dim3(nOn), dim3(1024), 0, stream, dT);
    T.end(t);
    t = T.begin("reloc_ransac");
    hipLaunchKernelGGL(P.mode ? k_reloc_ransac_p3p_b : k_reloc_ransac_b, dim3(H, nOn), dim3(64), 0, stream, dT);
    hipLaunchKernelGGL(P.mode ? k_reloc_best_p3p_b : k_reloc_best_b, dim3(nOn), dim3(64), 0, stream, dT);
    T.end(t);
    t = T.begin("reloc_refine");
    hipLaunchKernelGGL(k_reloc_problem_b, dim3(nOn), dim3(1024), 0, stream, dT);
    launch_pose_batch(stream, dP, nOn);
    T.end(t);
    t = T.begin("reloc_inframe");
    hipLaunchKernelGGL(k_reloc_inframe_b, dim3(std::max(gx, 1), nOn), dim3(256), 0, stream, dT);
    T.end(t);
    if (plan.nImu) {
        t = T.begin("reloc_velocity");
        hipLaunchKernelGGL(k_reloc_velocity_b, dim3(nOn), dim3(64), 0, stream, dT);
        T.end(t);
    }
    VS_HIP(hipGetLastError());
    VS_HIP(hipMemcpyAsync(blk.h_dn, blk.d_dn, plan.dnBytes, hipMemcpyDeviceToHost, stream));
    VS_HIP(hipStreamSynchronize(stream));
    int noFactor = -1;
    for (int b = 0; b < B; b++) {
        const RelocBatchLane& q = lanes[b];
        if (!q.m) continue;
        const double* s = (const double*)(blk.h_dn + q.oSum);
        const int* sI = (const int*)(s + RELOC_SUM_INTS);
        vslam_reloc_report& r = reps[b];
        r = vslam_reloc_report{};
        r.n_points = q.n; r.n_pairs = sI[0]; r.best_hypothesis = sI[1]; r.best_count = sI[2];
        q.m->rlLast[3] = sI[0];
        if (q.imu) {
            imuReps[b] = vslam_reloc_imu_report{};
            if (sI[10] && noFactor < 0) noFactor = b;
        }
        if (!sI[4]) continue;                               // fewer than three correspondences or no inlier: not refined, success = 0
        r.n_inliers = sI[5]; r.n_stereo = sI[6];
        r.lm.iterations = sI[7]; r.lm.inner_iterations = sI[8]; r.lm.initial_error = s[16]; r.lm.final_error = s[17]; r.lm.lambda = s[18];
        r.success = sI[9];
        if (r.success) memcpy(T_cw_out + 16 * (size_t)b, s, 16 * sizeof(double));
        if (q.imu && r.success) {
            vslam_reloc_imu_report& v = imuReps[b];
            const double* o = s + RELOC_SUM_VEL;
            v.phase = 2; v.dt = o[0]; v.rot_residual = o[7];
            for (int c = 0; c < 3; c++) { v.velocity_prev[c] = o[1 + c]; v.velocity[c] = o[4 + c]; }
        }
    }
    if (noFactor >= 0) {
        set_error("%sIMU pre-integration: the 15x15 covariance has no Cholesky factor (no information matrix, no IMU factor)", RelocWho(nameLanes, noFactor).s);
        return VSLAM_ERR_INVALID;
    }
    return VSLAM_OK;
}

vslam_status vslam::reloc_own_blocks(vslam_matcher* m, size_t upBytes, size_t dnBytes) {
    const size_t need[2] = {std::max<size_t>(upBytes, 256), std::max<size_t>(dnBytes, 256)};
    for (int k = 0; k < 2; k++) {
        if (need[k] <= m->rlBlkCap[k]) continue;
        VS_HIP(hipStreamSynchronize(m->stream));
        if (m->rlBlk[2 * k]) hipHostFree(m->rlBlk[2 * k]);
        hipFree(m->rlBlk[2 * k + 1]);
        m->rlBlk[2 * k] = m->rlBlk[2 * k + 1] = nullptr; m->rlBlkCap[k] = 0;
        const size_t cap = need[k] + need[k] / 2;
        VS_HIP(hipHostMalloc((void**)&m->rlBlk[2 * k], cap, hipHostMallocDefault));
        VS_HIP(hipMalloc((void**)&m->rlBlk[2 * k + 1], cap));
        m->rlBlkCap[k] = cap;
    }
    return VSLAM_OK;
}

// Test tap of the velocity rule: B buckets through ONE k_imu_preintegrate_b launch, then ONE k_reloc_velocity_b launch over a RelocLane
// table whose entries hold what the kernel reads - the pose where step D leaves it, an open gate, the pre-integration's outputs.  Everything lives in one temporary block; the rows of `out` are uploaded
// first, so an idle lane's row comes back as the caller filled it.
static vslam_status reinit_velocity_tap(vslam_matcher* m, int B, const vslam_imu_input* imus, const double* Tcw, double* out) {
    if (!m || B <= 0 || !imus || !Tcw || !out) { set_error("IMU velocity tap: invalid arguments"); return VSLAM_ERR_INVALID; }
    for (int b = 0; b < B; b++)
        if (imus[b].n_samples < 0) { set_error("IMU velocity tap: lane %d: bucket length %d", b, imus[b].n_samples); return VSLAM_ERR_INVALID; }
    VS_HIP(hipSetDevice(m->device));
    constexpr size_t PD = sizeof(DPim) / sizeof(double), ND = sizeof(DNav) / sizeof(double);
    // per lane (doubles): poseIO 32 | out 20 | pose-kernel ints 2 | summary | DPim | Lam 225 | DNav | status 1 | samples 7 n + 6
    constexpr size_t O_OUT = 32, O_INTS = 52, O_SUM = 54, O_PIM = O_SUM + RELOC_SUM_DOUBLES, O_LAM = O_PIM + PD, O_PRED = O_LAM + 225, O_ST = O_PRED + ND,
                     O_SMP = O_ST + 1;
    std::vector<size_t> off(B + 1, 0);
    for (int b = 0; b < B; b++) off[b + 1] = off[b] + O_SMP + 7 * (size_t)imus[b].n_samples + 6;
    std::vector<double> h(off[B], 0.0);
    std::vector<RelocLane> rl((size_t)B);
    std::vector<ImuLane> il((size_t)B);
    double* d = nullptr; RelocLane* dR = nullptr; ImuLane* dI = nullptr;
    auto run = [&]() -> vslam_status {
        VS_HIP(hipMalloc(&d, off[B] * sizeof(double)));
        VS_HIP(hipMalloc(&dR, (size_t)B * sizeof(RelocLane)));
        VS_HIP(hipMalloc(&dI, (size_t)B * sizeof(ImuLane)));
        for (int b = 0; b < B; b++) {
            double* hb = h.data() + off[b];
            double* db = d + off[b];
            memcpy(hb, Tcw + 16 * (size_t)b, 16 * sizeof(double));
            ((int*)(hb + O_OUT + 16))[4] = 1;                                   // the gate: open; inliers 0 >= min_inliers 0
            memcpy(hb + O_SUM + RELOC_SUM_VEL, out + 8 * (size_t)b, 8 * sizeof(double));
            RelocLane& L = rl[b];
            L = RelocLane{};
            ImuLane& I = il[b];
            I = ImuLane{};
            L.out = db + O_OUT; L.A.poseIO = db; L.A.out = (int*)(db + O_INTS); L.minInliers = 0; L.summary = db + O_SUM;
            if (imus[b].n_samples == 0) continue;                               // idle lane: both kernels leave at their first test
            VS_CHECK(m->imu_stage(&imus[b], 0.0, hb + O_SMP, db + O_SMP, I));
            for (int c = 0; c < 3; c++) I.si.v[c] = 0.0;
            I.takeFrom = nullptr;
            I.pim = (DPim*)(db + O_PIM); I.Lam = db + O_LAM; I.pred = (DNav*)(db + O_PRED); I.status = db + O_ST;
            L.velPim = db + O_PIM; L.velPred = db + O_PRED; L.velStatus = db + O_ST;
        }
        hipStream_t st = m->stream;
        VS_HIP(hipMemcpyAsync(d, h.data(), off[B] * sizeof(double), hipMemcpyHostToDevice, st));
        VS_HIP(hipMemcpyAsync(dR, rl.data(), (size_t)B * sizeof(RelocLane), hipMemcpyHostToDevice, st));
        VS_HIP(hipMemcpyAsync(dI, il.data(), (size_t)B * sizeof(ImuLane), hipMemcpyHostToDevice, st));
        launch_imu_batch(st, dI, B);
        hipLaunchKernelGGL(k_reloc_velocity_b, dim3(B), dim3(64), 0, st, (const RelocLane*)dR);
        VS_HIP(hipGetLastError());
        VS_HIP(hipMemcpyAsync(h.data(), d, off[B] * sizeof(double), hipMemcpyDeviceToHost, st));
        VS_HIP(hipStreamSynchronize(st));
        return VSLAM_OK;
    };
    const vslam_status rs = run();
    hipFree(d); hipFree(dR); hipFree(dI);
    m->imuSamplesDev = nullptr; m->imuBiasDev = nullptr; m->imuN = 0;      // (the staged views pointed into the temporary block)
    if (rs != VSLAM_OK) return rs;
    int bad = -1;
    for (int b = 0; b < B; b++) {
        const double* hb = h.data() + off[b];
        memcpy(out + 8 * (size_t)b, hb + O_SUM + RELOC_SUM_VEL, 8 * sizeof(double));
        if (imus[b].n_samples > 0 && hb[O_ST] != 0.0 && bad < 0) bad = b;
    }
    if (bad >= 0) {
        set_error("IMU velocity tap lane %d: the 15x15 covariance has no Cholesky factor (no information matrix)", bad);
        return VSLAM_ERR_INVALID;
    }
    return VSLAM_OK;
}

// The host side of vslam_relocalize (one lane, no lane named) and vslam_relocalize_batch: the lanes on the first matcher's own blocks and
// stream, the maps copied into the pinned block, the one driver, the pairs copied out.  The entries have checked the pointers.
static vslam_status reloc_run_matchers(vslam_matcher* const* matchers, int B, const double* const* xyz, const uint8_t* const* desc, const int32_t* n,
                                       const vslam_reloc_params& P, double* T_cw_out, int32_t* const* pairsOut, vslam_reloc_report* reps, bool nameLanes) {
    std::vector<RelocBatchLane> q((size_t)B);
    vslam_matcher* first = nullptr;
    for (int b = 0; b < B; b++) {
        if (!matchers[b]) continue;
        q[b].m = matchers[b]; q[b].n = n[b];
        if (!first) first = matchers[b];
    }
    if (!first) return VSLAM_OK;
    VS_CHECK(reloc_batch_check(q.data(), B, first->device, nameLanes));
    VS_HIP(hipSetDevice(first->device));
    for (int b = 0; b < B; b++)                             // work of the other matchers' own streams (key uploads, stereo) ends first
        if (q[b].m && q[b].m->stream != first->stream) VS_HIP(hipStreamSynchronize(q[b].m->stream));
    RelocBatchPlan plan;
    reloc_batch_plan(q.data(), B, plan);
    VS_CHECK(reloc_own_blocks(first, plan.upBytes, plan.dnBytes));
    const RelocBlocks blk{first->rlBlk[0], first->rlBlk[1], first->rlBlk[2], first->rlBlk[3]};
    for (int b = 0; b < B; b++) {
        if (!q[b].m || q[b].n <= 0) continue;
        memcpy(blk.h_up + q[b].oXyz, xyz[b], (size_t)q[b].n * 24);
        memcpy(blk.h_up + q[b].oDesc, desc[b], (size_t)q[b].n * 32);
    }
    VS_CHECK(reloc_batch_run(q.data(), B, plan, blk, first->stream, P, 1.0, &first->timer, T_cw_out, reps, nullptr, nameLanes));
    for (int b = 0; b < B; b++)
        if (q[b].m && q[b].n > 0 && pairsOut && pairsOut[b]) memcpy(pairsOut[b], blk.h_dn + q[b].oPairs, (size_t)q[b].n * sizeof(int));
    return VSLAM_OK;
}

vslam_status vslam_matcher::relocalize(const double* xyz, const uint8_t* desc, int n, const vslam_reloc_params* prm, double* T_cw_out,
                                       int32_t* pairsOut, vslam_reloc_report* rep) {
    if (n < 0 || (n > 0 && (!xyz || !desc)) || !T_cw_out || !rep) { set_error("relocalize: invalid arguments"); return VSLAM_ERR_INVALID; }
    if (mono) { set_error("relocalize on a mono matcher"); return VSLAM_ERR_INVALID; }
    vslam_reloc_params P;
    VS_CHECK(reloc_resolve_params(prm, P));
    VS_HIP(hipSetDevice(device));
    UseMark mark{this};
    vslam_matcher* self = this;
    return reloc_run_matchers(&self, 1, &xyz, &desc, &n, P, T_cw_out, &pairsOut, rep, false);
}

extern "C" {

vslam_status vslam_imu_reinit_velocity(vslam_matcher* m, const vslam_imu_input* imu, const double* T_cw_new, double* out) {
    if (m && imu && T_cw_new && out && imu->n_samples == 0) { set_error("IMU velocity tap: bucket length 0"); return VSLAM_ERR_INVALID; }
    return reinit_velocity_tap(m, 1, imu, T_cw_new, out);
}

vslam_status vslam_imu_reinit_velocity_batch(vslam_matcher* m, int32_t n_lanes, const vslam_imu_input* imus, const double* T_cw_new, double* out) {
    return reinit_velocity_tap(m, n_lanes, imus, T_cw_new, out);
}

vslam_status vslam_relocalize_batch(vslam_matcher* const* matchers, int32_t lanes, const double* const* points_xyz, const uint8_t* const* desc,
                                    const int32_t* n_points, const vslam_reloc_params* params, double* T_cw_out, int32_t* const* pairs_out,
                                    vslam_reloc_report* reports) {
    if (!matchers || lanes <= 0 || !n_points || !T_cw_out || !reports) { set_error("relocalize_batch: invalid arguments"); return VSLAM_ERR_INVALID; }
    vslam_reloc_params P;
    VS_CHECK(reloc_resolve_params(params, P));
    for (int b = 0; b < lanes; b++)
        if (matchers[b] && n_points[b] > 0 && (!points_xyz || !desc || !points_xyz[b] || !desc[b])) {
            set_error("relocalize_batch: lane %d: invalid arguments", b);
            return VSLAM_ERR_INVALID;
        }
    return reloc_run_matchers(matchers, lanes, points_xyz, desc, n_points, P, T_cw_out, pairs_out, reports, true);
}

vslam_status vslam_relocalize(vslam_matcher* m, const double* points_xyz, const uint8_t* desc, int32_t n_points,
                              const vslam_reloc_params* params, double* T_cw_out, int32_t* pairs_out, vslam_reloc_report* report) {
    if (!m) return VSLAM_ERR_INVALID;
    return m->relocalize(points_xyz, desc, n_points, params, T_cw_out, pairs_out, report);
}

vslam_status vslam_relocalize_debug(vslam_matcher* m, int32_t* d1_i1_d2, int32_t cap_points, int32_t* key_winner, int32_t cap_keys,
                                    int32_t* hyp_counts, int32_t cap_hypotheses, uint8_t* inlier_flags, int32_t cap_pairs, int32_t* sizes4) {
    if (!m) return VSLAM_ERR_INVALID;
    return m->relocalize_debug(d1_i1_d2, cap_points, key_winner, cap_keys, hyp_counts, cap_hypotheses, inlier_flags, cap_pairs, sizes4);
}

}  // extern "C"
