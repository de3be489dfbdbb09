// Device bodies of the global bundle adjustment (gba.hip): what one thread (or one wave's lane) of every stage does on ONE
// problem's arrays.  The kernels of vslam_global_ba and the `_b` kernels of vslam_global_ba_batch both call them - the first with
// the call's arrays, the second with a lane's part of the concatenated ones - so a lane's arithmetic is the single call's by
// construction.  Everything here is a __device__ body, a struct or a constant; the kernels stay in gba.hip.
#pragma once
#include "common.hpp"
#include "dmath.hpp"
#include "pgo_dev.hpp"
#include "gba_pack_host.hpp"

namespace {

using namespace vslam;

struct GbaCam { double fx, fy, cx, cy, bl; };

// One projection factor: q = R^T (X - t); the right camera sees q - (bl, 0, 0).  r = (projection - measurement) * is.
// Jp [2][6]: d r / d (a, b) of the pose retraction T [Exp(a), b];  Jl [2][3]: d r / d X.  Returns z > 0.
template <bool JAC>
__device__ __forceinline__ bool gba_factor(const double* __restrict__ T, const double* __restrict__ X, const GbaCam& cam, int right,
                                           double u, double v, double is, double* r, double* Jp, double* Jl) {
    double R[9];
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = T[k];
    const double d[3] = {X[0] - T[9], X[1] - T[10], X[2] - T[11]};
    double q[3];
    mat3T_vec(R, d, q);
    const double x = q[0], y = q[1], z = q[2];
    if (!(z > 0.0)) return false;
    const double iz = 1.0 / z;
    const double xx = right ? x - cam.bl : x;
    r[0] = (cam.fx * xx * iz + cam.cx - u) * is;
    r[1] = (cam.fy * y * iz + cam.cy - v) * is;
    if (JAC) {
        const double al[2][3] = {{cam.fx * iz, 0.0, -cam.fx * xx * iz * iz}, {0.0, cam.fy * iz, -cam.fy * y * iz * iz}};
        const double S[3][3] = {{0.0, -z, y}, {z, 0.0, -x}, {-y, x, 0.0}};
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int c = 0; c < 3; c++) {
                Jp[6 * a + c] = (al[a][0] * S[0][c] + al[a][1] * S[1][c] + al[a][2] * S[2][c]) * is;
                Jp[6 * a + 3 + c] = -al[a][c] * is;
                Jl[3 * a + c] = (al[a][0] * R[3 * c] + al[a][1] * R[3 * c + 1] + al[a][2] * R[3 * c + 2]) * is;
            }
    }
    return true;
}

// one problem's arrays on the device (read-only for the kernels) and the sizes
struct GbaDev {
    int K, L, P, M, nf, b, nBlk;
    GbaCam cam;
    const PgoEdge* edges;
    const int* pos;                 // [K]
    const int* rowStart; const int* inc;
    const int* pairKf; const int* pairLm; const uint8_t* pairFlags;
    const float* pairUv;            // [P][4]
    const double* pairIs;           // [P][2]  whitening factor of the left / right factor
    const double* pairThr;          // [P][2]  chi2 threshold
    const uint8_t* kfLocal; const uint8_t* lmPresent;
    const int* lmStart; const int* lmPairs;
    const int* blkC; const int* blkD; const int* blkStart; const int* list;
};

// slot t = 2 p + side.  A slot without a factor (or on a thin landmark) holds zeros and a zero cost term.
__device__ __forceinline__ void gba_linearize_slot(int t, const GbaDev& D, const PgoCtl* __restrict__ ctl, int init, const double* __restrict__ P0,
                                                   const double* __restrict__ P1, const double* __restrict__ L0,
                                                   const double* __restrict__ L1, double* __restrict__ Jp, double* __restrict__ Jl,
                                                   double* __restrict__ res, double* __restrict__ cost) {
    if (t >= 2 * D.P) return;
    if (!init && !(ctl->active && (ctl->need_linearize & PGO_NEED_J))) return;
    const int p = t >> 1, side = t & 1, kf = D.pairKf[p], lm = D.pairLm[p];
    double r[2] = {0.0, 0.0}, jp[12], jl[6];
#pragma unroll
    for (int k = 0; k < 12; k++) jp[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 6; k++) jl[k] = 0.0;
    double c = 0.0;
    if (((D.pairFlags[p] >> side) & 1) && D.lmPresent[lm]) {
        const double* T = (ctl->cur ? P1 : P0) + (size_t)kf * 12;
        const double* X = (ctl->cur ? L1 : L0) + (size_t)lm * 3;
        const bool ok = gba_factor<true>(T, X, D.cam, side, (double)D.pairUv[4 * (size_t)p + 2 * side], (double)D.pairUv[4 * (size_t)p + 2 * side + 1],
                                         D.pairIs[t], r, jp, jl);
        c = ok ? r[0] * r[0] + r[1] * r[1] : NAN;
    }
#pragma unroll
    for (int k = 0; k < 12; k++) Jp[(size_t)t * 12 + k] = jp[k];
#pragma unroll
    for (int k = 0; k < 6; k++) Jl[(size_t)t * 6 + k] = jl[k];
    res[(size_t)t * 2] = r[0]; res[(size_t)t * 2 + 1] = r[1];
    cost[t] = c;
}

// the trial values are the buffers that are not `cur`; a factor behind its camera makes the sum NaN (a rejected trial)
__device__ __forceinline__ void gba_cost_slot(int t, const GbaDev& D, const PgoCtl* __restrict__ ctl, const double* __restrict__ P0,
                                              const double* __restrict__ P1, const double* __restrict__ L0,
                                              const double* __restrict__ L1, double* __restrict__ cost) {
    if (t >= 2 * D.P || !ctl->active) return;
    const int p = t >> 1, side = t & 1, kf = D.pairKf[p], lm = D.pairLm[p];
    if (!(((D.pairFlags[p] >> side) & 1) && D.lmPresent[lm])) return;
    const double* T = (ctl->cur ? P0 : P1) + (size_t)kf * 12;
    const double* X = (ctl->cur ? L0 : L1) + (size_t)lm * 3;
    double r[2];
    const bool ok = gba_factor<false>(T, X, D.cam, side, (double)D.pairUv[4 * (size_t)p + 2 * side], (double)D.pairUv[4 * (size_t)p + 2 * side + 1],
                                      D.pairIs[t], r, nullptr, nullptr);
    cost[t] = ok ? r[0] * r[0] + r[1] * r[1] : NAN;
}

__device__ __forceinline__ void gba_edge_linearize_one(int e, const GbaDev& D, const PgoCtl* __restrict__ ctl, int init, const double* __restrict__ P0,
                                                       const double* __restrict__ P1, double* __restrict__ res, double* __restrict__ Ji,
                                                       double* __restrict__ Jj, double* __restrict__ cost) {
    if (e >= D.M) return;
    if (!init && !(ctl->active && (ctl->need_linearize & PGO_NEED_J))) return;
    pgo_linearize_edge(e, D.edges, ctl->cur ? P1 : P0, res, Ji, Jj, cost);
}

__device__ __forceinline__ void gba_edge_cost_one(int e, const GbaDev& D, const PgoCtl* __restrict__ ctl, const double* __restrict__ P0,
                                                  const double* __restrict__ P1, double* __restrict__ cost) {
    if (e >= D.M || !ctl->active) return;
    pgo_cost_edge(e, D.edges, ctl->cur ? P0 : P1, cost);
}

// Hll = sum Jl^T Jl over the landmark's factors, damped by lambda diag(Hll); Hinv [9] by cofactors; gl = sum Jl^T r.
// A pivot of the damped block that is not positive raises *flag.
__device__ __forceinline__ void gba_landmark_one(int l, const GbaDev& D, const PgoCtl* __restrict__ ctl, const double* __restrict__ Jl,
                                                 const double* __restrict__ res, double* __restrict__ Hinv, double* __restrict__ gl,
                                                 int* __restrict__ flag) {
    if (l >= D.L || !ctl->active || !D.lmPresent[l]) return;
    double h00 = 0.0, h01 = 0.0, h02 = 0.0, h11 = 0.0, h12 = 0.0, h22 = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0;
    for (int q = D.lmStart[l]; q < D.lmStart[l + 1]; q++) {
        const size_t p = (size_t)D.lmPairs[q];
#pragma unroll
        for (int a = 0; a < 4; a++) {
            const double* j = Jl + (p * 4 + a) * 3;
            const double j0 = j[0], j1 = j[1], j2 = j[2], r = res[p * 4 + a];
            h00 += j0 * j0; h01 += j0 * j1; h02 += j0 * j2; h11 += j1 * j1; h12 += j1 * j2; h22 += j2 * j2;
            g0 += j0 * r; g1 += j1 * r; g2 += j2 * r;
        }
    }
    const double lam = ctl->lambda;
    h00 += lam * h00; h11 += lam * h11; h22 += lam * h22;
    // pivots of the LDL^T factorisation
    const double d0 = h00, l10 = h01 / d0, l20 = h02 / d0;
    const double d1 = h11 - l10 * h01, u12 = h12 - l20 * h01;
    const double d2 = h22 - l20 * h02 - (u12 / d1) * u12;
    if (!(d0 > 0.0) || !(d1 > 0.0) || !(d2 > 0.0) || !(d0 < 1e300) || !(d1 < 1e300) || !(d2 < 1e300)) atomicOr(flag, 1);
    const double A = h11 * h22 - h12 * h12, B = h02 * h12 - h01 * h22, C = h01 * h12 - h02 * h11;
    const double id = 1.0 / (h00 * A + h01 * B + h02 * C);
    double* o = Hinv + (size_t)l * 9;
    o[0] = A * id; o[1] = B * id; o[2] = C * id;
    o[3] = B * id; o[4] = (h00 * h22 - h02 * h02) * id; o[5] = (h01 * h02 - h00 * h12) * id;
    o[6] = C * id; o[7] = (h01 * h02 - h00 * h12) * id; o[8] = (h00 * h11 - h01 * h01) * id;
    gl[(size_t)l * 3] = g0; gl[(size_t)l * 3 + 1] = g1; gl[(size_t)l * 3 + 2] = g2;
}

// W [6][3] = sum Jp^T Jl over the pair's factors, Y = W Hinv
__device__ __forceinline__ void gba_wy_pair(int p, const GbaDev& D, const PgoCtl* __restrict__ ctl, const double* __restrict__ Jp,
                                            const double* __restrict__ Jl, const double* __restrict__ Hinv, double* __restrict__ W,
                                            double* __restrict__ Y) {
    if (p >= D.P || !ctl->active) return;
    const int lm = D.pairLm[p];
    if (!(D.pairFlags[p] & 3) || !D.lmPresent[lm] || D.pos[D.pairKf[p]] < 0) return;
    double w[18];
#pragma unroll
    for (int k = 0; k < 18; k++) w[k] = 0.0;
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const double* jp = Jp + ((size_t)p * 4 + a) * 6;
        const double* jl = Jl + ((size_t)p * 4 + a) * 3;
        const double l0 = jl[0], l1 = jl[1], l2 = jl[2];
#pragma unroll
        for (int i = 0; i < 6; i++) { const double v = jp[i]; w[3 * i] += v * l0; w[3 * i + 1] += v * l1; w[3 * i + 2] += v * l2; }
    }
    double hi[9];
#pragma unroll
    for (int k = 0; k < 9; k++) hi[k] = Hinv[(size_t)lm * 9 + k];
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            W[(size_t)p * 18 + 3 * i + j] = w[3 * i + j];
            Y[(size_t)p * 18 + 3 * i + j] = w[3 * i] * hi[j] + w[3 * i + 1] * hi[3 + j] + w[3 * i + 2] * hi[6 + j];
        }
}

// the edges' part of column c: every block of the column is written (zero where no edge reaches), diagH and g too
__device__ __forceinline__ void gba_edge_column(int c, int lane, const GbaDev& D, const PgoCtl* __restrict__ ctl, const double* __restrict__ res,
                                                const double* __restrict__ Ji, const double* __restrict__ Jj,
                                                double* __restrict__ band, double* __restrict__ diagH, double* __restrict__ g) {
    if (c >= D.nf || lane >= 42 || !ctl->active) return;
    pgo_assemble_column(c, lane, D.nf, D.b, D.pos, D.rowStart, D.inc, D.edges, res, Ji, Jj, band, diagH, g);
}

// Block i of the landmark lists: H[c + d][c] += sum over its entries (p1 on c + d, p2 on c) of -Y_p1 W_p2^T, and on the diagonal
// (p1 == p2) the pair's Jp^T Jp; lanes 36 .. 41 of a diagonal block: g_c -= Jp^T r - Y_p gl.  diagH gets the undamped pose
// diagonal (Jp^T Jp alone).  It runs after the edges' columns, which wrote the block.
__device__ __forceinline__ void gba_gather_block(int i, int lane, const GbaDev& D, const PgoCtl* __restrict__ ctl, const double* __restrict__ Jp,
                                                 const double* __restrict__ res, const double* __restrict__ W, const double* __restrict__ Y,
                                                 const double* __restrict__ gl, double* __restrict__ band, double* __restrict__ diagH,
                                                 double* __restrict__ g) {
    if (i >= D.nBlk || lane >= 42 || !ctl->active) return;
    const int c = D.blkC[i], d = D.blkD[i];
    if (lane >= 36 && d != 0) return;
    const int r = lane / 6, s = lane % 6;
    double acc = 0.0, accH = 0.0;
    for (int k = D.blkStart[i]; k < D.blkStart[i + 1]; k++) {
        const size_t p1 = (size_t)D.list[2 * (size_t)k], p2 = (size_t)D.list[2 * (size_t)k + 1];
        if (lane < 36) {
            const double* y = Y + p1 * 18 + 3 * r;
            const double* w = W + p2 * 18 + 3 * s;
            acc -= y[0] * w[0] + y[1] * w[1] + y[2] * w[2];
            if (d == 0 && p1 == p2) {
                const double* jp = Jp + p1 * 24;
                double v = 0.0;
#pragma unroll
                for (int a = 0; a < 4; a++) v += jp[6 * a + r] * jp[6 * a + s];
                acc += v; accH += v;
            }
        } else if (p1 == p2) {
            const double* jp = Jp + p1 * 24;
            const double* rr = res + p1 * 4;
            const double* y = Y + p1 * 18 + 3 * s;
            const double* q = gl + (size_t)D.pairLm[p1] * 3;
            double v = 0.0;
#pragma unroll
            for (int a = 0; a < 4; a++) v += jp[6 * a + s] * rr[a];
            acc += v - (y[0] * q[0] + y[1] * q[1] + y[2] * q[2]);
        }
    }
    if (lane < 36) {
        band[((size_t)c * (D.b + 1) + d) * 36 + lane] += acc;
        if (d == 0 && r == s) diagH[(size_t)c * 6 + r] += accH;
    } else {
        g[(size_t)c * 6 + s] -= acc;
    }
}

__device__ __forceinline__ void gba_band_copy_one(size_t t, const GbaDev& D, const PgoCtl* __restrict__ ctl, const double* __restrict__ bandH,
                                                  const double* __restrict__ g, double* __restrict__ bandL, double* __restrict__ rhs) {
    if (t >= (size_t)(D.b + 1) * D.nf * 36 || !ctl->active) return;
    bandL[t] = bandH[t];
    if (t < (size_t)D.nf * 6) rhs[t] = g[t];
}

// the landmark step dX = Hinv (-gl - sum W_p^T delta_kf(p)) over the landmark's pairs on free keyframes, in list order; the trial
// landmark; a thin landmark's trial value is its value.  The steps follow the poses' in `delta` (|delta|_inf covers both).
__device__ __forceinline__ void gba_back_one(int l, const GbaDev& D, const PgoCtl* __restrict__ ctl, const double* __restrict__ W,
                                             const double* __restrict__ Hinv, const double* __restrict__ gl, double* __restrict__ L0,
                                             double* __restrict__ L1, double* __restrict__ delta) {
    if (l >= D.L || !ctl->active) return;
    const double* X = (ctl->cur ? L1 : L0) + (size_t)l * 3;
    double* Xt = (ctl->cur ? L0 : L1) + (size_t)l * 3;
    double* dl = delta + (size_t)D.nf * 6 + (size_t)l * 3;
    if (!D.lmPresent[l]) { Xt[0] = X[0]; Xt[1] = X[1]; Xt[2] = X[2]; dl[0] = dl[1] = dl[2] = 0.0; return; }
    double t0 = -gl[(size_t)l * 3], t1 = -gl[(size_t)l * 3 + 1], t2 = -gl[(size_t)l * 3 + 2];
    for (int q = D.lmStart[l]; q < D.lmStart[l + 1]; q++) {
        const size_t p = (size_t)D.lmPairs[q];
        const int c = D.pos[D.pairKf[p]];
        if (c < 0) continue;
        const double* w = W + p * 18;
        const double* dp = delta + (size_t)c * 6;
#pragma unroll
        for (int i = 0; i < 6; i++) { const double v = dp[i]; t0 -= w[3 * i] * v; t1 -= w[3 * i + 1] * v; t2 -= w[3 * i + 2] * v; }
    }
    const double* hi = Hinv + (size_t)l * 9;
    const double d0 = hi[0] * t0 + hi[1] * t1 + hi[2] * t2, d1 = hi[3] * t0 + hi[4] * t1 + hi[5] * t2, d2 = hi[6] * t0 + hi[7] * t1 + hi[8] * t2;
    Xt[0] = X[0] + d0; Xt[1] = X[1] + d1; Xt[2] = X[2] + d2;
    dl[0] = d0; dl[1] = d1; dl[2] = d2;
}

__device__ __forceinline__ void gba_retract_one(int k, const GbaDev& D, const PgoCtl* __restrict__ ctl, double* __restrict__ P0, double* __restrict__ P1,
                                                const double* __restrict__ delta) {
    if (k >= D.K || !ctl->active) return;
    pgo_retract_pose(k, D.pos, ctl->cur ? P1 : P0, delta, ctl->cur ? P0 : P1);
}

// the local BA's chi2 rule at the final values: pairs of kf_local keyframes on present landmarks, left then right
__device__ __forceinline__ void gba_chi2_pair(int p, const GbaDev& D, const PgoCtl* __restrict__ ctl, const double* __restrict__ P0,
                                              const double* __restrict__ P1, const double* __restrict__ L0, const double* __restrict__ L1,
                                              uint8_t* __restrict__ wrong) {
    if (p >= D.P) return;
    const int kf = D.pairKf[p], lm = D.pairLm[p], fl = D.pairFlags[p] & 3;
    uint8_t w = 0;
    if (fl && D.kfLocal[kf] && D.lmPresent[lm]) {
        const double* T = (ctl->cur ? P1 : P0) + (size_t)kf * 12;
        const double* X = (ctl->cur ? L1 : L0) + (size_t)lm * 3;
        const double d[3] = {X[0] - T[9], X[1] - T[10], X[2] - T[11]};
        double R[9], q[3];
#pragma unroll
        for (int k = 0; k < 9; k++) R[k] = T[k];
        mat3T_vec(R, d, q);
        const double z = q[2];
        bool out[2];
#pragma unroll
        for (int side = 0; side < 2; side++) {
            const double x = side ? q[0] - D.cam.bl : q[0];
            const double px = D.cam.fx * x + D.cam.cx * z, py = D.cam.fy * q[1] + D.cam.cy * z;
            const double eu = (double)D.pairUv[4 * (size_t)p + 2 * side] - px / z, ev = (double)D.pairUv[4 * (size_t)p + 2 * side + 1] - py / z;
            out[side] = !(z > 0.0) || (eu * eu + ev * ev) > D.pairThr[2 * (size_t)p + side];
        }
        w = ((fl & 1) && out[0]) || ((fl & 2) && out[1]);
    }
    wrong[p] = w;
}

// a lane of a batched call (gba_pack_host.hpp): the lane's sizes and camera, and its part of the concatenated arrays that B points to
__device__ __forceinline__ GbaDev gba_lane_dev(const GbaLane* T, const GbaDev& B) {
    GbaDev D;
    D.K = T->K; D.L = T->L; D.P = T->P; D.M = T->M; D.nf = T->nf; D.b = T->b; D.nBlk = T->nBlk;
    D.cam = GbaCam{T->fx, T->fy, T->cx, T->cy, T->bl};
    const size_t kf0 = (size_t)T->kf0, lm0 = (size_t)T->lm0, p0 = (size_t)T->pair0, ln = (size_t)T->lane;
    D.edges = B.edges + (size_t)T->edge0;
    D.pos = B.pos + kf0;
    D.rowStart = B.rowStart + (size_t)T->free0 + ln; D.inc = B.inc + (size_t)T->inc0;
    D.pairKf = B.pairKf + p0; D.pairLm = B.pairLm + p0; D.pairFlags = B.pairFlags + p0;
    D.pairUv = B.pairUv + p0 * 4; D.pairIs = B.pairIs + p0 * 2; D.pairThr = B.pairThr + p0 * 2;
    D.kfLocal = B.kfLocal + kf0; D.lmPresent = B.lmPresent + lm0;
    D.lmStart = B.lmStart + lm0 + ln; D.lmPairs = B.lmPairs + (size_t)T->lp0;
    D.blkC = B.blkC + (size_t)T->blk0; D.blkD = B.blkD + (size_t)T->blk0; D.blkStart = B.blkStart + (size_t)T->blk0 + ln;
    D.list = B.list + (size_t)T->list0 * 2;
    return D;
}

}  // namespace
