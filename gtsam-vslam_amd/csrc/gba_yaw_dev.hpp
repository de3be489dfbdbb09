// Device bodies of the yaw-only (4-DoF keyframe) global bundle adjustment (gba_yaw.hip; DESIGN.md section 6 item 30, restated by
// tests/gba_yaw_ref.py).  A free keyframe has the parameters (theta, delta): T_k <- [Exp(theta g) R_k, t_k + delta] with the unit
// axis g of the lane, so roll and pitch about g never change.  The projection factor (gba_factor), the landmark blocks, the cost,
// the chi2 rule, the fixed-order sum and the accept / reject rule are those of gba_dev.hpp and pgo_dev.hpp, used as they are;
// the edges' linearisation and columns, the 4x4 band walk and the retraction are those of pgo_yaw_dev.hpp.  What is written here
// is every body of gba_dev.hpp that counts a keyframe's parameters, with the 6 replaced by 4: the chain factor on the
// projection Jacobian, W / Y [4][3], the gather into 4x4 band blocks (three blocks per wave), the band copy and the landmark
// back-substitution.
#pragma once
#include "gba_dev.hpp"
#include "pgo_yaw_dev.hpp"

namespace {

constexpr int GBAY_JP = 8, GBAY_WY = 12;                      // doubles of a slot's [2][4] pose Jacobian, of a pair's W or Y [4][3]
constexpr int GBAY_BLKS_PER_WAVE = 3, GBAY_BLK_LANES = 20;    // 16 block elements + 4 gradient components per listed block

// Jp4 [2][4] = Jp6 [2][6] * M_k, M_k = [[R_k^T g, 0], [0, R_k^T]]: pgoy_chain on the two rows of a projection factor
__device__ __forceinline__ void gbay_chain2(const double* J6, const double* R, const double* g, double* out) {
    const double a[3] = {R[0] * g[0] + R[3] * g[1] + R[6] * g[2], R[1] * g[0] + R[4] * g[1] + R[7] * g[2],
                         R[2] * g[0] + R[5] * g[1] + R[8] * g[2]};
#pragma unroll
    for (int q = 0; q < 2; q++) {
        out[4 * q] = J6[6 * q] * a[0] + J6[6 * q + 1] * a[1] + J6[6 * q + 2] * a[2];
#pragma unroll
        for (int p = 0; p < 3; p++)
            out[4 * q + 1 + p] = J6[6 * q + 3] * R[3 * p] + J6[6 * q + 4] * R[3 * p + 1] + J6[6 * q + 5] * R[3 * p + 2];
    }
}

// slot t = 2 p + side: gba_linearize_slot with the pose Jacobian multiplied by M_k in registers (8 doubles a slot); Jl, the
// residual and the cost term are gba_factor's
__device__ __forceinline__ void gbay_linearize_slot(int t, const GbaDev& D, const PgoCtl* __restrict__ ctl, int init, const double* g,
                                                    const double* __restrict__ P0, const double* __restrict__ P1, const double* __restrict__ L0,
                                                    const double* __restrict__ L1, double* __restrict__ Jp, double* __restrict__ Jl,
                                                    double* __restrict__ res, double* __restrict__ cost) {
    if (t >= 2 * D.P) return;
    if (!init && !(ctl->active && (ctl->need_linearize & PGO_NEED_J))) return;
    const int p = t >> 1, side = t & 1, kf = D.pairKf[p], lm = D.pairLm[p];
    double r[2] = {0.0, 0.0}, jp[GBAY_JP], jl[6];
#pragma unroll
    for (int k = 0; k < GBAY_JP; k++) jp[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 6; k++) jl[k] = 0.0;
    double c = 0.0;
    if (((D.pairFlags[p] >> side) & 1) && D.lmPresent[lm]) {
        const double* T = (ctl->cur ? P1 : P0) + (size_t)kf * 12;
        const double* X = (ctl->cur ? L1 : L0) + (size_t)lm * 3;
        double jp6[12], R[9];
#pragma unroll
        for (int k = 0; k < 12; k++) jp6[k] = 0.0;
        const bool ok = gba_factor<true>(T, X, D.cam, side, (double)D.pairUv[4 * (size_t)p + 2 * side], (double)D.pairUv[4 * (size_t)p + 2 * side + 1],
                                         D.pairIs[t], r, jp6, jl);
#pragma unroll
        for (int k = 0; k < 9; k++) R[k] = T[k];
        gbay_chain2(jp6, R, g, jp);
        c = ok ? r[0] * r[0] + r[1] * r[1] : NAN;
    }
#pragma unroll
    for (int k = 0; k < GBAY_JP; k++) Jp[(size_t)t * GBAY_JP + k] = jp[k];
#pragma unroll
    for (int k = 0; k < 6; k++) Jl[(size_t)t * 6 + k] = jl[k];
    res[(size_t)t * 2] = r[0]; res[(size_t)t * 2 + 1] = r[1];
    cost[t] = c;
}

__device__ __forceinline__ void gbay_edge_linearize_one(int e, const GbaDev& D, const PgoCtl* __restrict__ ctl, int init, const double* g,
                                                        const double* __restrict__ P0, const double* __restrict__ P1, double* __restrict__ res,
                                                        double* __restrict__ Ji, double* __restrict__ Jj, double* __restrict__ cost) {
    if (e >= D.M) return;
    if (!init && !(ctl->active && (ctl->need_linearize & PGO_NEED_J))) return;
    pgoy_linearize_edge(e, D.edges, ctl->cur ? P1 : P0, g, res, Ji, Jj, cost);
}

// W [4][3] = sum Jp4^T Jl over the pair's factors, Y = W Hinv
__device__ __forceinline__ void gbay_wy_pair(int p, const GbaDev& D, const PgoCtl* __restrict__ ctl, const double* __restrict__ Jp,
                                             const double* __restrict__ Jl, const double* __restrict__ Hinv, double* __restrict__ W,
                                             double* __restrict__ Y) {
    if (p >= D.P || !ctl->active) return;
    const int lm = D.pairLm[p];
    if (!(D.pairFlags[p] & 3) || !D.lmPresent[lm] || D.pos[D.pairKf[p]] < 0) return;
    double w[GBAY_WY];
#pragma unroll
    for (int k = 0; k < GBAY_WY; k++) w[k] = 0.0;
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const double* jp = Jp + ((size_t)p * 4 + a) * 4;
        const double* jl = Jl + ((size_t)p * 4 + a) * 3;
        const double l0 = jl[0], l1 = jl[1], l2 = jl[2];
#pragma unroll
        for (int i = 0; i < 4; i++) { const double v = jp[i]; w[3 * i] += v * l0; w[3 * i + 1] += v * l1; w[3 * i + 2] += v * l2; }
    }
    double hi[9];
#pragma unroll
    for (int k = 0; k < 9; k++) hi[k] = Hinv[(size_t)lm * 9 + k];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            W[(size_t)p * GBAY_WY + 3 * i + j] = w[3 * i + j];
            Y[(size_t)p * GBAY_WY + 3 * i + j] = w[3 * i] * hi[j] + w[3 * i + 1] * hi[3 + j] + w[3 * i + 2] * hi[6 + j];
        }
}

// the edges' part of column c (sub < 20 of the column's lanes): every block of the column is written (zero where no edge
// reaches), diagH and g too
__device__ __forceinline__ void gbay_edge_column(int c, int sub, const GbaDev& D, const PgoCtl* __restrict__ ctl, const double* __restrict__ res,
                                                 const double* __restrict__ Ji, const double* __restrict__ Jj,
                                                 double* __restrict__ band, double* __restrict__ diagH, double* __restrict__ g) {
    if (c >= D.nf || sub >= PGOY_COL_LANES || !ctl->active) return;
    pgoy_assemble_column(c, sub, D.nf, D.b, D.pos, D.rowStart, D.inc, D.edges, res, Ji, Jj, band, diagH, g);
}

// Block i of the landmark lists, 20 lanes: sub < 16 owns element sub = 4 r + s of H[c + d][c] and adds, over the block's entries
// (p1 on c + d, p2 on c) in list order, -Y_p1 W_p2^T and on the diagonal (p1 == p2) the pair's Jp4^T Jp4; sub 16 .. 19 of a
// diagonal block: g_c -= Jp4^T r - Y_p gl.  diagH gets the undamped pose diagonal.  The caller puts three blocks of the list into
// a wave; each walks its own list, so an element's sum does not depend on the block's company.  It runs after the edges' columns.
__device__ __forceinline__ void gbay_gather_block(int i, int sub, const GbaDev& D, const PgoCtl* __restrict__ ctl, const double* __restrict__ Jp,
                                                  const double* __restrict__ res, const double* __restrict__ W, const double* __restrict__ Y,
                                                  const double* __restrict__ gl, double* __restrict__ band, double* __restrict__ diagH,
                                                  double* __restrict__ g) {
    if (i >= D.nBlk || sub >= GBAY_BLK_LANES || !ctl->active) return;
    const int c = D.blkC[i], d = D.blkD[i];
    if (sub >= 16 && d != 0) return;
    const int r = (sub & 15) >> 2, s = sub & 3;
    double acc = 0.0, accH = 0.0;
    for (int k = D.blkStart[i]; k < D.blkStart[i + 1]; k++) {
        const size_t p1 = (size_t)D.list[2 * (size_t)k], p2 = (size_t)D.list[2 * (size_t)k + 1];
        if (sub < 16) {
            const double* y = Y + p1 * GBAY_WY + 3 * r;
            const double* w = W + p2 * GBAY_WY + 3 * s;
            acc -= y[0] * w[0] + y[1] * w[1] + y[2] * w[2];
            if (d == 0 && p1 == p2) {
                const double* jp = Jp + p1 * 16;
                double v = 0.0;
#pragma unroll
                for (int a = 0; a < 4; a++) v += jp[4 * a + r] * jp[4 * a + s];
                acc += v; accH += v;
            }
        } else if (p1 == p2) {
            const double* jp = Jp + p1 * 16;
            const double* rr = res + p1 * 4;
            const double* y = Y + p1 * GBAY_WY + 3 * s;
            const double* q = gl + (size_t)D.pairLm[p1] * 3;
            double v = 0.0;
#pragma unroll
            for (int a = 0; a < 4; a++) v += jp[4 * a + s] * rr[a];
            acc += v - (y[0] * q[0] + y[1] * q[1] + y[2] * q[2]);
        }
    }
    if (sub < 16) {
        band[((size_t)c * (D.b + 1) + d) * PGOY_BLK + sub] += acc;
        if (d == 0 && r == s) diagH[(size_t)c * PGOY_D + r] += accH;
    } else {
        g[(size_t)c * PGOY_D + s] -= acc;
    }
}

__device__ __forceinline__ void gbay_band_copy_one(size_t t, const GbaDev& D, const PgoCtl* __restrict__ ctl, const double* __restrict__ bandH,
                                                   const double* __restrict__ g, double* __restrict__ bandL, double* __restrict__ rhs) {
    if (t >= (size_t)(D.b + 1) * D.nf * PGOY_BLK || !ctl->active) return;
    bandL[t] = bandH[t];
    if (t < (size_t)D.nf * PGOY_D) rhs[t] = g[t];
}

// gba_back_one with four pose steps per keyframe: `delta` holds nf * 4 pose entries, then L * 3 landmark steps
__device__ __forceinline__ void gbay_back_one(int l, const GbaDev& D, const PgoCtl* __restrict__ ctl, const double* __restrict__ W,
                                              const double* __restrict__ Hinv, const double* __restrict__ gl, double* __restrict__ L0,
                                              double* __restrict__ L1, double* __restrict__ delta) {
    if (l >= D.L || !ctl->active) return;
    const double* X = (ctl->cur ? L1 : L0) + (size_t)l * 3;
    double* Xt = (ctl->cur ? L0 : L1) + (size_t)l * 3;
    double* dl = delta + (size_t)D.nf * PGOY_D + (size_t)l * 3;
    if (!D.lmPresent[l]) { Xt[0] = X[0]; Xt[1] = X[1]; Xt[2] = X[2]; dl[0] = dl[1] = dl[2] = 0.0; return; }
    double t0 = -gl[(size_t)l * 3], t1 = -gl[(size_t)l * 3 + 1], t2 = -gl[(size_t)l * 3 + 2];
    for (int q = D.lmStart[l]; q < D.lmStart[l + 1]; q++) {
        const size_t p = (size_t)D.lmPairs[q];
        const int c = D.pos[D.pairKf[p]];
        if (c < 0) continue;
        const double* w = W + p * GBAY_WY;
        const double* dp = delta + (size_t)c * PGOY_D;
#pragma unroll
        for (int i = 0; i < 4; i++) { const double v = dp[i]; t0 -= w[3 * i] * v; t1 -= w[3 * i + 1] * v; t2 -= w[3 * i + 2] * v; }
    }
    const double* hi = Hinv + (size_t)l * 9;
    const double d0 = hi[0] * t0 + hi[1] * t1 + hi[2] * t2, d1 = hi[3] * t0 + hi[4] * t1 + hi[5] * t2, d2 = hi[6] * t0 + hi[7] * t1 + hi[8] * t2;
    Xt[0] = X[0] + d0; Xt[1] = X[1] + d1; Xt[2] = X[2] + d2;
    dl[0] = d0; dl[1] = d1; dl[2] = d2;
}

__device__ __forceinline__ void gbay_retract_one(int k, const GbaDev& D, const PgoCtl* __restrict__ ctl, const double* g, double* __restrict__ P0,
                                                 double* __restrict__ P1, const double* __restrict__ delta) {
    if (k >= D.K || !ctl->active) return;
    pgoy_retract_pose(k, D.pos, ctl->cur ? P1 : P0, g, delta, ctl->cur ? P0 : P1);
}

}  // namespace
