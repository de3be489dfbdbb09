// Device bodies of the yaw-only (4-DoF) pose-graph solve (pgo_yaw.hip; DESIGN.md section 6 item 29, restated by
// tests/pgo_yaw_ref.py).  A free pose has the parameters (theta, delta): T_k <- [Exp(theta g) R_k, t_k + delta] with the unit
// axis g of the call, so roll and pitch about g never change.  The residual, its 6-DoF Jacobians, the cost, the fixed-order sum
// and the accept / reject rule are those of pgo_dev.hpp, used as they are; what is written here is the 6x4 chain factor, the
// gather into 4x4 blocks (three block columns per wave), the block-banded Cholesky walk with 4x4 blocks and the retraction.
#pragma once
#include "pgo_dev.hpp"

namespace {

constexpr int PGOY_D = 4, PGOY_BLK = 16, PGOY_JAC = 24;      // parameters per pose, doubles per band block / per 6x4 Jacobian
constexpr int PGOY_COLS_PER_WAVE = 3, PGOY_COL_LANES = 20;   // 16 block elements + 4 gradient components per column

// J4 = J6 * M_k, M_k = [[R_k^T g, 0], [0, R_k^T]] (6x4): column 0 is the yaw about g seen from the pose's own frame, columns
// 1 .. 3 the world translation.  J6 [36] row-major as pgo_linearize_edge writes it, R the pose's rotation, out [24] row-major.
__device__ __forceinline__ void pgoy_chain(const double* J6, const double* R, const double* g, double* out) {
    const double a[3] = {R[0] * g[0] + R[3] * g[1] + R[6] * g[2], R[1] * g[0] + R[4] * g[1] + R[7] * g[2],
                         R[2] * g[0] + R[5] * g[1] + R[8] * g[2]};
#pragma unroll
    for (int q = 0; q < 6; q++) {
        out[4 * q] = J6[6 * q] * a[0] + J6[6 * q + 1] * a[1] + J6[6 * q + 2] * a[2];
#pragma unroll
        for (int p = 0; p < 3; p++)       // (J6[:, 3:6] R^T)[q][p] = sum_k J6[q][3 + k] R[p][k]
            out[4 * q + 1 + p] = J6[6 * q + 3] * R[3 * p] + J6[6 * q + 4] * R[3 * p + 1] + J6[6 * q + 5] * R[3 * p + 2];
    }
}

// per edge: r [6], Ji [24], Jj [24] (row = residual component, column = (theta, delta) of the pose), cost term.  The 6x6
// Jacobians are pgo_linearize_edge's, computed into registers and multiplied by M_i and M_j there.
__device__ __forceinline__ void pgoy_linearize_edge(int e, const PgoEdge* __restrict__ edges, const double* __restrict__ poses,
                                                    const double* g, double* __restrict__ res, double* __restrict__ Ji,
                                                    double* __restrict__ Jj, double* __restrict__ cost) {
    double r6[6], ji6[36], jj6[36], c1;
    pgo_linearize_edge(0, edges + e, poses, r6, ji6, jj6, &c1);
    const int i = edges[e].i, j = edges[e].j;
    double Ri[9], Rj[9];
#pragma unroll
    for (int k = 0; k < 9; k++) { Ri[k] = poses[(size_t)i * 12 + k]; Rj[k] = poses[(size_t)j * 12 + k]; }
    double oi[24], oj[24];
    pgoy_chain(ji6, Ri, g, oi);
    pgoy_chain(jj6, Rj, g, oj);
#pragma unroll
    for (int k = 0; k < 24; k++) { Ji[(size_t)e * 24 + k] = oi[k]; Jj[(size_t)e * 24 + k] = oj[k]; }
#pragma unroll
    for (int k = 0; k < 6; k++) res[(size_t)e * 6 + k] = r6[k];
    cost[e] = c1;
}

// Band storage: block (c, d), d = 0 .. b, is H[c + d][c] (lower), 16 doubles row-major, at ((c * (b + 1)) + d) * 16.
// A column takes 20 lanes: sub < 16 owns element sub = 4 r + s of every block of column c, sub 16 .. 19 own the gradient's
// components.  The caller puts three columns into a wave (lanes 0-19, 20-39, 40-59); each column walks its own incidence list in
// ascending order, so an element's sum has the order of a wave that carried this column alone, and the wave runs as long as its
// longest list.  inc[], pos[] as in pgo_assemble_column.
__device__ __forceinline__ void pgoy_assemble_column(int c, int sub, int nf, int b, const int* __restrict__ pos,
                                                     const int* __restrict__ rowStart, const int* __restrict__ inc,
                                                     const PgoEdge* __restrict__ edges, const double* __restrict__ res,
                                                     const double* __restrict__ Ji, const double* __restrict__ Jj,
                                                     double* __restrict__ band, double* __restrict__ diagH, double* __restrict__ rhs) {
    const int bc = min(b, nf - 1 - c);
    double* col = band + (size_t)c * (b + 1) * 16;
    const int r = (sub & 15) >> 2, s = sub & 3;
    if (sub < 16) for (int d = 1; d <= bc; d++) col[(size_t)d * 16 + sub] = 0.0;
    double acc = 0.0;
    for (int k = rowStart[c]; k < rowStart[c + 1]; k++) {
        const int e = inc[k] >> 1, side = inc[k] & 1;
        const double* Jc = (side ? Jj : Ji) + (size_t)e * 24;
        const double wr = edges[e].wr, wt = edges[e].wt;
        if (sub < 16) {
            double v = 0.0;
#pragma unroll
            for (int q = 0; q < 6; q++) v += Jc[4 * q + r] * (q < 3 ? wr : wt) * Jc[4 * q + s];
            acc += v;
            const int other = side ? edges[e].i : edges[e].j;
            const int o = pos[other];
            if (o > c) {                     // H[o][c] = Jo^T W Jc: the lower block of the pair, written by the lower position's lanes
                const double* Jo = (side ? Ji : Jj) + (size_t)e * 24;
                double u = 0.0;
#pragma unroll
                for (int q = 0; q < 6; q++) u += Jo[4 * q + r] * (q < 3 ? wr : wt) * Jc[4 * q + s];
                col[(size_t)(o - c) * 16 + sub] += u;
            }
        } else {
            const double* rr = res + (size_t)e * 6;
            double v = 0.0;
#pragma unroll
            for (int q = 0; q < 6; q++) v += Jc[4 * q + s] * (q < 3 ? wr : wt) * rr[q];
            acc += v;
        }
    }
    if (sub < 16) {
        col[sub] = acc;
        if (r == s) diagH[(size_t)c * 4 + r] = acc;
    } else {
        rhs[(size_t)c * 4 + s] = -acc;
    }
}

// lower-triangular 4x4 in 10 named registers, indexed by PGO_L
__device__ __forceinline__ void pgoy_chol4(double* l, int* bad) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
        double d = PGO_L(j, j);
#pragma unroll
        for (int k = 0; k < j; k++) d -= PGO_L(j, k) * PGO_L(j, k);
        if (!(d > 0.0) || !(d < 1e300)) { *bad = 1; d = 1.0; }      // the pivot rule of pgo_chol6
        const double sd = sqrt(d);
        PGO_L(j, j) = sd;
        const double inv = 1.0 / sd;
#pragma unroll
        for (int i = j + 1; i < 4; i++) {
            double v = PGO_L(i, j);
#pragma unroll
            for (int k = 0; k < j; k++) v -= PGO_L(i, k) * PGO_L(j, k);
            PGO_L(i, j) = v * inv;
        }
    }
}

// (H + lambda diag(H)) delta = rhs: the walk of pgo_band_chol_walk with 4x4 blocks.  One workgroup.  Per column c every thread
// factors the damped diagonal block and solves y_c in registers; the threads share the 4 bc block rows below it, then the
// 16 bc^2 elements of the trailing update (the upper half of the pairs skipped) and the 4 bc right-hand-side entries: the three
// barriers per column of the 6x6 walk.  Back substitution: PGO_BACK_PARTS x 4 lanes of wave 0 share a column's off-diagonal
// blocks, each part in ascending d, the parts added up in part order.
__device__ __forceinline__ void pgoy_band_chol_walk(int nf, int b, double lambda, double* __restrict__ band,
                                                    const double* __restrict__ diagH, double* __restrict__ rhs,
                                                    double* __restrict__ delta, int* __restrict__ flag) {
    __shared__ double sPart[PGO_BACK_PARTS][4];
    const int tid = threadIdx.x;
    const size_t cs = (size_t)(b + 1) * 16;      // column stride
    int bad = 0;
    for (int c = 0; c < nf; c++) {
        const int bc = min(b, nf - 1 - c);
        double* col = band + (size_t)c * cs;
        double l[10];
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j <= i; j++) PGO_L(i, j) = col[4 * i + j];
#pragma unroll
        for (int i = 0; i < 4; i++) PGO_L(i, i) += lambda * diagH[(size_t)c * 4 + i];
        pgoy_chol4(l, &bad);
        double y[4];
#pragma unroll
        for (int i = 0; i < 4; i++) y[i] = rhs[(size_t)c * 4 + i];
#pragma unroll
        for (int s = 0; s < 4; s++) {          // L y = rhs
            double v = y[s];
#pragma unroll
            for (int k = 0; k < s; k++) v -= PGO_L(s, k) * y[k];
            y[s] = v / PGO_L(s, s);
        }
        __syncthreads();                          // (every thread has read the column's diagonal block and rhs)
        for (int t = tid; t < 4 * bc; t += PGO_CHOL_NT) {
            double* row = col + (size_t)(1 + t / 4) * 16 + 4 * (t % 4);
            double x[4];
#pragma unroll
            for (int k = 0; k < 4; k++) x[k] = row[k];
#pragma unroll
            for (int s = 0; s < 4; s++) {      // x L^T = h
                double v = x[s];
#pragma unroll
                for (int k = 0; k < s; k++) v -= x[k] * PGO_L(s, k);
                x[s] = v / PGO_L(s, s);
            }
#pragma unroll
            for (int k = 0; k < 4; k++) row[k] = x[k];
        }
        if (tid == 0) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
#pragma unroll
                for (int j = 0; j < 4; j++) col[4 * i + j] = j <= i ? PGO_L(i, j) : 0.0;
                rhs[(size_t)c * 4 + i] = y[i];
            }
        }
        __syncthreads();
        // trailing update: H[c + d1][c + d2] -= L[c + d1][c] L[c + d2][c]^T for bc >= d1 >= d2 >= 1
        const int nsq = bc * bc * 16;
        for (int t = tid; t < nsq; t += PGO_CHOL_NT) {
            const int e = t % 16, pr = t / 16;
            const int d1 = 1 + pr / bc, d2 = 1 + pr % bc;
            if (d1 < d2) continue;
            const double* a = col + (size_t)d1 * 16 + 4 * (e / 4);
            const double* bb = col + (size_t)d2 * 16 + 4 * (e % 4);
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < 4; k++) v += a[k] * bb[k];
            band[(size_t)(c + d2) * cs + (size_t)(d1 - d2) * 16 + e] -= v;
        }
        for (int t = tid; t < 4 * bc; t += PGO_CHOL_NT) {
            const double* a = col + (size_t)(1 + t / 4) * 16 + 4 * (t % 4);
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < 4; k++) v += a[k] * y[k];
            rhs[(size_t)(c + 1 + t / 4) * 4 + t % 4] -= v;
        }
        __syncthreads();
    }
    for (int c = nf - 1; c >= 0; c--) {
        const int bc = min(b, nf - 1 - c);
        const double* col = band + (size_t)c * cs;
        if (tid < 4 * PGO_BACK_PARTS) {
            const int s = tid % 4, part = tid / 4;
            double acc = 0.0;
            for (int d = 1 + part; d <= bc; d += PGO_BACK_PARTS) {
                const double* blk = col + (size_t)d * 16;
                const double* dl = delta + (size_t)(c + d) * 4;
                double v = 0.0;
#pragma unroll
                for (int k = 0; k < 4; k++) v += blk[4 * k + s] * dl[k];
                acc += v;
            }
            sPart[part][s] = acc;
        }
        __syncthreads();
        if (tid == 0) {
            double l[10], x[4];
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j <= i; j++) PGO_L(i, j) = col[4 * i + j];
#pragma unroll
            for (int s = 0; s < 4; s++) {
                double v = rhs[(size_t)c * 4 + s];
#pragma unroll
                for (int q = 0; q < PGO_BACK_PARTS; q++) v -= sPart[q][s];
                x[s] = v;
            }
#pragma unroll
            for (int s = 3; s >= 0; s--) {     // L^T x = v
                double v = x[s];
#pragma unroll
                for (int k = s + 1; k < 4; k++) v -= PGO_L(k, s) * x[k];
                x[s] = v / PGO_L(s, s);
            }
#pragma unroll
            for (int s = 0; s < 4; s++) delta[(size_t)c * 4 + s] = x[s];
        }
        __syncthreads();
    }
    if (tid == 0) *flag = bad;
}

// trial poses: [Exp(theta_k g) R_k, t_k + delta_k] for a free pose, the pose itself otherwise
__device__ __forceinline__ void pgoy_retract_pose(int k, const int* __restrict__ pos, const double* __restrict__ poses,
                                                  const double* g, const double* __restrict__ delta, double* __restrict__ trial) {
    double P[12];
#pragma unroll
    for (int q = 0; q < 12; q++) P[q] = poses[(size_t)k * 12 + q];
    const int c = pos[k];
    if (c >= 0) {
        const double th = delta[(size_t)c * 4];
        const double w[3] = {th * g[0], th * g[1], th * g[2]};
        double Ex[9], R[9];
        so3_expmap(w, Ex);
        mat3_mul(Ex, P, R);
#pragma unroll
        for (int q = 0; q < 9; q++) P[q] = R[q];
#pragma unroll
        for (int q = 0; q < 3; q++) P[9 + q] += delta[(size_t)c * 4 + 1 + q];
    }
#pragma unroll
    for (int q = 0; q < 12; q++) trial[(size_t)k * 12 + q] = P[q];
}

}  // namespace
