// Device bodies of the pose-graph solve that the global bundle adjustment (gba.hip) shares with pgo.hip: the edge residual and
// its Jacobians, the gather of a block column over an incidence list, the block-banded fp64 Cholesky walk (factor, forward and
// back substitution by one workgroup), the pose retraction, the fixed-order sum and THE accept / reject rule of the
// Levenberg-Marquardt loop.  Everything here is a __device__ body or a constant; the kernels stay with their callers.
#pragma once
#include "common.hpp"
#include "dmath.hpp"

namespace {

using namespace vslam;

constexpr int PGO_MAX_POSES = 16384, PGO_MAX_EDGES = 262144, PGO_MAX_BLOCKS = 262144;
constexpr int PGO_CHOL_NT = 256;       // threads of the factorisation's workgroup
constexpr int PGO_RED_NT = 256;
constexpr int PGO_BACK_PARTS = 10;     // back substitution: 10 x 6 lanes of wave 0 share a column's off-diagonal blocks

// a pose on the device: R row-major [9], t [3]
struct PgoEdge { int i, j; double Rz[9], tz[3], wr, wt; };

// SO(3) logarithm: the rule of dmath.hpp's so3_logmap, written out so that the restatement can follow it line by line
__device__ __forceinline__ void pgo_log(const double* R, double* w) {
    const double tr = R[0] + R[4] + R[8];
    const double tr_3 = tr - 3.0;
    double mag;
    if (tr_3 < -1e-6) {
        double c = (tr - 1.0) / 2.0;
        c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
        const double theta = acos(c);
        mag = theta / (2.0 * sin(theta));
    } else {
        mag = 0.5 - tr_3 / 12.0 + tr_3 * tr_3 / 60.0;
    }
    w[0] = mag * (R[7] - R[5]);
    w[1] = mag * (R[2] - R[6]);
    w[2] = mag * (R[3] - R[1]);
}

// E = Z^-1 * T_i^-1 * T_j with rigid inverses; RD / tD = T_i^-1 * T_j
__device__ __forceinline__ void pgo_error(const double* Pi, const double* Pj, const PgoEdge& e, double* RD, double* tD, double* RE, double* tE) {
    double RiT[9], RzT[9];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) { RiT[3 * a + b] = Pi[3 * b + a]; RzT[3 * a + b] = e.Rz[3 * b + a]; }
    mat3_mul(RiT, Pj, RD);
    const double dt[3] = {Pj[9] - Pi[9], Pj[10] - Pi[10], Pj[11] - Pi[11]};
    mat3_vec(RiT, dt, tD);
    mat3_mul(RzT, RD, RE);
    const double dz[3] = {tD[0] - e.tz[0], tD[1] - e.tz[1], tD[2] - e.tz[2]};
    mat3_vec(RzT, dz, tE);
}

// per edge: r [6], Ji [36], Jj [36] (row = residual component, column = parameter (a, b) of the pose), cost term
// (the bodies below take one graph's arrays: the kernels pass a lane's part of the pooled ones)
__device__ __forceinline__ void pgo_linearize_edge(int e, const PgoEdge* __restrict__ edges, const double* __restrict__ poses,
                                                   double* __restrict__ res, double* __restrict__ Ji, double* __restrict__ Jj,
                                                   double* __restrict__ cost) {
    const PgoEdge E = edges[e];
    double Pi[12], Pj[12];
#pragma unroll
    for (int k = 0; k < 12; k++) { Pi[k] = poses[(size_t)E.i * 12 + k]; Pj[k] = poses[(size_t)E.j * 12 + k]; }
    double RD[9], tD[3], RE[9], tE[3], w[3];
    pgo_error(Pi, Pj, E, RD, tD, RE, tE);
    pgo_log(RE, w);
    // inverse right Jacobian of SO(3): I + W / 2 + c W^2
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    double c;
    if (th2 < 1e-10) c = 1.0 / 12.0;
    else { const double th = sqrt(th2); c = 1.0 / th2 - (1.0 + cos(th)) / (2.0 * th * sin(th)); }
    double W[9], WW[9], Jri[9];
    skew3(w, W);
    mat3_mul(W, W, WW);
#pragma unroll
    for (int k = 0; k < 9; k++) Jri[k] = ((k % 4 == 0) ? 1.0 : 0.0) + 0.5 * W[k] + c * WW[k];
    double RDT[9], RzT[9], A[9], S[9], B[9];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) { RDT[3 * a + b] = RD[3 * b + a]; RzT[3 * a + b] = E.Rz[3 * b + a]; }
    mat3_mul(Jri, RDT, A);          // d r_w / d a_i = -A
    skew3(tD, S);
    mat3_mul(RzT, S, B);            // d r_t / d a_i = B;  d r_t / d b_i = -RzT
    double* ji = Ji + (size_t)e * 36;
    double* jj = Jj + (size_t)e * 36;
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) {
            ji[6 * a + b] = -A[3 * a + b];        ji[6 * a + 3 + b] = 0.0;
            ji[6 * (a + 3) + b] = B[3 * a + b];   ji[6 * (a + 3) + 3 + b] = -RzT[3 * a + b];
            jj[6 * a + b] = Jri[3 * a + b];       jj[6 * a + 3 + b] = 0.0;
            jj[6 * (a + 3) + b] = 0.0;            jj[6 * (a + 3) + 3 + b] = RE[3 * a + b];
        }
    double* r = res + (size_t)e * 6;
    r[0] = w[0]; r[1] = w[1]; r[2] = w[2]; r[3] = tE[0]; r[4] = tE[1]; r[5] = tE[2];
    cost[e] = E.wr * th2 + E.wt * (tE[0] * tE[0] + tE[1] * tE[1] + tE[2] * tE[2]);
}

// the cost term alone, for trial poses
__device__ __forceinline__ void pgo_cost_edge(int e, const PgoEdge* __restrict__ edges, const double* __restrict__ poses,
                                              double* __restrict__ cost) {
    const PgoEdge E = edges[e];
    double Pi[12], Pj[12];
#pragma unroll
    for (int k = 0; k < 12; k++) { Pi[k] = poses[(size_t)E.i * 12 + k]; Pj[k] = poses[(size_t)E.j * 12 + k]; }
    double RD[9], tD[3], RE[9], tE[3], w[3];
    pgo_error(Pi, Pj, E, RD, tD, RE, tE);
    pgo_log(RE, w);
    cost[e] = E.wr * (w[0] * w[0] + w[1] * w[1] + w[2] * w[2]) + E.wt * (tE[0] * tE[0] + tE[1] * tE[1] + tE[2] * tE[2]);
}

// Band storage: block (c, d), d = 0 .. b, is H[c + d][c] (lower), 36 doubles row-major, at ((c * (b + 1)) + d) * 36.
// One wave per free pose (band position c).  Lane e < 36 owns element e = 6 r + s of every block of column c; lanes 36 .. 41 own
// the gradient's components.  inc[k] = edge << 1 | side (1: the pose is the edge's j), ascending; pos[] = band position or -1.
__device__ __forceinline__ void pgo_assemble_column(int c, int lane, int nf, int b, const int* __restrict__ pos,
                                                    const int* __restrict__ rowStart, const int* __restrict__ inc,
                                                    const PgoEdge* __restrict__ edges, const double* __restrict__ res,
                                                    const double* __restrict__ Ji, const double* __restrict__ Jj,
                                                    double* __restrict__ band, double* __restrict__ diagH, double* __restrict__ rhs) {
    const int bc = min(b, nf - 1 - c);
    double* col = band + (size_t)c * (b + 1) * 36;
    const int r = lane / 6, s = lane % 6;
    if (lane < 36) for (int d = 1; d <= bc; d++) col[(size_t)d * 36 + lane] = 0.0;
    double acc = 0.0;
    for (int k = rowStart[c]; k < rowStart[c + 1]; k++) {
        const int e = inc[k] >> 1, side = inc[k] & 1;
        const double* Jc = (side ? Jj : Ji) + (size_t)e * 36;
        const double wr = edges[e].wr, wt = edges[e].wt;
        if (lane < 36) {
            double v = 0.0;
#pragma unroll
            for (int q = 0; q < 6; q++) v += Jc[6 * q + r] * (q < 3 ? wr : wt) * Jc[6 * q + s];
            acc += v;
            const int other = side ? edges[e].i : edges[e].j;
            const int o = pos[other];
            if (o > c) {                     // H[o][c] = Jo^T W Jc: the lower block of the pair, written by the lower position's wave
                const double* Jo = (side ? Ji : Jj) + (size_t)e * 36;
                double u = 0.0;
#pragma unroll
                for (int q = 0; q < 6; q++) u += Jo[6 * q + r] * (q < 3 ? wr : wt) * Jc[6 * q + s];
                col[(size_t)(o - c) * 36 + lane] += u;
            }
        } else {
            const double* rr = res + (size_t)e * 6;
            double v = 0.0;
#pragma unroll
            for (int q = 0; q < 6; q++) v += Jc[6 * q + s] * (q < 3 ? wr : wt) * rr[q];
            acc += v;
        }
    }
    if (lane < 36) {
        col[lane] = acc;
        if (r == s) diagH[(size_t)c * 6 + r] = acc;
    } else {
        rhs[(size_t)c * 6 + s] = -acc;
    }
}

// lower-triangular 6x6 in 21 named registers: L(i, j) = l[i (i + 1) / 2 + j]
#define PGO_L(i, j) l[(i) * ((i) + 1) / 2 + (j)]

// in-place Cholesky of the lower triangle; a pivot that is not positive raises *bad and is replaced by 1
__device__ __forceinline__ void pgo_chol6(double* l, int* bad) {
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double d = PGO_L(j, j);
#pragma unroll
        for (int k = 0; k < j; k++) d -= PGO_L(j, k) * PGO_L(j, k);
        if (!(d > 0.0) || !(d < 1e300)) { *bad = 1; d = 1.0; }
        const double sd = sqrt(d);
        PGO_L(j, j) = sd;
        const double inv = 1.0 / sd;
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            double v = PGO_L(i, j);
#pragma unroll
            for (int k = 0; k < j; k++) v -= PGO_L(i, k) * PGO_L(j, k);
            PGO_L(i, j) = v * inv;
        }
    }
}
// x L^T = h  (one block row against the column's diagonal factor): x[s] = (h[s] - sum_{k < s} x[k] L(s, k)) / L(s, s)
__device__ __forceinline__ void pgo_row_solve(const double* l, double* x) {
#pragma unroll
    for (int s = 0; s < 6; s++) {
        double v = x[s];
#pragma unroll
        for (int k = 0; k < s; k++) v -= x[k] * PGO_L(s, k);
        x[s] = v / PGO_L(s, s);
    }
}
// L^T x = v
__device__ __forceinline__ void pgo_back_solve(const double* l, double* x) {
#pragma unroll
    for (int s = 5; s >= 0; s--) {
        double v = x[s];
#pragma unroll
        for (int k = s + 1; k < 6; k++) v -= PGO_L(k, s) * x[k];
        x[s] = v / PGO_L(s, s);
    }
}

// (H + lambda diag(H)) delta = rhs, H in `band` (overwritten by its factor), rhs overwritten by the forward solution y.
// One workgroup.  Per column c: (A) every thread factors the damped diagonal block and solves y_c in registers (redundantly: no
// broadcast is needed), the threads share the 6 bc block rows below it; (B) the threads share the 36 bc (bc + 1) / 2 elements of
// the trailing update and the 6 bc right-hand-side entries.  Two barriers per column; then the columns backwards.
// (the whole workgroup calls it; *flag: 1 if a pivot was not positive)
__device__ __forceinline__ void pgo_band_chol_walk(int nf, int b, double lambda, double* __restrict__ band,
                                                   const double* __restrict__ diagH, double* __restrict__ rhs,
                                                   double* __restrict__ delta, int* __restrict__ flag) {
    __shared__ double sPart[PGO_BACK_PARTS][6];
    const int tid = threadIdx.x;
    const size_t cs = (size_t)(b + 1) * 36;      // column stride
    int bad = 0;
    for (int c = 0; c < nf; c++) {
        const int bc = min(b, nf - 1 - c);
        double* col = band + (size_t)c * cs;
        double l[21];
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = 0; j <= i; j++) PGO_L(i, j) = col[6 * i + j];
#pragma unroll
        for (int i = 0; i < 6; i++) PGO_L(i, i) += lambda * diagH[(size_t)c * 6 + i];
        pgo_chol6(l, &bad);
        double y[6];
#pragma unroll
        for (int i = 0; i < 6; i++) y[i] = rhs[(size_t)c * 6 + i];
#pragma unroll
        for (int s = 0; s < 6; s++) {          // L y = rhs
            double v = y[s];
#pragma unroll
            for (int k = 0; k < s; k++) v -= PGO_L(s, k) * y[k];
            y[s] = v / PGO_L(s, s);
        }
        __syncthreads();                          // (every thread has read the column's diagonal block and rhs)
        for (int t = tid; t < 6 * bc; t += PGO_CHOL_NT) {
            double* row = col + (size_t)(1 + t / 6) * 36 + 6 * (t % 6);
            double x[6];
#pragma unroll
            for (int k = 0; k < 6; k++) x[k] = row[k];
            pgo_row_solve(l, x);
#pragma unroll
            for (int k = 0; k < 6; k++) row[k] = x[k];
        }
        if (tid == 0) {
#pragma unroll
            for (int i = 0; i < 6; i++) {
#pragma unroll
                for (int j = 0; j < 6; j++) col[6 * i + j] = j <= i ? PGO_L(i, j) : 0.0;
                rhs[(size_t)c * 6 + i] = y[i];
            }
        }
        __syncthreads();
        // trailing update: H[c + d1][c + d2] -= L[c + d1][c] L[c + d2][c]^T for bc >= d1 >= d2 >= 1
        const int nsq = bc * bc * 36;
        for (int t = tid; t < nsq; t += PGO_CHOL_NT) {
            const int e = t % 36, pr = t / 36;
            const int d1 = 1 + pr / bc, d2 = 1 + pr % bc;
            if (d1 < d2) continue;
            const double* a = col + (size_t)d1 * 36 + 6 * (e / 6);
            const double* bb = col + (size_t)d2 * 36 + 6 * (e % 6);
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < 6; k++) v += a[k] * bb[k];
            band[(size_t)(c + d2) * cs + (size_t)(d1 - d2) * 36 + e] -= v;
        }
        for (int t = tid; t < 6 * bc; t += PGO_CHOL_NT) {
            const double* a = col + (size_t)(1 + t / 6) * 36 + 6 * (t % 6);
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < 6; k++) v += a[k] * y[k];
            rhs[(size_t)(c + 1 + t / 6) * 6 + t % 6] -= v;
        }
        __syncthreads();
    }
    // back substitution: delta_c = L_cc^-T (y_c - sum_d L[c + d][c]^T delta_{c + d}); the sum in PGO_BACK_PARTS interleaved parts,
    // each in ascending d, added up in part order
    for (int c = nf - 1; c >= 0; c--) {
        const int bc = min(b, nf - 1 - c);
        const double* col = band + (size_t)c * cs;
        if (tid < 6 * PGO_BACK_PARTS) {
            const int s = tid % 6, part = tid / 6;
            double acc = 0.0;
            for (int d = 1 + part; d <= bc; d += PGO_BACK_PARTS) {
                const double* blk = col + (size_t)d * 36;
                const double* dl = delta + (size_t)(c + d) * 6;
                double v = 0.0;
#pragma unroll
                for (int k = 0; k < 6; k++) v += blk[6 * k + s] * dl[k];
                acc += v;
            }
            sPart[part][s] = acc;
        }
        __syncthreads();
        if (tid == 0) {
            double l[21], x[6];
#pragma unroll
            for (int i = 0; i < 6; i++)
#pragma unroll
                for (int j = 0; j <= i; j++) PGO_L(i, j) = col[6 * i + j];
#pragma unroll
            for (int s = 0; s < 6; s++) {
                double v = rhs[(size_t)c * 6 + s];
#pragma unroll
                for (int q = 0; q < PGO_BACK_PARTS; q++) v -= sPart[q][s];
                x[s] = v;
            }
            pgo_back_solve(l, x);
#pragma unroll
            for (int s = 0; s < 6; s++) delta[(size_t)c * 6 + s] = x[s];
        }
        __syncthreads();
    }
    if (tid == 0) *flag = bad;
}

// trial poses: T_k [Exp(a_k), b_k; 0, 1] for a free pose, the pose itself otherwise
__device__ __forceinline__ void pgo_retract_pose(int k, const int* __restrict__ pos, const double* __restrict__ poses,
                                                 const double* __restrict__ delta, double* __restrict__ trial) {
    double P[12];
#pragma unroll
    for (int q = 0; q < 12; q++) P[q] = poses[(size_t)k * 12 + q];
    const int c = pos[k];
    if (c >= 0) {
        double d[6], Ex[9], R[9], t[3];
#pragma unroll
        for (int q = 0; q < 6; q++) d[q] = delta[(size_t)c * 6 + q];
        so3_expmap(d, Ex);
        mat3_mul(P, Ex, R);
        mat3_vec(P, d + 3, t);
#pragma unroll
        for (int q = 0; q < 9; q++) P[q] = R[q];
#pragma unroll
        for (int q = 0; q < 3; q++) P[9 + q] += t[q];
    }
#pragma unroll
    for (int q = 0; q < 12; q++) trial[(size_t)k * 12 + q] = P[q];
}

// out[0] = sum of cost[0 .. m) (thread t adds entries t, t + 256, ... in order; then a fixed tree), out[1] = max |delta|
__device__ __forceinline__ void pgo_reduce_sum(int tid, int m, const double* __restrict__ cost, int nd, const double* __restrict__ delta,
                                               double* __restrict__ out, double* sS, double* sM) {
    double s = 0.0, mx = 0.0;
    for (int k = tid; k < m; k += PGO_RED_NT) s += cost[k];
    for (int k = tid; k < nd; k += PGO_RED_NT) { const double a = fabs(delta[k]); if (!(a <= mx)) mx = a; }     // (a NaN sticks)
    sS[tid] = s; sM[tid] = mx;
    __syncthreads();
    for (int h = PGO_RED_NT / 2; h > 0; h >>= 1) {
        if (tid < h) { sS[tid] += sS[tid + h]; if (!(sM[tid + h] <= sM[tid])) sM[tid] = sM[tid + h]; }
        __syncthreads();
    }
    if (tid == 0) { out[0] = sS[0]; out[1] = sM[0]; }
}

// A graph's Levenberg-Marquardt loop state, on the device.
constexpr int PGO_NEED_H = 1, PGO_NEED_J = 2;       // need_linearize: assemble H and g (1), from a fresh linearisation (1 | 2)
struct PgoCtl {
    int active, need_linearize, cur;        // cur: which of the two value buffers holds the accepted values
    int accepted, rejected, pad;
    double lambda, cost, initial_cost;
};

// THE accept / reject rule of the Levenberg-Marquardt loop (include/vslam_hip.h), fp64: one trial of an active graph.
// cn: the trial's cost; dmax: |delta|_inf; bad: a pivot was not positive.
__device__ __forceinline__ void pgo_lm_decide(PgoCtl& c, double cn, double dmax, int bad, int maxIt) {
    const bool tiny = !bad && dmax < 1e-12;      // (a flagged factorisation's delta means nothing: the trial is only rejected)
    if (!bad && isfinite(cn) && cn < c.cost) {
        const double rel = (c.cost - cn) / c.cost;
        c.cur ^= 1;
        c.cost = cn; c.accepted++;
        const double l3 = c.lambda / 3.0;
        c.lambda = l3 < 1e-12 ? 1e-12 : l3;
        if (c.accepted >= maxIt || rel < 1e-10 || tiny) c.active = 0;
        c.need_linearize = PGO_NEED_H | PGO_NEED_J;
    } else {
        c.rejected++;
        c.lambda *= 4.0;
        if (c.lambda > 1e8 || tiny) c.active = 0;
        c.need_linearize = 0;
    }
}

}  // namespace
