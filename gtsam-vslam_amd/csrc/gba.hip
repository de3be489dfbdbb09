// Global bundle adjustment on the device (no reference counterpart; DESIGN.md section 6 item 27, restated by tests/gba_ref.py):
// Levenberg-Marquardt over ALL keyframes and landmarks of a flattened problem (vslam_ba_problem), projection factors plus the
// caller's relative-pose edges, the landmarks eliminated onto the keyframes (Schur complement) and the reduced camera system
// solved DIRECTLY by the pose-graph solve's block-banded fp64 Cholesky (pgo_dev.hpp) after its reordering (gba_host.hpp).  No
// cap of 170 free keyframes: the band, not a dense matrix, bounds the call.  No floating-point atomics: every sum runs over a
// list built once per call on the host, in list order, so two calls on the same input return the same bytes.
//   k_gba_linearize / k_gba_edge_linearize   a thread per factor slot (pair, side) / per edge: residual, Jacobians, cost term;
//                         they run only after an accepted trial
//   k_gba_landmark        a thread per present landmark: the damped 3x3 block, its inverse, the gradient
//   k_gba_wy              a thread per pair on a free keyframe: W (6x3) and Y = W Hll^-1
//   k_gba_edge_columns    a wave per block column: the edges' blocks and gradient (pgo_assemble_column); it also clears the column
//   k_gba_gather          a wave per block of the band that a shared landmark fills: lane e < 36 owns an element and walks the
//                         block's (pair, pair) list; lanes 36 .. 41 of a diagonal block own the right-hand side
//   k_gba_band_copy / k_gba_band_chol        H and g into the factor's arrays; one workgroup walks the block columns
//   k_gba_back / k_gba_retract               a thread per landmark walks its pairs: the landmark step; the trial poses
//   k_gba_cost / k_gba_edge_cost / k_gba_reduce_decide   the trial's cost terms, their fixed-order sum, the accept / reject rule
//                         (pgo_lm_decide) on a device control block
//   k_gba_chi2            a thread per pair: the outlier flags at the final values
// The host waits once per trial, for one int.
#include "common.hpp"
#include "dmath.hpp"
#include "pgo_dev.hpp"
#include "gba_host.hpp"
#include <cmath>

using namespace vslam;

namespace {

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

// the problem's arrays on the device (read-only for the kernels) and the sizes
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
__global__ __launch_bounds__(256) void k_gba_linearize(GbaDev D, const PgoCtl* __restrict__ ctl, int init, const double* __restrict__ P0,
                                                       const double* __restrict__ P1, const double* __restrict__ L0,
                                                       const double* __restrict__ L1, double* __restrict__ Jp, double* __restrict__ Jl,
                                                       double* __restrict__ res, double* __restrict__ cost) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
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
__global__ __launch_bounds__(256) void k_gba_cost(GbaDev D, const PgoCtl* __restrict__ ctl, const double* __restrict__ P0,
                                                  const double* __restrict__ P1, const double* __restrict__ L0,
                                                  const double* __restrict__ L1, double* __restrict__ cost) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
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

__global__ __launch_bounds__(256) void k_gba_edge_linearize(GbaDev D, const PgoCtl* __restrict__ ctl, int init, const double* __restrict__ P0,
                                                            const double* __restrict__ P1, double* __restrict__ res, double* __restrict__ Ji,
                                                            double* __restrict__ Jj, double* __restrict__ cost) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= D.M) return;
    if (!init && !(ctl->active && (ctl->need_linearize & PGO_NEED_J))) return;
    pgo_linearize_edge(e, D.edges, ctl->cur ? P1 : P0, res, Ji, Jj, cost);
}

__global__ __launch_bounds__(256) void k_gba_edge_cost(GbaDev D, const PgoCtl* __restrict__ ctl, const double* __restrict__ P0,
                                                       const double* __restrict__ P1, double* __restrict__ cost) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= D.M || !ctl->active) return;
    pgo_cost_edge(e, D.edges, ctl->cur ? P0 : P1, cost);
}

// Hll = sum Jl^T Jl over the landmark's factors, damped by lambda diag(Hll); Hinv [9] by cofactors; gl = sum Jl^T r.
// A pivot of the damped block that is not positive raises *flag.
__global__ __launch_bounds__(256) void k_gba_landmark(GbaDev D, const PgoCtl* __restrict__ ctl, const double* __restrict__ Jl,
                                                      const double* __restrict__ res, double* __restrict__ Hinv, double* __restrict__ gl,
                                                      int* __restrict__ flag) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
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
__global__ __launch_bounds__(256) void k_gba_wy(GbaDev D, const PgoCtl* __restrict__ ctl, const double* __restrict__ Jp,
                                                const double* __restrict__ Jl, const double* __restrict__ Hinv, double* __restrict__ W,
                                                double* __restrict__ Y) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
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
__global__ __launch_bounds__(64) void k_gba_edge_columns(GbaDev D, const PgoCtl* __restrict__ ctl, const double* __restrict__ res,
                                                         const double* __restrict__ Ji, const double* __restrict__ Jj,
                                                         double* __restrict__ band, double* __restrict__ diagH, double* __restrict__ g) {
    const int c = blockIdx.x, lane = threadIdx.x;
    if (c >= D.nf || lane >= 42 || !ctl->active) return;
    pgo_assemble_column(c, lane, D.nf, D.b, D.pos, D.rowStart, D.inc, D.edges, res, Ji, Jj, band, diagH, g);
}

// Block i of the landmark lists: H[c + d][c] += sum over its entries (p1 on c + d, p2 on c) of -Y_p1 W_p2^T, and on the diagonal
// (p1 == p2) the pair's Jp^T Jp; lanes 36 .. 41 of a diagonal block: g_c -= Jp^T r - Y_p gl.  diagH gets the undamped pose
// diagonal (Jp^T Jp alone).  It runs after k_gba_edge_columns, which wrote the block.
__global__ __launch_bounds__(64) void k_gba_gather(GbaDev D, const PgoCtl* __restrict__ ctl, const double* __restrict__ Jp,
                                                   const double* __restrict__ res, const double* __restrict__ W, const double* __restrict__ Y,
                                                   const double* __restrict__ gl, double* __restrict__ band, double* __restrict__ diagH,
                                                   double* __restrict__ g) {
    const int i = blockIdx.x, lane = threadIdx.x;
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

__global__ __launch_bounds__(256) void k_gba_band_copy(GbaDev D, const PgoCtl* __restrict__ ctl, const double* __restrict__ bandH,
                                                       const double* __restrict__ g, double* __restrict__ bandL, double* __restrict__ rhs) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)(D.b + 1) * D.nf * 36 || !ctl->active) return;
    bandL[t] = bandH[t];
    if (t < (size_t)D.nf * 6) rhs[t] = g[t];
}

__global__ __launch_bounds__(PGO_CHOL_NT) void k_gba_band_chol(GbaDev D, const PgoCtl* __restrict__ ctl, double* __restrict__ bandL,
                                                               const double* __restrict__ diagH, double* __restrict__ rhs,
                                                               double* __restrict__ delta, int* __restrict__ flag) {
    if (!ctl->active) return;
    pgo_band_chol_walk(D.nf, D.b, ctl->lambda, bandL, diagH, rhs, delta, flag);
}

// the landmark step dX = Hinv (-gl - sum W_p^T delta_kf(p)) over the landmark's pairs on free keyframes, in list order; the trial
// landmark; a thin landmark's trial value is its value.  The steps follow the poses' in `delta` (|delta|_inf covers both).
__global__ __launch_bounds__(256) void k_gba_back(GbaDev D, const PgoCtl* __restrict__ ctl, const double* __restrict__ W,
                                                  const double* __restrict__ Hinv, const double* __restrict__ gl, double* __restrict__ L0,
                                                  double* __restrict__ L1, double* __restrict__ delta) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
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

__global__ __launch_bounds__(256) void k_gba_retract(GbaDev D, const PgoCtl* __restrict__ ctl, double* __restrict__ P0, double* __restrict__ P1,
                                                     const double* __restrict__ delta) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= D.K || !ctl->active) return;
    pgo_retract_pose(k, D.pos, ctl->cur ? P1 : P0, delta, ctl->cur ? P0 : P1);
}

// One workgroup: the fixed-order sum of the nCost cost terms and |delta|_inf, then thread 0 applies the rule (pgo_lm_decide).
// init: the initial cost; the call becomes active iff it exceeds 1e-20 and there is an unknown.  *nActive: what the host reads.
__global__ __launch_bounds__(PGO_RED_NT) void k_gba_reduce_decide(int init, int maxIt, int nCost, int nDelta, int hasUnknowns,
                                                                  PgoCtl* __restrict__ ctl, const double* __restrict__ cost,
                                                                  const double* __restrict__ delta, double* __restrict__ out,
                                                                  int* __restrict__ flagChol, int* __restrict__ flagLm, int* __restrict__ nActive) {
    __shared__ double sS[PGO_RED_NT], sM[PGO_RED_NT];
    if (!init && !ctl->active) return;
    pgo_reduce_sum(threadIdx.x, nCost, cost, init ? 0 : nDelta, delta, out, sS, sM);
    if (threadIdx.x != 0) return;
    PgoCtl c = *ctl;
    if (init) {
        c.cost = c.initial_cost = out[0];
        c.active = (c.cost > 1e-20) && hasUnknowns;
        c.need_linearize = PGO_NEED_H;
        *flagChol = 0;
    } else {
        pgo_lm_decide(c, out[0], out[1], *flagChol | *flagLm, maxIt);
    }
    *flagLm = 0;
    *ctl = c;
    *nActive = c.active;
}

// the local BA's chi2 rule at the final values: pairs of kf_local keyframes on present landmarks, left then right
__global__ __launch_bounds__(256) void k_gba_chi2(GbaDev D, const PgoCtl* __restrict__ ctl, const double* __restrict__ P0,
                                                  const double* __restrict__ P1, const double* __restrict__ L0, const double* __restrict__ L1,
                                                  uint8_t* __restrict__ wrong) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
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

thread_local std::vector<std::pair<const char*, float>> g_gbaTimes;
thread_local bool g_gbaTimingOn = false;

struct GbaLayout {
    size_t bytes = 0;
    size_t section(size_t n) { const size_t at = bytes; bytes = align_up_sz(bytes + std::max<size_t>(n, 8), 256); return at; }
};

inline bool gba_finite(const double* p, size_t n) { for (size_t k = 0; k < n; k++) if (!std::isfinite(p[k])) return false; return true; }
inline unsigned gba_grid(size_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

extern "C" vslam_status vslam_global_ba_set_timing(int32_t on) {
    g_gbaTimingOn = on != 0;
    g_gbaTimes.clear();
    return VSLAM_OK;
}

extern "C" vslam_status vslam_global_ba_timings(const char** names, float* ms, int32_t cap, int32_t* n_out) {
    if (!n_out || cap < 0 || (cap > 0 && (!names || !ms))) return VSLAM_ERR_INVALID;
    int n = 0;
    for (const auto& t : g_gbaTimes) { if (n >= cap) break; names[n] = t.first; ms[n] = t.second; n++; }
    *n_out = n;
    return VSLAM_OK;
}

extern "C" vslam_status vslam_global_ba(const vslam_ba_problem* problem, const vslam_pgo_edge* edges, int32_t n_edges,
                                        const vslam_gba_params* params, int32_t device, vslam_gba_result* result) {
    static const char* const who = "vslam_global_ba";
    if (!problem || !result) { set_error("%s: invalid arguments", who); return VSLAM_ERR_INVALID; }
    const vslam_ba_problem& Q = *problem;
    int maxIt = params ? params->max_iterations : 0;
    double lambda0 = params ? params->lambda0 : 0.0;
    if (maxIt < 0 || !(lambda0 >= 0.0) || !std::isfinite(lambda0)) { set_error("%s: negative or non-finite parameter", who); return VSLAM_ERR_INVALID; }
    if (maxIt == 0) maxIt = 20;
    if (lambda0 == 0.0) lambda0 = 1e-4;
    const int K = Q.n_kf, L = Q.n_lm, P = Q.n_pairs, M = n_edges;
    if (K < 1 || L < 0 || P < 0 || M < 0 || !Q.kf_pose_wc || !Q.kf_fixed || !Q.kf_local || !result->kf_pose_wc || (L > 0 && (!Q.lm_xyz || !result->lm_xyz)) ||
        (P > 0 && (!Q.pair_kf || !Q.pair_lm || !Q.pair_flags || !Q.pair_uv || !Q.pair_octave || !result->pair_wrong || !Q.sigma_factor || !Q.inv_sigma_factor || Q.n_levels < 1)) ||
        (M > 0 && !edges)) {
        set_error("%s: invalid arguments", who); return VSLAM_ERR_INVALID;
    }
    // host plan: presence, free set, gauge, reordering, lists (its limits come first)
    std::vector<int32_t> ei(std::max(M, 1)), ej(std::max(M, 1));
    GbaIndex I;
    I.n_kf = K; I.kf_fixed = Q.kf_fixed; I.n_lm = L; I.n_pairs = P; I.pair_kf = Q.pair_kf; I.pair_lm = Q.pair_lm; I.pair_flags = Q.pair_flags;
    I.n_edges = M; I.edge_i = ei.data(); I.edge_j = ej.data();
    GbaPlan G;
    if (const int st = gba_check_sizes(I, G)) { set_error("%s: %s", who, G.err.c_str()); return (vslam_status)st; }
    for (int e = 0; e < M; e++) { ei[e] = edges[e].i; ej[e] = edges[e].j; }
    if (const int st = gba_plan(I, G)) { set_error("%s: %s", who, G.err.c_str()); return (vslam_status)st; }
    if (!gba_finite(Q.kf_pose_wc, (size_t)K * 16) || !gba_finite(Q.lm_xyz, (size_t)L * 3) || !std::isfinite(Q.rig.fx) || !std::isfinite(Q.rig.fy) ||
        !std::isfinite(Q.rig.cx) || !std::isfinite(Q.rig.cy) || !std::isfinite(Q.rig.baseline)) {
        set_error("%s: non-finite pose, landmark or camera", who); return VSLAM_ERR_INVALID;
    }
    for (int e = 0; e < M; e++) {
        const vslam_pgo_edge& E = edges[e];
        if (!gba_finite(E.Z, 16) || !std::isfinite(E.w_rot) || !std::isfinite(E.w_trans)) { set_error("%s: edge %d has a non-finite value", who, e); return VSLAM_ERR_INVALID; }
        if (E.w_rot < 0 || E.w_trans < 0) { set_error("%s: edge %d has a negative weight", who, e); return VSLAM_ERR_INVALID; }
    }
    const int nf = G.nf, b = G.b;
    // device forms: poses [12], whitening and chi2 threshold per factor slot; the initial depth of every present factor
    std::vector<double> hp((size_t)K * 12), his((size_t)std::max(P, 1) * 2, 0.0), hthr((size_t)std::max(P, 1) * 2, 0.0);
    for (int k = 0; k < K; k++)
        for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) hp[(size_t)k * 12 + 3 * r + c] = Q.kf_pose_wc[(size_t)k * 16 + 4 * r + c]; hp[(size_t)k * 12 + 9 + r] = Q.kf_pose_wc[(size_t)k * 16 + 4 * r + 3]; }
    for (int p = 0; p < P; p++) {
        const int fl = Q.pair_flags[p] & 3, lm = Q.pair_lm[p];
        if (!fl || !G.lmPresent[lm]) continue;
        for (int side = 0; side < 2; side++) {
            if (!((fl >> side) & 1)) continue;
            const int oct = Q.pair_octave[2 * (size_t)p + side];
            if (oct < 0 || oct >= Q.n_levels) { set_error("%s: pair %d has octave %d of %d levels", who, p, oct, Q.n_levels); return VSLAM_ERR_INVALID; }
            if (!std::isfinite(Q.pair_uv[4 * (size_t)p + 2 * side]) || !std::isfinite(Q.pair_uv[4 * (size_t)p + 2 * side + 1])) { set_error("%s: pair %d has a non-finite measurement", who, p); return VSLAM_ERR_INVALID; }
            his[2 * (size_t)p + side] = 1.0 / (1.0 / (double)Q.inv_sigma_factor[oct]);           // sigma = 1 / inv_sigma_factor
            hthr[2 * (size_t)p + side] = (double)(float)((double)7.815f * (double)Q.sigma_factor[oct]);
        }
        const double* T = &hp[(size_t)Q.pair_kf[p] * 12];
        const double* X = Q.lm_xyz + (size_t)lm * 3;
        const double z = T[2] * (X[0] - T[9]) + T[5] * (X[1] - T[10]) + T[8] * (X[2] - T[11]);
        if (!(z > 0.0)) { set_error("%s: pair %d (keyframe %d, landmark %d) is not in front of its camera at the initial values", who, p, Q.pair_kf[p], lm); return VSLAM_ERR_INVALID; }
    }
    std::vector<PgoEdge> he(std::max(M, 1), PgoEdge{});
    for (int e = 0; e < M; e++) {
        PgoEdge& o = he[e];
        o.i = edges[e].i; o.j = edges[e].j; o.wr = edges[e].w_rot; o.wt = edges[e].w_trans;
        for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) o.Rz[3 * r + c] = edges[e].Z[4 * r + c]; o.tz[r] = edges[e].Z[4 * r + 3]; }
    }

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available (no CPU fallback)"); return VSLAM_ERR_NO_DEVICE; }
    if (device < 0 || device >= ndev) { set_error("%s: no device %d", who, device); return VSLAM_ERR_INVALID; }
    VS_HIP(hipSetDevice(device));
    DevPool* pool = thread_pool(device);
    if (!pool) { set_error("no device pool"); return VSLAM_ERR_HIP; }
    pool->pending.clear();
    hipStream_t st = pool->stream;

    GbaLayout up, wk;
    const size_t nList = (size_t)G.blkStart.back();
    const size_t oCtl = up.section(sizeof(PgoCtl)), oE = up.section((size_t)M * sizeof(PgoEdge)), oP0 = up.section((size_t)K * 96), oL0 = up.section((size_t)L * 24);
    const size_t oPos = up.section((size_t)K * 4), oRow = up.section((size_t)(nf + 1) * 4), oInc = up.section((size_t)G.rowStart[nf] * 4);
    const size_t oPk = up.section((size_t)P * 4), oPl = up.section((size_t)P * 4), oPf = up.section((size_t)P), oUv = up.section((size_t)P * 16);
    const size_t oIs = up.section((size_t)P * 16), oThr = up.section((size_t)P * 16), oLoc = up.section((size_t)K), oPres = up.section((size_t)L);
    const size_t oLs = up.section((size_t)(L + 1) * 4), oLp = up.section((size_t)G.lmStart[L] * 4);
    const size_t oBc = up.section((size_t)G.nBlk * 4), oBd = up.section((size_t)G.nBlk * 4), oBs = up.section((size_t)(G.nBlk + 1) * 4), oLi = up.section(nList * 8);
    const size_t bandBytes = (size_t)(b + 1) * nf * 36 * 8, vecBytes = (size_t)nf * 48;
    const size_t oP1 = wk.section((size_t)K * 96), oL1 = wk.section((size_t)L * 24);
    const size_t oJp = wk.section((size_t)P * 24 * 8), oJl = wk.section((size_t)P * 12 * 8), oRes = wk.section((size_t)P * 4 * 8);
    const size_t oCost = wk.section(((size_t)P * 2 + M) * 8), oERes = wk.section((size_t)M * 48), oEJi = wk.section((size_t)M * 288), oEJj = wk.section((size_t)M * 288);
    const size_t oHinv = wk.section((size_t)L * 72), oGl = wk.section((size_t)L * 24), oW = wk.section((size_t)P * 144), oY = wk.section((size_t)P * 144);
    const size_t oBandH = wk.section(bandBytes), oBandL = wk.section(bandBytes), oDiag = wk.section(vecBytes), oG = wk.section(vecBytes), oRhs = wk.section(vecBytes);
    const size_t oDelta = wk.section(vecBytes + (size_t)L * 24), oOut = wk.section(16), oFlagC = wk.section(4), oFlagL = wk.section(4), oAct = wk.section(4);
    const size_t oWrong = wk.section((size_t)P);
    std::vector<uint8_t> hUp(up.bytes, 0);
    auto put = [&](size_t at, const void* src, size_t n) { if (n) memcpy(hUp.data() + at, src, n); };
    PgoCtl c0{};
    c0.lambda = lambda0;
    put(oCtl, &c0, sizeof c0); put(oE, he.data(), (size_t)M * sizeof(PgoEdge)); put(oP0, hp.data(), (size_t)K * 96); put(oL0, Q.lm_xyz, (size_t)L * 24);
    put(oPos, G.pos.data(), (size_t)K * 4); put(oRow, G.rowStart.data(), (size_t)(nf + 1) * 4); put(oInc, G.inc.data(), (size_t)G.rowStart[nf] * 4);
    put(oPk, Q.pair_kf, (size_t)P * 4); put(oPl, Q.pair_lm, (size_t)P * 4); put(oPf, Q.pair_flags, (size_t)P); put(oUv, Q.pair_uv, (size_t)P * 16);
    put(oIs, his.data(), (size_t)P * 16); put(oThr, hthr.data(), (size_t)P * 16); put(oLoc, Q.kf_local, (size_t)K); put(oPres, G.lmPresent.data(), (size_t)L);
    put(oLs, G.lmStart.data(), (size_t)(L + 1) * 4); put(oLp, G.lmPairs.data(), (size_t)G.lmStart[L] * 4);
    put(oBc, G.blkC.data(), (size_t)G.nBlk * 4); put(oBd, G.blkD.data(), (size_t)G.nBlk * 4); put(oBs, G.blkStart.data(), (size_t)(G.nBlk + 1) * 4);
    put(oLi, G.list.data(), nList * 8);
    PoolBuf<uint8_t> dUp(pool), dWk(pool);
    VS_HIP(dUp.up(hUp.data(), up.bytes)); VS_HIP(dWk.alloc(wk.bytes));
    GbaDev D{};
    D.K = K; D.L = L; D.P = P; D.M = M; D.nf = nf; D.b = b; D.nBlk = G.nBlk;
    D.cam = GbaCam{Q.rig.fx, Q.rig.fy, Q.rig.cx, Q.rig.cy, (double)Q.rig.baseline};
    D.edges = (const PgoEdge*)(dUp.p + oE); D.pos = (const int*)(dUp.p + oPos); D.rowStart = (const int*)(dUp.p + oRow); D.inc = (const int*)(dUp.p + oInc);
    D.pairKf = (const int*)(dUp.p + oPk); D.pairLm = (const int*)(dUp.p + oPl); D.pairFlags = dUp.p + oPf; D.pairUv = (const float*)(dUp.p + oUv);
    D.pairIs = (const double*)(dUp.p + oIs); D.pairThr = (const double*)(dUp.p + oThr); D.kfLocal = dUp.p + oLoc; D.lmPresent = dUp.p + oPres;
    D.lmStart = (const int*)(dUp.p + oLs); D.lmPairs = (const int*)(dUp.p + oLp);
    D.blkC = (const int*)(dUp.p + oBc); D.blkD = (const int*)(dUp.p + oBd); D.blkStart = (const int*)(dUp.p + oBs); D.list = (const int*)(dUp.p + oLi);
    PgoCtl* dCtl = (PgoCtl*)(dUp.p + oCtl);
    double* dP0 = (double*)(dUp.p + oP0); double* dL0 = (double*)(dUp.p + oL0);
    auto W8 = [&](size_t at) { return (double*)(dWk.p + at); };
    double* dP1 = W8(oP1); double* dL1 = W8(oL1); double* dJp = W8(oJp); double* dJl = W8(oJl); double* dRes = W8(oRes); double* dCost = W8(oCost);
    double* dERes = W8(oERes); double* dEJi = W8(oEJi); double* dEJj = W8(oEJj); double* dHinv = W8(oHinv); double* dGl = W8(oGl);
    double* dW = W8(oW); double* dY = W8(oY); double* dBandH = W8(oBandH); double* dBandL = W8(oBandL); double* dDiag = W8(oDiag);
    double* dG = W8(oG); double* dRhs = W8(oRhs); double* dDelta = W8(oDelta); double* dOut = W8(oOut);
    int* dFlagC = (int*)(dWk.p + oFlagC); int* dFlagL = (int*)(dWk.p + oFlagL); int* dAct = (int*)(dWk.p + oAct);
    uint8_t* dWrong = dWk.p + oWrong;

    struct TimerOwner { StageTimer t; ~TimerOwner() { t.destroy(); } } timerOwner;
    StageTimer& timer = timerOwner.t;
    timer.stream = st; timer.multi = true; timer.enabled = g_gbaTimingOn;
    const int nCost = 2 * P + M, nDelta = nf * 6 + L * 3, hasUnknowns = (nf > 0 || G.nPresent > 0) ? 1 : 0;
    const dim3 gSlot(gba_grid((size_t)2 * P)), gEdge(gba_grid(M)), gLm(gba_grid(L)), gPair(gba_grid(P)), gKf(gba_grid(K)), B256(256);
    int nActive = 0;
    auto linearize = [&](int init) {
        const int t = timer.begin("gba_linearize");
        if (P) hipLaunchKernelGGL(k_gba_linearize, gSlot, B256, 0, st, D, dCtl, init, dP0, dP1, dL0, dL1, dJp, dJl, dRes, dCost);
        if (M) hipLaunchKernelGGL(k_gba_edge_linearize, gEdge, B256, 0, st, D, dCtl, init, dP0, dP1, dERes, dEJi, dEJj, dCost + (size_t)2 * P);
        timer.end(t);
    };
    auto decide = [&](int init, int t) -> vslam_status {        // closes the gba_cost group `t`, then the trial's one wait
        hipLaunchKernelGGL(k_gba_reduce_decide, dim3(1), dim3(PGO_RED_NT), 0, st, init, maxIt, nCost, nDelta, hasUnknowns, dCtl, dCost, dDelta, dOut, dFlagC, dFlagL, dAct);
        timer.end(t);
        VS_HIP(hipGetLastError());
        VS_HIP(pool->d2h(&nActive, dAct, sizeof(int)));
        VS_HIP(pool->sync());
        return VSLAM_OK;
    };
    linearize(1);
    VS_CHECK(decide(1, timer.begin("gba_cost")));
    while (nActive > 0) {       // one trial
        linearize(0);
        int t = timer.begin("gba_landmarks");
        if (L) hipLaunchKernelGGL(k_gba_landmark, gLm, B256, 0, st, D, dCtl, dJl, dRes, dHinv, dGl, dFlagL);
        if (P && nf) hipLaunchKernelGGL(k_gba_wy, gPair, B256, 0, st, D, dCtl, dJp, dJl, dHinv, dW, dY);
        timer.end(t);
        t = timer.begin("gba_assemble");
        if (nf) hipLaunchKernelGGL(k_gba_edge_columns, dim3(nf), dim3(64), 0, st, D, dCtl, dERes, dEJi, dEJj, dBandH, dDiag, dG);
        if (G.nBlk) hipLaunchKernelGGL(k_gba_gather, dim3(G.nBlk), dim3(64), 0, st, D, dCtl, dJp, dRes, dW, dY, dGl, dBandH, dDiag, dG);
        timer.end(t);
        t = timer.begin("gba_band_chol");
        if (nf) hipLaunchKernelGGL(k_gba_band_copy, dim3(gba_grid((size_t)(b + 1) * nf * 36)), B256, 0, st, D, dCtl, dBandH, dG, dBandL, dRhs);
        hipLaunchKernelGGL(k_gba_band_chol, dim3(1), dim3(PGO_CHOL_NT), 0, st, D, dCtl, dBandL, dDiag, dRhs, dDelta, dFlagC);
        timer.end(t);
        t = timer.begin("gba_back");
        if (L) hipLaunchKernelGGL(k_gba_back, gLm, B256, 0, st, D, dCtl, dW, dHinv, dGl, dL0, dL1, dDelta);
        hipLaunchKernelGGL(k_gba_retract, gKf, B256, 0, st, D, dCtl, dP0, dP1, dDelta);
        timer.end(t);
        t = timer.begin("gba_cost");
        if (P) hipLaunchKernelGGL(k_gba_cost, gSlot, B256, 0, st, D, dCtl, dP0, dP1, dL0, dL1, dCost);
        if (M) hipLaunchKernelGGL(k_gba_edge_cost, gEdge, B256, 0, st, D, dCtl, dP0, dP1, dCost + (size_t)2 * P);
        VS_CHECK(decide(0, t));
    }
    int t = timer.begin("gba_chi2");
    if (P) hipLaunchKernelGGL(k_gba_chi2, gPair, B256, 0, st, D, dCtl, dP0, dP1, dL0, dL1, dWrong);
    timer.end(t);
    VS_HIP(hipGetLastError());
    PgoCtl ctl{};
    VS_HIP(pool->d2h(&ctl, dCtl, sizeof ctl));
    VS_HIP(pool->sync());
    std::vector<double> hl((size_t)std::max(L, 1) * 3);
    std::vector<uint8_t> hw(std::max(P, 1));
    VS_HIP(pool->d2h(hp.data(), ctl.cur ? dP1 : dP0, (size_t)K * 96));
    VS_HIP(pool->d2h(hl.data(), ctl.cur ? dL1 : dL0, (size_t)L * 24));
    VS_HIP(pool->d2h(hw.data(), dWrong, (size_t)P));
    VS_HIP(pool->sync());
    if (timer.enabled) {
        const char* names[8]; float ms[8];
        const int k = timer.read(names, ms, 8);
        g_gbaTimes.clear();
        for (int q = 0; q < k; q++) g_gbaTimes.push_back({names[q], ms[q]});
    }
    // nothing is written before the last wait has returned; fixed and isolated keyframes and thin landmarks are the input's bytes
    for (int k = 0; k < K; k++) {
        double* o = result->kf_pose_wc + (size_t)k * 16;
        const double* in = Q.kf_pose_wc + (size_t)k * 16;
        if (G.pos[k] < 0) { if (o != in) memcpy(o, in, 128); continue; }
        for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) o[4 * r + c] = hp[(size_t)k * 12 + 3 * r + c]; o[4 * r + 3] = hp[(size_t)k * 12 + 9 + r]; }
        o[12] = o[13] = o[14] = 0.0; o[15] = 1.0;
    }
    for (int l = 0; l < L; l++) {
        double* o = result->lm_xyz + (size_t)l * 3;
        const double* in = G.lmPresent[l] ? &hl[(size_t)l * 3] : Q.lm_xyz + (size_t)l * 3;
        if (o != in) memcpy(o, in, 24);
    }
    if (P) memcpy(result->pair_wrong, hw.data(), (size_t)P);
    vslam_gba_report& R = result->report;
    R = vslam_gba_report{};
    R.accepted = ctl.accepted; R.rejected = ctl.rejected; R.iterations = ctl.accepted + ctl.rejected;
    R.n_free = nf; R.n_isolated = G.nIso; R.n_present = G.nPresent; R.n_thin = G.nThin; R.n_factors = G.nFactors; R.half_bandwidth = b;
    R.initial_cost = ctl.initial_cost; R.final_cost = ctl.cost; R.final_lambda = ctl.lambda;
    return VSLAM_OK;
}
