// Local bundle adjustment on gfx950 (K11/K12): numerical core of LocalMapper::localBA
// (reference src/OptimizationBA.cpp:543-873, setOrdering :942-953, checkOutlier(R) :393-424).
//
// Per LM step (one linearisation if due + one lambda trial); every kernel first checks the device-side LM state:
//   k_ba_factors<0>  ONE launch: obs-parallel whitened residual, 2x6 pose and 2x3 landmark Jacobian blocks of every
//                    GenericProjectionFactor (left, or right with the stereo extrinsics), stored as 20 doubles per
//                    observation; one workgroup per BetweenFactor<Pose3> edge (Logmap residual, LogmapDerivative /
//                    Adjoint Jacobians, 6x6 products); last-workgroup deterministic cost reduction; LM control.
//   k_ba_schur       landmark-parallel, one 64-lane wave per landmark, 16 per workgroup: Hll (+lambda I) inverse by
//                    cofactors, W = Hpl blocks staged in LDS, S -= W Hll^-1 W^T and rhs -= W Hll^-1 bl
//                    accumulated in a workgroup-private copy of the reduced camera system in LDS
//                    (6F x 6F doubles, F = free keyframes) and flushed once per workgroup; when that
//                    copy exceeds LDS (F > 20) the same updates go to HBM with fp64 atomics.
//   k_ba_reduce      sums the partial systems (the buffer the landmark-sharded multi-GPU path all-reduces over RCCL).
//   k_ba_solve_*     reduced camera system + damping, Cholesky + substitutions, trial poses: one wave with the 10
//                    16x16 tiles in MFMA accumulators (6F <= 64), eight waves with 136 tiles (6F <= 256), LDS / L2
//                    row-per-thread beyond.
//   k_ba_back        landmark-parallel back-substitution, trial landmark positions.
//   k_ba_factors<1>  linearised cost at delta (GTSAM's linear.error(delta)), nonlinear cost at the trial values,
//                    reduction, and the LM decision (accept / reject, lambda, convergence) - k_ba_ctl when the sums
//                    are all-reduced first.
// The LM policy (GTSAM 4.2) runs on the DEVICE (control block `ctl`); the host enqueues speculative
// steps and reads the block back to learn that a pass is done.  Both passes (5 then 10 iterations) start from the
// caller's values, separated by the chi2 re-check kernel.
#include "common.hpp"
#include "comm.hpp"
#include "dmath.hpp"
#include "ba_pool.hpp"
#include "ba_packed.hpp"
#include "ba_types.hpp"           // argument blocks, control block, launch constants
#include "ba_order_host.hpp"      // host: ordering, membership, second-pass statistics, reports
#include "ba_plan.hpp"            // host: launch geometry
#include "grow_buf.hpp"           // host: the grow-only buffers of the workspaces
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <memory>
#include <mutex>
#include <type_traits>
#include <vector>

namespace vslam {

static_assert(BA_MAX_LEVELS == MAX_LEVELS, "BaChi::thr holds one threshold per pyramid level");
// value slot of candidate c (BaDev: NB + 1 slots, `sel` is current)
__device__ __forceinline__ int ba_slot(int sel, int c, int NB) {
    const int s = sel + 1 + c;
    return s > NB ? s - (NB + 1) : s;
}
__device__ __forceinline__ bool ba_enter(BaDev& D, int state, int c = 0) {
    const int* ci = (const int*)(D.ctl + CTL_INTS);
    if (ci[CI_STATE] != state) return false;
    D.nAct = ci[CI_NACT];
    if (c >= D.nAct) return false;
    const int sel = ci[CI_SEL], ts = ba_slot(sel, c, D.NB);
    D.cand = c;
    D.poseCur = D.poseBase + (size_t)sel * D.K; D.poseTrial = D.poseBase + (size_t)ts * D.K;
    D.lmCur = D.lmBase + (size_t)sel * D.lmStride; D.lmTrial = D.lmBase + (size_t)ts * D.lmStride;
    if (D.specLin) {
        const size_t se = (size_t)D.n * D.n + D.n;
        D.facJ = D.facJBase + (size_t)sel * D.facJStride; D.facJ2 = D.facJBase + (size_t)ts * D.facJStride;
        D.Sedge = D.SedgeBase + (size_t)sel * se; D.Sedge2 = D.SedgeBase + (size_t)ts * se;
        D.edges = D.edgesBase + (size_t)sel * D.NE; D.edges2 = D.edgesBase + (size_t)ts * D.NE;
    }
    D.S += (size_t)c * D.sysStride; D.rhs += (size_t)c * D.sysStride; D.Spart += (size_t)c * D.spartStride;
    D.dP += (size_t)c * D.n; D.dL += (size_t)c * D.dLStride; D.partial += (size_t)c * D.partialStride;
    double lam = D.ctl[CTL_LAMBDA];
    for (int i = 0; i < c; i++) lam *= 10.0;       // the sequence the sequential policy would walk
    D.lambda = lam;
    return true;
}

// whitened residual / Jacobians of one projection factor (cheirality: constant 2*fx residual)
__device__ __forceinline__ void ba_eval_fac(const BaDev& D, const DPose& T, const double* p, bool right,
                                            const double* z, double is, double* r, double* Jp, double* Jl) {
    const double d[3] = {p[0] - T.t[0], p[1] - T.t[1], p[2] - T.t[2]};
    double q[3];
    mat3T_vec(T.R, d, q);
    if (Jp) { for (int c = 0; c < 12; c++) Jp[c] = 0; for (int c = 0; c < 6; c++) Jl[c] = 0; }
    if (is == 0.0) { r[0] = r[1] = 0.0; return; }          // factor masked out for the second pass (k_ba_mask)
    if (q[2] <= 0) { r[0] = r[1] = 2.0 * D.fx * is; return; }
    const double x = q[0], y = q[1], zz = q[2], iz = 1.0 / zz;
    const double xx = right ? x - D.b : x;
    r[0] = (D.fx * xx * iz + D.cx - z[0]) * is;
    r[1] = (D.fy * y * iz + D.cy - z[1]) * is;
    if (!Jp) return;
    const double al[2][3] = {{D.fx * iz, 0, -D.fx * xx * iz * iz}, {0, D.fy * iz, -D.fy * y * iz * iz}};
    const double Sk[3][3] = {{0, -zz, y}, {zz, 0, -x}, {-y, x, 0}};
    for (int a = 0; a < 2; a++)
        for (int c = 0; c < 3; c++) {
            Jp[a * 6 + c] = (al[a][0] * Sk[0][c] + al[a][1] * Sk[1][c] + al[a][2] * Sk[2][c]) * is;
            Jp[a * 6 + 3 + c] = -al[a][c] * is;
            Jl[a * 3 + c] = (al[a][0] * T.R[3 * c] + al[a][1] * T.R[3 * c + 1] + al[a][2] * T.R[3 * c + 2]) * is;
        }
}

__device__ __forceinline__ void ba_eval_edge(const BaEdge& e, const DPose& Ta, const DPose& Tb, double* r,
                                             double* Ja, double* Jb) {
    const double w = 1.0 / 0.01;
    DPose Tai, h, Mi, d;
    pose_inverse(Ta, Tai);
    pose_compose(Tai, Tb, h);
    pose_inverse(e.measured, Mi);
    pose_compose(Mi, h, d);
    pose3_logmap(d, r);
    for (int i = 0; i < 6; i++) r[i] *= w;
    if (!Ja) return;
    double Hl[36], Ad[36];
    DPose hi;
    pose3_logmap_derivative(d, Hl);
    pose_inverse(h, hi);
    pose3_adjoint(hi, Ad);
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) {
            double s = 0;
            for (int k = 0; k < 6; k++) s += Hl[i * 6 + k] * Ad[k * 6 + j];
            Ja[i * 6 + j] = -s * w;
            Jb[i * 6 + j] = Hl[i * 6 + j] * w;
        }
}

// Linearisation of one BetweenFactor<Pose3> edge by one wave: lane 0 does the Lie-group algebra, 36 lanes the 6x6
// products and the scatter into the edge accumulator Sacc (n x n | n, upper block triangle).  Static fields come
// from E, the linearisation is stored in `out` (the same element, or its twin of the speculative buffers).
// Returns sum r^2 on lane 0 (0 elsewhere).
__device__ __forceinline__ double ba_edge_linearize(BaEdge& out, const BaEdge& E, const DPose& Ta, const DPose& Tb,
                                                    double* sW, double* Sacc, int n, int tid) {
    double* Hl = sW; double* Ad = Hl + 36; double* Ja = Ad + 36; double* Jb = Ja + 36; double* rr = Jb + 36;
    const double w = 1.0 / 0.01;
    const int fa = E.fa, fb = E.fb;
    const int lane = tid & 63, wave = tid >> 6;
    double v = 0;
    // the three single-lane chains run on three waves at once (every thread of the workgroup calls this function):
    // wave 0 the residual (Logmap), wave 1 LogmapDerivative, wave 2 the adjoint; each rebuilds the cheap pose products
    if (lane == 0 && wave < 3) {
        DPose Tai, h;
        pose_inverse(Ta, Tai);
        pose_compose(Tai, Tb, h);
        if (wave == 2) {
            DPose hi;
            pose_inverse(h, hi);
            pose3_adjoint(hi, Ad);
        } else {
            DPose Mi, d;
            pose_inverse(E.measured, Mi);
            pose_compose(Mi, h, d);
            if (wave == 0) {
                double r[6];
                pose3_logmap(d, r);
                for (int i = 0; i < 6; i++) { r[i] *= w; rr[i] = r[i]; out.r[i] = r[i]; v += r[i] * r[i]; }
            } else pose3_logmap_derivative(d, Hl);
        }
    }
    __syncthreads();
    if (wave != 0) return 0.0;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const int i = lane / 6, j = lane % 6;
    if (lane < 36) {
        double s = 0;
        for (int k = 0; k < 6; k++) s += Hl[i * 6 + k] * Ad[k * 6 + j];
        const double ja = -s * w, jb = Hl[i * 6 + j] * w;
        Ja[lane] = ja; Jb[lane] = jb;
        out.Ja[lane] = ja; out.Jb[lane] = jb;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (lane < 36) {
        double aa = 0, ab = 0, bb = 0;
        for (int k = 0; k < 6; k++) {
            aa += Ja[k * 6 + i] * Ja[k * 6 + j];
            ab += Ja[k * 6 + i] * Jb[k * 6 + j];
            bb += Jb[k * 6 + i] * Jb[k * 6 + j];
        }
        out.Haa[lane] = aa; out.Hab[lane] = ab; out.Hbb[lane] = bb;
        if (fa >= 0) atomicAdd(&Sacc[(size_t)(6 * fa + i) * n + 6 * fa + j], aa);
        if (fb >= 0) atomicAdd(&Sacc[(size_t)(6 * fb + i) * n + 6 * fb + j], bb);
        if (fa >= 0 && fb >= 0) {     // upper triangle only (the solve mirrors it)
            if (fa < fb) atomicAdd(&Sacc[(size_t)(6 * fa + i) * n + 6 * fb + j], ab);
            else atomicAdd(&Sacc[(size_t)(6 * fb + j) * n + 6 * fa + i], ab);
        }
    } else if (lane < 42) {
        const int q = lane - 36;
        double ga = 0, gb = 0;
        for (int k = 0; k < 6; k++) { ga += Ja[k * 6 + q] * rr[k]; gb += Jb[k * 6 + q] * rr[k]; }
        out.ga[q] = ga; out.gb[q] = gb;
        if (fa >= 0) atomicAdd(&Sacc[(size_t)n * n + 6 * fa + q], -ga);
        if (fb >= 0) atomicAdd(&Sacc[(size_t)n * n + 6 * fb + q], -gb);
    }
    return v;
}

// cross-workgroup hand-off of the cost partials without a fence (see k_ba_factors)
__device__ __forceinline__ void ba_publish(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double ba_collect(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// block-wide sum of NV doubles (fixed tree), result valid in out[] for every thread after return
template <int NV, int NW>
__device__ __forceinline__ void ba_block_sum(double (&v)[NV], double* red, double* out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < NV; k++) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v[k] += __shfl_xor(v[k], d);
    }
    if (lane == 0)
        for (int k = 0; k < NV; k++) red[wave * NV + k] = v[k];
    __syncthreads();
    if (tid < NV) {
        double s = 0;
        for (int w = 0; w < NW; w++) s += red[w * NV + tid];
        out[tid] = s;
    }
    __syncthreads();
}

// LevenbergMarquardtOptimizer::iterate / tryLambda bookkeeping (GTSAM 4.2), one thread.
// mode 0: after a linearisation (sums[0] = current error);  mode 1: after a trial (sums[1] = linearised
// cost at delta, sums[2] = cost at the trial values, flags[0] = Cholesky failure).
__device__ __forceinline__ void ba_ctl(const BaDev& D, int mode, double relTol, double absTol) {
    double* c = D.ctl;
    int* ci = (int*)(D.ctl + CTL_INTS);
    if (mode == 0) {
        if (ci[CI_STATE] != BA_LINEARIZE) return;
        if (ci[CI_FIRST]) {
            ci[CI_FIRST] = 0;
            c[CTL_ERROR] = D.sums[0];
            c[CTL_INIT_ERR] = D.sums[0];
            ci[CI_STATE] = (!(c[CTL_ERROR] <= 0.0) && ci[CI_ITER] < ci[CI_MAXIT]) ? BA_TRY : BA_DONE;
        } else ci[CI_STATE] = BA_TRY;
        c[CTL_CUR] = c[CTL_ERROR];          // currentError = newError at the top of the do-body
        return;
    }
    if (ci[CI_STATE] != BA_TRY) return;
    ci[CI_ROUNDS]++;                 // (work figure: trial rounds this pass has evaluated)
    // walk the candidates in the order the sequential policy would have tried them
    const int nAct = ci[CI_NACT];
    for (int cand = 0; cand < nAct; cand++) {
        const double error = c[CTL_ERROR];
        double lambda = c[CTL_LAMBDA];
        bool stepOk = false, stop = false;
        double newErr = INFINITY;
        const double linChange = error - D.sums[SUMS_CAND + 2 * cand];
        if (!D.flags[FLAG_FAIL + cand] && linChange >= 0) {
            newErr = D.sums[SUMS_CAND + 2 * cand + 1];
            const double costChange = error - newErr;
            if (linChange > DBL_EPSILON * error) stepOk = (costChange / linChange) > 1e-3;
            if (fabs(costChange) < relTol * error) stop = true;
        }
        bool endInner = false;
        if (stepOk) {
            ci[CI_SEL] = ba_slot(ci[CI_SEL], cand, D.NB);   // every present landmark / every pose is rewritten per trial
            c[CTL_ERROR] = newErr;
            lambda = lambda / 10.0;
            c[CTL_LAMBDA] = lambda > 0.0 ? lambda : 0.0;
            ci[CI_ITER]++; ci[CI_INNER]++;
            endInner = true;
        } else if (!stop) {
            lambda *= 10.0;
            c[CTL_LAMBDA] = lambda;
            ci[CI_INNER]++;
            if (lambda >= 1e5) endInner = true;
        } else endInner = true;
        if (!endInner) continue;                 // same linearisation, larger lambda: the next candidate
        const double currentError = c[CTL_CUR], newError = c[CTL_ERROR];
        bool converged;
        if (newError <= 0.0) converged = true;
        else {
            const double absDec = currentError - newError, relDec = absDec / currentError;
            converged = (relDec <= relTol) || (absDec <= absTol);
        }
        ci[CI_STATE] = (ci[CI_ITER] < ci[CI_MAXIT] && !converged && isfinite(currentError)) ? BA_LINEARIZE : BA_DONE;
        if (D.specLin && ci[CI_STATE] == BA_LINEARIZE) {   // the trial just accepted was linearised speculatively
            c[CTL_CUR] = c[CTL_ERROR];
            ci[CI_STATE] = BA_TRY;
        }
        ci[CI_NACT] = D.adaptive ? 1 : D.NB;
        return;
    }
    ci[CI_NACT] = D.NB;          // every evaluated candidate was rejected: the chain continues with the full look-ahead
}

// The control step as its own launch: the multi-GPU path, where the cost sums are all-reduced between the
// evaluation and the decision.  After a trial that ends the inner loop the edge accumulator is cleared for the
// next linearisation (the fused kernel below does the same in its last workgroup).
__global__ __launch_bounds__(256) void k_ba_ctl(const BaDev* __restrict__ tab, int mode, double relTol, double absTol) {
    BaDev D = *lane_entry(tab, blockIdx.z);      // per-lane argument block (grid z = problem of the batch)
    __shared__ int sZero;
    if (threadIdx.x == 0) {
        ba_ctl(D, mode, relTol, absTol);
        sZero = mode == 1 && ((const int*)(D.ctl + CTL_INTS))[CI_STATE] == BA_LINEARIZE;
    }
    __syncthreads();
    if (sZero) for (int i = threadIdx.x; i < D.n * D.n + D.n; i += 256) D.Sedge[i] = 0;
}

// One launch per half-step: observation factors (one workgroup per 256-factor slice), BetweenFactor<Pose3>
// edges (one workgroup each, wave 0: the Lie-group algebra of the linearisation wants a large register
// budget; lane 0 does logmap / its derivative / the adjoint, the 6x6 products and the scatter into the reduced
// system are spread over 36 lanes), then the LAST workgroup to finish sums every partial in array order
// (deterministic) and - single GPU - takes the LM decision.
//   MODE 0: linearise at the current values: facJ, edge blocks into Sedge, sums[0] = current error
//   MODE 1: evaluate a trial: sums[1] = linearised cost at delta, sums[2] = cost at the trial values
template <int MODE>
__global__ __launch_bounds__(256) void k_ba_factors(const BaDev* __restrict__ tab, int obsBlocks, int fuseCtl, double relTol, double absTol) {
    BaDev D = *lane_entry(tab, blockIdx.z);      // per-lane argument block (grid z = problem of the batch)
    __shared__ double red[8], out[2];
    __shared__ double sW[160];       // edge scratch: Hl 36 | Ad 36 | Ja 36 | Jb 36 | r 6
    __shared__ int sLast;
    double* const partialBase = D.partial;
    const int cand = MODE == 0 ? 0 : (int)blockIdx.y;      // trial launches: grid y = lambda candidate
    // A workgroup of a candidate beyond nAct has no work but still ARRIVES below: the control step rewrites the block every workgroup
    // of this launch reads at entry (state, nAct, sel), so it may only run once all of them have read it.  (Counting the active
    // candidates' workgroups only, a workgroup of candidate >= 1 that was dispatched late - behind other streams' kernels - could enter
    // after a rejection had raised nAct from 1 to NB, take itself for active and bump the counter of the NEXT round: that round's
    // control step then ran early or, with the counter past its target, never again - "LM did not terminate", seen in long runs.)
    const bool active = ba_enter(D, MODE == 0 ? BA_LINEARIZE : BA_TRY, cand);
    if (!active && ((const int*)(D.ctl + CTL_INTS))[CI_STATE] != (MODE == 0 ? BA_LINEARIZE : BA_TRY)) return;      // (not this lane's turn: no workgroup of it counts)
    const int tid = threadIdx.x;
    if (!active) {
    } else if ((int)blockIdx.x < obsBlocks) {
        double v[2] = {0, 0};
        for (int f = blockIdx.x * 256 + tid; f < D.NF; f += obsBlocks * 256) {
            if (MODE == 0) {
                double r[2], Jp[12], Jl[6];
                ba_eval_fac(D, D.poseCur[D.facKf[f]], D.lmCur + 3 * (size_t)D.facLm[f], D.facRight[f], D.facZ + 2 * (size_t)f,
                            D.facIs[f], r, Jp, Jl);
                double* o = D.facJ + (size_t)f * 20;
                o[0] = r[0]; o[1] = r[1];
                for (int c = 0; c < 12; c++) o[2 + c] = Jp[c];
                for (int c = 0; c < 6; c++) o[14 + c] = Jl[c];
                v[0] += r[0] * r[0] + r[1] * r[1];
            } else {
                const double* o = D.facJ + (size_t)f * 20;
                const int fi = D.facFi[f], lp = D.facLp[f];
                double l0 = o[0], l1 = o[1];
                if (fi >= 0) {
                    const double* dp = D.dP + 6 * fi;
                    for (int i = 0; i < 6; i++) { l0 += o[2 + i] * dp[i]; l1 += o[8 + i] * dp[i]; }
                }
                const double* dl = D.dL + 3 * (size_t)lp;
                for (int i = 0; i < 3; i++) { l0 += o[14 + i] * dl[i]; l1 += o[17 + i] * dl[i]; }
                v[0] += l0 * l0 + l1 * l1;
                double r[2];
                if (D.specLin) {
                    double Jp[12], Jl[6];
                    ba_eval_fac(D, D.poseTrial[D.facKf[f]], D.lmTrial + 3 * (size_t)D.facLm[f], D.facRight[f], D.facZ + 2 * (size_t)f,
                                D.facIs[f], r, Jp, Jl);
                    double* o2 = D.facJ2 + (size_t)f * 20;
                    o2[0] = r[0]; o2[1] = r[1];
                    for (int c = 0; c < 12; c++) o2[2 + c] = Jp[c];
                    for (int c = 0; c < 6; c++) o2[14 + c] = Jl[c];
                } else
                    ba_eval_fac(D, D.poseTrial[D.facKf[f]], D.lmTrial + 3 * (size_t)D.facLm[f], D.facRight[f], D.facZ + 2 * (size_t)f,
                                D.facIs[f], r, nullptr, nullptr);
                v[1] += r[0] * r[0] + r[1] * r[1];
            }
        }
        ba_block_sum<2, 4>(v, red, out);
        if (tid == 0) { ba_publish(&D.partial[2 * blockIdx.x], out[0]); ba_publish(&D.partial[2 * blockIdx.x + 1], out[1]); }
    } else {
        const int e = blockIdx.x - obsBlocks;
        double v[2] = {0, 0};
        if (e < D.NE) {
            const BaEdge& E = D.edges[e];
            const int fa = E.fa, fb = E.fb;
            if (MODE == 0) {
                v[0] = ba_edge_linearize(D.edges[e], E, D.poseCur[E.a], D.poseCur[E.b], sW, D.Sedge, D.n, tid);
            } else {
                if (tid >= 8 && tid < 14) {            // linearised cost at delta, from the current linearisation
                    const int k = tid - 8;
                    double l = E.r[k];
                    for (int i = 0; i < 6; i++) {
                        if (fa >= 0) l += E.Ja[k * 6 + i] * D.dP[6 * fa + i];
                        if (fb >= 0) l += E.Jb[k * 6 + i] * D.dP[6 * fb + i];
                    }
                    v[0] += l * l;
                }
                if (D.specLin) v[1] = ba_edge_linearize(D.edges2[e], E, D.poseTrial[E.a], D.poseTrial[E.b], sW, D.Sedge2, D.n, tid);
                else if (tid == 0) {
                    DPose Tai, h, Mi, d;
                    pose_inverse(D.poseTrial[E.a], Tai);
                    pose_compose(Tai, D.poseTrial[E.b], h);
                    pose_inverse(E.measured, Mi);
                    pose_compose(Mi, h, d);
                    double r[6];
                    pose3_logmap(d, r);
                    for (int i = 0; i < 6; i++) { r[i] *= 1.0 / 0.01; v[1] += r[i] * r[i]; }
                }
            }
#pragma unroll
            for (int k = 0; k < 2; k++) {
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) v[k] += __shfl_xor(v[k], d);
            }
            if (tid == 0) { ba_publish(&D.partial[2 * obsBlocks + 2 * e], v[0]); ba_publish(&D.partial[2 * obsBlocks + 2 * e + 1], v[1]); }
        }
    }
    // The last workgroup to arrive sums every partial in array order.  No __threadfence here: on gfx950 an
    // agent-scope fence is an L2 write-back + invalidate (buffer_wbl2 / buffer_inv sc1) per workgroup, which
    // dominated this kernel.  The partials travel as agent-scope relaxed atomics (sc1 stores / loads that bypass
    // the per-XCD L2), each publisher waits for its stores to complete before it bumps the arrival counter.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const int nCandRun = MODE == 0 ? 1 : D.nAct;        // (candidates with partials: ba_enter read nAct before it turned the others away)
    if (tid == 0) sLast = (__hip_atomic_fetch_add(&D.flags[FLAG_COUNT], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)(gridDim.x * gridDim.y) - 1);
    __syncthreads();
    if (!sLast) return;
    const int nPart = obsBlocks + D.NE;         // (edge partials follow the observation partials)
    for (int c = 0; c < nCandRun; c++) {
        const double* part = partialBase + (size_t)c * D.partialStride;
        double t[2] = {0, 0};
        for (int i = tid; i < nPart; i += 256) { t[0] += ba_collect(&part[2 * i]); t[1] += ba_collect(&part[2 * i + 1]); }
        ba_block_sum<2, 4>(t, red, out);
        if (tid == 0) {
            if (MODE == 0) D.sums[0] = 0.5 * out[0];
            else { D.sums[SUMS_CAND + 2 * c] = 0.5 * out[0]; D.sums[SUMS_CAND + 2 * c + 1] = 0.5 * out[1]; }
        }
        __syncthreads();
    }
    if (tid == 0) {
        D.flags[FLAG_COUNT] = 0;
        sLast = 0;
        if (fuseCtl) {
            ba_ctl(D, MODE, relTol, absTol);
            sLast = MODE == 1 && !D.specLin && ((const int*)(D.ctl + CTL_INTS))[CI_STATE] == BA_LINEARIZE;
            if (D.ctlHost) {
                // The block was just written through int and double views of the same bytes: wait for those stores, then copy it with
                // alias-safe accesses.  (Copied as doubles right behind ba_ctl, a read could overtake the int stores it aliases - the
                // compiler sees no dependence between the types, and nothing else orders the load behind the store or keeps it off a
                // cached line: the mirror then lagged one control step behind, and a lane's final BA_DONE never reached the host.
                // Seen as one run in a dozen ending in "LM did not terminate" / a pass cut short.)
                asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                const unsigned long long* src = (const unsigned long long*)D.ctl;
                unsigned long long* dst = (unsigned long long*)D.ctlHost;
                for (int i = 0; i < CTL_DOUBLES; i++) dst[i] = __hip_atomic_load(&src[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (from the L2, not a cached line)
                // ... and the copy must have LANDED in host memory before this kernel ends: the next round's control step writes the same
                // 128 bytes from another CU, and nothing orders two CUs' writes to system memory against each other - an older block
                // arriving last would hide the lane's BA_DONE from the host for good (seen: one run in ten ended in "LM did not terminate")
                __threadfence_system();
            }
        }
    }
    __syncthreads();
    if (sLast) for (int i = tid; i < D.n * D.n + D.n; i += 256) D.Sedge[i] = 0;     // cleared for the next linearisation
}

// ---- landmark blocks shared by the Schur and back-substitution kernels ---------------------------
// W / sfi are private to the calling wave: LDS traffic of one wave is processed in order, so a compiler-level
// fence (no workgroup barrier) is all that separates the writes below from the reads that follow.
__device__ __forceinline__ void ba_wave_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// After the call (and a ba_wave_fence) W[s*18 + i*3 + j] holds Hpl of slot s; h = 6 unique entries of Hll (undamped)
// followed by bl, identical in every lane of the wave.
// BA_LPL lanes serve one landmark (a landmark has ~13 factors and <= 10 slots, a 64-lane wave per landmark leaves
// lanes idle; a wave can carry 64 / BA_LPL landmarks side by side; `act` = this lane group has a landmark);
// measured: the back-substitution is faster with two landmarks per wave, the Schur accumulation (longer per-landmark
// chains of LDS atomics) with one.
template <int BA_LPL>
__device__ __forceinline__ void ba_lm_blocks(const BaDev& D, int lp, bool act, double* W, int* sfi, double* h, int& ns) {
    const int lane = threadIdx.x & (BA_LPL - 1);
    const int f0 = act ? D.lpStart[lp] : 0, f1 = act ? D.lpStart[lp + 1] : 0;
#pragma unroll
    for (int k = 0; k < 9; k++) h[k] = 0;
    for (int f = f0 + lane; f < f1; f += BA_LPL) {
        const double* o = D.facJ + (size_t)f * 20;
        const double r0 = o[0], r1 = o[1];
        const double* Jl = o + 14;
        h[0] += Jl[0] * Jl[0] + Jl[3] * Jl[3];
        h[1] += Jl[0] * Jl[1] + Jl[3] * Jl[4];
        h[2] += Jl[0] * Jl[2] + Jl[3] * Jl[5];
        h[3] += Jl[1] * Jl[1] + Jl[4] * Jl[4];
        h[4] += Jl[1] * Jl[2] + Jl[4] * Jl[5];
        h[5] += Jl[2] * Jl[2] + Jl[5] * Jl[5];
        h[6] -= Jl[0] * r0 + Jl[3] * r1;
        h[7] -= Jl[1] * r0 + Jl[4] * r1;
        h[8] -= Jl[2] * r0 + Jl[5] * r1;
    }
#pragma unroll
    for (int k = 0; k < 9; k++) {
#pragma unroll
        for (int d = BA_LPL / 2; d >= 1; d >>= 1) h[k] += __shfl_xor(h[k], d);
    }
    const int s0 = act ? D.lpSlotStart[lp] : 0;
    ns = act ? D.lpSlotStart[lp + 1] - s0 - 1 : 0;   // one end sentinel per landmark
    for (int e = lane; e < ns * 18; e += BA_LPL) {
        const int s = e / 18, ij = e - s * 18, i = ij / 3, j = ij - i * 3;
        double acc = 0;
        for (int f = D.slotStart[s0 + s]; f < D.slotStart[s0 + s + 1]; f++) {
            const double* o = D.facJ + (size_t)f * 20;
            acc += o[2 + i] * o[14 + j] + o[2 + 6 + i] * o[14 + 3 + j];
        }
        W[e] = acc;
    }
    for (int s = lane; s < ns; s += BA_LPL) sfi[s] = D.slotFi[s0 + s];
}
// (Hll + lambda I)^-1
__device__ __forceinline__ void ba_hll_inverse(const double* h, double lambda, double* Hi) {
    const double Hll[9] = {h[0] + lambda, h[1], h[2], h[1], h[3] + lambda, h[4], h[2], h[4], h[5] + lambda};
    inv3sym(Hll, Hi);
}

// One wave per landmark.  sharedW: the workgroup serves every lambda candidate (grid y = 1): Hll, bl and the W blocks
// do not depend on the damping and are built once, only Hll^-1 and the rank-3 updates are per candidate, each into
// its own LDS copy of the reduced system.  Otherwise grid y = candidate.
__global__ __launch_bounds__(64 * BA_SCHUR_WAVES) void k_ba_schur(const BaDev* __restrict__ tab, int maxSlots, int sharedW) {
    BaDev D = *lane_entry(tab, blockIdx.z);      // per-lane argument block (grid z = problem of the batch)
    constexpr bool LDS_S = true;       // (windows of larger systems: k_ba_schur_win)
    extern __shared__ double sm[];
    double* const SBase = D.S;
    double* const SpartBase = D.Spart;
    (void)SBase;
    const int c0 = sharedW ? 0 : (int)blockIdx.y;
    if (!ba_enter(D, BA_TRY, c0)) return;
    const int nc = sharedW ? D.nAct : 1;
    const int n = D.n;
    const size_t sys = (size_t)n * n + n;
    constexpr int BA_LPL = BA_LPL_SCHUR;
    double* Sloc = sm;                                        // LDS_S: nc copies of n*n + n
    double* wbase = sm + (LDS_S ? (size_t)nc * sys : 0);
    static_assert(BA_LPL == 64, "one wave per landmark: the landmark index is wave-uniform");
    const int lane = threadIdx.x & (BA_LPL - 1);
    const int unit = __builtin_amdgcn_readfirstlane(threadIdx.x / BA_LPL);    // unit = landmark lane group (= wave) of the workgroup
    double* W = wbase + (size_t)unit * (2 * maxSlots * 18);
    double* WH = W + maxSlots * 18;
    const int nu = blockDim.x / BA_LPL, nt = blockDim.x;
    int* sfi = (int*)(wbase + (size_t)nu * (2 * maxSlots * 18)) + unit * maxSlots;
    if (LDS_S) {
        for (int i = threadIdx.x; i < (int)(nc * sys); i += nt) Sloc[i] = 0;
    }
    __syncthreads();
    // per-lane roles of the accumulation loops (fixed for the kernel)
    const int bi = lane / 6, bj = lane - bi * 6;
    const bool isBlk = lane < 36, isRhs = lane >= 36 && lane < 42;
    const int rr = isRhs ? lane - 36 : 0;
    const int hHalf = lane >= 27 ? 1 : 0, hq = lane - 27 * hHalf;
    const bool hRhs = hq >= 21;
    int hI = 0, hJ = 0;
    if (hRhs) hI = hq - 21;
    else { int rem = hq; while (rem >= 6 - hI) { rem -= 6 - hI; hI++; } hJ = hI + rem; }
    const int rounds = (D.Lp + gridDim.x * nu - 1) / (gridDim.x * nu);
    for (int rd = 0; rd < rounds; rd++) {
        const int lp = (rd * gridDim.x + blockIdx.x) * nu + unit;
        const bool act = lp < D.Lp;
        double h[9];
        int ns = 0;
        ba_lm_blocks<BA_LPL>(D, lp, act, W, sfi, h, ns);
        ba_wave_fence();
        double lamk = D.lambda;             // candidate c0 + k: lambda * 10^k, the sequence of the sequential policy
        for (int k = 0; k < nc; k++, lamk *= 10.0) {
            double* Sacc = LDS_S ? Sloc + (size_t)k * sys : SBase + (size_t)(c0 + k) * D.sysStride;
            double* racc = Sacc + (size_t)n * n;
            double Hi[9];
            ba_hll_inverse(h, lamk, Hi);
            for (int e = lane; e < ns * 18; e += BA_LPL) {
                const int s = e / 18, ij = e - s * 18, i = ij / 3, j = ij - i * 3;
                const double* w = W + s * 18 + i * 3;
                WH[e] = w[0] * Hi[j] + w[1] * Hi[3 + j] + w[2] * Hi[6 + j];
            }
            ba_wave_fence();
            // S -= W_s1 Hll^-1 W_s2^T for s1 <= s2 (upper block triangle), rhs -= W_s1 Hll^-1 bl.
            // Lane (bi, bj) < 36 owns one entry of every 6x6 block, lanes 36..41 the right-hand-side rows; the slot pair (s1, s2) is
            // wave-uniform, so a block costs three LDS reads of the W row, five fp64 operations and one LDS atomic - no per-entry
            // division / modulo chains (the PMC pass showed the first form VALU-bound on exactly that index arithmetic: ~2 700 VALU
            // instructions per landmark for ~100 wave-instructions of arithmetic).
            const int nsu = __builtin_amdgcn_readfirstlane(ns);
            for (int s1 = 0; s1 < nsu; s1++) {
                const int k1 = __builtin_amdgcn_readfirstlane(sfi[s1]);
                const double* a = WH + s1 * 18 + (isBlk ? bi : rr) * 3;
                const double a0 = a[0], a1 = a[1], a2 = a[2];
                if (isBlk) {
                    double* drow = Sacc + (size_t)(6 * k1 + bi) * n + bj;
                    for (int s2 = s1; s2 < nsu; s2++) {
                        const int k2 = __builtin_amdgcn_readfirstlane(sfi[s2]);
                        const double* bb = W + s2 * 18 + bj * 3;
                        atomicAdd(drow + 6 * k2, -(a0 * bb[0] + a1 * bb[1] + a2 * bb[2]));
                    }
                } else if (isRhs) atomicAdd(&racc[6 * k1 + rr], -(a0 * h[6] + a1 * h[7] + a2 * h[8]));
            }
            ba_wave_fence();        // WH is rewritten for the next candidate
        }
        // Hpp and bp from this landmark's observations of free keyframes (the same for every candidate): lanes 0..26 / 27..53
        // take the 21 + 6 entries of the even / odd factors of the landmark
        const int f0 = act ? D.lpStart[lp] : 0, f1 = act ? D.lpStart[lp + 1] : 0;
        if (lane < 54) {
            for (int f = f0 + hHalf; f < f1; f += 2) {
                const int fi = D.facFi[f];
                if (fi < 0) continue;
                const double* o = D.facJ + (size_t)f * 20;
                const double val = hRhs ? -(o[2 + hI] * o[0] + o[8 + hI] * o[1]) : o[2 + hI] * o[2 + hJ] + o[8 + hI] * o[8 + hJ];
                const size_t idx = hRhs ? (size_t)n * n + 6 * fi + hI : (size_t)(6 * fi + hI) * n + 6 * fi + hJ;
                for (int k = 0; k < nc; k++) atomicAdd((LDS_S ? Sloc + (size_t)k * sys : SBase + (size_t)(c0 + k) * D.sysStride) + idx, val);
            }
        }
    }
    if (LDS_S) {
        __syncthreads();
        for (int k = 0; k < nc; k++) {
            double* dst = SpartBase + (size_t)(c0 + k) * D.spartStride + (size_t)blockIdx.x * sys;
            for (int i = threadIdx.x; i < (int)sys; i += nt) dst[i] = Sloc[(size_t)k * sys + i];
        }
    }
}

// ---- k_ba_schur2: the accumulation for tracker windows (<= BA2_MAX_F free keyframes), written against the instruction counters -------
// k_ba_schur above spends ~2 700 VALU wave-instructions per landmark for ~100 of arithmetic (PMC pass): a wave per landmark
// that walks its factors through dependent global loads, reduces nine values with 108 ds_bpermute, and spreads 36-entry blocks over
// lanes with division / modulo chains.  This form keeps the wave per landmark but gives every LANE a whole unit of work:
//   stage   the landmark's factor rows are contiguous in facJ (the host sorts by landmark, then free index): one coalesced copy into a
//           wave-private LDS region, with the free indices and the slot table - ONE global round trip per landmark;
//   h       Hll (6) | bl (3): lane 4k + q sums the factors f = q (mod 4) of value k from LDS, two DPP quad steps finish it;
//   W, WH   lane (s, i) < 6 ns builds row i of the slot's Hpl block and of Hpl (Hll + lambda I)^-1, and adds its right-hand-side entry;
//   blocks  two lanes own ONE 6x6 block (s1 <= s2), three rows each: the rows of WH_s1 / W_s2 in registers, 54 multiply-adds, 18 LDS
//           atomics at constant offsets from one base address - no per-entry index arithmetic;
//   Hpp     lane (f, i) owns row i of the factor's Jp^T Jp (upper part) and its gradient entry.
// One LDS copy of the reduced system per workgroup; the look-ahead candidates are separate workgroups (grid y; candidates beyond the
// round's nAct leave at once).
__device__ __forceinline__ double ba2_dpp_xor(double v, int which) {      // lane ^ 1 (which = 0) / lane ^ 2 (which = 1) inside a quad
    const int lo = __double2loint(v), hi = __double2hiint(v);
    int l2, h2;
    if (which == 0) { l2 = __builtin_amdgcn_update_dpp(0, lo, 0xB1, 0xF, 0xF, true); h2 = __builtin_amdgcn_update_dpp(0, hi, 0xB1, 0xF, 0xF, true); }
    else { l2 = __builtin_amdgcn_update_dpp(0, lo, 0x4E, 0xF, 0xF, true); h2 = __builtin_amdgcn_update_dpp(0, hi, 0x4E, 0xF, 0xF, true); }
    return __hiloint2double(h2, l2);
}
// per-lane roles of the staged forms (fixed for a kernel) and the shared front part: stage -> Hll | bl -> (Hll + lambda I)^-1 -> W rows
struct Ba2Roles {
    int hk, hq, hx, hy, hyStep; bool hOn; double hSign;      // h: lane 4k + q, k < 9
    int ws, wi;                                               // W / WH: lane (s, i)
    __device__ __forceinline__ void init(int lane) {
        hk = lane >> 2; hq = lane & 3; hOn = hk < 9;
        // k < 6: (a, b) in (0,0) (0,1) (0,2) (1,1) (1,2) (2,2): Jl[a] Jl[b] + Jl[3 + a] Jl[3 + b];  k >= 6: -(Jl[a] r0 + Jl[3 + a] r1), a = k - 6
        const int ha = hk < 3 ? 0 : (hk < 5 ? 1 : (hk == 5 ? 2 : hk - 6));
        const int hbx = hk < 3 ? hk : (hk < 5 ? hk - 2 : 2);
        hx = 14 + ha;
        hy = hk < 6 ? 14 + hbx : 0;
        hyStep = hk < 6 ? 3 : 1;     // second operand of the second product: Jl[3 + b] or r1
        hSign = hk < 6 ? 1.0 : -1.0;
        ws = lane / 6; wi = lane - ws * 6;
    }
};
struct Ba2Region { double* F; double* W; double* WH; double* hb; int* ffi; int* sst; int* sfi; };
__device__ __forceinline__ Ba2Region ba2_region(double* base, int maxFac, int maxSlots) {
    Ba2Region g;
    g.F = base; g.W = g.F + maxFac * 20; g.WH = g.W + maxSlots * 18; g.hb = g.WH + maxSlots * 18;
    g.ffi = (int*)(g.hb + 10); g.sst = g.ffi + maxFac; g.sfi = g.sst + maxSlots + 1;
    return g;
}
// the landmark's factor rows, free indices and slot table into the wave's region; then h = Hll (6 unique, undamped) | bl in every lane
__device__ __forceinline__ void ba2_stage_h(const BaDev& D, int lp, const Ba2Region& g, const Ba2Roles& R, int lane, double* h, int& nf, int& ns) {
    const int f0 = D.lpStart[lp], s0 = D.lpSlotStart[lp];
    nf = D.lpStart[lp + 1] - f0;
    ns = D.lpSlotStart[lp + 1] - s0 - 1;     // one end sentinel per landmark
    // (prefetching the next landmark's rows into registers under this one's arithmetic was measured: no gain)
    {
        const double2* src = (const double2*)(D.facJ + (size_t)f0 * 20);
        double2* dst = (double2*)g.F;
        for (int i = lane; i < nf * 10; i += 64) dst[i] = src[i];
        for (int i = lane; i < nf; i += 64) g.ffi[i] = D.facFi[f0 + i];
        for (int i = lane; i <= ns; i += 64) { g.sst[i] = D.slotStart[s0 + i] - f0; g.sfi[i] = D.slotFi[s0 + i]; }
    }
    ba_wave_fence();
    {
        double acc = 0;
        if (R.hOn)
            for (int f = R.hq; f < nf; f += 4) {
                const double* o = g.F + f * 20;
                acc += o[R.hx] * o[R.hy] + o[R.hx + 3] * o[R.hy + R.hyStep];
            }
        acc += ba2_dpp_xor(acc, 0);
        acc += ba2_dpp_xor(acc, 1);
        if (R.hOn && R.hq == 0) g.hb[R.hk] = R.hSign * acc;
    }
    ba_wave_fence();
#pragma unroll
    for (int k = 0; k < 9; k++) h[k] = g.hb[k];
}
// row i of slot s's Hpl block from the staged rows (lane (s, i), s < ns)
__device__ __forceinline__ void ba2_w_row(const Ba2Region& g, const Ba2Roles& R, double& w0, double& w1, double& w2) {
    w0 = w1 = w2 = 0;
    for (int f = g.sst[R.ws]; f < g.sst[R.ws + 1]; f++) {
        const double* o = g.F + f * 20;
        const double a0 = o[2 + R.wi], a1 = o[8 + R.wi];
        w0 += a0 * o[14] + a1 * o[17];
        w1 += a0 * o[15] + a1 * o[18];
        w2 += a0 * o[16] + a1 * o[19];
    }
}

// the block phase: two lanes own one 6x6 block (s1 <= s2), three rows each; 32 blocks per pass.  One base address per lane, the 18
// atomics at constant offsets from it (PACKED: row pitch 6 - all of them immediates; else the rows are ld apart).
template <bool PACKED>
__device__ __forceinline__ void ba2_blocks(double* Sloc, const double* W, const double* WH, const int* sfi, int ns, int lane, int F, int ld) {
    const int nb = ns * (ns + 1) / 2, half = lane & 1;
    for (int b0 = 0; b0 < nb; b0 += 32) {
        int b = b0 + (lane >> 1), s1 = 0;
        if (b >= nb) continue;
        while (b >= ns - s1) { b -= ns - s1; s1++; }
        const int s2 = s1 + b;
        const double* A = WH + s1 * 18 + half * 9;
        const double* B = W + s2 * 18;
        double aa[9];
#pragma unroll
        for (int q = 0; q < 9; q++) aa[q] = A[q];
        double* d0 = Sloc + (PACKED ? ba_packed_block(F, sfi[s1], sfi[s2]) * BA_PACKED_PITCH + 18 * half : (6 * sfi[s1] + 3 * half) * ld + 6 * sfi[s2]);
        // (the lane's three A rows stay in registers; B goes through them three columns at a time)
#pragma unroll
        for (int jh = 0; jh < 2; jh++) {
            double bb[9];
#pragma unroll
            for (int q = 0; q < 9; q++) bb[q] = B[9 * jh + q];
#pragma unroll
            for (int i = 0; i < 3; i++) {
                double* dr = d0 + i * (PACKED ? 6 : ld) + 3 * jh;
#pragma unroll
                for (int j = 0; j < 3; j++) atomicAdd(dr + j, -(aa[3 * i] * bb[3 * j] + aa[3 * i + 1] * bb[3 * j + 1] + aa[3 * i + 2] * bb[3 * j + 2]));
            }
        }
    }
}

template <bool PACKED>
__device__ __forceinline__ void ba2_schur(const BaDev* __restrict__ tab, int maxSlots, int maxFac, int layout) {
    BaDev D = *lane_entry(tab, blockIdx.z);      // per-lane argument block (grid z = problem of the cohort)
    extern __shared__ double sm[];
    if (!ba_enter(D, BA_TRY, blockIdx.y)) return;
    const int n = D.n, F = n / 6;                // the lane's own system, not the cohort's largest
    constexpr bool packed = PACKED;
    const int ld = layout == BA2_ROWMAJOR1 ? n + 1 : n;
    const int sys = ba2_sys_doubles(n, layout);
    double* const Sloc = sm;
    double* const racc = Sloc + (packed ? ba_packed_rhs(F) : ld * n);
    const int lane = threadIdx.x & 63;
    const int unit = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nu = blockDim.x >> 6, nt = blockDim.x;
    const Ba2Region g = ba2_region(sm + sys + (size_t)unit * ba2_stage_doubles(maxFac, maxSlots), maxFac, maxSlots);
    double* const F_ = g.F; double* const W = g.W; double* const WH = g.WH;
    int* const ffi = g.ffi; int* const sfi = g.sfi;
    const double lam = D.lambda;
    Ba2Roles R;
    R.init(lane);
    const int pf = lane / 6, pi = lane - pf * 6;           // Hpp: lane (f, i), ten factors per pass
    for (int i = threadIdx.x; i < sys; i += nt) Sloc[i] = 0;
    __syncthreads();
    for (int lp = blockIdx.x * nu + unit; lp < D.Lp; lp += gridDim.x * nu) {
        double h[9];
        int nf, ns;
        ba2_stage_h(D, lp, g, R, lane, h, nf, ns);
        double Hi[9];
        ba_hll_inverse(h, lam, Hi);
        // ---- W, WH, rhs: lane (s, i) ----
        if (R.ws < ns) {
            double w0, w1, w2;
            ba2_w_row(g, R, w0, w1, w2);
            const double g0 = w0 * Hi[0] + w1 * Hi[3] + w2 * Hi[6], g1 = w0 * Hi[1] + w1 * Hi[4] + w2 * Hi[7], g2 = w0 * Hi[2] + w1 * Hi[5] + w2 * Hi[8];
            double* wr = W + R.ws * 18 + R.wi * 3;
            wr[0] = w0; wr[1] = w1; wr[2] = w2;
            double* gr = WH + R.ws * 18 + R.wi * 3;
            gr[0] = g0; gr[1] = g1; gr[2] = g2;
            atomicAdd(&racc[6 * sfi[R.ws] + R.wi], -(g0 * h[6] + g1 * h[7] + g2 * h[8]));
        }
        ba_wave_fence();
        // ---- blocks ----
        ba2_blocks<PACKED>(Sloc, W, WH, sfi, ns, lane, F, ld);
        // ---- Hpp and bp of the factors of free keyframes: lane (f, i), ten factors per pass ----
        if (pf < 10)
            for (int fb = 0; fb < nf; fb += 10) {
                const int f = fb + pf;
                if (f >= nf) break;
                const int fi = ffi[f];
                if (fi < 0) continue;
                const double* o = F_ + f * 20;
                const double a0 = o[2 + pi], a1 = o[8 + pi];
                double* dr = Sloc + (packed ? ba_packed_block(F, fi, fi) * BA_PACKED_PITCH + 6 * pi : (6 * fi + pi) * ld + 6 * fi);
                for (int j = pi; j < 6; j++) atomicAdd(dr + j, a0 * o[2 + j] + a1 * o[8 + j]);
                atomicAdd(&racc[6 * fi + pi], -(a0 * o[0] + a1 * o[1]));
            }
        ba_wave_fence();        // the region is rewritten for the next landmark
    }
    __syncthreads();
    const int part = ba2_part_doubles(n, layout);
    double* dst = D.Spart + (size_t)blockIdx.x * part;
    if (layout == BA2_ROWMAJOR1) {
        for (int i = threadIdx.x; i < part; i += nt) dst[i] = Sloc[i + i / n];      // pitch n + 1 -> n (the rhs is row n)
    } else {
        for (int i = threadIdx.x; i < part; i += nt) dst[i] = Sloc[i];
    }
}
__global__ __launch_bounds__(1024) void k_ba_schur2(const BaDev* __restrict__ tab, int maxSlots, int maxFac) { ba2_schur<true>(tab, maxSlots, maxFac, BA2_PACKED); }
// the row-major forms behind the developer switch (layout = BA2_ROWMAJOR / BA2_ROWMAJOR1)
__global__ __launch_bounds__(1024) void k_ba_schur2_rm(const BaDev* __restrict__ tab, int maxSlots, int maxFac, int layout) { ba2_schur<false>(tab, maxSlots, maxFac, layout); }

// Back-substitution on the same staged front part: dl = (Hll + lambda I)^-1 (bl - sum_s W_s^T dP_s) per candidate, trial landmark positions.
// Lane (s, i) multiplies its W row by its entry of the slot's pose update; the three sums over the <= 60 lanes finish with two DPP quad
// steps + four shuffles.  No reduced-system copy in LDS: two workgroups of eight waves per CU.
__global__ __launch_bounds__(512) void k_ba_back2(const BaDev* __restrict__ tab, int maxSlots, int maxFac) {
    BaDev D = *lane_entry(tab, blockIdx.z);      // per-lane argument block (grid z = problem of the cohort)
    extern __shared__ double sm[];
    if (!ba_enter(D, BA_TRY, 0)) return;
    const int nc = D.nAct;
    const int sel = ((const int*)(D.ctl + CTL_INTS))[CI_SEL];
    const int lane = threadIdx.x & 63;
    const int unit = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nu = blockDim.x >> 6;
    const Ba2Region g = ba2_region(sm + (size_t)unit * ba2_stage_doubles(maxFac, maxSlots), maxFac, maxSlots);
    Ba2Roles R;
    R.init(lane);
    for (int lp = blockIdx.x * nu + unit; lp < D.Lp; lp += gridDim.x * nu) {
        double h[9];
        int nf, ns;
        ba2_stage_h(D, lp, g, R, lane, h, nf, ns);
        double w0 = 0, w1 = 0, w2 = 0;
        int kcol = 0;
        if (R.ws < ns) { ba2_w_row(g, R, w0, w1, w2); kcol = 6 * g.sfi[R.ws] + R.wi; }
        const int l = D.lpOrig[lp];
        double lamk = D.lambda;
        for (int k = 0; k < nc; k++, lamk *= 10.0) {
            const double* dPk = D.dP + (size_t)k * D.n;         // (ba_enter already applied candidate 0)
            const double dp = R.ws < ns ? dPk[kcol] : 0.0;
            double t0 = w0 * dp, t1 = w1 * dp, t2 = w2 * dp;
            t0 += ba2_dpp_xor(t0, 0); t1 += ba2_dpp_xor(t1, 0); t2 += ba2_dpp_xor(t2, 0);
            t0 += ba2_dpp_xor(t0, 1); t1 += ba2_dpp_xor(t1, 1); t2 += ba2_dpp_xor(t2, 1);
#pragma unroll
            for (int d = 4; d <= 32; d <<= 1) { t0 += __shfl_xor(t0, d); t1 += __shfl_xor(t1, d); t2 += __shfl_xor(t2, d); }
            double Hi[9];
            ba_hll_inverse(h, lamk, Hi);
            if (lane < 3) {
                const double u0 = h[6] - t0, u1 = h[7] - t1, u2 = h[8] - t2;
                // (row `lane` of Hi picked by selects: indexing the register array by the lane would put it in scratch)
                const double h0 = lane == 0 ? Hi[0] : (lane == 1 ? Hi[3] : Hi[6]);
                const double h1 = lane == 0 ? Hi[1] : (lane == 1 ? Hi[4] : Hi[7]);
                const double h2 = lane == 0 ? Hi[2] : (lane == 1 ? Hi[5] : Hi[8]);
                const double dl = h0 * u0 + h1 * u1 + h2 * u2;
                D.dL[(size_t)k * D.dLStride + 3 * (size_t)lp + lane] = dl;
                double* lmT = D.lmBase + (size_t)ba_slot(sel, k, D.NB) * D.lmStride;
                lmT[3 * (size_t)l + lane] = D.lmCur[3 * (size_t)l + lane] + dl;
            }
        }
        ba_wave_fence();            // the region is rewritten for the next landmark
    }
}

// Sum of the per-workgroup partial systems.  This is the buffer the landmark-sharded multi-GPU path all-reduces (RCCL)
// before the solve.  A workgroup owns 32 entries; 8 thread groups sum slices of the partials, the 8 slice sums are
// then added in slice order through LDS - a fixed summation order, no atomics: the reduced system is bit-identical
// from run to run.
__global__ __launch_bounds__(256) void k_ba_reduce(const BaDev* __restrict__ tab, int nPart, int packed) {
    BaDev D = *lane_entry(tab, blockIdx.z);      // per-lane argument block (grid z = problem of the batch)
    __shared__ double sSl[8][33];
    if (!ba_enter(D, BA_TRY, blockIdx.y)) return;
    const int total = D.n * D.n + D.n, F = D.n / 6;
    // packed partials (k_ba_schur2, ba_packed.hpp): the workgroup's 32 slots are 32 consecutive packed offsets, read as they lie; the
    // slots behind the packed size own the entries below the block diagonal - in no partial, they get the edge term alone (what the
    // sum of their zeros gave)
    const int nSum = packed ? ba_packed_doubles(F) : total;            // slots with partials = doubles of one partial
    const int nSlots = packed ? ba_packed_reduce_slots(F) : total;
    const int e = threadIdx.x & 31, y = threadIdx.x >> 5;
    const int i = blockIdx.x * 32 + e;
    double s = 0;
    if (i < nSum) {
        const int per = (nPart + 7) / 8;
        const int p0 = y * per, p1 = min(nPart, p0 + per);
        double s0 = 0, s1 = 0, s2 = 0, s3 = 0;      // 4 independent accumulators keep the strided loads in flight
        // (int offsets: the partials of a candidate, at most a few hundred of <= 3 660 doubles, stay far below 2^31)
        int p = p0;
        for (; p + 3 < p1; p += 4) {
            s0 += D.Spart[p * nSum + i];
            s1 += D.Spart[(p + 1) * nSum + i];
            s2 += D.Spart[(p + 2) * nSum + i];
            s3 += D.Spart[(p + 3) * nSum + i];
        }
        for (; p < p1; p++) s0 += D.Spart[p * nSum + i];
        s = (s0 + s1) + (s2 + s3);
    }
    sSl[y][e] = s;
    __syncthreads();
    const int slot = blockIdx.x * 32 + threadIdx.x;      // = i in slice 0
    if (y == 0 && slot < nSlots) {
        const int io = packed ? ba_packed_reduce_entry(F, slot) : slot;      // the slot's row-major entry
        if (io >= 0) {
            double t = D.Sedge[io];          // BetweenFactor blocks of this linearisation
            for (int q = 0; q < 8; q++) t += sSl[q][threadIdx.x];
            if (D.specLin) D.Sedge2[io] = 0; // the trial's speculative linearisation accumulates here
            if (io < D.n * D.n) D.S[io] = t; else D.rhs[io - D.n * D.n] = t;
        }
    }
}

// ---- windowed Schur accumulation (more free keyframes than one LDS copy of the reduced system holds) ---------------
// The reduced camera system is tiled into WINDOWS of TB x TB keyframe blocks (upper block triangle, a <= b); a
// workgroup owns one window and a slice of the landmarks that touch it (host-built work lists: a landmark observed
// by free keyframes of block rows {a, b, ...} is listed under every window (a, b) of that set).  The window - one copy
// per lambda candidate - lives in LDS; a landmark adds the 6x6 blocks of its (slot, slot) pairs that fall inside
// it.  Partial windows are written out once and summed in a fixed order by k_ba_reduce_win.  No fp64 global atomics.
// Landmark blocks of the current linearisation, once per trial round: a landmark that is seen from several block rows
// sits in several windows' lists, which then only fetch the W blocks of their own rows / columns (144 B each) instead of
// rebuilding everything from the landmark's factors.
__global__ __launch_bounds__(64 * BA_SCHUR_WAVES) void k_ba_lm_prep(const BaDev* __restrict__ tab, BaWin Wn, int maxSlots) {
    BaDev D = *lane_entry(tab, blockIdx.z);      // per-lane argument block (grid z = problem of the batch)
    extern __shared__ int smi[];
    if (!ba_enter(D, BA_TRY, 0)) return;
    constexpr int BA_LPL = 64;
    const int lane = threadIdx.x & 63, unit = threadIdx.x >> 6, nu = blockDim.x >> 6;
    int* sfi = smi + unit * maxSlots;
    for (int lp = blockIdx.x * nu + unit; lp < D.Lp; lp += gridDim.x * nu) {
        double h[9];
        int ns = 0;
        ba_lm_blocks<BA_LPL>(D, lp, true, Wn.Wg + (size_t)D.lpSlotStart[lp] * 18, sfi, h, ns);
        double* Hl = Wn.Hg + (size_t)lp * BA_WIN_HG;
        if (lane < 9) {
            double v = h[0];
#pragma unroll
            for (int k = 1; k < 9; k++) if (lane == k) v = h[k];
            Hl[lane] = v;
        } else if (lane >= 16 && lane < 16 + D.nAct) {        // (Hll + lambda_k I)^-1 of every candidate: 6 unique entries
            double lamk = D.lambda;
            for (int k = 16; k < lane; k++) lamk *= 10.0;
            double Hi[9];
            ba_hll_inverse(h, lamk, Hi);
            double* o = Hl + 9 + 6 * (lane - 16);
            o[0] = Hi[0]; o[1] = Hi[1]; o[2] = Hi[2]; o[3] = Hi[4]; o[4] = Hi[5]; o[5] = Hi[8];
        }
    }
}

// Work decomposition: PAIR-parallel.  A wave takes 64 list entries at a time; every lane resolves one entry's slot
// ranges (64 independent chains of dependent loads in flight), a wave-wide prefix sum of the pair counts flattens
// (entry, pair) into one index space, and 6 lanes serve one pair (lane = row i of the 6x6 block: the W row of its own
// slot, the 18 W entries of the partner slot and Hll | bl come straight from HBM / L2, 6 LDS atomics per candidate).
// No staging, no per-landmark barriers or fences: the atomics are fire-and-forget until the final flush.
__global__ __launch_bounds__(64 * BA_SCHUR_WAVES) void k_ba_schur_win(const BaDev* __restrict__ tab, BaWin Wn) {
    BaDev D = *lane_entry(tab, blockIdx.z);      // per-lane argument block (grid z = problem of the batch)
    extern __shared__ double sm[];
    if (!ba_enter(D, BA_TRY, 0)) return;
    const int nc = D.nAct, T = Wn.T, TP = Wn.TP, tile = Wn.tileDoubles;
    const int win = Wn.wgWin[blockIdx.x], wa = Wn.winA[win], wb = Wn.winB[win];
    const int r0 = wa * Wn.TB, r1 = min(D.F, r0 + Wn.TB), c0 = wb * Wn.TB, c1 = min(D.F, c0 + Wn.TB);
    const bool diag = wa == wb;
    double* Sloc = sm;                                        // nc copies of the window
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6, nt = blockDim.x;
    int* meta = (int*)(sm + (size_t)nc * tile) + wave * BA_WIN_META;
    int* mLp = meta; int* mSeR = meta + 64; int* mNR = meta + 128; int* mSeC = meta + 192; int* mNC = meta + 256; int* pref = meta + 320;
    for (int i = threadIdx.x; i < nc * tile; i += nt) Sloc[i] = 0;
    __syncthreads();
    const int i0 = Wn.wgBegin[blockIdx.x], i1 = Wn.wgEnd[blockIdx.x];
    const int g = lane / 6, ri = lane - 6 * g;              // pair group of the lane (10 per pass), row of the 6x6 block
    for (int base = i0 + wave * 64; base < i1; base += nw * 64) {
        // ---- phase 1: lane = list entry ----------------------------------------------------------------
        {
            const int idx = base + lane;
            const bool valid = idx < i1;
            const int lp = valid ? Wn.winLm[idx] : 0;
            const int se0 = valid ? D.lpSlotStart[lp] : 0;
            const int ns = valid ? D.lpSlotStart[lp + 1] - se0 - 1 : 0;
            int sr0 = ns, sr1 = 0, sc0 = ns, sc1 = 0;
            for (int q = 0; q < ns; q++) {
                const int fi = D.slotFi[se0 + q];
                if (fi >= r0 && fi < r1) { sr0 = min(sr0, q); sr1 = q + 1; }
                if (fi >= c0 && fi < c1) { sc0 = min(sc0, q); sc1 = q + 1; }
            }
            const int nr = max(sr1 - sr0, 0), ncs = max(sc1 - sc0, 0);
            const int np = (nr > 0 && ncs > 0) ? (diag ? nr * (nr + 1) / 2 : nr * ncs) : 0;
            int incl = np;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(incl, d); if (lane >= d) incl += t; }
            mLp[lane] = lp; mSeR[lane] = se0 + sr0; mNR[lane] = nr; mSeC[lane] = se0 + sc0; mNC[lane] = ncs;
            pref[lane] = incl - np;
            if (lane == 63) pref[64] = incl;
        }
        ba_wave_fence();
        const int P = pref[64];
        // ---- phase 2: 6 lanes = one (slot, slot) pair ------------------------------------------------------
        for (int pb = 0; pb < P; pb += 10) {
            const int pi = pb + g;
            if (g >= 10 || pi >= P) continue;
            int lo = 0, hi = 64;
#pragma unroll
            for (int it = 0; it < 6; it++) { const int mid = (lo + hi) >> 1; if (pref[mid] <= pi) lo = mid; else hi = mid; }
            int p = pi - pref[lo];
            const int nR_ = mNR[lo], nC_ = mNC[lo], lp = mLp[lo];
            int as = 0, bs;
            if (diag) { while (p >= nR_ - as) { p -= nR_ - as; as++; } bs = as + p; }
            else { as = p / nC_; bs = p - as * nC_; }
            const int e1 = mSeR[lo] + as, e2 = mSeC[lo] + bs;
            const int k1 = D.slotFi[e1] - r0, k2 = D.slotFi[e2] - c0;
            const double* w1p = Wn.Wg + (size_t)e1 * 18 + ri * 3;
            const double* w2p = Wn.Wg + (size_t)e2 * 18;
            const double* hp = Wn.Hg + (size_t)lp * BA_WIN_HG;
            const double w1[3] = {w1p[0], w1p[1], w1p[2]};
            double w2[18];
#pragma unroll
            for (int q = 0; q < 18; q++) w2[q] = w2p[q];
            const bool same = diag && e1 == e2;
            const double bl[3] = {same ? hp[6] : 0.0, same ? hp[7] : 0.0, same ? hp[8] : 0.0};
            for (int k = 0; k < nc; k++) {
#pragma clang fp contract(fast)
                double* Sacc = Sloc + (size_t)k * tile;
                const double* hi = hp + 9 + 6 * k;         // (Hll + lambda_k I)^-1: xx xy xz yy yz zz
                const double h0 = hi[0], h1 = hi[1], h2 = hi[2], h3 = hi[3], h4 = hi[4], h5 = hi[5];
                const double wh[3] = {w1[0] * h0 + w1[1] * h1 + w1[2] * h2, w1[0] * h1 + w1[1] * h3 + w1[2] * h4,
                                      w1[0] * h2 + w1[1] * h4 + w1[2] * h5};
                double* row = Sacc + (size_t)(6 * k1 + ri) * TP + 6 * k2;
#pragma unroll
                for (int j = 0; j < 6; j++) atomicAdd(&row[j], -(wh[0] * w2[3 * j] + wh[1] * w2[3 * j + 1] + wh[2] * w2[3 * j + 2]));
                if (same) atomicAdd(&Sacc[(size_t)T * TP + 6 * k1 + ri], -(wh[0] * bl[0] + wh[1] * bl[1] + wh[2] * bl[2]));
            }
            if (same) {
                // Hpp and bp of this slot's factors (the same for every candidate): row ri, columns >= ri
                for (int f = D.slotStart[e1]; f < D.slotStart[e1 + 1]; f++) {
                    const double* o = D.facJ + (size_t)f * 20;
                    const double a0 = o[2 + ri], a1 = o[8 + ri];
                    const double bp = -(a0 * o[0] + a1 * o[1]);
                    for (int k = 0; k < nc; k++) {
                        double* Sacc = Sloc + (size_t)k * tile;
                        for (int j = ri; j < 6; j++) atomicAdd(&Sacc[(size_t)(6 * k1 + ri) * TP + 6 * k1 + j], a0 * o[2 + j] + a1 * o[8 + j]);
                        atomicAdd(&Sacc[(size_t)T * TP + 6 * k1 + ri], bp);
                    }
                }
            }
        }
        ba_wave_fence();            // the entry table is rewritten for the next batch
    }
    __syncthreads();
    double* dst = Wn.part + (size_t)blockIdx.x * D.NB * tile;
    for (int i = threadIdx.x; i < nc * tile; i += nt) dst[i] = Sloc[i];
}

// fixed-order sum of a window's partials into the reduced system (+ the BetweenFactor blocks of this linearisation);
// grid (window, candidate).  Entries of the lower block triangle are never written nor read (the solvers mirror the upper one).
__global__ __launch_bounds__(256) void k_ba_reduce_win(const BaDev* __restrict__ tab, BaWin Wn) {
    BaDev D = *lane_entry(tab, blockIdx.z);      // per-lane argument block (grid z = problem of the batch)
    if (!ba_enter(D, BA_TRY, blockIdx.y)) return;
    const int win = blockIdx.x, cand = blockIdx.y, nc = D.NB, T = Wn.T, TP = Wn.TP, tile = Wn.tileDoubles, n = D.n;
    const int wa = Wn.winA[win], wb = Wn.winB[win];
    const int g0 = Wn.winFirstWg[win], g1 = Wn.winFirstWg[win + 1];
    const int rows = 6 * (min(D.F, (wa + 1) * Wn.TB) - wa * Wn.TB), cols = 6 * (min(D.F, (wb + 1) * Wn.TB) - wb * Wn.TB);
    const int lim = wa == wb ? T * TP + T : T * TP;
    for (int e = threadIdx.x; e < lim; e += 256) {
        size_t dst;
        if (e < T * TP) {
            const int r = e / TP, c = e - r * TP;
            if (r >= rows || c >= cols) continue;
            dst = (size_t)(6 * wa * Wn.TB + r) * n + 6 * wb * Wn.TB + c;
        } else {
            const int r = e - T * TP;
            if (r >= rows) continue;
            dst = (size_t)n * n + 6 * wa * Wn.TB + r;
        }
        double s0 = 0, s1 = 0;
        int g = g0;
        for (; g + 1 < g1; g += 2) {
            s0 += Wn.part[((size_t)g * nc + cand) * tile + e];
            s1 += Wn.part[((size_t)(g + 1) * nc + cand) * tile + e];
        }
        if (g < g1) s0 += Wn.part[((size_t)g * nc + cand) * tile + e];
        const double t = D.Sedge[dst] + (s0 + s1);
        if (D.specLin) D.Sedge2[dst] = 0;
        if (dst < (size_t)n * n) D.S[dst] = t; else D.rhs[dst - (size_t)n * n] = t;
    }
}

// One workgroup of n threads (rounded up to whole waves): thread i owns row i.  Assembles the
// reduced camera system from D.S / D.rhs (upper triangle valid) + BetweenFactor blocks + lambda I,
// left-looking Cholesky (2 barriers per column), the two substitutions (1 barrier per column), then
// retracts the trial poses.  A (n x n) lives in LDS when it fits, else in D.S (L2-resident).
__global__ __launch_bounds__(1024) void k_ba_solve(const BaDev* __restrict__ tab, int useLds, int ld) {
    BaDev D = *lane_entry(tab, blockIdx.z);      // per-lane argument block (grid z = problem of the batch)
    extern __shared__ double sm[];
    if (!ba_enter(D, BA_TRY, blockIdx.x)) return;      // one workgroup per lambda candidate
    const double lambda = D.lambda;
    const int n = D.n, tid = threadIdx.x, nt = blockDim.x;
    double* A = useLds ? sm : D.S;                              // leading dimension ld (LDS: odd multiple, conflict-free rows)
    double* col = useLds ? sm + (size_t)n * ld : D.rhs + n;     // n scratch doubles (D.rhs holds 2n)
    __shared__ int sFail;
    __shared__ double rhsl[1024], idiag[1024];
#ifdef VSLAM_BA_STAMPS
#define BA_STAMP(i) if (tid == 0) D.sums[8 + (i)] = (double)__builtin_readcyclecounter();
#else
#define BA_STAMP(i)
#endif
    BA_STAMP(0)
    if (tid == 0) sFail = 0;
    if (useLds) {
        // column c = lane, rows unrolled: independent coalesced loads (the upper triangle of D.S is valid)
        for (int c = tid; c < n; c += nt) {
#pragma unroll 6
            for (int r = 0; r < n; r++) A[(size_t)r * ld + c] = D.S[r <= c ? (size_t)r * n + c : (size_t)c * n + r];
        }
    } else {
        __syncthreads();
        for (int e = tid; e < n * n; e += nt) {
            const int r = e / n, c = e - r * n;
            if (r > c) A[e] = A[(size_t)c * n + r];
        }
    }
    if (tid < n) rhsl[tid] = D.rhs[tid];
    __syncthreads();
    BA_STAMP(1)
    BA_STAMP(2)
    if (tid < n) A[(size_t)tid * ld + tid] += lambda;
    __syncthreads();
    // Blocked left-looking Cholesky, 6-column panels (n is a multiple of 6): thread i owns row i.
    // Per panel: (1) row update against the finished columns, (2) every thread factors the 6x6
    // diagonal block redundantly in registers and solves its own row against it, (3) write-back.
    for (int J = 0; J < n; J += 6) {
        if (tid >= J && tid < n) {
            double u[6];
            double* ri = A + (size_t)tid * ld;
#pragma unroll
            for (int c = 0; c < 6; c++) u[c] = ri[J + c];
            // J is a multiple of 6: issue the 7 x 6 LDS reads of six columns together, then the FMAs
            for (int k = 0; k < J; k += 6) {
                double a[6], l[6][6];
#pragma unroll
                for (int q = 0; q < 6; q++) a[q] = ri[k + q];
#pragma unroll
                for (int c = 0; c < 6; c++)
#pragma unroll
                    for (int q = 0; q < 6; q++) l[c][q] = A[(size_t)(J + c) * ld + k + q];
#pragma unroll
                for (int q = 0; q < 6; q++)
#pragma unroll
                    for (int c = 0; c < 6; c++) u[c] -= a[q] * l[c][q];
            }
#pragma unroll
            for (int c = 0; c < 6; c++) ri[J + c] = u[c];
        }
        __syncthreads();
        double Ld[6][6], inv[6];
        bool bad = false;
#pragma unroll
        for (int r = 0; r < 6; r++)
#pragma unroll
            for (int c = 0; c <= r; c++) Ld[r][c] = A[(size_t)(J + r) * ld + J + c];
#pragma unroll
        for (int c = 0; c < 6; c++) {
            double d = Ld[c][c];
#pragma unroll
            for (int m = 0; m < c; m++) d -= Ld[c][m] * Ld[c][m];
            if (!(d > 0)) { bad = true; d = 1.0; }
            const double id = rsqrt(d);          // one reciprocal square root per pivot; the rest are multiplies
            Ld[c][c] = d * id;
            inv[c] = id;
#pragma unroll
            for (int r = c + 1; r < 6; r++) {
                double v = Ld[r][c];
#pragma unroll
                for (int m = 0; m < c; m++) v -= Ld[r][m] * Ld[c][m];
                Ld[r][c] = v * id;
            }
        }
        double x[6];
        if (tid > J + 5 && tid < n) {
            const double* ri = A + (size_t)tid * ld;
#pragma unroll
            for (int c = 0; c < 6; c++) {
                double v = ri[J + c];
#pragma unroll
                for (int m = 0; m < c; m++) v -= x[m] * Ld[c][m];
                x[c] = v * inv[c];
            }
        }
        __syncthreads();
        if (bad) { if (tid == 0) sFail = 1; break; }
        if (tid > J + 5 && tid < n) {
#pragma unroll
            for (int c = 0; c < 6; c++) A[(size_t)tid * ld + J + c] = x[c];
        } else if (tid >= J && tid < J + 6) {
            const int r = tid - J;
#pragma unroll
            for (int c = 0; c < 6; c++) if (c <= r) A[(size_t)tid * ld + J + c] = Ld[r][c];
            idiag[tid] = inv[r];
        }
        __syncthreads();
    }
    __syncthreads();
    BA_STAMP(3)
    if (!sFail) {
        // L y = b, panel by panel: the 6 unknowns of a panel are solved redundantly by every thread
        double* bv = rhsl;
        for (int J = 0; J < n; J += 6) {
            double y[6];
#pragma unroll
            for (int c = 0; c < 6; c++) {
                double v = bv[J + c];
#pragma unroll
                for (int m = 0; m < c; m++) v -= A[(size_t)(J + c) * ld + J + m] * y[m];
                y[c] = v * idiag[J + c];
            }
            if (tid > J + 5 && tid < n) {
                const double* ri = A + (size_t)tid * ld + J;
                double v = bv[tid];
#pragma unroll
                for (int c = 0; c < 6; c++) v -= ri[c] * y[c];
                bv[tid] = v;
            }
            if (tid == J) {
#pragma unroll
                for (int c = 0; c < 6; c++) col[J + c] = y[c];
            }
            __syncthreads();
        }
        BA_STAMP(4)
        // L^T x = y, panels in reverse
        for (int J = n - 6; J >= 0; J -= 6) {
            double x[6];
#pragma unroll
            for (int c = 5; c >= 0; c--) {
                double v = col[J + c];
#pragma unroll
                for (int m = 5; m > c; m--) v -= A[(size_t)(J + m) * ld + J + c] * x[m];
                x[c] = v * idiag[J + c];
            }
            __syncthreads();
            if (tid < J) {
                double v = col[tid];
#pragma unroll
                for (int c = 0; c < 6; c++) v -= A[(size_t)(J + c) * ld + tid] * x[c];
                col[tid] = v;
            }
            if (tid == J) {
#pragma unroll
                for (int c = 0; c < 6; c++) D.dP[J + c] = x[c];
            }
            __syncthreads();
        }
        BA_STAMP(5)
        for (int k = tid; k < D.K; k += nt) {
            const int fi = D.fidx[k];
            if (fi >= 0) { DPose T; pose_retract(D.poseCur[k], D.dP + 6 * fi, T); D.poseTrial[k] = T; }
            else D.poseTrial[k] = D.poseCur[k];
        }
    }
    __syncthreads();
    BA_STAMP(6)
    if (tid == 0) D.flags[FLAG_FAIL + D.cand] = sFail;
}

// Reduced camera systems of up to BA_WAVE_N unknowns (10 free keyframes - the reference's local window) are
// solved by ONE wave with the matrix in registers: lane i owns row i, pivots and multipliers travel by
// v_readlane, no LDS round trip or barrier per column.  Right-looking Cholesky (rsqrt pivots as in k_ba_solve),
// forward substitution, transpose of L through LDS, column-oriented back substitution, pose retraction.
__global__ __launch_bounds__(64) void k_ba_solve_wave(const BaDev* __restrict__ tab) {
    BaDev D = *lane_entry(tab, blockIdx.z);      // per-lane argument block (grid z = problem of the batch)
    constexpr int N = BA_WAVE_N;
    __shared__ double Lt[N * (N + 1)];
    if (D.solveKind != BA_SOLVE_WAVE) return;
    if (!ba_enter(D, BA_TRY, blockIdx.x)) return;      // one workgroup per lambda candidate
    const double lambda = D.lambda;
    const int n = D.n, lane = threadIdx.x;
    const int r = lane < N ? lane : N - 1;
    double a[N];
#ifdef VSLAM_BA_STAMPS
#define BAW_STAMP(i) if (lane == 0) D.sums[8 + (i)] = (double)__builtin_readcyclecounter();
#else
#define BAW_STAMP(i)
#endif
    BAW_STAMP(0)
    // stage D.S through LDS with coalesced row reads (lane = column), then every lane picks up its own row;
    // the upper triangle of D.S is the valid one, rows >= n are identity padding
    for (int row = 0; row < n; row++)
        if (lane < n) Lt[row * (N + 1) + lane] = D.S[(size_t)row * n + lane];
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int c = 0; c < N; c++) {
        double v = (c == r) ? 1.0 : 0.0;
        if (r < n && c < n) v = Lt[r <= c ? r * (N + 1) + c : c * (N + 1) + r] + ((c == r) ? lambda : 0.0);
        a[c] = v;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    double b = r < n ? D.rhs[r] : 0.0;
    bool bad = false;
    BAW_STAMP(1)
    BAW_STAMP(2)
    double idg = 1.0;                 // 1 / L[r][r] once the pivot of this lane's row is known
#pragma unroll
    for (int k = 0; k < N; k++) {
        double d = readlane_d(a[k], k);
        if (!(d > 0)) { bad = true; d = 1.0; }
        const double id = rsqrt(d);
        const double lk = (r == k) ? d * id : a[k] * id;
        if (r == k) idg = id;
        a[k] = lk;
#pragma unroll
        for (int j = k + 1; j < N; j++) a[j] = __builtin_fma(-lk, readlane_d(lk, j), a[j]);     // (this solve is not on the bit-exact path)
    }
    BAW_STAMP(3)
    if (!bad) {
        // L y = b
#pragma unroll
        for (int k = 0; k < N; k++) {
            const double yk = readlane_d(b, k) * readlane_d(idg, k);
            if (r == k) b = yk; else if (r > k) b -= a[k] * yk;
        }
        BAW_STAMP(4)
        // column form of L: lane i gets L[k][i], k >= i
        if (lane < N) {
#pragma unroll
            for (int j = 0; j < N; j++) Lt[lane * (N + 1) + j] = a[j];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int k = 0; k < N; k++) a[k] = Lt[k * (N + 1) + r];
        // L^T x = y
#pragma unroll
        for (int k = N - 1; k >= 0; k--) {
            const double xk = readlane_d(b, k) * readlane_d(idg, k);
            if (r == k) b = xk; else if (r < k) b -= a[k] * xk;
        }
        BAW_STAMP(5)
        if (lane < n) D.dP[lane] = b;
        Lt[lane] = b;                 // (the column reads above have completed: their values are in registers)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        for (int k = lane; k < D.K; k += 64) {
            const int fi = D.fidx[k];
            if (fi >= 0) { DPose T; pose_retract(D.poseCur[k], Lt + 6 * fi, T); D.poseTrial[k] = T; }
            else D.poseTrial[k] = D.poseCur[k];
        }
    }
    BAW_STAMP(6)
    if (lane == 0) D.flags[FLAG_FAIL + D.cand] = bad ? 1 : 0;
}

// Reduced camera systems of 61..256 unknowns (11..42 free keyframes, e.g. the 20-KF KITTI window): blocked
// right-looking Cholesky with the WHOLE lower triangle resident in MFMA accumulators - 136 tiles of 16x16 doubles
// over 8 waves (17 tiles = 136 VGPRs per wave, two waves per SIMD), so the factorisation never touches HBM.  (A
// 384-unknown system is 614 KB of tiles, more than one CU's 512 KB register file: it needs the two-workgroup form.)  Per block
// column: the owners drop the panel tiles into LDS, wave 0 factors the 16x16 diagonal block in registers, every
// thread solves one panel row against it, then every wave updates its tiles with v_mfma_f64_16x16x4 (A and B
// operands straight from the LDS panel).  L is streamed to global memory column block by column block for the
// blocked forward / backward substitutions that follow.  Padding rows are identity.
typedef double ba_d4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(64 * BA_MFMA_NW) void k_ba_solve_mfma(const BaDev* __restrict__ tab, double* __restrict__ Lg) {
    BaDev D = *lane_entry(tab, blockIdx.z);      // per-lane argument block (grid z = problem of the batch)
    extern __shared__ double sm[];
    double* P = sm;                                   // [BA_MFMA_N][BA_MFMA_LD] current panel
    double* sInv = P + BA_MFMA_N * BA_MFMA_LD;        // [16]
    double* sB = sInv + 16;                           // [BA_MFMA_N] right-hand side / solution
    __shared__ int sBad;
    if (D.solveKind != BA_SOLVE_MFMA) return;
    if (!ba_enter(D, BA_TRY, blockIdx.x)) return;      // one workgroup per lambda candidate
    const double lambda = D.lambda;
    constexpr int N = BA_MFMA_N, NB = BA_MFMA_NB, LD = BA_MFMA_LD;
    if (D.Lg) Lg = D.Lg;
    Lg += (size_t)D.cand * N * N;
    const int n = D.n, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // (wave-uniform: the tile coordinates below stay in SGPRs - 34 VGPRs and the last spills)
    if (tid == 0) sBad = 0;
    // tile t = ib (ib + 1) / 2 + jb (jb <= ib) lives in slot t / 8 of wave t % 8; accumulator layout of
    // v_mfma_f64_16x16x4: register r of lane l = element (row (l >> 4) + 4 r, column l & 15)
    ba_d4 acc[BA_MFMA_SLOTS];
    int tpk[BA_MFMA_SLOTS];          // ib | jb << 8 (ib = 255: no tile), one SGPR per slot
#pragma unroll
    for (int s = 0; s < BA_MFMA_SLOTS; s++) {
        const int t = s * BA_MFMA_NW + wave;
        int ib = 0;
        while ((ib + 1) * (ib + 2) / 2 <= t) ib++;
        const int jb = t - ib * (ib + 1) / 2;
        const bool valid = ib < NB;
        tpk[s] = (valid ? ib : 255) | (jb << 8);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = ib * 16 + (lane >> 4) + 4 * r, col = jb * 16 + (lane & 15);
            double v = (row == col) ? 1.0 : 0.0;              // identity padding
            if (valid && row < n && col < n) v = D.S[(size_t)col * n + row] + ((row == col) ? lambda : 0.0);   // upper triangle of D.S is the valid one
            acc[s][r] = v;
        }
    }
    for (int i = tid; i < N; i += 64 * BA_MFMA_NW) sB[i] = i < n ? D.rhs[i] : 0.0;
    __syncthreads();
    for (int kb = 0; kb < NB; kb++) {
        // (a) panel tiles (ib, kb), ib >= kb -> LDS
#pragma unroll
        for (int s = 0; s < BA_MFMA_SLOTS; s++) {
            const int tib = tpk[s] & 255, tjb = tpk[s] >> 8;
            if (tib != 255 && tib >= kb && tjb == kb) {
#pragma unroll
                for (int r = 0; r < 4; r++) P[(tib * 16 + (lane >> 4) + 4 * r) * LD + (lane & 15)] = acc[s][r];
            }
        }
        __syncthreads();
        // (b) 16x16 diagonal block: lane i = row i, pivots by readlane (as k_ba_solve_wave)
        if (wave == 0) {
            const int r = lane & 15;
            double a[16];
#pragma unroll
            for (int c = 0; c < 16; c++) a[c] = P[(kb * 16 + r) * LD + c];
            bool bad = false;
            double idg = 1.0;
#pragma unroll
            for (int k = 0; k < 16; k++) {
                double d = readlane_d(a[k], k);
                if (!(d > 0)) { bad = true; d = 1.0; }
                const double id = rsqrt(d);
                const double lk = (r == k) ? d * id : a[k] * id;
                if (r == k) idg = id;
                a[k] = lk;
#pragma unroll
                for (int j = k + 1; j < 16; j++) a[j] = __builtin_fma(-lk, readlane_d(lk, j), a[j]);
            }
            if (lane < 16) {
#pragma unroll
                for (int c = 0; c < 16; c++) P[(kb * 16 + r) * LD + c] = a[c];
                sInv[r] = idg;
            }
            if (bad && lane == 0) sBad = 1;
        }
        __syncthreads();
        // (c) panel rows below the diagonal block: row <- row L11^-T; the finished column block goes to global L
        for (int row = (kb + 1) * 16 + tid; row < N; row += 64 * BA_MFMA_NW) {
            double x[16];
#pragma unroll
            for (int c = 0; c < 16; c++) {
                double v = P[row * LD + c];
#pragma unroll
                for (int m = 0; m < c; m++) v = __builtin_fma(-x[m], P[(kb * 16 + c) * LD + m], v);
                x[c] = v * sInv[c];
            }
#pragma unroll
            for (int c = 0; c < 16; c++) { P[row * LD + c] = x[c]; Lg[(size_t)row * N + kb * 16 + c] = x[c]; }
        }
        if (tid < 16) {
#pragma unroll
            for (int c = 0; c < 16; c++) Lg[(size_t)(kb * 16 + tid) * N + kb * 16 + c] = c <= tid ? P[(kb * 16 + tid) * LD + c] : 0.0;
        }
        __syncthreads();
        // (d) trailing update: tile (ib, jb) -= L21[ib] L21[jb]^T, 4 k-steps of v_mfma_f64_16x16x4
#pragma unroll
        for (int s = 0; s < BA_MFMA_SLOTS; s++) {
            const int tib = tpk[s] & 255, tjb = tpk[s] >> 8;
            if (tib != 255 && tib > kb && tjb > kb) {
                const double* pa = P + (tib * 16 + (lane & 15)) * LD + (lane >> 4);
                const double* pb = P + (tjb * 16 + (lane & 15)) * LD + (lane >> 4);
#pragma unroll
                for (int ks = 0; ks < 4; ks++) acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(-pa[4 * ks], pb[4 * ks], acc[s], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    const bool fail = sBad != 0;
    if (!fail) {
        __threadfence_block();
        // L y = b, block by block: wave 0 solves the 16 unknowns of the block, every later row takes its 16 products
        for (int kb = 0; kb < NB; kb++) {
            if (wave == 0) {
                const int r = lane & 15;
                double b = sB[kb * 16 + r];
                double lrow[16];
#pragma unroll
                for (int c = 0; c < 16; c++) lrow[c] = Lg[(size_t)(kb * 16 + r) * N + kb * 16 + c];
#pragma unroll
                for (int k = 0; k < 16; k++) {
                    const double yk = readlane_d(b, k) / readlane_d(lrow[k], k);
                    if (r == k) b = yk; else if (r > k) b = __builtin_fma(-lrow[k], yk, b);
                }
                if (lane < 16) sB[kb * 16 + r] = b;
            }
            __syncthreads();
            for (int row = (kb + 1) * 16 + tid; row < N; row += 64 * BA_MFMA_NW) {
                double v = sB[row];
                const double* lr = Lg + (size_t)row * N + kb * 16;
#pragma unroll
                for (int c = 0; c < 16; c++) v = __builtin_fma(-lr[c], sB[kb * 16 + c], v);
                sB[row] = v;
            }
            __syncthreads();
        }
        // L^T x = y, blocks in reverse
        for (int kb = NB - 1; kb >= 0; kb--) {
            if (wave == 0) {
                const int r = lane & 15;
                double b = sB[kb * 16 + r];
                double lcol[16];                         // column r of the diagonal block = row r of its transpose
#pragma unroll
                for (int c = 0; c < 16; c++) lcol[c] = Lg[(size_t)(kb * 16 + c) * N + kb * 16 + r];
#pragma unroll
                for (int k = 15; k >= 0; k--) {
                    const double xk = readlane_d(b, k) / readlane_d(lcol[k], k);
                    if (r == k) b = xk; else if (r < k) b = __builtin_fma(-lcol[k], xk, b);
                }
                if (lane < 16) sB[kb * 16 + r] = b;
            }
            __syncthreads();
            for (int row = tid; row < kb * 16; row += 64 * BA_MFMA_NW) {
                double v = sB[row];
#pragma unroll
                for (int c = 0; c < 16; c++) v = __builtin_fma(-Lg[(size_t)(kb * 16 + c) * N + row], sB[kb * 16 + c], v);
                sB[row] = v;
            }
            __syncthreads();
        }
        for (int i = tid; i < n; i += 64 * BA_MFMA_NW) D.dP[i] = sB[i];
        for (int k = tid; k < D.K; k += 64 * BA_MFMA_NW) {
            const int fi = D.fidx[k];
            if (fi >= 0) { DPose T; pose_retract(D.poseCur[k], sB + 6 * fi, T); D.poseTrial[k] = T; }
            else D.poseTrial[k] = D.poseCur[k];
        }
    }
    if (tid == 0) D.flags[FLAG_FAIL + D.cand] = fail ? 1 : 0;
}

// The 10-keyframe window (6F <= 64) on ONE wave with the same MFMA scheme: the 10 lower tiles of the 64 x 64 system
// stay in accumulators, the panel / L live in LDS, no workgroup barrier anywhere (wave-ordered LDS traffic only).
__global__ __launch_bounds__(64) void k_ba_solve_mfma64(const BaDev* __restrict__ tab) {
    BaDev D = *lane_entry(tab, blockIdx.z);      // per-lane argument block (grid z = problem of the batch)
    constexpr int N = 64, LDF = 65, LD = 17;
    __shared__ double Lf[N * LDF];                    // staged system (upper triangle valid), then L (lower)
    __shared__ double P[N * LD];                      // current panel
    __shared__ double sInv[16], sB[N];
    if (D.solveKind != BA_SOLVE_MFMA64) return;
    if (!ba_enter(D, BA_TRY, blockIdx.x)) return;      // one workgroup per lambda candidate
    const double lambda = D.lambda;
    const int n = D.n, lane = threadIdx.x;
    auto fence = []() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); };
    for (int row = 0; row < n; row++)
        if (lane < n) Lf[row * LDF + lane] = D.S[(size_t)row * n + lane];
    sB[lane] = lane < n ? D.rhs[lane] : 0.0;
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    ba_d4 acc[10];
#pragma unroll
    for (int ib = 0; ib < 4; ib++)
#pragma unroll
        for (int jb = 0; jb <= ib; jb++) {
            const int s = ib * (ib + 1) / 2 + jb;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int row = ib * 16 + (lane >> 4) + 4 * r, col = jb * 16 + (lane & 15);
                double v = (row == col) ? 1.0 : 0.0;
                if (row < n && col < n) v = (row >= col ? Lf[col * LDF + row] : Lf[row * LDF + col]) + ((row == col) ? lambda : 0.0);
                acc[s][r] = v;
            }
        }
    fence();
    bool bad = false;
#pragma unroll
    for (int kb = 0; kb < 4; kb++) {
#pragma unroll
        for (int ib = kb; ib < 4; ib++) {
            const int s = ib * (ib + 1) / 2 + kb;
#pragma unroll
            for (int r = 0; r < 4; r++) P[(ib * 16 + (lane >> 4) + 4 * r) * LD + (lane & 15)] = acc[s][r];
        }
        fence();
        {
            const int r = lane & 15;
            double a[16];
#pragma unroll
            for (int c = 0; c < 16; c++) a[c] = P[(kb * 16 + r) * LD + c];
            double idg = 1.0;
#pragma unroll
            for (int k = 0; k < 16; k++) {
                double d = readlane_d(a[k], k);
                if (!(d > 0)) { bad = true; d = 1.0; }
                const double id = rsqrt(d);
                const double lk = (r == k) ? d * id : a[k] * id;
                if (r == k) idg = id;
                a[k] = lk;
#pragma unroll
                for (int j = k + 1; j < 16; j++) a[j] = __builtin_fma(-lk, readlane_d(lk, j), a[j]);
            }
            if (lane < 16) {
#pragma unroll
                for (int c = 0; c < 16; c++) { P[(kb * 16 + r) * LD + c] = a[c]; Lf[(kb * 16 + r) * LDF + kb * 16 + c] = c <= r ? a[c] : 0.0; }
                sInv[r] = idg;
            }
        }
        fence();
        {
            const int row = (kb + 1) * 16 + lane;
            if (row < N) {
                double x[16];
#pragma unroll
                for (int c = 0; c < 16; c++) {
                    double v = P[row * LD + c];
#pragma unroll
                    for (int m = 0; m < c; m++) v = __builtin_fma(-x[m], P[(kb * 16 + c) * LD + m], v);
                    x[c] = v * sInv[c];
                }
#pragma unroll
                for (int c = 0; c < 16; c++) { P[row * LD + c] = x[c]; Lf[row * LDF + kb * 16 + c] = x[c]; }
            }
        }
        fence();
#pragma unroll
        for (int ib = kb + 1; ib < 4; ib++)
#pragma unroll
            for (int jb = kb + 1; jb <= ib; jb++) {
                const int s = ib * (ib + 1) / 2 + jb;
                const double* pa = P + (ib * 16 + (lane & 15)) * LD + (lane >> 4);
                const double* pb = P + (jb * 16 + (lane & 15)) * LD + (lane >> 4);
#pragma unroll
                for (int ks = 0; ks < 4; ks++) acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(-pa[4 * ks], pb[4 * ks], acc[s], 0, 0, 0);
            }
        fence();
    }
    if (!bad) {
        // L y = b, L^T x = y: lane = row, columns in order; 1 / L[k][k] sits in lane k's register (readlane), the
        // multipliers of a column are one LDS read per lane, prefetched a few columns ahead by the unrolling
        const double inv = 1.0 / Lf[lane * LDF + lane];
        double b = sB[lane];
#pragma unroll 8
        for (int k = 0; k < N; k++) {
            const double lik = Lf[lane * LDF + k];
            const double yk = readlane_d(b, k) * readlane_d(inv, k);
            if (lane == k) b = yk; else if (lane > k) b = __builtin_fma(-lik, yk, b);
        }
#pragma unroll 8
        for (int k = N - 1; k >= 0; k--) {
            const double lki = Lf[k * LDF + lane];
            const double xk = readlane_d(b, k) * readlane_d(inv, k);
            if (lane == k) b = xk; else if (lane < k) b = __builtin_fma(-lki, xk, b);
        }
        if (lane < n) D.dP[lane] = b;
        sB[lane] = b;
        fence();
        for (int k = lane; k < D.K; k += 64) {
            const int fi = D.fidx[k];
            if (fi >= 0) { DPose T; pose_retract(D.poseCur[k], sB + 6 * fi, T); D.poseTrial[k] = T; }
            else D.poseTrial[k] = D.poseCur[k];
        }
    }
    if (lane == 0) D.flags[FLAG_FAIL + D.cand] = bad ? 1 : 0;
}

// ---- reduced camera systems of more than 256 unknowns (43..170 free keyframes; the 64-keyframe window = 384) ---------
// Blocked left-looking Cholesky over 64-column blocks, ONE LAUNCH PER BLOCK COLUMN J (the dependency chain of the
// factorisation is the launch order; inside a launch the row tiles are independent workgroups - no cross-workgroup
// synchronisation, nothing to spin on).  Workgroup I >= J (4 waves):
//   C  = A[I,J] - sum_{K<J} L[I,K] L[J,K]^T        64x64 tile in v_mfma_f64_16x16x4 accumulators (wave w: rows 16w..),
//   Dg = A[J,J] - sum_{K<J} L[J,K] L[J,K]^T        the diagonal tile, recomputed by every workgroup (cheaper than a
//                                                  second launch), factored L_JJ L_JJ^T in LDS / registers (16-column
//                                                  panels: readlane Cholesky of the 16x16 block, row-per-thread
//                                                  triangular solve, MFMA trailing update),
//   L[I,J] = C L_JJ^-T                             per wave on its own 16 rows: 16-column blocks, MFMA updates in between.
// The workgroup I == J also carries the forward substitution y_J = L_JJ^-1 (b_J - sum_K L[J,K] y_K).  L (N x N, N = n
// rounded up to 64, identity padding) and y live in HBM / L2.  k_ba_chol_back then solves L^T x = y block by block in
// one workgroup and retracts the trial poses.  (n = 384: 6 + 1 launches, ~0.15 ms, against 1.7 ms for the row-per-thread
// kernel this replaces.)

__global__ __launch_bounds__(256) void k_ba_chol_col(const BaDev* __restrict__ tab, double* __restrict__ Lg, double* __restrict__ yG, int N, int J, int* __restrict__ failFlag) {
    BaDev D = *lane_entry(tab, blockIdx.z);      // per-lane argument block (grid z = problem of the batch)
    extern __shared__ double sm[];
    double* sA = sm;                         // [64][65] L[I,K]; later the wave-private X rows of the triangular solve
    double* sB = sA + CH_B * CH_LD;          // [64][65] L[J,K]; later L_JJ
    double* sP = sB + CH_B * CH_LD;          // [64][17] current 16-column panel of the diagonal factorisation
    double* sInv = sP + CH_B * CH_PLD;       // [64] 1 / L_JJ[k][k]
    double* sT = sInv + CH_B;                // [64] forward-substitution right-hand side
    double* sY = sT + CH_B;                  // [64] y_K of the current K block
    __shared__ int sBad;
    if (!ba_enter(D, BA_TRY, blockIdx.y)) return;
    const double lambda = D.lambda;
    const int n = D.n, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int I = J + (int)blockIdx.x;
    const bool isDiag = blockIdx.x == 0;
    Lg += (size_t)D.cand * N * N; yG += (size_t)D.cand * N;
    if (tid == 0) sBad = 0;
    // A(i, j) of the damped system (upper triangle of D.S valid), identity padding
    auto Aij = [&](int i, int j) -> double {
        if (i >= n || j >= n) return i == j ? 1.0 : 0.0;
        return D.S[i <= j ? (size_t)i * n + j : (size_t)j * n + i] + (i == j ? lambda : 0.0);
    };
    ba_d4 accC[4], accD[4];
#pragma unroll
    for (int cb = 0; cb < 4; cb++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int lr = 16 * wave + (lane >> 4) + 4 * r, lc = cb * 16 + (lane & 15);
            accD[cb][r] = Aij(J * CH_B + lr, J * CH_B + lc);
            accC[cb][r] = isDiag ? 0.0 : Aij(I * CH_B + lr, J * CH_B + lc);
        }
    double t = 0;
    if (isDiag && tid < CH_B) t = (J * CH_B + tid) < n ? D.rhs[J * CH_B + tid] : 0.0;
    for (int K = 0; K < J; K++) {
        __syncthreads();
        for (int e = tid; e < CH_B * CH_B; e += 256) {
            const int r = e >> 6, c = e & 63;
            sB[r * CH_LD + c] = Lg[(size_t)(J * CH_B + r) * N + K * CH_B + c];
            if (!isDiag) sA[r * CH_LD + c] = Lg[(size_t)(I * CH_B + r) * N + K * CH_B + c];
        }
        if (isDiag && tid < CH_B) sY[tid] = yG[K * CH_B + tid];
        __syncthreads();
        const double* pd = sB + (16 * wave + (lane & 15)) * CH_LD + (lane >> 4);
        const double* pa = sA + (16 * wave + (lane & 15)) * CH_LD + (lane >> 4);
#pragma unroll
        for (int cb = 0; cb < 4; cb++) {
            const double* pb = sB + (cb * 16 + (lane & 15)) * CH_LD + (lane >> 4);
#pragma unroll
            for (int ks = 0; ks < 16; ks++) {
                const double b = pb[4 * ks];
                if (cb <= wave) accD[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(-pd[4 * ks], b, accD[cb], 0, 0, 0);
                if (!isDiag) accC[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(-pa[4 * ks], b, accC[cb], 0, 0, 0);
            }
        }
        if (isDiag && tid < CH_B) {
            const double* lr = sB + tid * CH_LD;
            double a0 = 0, a1 = 0;
#pragma unroll 8
            for (int c = 0; c < CH_B; c += 2) { a0 += lr[c] * sY[c]; a1 += lr[c + 1] * sY[c + 1]; }
            t -= a0 + a1;
        }
    }
    __syncthreads();
    // ---- factor the diagonal tile: wave ib owns tile row ib (subtiles jb <= ib); L_JJ is assembled in sB ----------
    for (int e = tid; e < CH_B * CH_LD; e += 256) sB[e] = 0.0;
    __syncthreads();
#pragma unroll
    for (int kb = 0; kb < 4; kb++) {
        if (wave >= kb) {
#pragma unroll
            for (int r = 0; r < 4; r++) sP[(wave * 16 + (lane >> 4) + 4 * r) * CH_PLD + (lane & 15)] = accD[kb][r];
        }
        __syncthreads();
        if (wave == 0) {
            const int r = lane & 15;
            double a[16];
#pragma unroll
            for (int c = 0; c < 16; c++) a[c] = sP[(kb * 16 + r) * CH_PLD + c];
            bool bad = false;
            double idg = 1.0;
#pragma unroll
            for (int k = 0; k < 16; k++) {
                double d = readlane_d(a[k], k);
                if (!(d > 0)) { bad = true; d = 1.0; }
                const double id = rsqrt(d);
                const double lk = (r == k) ? d * id : a[k] * id;
                if (r == k) idg = id;
                a[k] = lk;
#pragma unroll
                for (int j = k + 1; j < 16; j++) a[j] = __builtin_fma(-lk, readlane_d(lk, j), a[j]);
            }
            if (lane < 16) {
#pragma unroll
                for (int c = 0; c < 16; c++) { sP[(kb * 16 + r) * CH_PLD + c] = a[c]; sB[(kb * 16 + r) * CH_LD + kb * 16 + c] = c <= r ? a[c] : 0.0; }
                sInv[kb * 16 + r] = idg;
            }
            if (bad && lane == 0) sBad = 1;
        }
        __syncthreads();
        {
            const int row = (kb + 1) * 16 + tid;
            if (row < CH_B) {
                double x[16];
#pragma unroll
                for (int c = 0; c < 16; c++) {
                    double v = sP[row * CH_PLD + c];
#pragma unroll
                    for (int m = 0; m < c; m++) v = __builtin_fma(-x[m], sP[(kb * 16 + c) * CH_PLD + m], v);
                    x[c] = v * sInv[kb * 16 + c];
                }
#pragma unroll
                for (int c = 0; c < 16; c++) { sP[row * CH_PLD + c] = x[c]; sB[row * CH_LD + kb * 16 + c] = x[c]; }
            }
        }
        __syncthreads();
        if (wave > kb) {
            const double* pa = sP + (wave * 16 + (lane & 15)) * CH_PLD + (lane >> 4);
#pragma unroll
            for (int jb = 1; jb < 4; jb++) {
                if (jb > kb && jb <= wave) {
                    const double* pb = sP + (jb * 16 + (lane & 15)) * CH_PLD + (lane >> 4);
#pragma unroll
                    for (int ks = 0; ks < 4; ks++) accD[jb] = __builtin_amdgcn_mfma_f64_16x16x4f64(-pa[4 * ks], pb[4 * ks], accD[jb], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }
    if (sBad) { if (tid == 0) atomicOr(failFlag + D.cand, 1); }
    if (isDiag) {
        for (int e = tid; e < CH_B * CH_B; e += 256) {
            const int r = e >> 6, c = e & 63;
            Lg[(size_t)(J * CH_B + r) * N + J * CH_B + c] = sB[r * CH_LD + c];
        }
        if (tid < CH_B) sT[tid] = t;
        __syncthreads();
        if (wave == 0) {          // y_J = L_JJ^-1 t : lane = row, columns in order
            double b = sT[lane];
            const double inv = sInv[lane];
#pragma unroll 8
            for (int k = 0; k < CH_B; k++) {
                const double lik = sB[lane * CH_LD + k];
                const double yk = readlane_d(b, k) * readlane_d(inv, k);
                if (lane == k) b = yk; else if (lane > k) b = __builtin_fma(-lik, yk, b);
            }
            yG[J * CH_B + lane] = b;
        }
        return;
    }
    // ---- X = C L_JJ^-T on the wave's own 16 rows: 16-column blocks; no workgroup barrier (wave-ordered LDS traffic) ----
    double* X = sA + (size_t)(16 * wave) * CH_LD;
#pragma unroll
    for (int cb = 0; cb < 4; cb++) {
#pragma unroll
        for (int r = 0; r < 4; r++) X[((lane >> 4) + 4 * r) * CH_LD + cb * 16 + (lane & 15)] = accC[cb][r];
        ba_wave_fence();
        if (lane < 16) {
            double x[16];
#pragma unroll
            for (int c = 0; c < 16; c++) {
                double v = X[lane * CH_LD + cb * 16 + c];
#pragma unroll
                for (int m = 0; m < c; m++) v = __builtin_fma(-x[m], sB[(cb * 16 + c) * CH_LD + cb * 16 + m], v);
                x[c] = v * sInv[cb * 16 + c];
            }
#pragma unroll
            for (int c = 0; c < 16; c++) X[lane * CH_LD + cb * 16 + c] = x[c];
        }
        ba_wave_fence();
        const double* pa = X + (lane & 15) * CH_LD + cb * 16 + (lane >> 4);
#pragma unroll
        for (int c2 = 1; c2 < 4; c2++) {
            if (c2 > cb) {
                const double* pb = sB + (c2 * 16 + (lane & 15)) * CH_LD + cb * 16 + (lane >> 4);
#pragma unroll
                for (int ks = 0; ks < 4; ks++) accC[c2] = __builtin_amdgcn_mfma_f64_16x16x4f64(-pa[4 * ks], pb[4 * ks], accC[c2], 0, 0, 0);
            }
        }
    }
    ba_wave_fence();
    for (int e = lane; e < 16 * CH_B; e += 64) {
        const int r = e >> 6, c = e & 63;
        Lg[(size_t)(I * CH_B + 16 * wave + r) * N + J * CH_B + c] = X[r * CH_LD + c];
    }
}

// L^T x = y, block columns in reverse, one workgroup per candidate; then the trial poses
__global__ __launch_bounds__(256) void k_ba_chol_back(const BaDev* __restrict__ tab, const double* __restrict__ Lg, const double* __restrict__ yG, int N, int* __restrict__ failFlag) {
    BaDev D = *lane_entry(tab, blockIdx.z);      // per-lane argument block (grid z = problem of the batch)
    extern __shared__ double sm[];
    double* sL = sm;                 // [64][65] L_JJ
    double* sX = sL + CH_B * CH_LD;  // [N] solution
    double* sR = sX + N;             // [4][64] partial sums
    if (!ba_enter(D, BA_TRY, blockIdx.x)) return;
    const int n = D.n, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    Lg += (size_t)D.cand * N * N; yG += (size_t)D.cand * N;
    const bool fail = failFlag[D.cand] != 0;
    __syncthreads();
    if (tid == 0) { D.flags[FLAG_FAIL + D.cand] = fail ? 1 : 0; failFlag[D.cand] = 0; }
    if (fail) return;
    const int NBk = N / CH_B;
    for (int J = NBk - 1; J >= 0; J--) {
        // t_j = y_J[j] - sum_{i >= (J+1) 64} L[i][J 64 + j] x[i] : thread (g, j) takes the rows i = g (mod 4)
        double acc = 0;
        for (int i = (J + 1) * CH_B + wave; i < N; i += 4) acc += Lg[(size_t)i * N + J * CH_B + lane] * sX[i];
        sR[wave * CH_B + lane] = acc;
        for (int e = tid; e < CH_B * CH_B; e += 256) {
            const int r = e >> 6, c = e & 63;
            sL[r * CH_LD + c] = Lg[(size_t)(J * CH_B + r) * N + J * CH_B + c];
        }
        __syncthreads();
        if (wave == 0) {
            double b = yG[J * CH_B + lane] - ((sR[lane] + sR[CH_B + lane]) + (sR[2 * CH_B + lane] + sR[3 * CH_B + lane]));
            const double inv = 1.0 / sL[lane * CH_LD + lane];
#pragma unroll 8
            for (int k = CH_B - 1; k >= 0; k--) {
                const double lki = sL[k * CH_LD + lane];
                const double xk = readlane_d(b, k) * readlane_d(inv, k);
                if (lane == k) b = xk; else if (lane < k) b = __builtin_fma(-lki, xk, b);
            }
            sX[J * CH_B + lane] = b;
        }
        __syncthreads();
    }
    for (int i = tid; i < n; i += 256) D.dP[i] = sX[i];
    for (int k = tid; k < D.K; k += 256) {
        const int fi = D.fidx[k];
        if (fi >= 0) { DPose T; pose_retract(D.poseCur[k], sX + 6 * fi, T); D.poseTrial[k] = T; }
        else D.poseTrial[k] = D.poseCur[k];
    }
}

// back-substitution: dl = Hll^-1 (bl - sum_k W_k^T dp_k); trial landmark = cur + dl.  One wave per landmark;
// allCand: the wave serves every lambda candidate from one build of Hll / bl / W (grid y = 1), else grid y = candidate.
__global__ __launch_bounds__(64 * BA_SCHUR_WAVES) void k_ba_back(const BaDev* __restrict__ tab, int maxSlots, int allCand) {
    BaDev D = *lane_entry(tab, blockIdx.z);      // per-lane argument block (grid z = problem of the batch)
    extern __shared__ double sm[];
    const int c0 = allCand ? 0 : (int)blockIdx.y;
    if (!ba_enter(D, BA_TRY, c0)) return;
    const int nc = allCand ? D.nAct : 1;
    const int sel = ((const int*)(D.ctl + CTL_INTS))[CI_SEL];
    constexpr int BA_LPL = BA_LPL_BACK;
    const int lane = threadIdx.x & (BA_LPL - 1), unit = threadIdx.x / BA_LPL;
    double* W = sm + (size_t)unit * (maxSlots * 18);
    const int nu = blockDim.x / BA_LPL;
    int* sfi = (int*)(sm + (size_t)nu * (maxSlots * 18)) + unit * maxSlots;
    const int rounds = (D.Lp + gridDim.x * nu - 1) / (gridDim.x * nu);
    for (int rd = 0; rd < rounds; rd++) {
        const int lp = (rd * gridDim.x + blockIdx.x) * nu + unit;
        const bool act = lp < D.Lp;
        double h[9];
        int ns = 0;
        ba_lm_blocks<BA_LPL>(D, lp, act, W, sfi, h, ns);
        ba_wave_fence();
        const int l = act ? D.lpOrig[lp] : 0;
        double lamk = D.lambda;
        for (int k = 0; k < nc; k++, lamk *= 10.0) {
            const double* dPk = D.dP + (size_t)k * D.n;         // (ba_enter already applied candidate c0)
            double Hi[9];
            ba_hll_inverse(h, lamk, Hi);
            double t[3] = {0, 0, 0};
            for (int e = lane; e < ns * 6; e += BA_LPL) {
                const int s = e / 6, i = e - s * 6;
                const double dp = dPk[6 * sfi[s] + i];
                const double* w = W + s * 18 + i * 3;
                t[0] += w[0] * dp; t[1] += w[1] * dp; t[2] += w[2] * dp;
            }
#pragma unroll
            for (int q = 0; q < 3; q++) {
#pragma unroll
                for (int d = BA_LPL / 2; d >= 1; d >>= 1) t[q] += __shfl_xor(t[q], d);
            }
            if (act && lane < 3) {
                const double u[3] = {h[6] - t[0], h[7] - t[1], h[8] - t[2]};
                // (row `lane` of Hi picked by selects: indexing the register array by the lane would put it in scratch)
                const double h0 = lane == 0 ? Hi[0] : (lane == 1 ? Hi[3] : Hi[6]);
                const double h1 = lane == 0 ? Hi[1] : (lane == 1 ? Hi[4] : Hi[7]);
                const double h2 = lane == 0 ? Hi[2] : (lane == 1 ? Hi[5] : Hi[8]);
                const double dl = h0 * u[0] + h1 * u[1] + h2 * u[2];
                D.dL[(size_t)k * D.dLStride + 3 * (size_t)lp + lane] = dl;
                double* lmT = D.lmBase + (size_t)ba_slot(sel, c0 + k, D.NB) * D.lmStride;
                lmT[3 * (size_t)l + lane] = D.lmCur[3 * (size_t)l + lane] + dl;
            }
        }
        ba_wave_fence();            // W / sfi are rewritten in the next round
    }
}

// chi2 re-check (src/OptimizationBA.cpp:787-871): pair-parallel
__device__ __forceinline__ bool ba_outlier(const BaChi& C, const double* pc, float ou, float ov, int oct, bool right) {
    const double x = right ? pc[0] - C.b : pc[0], y = pc[1], z = pc[2];
    if (z <= 0) return true;
    const double px = C.fx * x + C.cx * z, py = C.fy * y + C.cy * z;
    const double eu = (double)ou - px / z, ev = (double)ov - py / z;
    return (eu * eu + ev * ev) > (double)C.thr[oct];
}
__global__ __launch_bounds__(256) void k_ba_chi2(BaChi C) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= C.NP) return;
    uint8_t w = 0;
    const int kf = C.pairKf[p], lm = C.pairLm[p], fl = C.pairFlags[p];
    if (C.kfLocal[kf] && C.kfPresent[kf] && C.lmPresent[lm] && (fl & 3)) {
        DPose Tcw;
        pose_inverse(C.pose[kf], Tcw);
        double pc[3];
        mat3_vec(Tcw.R, C.lm + 3 * (size_t)lm, pc);
        for (int i = 0; i < 3; i++) pc[i] += Tcw.t[i];
        const float* uv = C.pairUv + 4 * (size_t)p;
        if (fl & 1) {
            if (ba_outlier(C, pc, uv[0], uv[1], C.pairOct[2 * p], false)) w = 1;
            else if ((fl & 2) && ba_outlier(C, pc, uv[2], uv[3], C.pairOct[2 * p + 1], true)) w = 1;
        } else if (ba_outlier(C, pc, uv[2], uv[3], C.pairOct[2 * p + 1], true)) w = 1;
    }
    C.wrong[p] = w;
}

// MapPoint::updatePos (src/Map.cpp:212-234) for every kFMatches entry: depth / close refresh from the optimised values.
// The close threshold (40 x baseline) is the camera's: kfCloseTh != null holds one per staged keyframe pose (the merged requests of a
// lockstep group's lanes, whose rigs may differ); null: closeTh for every pair (one request, one rig).
__global__ __launch_bounds__(256) void k_ba_refresh_depth(int NP, const int* __restrict__ pairKf, const int* __restrict__ pairLm,
                                                          const uint8_t* __restrict__ pairWrong, const uint8_t* __restrict__ lmOutlier,
                                                          const float* __restrict__ curDepth, const DPose* __restrict__ Tcw,
                                                          const double* __restrict__ lm, const float* __restrict__ kfCloseTh, float closeTh,
                                                          float* __restrict__ depthOut, uint8_t* __restrict__ closeOut,
                                                          uint8_t* __restrict__ updated) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= NP) return;
    uint8_t up = 0, cl = 0;
    float d = 0.f;
    const int l = pairLm[p];
    if (!pairWrong[p] && !lmOutlier[l] && !(curDepth[p] <= 0)) {
        const int k = pairKf[p];
        const DPose& T = Tcw[k];
        const double* w = lm + 3 * (size_t)l;
        const double z = T.R[6] * w[0] + T.R[7] * w[1] + T.R[8] * w[2] + T.t[2] * 1.0;     // row 2 of getInvPose() * wp
        d = (float)z;
        const float th = kfCloseTh ? kfCloseTh[k] : closeTh;
        cl = z <= (double)th ? 1 : 0;
        up = 1;
    }
    depthOut[p] = d; closeOut[p] = cl; updated[p] = up;
}

// landmark exchange of the sharded path: diff = cur - init (zero for landmarks this rank does not own),
// all-reduce, cur = init + diff
__global__ __launch_bounds__(256) void k_ba_lm_diff(int n, const double* __restrict__ cur, const double* __restrict__ init,
                                                    double* __restrict__ diff, int mode) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (mode == 0) diff[i] = cur[i] - init[i];
}
__global__ __launch_bounds__(256) void k_ba_lm_apply(int n, double* __restrict__ cur, const double* __restrict__ init,
                                                     const double* __restrict__ diff) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) cur[i] = init[i] + diff[i];
}

// Second pass without a rebuild: the factors of the pairs the first chi2 check rejected get weight zero (exact-zero
// residual and Jacobian rows), everything else - ordering, slots, free set - is the first pass's structure.
__global__ __launch_bounds__(256) void k_ba_mask(int NF, const int* __restrict__ facPair, const uint8_t* __restrict__ wrong,
                                                 double* __restrict__ facIs) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f < NF && wrong[facPair[f]]) facIs[f] = 0.0;
}

// every value slot starts from the caller's poses / landmarks (landmarks outside the graph are never rewritten)
__global__ __launch_bounds__(256) void k_ba_init_slots(int nPose, const double* __restrict__ pose0, double* __restrict__ poseBase,
                                                       int nLm, const double* __restrict__ lm0, double* __restrict__ lmBase) {
    const int i = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
    if (i < nPose) poseBase[(size_t)s * nPose + i] = pose0[i];
    if (i < nLm) lmBase[(size_t)s * nLm + i] = lm0[i];
}

// ---- batch-only kernels: the steps the one-problem path drives from the host, per lane of a batch (grid y = lane) ----------
// (the lane's BaChi block stays in the constant-addressed table - thr[oct] is indexed there: a by-value copy of the struct put its
//  threshold array in scratch, 192 bytes per lane)
__device__ __forceinline__ bool ba_outlier_at(const BaChi& C, const double* pc, float ou, float ov, int oct, bool right) {
    const double x = right ? pc[0] - C.b : pc[0], y = pc[1], z = pc[2];
    if (z <= 0) return true;
    const double px = C.fx * x + C.cx * z, py = C.fy * y + C.cy * z;
    const double eu = (double)ou - px / z, ev = (double)ov - py / z;
    return (eu * eu + ev * ev) > (double)C.thr[oct];
}
__global__ __launch_bounds__(256) void k_ba_chi2_b(const BaDev* __restrict__ tab, const BaLaneAux* __restrict__ aux, int gather) {
    const BaDev& D = *lane_entry(tab, blockIdx.y);
    const BaLaneAux& X = *lane_entry(aux, blockIdx.y);
    const BaChi& C = X.C;
    const int* ci = (const int*)(D.ctl + CTL_INTS);
    if (ci[CI_STATE] != BA_DONE) return;             // (lanes handed to the one-problem path keep BA_LINEARIZE / are skipped by the host)
    const int sel = ci[CI_SEL];
    const DPose* const pose = D.poseBase + (size_t)sel * D.K;
    const double* const lmv = D.lmBase + (size_t)sel * D.lmStride;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (gather) {                                    // the pass's result next to its flags
        for (int i = p; i < X.nPose; i += gridDim.x * 256) X.outPose[i] = ((const double*)pose)[i];
        for (int i = p; i < X.nLm; i += gridDim.x * 256) X.outLm[i] = lmv[i];
    }
    if (p >= C.NP) return;
    uint8_t w = 0;
    const int kf = C.pairKf[p], lm = C.pairLm[p], fl = C.pairFlags[p];
    if (C.kfLocal[kf] && C.kfPresent[kf] && C.lmPresent[lm] && (fl & 3)) {
        DPose Tcw;
        pose_inverse(pose[kf], Tcw);
        double pc[3];
        mat3_vec(Tcw.R, lmv + 3 * (size_t)lm, pc);
        for (int i = 0; i < 3; i++) pc[i] += Tcw.t[i];
        const float* uv = C.pairUv + 4 * (size_t)p;
        if (fl & 1) {
            if (ba_outlier_at(C, pc, uv[0], uv[1], C.pairOct[2 * p], false)) w = 1;
            else if ((fl & 2) && ba_outlier_at(C, pc, uv[2], uv[3], C.pairOct[2 * p + 1], true)) w = 1;
        } else if (ba_outlier_at(C, pc, uv[2], uv[3], C.pairOct[2 * p + 1], true)) w = 1;
    }
    C.wrong[p] = w;
}
__global__ __launch_bounds__(256) void k_ba_second_pass_b(const BaDev* __restrict__ tab, const BaLaneAux* __restrict__ aux) {
    const BaDev& D = *lane_entry(tab, blockIdx.y);
    const BaLaneAux& X = *lane_entry(aux, blockIdx.y);
    const int* ci = (const int*)(D.ctl + CTL_INTS);
    if (ci[CI_STATE] != BA_LINEARIZE || !ci[CI_FIRST]) return;      // only lanes whose control block was re-armed for pass 2
    const int i = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    for (int f = i; f < X.NF; f += stride) if (X.C.wrong[X.facPair[f]]) X.facIs[f] = 0.0;
    for (int s2 = 0; s2 <= D.NB; s2++) {
        for (int q = i; q < X.nPose; q += stride) ((double*)D.poseBase)[(size_t)s2 * X.nPose + q] = X.pose0[q];
        for (int q = i; q < X.nLm; q += stride) D.lmBase[(size_t)s2 * D.lmStride + q] = X.lm0[q];
    }
    for (int q = i; q < D.n * D.n + D.n; q += stride) D.SedgeBase[q] = 0;        // first linearisation of the pass accumulates into slot 0
}
__global__ __launch_bounds__(256) void k_ba_init_slots_b(const BaDev* __restrict__ tab, const BaLaneAux* __restrict__ aux) {
    const BaDev& D = *lane_entry(tab, blockIdx.y);
    const BaLaneAux& X = *lane_entry(aux, blockIdx.y);
    const int i = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    for (int s2 = 0; s2 <= D.NB; s2++) {
        for (int q = i; q < X.nPose; q += stride) ((double*)D.poseBase)[(size_t)s2 * X.nPose + q] = X.pose0[q];
        for (int q = i; q < X.nLm; q += stride) D.lmBase[(size_t)s2 * D.lmStride + q] = X.lm0[q];
    }
}


}  // namespace vslam

using namespace vslam;

namespace {

// ---- the grow-only buffers of the workspaces: GrowBuf (grow_buf.hpp) over device memory and pinned host memory -------------------
struct DeviceAlloc {
    static hipError_t alloc(void** p, size_t bytes) {      // (hipMalloc: with the debug poison fill, common.hpp)
        const hipError_t e = hipMalloc(p, bytes);
        if (e != hipSuccess && *p) { (void)hipFree(*p); *p = nullptr; }      // (the fill failed: no block without success)
        return e;
    }
    static void free(void* p) { (void)hipFree(p); }
};
struct PinnedAlloc {
    static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void free(void* p) { (void)hipHostFree(p); }
};
template <typename T>
struct DevBuf : GrowBuf<T, DeviceAlloc> {
    // grow with headroom (grow_dev): a mapping thread serves sessions whose windows differ a little from call to call, and every
    // new maximum used to cost a hipFree (a device-wide synchronisation: it waits for the lockstep groups' kernels) +
    // hipMalloc - 1.6 ms per local BA on average at 128 sessions.
    // (A request of 0 still gives an empty buffer its floor block: the argument blocks of the kernels carry no null pointers.)
    hipError_t alloc(size_t count) { return this->ensure(std::max<size_t>(count, 1), grow_dev<T>()); }
};
using PinBuf = GrowBuf<uint8_t, PinnedAlloc>;      // (sized in bytes)
static_assert(sizeof(DevBuf<double>) == sizeof(PinBuf), "release_bufs counts the buffers of a struct by its size");
// frees the N buffers of a struct that holds nothing else: one that is added to the struct and not named here does not compile
template <size_t N, class... B>
void release_bufs(B&... b) {
    static_assert(sizeof...(B) == N, "every buffer of the struct is released");
    (b.release(), ...);
}

thread_local StageTimer g_baTimer;

// Pinned host arena with a device mirror: the per-pass index / measurement arrays are written straight into
// pinned memory and travel in ONE copy.
struct PinnedArena : BaArenaView {
    uint8_t* d = nullptr;
    PinBuf hostHalf;
    GrowBuf<uint8_t, DeviceAlloc> devHalf;
    hipError_t ensure(size_t bytes, hipStream_t s) {
        if (bytes <= cap) return hipSuccess;
        hipError_t e = hipStreamSynchronize(s);
        if (e != hipSuccess) return e;
        release();      // (re-growing costs a synchronisation + two device-synchronising frees)
        e = hostHalf.ensure(bytes, grow_block());
        if (e == hipSuccess) e = devHalf.ensure(bytes, grow_block());
        if (e != hipSuccess) { release(); return e; }      // (one half without the other is no arena)
        h = hostHalf.p; d = devHalf.p; cap = hostHalf.n;
        return hipSuccess;
    }
    void release() { hostHalf.release(); devHalf.release(); h = nullptr; d = nullptr; cap = 0; }
    template <class T> T* dev(T* hostPtr) const { return (T*)(d + ((uint8_t*)hostPtr - h)); }
    hipError_t upload(hipStream_t s) const { return hipMemcpyAsync(d, h, used, hipMemcpyHostToDevice, s); }
};

// the problem's pair arrays (device addresses): what the chi2 kernels and the device ordering read
struct BaPairArrays { const int* kf; const int* lm; const int* oct; const uint8_t* flags; const float* uv; const uint8_t* kfLocal; };

}  // namespace

#include "ba_order_dev.hpp"       // k_ord_* / k_win_* and their host unit (BaDeviceOrder)

namespace {

// vslam_local_ba_set_lookahead (-1: environment / default).  Like the timing switch and the workspace these belong to
// the CALLING THREAD (one optimizer thread = one local-BA context): sessions with different settings do not interact.
thread_local int g_baLookahead = -1, g_baSpecLin = -1, g_baMask = 1, g_baSolver = -1;      // g_baSolver: -1 default (env), 0 MFMA forms, 1 wave / LDS forms
static bool ba_use_mfma() {
    static const bool envOff = getenv("VSLAM_BA_NO_MFMA") != nullptr;      // process-wide default; vslam_local_ba_set_solver overrides it per thread
    return g_baSolver < 0 ? !envOff : g_baSolver == 0;
}
// lambda look-ahead (see BaDev): candidates per trial round and speculative linearisation - the thread's setting, else the environment
struct BaLmKnobs { int NB; bool specLin; };
static BaLmKnobs ba_lm_knobs() {
    static const int nbEnv = [] { const char* e = getenv("VSLAM_BA_LOOKAHEAD"); return e ? std::max(1, std::min((int)BA_MAX_NB, atoi(e))) : (int)BA_MAX_NB; }();
    static const bool specEnv = !getenv("VSLAM_BA_NO_SPECLIN");
    return {g_baLookahead > 0 ? std::min(g_baLookahead, (int)BA_MAX_NB) : nbEnv, g_baSpecLin >= 0 ? g_baSpecLin != 0 : specEnv};
}
static int ba_adaptive_env() { const char* e = getenv("VSLAM_BA_ADAPTIVE"); return e ? atoi(e) : -1; }      // -1: the caller's default

// the device of a call: there is one, `device` names one (ba_select_device: and it becomes the calling thread's current device)
static vslam_status ba_check_device(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available (no CPU fallback)"); return VSLAM_ERR_NO_DEVICE; }
    return device < 0 || device >= ndev ? VSLAM_ERR_INVALID : VSLAM_OK;
}
static vslam_status ba_select_device(int device) {
    VS_CHECK(ba_check_device(device));
    VS_HIP(hipSetDevice(device));
    return VSLAM_OK;
}

// The fields of a problem's argument block that both entry points fill alike: the pass's arrays in the arena, the value slots and
// work buffers of the lane.  The caller adds what is its own: partial / Spart (+ strides), solveKind, Lg, ctlHost.
struct BaLaneBufs { int K, L; DPose* poseS; double *lmS, *facJ, *S, *Sedge, *dP, *dL, *sums; int* flags; };
static void ba_fill_dev(BaDev& D, const BaPassHost& H, const PinnedArena& A, const BaLaneBufs& B, const vslam_rig& rig, int NB, bool specLin, bool adaptive) {
    const int n = H.n;
    D.NF = H.NF; D.Lp = H.Lp; D.F = H.F; D.K = B.K; D.NE = H.NE; D.n = n;
    D.facKf = A.dev(H.h_facKf); D.facFi = A.dev(H.h_facFi); D.facLp = A.dev(H.h_facLp); D.facLm = A.dev(H.h_facLm);
    D.facZ = A.dev(H.h_facZ); D.facIs = A.dev(H.h_facIs); D.facRight = A.dev(H.h_facRight); D.facJ = B.facJ;
    D.lpStart = A.dev(H.h_lpStart); D.lpSlotStart = A.dev(H.h_lpSlotStart); D.slotStart = A.dev(H.h_slotStart); D.slotFi = A.dev(H.h_slotFi);
    D.lpOrig = A.dev(H.h_lpOrig); D.poseCur = B.poseS; D.poseTrial = B.poseS + B.K; D.fidx = A.dev(H.h_fidx);
    D.lmCur = B.lmS; D.lmTrial = B.lmS + (size_t)3 * B.L; D.edges = A.dev(H.h_edges);
    D.S = B.S; D.rhs = B.S + (size_t)n * n; D.Sedge = B.Sedge; D.dP = B.dP; D.dL = B.dL; D.sums = B.sums; D.flags = B.flags;
    D.fx = rig.fx; D.fy = rig.fy; D.cx = rig.cx; D.cy = rig.cy; D.b = (double)rig.baseline;
    D.ctl = A.dev(H.h_ctl);
    D.NB = NB; D.specLin = specLin ? 1 : 0; D.adaptive = adaptive ? 1 : 0;
    D.poseBase = B.poseS; D.lmBase = B.lmS; D.lmStride = (size_t)3 * B.L;
    D.facJBase = B.facJ; D.facJStride = (size_t)20 * H.NF; D.SedgeBase = B.Sedge; D.edgesBase = A.dev(H.h_edges);
    D.sysStride = (size_t)n * n + 2 * n + 8; D.dLStride = (size_t)3 * H.Lp;
}
// chi2 arguments: the problem's pair arrays, the pass's membership arrays, thresholds 7.815 * sigmaFactor, the rig
static void ba_fill_chi(BaChi& C, const vslam_ba_problem* P, const BaPairArrays& a, const uint8_t* kfPresent, const uint8_t* lmPresent, uint8_t* wrong) {
    C.NP = P->n_pairs; C.pairKf = a.kf; C.pairLm = a.lm; C.pairFlags = a.flags; C.pairUv = a.uv;
    C.pairOct = a.oct; C.kfLocal = a.kfLocal; C.kfPresent = kfPresent; C.lmPresent = lmPresent; C.wrong = wrong;
    for (int l = 0; l < P->n_levels; l++) C.thr[l] = (float)((double)7.815f * (double)P->sigma_factor[l]);
    C.fx = P->rig.fx; C.fy = P->rig.fy; C.cx = P->rig.cx; C.cy = P->rig.cy; C.b = (double)P->rig.baseline;
}

// ---- the calling thread's local-BA state ------------------------------------------------------------------------------------------
// Grow-only device workspace + stream of vslam_local_ba, kept per host thread across calls (one local BA per keyframe:
// re-allocating ~40 buffers every call cost more than the solve itself).
struct BaSingleBufs {
    DevBuf<DPose> d_poseS;
    DevBuf<double> d_lmS, d_facJ, d_S, d_Spart, d_Sedge, d_dP, d_dL, d_lmDiff, d_sums, d_partial, d_Lg, d_cholY, d_winW, d_winH;
    DevBuf<int> d_flags, d_win, d_cholFail;
    DevBuf<uint8_t> d_wrong;
    DevBuf<uint8_t> d_const; PinBuf h_const;      // the call's constant inputs, one block, and its pinned staging block
    PinBuf h_wrong;                                // landing area of the chi2 flags
    PinBuf h_out;                                  // pinned landing area of the result (poses | landmarks)
    PinBuf h_ctlOut;                               // read-back of the LM control block
    void release_buffers() {
        release_bufs<sizeof(BaSingleBufs) / sizeof(PinBuf)>(d_poseS, d_lmS, d_facJ, d_S, d_Spart, d_Sedge, d_dP, d_dL, d_lmDiff, d_sums, d_partial, d_Lg, d_cholY,
                                                           d_winW, d_winH, d_flags, d_win, d_cholFail, d_wrong, d_const, h_const, h_wrong, h_out, h_ctlOut);
    }
};
struct BaSingleWs : BaSingleBufs {
    hipStream_t stream = nullptr;
    int device = -1;
    PinnedArena arena;
    BaHostTmp tmp;
    BaPool pool;
    vslam_status open(int dev) {
        device = dev;
        VS_HIP(vslam::create_side_stream(&stream));
        VS_HIP(h_ctlOut.ensure(CTL_DOUBLES * sizeof(double), GrowPlus{0}));
        int nt = 7;      // + the calling thread; VSLAM_BA_HOST_THREADS overrides (0 = none).  (C5-size problems: 52 -> 43 ms per BA with 4 threads, 35 with 8)
        if (const char* e = getenv("VSLAM_BA_HOST_THREADS")) nt = std::max(0, std::min(15, atoi(e)));
        pool.start(nt);
        return VSLAM_OK;
    }
    void release() {      // (the owner has made `device` current)
        if (stream) { hipStreamSynchronize(stream); hipStreamDestroy(stream); stream = nullptr; }
        release_buffers();
        arena.release();
    }
};
// The same for vslam_local_ba_batch: its own stream, one device block, one landing area.
struct BaBatchWs {
    hipStream_t stream = nullptr;
    int device = -1;
    PinnedArena arena;
    DevBuf<uint8_t> d_mem;
    PinBuf h_back;        // pinned landing area: control blocks | chi2 flags | results
    BaPool pool;
    vslam_status open(int dev) {
        device = dev;
        VS_HIP(vslam::create_side_stream(&stream));
        pool.start(2);
        return VSLAM_OK;
    }
    void release() {
        if (stream) { hipStreamSynchronize(stream); hipStreamDestroy(stream); stream = nullptr; }
        d_mem.release(); h_back.release();
        arena.release();
    }
};
// One owner for both workspaces, the device ordering's buffers (on the single workspace's device) and the timer's events.  A
// workspace is created on the first use of its entry point and again when `device` changes.  Nothing here frees from a destructor
// (no HIP calls from a thread_local destructor: see DevPool): a short-lived optimizer thread that must not leak its streams, pinned
// buffers and device memory calls vslam_thread_release(); what is left at thread exit (the pools' threads aside, which are joined)
// is reclaimed with the process.
struct BaThread {
    std::unique_ptr<BaSingleWs> single;
    std::unique_ptr<BaBatchWs> batch;
    BaDeviceOrder order;
    vslam_status single_ws(int device, BaSingleWs** out) { return get(single, device, out); }
    vslam_status batch_ws(int device, BaBatchWs** out) { return get(batch, device, out); }
    void release() {
        drop(single);
        drop(batch);
        g_baTimer.destroy();
    }

private:
    template <class W>
    vslam_status get(std::unique_ptr<W>& w, int device, W** out) {
        if (!w || w->device != device) {
            drop(w);
            w.reset(new W());
            const vslam_status st = w->open(device);
            if (st != VSLAM_OK) { drop(w); return st; }      // (no half-opened workspace for the next call to find)
        }
        *out = w.get();
        return VSLAM_OK;
    }
    template <class W>
    void drop(std::unique_ptr<W>& w) {
        if (!w) return;
        const bool own = std::is_same<W, BaSingleWs>::value;      // the ordering's buffers go with the single workspace
        if (w->device >= 0 && hipSetDevice(w->device) == hipSuccess) {
            w->release();
            if (own) order.release();
        }
        if (own) order = BaDeviceOrder{};
        w.reset();
    }
};
thread_local std::unique_ptr<BaThread> g_baThread;
static BaThread& ba_thread() {
    if (!g_baThread) g_baThread.reset(new BaThread());
    return *g_baThread;
}
// frees the calling thread's local-BA state (vslam::thread_release)
static void ba_thread_release() {
    if (g_baThread) { g_baThread->release(); g_baThread.reset(); }
}

}  // namespace

void vslam::thread_release() {
    ba_thread_release();
    thread_pool_release();
}

// ---- host sections: where the wall time of the two entry points goes ------------------------------------------------------------------
static std::atomic<long long> g_bbsNs[12], g_bbsCalls{0}, g_bbsPolls{0};
static const char* g_bbsName[12] = {"check+count", "arena fill", "tables+upload", "lm pass 1", "chi2 1", "second-pass prep", "lm pass 2", "chi2 2 + fetch", "results", nullptr, nullptr, nullptr};

// The section marks of ba_run, one object in two forms; VSLAM_HOST_STAMPS (tools/stampbuild.sh) chooses here, once.
//   fine(name)          a mark only the accumulating form keeps
//   begin_sections(s)   the call's constants are on their way; the sections below are timed on stream s
//   section(name)       the end of a section
#ifdef VSLAM_HOST_STAMPS
// the stamp build: every section mark synchronises the stream and prints the time since the mark before
static double bhs_now() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
struct BaMarks {
    const double entry = bhs_now();
    double t = 0;
    hipStream_t stream = nullptr;
    void fine(const char*) {}
    void begin_sections(hipStream_t s) { stream = s; t = entry; section("entry..const"); }
    void section(const char* name) {
        hipStreamSynchronize(stream);
        const double t_ = bhs_now();
        fprintf(stderr, "  ba host: %-12s %8.1f us\n", name, t_ - t);
        t = t_;
    }
    static void print() {}
};
#else
// cumulative wall time between the marks (no synchronisation added): the VSLAM_BATCH_PHASES diagnostics
static std::atomic<long long> g_bhsNs[20], g_bhsCalls{0};
static const char* const g_bhsName[20] = {"s_check", "s_ws", "s_alloc", "s_const", "setup", "count", "fill", "prep", "u_arena", "u_alloc", "u_attr", "upload",
                                          "lm", "p2stats", "chi2", "fetch", nullptr, nullptr, nullptr, nullptr};
static int bhs_slot(const char* name) { for (int i = 0; i < 20 && g_bhsName[i]; i++) if (!strcmp(g_bhsName[i], name)) return i; return 19; }      // 19: "other"
struct BaMarks {
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    BaMarks() { g_bhsCalls++; }
    void fine(const char* name) { section(name); }
    void begin_sections(hipStream_t) {}
    void section(const char* name) {
        const auto t_ = std::chrono::steady_clock::now();
        g_bhsNs[bhs_slot(name)] += std::chrono::duration_cast<std::chrono::nanoseconds>(t_ - t).count();
        t = t_;
    }
    // averages per call; the marks do not synchronise, so "lm" holds the polls of both LM loops, "chi2" the re-check + second-pass
    // preparation + result fetch
    static void print() {
        if (const long long nb = g_bbsCalls.load()) {
            fprintf(stderr, "  vslam_local_ba_batch host sections (us per cohort, %lld cohorts, %.1f polls each):", nb, (double)g_bbsPolls.load() / (double)nb);
            for (int i = 0; i < 12 && g_bbsName[i]; i++) fprintf(stderr, " %s %.1f |", g_bbsName[i], 1e-3 * (double)g_bbsNs[i].load() / (double)nb);
            fprintf(stderr, "\n");
        }
        const long long n = g_bhsCalls.load();
        if (!n) return;
        fprintf(stderr, "  vslam_local_ba host sections (us per call, %lld calls):", n);
        for (int i = 0; i < 20; i++) if (g_bhsName[i] || g_bhsNs[i].load()) fprintf(stderr, " %s %.1f |", g_bhsName[i] ? g_bhsName[i] : "other", 1e-3 * (double)g_bhsNs[i].load() / (double)n);
        fprintf(stderr, "\n");
    }
};
#endif

// hipFuncSetAttribute is PROCESS-global state: set once, to the largest dynamic LDS size any call may ask for (a per-call,
// problem-dependent value written by several mapping threads while others launch the same kernel is a race on the runtime's
// function record).  The launch's own dynamic size is what a workgroup actually gets.
static vslam_status ba_kernel_attributes() {
    static std::once_flag once;
    static hipError_t err = hipSuccess;
    static bool reserveOk = true;
    std::call_once(once, [] {
        const int cap = BA_LDS_BYTES;
        const void* fns[] = {(const void*)k_ba_schur, (const void*)k_ba_schur_win, (const void*)k_ba_solve, (const void*)k_ba_back,
                             (const void*)k_ba_solve_mfma, (const void*)k_ba_chol_col, (const void*)k_ba_chol_back, (const void*)k_ba_lm_prep,
                             (const void*)k_ba_schur2, (const void*)k_ba_schur2_rm, (const void*)k_ba_back2};
        const void* batchFns[] = {(const void*)k_ba_schur, (const void*)k_ba_schur2, (const void*)k_ba_schur2_rm, (const void*)k_ba_back, (const void*)k_ba_back2, (const void*)k_ba_solve_mfma};
        for (const void* f : fns) {
            hipFuncAttributes fa{};      // (the limit is on static + dynamic LDS together)
            hipError_t e = hipFuncGetAttributes(&fa, f);
            if (e == hipSuccess) e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, cap - (int)fa.sharedSizeBytes);
            if (e != hipSuccess && err == hipSuccess) err = e;
            for (const void* b : batchFns) if (b == f && e == hipSuccess && fa.sharedSizeBytes > (size_t)BA_STATIC_LDS_RESERVE) reserveOk = false;
        }
    });
    if (err != hipSuccess) { set_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize): %s", hipGetErrorString(err)); return VSLAM_ERR_HIP; }
    if (!reserveOk) { set_error("local BA: a batch kernel's static LDS exceeds BA_STATIC_LDS_RESERVE"); return VSLAM_ERR_CAPACITY; }
    return VSLAM_OK;
}

namespace {

// ---- one vslam_local_ba call: what its stages share, and the stages in the order run() calls them ---------------------------------
struct BaCall {
    const vslam_ba_problem* const P;
    vslam_ba_result* const R;
    const vslam_comm* const comm;
    BaSingleWs& ws;
    BaDeviceOrder& ord;
    BaMarks& marks;
    PinnedArena& A;
    const hipStream_t stream;
    const int rank, world, K, L, NP;
    // (the landmark-sharded path runs the same look-ahead scheme: every rank evaluates the same candidates, the NB partial systems
    // travel in one all-reduce, the control step walks them identically on every rank)
    const int NB, nSlots;
    const bool specLin;
    static constexpr double relTol = 1e-5, absTol = 1e-5;
    std::vector<DPose> pose0;
    std::vector<uint8_t> wrong;           // chi2 flags of the pass before (host copy)
    // the call's constants in the device block
    DPose* p_pose0 = nullptr;
    double* p_lm0 = nullptr;
    BaPairArrays pairs{};
    // the values of the last pass on the device, and the pinned landing area of the result
    DPose* poseFinal = nullptr;
    double* lmFinal = nullptr;
    DPose* poseOut = nullptr;
    double* lmOut = nullptr;
    bool resultFetched = false;
    // one pass: its ordering, launch plan and argument block
    struct Pass {
        BaPassHost H;
        bool devOrder = false, adaptive = false;
        BaSinglePlan plan;
        BaDev D{};                        // host copy of the argument block; poseCur / lmCur: the pass's final values once it is done
        const BaDev* dD = nullptr;
        BaWin Wn{};
        int nWinWg = 0;
    } q;

    BaCall(const vslam_ba_problem* P_, vslam_ba_result* R_, const vslam_comm* comm_, BaSingleWs& ws_, BaDeviceOrder& ord_, BaMarks& marks_)
        : P(P_), R(R_), comm(comm_), ws(ws_), ord(ord_), marks(marks_), A(ws_.arena), stream(ws_.stream), rank(comm_ ? comm_->rank : 0), world(comm_ ? comm_->world : 1),
          K(P_->n_kf), L(P_->n_lm), NP(P_->n_pairs), NB(ba_lm_knobs().NB), nSlots(NB + 1), specLin(ba_lm_knobs().specLin), pose0(P_->n_kf), wrong(P_->n_pairs, 0) {
        for (int k = 0; k < K; k++) pose_from_rm16(P->kf_pose_wc + 16 * (size_t)k, pose0[k]);
    }
    int edge_slots() const { return specLin ? nSlots : 1; }

    vslam_status run() {
        VS_CHECK(constants());
        marks.begin_sections(stream);
        marks.section("setup");
        for (int pass = 0; pass < 2; pass++) {
            q = Pass{};
            VS_CHECK(order(pass));
            VS_CHECK(arm_and_upload(pass));
            VS_CHECK(plan_and_buffers());
            if (!q.plan.ldsS) VS_CHECK(window_lists());
            VS_CHECK(argument_block());
            VS_CHECK(run_lm(pass, q.H.NF, q.H.Lp, q.H.sumK2));
            bool done = false;
            if (pass == 0) VS_CHECK(masked_second_pass(&done));
            if (done) break;
        }
        return result();
    }

    // ---- the call's constant inputs (initial poses / landmarks, the pair arrays, kf_local) travel in ONE copy through a pinned
    // staging block into one device block (they used to be eight pageable copies)
    vslam_status constants() {
        VS_HIP(ws.d_poseS.alloc((size_t)nSlots * K));
        VS_HIP(ws.d_lmS.alloc((size_t)nSlots * 3 * L));
        VS_HIP(ws.d_wrong.alloc(NP));
        marks.fine("s_alloc");
        size_t cBytes = 0;
        auto cOff = [&](size_t bytes) { const size_t at = cBytes; cBytes = (cBytes + std::max<size_t>(bytes, 8) + 255) & ~(size_t)255; return at; };
        const size_t oPose0 = cOff((size_t)K * sizeof(DPose)), oLm0 = cOff((size_t)3 * L * sizeof(double)), oPairKf = cOff((size_t)NP * 4),
                     oPairLm = cOff((size_t)NP * 4), oPairOct = cOff((size_t)2 * NP * 4), oPairFlags = cOff((size_t)NP), oPairUv = cOff((size_t)4 * NP * 4),
                     oKfLocal = cOff((size_t)K);
        // small problems (a tracker's local window): through the pinned block, one copy.  Large ones (the 100 k-landmark window:
        // 40 MB of pair arrays): straight from the caller's arrays - staging them would cost a host memcpy of the same size.
        const bool staged = cBytes <= ((size_t)8 << 20);
        if (ws.d_const.n < cBytes) VS_HIP(ws.d_const.alloc(cBytes));     // (DevBuf adds its own headroom)
        if (staged) VS_HIP(ws.h_const.ensure(cBytes, grow_block(), [&] { return hipStreamSynchronize(stream); }));
        uint8_t* const h = staged ? ws.h_const.p : nullptr;
        uint8_t* const dc = ws.d_const.p;
        auto put = [&](size_t at, const void* src, size_t bytes) -> hipError_t {
            if (!bytes) return hipSuccess;
            if (h) { memcpy(h + at, src, bytes); return hipSuccess; }
            return hipMemcpyAsync(dc + at, src, bytes, hipMemcpyHostToDevice, stream);
        };
        VS_HIP(put(oPose0, pose0.data(), (size_t)K * sizeof(DPose)));
        VS_HIP(put(oLm0, P->lm_xyz, (size_t)3 * L * sizeof(double)));
        VS_HIP(put(oPairKf, P->pair_kf, (size_t)NP * 4)); VS_HIP(put(oPairLm, P->pair_lm, (size_t)NP * 4));
        VS_HIP(put(oPairOct, P->pair_octave, (size_t)2 * NP * 4)); VS_HIP(put(oPairFlags, P->pair_flags, (size_t)NP));
        VS_HIP(put(oPairUv, P->pair_uv, (size_t)4 * NP * 4));
        VS_HIP(put(oKfLocal, P->kf_local, (size_t)K));
        if (h) VS_HIP(hipMemcpyAsync(dc, h, cBytes, hipMemcpyHostToDevice, stream));
        marks.fine("s_const");
        p_pose0 = (DPose*)(dc + oPose0);
        p_lm0 = (double*)(dc + oLm0);
        pairs = BaPairArrays{(const int*)(dc + oPairKf), (const int*)(dc + oPairLm), (const int*)(dc + oPairOct), dc + oPairFlags, (const float*)(dc + oPairUv), dc + oKfLocal};
        VS_HIP(ws.d_sums.alloc(32));
        if (!ws.d_flags.p) { VS_HIP(ws.d_flags.alloc(16)); VS_HIP(hipMemsetAsync(ws.d_flags.p, 0, 16 * sizeof(int), stream)); }
        poseFinal = p_pose0;
        lmFinal = p_lm0;
        // pinned landing area of the result (see result())
        poseOut = (DPose*)ws.h_out.p;
        lmOut = (double*)(ws.h_out.p + (((size_t)K * sizeof(DPose) + 63) & ~(size_t)63));
        return VSLAM_OK;
    }

    // ---- factor list of this pass, ordered by (landmark, free index, pair, side) -------------------------------------------------
    // Everything the kernels read is written straight into ONE pinned arena and uploaded with one copy.
    // Large problems order their factors ON THE DEVICE (BaDeviceOrder: the raw pair arrays are there for the chi2 kernel anyway); the
    // host keeps the free set and the BetweenFactor chain.  VSLAM_BA_DEVICE_ORDER = 0: host ordering always, 2: device ordering for
    // every size (tests; read at every pass).
    vslam_status order(int pass) {
        BaPassHost& H = q.H;
        const int ordEnv = getenv("VSLAM_BA_DEVICE_ORDER") ? atoi(getenv("VSLAM_BA_DEVICE_ORDER")) : 1;
        q.devOrder = NP > 0 && L > 0 && (ordEnv == 2 || (ordEnv == 1 && NP >= 200000));
        if (q.devOrder) VS_CHECK(ord.count(P, pairs, ws.d_wrong.p, pass, rank, world, stream, H, ws.tmp));
        else H.count(P, wrong.data(), rank, world, ws.tmp, &ws.pool);
        marks.section("count");
        if (H.F > BA_MAX_FREE_KF) { set_error("local BA: more than 170 free keyframes is not supported"); return VSLAM_ERR_CAPACITY; }      // (before anything is sized by F)
        VS_HIP(A.ensure(H.arena_bytes(K, L, edge_slots()), stream));
        A.reset();
        if (!H.take(A, K, L, edge_slots())) { set_error("local BA: upload arena too small"); return VSLAM_ERR_CAPACITY; }
        if (q.devOrder) VS_CHECK(ord.emit(P, pose0.data(), edge_slots(), A, stream, H, ws.tmp));
        else H.fill(P, wrong.data(), rank, world, ws.tmp, pose0.data(), &ws.pool, edge_slots());
        marks.section("fill");
        return VSLAM_OK;
    }

    // ---- LM control block (GTSAM 4.2 policy; k_ba_ctl) ----------------------------------------------------------------------------
    void arm_ctl(int ps) { ba_init_ctl(q.H.h_ctl, ps, q.adaptive ? 1 : NB); }
    vslam_status arm_and_upload(int pass) {
        const BaPassHost& H = q.H;
        // adaptive look-ahead for large problems (every candidate costs a full Schur / back-substitution / evaluation pass)
        const int adaptEnv = ba_adaptive_env();
        q.adaptive = NB > 1 && (adaptEnv >= 0 ? adaptEnv != 0 : H.NF > 200000);
        arm_ctl(pass);
        // The arena is complete except for the kernels' argument block (h_D, written after the launch geometry): its upload
        // starts now and runs under the host work that follows (the window lists of a large problem); h_D follows as a copy of its own.
        // (Device ordering: the factor arrays were written in place on the device; only the host-written small pieces travel.)
        if (q.devOrder) {
            VS_HIP(hipMemcpyAsync(A.dev(H.h_ctl), H.h_ctl, CTL_DOUBLES * sizeof(double), hipMemcpyHostToDevice, stream));
            VS_HIP(hipMemcpyAsync(A.dev(H.h_kfPresent), H.h_kfPresent, (size_t)K, hipMemcpyHostToDevice, stream));
            if (H.NE > 0) VS_HIP(hipMemcpyAsync(A.dev(H.h_edges), H.h_edges, (size_t)edge_slots() * H.NE * sizeof(BaEdge), hipMemcpyHostToDevice, stream));
        } else VS_HIP(A.upload(stream));
        marks.section("prep");
        return VSLAM_OK;
    }

    void init_slots() {      // every value slot starts from the caller's values
        const int nPose = K * (int)(sizeof(DPose) / sizeof(double)), nLm = 3 * L;
        hipLaunchKernelGGL(k_ba_init_slots, dim3((std::max(nPose, nLm) + 255) / 256, nSlots), dim3(256), 0, stream,
                           nPose, (const double*)p_pose0, (double*)ws.d_poseS.p, nLm, p_lm0, ws.d_lmS.p);
    }
    // ---- device buffers sized by the pass, the argument block's common part, the launch geometry -------------------------------
    vslam_status plan_and_buffers() {
        const BaPassHost& H = q.H;
        const int n = H.n, NF = H.NF;
        const size_t sysStride = (size_t)n * n + 2 * n + 8, seDoubles = (size_t)n * n + n;
        VS_HIP(ws.d_facJ.alloc((size_t)20 * NF * edge_slots()));
        VS_HIP(ws.d_dP.alloc((size_t)NB * n)); VS_HIP(ws.d_dL.alloc((size_t)NB * 3 * H.Lp));
        VS_HIP(ws.d_S.alloc(sysStride * NB));         // per candidate: S | rhs | scratch contiguous (one all-reduce buffer)
        VS_HIP(ws.d_Sedge.alloc(seDoubles * edge_slots()));
        init_slots();
        ba_fill_dev(q.D, H, A, BaLaneBufs{K, L, ws.d_poseS.p, ws.d_lmS.p, ws.d_facJ.p, ws.d_S.p, ws.d_Sedge.p, ws.d_dP.p, ws.d_dL.p, ws.d_sums.p, ws.d_flags.p},
                    P->rig, NB, specLin, q.adaptive);
        // launch geometry (ba_plan.hpp); the environment caps the waves per workgroup of the landmark kernels
        static const BaSingleKnobs envKnobs = {getenv("VSLAM_BA_SCHUR_WAVES") ? std::max(2, std::min(BA_SCHUR_WAVES, atoi(getenv("VSLAM_BA_SCHUR_WAVES")))) : BA_SCHUR_WAVES,
                                               getenv("VSLAM_BA_BACK_WAVES") ? std::max(1, atoi(getenv("VSLAM_BA_BACK_WAVES"))) : 64, 0, !getenv("VSLAM_BA_NO_SHARED_W")};
        BaSingleKnobs knobs = envKnobs;
        if (const char* e = getenv("VSLAM_BA_WINDOW_TB")) knobs.windowTB = std::max(1, std::min(32, atoi(e)));
        q.plan = ba_single_plan(BaSingleShape{NF, H.Lp, H.F, H.NE, H.maxSlots, NB, ba_use_mfma(), q.devOrder}, knobs);
        if (q.plan.why) { set_error("%s", q.plan.why); return VSLAM_ERR_CAPACITY; }
        return VSLAM_OK;
    }

    // ---- windowed accumulation: tile, work lists (host ordering: ba_window_lists_host alone; device ordering: counts and fill by k_win_*)
    vslam_status window_lists() {
        const BaPassHost& H = q.H;
        const BaSinglePlan& plan = q.plan;
        BaWin& Wn = q.Wn;
        const int TB = plan.win.TB, nBR = plan.win.nBR, nWin = plan.win.nWin, n = H.n, Lp = H.Lp;
        Wn.TB = TB; Wn.T = plan.win.T; Wn.TP = plan.win.TP; Wn.tileDoubles = plan.win.tileDoubles; Wn.nWin = nWin;
        const int* devWinCnt = nullptr;
        if (q.devOrder) VS_CHECK(ord.window_counts(H, A, TB, nBR, nWin, stream, &devWinCnt));
        const BaWinLists WL = ba_window_lists_host(Lp, H.h_lpSlotStart, H.h_slotFi, TB, nBR, &ws.pool, BA_NCU, devWinCnt);
        const int nWinWg = q.nWinWg = WL.nWinWg;
        VS_HIP(ws.d_win.alloc(WL.nInts));
        int* const dw = ws.d_win.p;
        VS_HIP(hipMemcpyAsync(dw, WL.pack.data(), WL.pack.size() * sizeof(int), hipMemcpyHostToDevice, stream));
        if (q.devOrder) VS_CHECK(ord.window_fill(dw + WL.oWg + 3 * (size_t)std::max(nWinWg, 1), WL.total, stream));
        VS_HIP(hipStreamSynchronize(stream));          // (WL.pack is a local: the copy must have left it)
        Wn.winA = dw; Wn.winB = dw + nWin; Wn.winFirstWg = dw + 2 * nWin;
        Wn.wgWin = dw + WL.oWg; Wn.wgBegin = Wn.wgWin + std::max(nWinWg, 1); Wn.wgEnd = Wn.wgBegin + std::max(nWinWg, 1);
        Wn.winLm = Wn.wgEnd + std::max(nWinWg, 1);
        VS_HIP(ws.d_Spart.alloc((size_t)std::max(nWinWg, 1) * NB * Wn.tileDoubles));
        Wn.part = ws.d_Spart.p;
        VS_HIP(ws.d_winW.alloc((size_t)std::max(H.nSlotEntries, 1) * 18)); VS_HIP(ws.d_winH.alloc((size_t)std::max(Lp, 1) * BA_WIN_HG));
        Wn.Wg = ws.d_winW.p; Wn.Hg = ws.d_winH.p;
        // the lower block triangle is never written (nor read by a solver): keep it at zero for the all-reduce
        VS_HIP(hipMemsetAsync(ws.d_S.p, 0, ((size_t)n * n + 2 * n + 8) * NB * sizeof(double), stream));
        return VSLAM_OK;
    }

    // ---- what the plan adds to the argument block, then its upload ------------------------------------------------------------
    vslam_status argument_block() {
        const BaPassHost& H = q.H;
        const BaSinglePlan& plan = q.plan;
        BaDev& D = q.D;
        const size_t sysDoubles = (size_t)H.n * H.n + H.n;
        D.partialStride = (size_t)2 * plan.obsBlocks + 2 * (size_t)std::max(H.NE, 1);
        VS_HIP(ws.d_partial.alloc(D.partialStride * NB));
        D.partial = ws.d_partial.p;
        D.spartStride = sysDoubles * plan.lmBlocks;
        if (plan.ldsS) { VS_HIP(ws.d_Spart.alloc(D.spartStride * NB)); D.Spart = ws.d_Spart.p; }
        marks.fine("u_alloc");
        VS_CHECK(ba_kernel_attributes());
        if (plan.solveKind == BA_SOLVE_MFMA) VS_HIP(ws.d_Lg.alloc((size_t)BA_MFMA_N * BA_MFMA_N * NB));
        // larger systems: block-column MFMA Cholesky (k_ba_chol_col / k_ba_chol_back)
        if (plan.useChol) {
            VS_HIP(ws.d_Lg.alloc((size_t)plan.cholN * plan.cholN * NB));
            VS_HIP(ws.d_cholY.alloc((size_t)plan.cholN * NB));
            if (!ws.d_cholFail.p) { VS_HIP(ws.d_cholFail.alloc(BA_MAX_NB)); VS_HIP(hipMemsetAsync(ws.d_cholFail.p, 0, BA_MAX_NB * sizeof(int), stream)); }
        }
        marks.fine("u_attr");
        D.solveKind = plan.solveKind;
        *H.h_D = D;
        q.dD = A.dev(H.h_D);
        VS_HIP(hipMemcpyAsync((void*)q.dD, H.h_D, sizeof(BaDev), hipMemcpyHostToDevice, stream));
        marks.section("upload");
        return VSLAM_OK;
    }

    // ---- LM: speculative steps, the device decides (k_ba_ctl) ------------------------------------------------------------------
    // One step = [linearise if the state asks for it] + one lambda trial.  Kernels that are not due
    // return at once, so the host may enqueue a few steps ahead and only then look at the state.
    vslam_status lm_step(bool first) {
        const BaPassHost& H = q.H;
        const BaSinglePlan& plan = q.plan;
        const BaDev* const dD = q.dD;
        const BaWin& Wn = q.Wn;
        const int n = H.n, NF = H.NF, NE = H.NE, Lp = H.Lp, maxSlots = H.maxSlots, nWinWg = q.nWinWg, nCU = BA_NCU;
        const size_t sysStride = (size_t)n * n + 2 * n + 8, sysDoubles = (size_t)n * n + n;
        const bool ldsS = plan.ldsS;
        const int fuseCtl = comm ? 0 : 1;
        const int facBlocks = (NF ? plan.obsBlocks : 0) + std::max(NE, 1);
        const int nObs = NF ? plan.obsBlocks : 0;
        int t = -1;
        // with speculative linearisation only the first step of a pass linearises on its own
        if (first || !specLin) {
            t = g_baTimer.begin("ba_linearize");
            hipLaunchKernelGGL(k_ba_factors<0>, dim3(facBlocks), dim3(256), 0, stream, dD, nObs, fuseCtl, relTol, absTol);
            g_baTimer.end(t);
        }
        if (comm) {
            const int tc = g_baTimer.begin("ba_allreduce"); VS_CHECK(comm_allreduce(comm, ws.d_sums.p, 1, stream)); g_baTimer.end(tc);
            hipLaunchKernelGGL(k_ba_ctl, dim3(1), dim3(256), 0, stream, dD, 0, relTol, absTol);
        }
        t = g_baTimer.begin("ba_schur");
        if (n > 0) {
            if (ldsS) hipLaunchKernelGGL(k_ba_schur, dim3(plan.lmBlocks, plan.sharedW ? 1 : NB), dim3(64 * plan.schurWaves), plan.schurLds, stream, dD, maxSlots, plan.sharedW);
            else if (nWinWg) {
                hipLaunchKernelGGL(k_ba_lm_prep, dim3(std::max(1, std::min((Lp + BA_SCHUR_WAVES - 1) / BA_SCHUR_WAVES, 4 * nCU))), dim3(64 * BA_SCHUR_WAVES),
                                   (size_t)BA_SCHUR_WAVES * maxSlots * sizeof(int), stream, dD, Wn, maxSlots);
                hipLaunchKernelGGL(k_ba_schur_win, dim3(nWinWg), dim3(64 * plan.schurWaves), plan.schurLds, stream, dD, Wn);
            }
        }
        g_baTimer.end(t);
        t = g_baTimer.begin("ba_solve");
        if (n > 0) {     // sum of the partial systems + BetweenFactor blocks
            if (ldsS) hipLaunchKernelGGL(k_ba_reduce, dim3(((int)sysDoubles + 31) / 32, NB), dim3(256), 0, stream, dD, plan.lmBlocks, 0);
            else hipLaunchKernelGGL(k_ba_reduce_win, dim3(Wn.nWin, NB), dim3(256), 0, stream, dD, Wn);
        }
        // the NB candidates' systems are contiguous (sysStride apart): one all-reduce for all of them
        if (comm && n > 0) { const int tc = g_baTimer.begin("ba_allreduce"); VS_CHECK(comm_allreduce(comm, ws.d_S.p, sysStride * (NB - 1) + (size_t)n * n + n, stream)); g_baTimer.end(tc); }
        if (q.D.solveKind == BA_SOLVE_MFMA64) hipLaunchKernelGGL(k_ba_solve_mfma64, dim3(NB), dim3(64), 0, stream, dD);
        else if (q.D.solveKind == BA_SOLVE_WAVE) hipLaunchKernelGGL(k_ba_solve_wave, dim3(NB), dim3(64), 0, stream, dD);
        else if (q.D.solveKind == BA_SOLVE_MFMA) hipLaunchKernelGGL(k_ba_solve_mfma, dim3(NB), dim3(64 * BA_MFMA_NW), plan.mfmaLds, stream, dD, ws.d_Lg.p);
        else if (plan.useChol) {
            for (int J = 0; J < plan.cholN / CH_B; J++)
                hipLaunchKernelGGL(k_ba_chol_col, dim3(plan.cholN / CH_B - J, NB), dim3(256), plan.cholColLds, stream, dD, ws.d_Lg.p, ws.d_cholY.p, plan.cholN, J, ws.d_cholFail.p);
            hipLaunchKernelGGL(k_ba_chol_back, dim3(NB), dim3(256), plan.cholBackLds, stream, dD, (const double*)ws.d_Lg.p, (const double*)ws.d_cholY.p, plan.cholN, ws.d_cholFail.p);
        } else hipLaunchKernelGGL(k_ba_solve, dim3(NB), dim3(std::max(64, vslam::align_up(n, 64))),
                                plan.solveLds ? plan.solveLdsBytes : 64, stream, dD, plan.solveLds ? 1 : 0, plan.solveLds ? plan.ldA : n);
        g_baTimer.end(t);
        t = g_baTimer.begin("ba_back");
        if (Lp) hipLaunchKernelGGL(k_ba_back, dim3(plan.backBlocks, plan.sharedBack ? 1 : NB), dim3(64 * plan.backWaves), plan.backLds, stream, dD, maxSlots, plan.sharedBack);
        g_baTimer.end(t);
        t = g_baTimer.begin("ba_eval");
        hipLaunchKernelGGL(k_ba_factors<1>, dim3(facBlocks, NB), dim3(256), 0, stream, dD, nObs, fuseCtl, relTol, absTol);
        g_baTimer.end(t);
        if (comm) {
            const int tc = g_baTimer.begin("ba_allreduce"); VS_CHECK(comm_allreduce(comm, ws.d_sums.p + SUMS_CAND, (size_t)2 * NB, stream)); g_baTimer.end(tc);
            hipLaunchKernelGGL(k_ba_ctl, dim3(1), dim3(256), 0, stream, dD, 1, relTol, absTol);
        }
        VS_HIP(hipGetLastError());
        return VSLAM_OK;
    }
    // one pass of LM on the armed control block, its report (with the statistics of the graph it ran on), then the chi2 re-check
    vslam_status run_lm(int ps, long long nfStat, long long lpStat, long long k2Stat) {
        BaDev& D = q.D;
        const int n = q.H.n;
        VS_HIP(hipMemsetAsync(ws.d_Sedge.p, 0, ((size_t)n * n + n) * sizeof(double), stream));     // first linearisation; later ones: see k_ba_factors
        double* const h_ctlOut = (double*)ws.h_ctlOut.p;
        const int* co = (const int*)(h_ctlOut + CTL_INTS);
        int enq = 0;
        for (;;) {
            static const int perPoll = getenv("VSLAM_BA_STEPS_PER_POLL") ? std::max(1, atoi(getenv("VSLAM_BA_STEPS_PER_POLL"))) : 4;
            for (int b = 0; b < perPoll; b++) VS_CHECK(lm_step(enq + b == 0));
            enq += perPoll;
            VS_HIP(hipMemcpyAsync(h_ctlOut, D.ctl, CTL_DOUBLES * sizeof(double), hipMemcpyDeviceToHost, stream));
            VS_HIP(vslam::stream_wait_blocking(stream));
            if (co[CI_STATE] == BA_DONE) break;
            if (enq > 400) { set_error("local BA: LM did not terminate"); return VSLAM_ERR_INVALID; }
        }
        D.poseCur = ws.d_poseS.p + (size_t)co[CI_SEL] * K; D.lmCur = ws.d_lmS.p + (size_t)co[CI_SEL] * 3 * L;
        ba_write_report(R, ps, h_ctlOut, q.H.F, nfStat, lpStat, k2Stat);
        if (comm) VS_CHECK(exchange_shards(nfStat, lpStat, k2Stat));
        marks.section("lm");
        return chi2_and_fetch(ps);
    }
    // landmark shards: every rank needs all landmarks for the chi2 pass and the result - exchange the shard updates and the statistics
    vslam_status exchange_shards(long long nfStat, long long lpStat, long long k2Stat) {
        BaDev& D = q.D;
        const int tc = g_baTimer.begin("ba_allreduce");
        if (L) {
            VS_HIP(ws.d_lmDiff.alloc((size_t)3 * L));
            hipLaunchKernelGGL(k_ba_lm_diff, dim3((3 * L + 255) / 256), dim3(256), 0, stream, 3 * L, D.lmCur, p_lm0, ws.d_lmDiff.p, 0);
            VS_CHECK(comm_allreduce(comm, ws.d_lmDiff.p, (size_t)3 * L, stream));
            hipLaunchKernelGGL(k_ba_lm_apply, dim3((3 * L + 255) / 256), dim3(256), 0, stream, 3 * L, D.lmCur, p_lm0, ws.d_lmDiff.p);
        }
        double st[4] = {(double)nfStat, (double)lpStat, (double)k2Stat, 0.0};
        VS_HIP(hipMemcpyAsync(ws.d_sums.p + 4, st, sizeof(st), hipMemcpyHostToDevice, stream));
        VS_CHECK(comm_allreduce(comm, ws.d_sums.p + 4, 3, stream));
        VS_HIP(hipMemcpyAsync(st, ws.d_sums.p + 4, sizeof(st), hipMemcpyDeviceToHost, stream));
        VS_HIP(hipStreamSynchronize(stream));
        R->n_residuals = (int64_t)llround(st[0]); R->n_landmarks = (int64_t)llround(st[1]); R->sum_k2 = (int64_t)llround(st[2]);
        g_baTimer.end(tc);
        return VSLAM_OK;
    }
    // ---- chi2 re-check with the optimised values; the flags come back, and behind the last pass's flags its values --------------
    vslam_status chi2_and_fetch(int ps) {
        const BaPassHost& H = q.H;
        const BaDev& D = q.D;
        BaChi C{};
        ba_fill_chi(C, P, pairs, A.dev(H.h_kfPresent), A.dev(H.h_lmPresent), ws.d_wrong.p);
        C.pose = D.poseCur; C.lm = D.lmCur;
        const int t = g_baTimer.begin("ba_chi2");
        if (NP) hipLaunchKernelGGL(k_ba_chi2, dim3((NP + 255) / 256), dim3(256), 0, stream, C);
        g_baTimer.end(t);
        VS_HIP(hipGetLastError());
        if (NP) VS_HIP(hipMemcpyAsync(ws.h_wrong.p, ws.d_wrong.p, NP, hipMemcpyDeviceToHost, stream));
        if (ps == 1) {      // the second pass is the last one: its values ride behind the flags, one synchronisation for both
            VS_HIP(hipMemcpyAsync(poseOut, D.poseCur, K * sizeof(DPose), hipMemcpyDeviceToHost, stream));
            if (L) VS_HIP(hipMemcpyAsync(lmOut, D.lmCur, (size_t)3 * L * sizeof(double), hipMemcpyDeviceToHost, stream));
            resultFetched = true;
        }
        VS_HIP(hipStreamSynchronize(stream));
        if (NP) memcpy(wrong.data(), ws.h_wrong.p, NP);
        if (ps == 0 && R->pair_wrong_pass1 && NP) memcpy(R->pair_wrong_pass1, wrong.data(), NP);
        poseFinal = D.poseCur;
        lmFinal = D.lmCur;
        return VSLAM_OK;
    }

    // ---- second pass on the first pass's structure (single GPU): mask instead of rebuild ------------------------------------------
    // Membership / statistics of the second graph from the chi2 flags (large problems: by landmark range on the pool, as
    // BaPassHost::count - every worker reads all pairs and handles its range; with the device ordering: the same kernels again).
    // *done: the second pass has run here; otherwise the caller rebuilds the graph for it.
    vslam_status masked_second_pass(bool* done) {
        static const bool maskEnv = !getenv("VSLAM_BA_NO_MASK");
        if (!maskEnv || !g_baMask) return VSLAM_OK;
        const BaPassHost& H = q.H;
        BaSecondPass S2;
        if (q.devOrder) VS_CHECK(ord.second_pass(H.Lp, ws.tmp, stream, S2));
        else H.second_pass(P, wrong.data(), rank, world, ws.tmp, &ws.pool, S2);
        if (!S2.same) return VSLAM_OK;       // same keyframes => same free set, same BetweenFactor chain; landmarks may only drop out
        marks.section("p2stats");
        for (int k = 0; k < K; k++) H.h_kfPresent[k] = S2.kfP2[k];
        if (!q.devOrder) for (int l = 0; l < L; l++) H.h_lmPresent[l] = S2.lmP2[l];
        arm_ctl(1);
        VS_HIP(hipMemcpyAsync(A.dev(H.h_kfPresent), H.h_kfPresent, K, hipMemcpyHostToDevice, stream));
        if (q.devOrder) VS_HIP(hipMemcpyAsync(A.dev(H.h_lmPresent), ord.lm_present(), (size_t)L, hipMemcpyDeviceToDevice, stream));
        else if (L) VS_HIP(hipMemcpyAsync(A.dev(H.h_lmPresent), H.h_lmPresent, L, hipMemcpyHostToDevice, stream));
        VS_HIP(hipMemcpyAsync(A.dev(H.h_ctl), H.h_ctl, CTL_DOUBLES * sizeof(double), hipMemcpyHostToDevice, stream));
        if (H.NF) hipLaunchKernelGGL(k_ba_mask, dim3((H.NF + 255) / 256), dim3(256), 0, stream, H.NF, A.dev(H.h_facPair), ws.d_wrong.p, A.dev(H.h_facIs));
        init_slots();
        VS_CHECK(run_lm(1, S2.NF2, S2.Lp2, S2.k2));
        *done = true;
        return VSLAM_OK;
    }

    // ---- results land in pinned memory (a copy into the caller's pageable arrays is staged and synchronised by the runtime) ------
    vslam_status result() {
        marks.section("chi2");
        marks.section("fetch");
        if (!resultFetched) {
            VS_HIP(hipMemcpyAsync(poseOut, poseFinal, K * sizeof(DPose), hipMemcpyDeviceToHost, stream));
            if (L) VS_HIP(hipMemcpyAsync(lmOut, lmFinal, (size_t)3 * L * sizeof(double), hipMemcpyDeviceToHost, stream));
            VS_HIP(hipStreamSynchronize(stream));
        }
        ba_write_result(R, poseOut, lmOut, wrong.data(), K, L, NP);
        return VSLAM_OK;
    }
};

}  // namespace

static vslam_status ba_run(const vslam_ba_problem* P, vslam_ba_result* R, int device, const vslam_comm* comm) {
    BaMarks marks;
    if (!ba_check_args(P, R)) { set_error("vslam_local_ba: invalid problem"); return VSLAM_ERR_INVALID; }
    VS_CHECK(ba_select_device(device));
    // (the index check of a large problem - 1.2 M pairs: ~1 ms on one core - runs on the workspace's pool, below)
    const bool pooledCheck = P->n_pairs >= BaHostTune{}.parPairs;
    if (!pooledCheck && !ba_check_pairs(P)) { set_error("vslam_local_ba: pair index out of range"); return VSLAM_ERR_INVALID; }
    marks.fine("s_check");
    BaThread& th = ba_thread();
    BaSingleWs* ws = nullptr;
    VS_CHECK(th.single_ws(device, &ws));
    if (pooledCheck && !ba_check_pairs(P, &ws->pool)) { set_error("vslam_local_ba: pair index out of range"); return VSLAM_ERR_INVALID; }
    VS_HIP(ws->h_wrong.ensure((size_t)P->n_pairs, grow_wrong()));
    VS_HIP(ws->h_out.ensure((size_t)P->n_kf * sizeof(DPose) + 64 + (size_t)3 * P->n_lm * sizeof(double), grow_out()));
    marks.fine("s_ws");
    g_baTimer.reset();
    g_baTimer.stream = ws->stream;
    g_baTimer.multi = true;
    return BaCall(P, R, comm, *ws, th.order, marks).run();
}

// ---- batched local BA: N independent tracker-window problems, ONE launch per stage for all of them -------------------------------
// The local mapping of a lockstep group (batch.hip): the passes that become due at a step are optimised together.  Each problem
// ("lane") keeps its own argument block (BaDev, entry of a device table; grid z = lane), its own device-side LM control block
// and value slots, so the LM trajectories are exactly those of N one-problem calls; lanes that finish early leave every
// kernel at ba_enter.  Host work per pass: one upload, a poll of the N control blocks every few rounds, one download of the
// chi2 flags; the second pass is re-armed for all lanes together (mask, no rebuild).  Problems outside the tracker-window
// class (more than BA_LDS_MAX_F free keyframes, empty graphs) and lanes whose second graph loses a keyframe take the
// one-problem path.

// ---- launch plan of the batch: a pure function of the cohort's shape (no device calls; exported as vslam_local_ba_batch_plan) -----
static BaPlanKnobs ba_plan_knobs() {      // developer overrides from the environment (none set: the production plan)
    static const bool s2Env = !(getenv("VSLAM_BA_SCHUR2") && atoi(getenv("VSLAM_BA_SCHUR2")) == 0);
    static const bool b2Env = !(getenv("VSLAM_BA_BACK2") && atoi(getenv("VSLAM_BA_BACK2")) == 0);
    BaPlanKnobs k;
    k.schur2 = s2Env; k.back2 = b2Env;
    k.sharedW = getenv("VSLAM_BA_SCHUR_SHARED") ? atoi(getenv("VSLAM_BA_SCHUR_SHARED")) != 0 : true;
    k.schurWaves = getenv("VSLAM_BA_SCHUR_WAVES_B") ? atoi(getenv("VSLAM_BA_SCHUR_WAVES_B")) : 0;
    k.lmBlocks = getenv("VSLAM_BA_LMBLOCKS") ? atoi(getenv("VSLAM_BA_LMBLOCKS")) : 0;
    // (alone on the GPU 8 / 12 / 16 waves per workgroup take the same time; between the lockstep groups' wide kernels the smaller LDS footprint
    //  finds a CU sooner: 8 waves here, 4 for the back-substitution - ba_back 15.7 -> 10.6 us per tracked frame)
    k.s2Waves = getenv("VSLAM_BA_SCHUR2_WAVES") ? atoi(getenv("VSLAM_BA_SCHUR2_WAVES")) : 8;
    k.b2Waves = getenv("VSLAM_BA_BACK2_WAVES") ? atoi(getenv("VSLAM_BA_BACK2_WAVES")) : 4;
    // k_ba_schur2's LDS system: packed upper blocks; 0 / 1: the row-major forms (pitch n, n + 1) for comparison
    k.s2Layout = getenv("VSLAM_BA_SCHUR2_LAYOUT") ? std::max(0, std::min((int)BA2_PACKED, atoi(getenv("VSLAM_BA_SCHUR2_LAYOUT")))) : (int)BA2_PACKED;
    return k;
}
thread_local vslam_ba_batch_plan g_baLastPlan{};

static vslam_status ba_run_batch(const vslam_ba_problem* const* Ps, vslam_ba_result* const* Rs, int N, int device) {
    g_baLastPlan = vslam_ba_batch_plan{};
    if (N <= 0 || !Ps || !Rs) return VSLAM_ERR_INVALID;
    if (N == 1) { g_baLastPlan.n_single = 1; return ba_run(Ps[0], Rs[0], device, nullptr); }
    auto bbs_t = std::chrono::steady_clock::now();
    g_bbsCalls++;
    auto BBS = [&](int k) { const auto t_ = std::chrono::steady_clock::now(); g_bbsNs[k] += std::chrono::duration_cast<std::chrono::nanoseconds>(t_ - bbs_t).count(); bbs_t = t_; };
    VS_CHECK(ba_select_device(device));
    BaBatchWs* bws = nullptr;
    VS_CHECK(ba_thread().batch_ws(device, &bws));
    BaBatchWs& W = *bws;
    hipStream_t stream = W.stream;
    g_baTimer.reset(); g_baTimer.stream = stream; g_baTimer.multi = true;

    const int NB = ba_lm_knobs().NB, nSlots = NB + 1;
    const bool useMfma = ba_use_mfma();
    const double relTol = 1e-5, absTol = 1e-5;
    // adaptive look-ahead (BaDev::adaptive): a round evaluates ONE lambda candidate while steps are being accepted and all NB only
    // after a rejection - the same LM trajectory; in a batch the cost of a round is the candidates it evaluates (throughput, not latency)
    static const int adaptEnv = ba_adaptive_env();
    const bool adaptive = NB > 1 && (adaptEnv >= 0 ? adaptEnv != 0 : true);

    struct Lane {
        const vslam_ba_problem* P; vslam_ba_result* R; int K, L, NP;
        std::vector<DPose> pose0; BaHostTmp T; BaPassHost H; bool single = false, ownRig = false;
        std::vector<uint8_t> wrong;
        // constants of the call in the arena
        DPose* h_pose0; double* h_lm0; int *h_pairKf, *h_pairLm, *h_pairOct; uint8_t *h_pairFlags, *h_kfLocal; float* h_pairUv;
        // device slices
        DPose* d_poseS; double *d_lmS, *d_facJ, *d_dP, *d_dL, *d_S, *d_Sedge, *d_partial, *d_Spart, *d_sums, *d_Lg; int* d_flags; uint8_t* d_wrong;
        double *d_outPose, *d_outLm;
        size_t oWrong, oOut;          // offsets in the landing area
        BaSecondPass S2;
        bool pass2 = false;
    };
    std::vector<Lane> lanes(N);
    auto lane_shape = [](const Lane& q) {      // (max_slots / max_factors are known after the fill)
        vslam_ba_lane_shape s{};
        s.n_free_kf = q.H.F; s.n_points = q.H.Lp; s.n_factors = q.H.NF; s.n_edges = q.H.NE; s.n_pairs = q.NP;
        s.max_slots = q.H.maxSlots; s.max_factors = q.H.maxFac; s.own_rig = q.ownRig ? 1 : 0;
        return s;
    };
    std::vector<int> singles;
    for (int i = 0; i < N; i++) {
        Lane& q = lanes[i];
        const vslam_ba_problem* P = Ps[i]; vslam_ba_result* R = Rs[i];
        const int bad = ba_check_problem(P, R);
        if (bad == BA_PROBLEM_INVALID) { set_error("vslam_local_ba_batch: invalid problem %d", i); return VSLAM_ERR_INVALID; }
        if (bad) { set_error("vslam_local_ba_batch: pair index out of range (problem %d)", i); return VSLAM_ERR_INVALID; }
        q.P = P; q.R = R; q.K = P->n_kf; q.L = P->n_lm; q.NP = P->n_pairs;
        // (the rig is the lane's own - BaDev / BaChi2 carry fx, fy, cx, cy, b per lane, the host fill reads its own problem: the lanes of a
        //  fleet's cohort have different cameras and stay on the batched path; only another pyramid depth runs on its own)
        q.ownRig = P->n_levels != Ps[0]->n_levels;
        q.wrong.assign(std::max(q.NP, 1), 0);
        q.pose0.resize(q.K);
        for (int k = 0; k < q.K; k++) pose_from_rm16(P->kf_pose_wc + 16 * (size_t)k, q.pose0[k]);
    }
    // ---- host: count, arena layout, fill (lanes in parallel) -----------------------------------------------------------
    W.pool.run(N, [&](int i) {
        Lane& q = lanes[i];
        q.H.count(q.P, q.wrong.data(), 0, 1, q.T);
        q.single = ba_batch_single(lane_shape(q), useMfma);
    });
    std::vector<int> act;
    for (int i = 0; i < N; i++) (lanes[i].single ? singles : act).push_back(i);
    const int NL = (int)act.size();
    BBS(0);
    auto run_singles = [&]() -> vslam_status { for (int i : singles) VS_CHECK(ba_run(Ps[i], Rs[i], device, nullptr)); return VSLAM_OK; };
    auto plan_cohort = [&]() {
        std::vector<vslam_ba_lane_shape> shapes(N);
        for (int i = 0; i < N; i++) shapes[i] = lane_shape(lanes[i]);
        ba_batch_plan(vslam_ba_batch_shape{N, shapes.data(), NB, useMfma ? 0 : 1}, ba_plan_knobs(), g_baLastPlan);
    };
    if (NL == 0) { plan_cohort(); return run_singles(); }
    auto& A = W.arena;
    size_t arenaBytes = 8192 + (size_t)NL * (CTL_DOUBLES * 8 + sizeof(BaDev) + sizeof(BaLaneAux) + 768);
    for (int i : act) arenaBytes += (size_t)lanes[i].K + std::max(lanes[i].L, 1) + 64;      // (the shared membership block)
    for (int i : act) {
        Lane& q = lanes[i];
        arenaBytes += q.H.arena_bytes(q.K, q.L, nSlots) + (size_t)q.K * (sizeof(DPose) + 1) + (size_t)q.L * 24 + (size_t)q.NP * (4 + 4 + 8 + 1 + 16) + 10 * 256;
    }
    VS_HIP(A.ensure(arenaBytes, stream));
    A.reset();
    double* h_ctlAll = A.take<double>((size_t)CTL_DOUBLES * NL);         // contiguous: polled with one copy
    BaDev* h_tab = A.take<BaDev>(NL);
    BaLaneAux* h_aux = A.take<BaLaneAux>(NL);
    bool fits = h_aux != nullptr;
    for (int a = 0; a < NL && fits; a++) {
        Lane& q = lanes[act[a]];
        q.h_pose0 = A.take<DPose>(q.K); q.h_lm0 = A.take<double>((size_t)3 * q.L);
        q.h_pairKf = A.take<int>(q.NP); q.h_pairLm = A.take<int>(q.NP); q.h_pairOct = A.take<int>((size_t)2 * q.NP);
        q.h_pairFlags = A.take<uint8_t>(q.NP); q.h_pairUv = A.take<float>((size_t)4 * q.NP); q.h_kfLocal = A.take<uint8_t>(q.K);
        fits = q.h_kfLocal && q.H.take(A, q.K, q.L, nSlots);
        q.H.h_ctl = h_ctlAll + (size_t)CTL_DOUBLES * a; q.H.h_D = h_tab + a;      // (the lane's slots of the shared tables)
    }
    // the lanes' membership arrays (rewritten for the second pass) side by side: ONE re-upload instead of one per lane
    size_t presentBytes = 0;
    for (int a = 0; a < NL; a++) presentBytes += (size_t)lanes[act[a]].K + std::max(lanes[act[a]].L, 1);
    uint8_t* const h_present = fits ? A.take<uint8_t>(presentBytes) : nullptr;
    fits = fits && h_present;
    if (fits) {
        uint8_t* pp = h_present;
        for (int a = 0; a < NL; a++) { Lane& q = lanes[act[a]]; q.H.h_kfPresent = pp; pp += q.K; q.H.h_lmPresent = pp; pp += std::max(q.L, 1); }
    }
    if (!fits) { set_error("local BA batch: upload arena too small"); return VSLAM_ERR_CAPACITY; }
    W.pool.run(NL, [&](int a) {
        Lane& q = lanes[act[a]];
        const vslam_ba_problem* P = q.P;
        memcpy(q.h_pose0, q.pose0.data(), (size_t)q.K * sizeof(DPose));
        if (q.L) memcpy(q.h_lm0, P->lm_xyz, (size_t)3 * q.L * sizeof(double));
        memcpy(q.h_pairKf, P->pair_kf, (size_t)q.NP * 4); memcpy(q.h_pairLm, P->pair_lm, (size_t)q.NP * 4);
        memcpy(q.h_pairOct, P->pair_octave, (size_t)2 * q.NP * 4); memcpy(q.h_pairFlags, P->pair_flags, q.NP);
        memcpy(q.h_pairUv, P->pair_uv, (size_t)4 * q.NP * 4); memcpy(q.h_kfLocal, P->kf_local, q.K);
        q.H.fill(P, q.wrong.data(), 0, 1, q.T, q.pose0.data(), nullptr, nSlots);
        ba_init_ctl(q.H.h_ctl, 0, adaptive ? 1 : NB);
    });
    BBS(1);
    // ---- launch geometry shared by the lanes: the plan of the cohort's shape -----------------------------------------------
    int nMax = 0, neMax = 0, nfMax = 0, npMax = 0, valMax = 0;
    for (int i : act) {
        const Lane& q = lanes[i];
        nMax = std::max(nMax, q.H.n); neMax = std::max(neMax, q.H.NE);
        nfMax = std::max(nfMax, q.H.NF); npMax = std::max(npMax, q.NP);
        valMax = std::max(valMax, std::max(q.K * (int)(sizeof(DPose) / sizeof(double)), 3 * q.L));
    }
    plan_cohort();
    const vslam_ba_batch_plan& plan = g_baLastPlan;
    if (plan.status != VSLAM_OK) { set_error("local BA batch: landmark with too many views for the LDS staging"); return VSLAM_ERR_CAPACITY; }
    const int nCU = BA_NCU;
    const int obsBlocks = std::max(1, std::min((nfMax + 255) / 256, std::max(16, 2 * nCU / NL)));
    const int facBlocks = obsBlocks + std::max(neMax, 1);
    const size_t sysMax = (size_t)nMax * nMax + nMax;
    const int maxSlots = plan.max_slots, maxFac = plan.max_factors, lmBlocks = plan.schur_blocks;
    const bool useSchur2 = plan.schur_kernel == VSLAM_BA_KERNEL_SCHUR2, useBack2 = plan.back_kernel == VSLAM_BA_KERNEL_BACK2;
    const int s2Layout = ba_plan_knobs().s2Layout;
    const bool packedS = useSchur2 && s2Layout == BA2_PACKED;
    const int reduceSlots = packedS ? ba_packed_reduce_slots(nMax / 6) : (int)sysMax;      // k_ba_reduce: 32 slots per workgroup
    auto part_doubles = [&](int n) { return (size_t)(useSchur2 ? ba2_part_doubles(n, s2Layout) : n * n + n); };      // one workgroup's partial in Spart
    const bool anyMfma64 = plan.solve_kinds & (1 << BA_SOLVE_MFMA64), anyWave = plan.solve_kinds & (1 << BA_SOLVE_WAVE),
               anyMfma = plan.solve_kinds & (1 << BA_SOLVE_MFMA);
    VS_CHECK(ba_kernel_attributes());
    // ---- device memory: one buffer, bump-allocated; a zeroed head region (arrival counters, slot-0 edge accumulators) ----
    size_t dBytes = 0;
    auto dtake = [&](size_t bytes) { const size_t at = dBytes; dBytes = (dBytes + std::max<size_t>(bytes, 8) + 255) & ~(size_t)255; return at; };
    struct Off { size_t flags, sedge, poseS, lmS, facJ, dP, dL, S, partial, spart, sums, Lg, wrong, outPose, outLm; };
    std::vector<Off> off(NL);
    for (int a = 0; a < NL; a++) { const Lane& q = lanes[act[a]]; off[a].flags = dtake(16 * sizeof(int)); off[a].sedge = dtake(((size_t)q.H.n * q.H.n + q.H.n) * nSlots * 8); }
    const size_t zeroBytes = dBytes;
    size_t wrongBase = 0, wrongEnd = 0, outBase = 0, outEnd = 0;
    wrongBase = dBytes;
    for (int a = 0; a < NL; a++) off[a].wrong = dtake(lanes[act[a]].NP);
    wrongEnd = dBytes;
    outBase = dBytes;
    for (int a = 0; a < NL; a++) { const Lane& q = lanes[act[a]]; off[a].outPose = dtake((size_t)q.K * sizeof(DPose)); off[a].outLm = dtake((size_t)3 * q.L * 8); }
    outEnd = dBytes;
    for (int a = 0; a < NL; a++) {
        const Lane& q = lanes[act[a]];
        const BaPassHost& H = q.H;
        const size_t sysStride = (size_t)H.n * H.n + 2 * H.n + 8;
        off[a].poseS = dtake((size_t)nSlots * q.K * sizeof(DPose)); off[a].lmS = dtake((size_t)nSlots * 3 * q.L * 8);
        off[a].facJ = dtake((size_t)20 * H.NF * nSlots * 8); off[a].dP = dtake((size_t)NB * H.n * 8); off[a].dL = dtake((size_t)NB * 3 * H.Lp * 8);
        off[a].S = dtake(sysStride * NB * 8); off[a].partial = dtake(((size_t)2 * obsBlocks + 2 * (size_t)std::max(H.NE, 1)) * NB * 8);
        off[a].spart = dtake(part_doubles(H.n) * lmBlocks * NB * 8); off[a].sums = dtake(32 * 8);
        off[a].Lg = (H.n > 64 || !useMfma) && H.n > BA_WAVE_N ? dtake((size_t)BA_MFMA_N * BA_MFMA_N * NB * 8) : 0;
    }
    VS_HIP(W.d_mem.alloc(dBytes));
    uint8_t* const dm = W.d_mem.p;
    // landing area: [control blocks][flags of all lanes][results of all lanes]
    const size_t oBackCtl = 0, oBackWrong = ((size_t)CTL_DOUBLES * 8 * NL + 255) & ~(size_t)255, oBackOut = oBackWrong + (wrongEnd - wrongBase);
    const size_t backBytes = oBackOut + (outEnd - outBase);
    VS_HIP(W.h_back.ensure(backBytes, grow_back(), [&] { return hipStreamSynchronize(stream); }));
    uint8_t* const h_back = W.h_back.p;
    // ---- argument tables ------------------------------------------------------------------------------------------------
    for (int a = 0; a < NL; a++) {
        Lane& q = lanes[act[a]];
        const BaPassHost& H = q.H;
        const vslam_ba_problem* P = q.P;
        const Off& o = off[a];
        q.d_flags = (int*)(dm + o.flags); q.d_Sedge = (double*)(dm + o.sedge); q.d_poseS = (DPose*)(dm + o.poseS); q.d_lmS = (double*)(dm + o.lmS);
        q.d_facJ = (double*)(dm + o.facJ); q.d_dP = (double*)(dm + o.dP); q.d_dL = (double*)(dm + o.dL); q.d_S = (double*)(dm + o.S);
        q.d_partial = (double*)(dm + o.partial); q.d_Spart = (double*)(dm + o.spart); q.d_sums = (double*)(dm + o.sums);
        q.d_Lg = o.Lg ? (double*)(dm + o.Lg) : nullptr; q.oWrong = oBackWrong + (o.wrong - wrongBase); q.oOut = oBackOut + (o.outPose - outBase);
        // the chi2 kernel writes its flags and the pass's final values STRAIGHT into the pinned landing area (device-addressable host
        // memory): no download copies behind it - each was a blit launch of its own that queued behind the groups' wide kernels
        q.d_wrong = h_back + q.oWrong; q.d_outPose = (double*)(h_back + q.oOut);
        q.d_outLm = (double*)(h_back + q.oOut + (o.outLm - o.outPose));
        BaDev D{};
        const int n = H.n, K = q.K, L = q.L;
        ba_fill_dev(D, H, A, BaLaneBufs{K, L, q.d_poseS, q.d_lmS, q.d_facJ, q.d_S, q.d_Sedge, q.d_dP, q.d_dL, q.d_sums, q.d_flags}, P->rig, NB, true, adaptive);
        D.partialStride = (size_t)2 * obsBlocks + 2 * (size_t)std::max(H.NE, 1); D.partial = q.d_partial;
        D.spartStride = part_doubles(n) * lmBlocks; D.Spart = q.d_Spart;
        D.solveKind = ba_solve_kind(n, useMfma);
        D.Lg = q.d_Lg;
        D.ctlHost = (double*)(h_back + oBackCtl) + (size_t)CTL_DOUBLES * a;
        *H.h_D = D;
        BaLaneAux X{};
        ba_fill_chi(X.C, P, BaPairArrays{A.dev(q.h_pairKf), A.dev(q.h_pairLm), A.dev(q.h_pairOct), A.dev(q.h_pairFlags), A.dev(q.h_pairUv), A.dev(q.h_kfLocal)},
                    A.dev(H.h_kfPresent), A.dev(H.h_lmPresent), q.d_wrong);
        X.NF = H.NF; X.facPair = A.dev(H.h_facPair); X.facIs = A.dev(H.h_facIs);
        X.nPose = K * (int)(sizeof(DPose) / sizeof(double)); X.nLm = 3 * L; X.pose0 = (const double*)A.dev(q.h_pose0); X.lm0 = A.dev(q.h_lm0);
        X.outPose = q.d_outPose; X.outLm = q.d_outLm;
        h_aux[a] = X;
    }
    const BaDev* const dTab = A.dev(h_tab);
    const BaLaneAux* const dAux = A.dev(h_aux);
    VS_HIP(A.upload(stream));
    VS_HIP(hipMemsetAsync(dm, 0, zeroBytes, stream));
    const int valBlocks = std::max(1, std::min((valMax + 255) / 256, 64));
    hipLaunchKernelGGL(k_ba_init_slots_b, dim3(valBlocks, NL), dim3(256), 0, stream, dTab, dAux);

    // ---- LM rounds for all lanes; the device decides per lane (its own control block) -----------------------------------------
    auto step = [&](bool first) -> vslam_status {
        int t = -1;
        if (first) {
            t = g_baTimer.begin("ba_linearize");
            hipLaunchKernelGGL(k_ba_factors<0>, dim3(facBlocks, 1, NL), dim3(256), 0, stream, dTab, obsBlocks, 1, relTol, absTol);
            g_baTimer.end(t);
        }
        t = g_baTimer.begin("ba_schur");
        if (useSchur2 && s2Layout == BA2_PACKED) hipLaunchKernelGGL(k_ba_schur2, dim3(lmBlocks, NB, NL), dim3(64 * plan.schur_waves), plan.schur_lds, stream, dTab, maxSlots, maxFac);
        else if (useSchur2) hipLaunchKernelGGL(k_ba_schur2_rm, dim3(lmBlocks, NB, NL), dim3(64 * plan.schur_waves), plan.schur_lds, stream, dTab, maxSlots, maxFac, s2Layout);
        else hipLaunchKernelGGL(k_ba_schur, dim3(lmBlocks, plan.schur_shared_w ? 1 : NB, NL), dim3(64 * plan.schur_waves), plan.schur_lds, stream, dTab, maxSlots, plan.schur_shared_w);
        g_baTimer.end(t);
        t = g_baTimer.begin("ba_solve");
        hipLaunchKernelGGL(k_ba_reduce, dim3((reduceSlots + 31) / 32, NB, NL), dim3(256), 0, stream, dTab, lmBlocks, packedS ? 1 : 0);
        if (anyMfma64) hipLaunchKernelGGL(k_ba_solve_mfma64, dim3(NB, 1, NL), dim3(64), 0, stream, dTab);
        if (anyWave) hipLaunchKernelGGL(k_ba_solve_wave, dim3(NB, 1, NL), dim3(64), 0, stream, dTab);
        if (anyMfma) hipLaunchKernelGGL(k_ba_solve_mfma, dim3(NB, 1, NL), dim3(64 * BA_MFMA_NW), plan.solve_lds, stream, dTab, (double*)nullptr);
        g_baTimer.end(t);
        t = g_baTimer.begin("ba_back");
        if (useBack2) hipLaunchKernelGGL(k_ba_back2, dim3(plan.back_blocks, 1, NL), dim3(64 * plan.back_waves), plan.back_lds, stream, dTab, maxSlots, maxFac);
        else hipLaunchKernelGGL(k_ba_back, dim3(plan.back_blocks, plan.back_shared ? 1 : NB, NL), dim3(64 * plan.back_waves), plan.back_lds, stream, dTab, maxSlots, plan.back_shared);
        g_baTimer.end(t);
        t = g_baTimer.begin("ba_eval");
        hipLaunchKernelGGL(k_ba_factors<1>, dim3(facBlocks, NB, NL), dim3(256), 0, stream, dTab, obsBlocks, 1, relTol, absTol);
        g_baTimer.end(t);
        VS_HIP(hipGetLastError());
        return VSLAM_OK;
    };
    double* const b_ctl = (double*)(h_back + oBackCtl);
    // The host's copy of the lanes' control blocks is written by the control steps themselves (BaDev::ctlHost).  It starts every pass as
    // the ARMED block, so that a poll can only ever see "not done" until a lane's own control step has said otherwise - a block left
    // over from the previous pass (BA_DONE) would end the pass before it began and leave the chi2 kernel with lanes it skips.
    memcpy(b_ctl, h_ctlAll, (size_t)CTL_DOUBLES * 8 * NL);
    // Rounds are enqueued ahead of the poll that tells whether every lane has finished: `first` rounds (a pass of m iterations needs
    // at least m - the device skips the rounds of lanes that are done, a skipped launch costs a few microseconds, a poll a
    // synchronisation of this stream), then two at a time.
    auto lm_loop = [&](int first) -> vslam_status {
        static const int perPollEnv = getenv("VSLAM_BA_STEPS_PER_POLL") ? std::max(1, atoi(getenv("VSLAM_BA_STEPS_PER_POLL"))) : 0;
        int enq = 0, polls = 0;
        for (;;) {
            const int batch = perPollEnv ? perPollEnv : (enq == 0 ? first : 2);
            for (int b = 0; b < batch; b++) VS_CHECK(step(enq + b == 0));
            enq += batch;
            static const bool mirrorOff = getenv("VSLAM_BA_CTL_MIRROR") && atoi(getenv("VSLAM_BA_CTL_MIRROR")) == 0;
            // (belt and braces: a pass that needs more than a handful of polls reads the device's own blocks - the authoritative copy)
            if (mirrorOff || ++polls > 4) VS_HIP(hipMemcpyAsync(b_ctl, A.dev(h_ctlAll), (size_t)CTL_DOUBLES * 8 * NL, hipMemcpyDeviceToHost, stream));
            VS_HIP(vslam::stream_wait_blocking(stream));      // (every control step mirrors its block into the landing area: BaDev::ctlHost)
            g_bbsPolls++;
            bool all = true;
            for (int a = 0; a < NL; a++) all &= ((const int*)(b_ctl + (size_t)CTL_DOUBLES * a + CTL_INTS))[CI_STATE] == BA_DONE;
            if (all) return VSLAM_OK;
            if (enq > 400) {
                // (diagnosis in the message: the control block of the first lane that is not done, as the device holds it)
                (void)hipMemcpy(b_ctl, A.dev(h_ctlAll), (size_t)CTL_DOUBLES * 8 * NL, hipMemcpyDeviceToHost);
                for (int a = 0; a < NL; a++) {
                    const double* c = b_ctl + (size_t)CTL_DOUBLES * a;
                    const int* ci = (const int*)(c + CTL_INTS);
                    if (ci[CI_STATE] == BA_DONE) continue;
                    int fl[8] = {0};
                    (void)hipMemcpy(fl, lanes[act[a]].d_flags, sizeof(fl), hipMemcpyDeviceToHost);
                    set_error("local BA batch: LM did not terminate (lane %d of %d: state %d sel %d iter %d inner %d maxit %d first %d nact %d rounds %d lambda %g error %g cur %g; "
                              "F %d NF %d Lp %d NE %d; flags %d %d %d %d | %d %d %d %d; obsBlocks %d neMax %d)", a, NL, ci[CI_STATE], ci[CI_SEL], ci[CI_ITER], ci[CI_INNER], ci[CI_MAXIT], ci[CI_FIRST], ci[CI_NACT], ci[CI_ROUNDS],
                              c[CTL_LAMBDA], c[CTL_ERROR], c[CTL_CUR], lanes[act[a]].H.F, lanes[act[a]].H.NF, lanes[act[a]].H.Lp, lanes[act[a]].H.NE,
                              fl[0], fl[1], fl[2], fl[3], fl[4], fl[5], fl[6], fl[7], obsBlocks, neMax);
                    return VSLAM_ERR_INVALID;
                }
                set_error("local BA batch: LM did not terminate (every lane done on the device: the host's copy lagged)");
                return VSLAM_ERR_INVALID;
            }
        }
    };
    auto report = [&](int ps) {
        for (int a = 0; a < NL; a++) {
            Lane& q = lanes[act[a]];
            if (ps == 1 && !q.pass2) continue;
            if (ps == 0) ba_write_report(q.R, 0, b_ctl + (size_t)CTL_DOUBLES * a, q.H.F, q.H.NF, q.H.Lp, q.H.sumK2);
            else ba_write_report(q.R, 1, b_ctl + (size_t)CTL_DOUBLES * a, q.H.F, q.S2.NF2, q.S2.Lp2, q.S2.k2);
        }
    };
    const int chiBlocks = std::max(1, (std::max(npMax, valMax) + 255) / 256);
    auto chi2 = [&](int gather) -> vslam_status {
        const int t = g_baTimer.begin("ba_chi2");
        hipLaunchKernelGGL(k_ba_chi2_b, dim3(chiBlocks, NL), dim3(256), 0, stream, dTab, dAux, gather);
        g_baTimer.end(t);
        VS_HIP(hipGetLastError());
        VS_HIP(vslam::stream_wait_blocking(stream));      // (flags / values are in the landing area: see the argument tables)
        return VSLAM_OK;
    };
    // ---- pass 1 ------------------------------------------------------------------------------------------------------------------
    BBS(2);
    VS_CHECK(lm_loop(5));
    report(0);
    BBS(3);
    VS_CHECK(chi2(0));
    BBS(4);
    // ---- second pass on the first pass's structure: membership / statistics from the flags; lanes whose graph loses a keyframe
    //      (their free index would change) go to the one-problem path, which rebuilds ------------------------------------------------
    std::vector<int> redo;
    W.pool.run(NL, [&](int a) {
        Lane& q = lanes[act[a]];
        const vslam_ba_problem* P = q.P;
        const BaPassHost& H = q.H;
        memcpy(q.wrong.data(), h_back + q.oWrong, q.NP);
        if (q.R->pair_wrong_pass1) memcpy(q.R->pair_wrong_pass1, q.wrong.data(), q.NP);
        H.second_pass(P, q.wrong.data(), 0, 1, q.T, nullptr, q.S2);
        q.pass2 = g_baMask != 0 && q.S2.same;
        if (!q.pass2) { int* ci = (int*)(H.h_ctl + CTL_INTS); ci[CI_STATE] = BA_DONE; ci[CI_FIRST] = 0; return; }      // (stays out of the second round)
        for (int k = 0; k < q.K; k++) H.h_kfPresent[k] = q.S2.kfP2[k];
        for (int l = 0; l < q.L; l++) H.h_lmPresent[l] = q.S2.lmP2[l];
        ba_init_ctl(H.h_ctl, 1, adaptive ? 1 : NB);
    });
    for (int a = 0; a < NL; a++) if (!lanes[act[a]].pass2) redo.push_back(act[a]);
    BBS(5);
    if ((int)redo.size() < NL) {
        // re-armed control blocks and the membership arrays: the arena's head (control blocks) + each lane's present arrays
        VS_HIP(hipMemcpyAsync(A.dev(h_ctlAll), h_ctlAll, (size_t)CTL_DOUBLES * 8 * NL, hipMemcpyHostToDevice, stream));
        VS_HIP(hipMemcpyAsync(A.dev(h_present), h_present, presentBytes, hipMemcpyHostToDevice, stream));
        memcpy(b_ctl, h_ctlAll, (size_t)CTL_DOUBLES * 8 * NL);      // (the re-armed blocks; lanes that stay out of the pass carry BA_DONE)
        hipLaunchKernelGGL(k_ba_second_pass_b, dim3(std::max(1, std::min((std::max(nfMax, valMax) + 255) / 256, 64)), NL), dim3(256), 0, stream, dTab, dAux);
        VS_CHECK(lm_loop(6));
        report(1);
        BBS(6);
        VS_CHECK(chi2(1));
        BBS(7);
    }
    for (int a = 0; a < NL; a++) {
        Lane& q = lanes[act[a]];
        if (!q.pass2) continue;
        const DPose* po = (const DPose*)(h_back + q.oOut);
        const double* lo = (const double*)(h_back + q.oOut + (((size_t)q.K * sizeof(DPose) + 255) & ~(size_t)255));
        ba_write_result(q.R, po, lo, h_back + q.oWrong, q.K, q.L, q.NP);
    }
    BBS(8);
    for (int i : redo) VS_CHECK(ba_run(Ps[i], Rs[i], device, nullptr));
    return run_singles();
}

namespace vslam {
// VSLAM_BATCH_PHASES: where ba_run's wall time goes (averages per call; the marks do not synchronise, so "lm" holds the
// polls of both LM loops, "chi2" the re-check + second-pass preparation + result fetch)
void ba_host_profile_print() { BaMarks::print(); }
}  // namespace vslam

extern "C" {

vslam_status vslam_local_ba(const vslam_ba_problem* problem, vslam_ba_result* result, int32_t device,
                            const vslam_comm* comm) {
    return ba_run(problem, result, device, comm);
}

/* n tracker-window problems optimised together (one launch per stage for all of them); results equal n vslam_local_ba calls */
vslam_status vslam_local_ba_batch(const vslam_ba_problem* const* problems, vslam_ba_result* const* results, int32_t n, int32_t device) {
    return ba_run_batch(problems, results, n, device);
}

vslam_status vslam_local_ba_batch_plan(const vslam_ba_batch_shape* shape, vslam_ba_batch_plan* plan) {
    if (!shape || !plan || shape->n_lanes < 0 || (shape->n_lanes > 0 && !shape->lanes) || shape->lookahead < 1 || shape->lookahead > BA_MAX_NB ||
        shape->solver < 0 || shape->solver > 1) return VSLAM_ERR_INVALID;
    ba_batch_plan(*shape, ba_plan_knobs(), *plan);
    return VSLAM_OK;
}

vslam_status vslam_local_ba_last_batch_plan(vslam_ba_batch_plan* plan) {
    if (!plan) return VSLAM_ERR_INVALID;
    *plan = g_baLastPlan;
    return VSLAM_OK;
}

vslam_status vslam_local_ba_timings(const char** names, float* ms, int32_t cap, int32_t* n_out) {
    if (!n_out) return VSLAM_ERR_INVALID;
    const char* nm[64];
    float tv[64];
    int n = g_baTimer.read(nm, tv, cap < 64 ? cap : 64);
    for (int i = 0; i < n; i++) { if (names) names[i] = nm[i]; if (ms) ms[i] = tv[i]; }
    // "<group>#n": the number of timed intervals (= launches of the group's kernel) behind each sum, as further entries
    static const char* const cntName[][2] = {{"ba_linearize", "ba_linearize#n"}, {"ba_schur", "ba_schur#n"}, {"ba_solve", "ba_solve#n"},
                                             {"ba_back", "ba_back#n"}, {"ba_eval", "ba_eval#n"}, {"ba_chi2", "ba_chi2#n"}, {"ba_allreduce", "ba_allreduce#n"}};
    const int base = n;
    for (int i = 0; i < base && n < cap; i++)
        for (const auto& c : cntName)
            if (!strcmp(nm[i], c[0])) {
                int k = 0;
                for (size_t q = 0; q < g_baTimer.used; q++) if (!strcmp(g_baTimer.items[q].name, c[0])) k++;
                if (names) names[n] = c[1];
                if (ms) ms[n] = (float)k;
                n++;
                break;
            }
    *n_out = n;
    return VSLAM_OK;
}

vslam_status vslam_local_ba_set_lookahead(int32_t candidates, int32_t speculative_linearize, int32_t mask_second_pass) {
    if (candidates > BA_MAX_NB) return VSLAM_ERR_INVALID;
    g_baLookahead = candidates > 0 ? candidates : -1;
    g_baSpecLin = speculative_linearize < 0 ? -1 : (speculative_linearize ? 1 : 0);
    g_baMask = mask_second_pass != 0 ? 1 : 0;
    return VSLAM_OK;
}

vslam_status vslam_local_ba_set_solver(int32_t kind) {
    if (kind < -1 || kind > 1) return VSLAM_ERR_INVALID;
    g_baSolver = kind;
    return VSLAM_OK;
}

vslam_status vslam_local_ba_set_timing(int32_t on) {
    g_baTimer.enabled = on != 0;
    return VSLAM_OK;
}
int32_t vslam_local_ba_get_timing(void) { return g_baTimer.enabled ? 1 : 0; }

}  // extern "C"

namespace vslam {
// Zero-copy, NOT synchronised form of vslam_ba_refresh_depth for a caller that serves several requests with one wait (the lockstep
// group's serve_requests): inputs are staged in the calling thread's pinned arena, which the kernel addresses directly, the outputs land
// there too; `out` points into the arena and is valid once the pool's stream has been synchronised (DevPool::sync recycles the arena,
// so the caller copies the results out first).  Returns VSLAM_ERR_CAPACITY when the arena has no room yet (it grows at the next sync):
// the caller then takes the synchronous form.  The requests may come from different cameras: kf_close_th holds the close threshold
// (refresh_close_th) of every staged keyframe pose, written into the same arena block as the poses.  Other arguments as
// vslam_ba_refresh_depth (validated by the caller).
vslam_status refresh_depth_enqueue(const float* kf_close_th, int n_kf, const double* kf_pose_wc, int n_lm, const double* lm_xyz,
                                   const uint8_t* lm_outlier, int n_pairs, const int* pair_kf, const int* pair_lm, const uint8_t* pair_wrong,
                                   const float* cur_depth, int device, RefreshTicket* out) {
    if (n_pairs <= 0 || n_kf < 1 || !out || !kf_close_th) return VSLAM_ERR_INVALID;
    // test switch: behave as if the arena had no room, so that the callers' synchronous per-keyframe form is reached at will
    if (const char* e = getenv("VSLAM_REFRESH_FORCE_CAPACITY")) if (atoi(e) != 0) return VSLAM_ERR_CAPACITY;
    VS_HIP(hipSetDevice(device));
    DevPool* pool = thread_pool(device);
    if (!pool) { set_error("no device pool"); return VSLAM_ERR_HIP; }
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off = (off + bytes + 255) & ~(size_t)255; return o; };
    const size_t oT = take(n_kf * sizeof(DPose)), oTh = take(n_kf * sizeof(float)), oLm = take((size_t)3 * std::max(n_lm, 1) * sizeof(double)),
                 oO = take(std::max(n_lm, 1)), oKf = take(n_pairs * sizeof(int)), oL = take(n_pairs * sizeof(int)), oW = take(n_pairs),
                 oCur = take(n_pairs * sizeof(float)), oD = take(n_pairs * sizeof(float)), oC = take(n_pairs), oU = take(n_pairs);
    uint8_t* st = pool->stage(off);
    if (!st) return VSLAM_ERR_CAPACITY;
    DPose* Tcw = (DPose*)(st + oT);
    for (int k = 0; k < n_kf; k++) { DPose T; pose_from_rm16(kf_pose_wc + 16 * (size_t)k, T); pose_inverse(T, Tcw[k]); }
    memcpy(st + oTh, kf_close_th, n_kf * sizeof(float));
    if (n_lm) { memcpy(st + oLm, lm_xyz, (size_t)3 * n_lm * sizeof(double)); memcpy(st + oO, lm_outlier, n_lm); }
    memcpy(st + oKf, pair_kf, n_pairs * sizeof(int)); memcpy(st + oL, pair_lm, n_pairs * sizeof(int));
    memcpy(st + oW, pair_wrong, n_pairs); memcpy(st + oCur, cur_depth, n_pairs * sizeof(float));
    hipLaunchKernelGGL(k_ba_refresh_depth, dim3((n_pairs + 255) / 256), dim3(256), 0, pool->stream, n_pairs, (const int*)(st + oKf),
                       (const int*)(st + oL), (const uint8_t*)(st + oW), (const uint8_t*)(st + oO), (const float*)(st + oCur),
                       (const DPose*)(st + oT), (const double*)(st + oLm), (const float*)(st + oTh), 0.f, (float*)(st + oD), st + oC, st + oU);
    VS_HIP(hipGetLastError());
    out->dep = (const float*)(st + oD); out->clo = st + oC; out->up = st + oU;
    return VSLAM_OK;
}

// The synchronous form behind vslam_ba_refresh_depth: one threshold for all pairs (kf_close_th == null: the public call, as it always
// was) or one per keyframe pose (the group's fallback while the arena has no room).  Arguments validated by the caller.
vslam_status refresh_depth_sync(const float* kf_close_th, float closeTh, int n_kf, const double* kf_pose_wc, int n_lm, const double* lm_xyz,
                                const uint8_t* lm_outlier, int n_pairs, const int* pair_kf, const int* pair_lm, const uint8_t* pair_wrong,
                                const float* cur_depth, int device, float* depth_out, uint8_t* close_out, uint8_t* updated_out) {
    VS_HIP(hipSetDevice(device));
    std::vector<DPose> Tcw(n_kf);
    for (int k = 0; k < n_kf; k++) { DPose T; pose_from_rm16(kf_pose_wc + 16 * (size_t)k, T); pose_inverse(T, Tcw[k]); }
    // one device block for all operands, from the calling thread's block cache (no hipMalloc / hipFree in the steady state)
    DevPool* pool = thread_pool(device);
    if (!pool) { set_error("no device pool"); return VSLAM_ERR_HIP; }
    hipStream_t ps = pool->stream;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off = (off + bytes + 255) & ~(size_t)255; return o; };
    const size_t oT = take(n_kf * sizeof(DPose)), oLm = take((size_t)3 * std::max(n_lm, 1) * sizeof(double)), oO = take(std::max(n_lm, 1)),
                 oKf = take(n_pairs * sizeof(int)), oL = take(n_pairs * sizeof(int)), oW = take(n_pairs), oCur = take(n_pairs * sizeof(float)),
                 oTh = take(kf_close_th ? n_kf * sizeof(float) : 0),
                 oD = take(n_pairs * sizeof(float)), oC = take(n_pairs), oU = take(n_pairs);
    PoolBuf<uint8_t> mem(pool);
    VS_HIP(mem.alloc(off));
    // ONE upload for the inputs (they are laid out back to back, oT .. oTh: staged in the pool's pinned arena in the
    // device layout) and ONE download for the three outputs (oD .. oU): every copy is a blit launch that queues behind the
    // lockstep groups' wide kernels, and a mapping pass had ~37 of them
    {
        const size_t inBytes = oD;
        uint8_t* st = pool->stage(inBytes);
        auto put = [&](size_t at, const void* src, size_t bytes) -> hipError_t {
            if (!bytes) return hipSuccess;
            if (st) { memcpy(st + at, src, bytes); return hipSuccess; }
            return pool->h2d(mem.p + at, src, bytes);      // (no staging room yet: one copy per array)
        };
        VS_HIP(put(oT, Tcw.data(), n_kf * sizeof(DPose)));
        if (n_lm) { VS_HIP(put(oLm, lm_xyz, (size_t)3 * n_lm * sizeof(double))); VS_HIP(put(oO, lm_outlier, n_lm)); }
        VS_HIP(put(oKf, pair_kf, n_pairs * sizeof(int))); VS_HIP(put(oL, pair_lm, n_pairs * sizeof(int)));
        VS_HIP(put(oW, pair_wrong, n_pairs)); VS_HIP(put(oCur, cur_depth, n_pairs * sizeof(float)));
        if (kf_close_th) VS_HIP(put(oTh, kf_close_th, n_kf * sizeof(float)));
        if (st) VS_HIP(hipMemcpyAsync(mem.p, st, inBytes, hipMemcpyHostToDevice, ps));
    }
    hipLaunchKernelGGL(k_ba_refresh_depth, dim3((n_pairs + 255) / 256), dim3(256), 0, ps, n_pairs, (const int*)(mem.p + oKf),
                       (const int*)(mem.p + oL), (const uint8_t*)(mem.p + oW), (const uint8_t*)(mem.p + oO), (const float*)(mem.p + oCur),
                       (const DPose*)(mem.p + oT), (const double*)(mem.p + oLm), kf_close_th ? (const float*)(mem.p + oTh) : nullptr, closeTh,
                       (float*)(mem.p + oD), mem.p + oC, mem.p + oU);
    VS_HIP(hipGetLastError());
    {
        const size_t outBytes = off - oD;
        uint8_t* st = pool->stage(outBytes);
        if (st) {
            VS_HIP(hipMemcpyAsync(st, mem.p + oD, outBytes, hipMemcpyDeviceToHost, ps));
            VS_HIP(hipStreamSynchronize(ps));
            memcpy(depth_out, st, n_pairs * sizeof(float)); memcpy(close_out, st + (oC - oD), n_pairs); memcpy(updated_out, st + (oU - oD), n_pairs);
            VS_HIP(pool->sync());       // (recycles the arena - and may re-allocate it, hence after the copies)
        } else {
            VS_HIP(pool->d2h(depth_out, mem.p + oD, n_pairs * sizeof(float)));
            VS_HIP(pool->d2h(close_out, mem.p + oC, n_pairs));
            VS_HIP(pool->d2h(updated_out, mem.p + oU, n_pairs));
            VS_HIP(pool->sync());
        }
    }
    return VSLAM_OK;
}
}  // namespace vslam

extern "C" {

vslam_status vslam_ba_refresh_depth(const vslam_rig* rig, int32_t n_kf, const double* kf_pose_wc, int32_t n_lm,
                                    const double* lm_xyz, const uint8_t* lm_outlier, int32_t n_pairs,
                                    const int32_t* pair_kf, const int32_t* pair_lm, const uint8_t* pair_wrong,
                                    const float* cur_depth, int32_t device, float* depth_out, uint8_t* close_out,
                                    uint8_t* updated_out) {
    if (!rig || n_kf < 1 || n_lm < 0 || n_pairs < 0 || !kf_pose_wc || (n_lm > 0 && (!lm_xyz || !lm_outlier)) ||
        (n_pairs > 0 && (!pair_kf || !pair_lm || !pair_wrong || !cur_depth || !depth_out || !close_out || !updated_out))) {
        set_error("vslam_ba_refresh_depth: invalid arguments");
        return VSLAM_ERR_INVALID;
    }
    for (int p = 0; p < n_pairs; p++)
        if (pair_kf[p] < 0 || pair_kf[p] >= n_kf || pair_lm[p] < 0 || pair_lm[p] >= n_lm) { set_error("vslam_ba_refresh_depth: pair index out of range"); return VSLAM_ERR_INVALID; }
    VS_CHECK(ba_check_device(device));
    if (n_pairs == 0) return VSLAM_OK;
    return vslam::refresh_depth_sync(nullptr, vslam::refresh_close_th(*rig), n_kf, kf_pose_wc, n_lm, lm_xyz, lm_outlier, n_pairs, pair_kf, pair_lm,
                                     pair_wrong, cur_depth, device, depth_out, close_out, updated_out);
}

// The merged form a lockstep group uses (batch.hip serve_requests) as a call of its own: n_req requests staged together - request r
// brings req_n_kf[r] keyframe poses and its camera rigs[r]; kf_pose_wc / pair_kf index the concatenation - ONE launch, every pair
// tested against the threshold of its own keyframe's camera.  Results are those of one vslam_ba_refresh_depth call per request.
vslam_status vslam_ba_refresh_depth_merged(const vslam_rig* rigs, const int32_t* req_n_kf, int32_t n_req, const double* kf_pose_wc,
                                           int32_t n_lm, const double* lm_xyz, const uint8_t* lm_outlier, int32_t n_pairs,
                                           const int32_t* pair_kf, const int32_t* pair_lm, const uint8_t* pair_wrong,
                                           const float* cur_depth, int32_t device, float* depth_out, uint8_t* close_out,
                                           uint8_t* updated_out) {
    if (!rigs || !req_n_kf || n_req < 1) { set_error("vslam_ba_refresh_depth_merged: invalid arguments"); return VSLAM_ERR_INVALID; }
    std::vector<float> th;
    for (int r = 0; r < n_req; r++) {
        if (req_n_kf[r] < 0) { set_error("vslam_ba_refresh_depth_merged: invalid arguments"); return VSLAM_ERR_INVALID; }
        th.insert(th.end(), (size_t)req_n_kf[r], vslam::refresh_close_th(rigs[r]));
    }
    const int n_kf = (int)th.size();
    if (n_kf < 1 || n_lm < 0 || n_pairs < 0 || !kf_pose_wc || (n_lm > 0 && (!lm_xyz || !lm_outlier)) ||
        (n_pairs > 0 && (!pair_kf || !pair_lm || !pair_wrong || !cur_depth || !depth_out || !close_out || !updated_out))) {
        set_error("vslam_ba_refresh_depth_merged: invalid arguments");
        return VSLAM_ERR_INVALID;
    }
    for (int p = 0; p < n_pairs; p++)
        if (pair_kf[p] < 0 || pair_kf[p] >= n_kf || pair_lm[p] < 0 || pair_lm[p] >= n_lm) { set_error("vslam_ba_refresh_depth_merged: pair index out of range"); return VSLAM_ERR_INVALID; }
    VS_CHECK(ba_check_device(device));
    if (n_pairs == 0) return VSLAM_OK;
    vslam::RefreshTicket tk{};
    vslam_status st = VSLAM_ERR_CAPACITY;
    for (int attempt = 0; attempt < 2 && st == VSLAM_ERR_CAPACITY; attempt++) {
        st = vslam::refresh_depth_enqueue(th.data(), n_kf, kf_pose_wc, n_lm, lm_xyz, lm_outlier, n_pairs, pair_kf, pair_lm, pair_wrong, cur_depth, device, &tk);
        vslam::DevPool* pool = vslam::thread_pool(device);
        if (!pool) return VSLAM_ERR_HIP;
        if (st == VSLAM_OK) {
            VS_HIP(hipStreamSynchronize(pool->stream));
            memcpy(depth_out, tk.dep, n_pairs * sizeof(float)); memcpy(close_out, tk.clo, n_pairs); memcpy(updated_out, tk.up, n_pairs);
        }
        if (st == VSLAM_OK || st == VSLAM_ERR_CAPACITY) VS_HIP(pool->sync());      // (recycles the arena; grows it when there was no room)
    }
    if (st == VSLAM_ERR_CAPACITY)
        return vslam::refresh_depth_sync(th.data(), 0.f, n_kf, kf_pose_wc, n_lm, lm_xyz, lm_outlier, n_pairs, pair_kf, pair_lm, pair_wrong, cur_depth,
                                         device, depth_out, close_out, updated_out);
    return st;
}

}  // extern "C"
