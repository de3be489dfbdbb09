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
// vslam_global_ba_batch runs several problems (lanes) at once: every stage has a k_gba_*_b kernel
// with the lane as a grid dimension, the reduce is one workgroup per lane (k_gba_reduce_b) and the rule one thread per lane
// (k_gba_decide_b); the host waits once per ROUND (one trial of every active lane).  The bodies of all kernels are in
// gba_dev.hpp, one function per stage on ONE problem's arrays, called by k_gba_* and k_gba_*_b alike: a lane's bytes are the
// single call's.  The lane table is packed by gba_pack_host.hpp (no HIP).
#include "common.hpp"
#include "dmath.hpp"
#include "pgo_dev.hpp"
#include "gba_host.hpp"
#include "gba_pack_host.hpp"
#include "gba_call.hpp"
#include "gba_dev.hpp"
#include <cmath>

using namespace vslam;

namespace {

// ---- the kernels of vslam_global_ba: one problem, the bodies of gba_dev.hpp on the call's arrays
__global__ __launch_bounds__(256) void k_gba_linearize(GbaDev D, const PgoCtl* __restrict__ ctl, int init, const double* __restrict__ P0,
                                                       const double* __restrict__ P1, const double* __restrict__ L0,
                                                       const double* __restrict__ L1, double* __restrict__ Jp, double* __restrict__ Jl,
                                                       double* __restrict__ res, double* __restrict__ cost) {
    gba_linearize_slot(blockIdx.x * blockDim.x + threadIdx.x, D, ctl, init, P0, P1, L0, L1, Jp, Jl, res, cost);
}

__global__ __launch_bounds__(256) void k_gba_cost(GbaDev D, const PgoCtl* __restrict__ ctl, const double* __restrict__ P0,
                                                  const double* __restrict__ P1, const double* __restrict__ L0,
                                                  const double* __restrict__ L1, double* __restrict__ cost) {
    gba_cost_slot(blockIdx.x * blockDim.x + threadIdx.x, D, ctl, P0, P1, L0, L1, cost);
}

__global__ __launch_bounds__(256) void k_gba_edge_linearize(GbaDev D, const PgoCtl* __restrict__ ctl, int init, const double* __restrict__ P0,
                                                            const double* __restrict__ P1, double* __restrict__ res, double* __restrict__ Ji,
                                                            double* __restrict__ Jj, double* __restrict__ cost) {
    gba_edge_linearize_one(blockIdx.x * blockDim.x + threadIdx.x, D, ctl, init, P0, P1, res, Ji, Jj, cost);
}

__global__ __launch_bounds__(256) void k_gba_edge_cost(GbaDev D, const PgoCtl* __restrict__ ctl, const double* __restrict__ P0,
                                                       const double* __restrict__ P1, double* __restrict__ cost) {
    gba_edge_cost_one(blockIdx.x * blockDim.x + threadIdx.x, D, ctl, P0, P1, cost);
}

__global__ __launch_bounds__(256) void k_gba_landmark(GbaDev D, const PgoCtl* __restrict__ ctl, const double* __restrict__ Jl,
                                                      const double* __restrict__ res, double* __restrict__ Hinv, double* __restrict__ gl,
                                                      int* __restrict__ flag) {
    gba_landmark_one(blockIdx.x * blockDim.x + threadIdx.x, D, ctl, Jl, res, Hinv, gl, flag);
}

__global__ __launch_bounds__(256) void k_gba_wy(GbaDev D, const PgoCtl* __restrict__ ctl, const double* __restrict__ Jp,
                                                const double* __restrict__ Jl, const double* __restrict__ Hinv, double* __restrict__ W,
                                                double* __restrict__ Y) {
    gba_wy_pair(blockIdx.x * blockDim.x + threadIdx.x, D, ctl, Jp, Jl, Hinv, W, Y);
}

__global__ __launch_bounds__(64) void k_gba_edge_columns(GbaDev D, const PgoCtl* __restrict__ ctl, const double* __restrict__ res,
                                                         const double* __restrict__ Ji, const double* __restrict__ Jj,
                                                         double* __restrict__ band, double* __restrict__ diagH, double* __restrict__ g) {
    gba_edge_column(blockIdx.x, threadIdx.x, D, ctl, res, Ji, Jj, band, diagH, g);
}

__global__ __launch_bounds__(64) void k_gba_gather(GbaDev D, const PgoCtl* __restrict__ ctl, const double* __restrict__ Jp,
                                                   const double* __restrict__ res, const double* __restrict__ W, const double* __restrict__ Y,
                                                   const double* __restrict__ gl, double* __restrict__ band, double* __restrict__ diagH,
                                                   double* __restrict__ g) {
    gba_gather_block(blockIdx.x, threadIdx.x, D, ctl, Jp, res, W, Y, gl, band, diagH, g);
}

__global__ __launch_bounds__(256) void k_gba_band_copy(GbaDev D, const PgoCtl* __restrict__ ctl, const double* __restrict__ bandH,
                                                       const double* __restrict__ g, double* __restrict__ bandL, double* __restrict__ rhs) {
    gba_band_copy_one((size_t)blockIdx.x * blockDim.x + threadIdx.x, D, ctl, bandH, g, bandL, rhs);
}

__global__ __launch_bounds__(PGO_CHOL_NT) void k_gba_band_chol(GbaDev D, const PgoCtl* __restrict__ ctl, double* __restrict__ bandL,
                                                               const double* __restrict__ diagH, double* __restrict__ rhs,
                                                               double* __restrict__ delta, int* __restrict__ flag) {
    if (!ctl->active) return;
    pgo_band_chol_walk(D.nf, D.b, ctl->lambda, bandL, diagH, rhs, delta, flag);
}

__global__ __launch_bounds__(256) void k_gba_back(GbaDev D, const PgoCtl* __restrict__ ctl, const double* __restrict__ W,
                                                  const double* __restrict__ Hinv, const double* __restrict__ gl, double* __restrict__ L0,
                                                  double* __restrict__ L1, double* __restrict__ delta) {
    gba_back_one(blockIdx.x * blockDim.x + threadIdx.x, D, ctl, W, Hinv, gl, L0, L1, delta);
}

__global__ __launch_bounds__(256) void k_gba_retract(GbaDev D, const PgoCtl* __restrict__ ctl, double* __restrict__ P0, double* __restrict__ P1,
                                                     const double* __restrict__ delta) {
    gba_retract_one(blockIdx.x * blockDim.x + threadIdx.x, D, ctl, P0, P1, delta);
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

__global__ __launch_bounds__(256) void k_gba_chi2(GbaDev D, const PgoCtl* __restrict__ ctl, const double* __restrict__ P0,
                                                  const double* __restrict__ P1, const double* __restrict__ L0, const double* __restrict__ L1,
                                                  uint8_t* __restrict__ wrong) {
    gba_chi2_pair(blockIdx.x * blockDim.x + threadIdx.x, D, ctl, P0, P1, L0, L1, wrong);
}

// ---- the kernels of vslam_global_ba_batch: several problems (lanes) in one launch per stage, blockIdx.y (blockIdx.x of the
// one-workgroup-per-lane kernels) = lane.  The lanes' arrays are concatenated (gba_pack_host.hpp); `B` and `Wb` hold where the
// concatenated arrays begin, a lane's table entry where its parts begin in them.  Indices inside a lane's arrays are lane-local,
// so every body sees one problem's arrays whatever the other lanes are.  A lane that has stopped costs a workgroup one load.
struct GbaWork {                    // the device's own arrays
    double *P0, *P1, *L0, *L1;      // both value buffers (P0 and L0 come up with the problem)
    double *Jp, *Jl, *res, *cost, *eres, *eJi, *eJj, *Hinv, *gl, *W, *Y, *bandH, *bandL, *diagH, *g, *rhs, *delta;
    uint8_t* wrong;
};

__device__ __forceinline__ GbaWork gba_lane_work(const GbaLane* T, const GbaWork& B) {
    GbaWork W;
    const size_t kf0 = (size_t)T->kf0, lm0 = (size_t)T->lm0, p0 = (size_t)T->pair0, e0 = (size_t)T->edge0, f0 = (size_t)T->free0;
    W.P0 = B.P0 + kf0 * 12; W.P1 = B.P1 + kf0 * 12; W.L0 = B.L0 + lm0 * 3; W.L1 = B.L1 + lm0 * 3;
    W.Jp = B.Jp + p0 * 24; W.Jl = B.Jl + p0 * 12; W.res = B.res + p0 * 4; W.cost = B.cost + p0 * 2 + e0;
    W.eres = B.eres + e0 * 6; W.eJi = B.eJi + e0 * 36; W.eJj = B.eJj + e0 * 36;
    W.Hinv = B.Hinv + lm0 * 9; W.gl = B.gl + lm0 * 3; W.W = B.W + p0 * 18; W.Y = B.Y + p0 * 18;
    W.bandH = B.bandH + (size_t)T->band0 * 36; W.bandL = B.bandL + (size_t)T->band0 * 36;
    W.diagH = B.diagH + f0 * 6; W.g = B.g + f0 * 6; W.rhs = B.rhs + f0 * 6; W.delta = B.delta + f0 * 6 + lm0 * 3;
    W.wrong = B.wrong + p0;
    return W;
}

__global__ __launch_bounds__(256) void k_gba_linearize_b(const GbaLane* __restrict__ tab, const PgoCtl* __restrict__ ctl, int init, GbaDev B, GbaWork Wb) {
    const PgoCtl* C = ctl + blockIdx.y;
    if (!init && !C->active) return;
    const GbaLane* T = lane_entry(tab, blockIdx.y);
    const GbaWork W = gba_lane_work(T, Wb);
    gba_linearize_slot(blockIdx.x * blockDim.x + threadIdx.x, gba_lane_dev(T, B), C, init, W.P0, W.P1, W.L0, W.L1, W.Jp, W.Jl, W.res, W.cost);
}

__global__ __launch_bounds__(256) void k_gba_edge_linearize_b(const GbaLane* __restrict__ tab, const PgoCtl* __restrict__ ctl, int init, GbaDev B, GbaWork Wb) {
    const PgoCtl* C = ctl + blockIdx.y;
    if (!init && !C->active) return;
    const GbaLane* T = lane_entry(tab, blockIdx.y);
    const GbaWork W = gba_lane_work(T, Wb);
    gba_edge_linearize_one(blockIdx.x * blockDim.x + threadIdx.x, gba_lane_dev(T, B), C, init, W.P0, W.P1, W.eres, W.eJi, W.eJj, W.cost + (size_t)2 * T->P);
}

__global__ __launch_bounds__(256) void k_gba_landmark_b(const GbaLane* __restrict__ tab, const PgoCtl* __restrict__ ctl, GbaDev B, GbaWork Wb, int* __restrict__ flagLm) {
    const PgoCtl* C = ctl + blockIdx.y;
    if (!C->active) return;
    const GbaLane* T = lane_entry(tab, blockIdx.y);
    const GbaWork W = gba_lane_work(T, Wb);
    gba_landmark_one(blockIdx.x * blockDim.x + threadIdx.x, gba_lane_dev(T, B), C, W.Jl, W.res, W.Hinv, W.gl, flagLm + blockIdx.y);
}

__global__ __launch_bounds__(256) void k_gba_wy_b(const GbaLane* __restrict__ tab, const PgoCtl* __restrict__ ctl, GbaDev B, GbaWork Wb) {
    const PgoCtl* C = ctl + blockIdx.y;
    if (!C->active) return;
    const GbaLane* T = lane_entry(tab, blockIdx.y);
    const GbaWork W = gba_lane_work(T, Wb);
    gba_wy_pair(blockIdx.x * blockDim.x + threadIdx.x, gba_lane_dev(T, B), C, W.Jp, W.Jl, W.Hinv, W.W, W.Y);
}

__global__ __launch_bounds__(64) void k_gba_edge_columns_b(const GbaLane* __restrict__ tab, const PgoCtl* __restrict__ ctl, GbaDev B, GbaWork Wb) {
    const PgoCtl* C = ctl + blockIdx.y;
    if (!C->active) return;
    const GbaLane* T = lane_entry(tab, blockIdx.y);
    const GbaWork W = gba_lane_work(T, Wb);
    gba_edge_column(blockIdx.x, threadIdx.x, gba_lane_dev(T, B), C, W.eres, W.eJi, W.eJj, W.bandH, W.diagH, W.g);
}

__global__ __launch_bounds__(64) void k_gba_gather_b(const GbaLane* __restrict__ tab, const PgoCtl* __restrict__ ctl, GbaDev B, GbaWork Wb) {
    const PgoCtl* C = ctl + blockIdx.y;
    if (!C->active) return;
    const GbaLane* T = lane_entry(tab, blockIdx.y);
    const GbaWork W = gba_lane_work(T, Wb);
    gba_gather_block(blockIdx.x, threadIdx.x, gba_lane_dev(T, B), C, W.Jp, W.res, W.W, W.Y, W.gl, W.bandH, W.diagH, W.g);
}

__global__ __launch_bounds__(256) void k_gba_band_copy_b(const GbaLane* __restrict__ tab, const PgoCtl* __restrict__ ctl, GbaDev B, GbaWork Wb) {
    const PgoCtl* C = ctl + blockIdx.y;
    if (!C->active) return;
    const GbaLane* T = lane_entry(tab, blockIdx.y);
    const GbaWork W = gba_lane_work(T, Wb);
    gba_band_copy_one((size_t)blockIdx.x * blockDim.x + threadIdx.x, gba_lane_dev(T, B), C, W.bandH, W.g, W.bandL, W.rhs);
}

// one workgroup per lane: the walk on the lane's band with the lane's n_free, b and lambda
__global__ __launch_bounds__(PGO_CHOL_NT) void k_gba_band_chol_b(const GbaLane* __restrict__ tab, const PgoCtl* __restrict__ ctl, GbaWork Wb,
                                                                 int* __restrict__ flagChol) {
    const PgoCtl* C = ctl + blockIdx.x;
    if (!C->active) return;
    const GbaLane* T = lane_entry(tab, blockIdx.x);
    const GbaWork W = gba_lane_work(T, Wb);
    pgo_band_chol_walk(T->nf, T->b, C->lambda, W.bandL, W.diagH, W.rhs, W.delta, flagChol + blockIdx.x);
}

__global__ __launch_bounds__(256) void k_gba_back_b(const GbaLane* __restrict__ tab, const PgoCtl* __restrict__ ctl, GbaDev B, GbaWork Wb) {
    const PgoCtl* C = ctl + blockIdx.y;
    if (!C->active) return;
    const GbaLane* T = lane_entry(tab, blockIdx.y);
    const GbaWork W = gba_lane_work(T, Wb);
    gba_back_one(blockIdx.x * blockDim.x + threadIdx.x, gba_lane_dev(T, B), C, W.W, W.Hinv, W.gl, W.L0, W.L1, W.delta);
}

__global__ __launch_bounds__(256) void k_gba_retract_b(const GbaLane* __restrict__ tab, const PgoCtl* __restrict__ ctl, GbaDev B, GbaWork Wb) {
    const PgoCtl* C = ctl + blockIdx.y;
    if (!C->active) return;
    const GbaLane* T = lane_entry(tab, blockIdx.y);
    const GbaWork W = gba_lane_work(T, Wb);
    gba_retract_one(blockIdx.x * blockDim.x + threadIdx.x, gba_lane_dev(T, B), C, W.P0, W.P1, W.delta);
}

__global__ __launch_bounds__(256) void k_gba_cost_b(const GbaLane* __restrict__ tab, const PgoCtl* __restrict__ ctl, GbaDev B, GbaWork Wb) {
    const PgoCtl* C = ctl + blockIdx.y;
    if (!C->active) return;
    const GbaLane* T = lane_entry(tab, blockIdx.y);
    const GbaWork W = gba_lane_work(T, Wb);
    gba_cost_slot(blockIdx.x * blockDim.x + threadIdx.x, gba_lane_dev(T, B), C, W.P0, W.P1, W.L0, W.L1, W.cost);
}

__global__ __launch_bounds__(256) void k_gba_edge_cost_b(const GbaLane* __restrict__ tab, const PgoCtl* __restrict__ ctl, GbaDev B, GbaWork Wb) {
    const PgoCtl* C = ctl + blockIdx.y;
    if (!C->active) return;
    const GbaLane* T = lane_entry(tab, blockIdx.y);
    const GbaWork W = gba_lane_work(T, Wb);
    gba_edge_cost_one(blockIdx.x * blockDim.x + threadIdx.x, gba_lane_dev(T, B), C, W.P0, W.P1, W.cost + (size_t)2 * T->P);
}

// out[2 lane], out[2 lane + 1]: the lane's 2 P + M cost terms summed in the single call's order, and |delta|_inf over its 6 nf + 3 L
// steps (init: every lane's initial cost, no delta yet)
__global__ __launch_bounds__(PGO_RED_NT) void k_gba_reduce_b(const GbaLane* __restrict__ tab, const PgoCtl* __restrict__ ctl, int init, GbaWork Wb,
                                                             double* __restrict__ out) {
    __shared__ double sS[PGO_RED_NT], sM[PGO_RED_NT];
    if (!init && !ctl[blockIdx.x].active) return;
    const GbaLane* T = lane_entry(tab, blockIdx.x);
    const GbaWork W = gba_lane_work(T, Wb);
    pgo_reduce_sum(threadIdx.x, 2 * T->P + T->M, W.cost, init ? 0 : T->nf * 6 + T->L * 3, W.delta, out + 2 * (size_t)blockIdx.x, sS, sM);
}

// The accept / reject rule, one thread per lane (what thread 0 of k_gba_reduce_decide does for the single call).
// *nActive: what the host reads once per round.
__global__ __launch_bounds__(GBA_MAX_LANES) void k_gba_decide_b(int lanes, int init, int maxIt, const GbaLane* __restrict__ tab,
                                                                PgoCtl* __restrict__ ctl, const double* __restrict__ out,
                                                                int* __restrict__ flagChol, int* __restrict__ flagLm, int* __restrict__ nActive) {
    const int l = threadIdx.x;
    int act = 0;
    if (l < lanes) {
        PgoCtl c = ctl[l];
        if (init) {
            c.cost = c.initial_cost = out[2 * l];
            c.active = (c.cost > 1e-20) && tab[l].hasUnknowns;
            c.need_linearize = PGO_NEED_H;
            flagChol[l] = 0; flagLm[l] = 0;
            ctl[l] = c;
        } else if (c.active) {
            pgo_lm_decide(c, out[2 * l], out[2 * l + 1], flagChol[l] | flagLm[l], maxIt);
            flagLm[l] = 0;
            ctl[l] = c;
        }
        act = c.active;
    }
    const int cnt = __syncthreads_count(act);
    if (threadIdx.x == 0) *nActive = cnt;
}

__global__ __launch_bounds__(256) void k_gba_chi2_b(const GbaLane* __restrict__ tab, const PgoCtl* __restrict__ ctl, GbaDev B, GbaWork Wb) {
    const GbaLane* T = lane_entry(tab, blockIdx.y);
    const GbaWork W = gba_lane_work(T, Wb);
    gba_chi2_pair(blockIdx.x * blockDim.x + threadIdx.x, gba_lane_dev(T, B), ctl + blockIdx.y, W.P0, W.P1, W.L0, W.L1, W.wrong);
}

// (the host side of a call - checks, plan, device forms, write-out - is gba_call.hpp, shared with gba_yaw.hip)

}  // namespace

thread_local std::vector<std::pair<const char*, float>> vslam::g_gbaTimes;
thread_local bool vslam::g_gbaTimingOn = false;

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
    int maxIt = 0;
    double lambda0 = 0.0;
    VS_CHECK(gba_check_params(who, params, &maxIt, &lambda0));
    const int K = Q.n_kf, L = Q.n_lm, P = Q.n_pairs, M = n_edges;
    VS_CHECK(gba_check_args(who, Q, edges, M, result));
    GbaPrep prep;
    VS_CHECK(gba_prepare(who, Q, edges, M, prep));
    const GbaPlan& G = prep.G;
    std::vector<double>& hp = prep.hp;
    const std::vector<double>& his = prep.his; const std::vector<double>& hthr = prep.hthr;
    const std::vector<PgoEdge>& he = prep.he;
    const int nf = G.nf, b = G.b;

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
    // nothing is written before the last wait has returned
    gba_write_out(Q, G, hp.data(), hl.data(), hw.data(), ctl, result);
    return VSLAM_OK;
}

// Several problems (lanes) at once: one launch per stage for all of them, in the layout of pgo_solve (pgo.hip).  Host work per
// lane is gba_check_args and gba_prepare, exactly the single call's; the lanes' arrays then go up as ONE block (table, control
// blocks, the problems' and the plans' arrays) and the device's own arrays are one more block from the thread's cache.  A round is
// one trial of every active lane and ends with one wait, for a single int (how many lanes are still active).  Nothing is written
// before the last wait has returned, so a refusal leaves every lane's outputs alone.
extern "C" vslam_status vslam_global_ba_batch(const vslam_gba_lane* lanes, int32_t n_lanes, const vslam_gba_params* params, int32_t device) {
    static const char* const who = "vslam_global_ba_batch";
    if (!lanes || n_lanes < 1) { set_error("%s: invalid arguments", who); return VSLAM_ERR_INVALID; }
    if (n_lanes > GBA_MAX_LANES) { set_error("%s: %d lanes exceed the limit (%d)", who, n_lanes, GBA_MAX_LANES); return VSLAM_ERR_CAPACITY; }
    int maxIt = 0;
    double lambda0 = 0.0;
    VS_CHECK(gba_check_params(who, params, &maxIt, &lambda0));
    char lw[96];
    auto lane_text = [&](int g) { snprintf(lw, sizeof lw, "%s: lane %d", who, g); return lw; };
    std::vector<int> live;                  // the lanes that hold a problem, in call order: the device's lanes
    std::vector<GbaLaneShape> shape;
    for (int g = 0; g < n_lanes; g++) {
        const vslam_gba_lane& Ln = lanes[g];
        if (!Ln.problem || Ln.problem->n_kf == 0) continue;
        if (!Ln.result) { set_error("%s: no result", lane_text(g)); return VSLAM_ERR_INVALID; }
        VS_CHECK(gba_check_args(lane_text(g), *Ln.problem, Ln.edges, Ln.n_edges, Ln.result));
        GbaLaneShape S;
        S.K = Ln.problem->n_kf; S.L = Ln.problem->n_lm; S.P = Ln.problem->n_pairs; S.M = Ln.n_edges;
        shape.push_back(S);
        live.push_back(g);
    }
    const int nl = (int)live.size();
    std::string err;
    if (const int st = gba_pack_check_sizes(shape.data(), nl, &err)) { set_error("%s: %s", who, err.c_str()); return (vslam_status)st; }
    std::vector<GbaPrep> prep(nl);
    for (int l = 0; l < nl; l++) {
        const vslam_gba_lane& Ln = lanes[live[l]];
        VS_CHECK(gba_prepare(lane_text(live[l]), *Ln.problem, Ln.edges, Ln.n_edges, prep[l]));
        const GbaPlan& G = prep[l].G;
        const auto& rig = Ln.problem->rig;
        GbaLaneShape& S = shape[l];
        S.nf = G.nf; S.b = G.b; S.nBlk = G.nBlk; S.nInc = G.rowStart[G.nf]; S.nLmPairs = G.lmStart[S.L]; S.nList = G.blkStart.back();
        S.hasUnknowns = (G.nf > 0 || G.nPresent > 0) ? 1 : 0;
        S.fx = rig.fx; S.fy = rig.fy; S.cx = rig.cx; S.cy = rig.cy; S.bl = (double)rig.baseline;
    }
    if (nl == 0) return VSLAM_OK;           // (every lane idle: nothing to solve, nothing written)
    std::vector<GbaLane> tab;
    GbaPackSums S;
    if (const int st = gba_pack(shape.data(), nl, tab, S, &err)) { set_error("%s: %s", who, err.c_str()); return (vslam_status)st; }

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available (no CPU fallback)"); return VSLAM_ERR_NO_DEVICE; }
    if (device < 0 || device >= ndev) { set_error("%s: no device %d", who, device); return VSLAM_ERR_INVALID; }
    VS_HIP(hipSetDevice(device));
    DevPool* pool = thread_pool(device);
    if (!pool) { set_error("no device pool"); return VSLAM_ERR_HIP; }
    pool->pending.clear();
    hipStream_t st = pool->stream;

    GbaLayout up, wk;                       // the upload block and the work block
    const size_t sK = (size_t)S.K, sL = (size_t)S.L, sP = (size_t)S.P, sM = (size_t)S.M, sF = (size_t)S.nf, sB = (size_t)S.band * 36 * 8;
    const size_t oTab = up.section(nl * sizeof(GbaLane)), oCtl = up.section(nl * sizeof(PgoCtl));
    const size_t oE = up.section(sM * sizeof(PgoEdge)), oP0 = up.section(sK * 96), oL0 = up.section(sL * 24);
    const size_t oPos = up.section(sK * 4), oRow = up.section((sF + nl) * 4), oInc = up.section((size_t)S.inc * 4);
    const size_t oPk = up.section(sP * 4), oPl = up.section(sP * 4), oPf = up.section(sP), oUv = up.section(sP * 16);
    const size_t oIs = up.section(sP * 16), oThr = up.section(sP * 16), oLoc = up.section(sK), oPres = up.section(sL);
    const size_t oLs = up.section((sL + nl) * 4), oLp = up.section((size_t)S.lp * 4);
    const size_t oBc = up.section((size_t)S.blk * 4), oBd = up.section((size_t)S.blk * 4), oBs = up.section(((size_t)S.blk + nl) * 4), oLi = up.section((size_t)S.list * 8);
    const size_t oP1 = wk.section(sK * 96), oL1 = wk.section(sL * 24);
    const size_t oJp = wk.section(sP * 24 * 8), oJl = wk.section(sP * 12 * 8), oRes = wk.section(sP * 4 * 8);
    const size_t oCost = wk.section((sP * 2 + sM) * 8), oERes = wk.section(sM * 48), oEJi = wk.section(sM * 288), oEJj = wk.section(sM * 288);
    const size_t oHinv = wk.section(sL * 72), oGl = wk.section(sL * 24), oW = wk.section(sP * 144), oY = wk.section(sP * 144);
    const size_t oBandH = wk.section(sB), oBandL = wk.section(sB), oDiag = wk.section(sF * 48), oG = wk.section(sF * 48), oRhs = wk.section(sF * 48);
    const size_t oDelta = wk.section(sF * 48 + sL * 24), oOut = wk.section((size_t)nl * 16), oFlagC = wk.section((size_t)nl * 4), oFlagL = wk.section((size_t)nl * 4);
    const size_t oAct = wk.section(4), oWrong = wk.section(sP);
    std::vector<uint8_t> hUp(up.bytes, 0);
    auto put = [&](size_t at, const void* src, size_t n) { if (n) memcpy(hUp.data() + at, src, n); };
    put(oTab, tab.data(), nl * sizeof(GbaLane));
    int maxK = 0, maxL = 0, maxP = 0, maxM = 0, maxNf = 0, maxBlk = 0;
    size_t maxBand = 0;                     // doubles of the largest lane's band
    for (int l = 0; l < nl; l++) {
        const vslam_ba_problem& Q = *lanes[live[l]].problem;
        const GbaPrep& R = prep[l];
        const GbaPlan& G = R.G;
        const GbaLane& T = tab[l];
        const size_t K = T.K, L = T.L, P = T.P, M = T.M, kf0 = T.kf0, lm0 = T.lm0, p0 = T.pair0, f0 = T.free0, b0 = T.blk0;
        PgoCtl c0{};
        c0.lambda = lambda0;
        put(oCtl + l * sizeof(PgoCtl), &c0, sizeof c0);
        put(oE + (size_t)T.edge0 * sizeof(PgoEdge), R.he.data(), M * sizeof(PgoEdge));
        put(oP0 + kf0 * 96, R.hp.data(), K * 96); put(oL0 + lm0 * 24, Q.lm_xyz, L * 24);
        put(oPos + kf0 * 4, G.pos.data(), K * 4); put(oRow + (f0 + l) * 4, G.rowStart.data(), (size_t)(G.nf + 1) * 4);
        put(oInc + (size_t)T.inc0 * 4, G.inc.data(), (size_t)G.rowStart[G.nf] * 4);
        put(oPk + p0 * 4, Q.pair_kf, P * 4); put(oPl + p0 * 4, Q.pair_lm, P * 4); put(oPf + p0, Q.pair_flags, P); put(oUv + p0 * 16, Q.pair_uv, P * 16);
        put(oIs + p0 * 16, R.his.data(), P * 16); put(oThr + p0 * 16, R.hthr.data(), P * 16);
        put(oLoc + kf0, Q.kf_local, K); put(oPres + lm0, G.lmPresent.data(), L);
        put(oLs + (lm0 + l) * 4, G.lmStart.data(), (L + 1) * 4); put(oLp + (size_t)T.lp0 * 4, G.lmPairs.data(), (size_t)G.lmStart[L] * 4);
        put(oBc + b0 * 4, G.blkC.data(), (size_t)G.nBlk * 4); put(oBd + b0 * 4, G.blkD.data(), (size_t)G.nBlk * 4);
        put(oBs + (b0 + l) * 4, G.blkStart.data(), (size_t)(G.nBlk + 1) * 4);
        put(oLi + (size_t)T.list0 * 8, G.list.data(), (size_t)G.blkStart.back() * 8);
        maxK = std::max(maxK, T.K); maxL = std::max(maxL, T.L); maxP = std::max(maxP, T.P); maxM = std::max(maxM, T.M);
        maxNf = std::max(maxNf, T.nf); maxBlk = std::max(maxBlk, T.nBlk);
        maxBand = std::max(maxBand, (size_t)(T.b + 1) * T.nf * 36);
    }
    PoolBuf<uint8_t> dUp(pool), dWk(pool);
    VS_HIP(dUp.up(hUp.data(), up.bytes)); VS_HIP(dWk.alloc(wk.bytes));
    GbaDev B{};                             // where the concatenated arrays begin (the sizes and the camera are the lanes')
    B.edges = (const PgoEdge*)(dUp.p + oE); B.pos = (const int*)(dUp.p + oPos); B.rowStart = (const int*)(dUp.p + oRow); B.inc = (const int*)(dUp.p + oInc);
    B.pairKf = (const int*)(dUp.p + oPk); B.pairLm = (const int*)(dUp.p + oPl); B.pairFlags = dUp.p + oPf; B.pairUv = (const float*)(dUp.p + oUv);
    B.pairIs = (const double*)(dUp.p + oIs); B.pairThr = (const double*)(dUp.p + oThr); B.kfLocal = dUp.p + oLoc; B.lmPresent = dUp.p + oPres;
    B.lmStart = (const int*)(dUp.p + oLs); B.lmPairs = (const int*)(dUp.p + oLp);
    B.blkC = (const int*)(dUp.p + oBc); B.blkD = (const int*)(dUp.p + oBd); B.blkStart = (const int*)(dUp.p + oBs); B.list = (const int*)(dUp.p + oLi);
    const GbaLane* dTab = (const GbaLane*)(dUp.p + oTab);
    PgoCtl* dCtl = (PgoCtl*)(dUp.p + oCtl);
    auto W8 = [&](size_t at) { return (double*)(dWk.p + at); };
    GbaWork Wb{};
    Wb.P0 = (double*)(dUp.p + oP0); Wb.L0 = (double*)(dUp.p + oL0); Wb.P1 = W8(oP1); Wb.L1 = W8(oL1);
    Wb.Jp = W8(oJp); Wb.Jl = W8(oJl); Wb.res = W8(oRes); Wb.cost = W8(oCost); Wb.eres = W8(oERes); Wb.eJi = W8(oEJi); Wb.eJj = W8(oEJj);
    Wb.Hinv = W8(oHinv); Wb.gl = W8(oGl); Wb.W = W8(oW); Wb.Y = W8(oY); Wb.bandH = W8(oBandH); Wb.bandL = W8(oBandL);
    Wb.diagH = W8(oDiag); Wb.g = W8(oG); Wb.rhs = W8(oRhs); Wb.delta = W8(oDelta); Wb.wrong = dWk.p + oWrong;
    double* dOut = W8(oOut);
    int* dFlagC = (int*)(dWk.p + oFlagC); int* dFlagL = (int*)(dWk.p + oFlagL); int* dAct = (int*)(dWk.p + oAct);

    struct TimerOwner { StageTimer t; ~TimerOwner() { t.destroy(); } } timerOwner;      // (the events go on every return path)
    StageTimer& timer = timerOwner.t;
    timer.stream = st; timer.multi = true; timer.enabled = g_gbaTimingOn;
    // grids are sized by the largest lane; a stage no lane has anything for is not launched
    const dim3 gSlot(gba_grid((size_t)2 * maxP), nl), gEdge(gba_grid(maxM), nl), gLm(gba_grid(maxL), nl), gPair(gba_grid(maxP), nl), gKf(gba_grid(maxK), nl), B256(256);
    int nActive = 0;
    auto linearize = [&](int init) {
        const int t = timer.begin("gba_linearize");
        if (maxP) hipLaunchKernelGGL(k_gba_linearize_b, gSlot, B256, 0, st, dTab, dCtl, init, B, Wb);
        if (maxM) hipLaunchKernelGGL(k_gba_edge_linearize_b, gEdge, B256, 0, st, dTab, dCtl, init, B, Wb);
        timer.end(t);
    };
    auto decide = [&](int init, int t) -> vslam_status {        // closes the gba_cost group `t`, then the round's one wait
        hipLaunchKernelGGL(k_gba_reduce_b, dim3(nl), dim3(PGO_RED_NT), 0, st, dTab, dCtl, init, Wb, dOut);
        hipLaunchKernelGGL(k_gba_decide_b, dim3(1), dim3(GBA_MAX_LANES), 0, st, nl, init, maxIt, dTab, dCtl, dOut, dFlagC, dFlagL, dAct);
        timer.end(t);
        VS_HIP(hipGetLastError());
        VS_HIP(pool->d2h(&nActive, dAct, sizeof(int)));
        VS_HIP(pool->sync());
        return VSLAM_OK;
    };
    linearize(1);
    VS_CHECK(decide(1, timer.begin("gba_cost")));
    while (nActive > 0) {       // one round
        linearize(0);
        int t = timer.begin("gba_landmarks");
        if (maxL) hipLaunchKernelGGL(k_gba_landmark_b, gLm, B256, 0, st, dTab, dCtl, B, Wb, dFlagL);
        if (maxP && maxNf) hipLaunchKernelGGL(k_gba_wy_b, gPair, B256, 0, st, dTab, dCtl, B, Wb);
        timer.end(t);
        t = timer.begin("gba_assemble");
        if (maxNf) hipLaunchKernelGGL(k_gba_edge_columns_b, dim3(maxNf, nl), dim3(64), 0, st, dTab, dCtl, B, Wb);
        if (maxBlk) hipLaunchKernelGGL(k_gba_gather_b, dim3(maxBlk, nl), dim3(64), 0, st, dTab, dCtl, B, Wb);
        timer.end(t);
        t = timer.begin("gba_band_chol");
        if (maxNf) hipLaunchKernelGGL(k_gba_band_copy_b, dim3(gba_grid(maxBand), nl), B256, 0, st, dTab, dCtl, B, Wb);
        hipLaunchKernelGGL(k_gba_band_chol_b, dim3(nl), dim3(PGO_CHOL_NT), 0, st, dTab, dCtl, Wb, dFlagC);
        timer.end(t);
        t = timer.begin("gba_back");
        if (maxL) hipLaunchKernelGGL(k_gba_back_b, gLm, B256, 0, st, dTab, dCtl, B, Wb);
        hipLaunchKernelGGL(k_gba_retract_b, gKf, B256, 0, st, dTab, dCtl, B, Wb);
        timer.end(t);
        t = timer.begin("gba_cost");
        if (maxP) hipLaunchKernelGGL(k_gba_cost_b, gSlot, B256, 0, st, dTab, dCtl, B, Wb);
        if (maxM) hipLaunchKernelGGL(k_gba_edge_cost_b, gEdge, B256, 0, st, dTab, dCtl, B, Wb);
        VS_CHECK(decide(0, t));
    }
    int t = timer.begin("gba_chi2");
    if (maxP) hipLaunchKernelGGL(k_gba_chi2_b, gPair, B256, 0, st, dTab, dCtl, B, Wb);
    timer.end(t);
    VS_HIP(hipGetLastError());
    std::vector<PgoCtl> ctl(nl);
    VS_HIP(pool->d2h(ctl.data(), dCtl, nl * sizeof(PgoCtl)));
    VS_HIP(pool->sync());
    std::vector<double> hl(std::max<size_t>(sL, 1) * 3);
    std::vector<uint8_t> hw(std::max<size_t>(sP, 1));
    for (int l = 0; l < nl; l++) {
        const GbaLane& T = tab[l];
        VS_HIP(pool->d2h(prep[l].hp.data(), (ctl[l].cur ? Wb.P1 : Wb.P0) + (size_t)T.kf0 * 12, (size_t)T.K * 96));
        if (T.L) VS_HIP(pool->d2h(hl.data() + (size_t)T.lm0 * 3, (ctl[l].cur ? Wb.L1 : Wb.L0) + (size_t)T.lm0 * 3, (size_t)T.L * 24));
    }
    if (sP) VS_HIP(pool->d2h(hw.data(), Wb.wrong, sP));
    VS_HIP(pool->sync());
    if (timer.enabled) {
        const char* names[8]; float ms[8];
        const int k = timer.read(names, ms, 8);
        g_gbaTimes.clear();
        for (int q = 0; q < k; q++) g_gbaTimes.push_back({names[q], ms[q]});
    }
    // nothing is written before the last wait has returned
    for (int l = 0; l < nl; l++) {
        const vslam_gba_lane& Ln = lanes[live[l]];
        gba_write_out(*Ln.problem, prep[l].G, prep[l].hp.data(), hl.data() + (size_t)tab[l].lm0 * 3, hw.data() + tab[l].pair0, ctl[l], Ln.result);
    }
    return VSLAM_OK;
}
