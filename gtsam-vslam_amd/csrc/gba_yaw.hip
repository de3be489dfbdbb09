// Global bundle adjustment with YAW-ONLY keyframes on the device (no reference counterpart; DESIGN.md section 6 item 30, restated
// by tests/gba_yaw_ref.py): the problem, factors, presence, gauge, Levenberg-Marquardt schedule, damping, flags, refusals and
// limits of gba.hip, but a free keyframe moves only by a rotation about ONE world axis g (gravity) and a world translation,
// T_k <- [Exp(theta g) R_k, t_k + delta]: what a stereo + IMU session needs from a global adjustment, whose roll and pitch the
// IMU observes.  The reduced camera system is block-banded with 4x4 fp64 blocks.
// There is ONE solve path, the lanes of vslam_global_ba_batch: one launch per stage for all problems, the lane as a grid
// dimension; vslam_global_ba_yaw is its one-lane case.  The host side (checks, plan, packing, write-out) is gba_call.hpp,
// gba_host.hpp and gba_pack_host.hpp, shared with gba.hip and counted in blocks; the device bodies are gba_yaw_dev.hpp and,
// unchanged, those of gba_dev.hpp, pgo_dev.hpp and pgo_yaw_dev.hpp.
//   k_gbay_linearize_b / k_gbay_edge_linearize_b   a thread per factor slot / per edge: the 6-DoF Jacobian in registers times M_k
//   k_gbay_landmark_b     gba_landmark_one, as it is
//   k_gbay_wy_b           a thread per pair on a free keyframe: W (4x3) and Y = W Hll^-1
//   k_gbay_edge_columns_b three block columns per wave (20 lanes each): the edges' blocks and gradient; it also clears the column
//   k_gbay_gather_b       three listed blocks per wave (20 lanes each), each walking its own (pair, pair) list; no atomics
//   k_gbay_band_copy_b / k_gbay_band_chol_b   H and g into the factor's arrays; one workgroup per lane walks the block columns
//   k_gbay_back_b / k_gbay_retract_b          the landmark steps; the trial poses
//   k_gbay_cost_b / k_gbay_edge_cost_b / k_gbay_reduce_b / k_gbay_decide_b   gba_cost_slot, gba_edge_cost_one, pgo_reduce_sum and
//                         pgo_lm_decide, as they are
//   k_gbay_chi2_b         gba_chi2_pair, as it is
// The host waits once per round, for one int.
#include "common.hpp"
#include "dmath.hpp"
#include "gba_host.hpp"
#include "gba_pack_host.hpp"
#include "gba_call.hpp"
#include "gba_yaw_dev.hpp"
#include <array>
#include <cmath>

using namespace vslam;

namespace {

struct GbayLane { GbaLane L; double g[3]; };      // free0 counts band positions (x 4), band0 blocks (x 16); g: the lane's unit axis

struct GbayWork {                   // the device's own arrays
    double *P0, *P1, *L0, *L1;      // both value buffers (P0 and L0 come up with the problem)
    double *Jp, *Jl, *res, *cost, *eres, *eJi, *eJj, *Hinv, *gl, *W, *Y, *bandH, *bandL, *diagH, *g, *rhs, *delta;
    uint8_t* wrong;
};

__device__ __forceinline__ GbayWork gbay_lane_work(const GbaLane* T, const GbayWork& B) {
    GbayWork W;
    const size_t kf0 = (size_t)T->kf0, lm0 = (size_t)T->lm0, p0 = (size_t)T->pair0, e0 = (size_t)T->edge0, f0 = (size_t)T->free0;
    W.P0 = B.P0 + kf0 * 12; W.P1 = B.P1 + kf0 * 12; W.L0 = B.L0 + lm0 * 3; W.L1 = B.L1 + lm0 * 3;
    W.Jp = B.Jp + p0 * 16; W.Jl = B.Jl + p0 * 12; W.res = B.res + p0 * 4; W.cost = B.cost + p0 * 2 + e0;
    W.eres = B.eres + e0 * 6; W.eJi = B.eJi + e0 * PGOY_JAC; W.eJj = B.eJj + e0 * PGOY_JAC;
    W.Hinv = B.Hinv + lm0 * 9; W.gl = B.gl + lm0 * 3; W.W = B.W + p0 * GBAY_WY; W.Y = B.Y + p0 * GBAY_WY;
    W.bandH = B.bandH + (size_t)T->band0 * PGOY_BLK; W.bandL = B.bandL + (size_t)T->band0 * PGOY_BLK;
    W.diagH = B.diagH + f0 * PGOY_D; W.g = B.g + f0 * PGOY_D; W.rhs = B.rhs + f0 * PGOY_D; W.delta = B.delta + f0 * PGOY_D + lm0 * 3;
    W.wrong = B.wrong + p0;
    return W;
}

// blockIdx.y (blockIdx.x of the one-workgroup-per-lane kernels) = lane.  A lane that has stopped costs a workgroup one load.
__global__ __launch_bounds__(256) void k_gbay_linearize_b(const GbayLane* __restrict__ tab, const PgoCtl* __restrict__ ctl, int init, GbaDev B, GbayWork Wb) {
    const PgoCtl* C = ctl + blockIdx.y;
    if (!init && !C->active) return;
    const GbayLane* Y = lane_entry(tab, blockIdx.y);
    const GbaLane* T = &Y->L;
    const GbayWork W = gbay_lane_work(T, Wb);
    const double g[3] = {Y->g[0], Y->g[1], Y->g[2]};
    gbay_linearize_slot(blockIdx.x * blockDim.x + threadIdx.x, gba_lane_dev(T, B), C, init, g, W.P0, W.P1, W.L0, W.L1, W.Jp, W.Jl, W.res, W.cost);
}

__global__ __launch_bounds__(256) void k_gbay_edge_linearize_b(const GbayLane* __restrict__ tab, const PgoCtl* __restrict__ ctl, int init, GbaDev B, GbayWork Wb) {
    const PgoCtl* C = ctl + blockIdx.y;
    if (!init && !C->active) return;
    const GbayLane* Y = lane_entry(tab, blockIdx.y);
    const GbaLane* T = &Y->L;
    const GbayWork W = gbay_lane_work(T, Wb);
    const double g[3] = {Y->g[0], Y->g[1], Y->g[2]};
    gbay_edge_linearize_one(blockIdx.x * blockDim.x + threadIdx.x, gba_lane_dev(T, B), C, init, g, W.P0, W.P1, W.eres, W.eJi, W.eJj, W.cost + (size_t)2 * T->P);
}

__global__ __launch_bounds__(256) void k_gbay_landmark_b(const GbayLane* __restrict__ tab, const PgoCtl* __restrict__ ctl, GbaDev B, GbayWork Wb, int* __restrict__ flagLm) {
    const PgoCtl* C = ctl + blockIdx.y;
    if (!C->active) return;
    const GbaLane* T = &lane_entry(tab, blockIdx.y)->L;
    const GbayWork W = gbay_lane_work(T, Wb);
    gba_landmark_one(blockIdx.x * blockDim.x + threadIdx.x, gba_lane_dev(T, B), C, W.Jl, W.res, W.Hinv, W.gl, flagLm + blockIdx.y);
}

__global__ __launch_bounds__(256) void k_gbay_wy_b(const GbayLane* __restrict__ tab, const PgoCtl* __restrict__ ctl, GbaDev B, GbayWork Wb) {
    const PgoCtl* C = ctl + blockIdx.y;
    if (!C->active) return;
    const GbaLane* T = &lane_entry(tab, blockIdx.y)->L;
    const GbayWork W = gbay_lane_work(T, Wb);
    gbay_wy_pair(blockIdx.x * blockDim.x + threadIdx.x, gba_lane_dev(T, B), C, W.Jp, W.Jl, W.Hinv, W.W, W.Y);
}

// blockIdx.x: a wave of three block columns 3 x .. 3 x + 2 (the last wave of a lane may hold one or two)
__global__ __launch_bounds__(64) void k_gbay_edge_columns_b(const GbayLane* __restrict__ tab, const PgoCtl* __restrict__ ctl, GbaDev B, GbayWork Wb) {
    const PgoCtl* C = ctl + blockIdx.y;
    if (!C->active) return;
    const int lane = threadIdx.x;
    if (lane >= PGOY_COLS_PER_WAVE * PGOY_COL_LANES) return;
    const GbaLane* T = &lane_entry(tab, blockIdx.y)->L;
    const GbayWork W = gbay_lane_work(T, Wb);
    gbay_edge_column(blockIdx.x * PGOY_COLS_PER_WAVE + lane / PGOY_COL_LANES, lane % PGOY_COL_LANES, gba_lane_dev(T, B), C, W.eres, W.eJi, W.eJj, W.bandH, W.diagH, W.g);
}

// blockIdx.x: a wave of three listed blocks 3 x .. 3 x + 2
__global__ __launch_bounds__(64) void k_gbay_gather_b(const GbayLane* __restrict__ tab, const PgoCtl* __restrict__ ctl, GbaDev B, GbayWork Wb) {
    const PgoCtl* C = ctl + blockIdx.y;
    if (!C->active) return;
    const int lane = threadIdx.x;
    if (lane >= GBAY_BLKS_PER_WAVE * GBAY_BLK_LANES) return;
    const GbaLane* T = &lane_entry(tab, blockIdx.y)->L;
    const GbayWork W = gbay_lane_work(T, Wb);
    gbay_gather_block(blockIdx.x * GBAY_BLKS_PER_WAVE + lane / GBAY_BLK_LANES, lane % GBAY_BLK_LANES, gba_lane_dev(T, B), C, W.Jp, W.res, W.W, W.Y, W.gl, W.bandH,
                      W.diagH, W.g);
}

__global__ __launch_bounds__(256) void k_gbay_band_copy_b(const GbayLane* __restrict__ tab, const PgoCtl* __restrict__ ctl, GbaDev B, GbayWork Wb) {
    const PgoCtl* C = ctl + blockIdx.y;
    if (!C->active) return;
    const GbaLane* T = &lane_entry(tab, blockIdx.y)->L;
    const GbayWork W = gbay_lane_work(T, Wb);
    gbay_band_copy_one((size_t)blockIdx.x * blockDim.x + threadIdx.x, gba_lane_dev(T, B), C, W.bandH, W.g, W.bandL, W.rhs);
}

// one workgroup per lane: the 4x4 walk on the lane's band with the lane's n_free, b and lambda
__global__ __launch_bounds__(PGO_CHOL_NT) void k_gbay_band_chol_b(const GbayLane* __restrict__ tab, const PgoCtl* __restrict__ ctl, GbayWork Wb,
                                                                  int* __restrict__ flagChol) {
    const PgoCtl* C = ctl + blockIdx.x;
    if (!C->active) return;
    const GbaLane* T = &lane_entry(tab, blockIdx.x)->L;
    const GbayWork W = gbay_lane_work(T, Wb);
    pgoy_band_chol_walk(T->nf, T->b, C->lambda, W.bandL, W.diagH, W.rhs, W.delta, flagChol + blockIdx.x);
}

__global__ __launch_bounds__(256) void k_gbay_back_b(const GbayLane* __restrict__ tab, const PgoCtl* __restrict__ ctl, GbaDev B, GbayWork Wb) {
    const PgoCtl* C = ctl + blockIdx.y;
    if (!C->active) return;
    const GbaLane* T = &lane_entry(tab, blockIdx.y)->L;
    const GbayWork W = gbay_lane_work(T, Wb);
    gbay_back_one(blockIdx.x * blockDim.x + threadIdx.x, gba_lane_dev(T, B), C, W.W, W.Hinv, W.gl, W.L0, W.L1, W.delta);
}

__global__ __launch_bounds__(256) void k_gbay_retract_b(const GbayLane* __restrict__ tab, const PgoCtl* __restrict__ ctl, GbaDev B, GbayWork Wb) {
    const PgoCtl* C = ctl + blockIdx.y;
    if (!C->active) return;
    const GbayLane* Y = lane_entry(tab, blockIdx.y);
    const GbaLane* T = &Y->L;
    const GbayWork W = gbay_lane_work(T, Wb);
    const double g[3] = {Y->g[0], Y->g[1], Y->g[2]};
    gbay_retract_one(blockIdx.x * blockDim.x + threadIdx.x, gba_lane_dev(T, B), C, g, W.P0, W.P1, W.delta);
}

__global__ __launch_bounds__(256) void k_gbay_cost_b(const GbayLane* __restrict__ tab, const PgoCtl* __restrict__ ctl, GbaDev B, GbayWork Wb) {
    const PgoCtl* C = ctl + blockIdx.y;
    if (!C->active) return;
    const GbaLane* T = &lane_entry(tab, blockIdx.y)->L;
    const GbayWork W = gbay_lane_work(T, Wb);
    gba_cost_slot(blockIdx.x * blockDim.x + threadIdx.x, gba_lane_dev(T, B), C, W.P0, W.P1, W.L0, W.L1, W.cost);
}

__global__ __launch_bounds__(256) void k_gbay_edge_cost_b(const GbayLane* __restrict__ tab, const PgoCtl* __restrict__ ctl, GbaDev B, GbayWork Wb) {
    const PgoCtl* C = ctl + blockIdx.y;
    if (!C->active) return;
    const GbaLane* T = &lane_entry(tab, blockIdx.y)->L;
    const GbayWork W = gbay_lane_work(T, Wb);
    gba_edge_cost_one(blockIdx.x * blockDim.x + threadIdx.x, gba_lane_dev(T, B), C, W.P0, W.P1, W.cost + (size_t)2 * T->P);
}

// out[2 lane], out[2 lane + 1]: the lane's 2 P + M cost terms summed in fixed order, and |delta|_inf over its 4 nf + 3 L steps
// (init: every lane's initial cost, no delta yet)
__global__ __launch_bounds__(PGO_RED_NT) void k_gbay_reduce_b(const GbayLane* __restrict__ tab, const PgoCtl* __restrict__ ctl, int init, GbayWork Wb,
                                                              double* __restrict__ out) {
    __shared__ double sS[PGO_RED_NT], sM[PGO_RED_NT];
    if (!init && !ctl[blockIdx.x].active) return;
    const GbaLane* T = &lane_entry(tab, blockIdx.x)->L;
    const GbayWork W = gbay_lane_work(T, Wb);
    pgo_reduce_sum(threadIdx.x, 2 * T->P + T->M, W.cost, init ? 0 : T->nf * PGOY_D + T->L * 3, W.delta, out + 2 * (size_t)blockIdx.x, sS, sM);
}

// The accept / reject rule (pgo_lm_decide), one thread per lane.  *nActive: what the host reads once per round.
__global__ __launch_bounds__(GBA_MAX_LANES) void k_gbay_decide_b(int lanes, int init, int maxIt, const GbayLane* __restrict__ tab,
                                                                 PgoCtl* __restrict__ ctl, const double* __restrict__ out,
                                                                 int* __restrict__ flagChol, int* __restrict__ flagLm, int* __restrict__ nActive) {
    const int l = threadIdx.x;
    int act = 0;
    if (l < lanes) {
        PgoCtl c = ctl[l];
        if (init) {
            c.cost = c.initial_cost = out[2 * l];
            c.active = (c.cost > 1e-20) && tab[l].L.hasUnknowns;
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

__global__ __launch_bounds__(256) void k_gbay_chi2_b(const GbayLane* __restrict__ tab, const PgoCtl* __restrict__ ctl, GbaDev B, GbayWork Wb) {
    const GbaLane* T = &lane_entry(tab, blockIdx.y)->L;
    const GbayWork W = gbay_lane_work(T, Wb);
    gba_chi2_pair(blockIdx.x * blockDim.x + threadIdx.x, gba_lane_dev(T, B), ctl + blockIdx.y, W.P0, W.P1, W.L0, W.L1, W.wrong);
}

// g = axis / |axis| in fp64 (the expression of pgo_yaw.hip); a zero or non-finite axis is refused
vslam_status gbay_axis(const char* who, const double* axis, double* g) {
    const double x = axis[0], y = axis[1], z = axis[2];
    const double nrm = std::sqrt(x * x + y * y + z * z);
    if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(z) || !std::isfinite(nrm) || !(nrm > 0.0)) {
        set_error("%s: the axis is zero or not finite", who); return VSLAM_ERR_INVALID;
    }
    g[0] = x / nrm; g[1] = y / nrm; g[2] = z / nrm;
    return VSLAM_OK;
}

// The one solve path.  Host work per lane is gba_check_args, the axis and gba_prepare; the lanes' arrays then go up as ONE block
// (table, control blocks, the problems' and the plans' arrays) and the device's own arrays are one more block from the thread's
// cache.  A round is one trial of every active lane and ends with one wait, for a single int.  Nothing is written before the last
// wait has returned, so a refusal leaves every lane's outputs alone.  batched: a lane without a problem is idle and the error
// texts name the lane; otherwise (the single call) there is one lane, which must hold a problem.
vslam_status gbay_solve(const char* who, bool batched, const vslam_gba_yaw_lane* lanes, int n_lanes, int maxIt, double lambda0, int device) {
    char lw[96];
    auto lane_text = [&](int g) { if (!batched) return who; snprintf(lw, sizeof lw, "%s: lane %d", who, g); return (const char*)lw; };
    std::vector<int> live;                  // the lanes that hold a problem, in call order: the device's lanes
    std::vector<GbaLaneShape> shape;
    std::vector<std::array<double, 3>> axes;
    for (int g = 0; g < n_lanes; g++) {
        const vslam_gba_lane& Ln = lanes[g].lane;
        if (batched && (!Ln.problem || Ln.problem->n_kf == 0)) continue;
        if (!Ln.result) { set_error("%s: no result", lane_text(g)); return VSLAM_ERR_INVALID; }
        VS_CHECK(gba_check_args(lane_text(g), *Ln.problem, Ln.edges, Ln.n_edges, Ln.result));
        std::array<double, 3> ax;
        VS_CHECK(gbay_axis(lane_text(g), lanes[g].axis, ax.data()));
        GbaLaneShape S;
        S.K = Ln.problem->n_kf; S.L = Ln.problem->n_lm; S.P = Ln.problem->n_pairs; S.M = Ln.n_edges;
        shape.push_back(S);
        axes.push_back(ax);
        live.push_back(g);
    }
    const int nl = (int)live.size();
    std::string err;
    if (const int st = gba_pack_check_sizes(shape.data(), nl, &err)) { set_error("%s: %s", who, err.c_str()); return (vslam_status)st; }
    std::vector<GbaPrep> prep(nl);
    for (int l = 0; l < nl; l++) {
        const vslam_gba_lane& Ln = lanes[live[l]].lane;
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
    std::vector<GbayLane> ytab(nl);
    for (int l = 0; l < nl; l++) { ytab[l].L = tab[l]; for (int k = 0; k < 3; k++) ytab[l].g[k] = axes[l][k]; }

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available (no CPU fallback)"); return VSLAM_ERR_NO_DEVICE; }
    if (device < 0 || device >= ndev) { set_error("%s: no device %d", who, device); return VSLAM_ERR_INVALID; }
    VS_HIP(hipSetDevice(device));
    DevPool* pool = thread_pool(device);
    if (!pool) { set_error("no device pool"); return VSLAM_ERR_HIP; }
    pool->pending.clear();
    hipStream_t st = pool->stream;

    GbaLayout up, wk;                       // the upload block and the work block
    const size_t sK = (size_t)S.K, sL = (size_t)S.L, sP = (size_t)S.P, sM = (size_t)S.M, sF = (size_t)S.nf, sB = (size_t)S.band * PGOY_BLK * 8;
    const size_t oTab = up.section(nl * sizeof(GbayLane)), oCtl = up.section(nl * sizeof(PgoCtl));
    const size_t oE = up.section(sM * sizeof(PgoEdge)), oP0 = up.section(sK * 96), oL0 = up.section(sL * 24);
    const size_t oPos = up.section(sK * 4), oRow = up.section((sF + nl) * 4), oInc = up.section((size_t)S.inc * 4);
    const size_t oPk = up.section(sP * 4), oPl = up.section(sP * 4), oPf = up.section(sP), oUv = up.section(sP * 16);
    const size_t oIs = up.section(sP * 16), oThr = up.section(sP * 16), oLoc = up.section(sK), oPres = up.section(sL);
    const size_t oLs = up.section((sL + nl) * 4), oLp = up.section((size_t)S.lp * 4);
    const size_t oBc = up.section((size_t)S.blk * 4), oBd = up.section((size_t)S.blk * 4), oBs = up.section(((size_t)S.blk + nl) * 4), oLi = up.section((size_t)S.list * 8);
    const size_t vec = sF * PGOY_D * 8;
    const size_t oP1 = wk.section(sK * 96), oL1 = wk.section(sL * 24);
    const size_t oJp = wk.section(sP * 16 * 8), oJl = wk.section(sP * 12 * 8), oRes = wk.section(sP * 4 * 8);
    const size_t oCost = wk.section((sP * 2 + sM) * 8), oERes = wk.section(sM * 48), oEJi = wk.section(sM * PGOY_JAC * 8), oEJj = wk.section(sM * PGOY_JAC * 8);
    const size_t oHinv = wk.section(sL * 72), oGl = wk.section(sL * 24), oW = wk.section(sP * GBAY_WY * 8), oY = wk.section(sP * GBAY_WY * 8);
    const size_t oBandH = wk.section(sB), oBandL = wk.section(sB), oDiag = wk.section(vec), oG = wk.section(vec), oRhs = wk.section(vec);
    const size_t oDelta = wk.section(vec + sL * 24), oOut = wk.section((size_t)nl * 16), oFlagC = wk.section((size_t)nl * 4), oFlagL = wk.section((size_t)nl * 4);
    const size_t oAct = wk.section(4), oWrong = wk.section(sP);
    std::vector<uint8_t> hUp(up.bytes, 0);
    auto put = [&](size_t at, const void* src, size_t n) { if (n) memcpy(hUp.data() + at, src, n); };
    put(oTab, ytab.data(), nl * sizeof(GbayLane));
    int maxK = 0, maxL = 0, maxP = 0, maxM = 0, maxNf = 0, maxBlk = 0;
    size_t maxBand = 0;                     // doubles of the largest lane's band
    for (int l = 0; l < nl; l++) {
        const vslam_ba_problem& Q = *lanes[live[l]].lane.problem;
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
        maxBand = std::max(maxBand, (size_t)(T.b + 1) * T.nf * PGOY_BLK);
    }
    PoolBuf<uint8_t> dUp(pool), dWk(pool);
    VS_HIP(dUp.up(hUp.data(), up.bytes)); VS_HIP(dWk.alloc(wk.bytes));
    GbaDev B{};                             // where the concatenated arrays begin (the sizes and the camera are the lanes')
    B.edges = (const PgoEdge*)(dUp.p + oE); B.pos = (const int*)(dUp.p + oPos); B.rowStart = (const int*)(dUp.p + oRow); B.inc = (const int*)(dUp.p + oInc);
    B.pairKf = (const int*)(dUp.p + oPk); B.pairLm = (const int*)(dUp.p + oPl); B.pairFlags = dUp.p + oPf; B.pairUv = (const float*)(dUp.p + oUv);
    B.pairIs = (const double*)(dUp.p + oIs); B.pairThr = (const double*)(dUp.p + oThr); B.kfLocal = dUp.p + oLoc; B.lmPresent = dUp.p + oPres;
    B.lmStart = (const int*)(dUp.p + oLs); B.lmPairs = (const int*)(dUp.p + oLp);
    B.blkC = (const int*)(dUp.p + oBc); B.blkD = (const int*)(dUp.p + oBd); B.blkStart = (const int*)(dUp.p + oBs); B.list = (const int*)(dUp.p + oLi);
    const GbayLane* dTab = (const GbayLane*)(dUp.p + oTab);
    PgoCtl* dCtl = (PgoCtl*)(dUp.p + oCtl);
    auto W8 = [&](size_t at) { return (double*)(dWk.p + at); };
    GbayWork Wb{};
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
    const dim3 gCols((maxNf + PGOY_COLS_PER_WAVE - 1) / PGOY_COLS_PER_WAVE, nl), gBlks((maxBlk + GBAY_BLKS_PER_WAVE - 1) / GBAY_BLKS_PER_WAVE, nl);
    int nActive = 0;
    auto linearize = [&](int init) {
        const int t = timer.begin("gba_linearize");
        if (maxP) hipLaunchKernelGGL(k_gbay_linearize_b, gSlot, B256, 0, st, dTab, dCtl, init, B, Wb);
        if (maxM) hipLaunchKernelGGL(k_gbay_edge_linearize_b, gEdge, B256, 0, st, dTab, dCtl, init, B, Wb);
        timer.end(t);
    };
    auto decide = [&](int init, int t) -> vslam_status {        // closes the gba_cost group `t`, then the round's one wait
        hipLaunchKernelGGL(k_gbay_reduce_b, dim3(nl), dim3(PGO_RED_NT), 0, st, dTab, dCtl, init, Wb, dOut);
        hipLaunchKernelGGL(k_gbay_decide_b, dim3(1), dim3(GBA_MAX_LANES), 0, st, nl, init, maxIt, dTab, dCtl, dOut, dFlagC, dFlagL, dAct);
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
        if (maxL) hipLaunchKernelGGL(k_gbay_landmark_b, gLm, B256, 0, st, dTab, dCtl, B, Wb, dFlagL);
        if (maxP && maxNf) hipLaunchKernelGGL(k_gbay_wy_b, gPair, B256, 0, st, dTab, dCtl, B, Wb);
        timer.end(t);
        t = timer.begin("gba_assemble");
        if (maxNf) hipLaunchKernelGGL(k_gbay_edge_columns_b, gCols, dim3(64), 0, st, dTab, dCtl, B, Wb);
        if (maxBlk) hipLaunchKernelGGL(k_gbay_gather_b, gBlks, dim3(64), 0, st, dTab, dCtl, B, Wb);
        timer.end(t);
        t = timer.begin("gba_band_chol");
        if (maxNf) hipLaunchKernelGGL(k_gbay_band_copy_b, dim3(gba_grid(maxBand), nl), B256, 0, st, dTab, dCtl, B, Wb);
        hipLaunchKernelGGL(k_gbay_band_chol_b, dim3(nl), dim3(PGO_CHOL_NT), 0, st, dTab, dCtl, Wb, dFlagC);
        timer.end(t);
        t = timer.begin("gba_back");
        if (maxL) hipLaunchKernelGGL(k_gbay_back_b, gLm, B256, 0, st, dTab, dCtl, B, Wb);
        hipLaunchKernelGGL(k_gbay_retract_b, gKf, B256, 0, st, dTab, dCtl, B, Wb);
        timer.end(t);
        t = timer.begin("gba_cost");
        if (maxP) hipLaunchKernelGGL(k_gbay_cost_b, gSlot, B256, 0, st, dTab, dCtl, B, Wb);
        if (maxM) hipLaunchKernelGGL(k_gbay_edge_cost_b, gEdge, B256, 0, st, dTab, dCtl, B, Wb);
        VS_CHECK(decide(0, t));
    }
    int t = timer.begin("gba_chi2");
    if (maxP) hipLaunchKernelGGL(k_gbay_chi2_b, gPair, B256, 0, st, dTab, dCtl, B, Wb);
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
        const vslam_gba_lane& Ln = lanes[live[l]].lane;
        gba_write_out(*Ln.problem, prep[l].G, prep[l].hp.data(), hl.data() + (size_t)tab[l].lm0 * 3, hw.data() + tab[l].pair0, ctl[l], Ln.result);
    }
    return VSLAM_OK;
}

}  // namespace

// the one-lane case of the batched call (no idle lane: a missing problem is refused; its error texts name no lane)
extern "C" vslam_status vslam_global_ba_yaw(const vslam_ba_problem* problem, const vslam_pgo_edge* edges, int32_t n_edges, const double* axis,
                                            const vslam_gba_params* params, int32_t device, vslam_gba_result* result) {
    static const char* const who = "vslam_global_ba_yaw";
    if (!problem || !result || !axis) { set_error("%s: invalid arguments", who); return VSLAM_ERR_INVALID; }
    int maxIt = 0;
    double lambda0 = 0.0;
    VS_CHECK(gba_check_params(who, params, &maxIt, &lambda0));
    const vslam_gba_yaw_lane lane{{problem, edges, n_edges, result}, {axis[0], axis[1], axis[2]}};
    return gbay_solve(who, false, &lane, 1, maxIt, lambda0, device);
}

extern "C" vslam_status vslam_global_ba_yaw_batch(const vslam_gba_yaw_lane* lanes, int32_t n_lanes, const vslam_gba_params* params, int32_t device) {
    static const char* const who = "vslam_global_ba_yaw_batch";
    if (!lanes || n_lanes < 1) { set_error("%s: invalid arguments", who); return VSLAM_ERR_INVALID; }
    if (n_lanes > GBA_MAX_LANES) { set_error("%s: %d lanes exceed the limit (%d)", who, n_lanes, GBA_MAX_LANES); return VSLAM_ERR_CAPACITY; }
    int maxIt = 0;
    double lambda0 = 0.0;
    VS_CHECK(gba_check_params(who, params, &maxIt, &lambda0));
    return gbay_solve(who, true, lanes, n_lanes, maxIt, lambda0, device);
}
