// Yaw-only (4-DoF) pose-graph optimisation on the device (no reference counterpart; DESIGN.md section 6 item 29, restated by
// tests/pgo_yaw_ref.py): the graph, residual, cost, weights, Levenberg-Marquardt schedule, refusals and report of pgo.hip, but
// every free pose moves only by a rotation about ONE world axis g (gravity) and a world translation,
// T_k <- [Exp(theta g) R_k, t_k + delta].  Roll and pitch about g stay exactly as they are: what a session with an IMU needs
// from a loop correction.  The damped normal equations are block-banded with 4x4 fp64 blocks.
// There is ONE solve path, pgo_solve of pgo_host.hpp with the kernel set below, the lanes of pgo.hip: one launch per stage for
// all graphs, blockIdx = lane;
// vslam_pose_graph_optimize_yaw is its one-lane case.  The host side (validation, gauge check, reverse Cuthill-McKee, packing) is
// pgo_host.hpp, shared with pgo.hip; the device bodies are pgo_yaw_dev.hpp and, unchanged, those of pgo_dev.hpp.
//   k_pgoy_linearize_b   one thread per edge: the 6-DoF linearisation in registers, times M_i and M_j: two 6x4 Jacobians
//   k_pgoy_assemble_b    three block columns per wave (20 lanes each), each a gather over its own incidence list; no atomics
//   k_pgoy_band_copy_b / k_pgoy_band_chol_b   H and g into the factor's arrays; one workgroup per lane walks the block columns
//   k_pgoy_retract_b / k_pgoy_cost_b / k_pgoy_reduce_b / k_pgoy_decide_b   trial poses, cost (pgo_cost_edge), the fixed-order sum
//                        (pgo_reduce_sum) and the accept / reject rule (pgo_lm_decide)
// The host waits once per round, for one int.
#include "common.hpp"
#include "dmath.hpp"
#include "pgo_yaw_dev.hpp"
#include "pgo_host.hpp"

using namespace vslam;

namespace {

struct PgoyLane { PgoLane L; double g[3]; };      // free0 counts band positions (x 4), band0 blocks (x 16); g: the lane's unit axis

__global__ __launch_bounds__(256) void k_pgoy_linearize_b(const PgoyLane* __restrict__ tab, const PgoCtl* __restrict__ ctl, int init,
                                                          const PgoEdge* __restrict__ edges, const double* __restrict__ P0,
                                                          const double* __restrict__ P1, double* __restrict__ res,
                                                          double* __restrict__ Ji, double* __restrict__ Jj, double* __restrict__ cost) {
    const PgoyLane* Y = lane_entry(tab, blockIdx.y);
    const PgoLane* L = &Y->L;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= L->m) return;
    const PgoCtl* C = ctl + blockIdx.y;
    if (!init && !(C->active && (C->need_linearize & PGO_NEED_J))) return;
    const size_t e0 = (size_t)L->edge0;
    const double g[3] = {Y->g[0], Y->g[1], Y->g[2]};
    pgoy_linearize_edge(e, edges + e0, (C->cur ? P1 : P0) + (size_t)L->pose0 * 12, g, res + e0 * 6, Ji + e0 * PGOY_JAC, Jj + e0 * PGOY_JAC, cost + e0);
}

// the trial poses are the buffer that is not `cur`
__global__ __launch_bounds__(256) void k_pgoy_cost_b(const PgoyLane* __restrict__ tab, const PgoCtl* __restrict__ ctl,
                                                     const PgoEdge* __restrict__ edges, const double* __restrict__ P0,
                                                     const double* __restrict__ P1, double* __restrict__ cost) {
    const PgoLane* L = &lane_entry(tab, blockIdx.y)->L;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= L->m) return;
    const PgoCtl* C = ctl + blockIdx.y;
    if (!C->active) return;
    pgo_cost_edge(e, edges + L->edge0, (C->cur ? P0 : P1) + (size_t)L->pose0 * 12, cost + L->edge0);
}

// blockIdx.x: a wave of three block columns 3 x .. 3 x + 2 (the last wave of a lane may hold one or two)
__global__ __launch_bounds__(64) void k_pgoy_assemble_b(const PgoyLane* __restrict__ tab, const PgoCtl* __restrict__ ctl,
                                                        const int* __restrict__ pos, const int* __restrict__ rowStart,
                                                        const int* __restrict__ inc, const PgoEdge* __restrict__ edges,
                                                        const double* __restrict__ res, const double* __restrict__ Ji,
                                                        const double* __restrict__ Jj, double* __restrict__ band,
                                                        double* __restrict__ diagH, double* __restrict__ g) {
    const PgoLane* L = &lane_entry(tab, blockIdx.y)->L;
    const int lane = threadIdx.x;
    const int c = blockIdx.x * PGOY_COLS_PER_WAVE + lane / PGOY_COL_LANES, sub = lane % PGOY_COL_LANES;
    if (lane >= PGOY_COLS_PER_WAVE * PGOY_COL_LANES || c >= L->nf) return;
    const PgoCtl* C = ctl + blockIdx.y;
    if (!(C->active && (C->need_linearize & PGO_NEED_H))) return;
    const size_t e0 = (size_t)L->edge0, f0 = (size_t)L->free0 * PGOY_D;
    pgoy_assemble_column(c, sub, L->nf, L->b, pos + L->pose0, rowStart + L->row0, inc + L->inc0, edges + e0, res + e0 * 6,
                         Ji + e0 * PGOY_JAC, Jj + e0 * PGOY_JAC, band + (size_t)L->band0 * PGOY_BLK, diagH + f0, g + f0);
}

// every active lane's H band and gradient into the factor and the right-hand side, one element per thread
__global__ __launch_bounds__(256) void k_pgoy_band_copy_b(const PgoyLane* __restrict__ tab, const PgoCtl* __restrict__ ctl,
                                                          const double* __restrict__ bandH, const double* __restrict__ g,
                                                          double* __restrict__ bandL, double* __restrict__ rhs) {
    const PgoLane* L = &lane_entry(tab, blockIdx.y)->L;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t bandN = (size_t)(L->b + 1) * L->nf * PGOY_BLK;
    if (t >= bandN || !ctl[blockIdx.y].active) return;
    const size_t b0 = (size_t)L->band0 * PGOY_BLK;
    bandL[b0 + t] = bandH[b0 + t];
    if (t < (size_t)L->nf * PGOY_D) { const size_t f0 = (size_t)L->free0 * PGOY_D; rhs[f0 + t] = g[f0 + t]; }
}

// one workgroup per lane: the walk on the lane's band with the lane's n_free, b and lambda
__global__ __launch_bounds__(PGO_CHOL_NT) void k_pgoy_band_chol_b(const PgoyLane* __restrict__ tab, const PgoCtl* __restrict__ ctl,
                                                                  double* __restrict__ bandL, const double* __restrict__ diagH,
                                                                  double* __restrict__ rhs, double* __restrict__ delta,
                                                                  int* __restrict__ flag) {
    const PgoLane* L = &lane_entry(tab, blockIdx.x)->L;
    const PgoCtl* C = ctl + blockIdx.x;
    if (!C->active) return;
    const size_t f0 = (size_t)L->free0 * PGOY_D;
    pgoy_band_chol_walk(L->nf, L->b, C->lambda, bandL + (size_t)L->band0 * PGOY_BLK, diagH + f0, rhs + f0, delta + f0, flag + blockIdx.x);
}

__global__ __launch_bounds__(256) void k_pgoy_retract_b(const PgoyLane* __restrict__ tab, const PgoCtl* __restrict__ ctl,
                                                        const int* __restrict__ pos, double* __restrict__ P0, double* __restrict__ P1,
                                                        const double* __restrict__ delta) {
    const PgoyLane* Y = lane_entry(tab, blockIdx.y);
    const PgoLane* L = &Y->L;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= L->n) return;
    const PgoCtl* C = ctl + blockIdx.y;
    if (!C->active) return;
    const size_t p0 = (size_t)L->pose0 * 12;
    const double g[3] = {Y->g[0], Y->g[1], Y->g[2]};
    pgoy_retract_pose(k, pos + L->pose0, (C->cur ? P1 : P0) + p0, g, delta + (size_t)L->free0 * PGOY_D, (C->cur ? P0 : P1) + p0);
}

// out[2 lane], out[2 lane + 1]: the lane's cost sum and |delta|_inf (init: every lane's initial cost, no delta yet)
__global__ __launch_bounds__(PGO_RED_NT) void k_pgoy_reduce_b(const PgoyLane* __restrict__ tab, const PgoCtl* __restrict__ ctl, int init,
                                                              const double* __restrict__ cost, const double* __restrict__ delta,
                                                              double* __restrict__ out) {
    __shared__ double sS[PGO_RED_NT], sM[PGO_RED_NT];
    const PgoLane* L = &lane_entry(tab, blockIdx.x)->L;
    if (!init && !ctl[blockIdx.x].active) return;
    pgo_reduce_sum(threadIdx.x, L->m, cost + L->edge0, init ? 0 : L->nf * PGOY_D, delta + (size_t)L->free0 * PGOY_D, out + 2 * (size_t)blockIdx.x, sS, sM);
}

// pgo_lm_decide, one thread per lane; init as in k_pgo_decide_b: a lane with a cost <= 1e-20 or no free pose never becomes active
__global__ __launch_bounds__(PGO_MAX_LANES) void k_pgoy_decide_b(int lanes, int init, int maxIt, const PgoyLane* __restrict__ tab,
                                                                 PgoCtl* __restrict__ ctl, const double* __restrict__ out,
                                                                 const int* __restrict__ flag, int* __restrict__ nActive) {
    const int l = threadIdx.x;
    int act = 0;
    if (l < lanes) {
        PgoCtl c = ctl[l];
        if (init) {
            c.cost = c.initial_cost = out[2 * l];
            c.active = (c.cost > 1e-20) && tab[l].L.nf != 0;
            c.need_linearize = PGO_NEED_H;
        } else if (c.active) {
            pgo_lm_decide(c, out[2 * l], out[2 * l + 1], flag[l], maxIt);
        }
        ctl[l] = c;
        act = c.active;
    }
    const int cnt = __syncthreads_count(act);
    if (threadIdx.x == 0) *nActive = cnt;
}

// g = axis / |axis| in fp64; a zero or non-finite axis is refused
vslam_status pgoy_axis(const char* who, const double* axis, double* g) {
    if (!axis) { set_error("%s: invalid arguments", who); return VSLAM_ERR_INVALID; }
    const double x = axis[0], y = axis[1], z = axis[2];
    const double nrm = std::sqrt(x * x + y * y + z * z);
    if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(z) || !std::isfinite(nrm) || !(nrm > 0.0)) {
        set_error("%s: the axis is zero or not finite", who); return VSLAM_ERR_INVALID;
    }
    g[0] = x / nrm; g[1] = y / nrm; g[2] = z / nrm;
    return VSLAM_OK;
}

// the kernel set of the yaw-only solve for pgo_solve (pgo_host.hpp); a lane's axis is checked where its table entry is made
struct PgoYaw4 {
    static constexpr int D = PGOY_D, BLK = PGOY_BLK, JAC = PGOY_JAC;
    typedef vslam_pgo_yaw_graph Graph;
    typedef PgoyLane Lane;
    static constexpr const char* names[5] = {"pgoy_linearize", "pgoy_assemble", "pgoy_band_chol", "pgoy_retract", "pgoy_cost"};
    static const vslam_pgo_graph& graph(const Graph& g) { return g.graph; }
    static vslam_status lane(const char* who, const PgoLane& L, const Graph& g, Lane& out) { out.L = L; return pgoy_axis(who, g.axis, out.g); }
    static const PgoyLane* tab(const PgoDev& d) { return (const PgoyLane*)d.tab; }
    static void linearize(hipStream_t st, dim3 gEdge, int init, const PgoDev& d) {
        hipLaunchKernelGGL(k_pgoy_linearize_b, gEdge, dim3(256), 0, st, tab(d), d.ctl, init, d.E, d.P0, d.P1, d.res, d.Ji, d.Jj, d.cost);
    }
    static void assemble(hipStream_t st, int maxNf, int nl, const PgoDev& d) {
        hipLaunchKernelGGL(k_pgoy_assemble_b, dim3((maxNf + PGOY_COLS_PER_WAVE - 1) / PGOY_COLS_PER_WAVE, nl), dim3(64), 0, st, tab(d), d.ctl, d.pos, d.row,
                           d.inc, d.E, d.res, d.Ji, d.Jj, d.bandH, d.diag, d.g);
    }
    static void band(hipStream_t st, size_t maxBand, int nl, const PgoDev& d) {
        hipLaunchKernelGGL(k_pgoy_band_copy_b, dim3((unsigned)((maxBand + 255) / 256), nl), dim3(256), 0, st, tab(d), d.ctl, d.bandH, d.g, d.bandL, d.rhs);
        hipLaunchKernelGGL(k_pgoy_band_chol_b, dim3(nl), dim3(PGO_CHOL_NT), 0, st, tab(d), d.ctl, d.bandL, d.diag, d.rhs, d.delta, d.flag);
    }
    static void retract(hipStream_t st, dim3 gPose, const PgoDev& d) {
        hipLaunchKernelGGL(k_pgoy_retract_b, gPose, dim3(256), 0, st, tab(d), d.ctl, d.pos, d.P0, d.P1, d.delta);
    }
    static void cost(hipStream_t st, dim3 gEdge, const PgoDev& d) {
        hipLaunchKernelGGL(k_pgoy_cost_b, gEdge, dim3(256), 0, st, tab(d), d.ctl, d.E, d.P0, d.P1, d.cost);
    }
    static void decide(hipStream_t st, int nl, int init, int maxIt, const PgoDev& d) {
        hipLaunchKernelGGL(k_pgoy_reduce_b, dim3(nl), dim3(PGO_RED_NT), 0, st, tab(d), d.ctl, init, d.cost, d.delta, d.out);
        hipLaunchKernelGGL(k_pgoy_decide_b, dim3(1), dim3(PGO_MAX_LANES), 0, st, nl, init, maxIt, tab(d), d.ctl, d.out, d.flag, d.act);
    }
};
constexpr const char* PgoYaw4::names[5];

}  // namespace

// the one-lane case of the batched call (no idle lane: n < 1 is refused; its error texts name no lane)
extern "C" vslam_status vslam_pose_graph_optimize_yaw(const double* T_wc, const uint8_t* fixed, int32_t n, const vslam_pgo_edge* edges, int32_t m,
                                                      const double* axis, const vslam_pgo_params* params, int32_t device, double* T_wc_out,
                                                      vslam_pgo_report* report) {
    static const char* const who = "vslam_pose_graph_optimize_yaw";
    if (!report || n < 1 || !axis) { set_error("%s: invalid arguments", who); return VSLAM_ERR_INVALID; }
    int maxIt = 0;
    double lambda0 = 0.0;
    VS_CHECK(pgo_check_params(who, params, &maxIt, &lambda0));
    const vslam_pgo_yaw_graph graph{{T_wc, fixed, n, edges, m, T_wc_out}, {axis[0], axis[1], axis[2]}};
    return pgo_solve<PgoYaw4>(who, false, &graph, 1, maxIt, lambda0, device, report);
}

extern "C" vslam_status vslam_pose_graph_optimize_yaw_batch(const vslam_pgo_yaw_graph* graphs, int32_t lanes, const vslam_pgo_params* params,
                                                            int32_t device, vslam_pgo_report* reports) {
    static const char* const who = "vslam_pose_graph_optimize_yaw_batch";
    if (!graphs || !reports || lanes < 1) { set_error("%s: invalid arguments", who); return VSLAM_ERR_INVALID; }
    if (lanes > PGO_MAX_LANES) { set_error("%s: %d lanes exceed the limit (%d)", who, lanes, PGO_MAX_LANES); return VSLAM_ERR_CAPACITY; }
    int maxIt = 0;
    double lambda0 = 0.0;
    VS_CHECK(pgo_check_params(who, params, &maxIt, &lambda0));
    return pgo_solve<PgoYaw4>(who, true, graphs, lanes, maxIt, lambda0, device, reports);
}
