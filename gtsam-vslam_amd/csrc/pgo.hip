// Pose-graph optimisation on the device (no reference counterpart; DESIGN.md section 6 item 24, restated by tests/pgo_ref.py):
// Levenberg-Marquardt over SE(3) poses tied by relative-pose edges, the damped normal equations solved DIRECTLY by a
// block-banded Cholesky of 6x6 fp64 blocks after a reverse Cuthill-McKee reordering of the free poses on the host.
// There is ONE solve path (pgo_solve, pgo_host.hpp: a template over the kernel set, shared with the yaw-only solve of
// pgo_yaw.hip): several graphs (lanes) at once, one launch per stage for all of them, each kernel working on
// a lane's part of concatenated arrays.  vslam_pose_graph_optimize is its one-lane case, so a lane's bytes are the single call's
// by construction.
//   k_pgo_linearize_b   one thread per edge: residual, both 6x6 Jacobians, the edge's cost term
//   k_pgo_assemble_b    one wave per free pose, one lane per block element: a gather over the pose's incidence list (CSR, built
//                       once per call, ascending edge index) into the band's column and the gradient.  No atomics; every sum
//                       runs in list order.
//   k_pgo_band_copy_b / k_pgo_band_chol_b   H and g into the factor's arrays; one workgroup per lane walks the block columns:
//                       factor, forward substitution (carried as an extra row), back substitution.  Nothing on the host waits
//                       inside it.
//   k_pgo_retract_b / k_pgo_cost_b / k_pgo_reduce_b   the trial poses, their per-edge cost, the fixed-order sum and |delta|_inf
//   k_pgo_decide_b      the accept / reject rule, a thread per lane on a device control block
//   k_pgo_move_points_b one thread per map point: X' = T_new[ref] * T_old[ref]^-1 * X
// The host waits once per ROUND (one trial of every active lane), for how many lanes are still active.
// The __device__ bodies of these kernels and the accept / reject rule are in pgo_dev.hpp, the reordering in pgo_order_host.hpp:
// the global bundle adjustment (gba.hip) uses the same ones.  The lane table, validation, numbering and packing on the host are in
// pgo_host.hpp, which the yaw-only solve (pgo_yaw.hip) shares.
#include "common.hpp"
#include "dmath.hpp"
#include "pgo_dev.hpp"
#include "pgo_host.hpp"

using namespace vslam;

namespace {

__device__ __forceinline__ void pgo_move_point(int k, const double* __restrict__ pts, const int* __restrict__ ref,
                                               const double* __restrict__ Told, const double* __restrict__ Tnew,
                                               double* __restrict__ out) {
    const double x = pts[3 * (size_t)k], y = pts[3 * (size_t)k + 1], z = pts[3 * (size_t)k + 2];
    const int r = ref[k];
    if (r < 0) { out[3 * (size_t)k] = x; out[3 * (size_t)k + 1] = y; out[3 * (size_t)k + 2] = z; return; }
    const double* A = Told + (size_t)r * 16;
    const double* B = Tnew + (size_t)r * 16;
    const double dx = x - A[3], dy = y - A[7], dz = z - A[11];
    const double cx = A[0] * dx + A[4] * dy + A[8] * dz, cy = A[1] * dx + A[5] * dy + A[9] * dz, cz = A[2] * dx + A[6] * dy + A[10] * dz;
    out[3 * (size_t)k] = B[0] * cx + B[1] * cy + B[2] * cz + B[3];
    out[3 * (size_t)k + 1] = B[4] * cx + B[5] * cy + B[6] * cz + B[7];
    out[3 * (size_t)k + 2] = B[8] * cx + B[9] * cy + B[10] * cz + B[11];
}

// ---- the kernels: G graphs (lanes) in one launch per stage, blockIdx.y (or .x of the one-workgroup-per-lane kernels) = lane.
// The lanes' arrays are concatenated; a lane's entry of the table holds its sizes and where its parts begin.  Indices inside
// a lane's arrays (edge ends, incidence entries, band positions) are lane-local, so every body above sees one graph's arrays
// whatever the other lanes are.  The control block is a lane's Levenberg-Marquardt loop state.

// init: the linearisation every lane starts from (no lane is active yet)
__global__ __launch_bounds__(256) void k_pgo_linearize_b(const PgoLane* __restrict__ tab, const PgoCtl* __restrict__ ctl, int init,
                                                         const PgoEdge* __restrict__ edges, const double* __restrict__ P0,
                                                         const double* __restrict__ P1, double* __restrict__ res,
                                                         double* __restrict__ Ji, double* __restrict__ Jj, double* __restrict__ cost) {
    const PgoLane* L = lane_entry(tab, blockIdx.y);
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= L->m) return;
    const PgoCtl* C = ctl + blockIdx.y;
    if (!init && !(C->active && (C->need_linearize & PGO_NEED_J))) return;
    const size_t e0 = (size_t)L->edge0;
    pgo_linearize_edge(e, edges + e0, (C->cur ? P1 : P0) + (size_t)L->pose0 * 12, res + e0 * 6, Ji + e0 * 36, Jj + e0 * 36, cost + e0);
}

// the trial poses are the buffer that is not `cur`
__global__ __launch_bounds__(256) void k_pgo_cost_b(const PgoLane* __restrict__ tab, const PgoCtl* __restrict__ ctl,
                                                    const PgoEdge* __restrict__ edges, const double* __restrict__ P0,
                                                    const double* __restrict__ P1, double* __restrict__ cost) {
    const PgoLane* L = lane_entry(tab, blockIdx.y);
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= L->m) return;
    const PgoCtl* C = ctl + blockIdx.y;
    if (!C->active) return;
    pgo_cost_edge(e, edges + L->edge0, (C->cur ? P0 : P1) + (size_t)L->pose0 * 12, cost + L->edge0);
}

__global__ __launch_bounds__(64) void k_pgo_assemble_b(const PgoLane* __restrict__ tab, const PgoCtl* __restrict__ ctl,
                                                       const int* __restrict__ pos, const int* __restrict__ rowStart,
                                                       const int* __restrict__ inc, const PgoEdge* __restrict__ edges,
                                                       const double* __restrict__ res, const double* __restrict__ Ji,
                                                       const double* __restrict__ Jj, double* __restrict__ band,
                                                       double* __restrict__ diagH, double* __restrict__ g) {
    const PgoLane* L = lane_entry(tab, blockIdx.y);
    const int c = blockIdx.x, lane = threadIdx.x;
    if (c >= L->nf || lane >= 42) return;
    const PgoCtl* C = ctl + blockIdx.y;
    if (!(C->active && (C->need_linearize & PGO_NEED_H))) return;
    const size_t e0 = (size_t)L->edge0, f0 = (size_t)L->free0 * 6;
    pgo_assemble_column(c, lane, L->nf, L->b, pos + L->pose0, rowStart + L->row0, inc + L->inc0, edges + e0, res + e0 * 6,
                        Ji + e0 * 36, Jj + e0 * 36, band + (size_t)L->band0 * 36, diagH + f0, g + f0);
}

// every active lane's H band and gradient into the factor and the right-hand side, one element per thread (H and g survive a
// rejected trial; one workgroup copying its lane's band ahead of the walk was measured: 0.3 ms per round at 1 300 poses, a chain
// of ~900 dependent load / store pairs per thread)
__global__ __launch_bounds__(256) void k_pgo_band_copy_b(const PgoLane* __restrict__ tab, const PgoCtl* __restrict__ ctl,
                                                         const double* __restrict__ bandH, const double* __restrict__ g,
                                                         double* __restrict__ bandL, double* __restrict__ rhs) {
    const PgoLane* L = lane_entry(tab, blockIdx.y);
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t bandN = (size_t)(L->b + 1) * L->nf * 36;
    if (t >= bandN || !ctl[blockIdx.y].active) return;
    const size_t b0 = (size_t)L->band0 * 36;
    bandL[b0 + t] = bandH[b0 + t];
    if (t < (size_t)L->nf * 6) { const size_t f0 = (size_t)L->free0 * 6; rhs[f0 + t] = g[f0 + t]; }
}

// one workgroup per lane: the walk on the lane's band with the lane's n_free, b and lambda
__global__ __launch_bounds__(PGO_CHOL_NT) void k_pgo_band_chol_b(const PgoLane* __restrict__ tab, const PgoCtl* __restrict__ ctl,
                                                                 double* __restrict__ bandL, const double* __restrict__ diagH,
                                                                 double* __restrict__ rhs, double* __restrict__ delta,
                                                                 int* __restrict__ flag) {
    const PgoLane* L = lane_entry(tab, blockIdx.x);
    const PgoCtl* C = ctl + blockIdx.x;
    if (!C->active) return;
    const size_t f0 = (size_t)L->free0 * 6;
    pgo_band_chol_walk(L->nf, L->b, C->lambda, bandL + (size_t)L->band0 * 36, diagH + f0, rhs + f0, delta + f0, flag + blockIdx.x);
}

__global__ __launch_bounds__(256) void k_pgo_retract_b(const PgoLane* __restrict__ tab, const PgoCtl* __restrict__ ctl,
                                                       const int* __restrict__ pos, double* __restrict__ P0, double* __restrict__ P1,
                                                       const double* __restrict__ delta) {
    const PgoLane* L = lane_entry(tab, blockIdx.y);
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= L->n) return;
    const PgoCtl* C = ctl + blockIdx.y;
    if (!C->active) return;
    const size_t p0 = (size_t)L->pose0 * 12;
    pgo_retract_pose(k, pos + L->pose0, (C->cur ? P1 : P0) + p0, delta + (size_t)L->free0 * 6, (C->cur ? P0 : P1) + p0);
}

// out[2 lane], out[2 lane + 1]: the lane's cost sum and |delta|_inf (init: every lane's initial cost, no delta yet)
__global__ __launch_bounds__(PGO_RED_NT) void k_pgo_reduce_b(const PgoLane* __restrict__ tab, const PgoCtl* __restrict__ ctl, int init,
                                                             const double* __restrict__ cost, const double* __restrict__ delta,
                                                             double* __restrict__ out) {
    __shared__ double sS[PGO_RED_NT], sM[PGO_RED_NT];
    const PgoLane* L = lane_entry(tab, blockIdx.x);
    if (!init && !ctl[blockIdx.x].active) return;
    pgo_reduce_sum(threadIdx.x, L->m, cost + L->edge0, init ? 0 : L->nf * 6, delta + (size_t)L->free0 * 6, out + 2 * (size_t)blockIdx.x, sS, sM);
}

// The accept / reject rule of the Levenberg-Marquardt loop (pgo_lm_decide, pgo_dev.hpp), one thread per lane, fp64.
// init: the lanes' initial costs have been summed; a lane with a cost <= 1e-20 or no free pose never becomes active.
// *nActive: what the host reads once per round.
__global__ __launch_bounds__(PGO_MAX_LANES) void k_pgo_decide_b(int lanes, int init, int maxIt, const PgoLane* __restrict__ tab,
                                                                PgoCtl* __restrict__ ctl, const double* __restrict__ out,
                                                                const int* __restrict__ flag, int* __restrict__ nActive) {
    const int l = threadIdx.x;
    int act = 0;
    if (l < lanes) {
        PgoCtl c = ctl[l];
        if (init) {
            c.cost = c.initial_cost = out[2 * l];
            c.active = (c.cost > 1e-20) && tab[l].nf != 0;
            c.need_linearize = PGO_NEED_H;                  // (the initial linearisation serves the first assembly)
        } else if (c.active) {
            pgo_lm_decide(c, out[2 * l], out[2 * l + 1], flag[l], maxIt);
        }
        ctl[l] = c;
        act = c.active;
    }
    const int cnt = __syncthreads_count(act);
    if (threadIdx.x == 0) *nActive = cnt;
}

// the map points of several graphs in one launch: a lane's points, references and poses are its part of the concatenated arrays
struct PgoMoveLane { int n, pt0, pose0; };
__global__ __launch_bounds__(256) void k_pgo_move_points_b(const PgoMoveLane* __restrict__ tab, const double* __restrict__ pts,
                                                            const int* __restrict__ ref, const double* __restrict__ Told,
                                                            const double* __restrict__ Tnew, double* __restrict__ out) {
    const PgoMoveLane* L = lane_entry(tab, blockIdx.y);
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= L->n) return;
    const size_t p0 = (size_t)L->pt0, t0 = (size_t)L->pose0 * 16;
    pgo_move_point(k, pts + 3 * p0, ref + p0, Told + t0, Tnew + t0, out + 3 * p0);
}

}  // namespace

std::vector<std::pair<const char*, float>>& vslam::pgo_times() {
    thread_local std::vector<std::pair<const char*, float>> times;
    return times;
}
bool& vslam::pgo_timing_on() {
    thread_local bool on = false;
    return on;
}

long long& vslam::pgo_solve_count() {
    thread_local long long n = 0;
    return n;
}

extern "C" vslam_status vslam_pose_graph_solve_count(int64_t* n_out) {
    if (!n_out) return VSLAM_ERR_INVALID;
    *n_out = pgo_solve_count();
    return VSLAM_OK;
}

extern "C" vslam_status vslam_pose_graph_set_timing(int32_t on) {
    pgo_timing_on() = on != 0;
    pgo_times().clear();
    pgo_solve_count() = 0;
    return VSLAM_OK;
}

extern "C" vslam_status vslam_pose_graph_timings(const char** names, float* ms, int32_t cap, int32_t* n_out) {
    if (!n_out || cap < 0 || (cap > 0 && (!names || !ms))) return VSLAM_ERR_INVALID;
    int n = 0;
    for (const auto& t : pgo_times()) { if (n >= cap) break; names[n] = t.first; ms[n] = t.second; n++; }
    *n_out = n;
    return VSLAM_OK;
}

namespace {

// the kernel set of the 6-DoF solve for pgo_solve (pgo_host.hpp)
struct Pgo6 {
    static constexpr int D = 6, BLK = 36, JAC = 36;
    typedef vslam_pgo_graph Graph;
    typedef PgoLane Lane;
    static constexpr const char* names[5] = {"pgo_linearize", "pgo_assemble", "pgo_band_chol", "pgo_retract", "pgo_cost"};
    static const vslam_pgo_graph& graph(const Graph& g) { return g; }
    static vslam_status lane(const char*, const PgoLane& L, const Graph&, Lane& out) { out = L; return VSLAM_OK; }
    static const PgoLane* tab(const PgoDev& d) { return (const PgoLane*)d.tab; }
    static void linearize(hipStream_t st, dim3 gEdge, int init, const PgoDev& d) {
        hipLaunchKernelGGL(k_pgo_linearize_b, gEdge, dim3(256), 0, st, tab(d), d.ctl, init, d.E, d.P0, d.P1, d.res, d.Ji, d.Jj, d.cost);
    }
    static void assemble(hipStream_t st, int maxNf, int nl, const PgoDev& d) {
        hipLaunchKernelGGL(k_pgo_assemble_b, dim3(maxNf, nl), dim3(64), 0, st, tab(d), d.ctl, d.pos, d.row, d.inc, d.E, d.res, d.Ji, d.Jj, d.bandH, d.diag, d.g);
    }
    static void band(hipStream_t st, size_t maxBand, int nl, const PgoDev& d) {
        hipLaunchKernelGGL(k_pgo_band_copy_b, dim3((unsigned)((maxBand + 255) / 256), nl), dim3(256), 0, st, tab(d), d.ctl, d.bandH, d.g, d.bandL, d.rhs);
        hipLaunchKernelGGL(k_pgo_band_chol_b, dim3(nl), dim3(PGO_CHOL_NT), 0, st, tab(d), d.ctl, d.bandL, d.diag, d.rhs, d.delta, d.flag);
    }
    static void retract(hipStream_t st, dim3 gPose, const PgoDev& d) {
        hipLaunchKernelGGL(k_pgo_retract_b, gPose, dim3(256), 0, st, tab(d), d.ctl, d.pos, d.P0, d.P1, d.delta);
    }
    static void cost(hipStream_t st, dim3 gEdge, const PgoDev& d) {
        hipLaunchKernelGGL(k_pgo_cost_b, gEdge, dim3(256), 0, st, tab(d), d.ctl, d.E, d.P0, d.P1, d.cost);
    }
    static void decide(hipStream_t st, int nl, int init, int maxIt, const PgoDev& d) {
        hipLaunchKernelGGL(k_pgo_reduce_b, dim3(nl), dim3(PGO_RED_NT), 0, st, tab(d), d.ctl, init, d.cost, d.delta, d.out);
        hipLaunchKernelGGL(k_pgo_decide_b, dim3(1), dim3(PGO_MAX_LANES), 0, st, nl, init, maxIt, tab(d), d.ctl, d.out, d.flag, d.act);
    }
};
constexpr const char* Pgo6::names[5];

}  // namespace

// the one-lane case of pgo_solve (no idle lane: n < 1 is refused; its error texts name no lane)
extern "C" vslam_status vslam_pose_graph_optimize(const double* T_wc, const uint8_t* fixed, int32_t n, const vslam_pgo_edge* edges, int32_t m,
                                                  const vslam_pgo_params* params, int32_t device, double* T_wc_out, vslam_pgo_report* report) {
    static const char* const who = "vslam_pose_graph_optimize";
    if (!report || n < 1) { set_error("%s: invalid arguments", who); return VSLAM_ERR_INVALID; }
    int maxIt = 0;
    double lambda0 = 0.0;
    VS_CHECK(pgo_check_params(who, params, &maxIt, &lambda0));
    const vslam_pgo_graph graph{T_wc, fixed, n, edges, m, T_wc_out};
    return pgo_solve<Pgo6>(who, false, &graph, 1, maxIt, lambda0, device, report);
}

extern "C" vslam_status vslam_pose_graph_optimize_batch(const vslam_pgo_graph* graphs, int32_t lanes, const vslam_pgo_params* params,
                                                        int32_t device, vslam_pgo_report* reports) {
    static const char* const who = "vslam_pose_graph_optimize_batch";
    if (!graphs || !reports || lanes < 1) { set_error("%s: invalid arguments", who); return VSLAM_ERR_INVALID; }
    if (lanes > PGO_MAX_LANES) { set_error("%s: %d lanes exceed the limit (%d)", who, lanes, PGO_MAX_LANES); return VSLAM_ERR_CAPACITY; }
    int maxIt = 0;
    double lambda0 = 0.0;
    VS_CHECK(pgo_check_params(who, params, &maxIt, &lambda0));
    return pgo_solve<Pgo6>(who, true, graphs, lanes, maxIt, lambda0, device, reports);
}

vslam_status vslam::pgo_move_points_batch(const PgoMoveGraph* graphs, int lanes, int device) {
    if (!graphs || lanes < 1) { set_error("pgo_move_points_batch: invalid arguments"); return VSLAM_ERR_INVALID; }
    std::vector<PgoMoveLane> tab;
    std::vector<int> live;
    size_t nPts = 0, nPoses = 0;
    int maxPts = 0;
    for (int g = 0; g < lanes; g++) {
        const PgoMoveGraph& Q = graphs[g];
        if (Q.n_points < 0 || Q.n_poses < 0 || (Q.n_points > 0 && (!Q.xyz || !Q.ref || !Q.out)) || (Q.n_poses > 0 && (!Q.T_old || !Q.T_new))) {
            set_error("pgo_move_points_batch: lane %d: invalid arguments", g); return VSLAM_ERR_INVALID;
        }
        for (int k = 0; k < Q.n_points; k++)
            if (Q.ref[k] >= Q.n_poses) { set_error("pgo_move_points_batch: lane %d: point %d refers to pose %d of %d", g, k, Q.ref[k], Q.n_poses); return VSLAM_ERR_INVALID; }
        if (Q.n_points == 0) continue;
        if (nPts + (size_t)Q.n_points > (size_t)INT32_MAX / 4 || nPoses + (size_t)Q.n_poses > (size_t)INT32_MAX / 16) {
            set_error("pgo_move_points_batch: too many points or poses in all"); return VSLAM_ERR_CAPACITY;
        }
        tab.push_back(PgoMoveLane{Q.n_points, (int)nPts, (int)nPoses});
        live.push_back(g);
        nPts += Q.n_points; nPoses += Q.n_poses; maxPts = std::max(maxPts, Q.n_points);
    }
    const int nl = (int)live.size();
    if (!nl) return VSLAM_OK;
    DevPool* pool = nullptr;
    VS_CHECK(pgo_device_pool(device, &pool));
    PgoLayout up;
    const size_t oTab = up.section(nl * sizeof(PgoMoveLane)), oPts = up.section(nPts * 24), oRef = up.section(nPts * 4);
    const size_t oOld = up.section(nPoses * 128), oNew = up.section(nPoses * 128);
    std::vector<uint8_t> hUp(up.bytes, 0);
    memcpy(hUp.data() + oTab, tab.data(), nl * sizeof(PgoMoveLane));
    for (int l = 0; l < nl; l++) {
        const PgoMoveGraph& Q = graphs[live[l]];
        memcpy(hUp.data() + oPts + (size_t)tab[l].pt0 * 24, Q.xyz, (size_t)Q.n_points * 24);
        memcpy(hUp.data() + oRef + (size_t)tab[l].pt0 * 4, Q.ref, (size_t)Q.n_points * 4);
        if (Q.n_poses) {
            memcpy(hUp.data() + oOld + (size_t)tab[l].pose0 * 128, Q.T_old, (size_t)Q.n_poses * 128);
            memcpy(hUp.data() + oNew + (size_t)tab[l].pose0 * 128, Q.T_new, (size_t)Q.n_poses * 128);
        }
    }
    PoolBuf<uint8_t> dUp(pool); PoolBuf<double> dOut(pool);
    VS_HIP(dUp.up(hUp.data(), up.bytes)); VS_HIP(dOut.alloc(nPts * 3));
    hipLaunchKernelGGL(k_pgo_move_points_b, dim3((maxPts + 255) / 256, nl), dim3(256), 0, pool->stream, (const PgoMoveLane*)(dUp.p + oTab),
                       (const double*)(dUp.p + oPts), (const int*)(dUp.p + oRef), (const double*)(dUp.p + oOld), (const double*)(dUp.p + oNew), dOut.p);
    VS_HIP(hipGetLastError());
    for (int l = 0; l < nl; l++) VS_HIP(pool->d2h(graphs[live[l]].out, dOut.p + 3 * (size_t)tab[l].pt0, (size_t)tab[l].n * 24));
    VS_HIP(pool->sync());
    return VSLAM_OK;
}

// its own checks (its own wording), then the one-lane case of pgo_move_points_batch
extern "C" vslam_status vslam_pose_graph_move_points(const double* points_xyz, const int32_t* ref_index, const double* T_old, const double* T_new,
                                                     int32_t n_points, int32_t n_poses, int32_t device, double* points_out) {
    if (n_points < 0 || n_poses < 0 || (n_points > 0 && (!points_xyz || !ref_index || !points_out)) || (n_poses > 0 && (!T_old || !T_new))) {
        set_error("vslam_pose_graph_move_points: invalid arguments"); return VSLAM_ERR_INVALID;
    }
    for (int k = 0; k < n_points; k++) if (ref_index[k] >= n_poses) { set_error("vslam_pose_graph_move_points: point %d refers to pose %d of %d", k, ref_index[k], n_poses); return VSLAM_ERR_INVALID; }
    const PgoMoveGraph graph{points_xyz, ref_index, n_points, T_old, T_new, n_poses, points_out};
    return pgo_move_points_batch(&graph, 1, device);
}
