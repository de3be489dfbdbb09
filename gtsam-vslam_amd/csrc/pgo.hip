// Pose-graph optimisation on the device (no reference counterpart; DESIGN.md section 6 item 24, restated by tests/pgo_ref.py):
// Levenberg-Marquardt over SE(3) poses tied by relative-pose edges, the damped normal equations solved DIRECTLY by a
// block-banded Cholesky of 6x6 fp64 blocks after a reverse Cuthill-McKee reordering of the free poses on the host.
// There is ONE solve path (pgo_solve): several graphs (lanes) at once, one launch per stage for all of them, each kernel working on
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
// the global bundle adjustment (gba.hip) uses the same ones.
#include "common.hpp"
#include "dmath.hpp"
#include "pgo_dev.hpp"
#include "pgo_order_host.hpp"
#include <cmath>
#include <numeric>

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
constexpr int PGO_MAX_LANES = 1024;                 // (k_pgo_decide_b is ONE workgroup with a thread per lane)
constexpr int PGO_SUM_POSES = 262144, PGO_SUM_EDGES = 1048576, PGO_SUM_BLOCKS = 1048576;

struct PgoLane {
    int n, m, nf, b;
    int pose0, edge0;      // first pose (poses, pos), first edge (edges, res, Ji, Jj, cost)
    int free0, row0;       // first band position (diagH, g, rhs, delta: x 6), first entry of the lane's nf + 1 row starts
    int inc0, band0;       // first incidence entry, first band block (x 36)
};

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

inline bool finite16(const double* p, int n) { for (int k = 0; k < n; k++) if (!std::isfinite(p[k])) return false; return true; }

thread_local std::vector<std::pair<const char*, float>> g_pgoTimes;
thread_local bool g_pgoTimingOn = false;

// what every entry point does before its first device call: `device` names a device, the calling thread's pool with nothing pending
vslam_status pgo_device_pool(int device, DevPool** out) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available (no CPU fallback)"); return VSLAM_ERR_NO_DEVICE; }
    if (device < 0 || device >= ndev) return VSLAM_ERR_INVALID;
    VS_HIP(hipSetDevice(device));
    DevPool* pool = thread_pool(device);
    if (!pool) { set_error("no device pool"); return VSLAM_ERR_HIP; }
    pool->pending.clear();
    *out = pool;
    return VSLAM_OK;
}

// the sections of one device block, at 256-byte steps: section() returns where the next one begins
struct PgoLayout {
    size_t bytes = 0;
    size_t section(size_t n) { const size_t at = bytes; bytes = align_up_sz(bytes + std::max<size_t>(n, 8), 256); return at; }
};

}  // namespace

extern "C" vslam_status vslam_pose_graph_set_timing(int32_t on) {
    g_pgoTimingOn = on != 0;
    g_pgoTimes.clear();
    return VSLAM_OK;
}

extern "C" vslam_status vslam_pose_graph_timings(const char** names, float* ms, int32_t cap, int32_t* n_out) {
    if (!n_out || cap < 0 || (cap > 0 && (!names || !ms))) return VSLAM_ERR_INVALID;
    int n = 0;
    for (const auto& t : g_pgoTimes) { if (n >= cap) break; names[n] = t.first; ms[n] = t.second; n++; }
    *n_out = n;
    return VSLAM_OK;
}

namespace {

// What the host derives from one graph before anything is launched: the free poses' band positions, the band width, the incidence
// lists and the device forms of edges and poses.  Every lane goes through pgo_check_sizes and pgo_prepare; `who` (the entry
// point, with the lane for a batched call) starts every error text.
struct PgoPrep {
    int n = 0, m = 0, nf = 0, nIso = 0, b = 0;
    std::vector<int> pos, rowStart, inc;      // pos [n]: band position or -1; rowStart [nf + 1]; inc: edge << 1 | side, ascending
    std::vector<PgoEdge> he;
    std::vector<double> hp;                   // [n][12]
};

vslam_status pgo_check_sizes(const char* who, const double* T_wc, const uint8_t* fixed, int n, const vslam_pgo_edge* edges, int m, const double* T_wc_out) {
    if (!T_wc || !fixed || !T_wc_out || n < 1 || m < 0 || (m > 0 && !edges)) { set_error("%s: invalid arguments", who); return VSLAM_ERR_INVALID; }
    if (n > PGO_MAX_POSES || m > PGO_MAX_EDGES) { set_error("%s: %d poses / %d edges exceed the limits (%d / %d)", who, n, m, PGO_MAX_POSES, PGO_MAX_EDGES); return VSLAM_ERR_CAPACITY; }
    return VSLAM_OK;
}

vslam_status pgo_check_params(const char* who, const vslam_pgo_params* params, int* maxIt, double* lambda) {
    *maxIt = params ? params->max_iterations : 0;
    *lambda = params ? params->lambda0 : 0.0;
    if (*maxIt < 0 || !(*lambda >= 0.0) || !std::isfinite(*lambda)) { set_error("%s: negative or non-finite parameter", who); return VSLAM_ERR_INVALID; }
    if (*maxIt == 0) *maxIt = 20;
    if (*lambda == 0.0) *lambda = 1e-4;
    return VSLAM_OK;
}

vslam_status pgo_prepare(const char* who, const double* T_wc, const uint8_t* fixed, int n, const vslam_pgo_edge* edges, int m, PgoPrep& G) {
    G.n = n; G.m = m;
    if (!finite16(T_wc, 16 * n)) { set_error("%s: non-finite pose", who); return VSLAM_ERR_INVALID; }
    std::vector<int> deg(n, 0);
    for (int e = 0; e < m; e++) {
        const vslam_pgo_edge& E = edges[e];
        if (E.i < 0 || E.j < 0 || E.i >= n || E.j >= n || E.i == E.j) { set_error("%s: edge %d joins poses %d and %d (n = %d)", who, e, E.i, E.j, n); return VSLAM_ERR_INVALID; }
        if (!finite16(E.Z, 16) || !std::isfinite(E.w_rot) || !std::isfinite(E.w_trans)) { set_error("%s: edge %d has a non-finite value", who, e); return VSLAM_ERR_INVALID; }
        if (E.w_rot < 0 || E.w_trans < 0) { set_error("%s: edge %d has a negative weight", who, e); return VSLAM_ERR_INVALID; }
        deg[E.i]++; deg[E.j]++;
    }
    // free poses (not fixed, at least one edge), numbered in ascending pose index
    std::vector<int> fidx(n, -1), fpose;
    int nIso = 0;
    for (int k = 0; k < n; k++) {
        if (fixed[k]) continue;
        if (!deg[k]) { nIso++; continue; }
        fidx[k] = (int)fpose.size(); fpose.push_back(k);
    }
    const int nf = (int)fpose.size();
    std::vector<std::vector<int>> adj(nf);
    std::vector<uint8_t> anchored(nf, 0);
    for (int e = 0; e < m; e++) {
        const int a = fidx[edges[e].i], b2 = fidx[edges[e].j];
        if (a >= 0 && b2 >= 0) { adj[a].push_back(b2); adj[b2].push_back(a); }
        else if (a >= 0) anchored[a] = 1;
        else if (b2 >= 0) anchored[b2] = 1;
    }
    for (auto& v : adj) { std::sort(v.begin(), v.end()); v.erase(std::unique(v.begin(), v.end()), v.end()); }
    {   // every component of free poses needs an edge to a fixed pose
        std::vector<uint8_t> seen(nf, 0);
        std::vector<int> comp;
        for (int s0 = 0; s0 < nf; s0++) {
            if (seen[s0]) continue;
            comp.clear(); comp.push_back(s0); seen[s0] = 1;
            bool anc = false;
            for (size_t h = 0; h < comp.size(); h++) {
                anc = anc || anchored[comp[h]];
                for (int v : adj[comp[h]]) if (!seen[v]) { seen[v] = 1; comp.push_back(v); }
            }
            if (!anc) { set_error("%s: the free poses connected to pose %d have no edge to a fixed pose (free gauge)", who, fpose[s0]); return VSLAM_ERR_INVALID; }
        }
    }
    std::vector<int> order;
    pgo_rcm(nf, adj, order);
    std::vector<int>& pos = G.pos;
    std::vector<int> perm(std::max(nf, 1), 0);
    pos.assign(n, -1);
    for (int c = 0; c < nf; c++) { perm[c] = fpose[order[c]]; pos[perm[c]] = c; }
    int b = 0;
    for (int e = 0; e < m; e++) { const int a = pos[edges[e].i], c = pos[edges[e].j]; if (a >= 0 && c >= 0) b = std::max(b, std::abs(a - c)); }
    if ((long long)(b + 1) * nf > PGO_MAX_BLOCKS) { set_error("%s: the band needs %lld blocks (limit %d)", who, (long long)(b + 1) * nf, PGO_MAX_BLOCKS); return VSLAM_ERR_CAPACITY; }
    G.nf = nf; G.nIso = nIso; G.b = b;
    // incidence lists by band position, ascending edge index
    std::vector<int>& rowStart = G.rowStart;
    std::vector<int>& inc = G.inc;
    rowStart.assign(nf + 1, 0);
    for (int e = 0; e < m; e++) { if (pos[edges[e].i] >= 0) rowStart[pos[edges[e].i] + 1]++; if (pos[edges[e].j] >= 0) rowStart[pos[edges[e].j] + 1]++; }
    for (int c = 0; c < nf; c++) rowStart[c + 1] += rowStart[c];
    inc.assign(std::max(rowStart[nf], 1), 0);
    {
        std::vector<int> fill(rowStart.begin(), rowStart.end() - 1);
        for (int e = 0; e < m; e++) {
            if (pos[edges[e].i] >= 0) inc[fill[pos[edges[e].i]]++] = e << 1;
            if (pos[edges[e].j] >= 0) inc[fill[pos[edges[e].j]]++] = e << 1 | 1;
        }
    }
    G.he.assign(std::max(m, 1), PgoEdge{});
    for (int e = 0; e < m; e++) {
        PgoEdge& o = G.he[e];
        o.i = edges[e].i; o.j = edges[e].j; o.wr = edges[e].w_rot; o.wt = edges[e].w_trans;
        for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) o.Rz[3 * r + c] = edges[e].Z[4 * r + c]; o.tz[r] = edges[e].Z[4 * r + 3]; }
    }
    G.hp.resize((size_t)n * 12);
    for (int k = 0; k < n; k++)
        for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) G.hp[(size_t)k * 12 + 3 * r + c] = T_wc[(size_t)k * 16 + 4 * r + c]; G.hp[(size_t)k * 12 + 9 + r] = T_wc[(size_t)k * 16 + 4 * r + 3]; }
    return VSLAM_OK;
}

// the optimised poses back into the caller's [n][16] form: fixed and isolated poses are the input's bytes
void pgo_write_out(const PgoPrep& G, const double* hp, const double* T_wc, double* T_wc_out) {
    for (int k = 0; k < G.n; k++) {
        double* o = T_wc_out + (size_t)k * 16;
        if (G.pos[k] < 0) { if (o != T_wc + (size_t)k * 16) memcpy(o, T_wc + (size_t)k * 16, 16 * sizeof(double)); continue; }
        for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) o[4 * r + c] = hp[(size_t)k * 12 + 3 * r + c]; o[4 * r + 3] = hp[(size_t)k * 12 + 9 + r]; }
        o[12] = o[13] = o[14] = 0.0; o[15] = 1.0;
    }
}

// THE solve, behind both entry points: `lanes` graphs, the checked parameters.  A lane with n == 0 is idle (the single call never
// passes one).  Host work per lane is pgo_prepare; the lanes' arrays then go up as ONE block (table, control blocks, edges,
// poses, positions, incidence lists) and the device's own arrays are one more block from the thread's cache.  A round is one
// trial of every active lane: eight launches and one wait, for a single int (how many lanes are still active).
// `who` starts every error text, with the lane where `nameLane` says so.  Nothing is written before the last wait has returned.
vslam_status pgo_solve(const char* who, bool nameLane, const vslam_pgo_graph* graphs, int lanes, int maxIt, double lambda0, int device,
                       vslam_pgo_report* reports) {
    char lw[96];
    auto lane_text = [&](int g) { if (nameLane) snprintf(lw, sizeof lw, "%s: lane %d", who, g); else snprintf(lw, sizeof lw, "%s", who); return lw; };
    std::vector<int> live;                  // the lanes that hold a graph, in call order: the device's lanes
    long long sumN = 0, sumM = 0;
    for (int g = 0; g < lanes; g++) {
        const vslam_pgo_graph& Q = graphs[g];
        if (Q.n == 0) continue;
        VS_CHECK(pgo_check_sizes(lane_text(g), Q.T_wc, Q.fixed, Q.n, Q.edges, Q.m, Q.T_wc_out));
        sumN += Q.n; sumM += Q.m;
        live.push_back(g);
    }
    if (sumN > PGO_SUM_POSES || sumM > PGO_SUM_EDGES) {
        set_error("%s: %lld poses / %lld edges in all exceed the limits (%d / %d)", who, sumN, sumM, PGO_SUM_POSES, PGO_SUM_EDGES);
        return VSLAM_ERR_CAPACITY;
    }
    const int nl = (int)live.size();
    std::vector<PgoPrep> prep(nl);
    std::vector<PgoLane> tab(std::max(nl, 1));
    long long sumB = 0;
    int N = 0, M = 0, NF = 0, INC = 0, maxN = 0, maxM = 0, maxNf = 0;
    size_t maxBand = 0;                     // doubles of the largest lane's band
    for (int l = 0; l < nl; l++) {
        const vslam_pgo_graph& Q = graphs[live[l]];
        VS_CHECK(pgo_prepare(lane_text(live[l]), Q.T_wc, Q.fixed, Q.n, Q.edges, Q.m, prep[l]));
        const PgoPrep& G = prep[l];
        if (sumB + (long long)(G.b + 1) * G.nf > PGO_SUM_BLOCKS) {
            set_error("%s: the lanes' bands need more than %d blocks in all (reached at lane %d)", who, PGO_SUM_BLOCKS, live[l]);
            return VSLAM_ERR_CAPACITY;
        }
        tab[l] = PgoLane{G.n, G.m, G.nf, G.b, N, M, NF, NF + l, INC, (int)sumB};
        N += G.n; M += G.m; NF += G.nf; INC += G.rowStart[G.nf]; sumB += (long long)(G.b + 1) * G.nf;
        maxN = std::max(maxN, G.n); maxM = std::max(maxM, G.m); maxNf = std::max(maxNf, G.nf);
        maxBand = std::max(maxBand, (size_t)(G.b + 1) * G.nf * 36);
    }
    if (nl == 0) return VSLAM_OK;           // (every lane idle: nothing to solve, nothing written)
    DevPool* pool = nullptr;
    VS_CHECK(pgo_device_pool(device, &pool));
    hipStream_t st = pool->stream;

    PgoLayout up, wk;                       // the upload block and the work block
    const size_t oTab = up.section(nl * sizeof(PgoLane)), oCtl = up.section(nl * sizeof(PgoCtl));
    const size_t oE = up.section((size_t)M * sizeof(PgoEdge)), oP0 = up.section((size_t)N * 12 * sizeof(double));
    const size_t oPos = up.section((size_t)N * sizeof(int)), oRow = up.section((size_t)(NF + nl) * sizeof(int));
    const size_t oInc = up.section((size_t)INC * sizeof(int));
    const size_t bandBytes = (size_t)sumB * 36 * sizeof(double), vecBytes = (size_t)NF * 6 * sizeof(double);
    const size_t oP1 = wk.section((size_t)N * 12 * sizeof(double)), oRes = wk.section((size_t)M * 6 * sizeof(double));
    const size_t oJi = wk.section((size_t)M * 36 * sizeof(double)), oJj = wk.section((size_t)M * 36 * sizeof(double));
    const size_t oCost = wk.section((size_t)M * sizeof(double));
    const size_t oBandH = wk.section(bandBytes), oBandL = wk.section(bandBytes);
    const size_t oDiag = wk.section(vecBytes), oG = wk.section(vecBytes), oRhs = wk.section(vecBytes), oDelta = wk.section(vecBytes);
    const size_t oOut = wk.section((size_t)nl * 2 * sizeof(double)), oFlag = wk.section((size_t)nl * sizeof(int));
    const size_t oAct = wk.section(sizeof(int));
    std::vector<uint8_t> hUp(up.bytes, 0);
    memcpy(hUp.data() + oTab, tab.data(), nl * sizeof(PgoLane));
    for (int l = 0; l < nl; l++) {
        const PgoPrep& G = prep[l];
        PgoCtl c{};
        c.lambda = lambda0;
        memcpy(hUp.data() + oCtl + l * sizeof(PgoCtl), &c, sizeof c);
        memcpy(hUp.data() + oE + (size_t)tab[l].edge0 * sizeof(PgoEdge), G.he.data(), (size_t)G.m * sizeof(PgoEdge));
        memcpy(hUp.data() + oP0 + (size_t)tab[l].pose0 * 12 * sizeof(double), G.hp.data(), (size_t)G.n * 12 * sizeof(double));
        memcpy(hUp.data() + oPos + (size_t)tab[l].pose0 * sizeof(int), G.pos.data(), (size_t)G.n * sizeof(int));
        memcpy(hUp.data() + oRow + (size_t)tab[l].row0 * sizeof(int), G.rowStart.data(), (size_t)(G.nf + 1) * sizeof(int));
        memcpy(hUp.data() + oInc + (size_t)tab[l].inc0 * sizeof(int), G.inc.data(), (size_t)G.rowStart[G.nf] * sizeof(int));
    }
    PoolBuf<uint8_t> dUp(pool), dWk(pool);
    VS_HIP(dUp.up(hUp.data(), up.bytes)); VS_HIP(dWk.alloc(wk.bytes));
    const PgoLane* dTab = (const PgoLane*)(dUp.p + oTab);
    PgoCtl* dCtl = (PgoCtl*)(dUp.p + oCtl);
    const PgoEdge* dE = (const PgoEdge*)(dUp.p + oE);
    double* dP0 = (double*)(dUp.p + oP0);
    const int* dPos = (const int*)(dUp.p + oPos);
    const int* dRow = (const int*)(dUp.p + oRow);
    const int* dInc = (const int*)(dUp.p + oInc);
    double* dP1 = (double*)(dWk.p + oP1); double* dRes = (double*)(dWk.p + oRes); double* dJi = (double*)(dWk.p + oJi);
    double* dJj = (double*)(dWk.p + oJj); double* dCost = (double*)(dWk.p + oCost); double* dBandH = (double*)(dWk.p + oBandH);
    double* dBandL = (double*)(dWk.p + oBandL); double* dDiag = (double*)(dWk.p + oDiag); double* dG = (double*)(dWk.p + oG);
    double* dRhs = (double*)(dWk.p + oRhs); double* dDelta = (double*)(dWk.p + oDelta); double* dOut = (double*)(dWk.p + oOut);
    int* dFlag = (int*)(dWk.p + oFlag); int* dAct = (int*)(dWk.p + oAct);

    struct TimerOwner { StageTimer t; ~TimerOwner() { t.destroy(); } } timerOwner;      // (the events go on every return path)
    StageTimer& timer = timerOwner.t;
    timer.stream = st; timer.multi = true; timer.enabled = g_pgoTimingOn;
    const dim3 gEdge((maxM + 255) / 256, nl), gPose((maxN + 255) / 256, nl);
    int nActive = 0;
    auto decide = [&](int init, int t) -> vslam_status {        // closes the pgo_cost group `t`, then the round's one wait
        hipLaunchKernelGGL(k_pgo_reduce_b, dim3(nl), dim3(PGO_RED_NT), 0, st, dTab, dCtl, init, dCost, dDelta, dOut);
        hipLaunchKernelGGL(k_pgo_decide_b, dim3(1), dim3(PGO_MAX_LANES), 0, st, nl, init, maxIt, dTab, dCtl, dOut, dFlag, dAct);
        timer.end(t);
        VS_HIP(hipGetLastError());
        VS_HIP(pool->d2h(&nActive, dAct, sizeof(int)));
        VS_HIP(pool->sync());
        return VSLAM_OK;
    };
    int t = timer.begin("pgo_linearize");
    if (maxM) hipLaunchKernelGGL(k_pgo_linearize_b, gEdge, dim3(256), 0, st, dTab, dCtl, 1, dE, dP0, dP1, dRes, dJi, dJj, dCost);
    timer.end(t);
    VS_CHECK(decide(1, timer.begin("pgo_cost")));
    while (nActive > 0) {       // one round
        t = timer.begin("pgo_linearize");
        hipLaunchKernelGGL(k_pgo_linearize_b, gEdge, dim3(256), 0, st, dTab, dCtl, 0, dE, dP0, dP1, dRes, dJi, dJj, dCost);
        timer.end(t);
        t = timer.begin("pgo_assemble");
        hipLaunchKernelGGL(k_pgo_assemble_b, dim3(maxNf, nl), dim3(64), 0, st, dTab, dCtl, dPos, dRow, dInc, dE, dRes, dJi, dJj, dBandH, dDiag, dG);
        timer.end(t);
        t = timer.begin("pgo_band_chol");
        hipLaunchKernelGGL(k_pgo_band_copy_b, dim3((unsigned)((maxBand + 255) / 256), nl), dim3(256), 0, st, dTab, dCtl, dBandH, dG, dBandL, dRhs);
        hipLaunchKernelGGL(k_pgo_band_chol_b, dim3(nl), dim3(PGO_CHOL_NT), 0, st, dTab, dCtl, dBandL, dDiag, dRhs, dDelta, dFlag);
        timer.end(t);
        t = timer.begin("pgo_retract");
        hipLaunchKernelGGL(k_pgo_retract_b, gPose, dim3(256), 0, st, dTab, dCtl, dPos, dP0, dP1, dDelta);
        timer.end(t);
        t = timer.begin("pgo_cost");
        hipLaunchKernelGGL(k_pgo_cost_b, gEdge, dim3(256), 0, st, dTab, dCtl, dE, dP0, dP1, dCost);
        VS_CHECK(decide(0, t));
    }
    std::vector<PgoCtl> ctl(nl);
    VS_HIP(pool->d2h(ctl.data(), dCtl, nl * sizeof(PgoCtl)));
    VS_HIP(pool->sync());
    for (int l = 0; l < nl; l++)
        if (ctl[l].accepted) VS_HIP(pool->d2h(prep[l].hp.data(), (ctl[l].cur ? dP1 : dP0) + (size_t)tab[l].pose0 * 12, (size_t)prep[l].n * 12 * sizeof(double)));
    VS_HIP(pool->sync());
    if (timer.enabled) {
        const char* names[8]; float ms[8];
        const int k = timer.read(names, ms, 8);
        g_pgoTimes.clear();
        for (int q = 0; q < k; q++) g_pgoTimes.push_back({names[q], ms[q]});
    }
    for (int l = 0; l < nl; l++) {
        const vslam_pgo_graph& Q = graphs[live[l]];
        const PgoPrep& G = prep[l];
        pgo_write_out(G, G.hp.data(), Q.T_wc, Q.T_wc_out);
        vslam_pgo_report& R = reports[live[l]];
        R = vslam_pgo_report{};
        R.n_free = G.nf; R.n_isolated = G.nIso; R.half_bandwidth = G.b;
        R.accepted = ctl[l].accepted; R.rejected = ctl[l].rejected; R.iterations = ctl[l].accepted + ctl[l].rejected;
        R.initial_cost = ctl[l].initial_cost; R.final_cost = ctl[l].cost; R.final_lambda = ctl[l].lambda;
    }
    return VSLAM_OK;
}

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
    return pgo_solve(who, false, &graph, 1, maxIt, lambda0, device, report);
}

extern "C" vslam_status vslam_pose_graph_optimize_batch(const vslam_pgo_graph* graphs, int32_t lanes, const vslam_pgo_params* params,
                                                        int32_t device, vslam_pgo_report* reports) {
    static const char* const who = "vslam_pose_graph_optimize_batch";
    if (!graphs || !reports || lanes < 1) { set_error("%s: invalid arguments", who); return VSLAM_ERR_INVALID; }
    if (lanes > PGO_MAX_LANES) { set_error("%s: %d lanes exceed the limit (%d)", who, lanes, PGO_MAX_LANES); return VSLAM_ERR_CAPACITY; }
    int maxIt = 0;
    double lambda0 = 0.0;
    VS_CHECK(pgo_check_params(who, params, &maxIt, &lambda0));
    return pgo_solve(who, true, graphs, lanes, maxIt, lambda0, device, reports);
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
