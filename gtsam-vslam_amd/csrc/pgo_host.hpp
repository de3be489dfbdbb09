// Host side that the pose-graph solves share (pgo.hip: 6-DoF, 6x6 blocks; pgo_yaw.hip: yaw-only, 4x4 blocks): the lane table, the
// limits, validation, the gauge check, the numbering and reordering of the free poses, the incidence lists, the packing and the
// layout of the device blocks, and THE driver of a solve (pgo_solve), a template over the solve's kernel set.  Validation and ordering do
// not depend on the block dimension (a band's capacity is counted in blocks); the driver takes it from the kernel set.
#pragma once
#include "common.hpp"
#include "pgo_dev.hpp"
#include "pgo_order_host.hpp"
#include <cmath>
#include <numeric>

namespace vslam {
// the measurement hook's thread-local state (vslam_pose_graph_set_timing / vslam_pose_graph_timings, defined in pgo.hip)
std::vector<std::pair<const char*, float>>& pgo_times();
bool& pgo_timing_on();
long long& pgo_solve_count();      // solves (single or batched calls, either kind) that reached the device on this thread since set_timing
}

namespace {

constexpr int PGO_MAX_LANES = 1024;                 // (the decide kernels are ONE workgroup with a thread per lane)
constexpr int PGO_SUM_POSES = 262144, PGO_SUM_EDGES = 1048576, PGO_SUM_BLOCKS = 1048576;

struct PgoLane {
    int n, m, nf, b;
    int pose0, edge0;      // first pose (poses, pos), first edge (edges, res, Ji, Jj, cost)
    int free0, row0;       // first band position (diagH, g, rhs, delta: x block dimension), first entry of the lane's nf + 1 row starts
    int inc0, band0;       // first incidence entry, first band block (x block size)
};

inline bool finite16(const double* p, int n) { for (int k = 0; k < n; k++) if (!std::isfinite(p[k])) return false; return true; }

// what every entry point does before its first device call: `device` names a device, the calling thread's pool with nothing pending
inline vslam_status pgo_device_pool(int device, DevPool** out) {
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

// What the host derives from one graph before anything is launched: the free poses' band positions, the band width, the incidence
// lists and the device forms of edges and poses.  Every lane goes through pgo_check_sizes and pgo_prepare; `who` (the entry
// point, with the lane for a batched call) starts every error text.
struct PgoPrep {
    int n = 0, m = 0, nf = 0, nIso = 0, b = 0;
    std::vector<int> pos, rowStart, inc;      // pos [n]: band position or -1; rowStart [nf + 1]; inc: edge << 1 | side, ascending
    std::vector<PgoEdge> he;
    std::vector<double> hp;                   // [n][12]
};

inline vslam_status pgo_check_sizes(const char* who, const double* T_wc, const uint8_t* fixed, int n, const vslam_pgo_edge* edges, int m, const double* T_wc_out) {
    if (!T_wc || !fixed || !T_wc_out || n < 1 || m < 0 || (m > 0 && !edges)) { set_error("%s: invalid arguments", who); return VSLAM_ERR_INVALID; }
    if (n > PGO_MAX_POSES || m > PGO_MAX_EDGES) { set_error("%s: %d poses / %d edges exceed the limits (%d / %d)", who, n, m, PGO_MAX_POSES, PGO_MAX_EDGES); return VSLAM_ERR_CAPACITY; }
    return VSLAM_OK;
}

inline vslam_status pgo_check_params(const char* who, const vslam_pgo_params* params, int* maxIt, double* lambda) {
    *maxIt = params ? params->max_iterations : 0;
    *lambda = params ? params->lambda0 : 0.0;
    if (*maxIt < 0 || !(*lambda >= 0.0) || !std::isfinite(*lambda)) { set_error("%s: negative or non-finite parameter", who); return VSLAM_ERR_INVALID; }
    if (*maxIt == 0) *maxIt = 20;
    if (*lambda == 0.0) *lambda = 1e-4;
    return VSLAM_OK;
}

inline vslam_status pgo_prepare(const char* who, const double* T_wc, const uint8_t* fixed, int n, const vslam_pgo_edge* edges, int m, PgoPrep& G) {
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
inline void pgo_write_out(const PgoPrep& G, const double* hp, const double* T_wc, double* T_wc_out) {
    for (int k = 0; k < G.n; k++) {
        double* o = T_wc_out + (size_t)k * 16;
        if (G.pos[k] < 0) { if (o != T_wc + (size_t)k * 16) memcpy(o, T_wc + (size_t)k * 16, 16 * sizeof(double)); continue; }
        for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) o[4 * r + c] = hp[(size_t)k * 12 + 3 * r + c]; o[4 * r + 3] = hp[(size_t)k * 12 + 9 + r]; }
        o[12] = o[13] = o[14] = 0.0; o[15] = 1.0;
    }
}

// The device arrays of a solve, as the kernel sets' launch functions take them
struct PgoDev {
    const void* tab; PgoCtl* ctl; const PgoEdge* E;
    double *P0, *P1, *res, *Ji, *Jj, *cost, *bandH, *bandL, *diag, *g, *rhs, *delta, *out;
    const int *pos, *row, *inc;
    int *flag, *act;
};

// THE solve, behind every optimise entry point: `lanes` graphs, the checked parameters.  K is the kernel set of a solve (pgo.hip:
// 6 parameters per pose, 6x6 blocks; pgo_yaw.hip: 4 and 4x4 with an axis per lane):
//   K::D, K::BLK, K::JAC          parameters per pose, doubles per band block, doubles per Jacobian
//   K::Graph, K::graph(Graph&)    a lane as the caller passes it, and its vslam_pgo_graph
//   K::Lane, K::lane(...)         the device table's entry, filled from the PgoLane and the caller's lane (may refuse: the axis)
//   K::linearize / assemble / band / retract / cost / decide   the launches of a round; K::names: their timer groups
// A lane with n == 0 is idle (the single calls never pass one).  Host work per lane is pgo_prepare; the lanes' arrays then go up as
// ONE block (table, control blocks, edges, poses, positions, incidence lists) and the device's own arrays are one more block from
// the thread's cache.  A round is one trial of every active lane: eight launches and one wait, for a single int (how many lanes
// are still active).  `who` starts every error text, with the lane where `nameLane` says so.  Nothing is written before the
// last wait has returned.
template <class K>
vslam_status pgo_solve(const char* who, bool nameLane, const typename K::Graph* graphs, int lanes, int maxIt, double lambda0, int device,
                       vslam_pgo_report* reports) {
    char lw[96];
    auto lane_text = [&](int g) { if (nameLane) snprintf(lw, sizeof lw, "%s: lane %d", who, g); else snprintf(lw, sizeof lw, "%s", who); return lw; };
    std::vector<int> live;                  // the lanes that hold a graph, in call order: the device's lanes
    long long sumN = 0, sumM = 0;
    for (int g = 0; g < lanes; g++) {
        const vslam_pgo_graph& Q = K::graph(graphs[g]);
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
    std::vector<typename K::Lane> dtab(std::max(nl, 1));
    long long sumB = 0;
    int N = 0, M = 0, NF = 0, INC = 0, maxN = 0, maxM = 0, maxNf = 0;
    size_t maxBand = 0;                     // doubles of the largest lane's band
    for (int l = 0; l < nl; l++) {
        const vslam_pgo_graph& Q = K::graph(graphs[live[l]]);
        VS_CHECK(pgo_prepare(lane_text(live[l]), Q.T_wc, Q.fixed, Q.n, Q.edges, Q.m, prep[l]));
        const PgoPrep& G = prep[l];
        if (sumB + (long long)(G.b + 1) * G.nf > PGO_SUM_BLOCKS) {
            set_error("%s: the lanes' bands need more than %d blocks in all (reached at lane %d)", who, PGO_SUM_BLOCKS, live[l]);
            return VSLAM_ERR_CAPACITY;
        }
        tab[l] = PgoLane{G.n, G.m, G.nf, G.b, N, M, NF, NF + l, INC, (int)sumB};
        VS_CHECK(K::lane(lane_text(live[l]), tab[l], graphs[live[l]], dtab[l]));
        N += G.n; M += G.m; NF += G.nf; INC += G.rowStart[G.nf]; sumB += (long long)(G.b + 1) * G.nf;
        maxN = std::max(maxN, G.n); maxM = std::max(maxM, G.m); maxNf = std::max(maxNf, G.nf);
        maxBand = std::max(maxBand, (size_t)(G.b + 1) * G.nf * K::BLK);
    }
    if (nl == 0) return VSLAM_OK;           // (every lane idle: nothing to solve, nothing written)
    DevPool* pool = nullptr;
    VS_CHECK(pgo_device_pool(device, &pool));
    hipStream_t st = pool->stream;
    pgo_solve_count()++;

    PgoLayout up, wk;                       // the upload block and the work block
    const size_t oTab = up.section(nl * sizeof(typename K::Lane)), oCtl = up.section(nl * sizeof(PgoCtl));
    const size_t oE = up.section((size_t)M * sizeof(PgoEdge)), oP0 = up.section((size_t)N * 12 * sizeof(double));
    const size_t oPos = up.section((size_t)N * sizeof(int)), oRow = up.section((size_t)(NF + nl) * sizeof(int));
    const size_t oInc = up.section((size_t)INC * sizeof(int));
    const size_t bandBytes = (size_t)sumB * K::BLK * sizeof(double), vecBytes = (size_t)NF * K::D * sizeof(double);
    const size_t oP1 = wk.section((size_t)N * 12 * sizeof(double)), oRes = wk.section((size_t)M * 6 * sizeof(double));
    const size_t oJi = wk.section((size_t)M * K::JAC * sizeof(double)), oJj = wk.section((size_t)M * K::JAC * sizeof(double));
    const size_t oCost = wk.section((size_t)M * sizeof(double));
    const size_t oBandH = wk.section(bandBytes), oBandL = wk.section(bandBytes);
    const size_t oDiag = wk.section(vecBytes), oG = wk.section(vecBytes), oRhs = wk.section(vecBytes), oDelta = wk.section(vecBytes);
    const size_t oOut = wk.section((size_t)nl * 2 * sizeof(double)), oFlag = wk.section((size_t)nl * sizeof(int));
    const size_t oAct = wk.section(sizeof(int));
    std::vector<uint8_t> hUp(up.bytes, 0);
    memcpy(hUp.data() + oTab, dtab.data(), nl * sizeof(typename K::Lane));
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
    PgoDev d{};
    d.tab = dUp.p + oTab; d.ctl = (PgoCtl*)(dUp.p + oCtl); d.E = (const PgoEdge*)(dUp.p + oE); d.P0 = (double*)(dUp.p + oP0);
    d.pos = (const int*)(dUp.p + oPos); d.row = (const int*)(dUp.p + oRow); d.inc = (const int*)(dUp.p + oInc);
    d.P1 = (double*)(dWk.p + oP1); d.res = (double*)(dWk.p + oRes); d.Ji = (double*)(dWk.p + oJi); d.Jj = (double*)(dWk.p + oJj);
    d.cost = (double*)(dWk.p + oCost); d.bandH = (double*)(dWk.p + oBandH); d.bandL = (double*)(dWk.p + oBandL);
    d.diag = (double*)(dWk.p + oDiag); d.g = (double*)(dWk.p + oG); d.rhs = (double*)(dWk.p + oRhs); d.delta = (double*)(dWk.p + oDelta);
    d.out = (double*)(dWk.p + oOut); d.flag = (int*)(dWk.p + oFlag); d.act = (int*)(dWk.p + oAct);

    struct TimerOwner { StageTimer t; ~TimerOwner() { t.destroy(); } } timerOwner;      // (the events go on every return path)
    StageTimer& timer = timerOwner.t;
    timer.stream = st; timer.multi = true; timer.enabled = pgo_timing_on();
    const dim3 gEdge((maxM + 255) / 256, nl), gPose((maxN + 255) / 256, nl);
    int nActive = 0;
    auto decide = [&](int init, int t) -> vslam_status {        // closes the cost group `t`, then the round's one wait
        K::decide(st, nl, init, maxIt, d);
        timer.end(t);
        VS_HIP(hipGetLastError());
        VS_HIP(pool->d2h(&nActive, d.act, sizeof(int)));
        VS_HIP(pool->sync());
        return VSLAM_OK;
    };
    int t = timer.begin(K::names[0]);
    if (maxM) K::linearize(st, gEdge, 1, d);
    timer.end(t);
    VS_CHECK(decide(1, timer.begin(K::names[4])));
    while (nActive > 0) {       // one round
        t = timer.begin(K::names[0]);
        K::linearize(st, gEdge, 0, d);
        timer.end(t);
        t = timer.begin(K::names[1]);
        K::assemble(st, maxNf, nl, d);
        timer.end(t);
        t = timer.begin(K::names[2]);
        K::band(st, maxBand, nl, d);
        timer.end(t);
        t = timer.begin(K::names[3]);
        K::retract(st, gPose, d);
        timer.end(t);
        t = timer.begin(K::names[4]);
        K::cost(st, gEdge, d);
        VS_CHECK(decide(0, t));
    }
    std::vector<PgoCtl> ctl(nl);
    VS_HIP(pool->d2h(ctl.data(), d.ctl, nl * sizeof(PgoCtl)));
    VS_HIP(pool->sync());
    for (int l = 0; l < nl; l++)
        if (ctl[l].accepted) VS_HIP(pool->d2h(prep[l].hp.data(), (ctl[l].cur ? d.P1 : d.P0) + (size_t)tab[l].pose0 * 12, (size_t)prep[l].n * 12 * sizeof(double)));
    VS_HIP(pool->sync());
    if (timer.enabled) {
        const char* names[8]; float ms[8];
        const int k = timer.read(names, ms, 8);
        pgo_times().clear();
        for (int q = 0; q < k; q++) pgo_times().push_back({names[q], ms[q]});
    }
    for (int l = 0; l < nl; l++) {
        const vslam_pgo_graph& Q = K::graph(graphs[live[l]]);
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
