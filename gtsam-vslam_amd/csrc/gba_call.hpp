// Host side of one global-BA call, shared by gba.hip (vslam_global_ba / _batch) and gba_yaw.hip (vslam_global_ba_yaw / _batch):
// the argument and parameter checks, what the host derives from one problem before anything is launched (the plan of
// gba_host.hpp and the device forms of poses, edges, whitening factors and chi2 thresholds), the write-out of a solved problem
// and the timing hook's state.  Nothing here depends on how a keyframe is parameterised.
#pragma once
#include "common.hpp"
#include "pgo_dev.hpp"
#include "gba_host.hpp"
#include <cmath>

namespace vslam {
// vslam_global_ba_set_timing / _timings (defined in gba.hip): the calling thread's switch and its last call's groups
extern thread_local std::vector<std::pair<const char*, float>> g_gbaTimes;
extern thread_local bool g_gbaTimingOn;
}  // namespace vslam

namespace {

using namespace vslam;

struct GbaLayout {
    size_t bytes = 0;
    size_t section(size_t n) { const size_t at = bytes; bytes = align_up_sz(bytes + std::max<size_t>(n, 8), 256); return at; }
};

inline bool gba_finite(const double* p, size_t n) { for (size_t k = 0; k < n; k++) if (!std::isfinite(p[k])) return false; return true; }
inline unsigned gba_grid(size_t n) { return (unsigned)((n + 255) / 256); }

// What the host derives from one problem before anything is launched, for the single call and for every lane of the batched one:
// the plan (gba_host.hpp) and the device forms of poses, edges, whitening factors and chi2 thresholds.  `who` (the entry point,
// with the lane for a batched call) starts every error text.
struct GbaPrep {
    GbaPlan G;
    std::vector<double> hp, his, hthr;      // poses [K][12]; per factor slot [P][2]
    std::vector<PgoEdge> he;
};

inline vslam_status gba_check_args(const char* who, const vslam_ba_problem& Q, const vslam_pgo_edge* edges, int M, const vslam_gba_result* result) {
    const int K = Q.n_kf, L = Q.n_lm, P = Q.n_pairs;
    if (K < 1 || L < 0 || P < 0 || M < 0 || !Q.kf_pose_wc || !Q.kf_fixed || !Q.kf_local || !result->kf_pose_wc || (L > 0 && (!Q.lm_xyz || !result->lm_xyz)) ||
        (P > 0 && (!Q.pair_kf || !Q.pair_lm || !Q.pair_flags || !Q.pair_uv || !Q.pair_octave || !result->pair_wrong || !Q.sigma_factor || !Q.inv_sigma_factor || Q.n_levels < 1)) ||
        (M > 0 && !edges)) {
        set_error("%s: invalid arguments", who); return VSLAM_ERR_INVALID;
    }
    // the plan's limits come first (the edge ends are copied only after them)
    static const int32_t none = 0;
    GbaIndex I;
    I.n_kf = K; I.kf_fixed = Q.kf_fixed; I.n_lm = L; I.n_pairs = P; I.pair_kf = Q.pair_kf; I.pair_lm = Q.pair_lm; I.pair_flags = Q.pair_flags;
    I.n_edges = M; I.edge_i = &none; I.edge_j = &none;
    GbaPlan G;
    if (const int st = gba_check_sizes(I, G)) { set_error("%s: %s", who, G.err.c_str()); return (vslam_status)st; }
    return VSLAM_OK;
}

// (after gba_check_args) host plan: presence, free set, gauge, reordering, lists; then every value is checked and converted
inline vslam_status gba_prepare(const char* who, const vslam_ba_problem& Q, const vslam_pgo_edge* edges, int M, GbaPrep& R) {
    const int K = Q.n_kf, L = Q.n_lm, P = Q.n_pairs;
    std::vector<int32_t> ei(std::max(M, 1)), ej(std::max(M, 1));
    GbaIndex I;
    I.n_kf = K; I.kf_fixed = Q.kf_fixed; I.n_lm = L; I.n_pairs = P; I.pair_kf = Q.pair_kf; I.pair_lm = Q.pair_lm; I.pair_flags = Q.pair_flags;
    I.n_edges = M; I.edge_i = ei.data(); I.edge_j = ej.data();
    GbaPlan& G = R.G;
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
    // device forms: poses [12], whitening and chi2 threshold per factor slot; the initial depth of every present factor
    std::vector<double>& hp = R.hp; std::vector<double>& his = R.his; std::vector<double>& hthr = R.hthr;
    hp.assign((size_t)K * 12, 0.0); his.assign((size_t)std::max(P, 1) * 2, 0.0); hthr.assign((size_t)std::max(P, 1) * 2, 0.0);
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
    R.he.assign(std::max(M, 1), PgoEdge{});
    for (int e = 0; e < M; e++) {
        PgoEdge& o = R.he[e];
        o.i = edges[e].i; o.j = edges[e].j; o.wr = edges[e].w_rot; o.wt = edges[e].w_trans;
        for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) o.Rz[3 * r + c] = edges[e].Z[4 * r + c]; o.tz[r] = edges[e].Z[4 * r + 3]; }
    }
    return VSLAM_OK;
}

// The solved values into the caller's arrays (hp [K][12], hl [L][3], hw [P] from the device) and the report.  Fixed and isolated
// keyframes and thin landmarks are the input's bytes.  The outputs may be the problem's arrays.
inline void gba_write_out(const vslam_ba_problem& Q, const GbaPlan& G, const double* hp, const double* hl, const uint8_t* hw, const PgoCtl& ctl, vslam_gba_result* result) {
    const int K = Q.n_kf, L = Q.n_lm, P = Q.n_pairs;
    for (int k = 0; k < K; k++) {
        double* o = result->kf_pose_wc + (size_t)k * 16;
        const double* in = Q.kf_pose_wc + (size_t)k * 16;
        if (G.pos[k] < 0) { if (o != in) memcpy(o, in, 128); continue; }
        for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) o[4 * r + c] = hp[(size_t)k * 12 + 3 * r + c]; o[4 * r + 3] = hp[(size_t)k * 12 + 9 + r]; }
        o[12] = o[13] = o[14] = 0.0; o[15] = 1.0;
    }
    for (int l = 0; l < L; l++) {
        double* o = result->lm_xyz + (size_t)l * 3;
        const double* in = G.lmPresent[l] ? hl + (size_t)l * 3 : Q.lm_xyz + (size_t)l * 3;
        if (o != in) memcpy(o, in, 24);
    }
    if (P) memcpy(result->pair_wrong, hw, (size_t)P);
    vslam_gba_report& R = result->report;
    R = vslam_gba_report{};
    R.accepted = ctl.accepted; R.rejected = ctl.rejected; R.iterations = ctl.accepted + ctl.rejected;
    R.n_free = G.nf; R.n_isolated = G.nIso; R.n_present = G.nPresent; R.n_thin = G.nThin; R.n_factors = G.nFactors; R.half_bandwidth = G.b;
    R.initial_cost = ctl.initial_cost; R.final_cost = ctl.cost; R.final_lambda = ctl.lambda;
}

inline vslam_status gba_check_params(const char* who, const vslam_gba_params* params, int* maxIt, double* lambda0) {
    *maxIt = params ? params->max_iterations : 0;
    *lambda0 = params ? params->lambda0 : 0.0;
    if (*maxIt < 0 || !(*lambda0 >= 0.0) || !std::isfinite(*lambda0)) { set_error("%s: negative or non-finite parameter", who); return VSLAM_ERR_INVALID; }
    if (*maxIt == 0) *maxIt = 20;
    if (*lambda0 == 0.0) *lambda0 = 1e-4;
    return VSLAM_OK;
}

}  // namespace
