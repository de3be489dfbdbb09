// Loop closing of a stereo session (no reference counterpart; vslam_hip.h): the relocalisation
// stage asked on the part of the map the tracker has left behind, a pose graph over the keyframes solved by
// vslam_pose_graph_optimize, and the commit that hands the old copy of the place back to the tracker.  vslam_system_fuse_loop (item 26)
// then makes one map point of each landmark the two visits both triangulated; vslam_system_global_ba (item 27) runs one bundle
// adjustment over the whole map.  Each of the three calls is a sequence of stages that vslam_batch (batch.hip) runs for its lanes
// too, with the device work of all lanes in one batched call between them (items 25 and 28).
#include "system.hpp"
#include "fuse_host.hpp"
#include <array>
#include <set>

using namespace vslam;
using namespace vslam_sys;

bool vslam_sys::resolve_loop_params(const vslam_loop_params* prm, vslam_loop_params& P) {
    P = prm ? *prm : vslam_loop_params{};
    if (P.min_kf_gap < 0 || P.covis_min < 0 || !(P.loop_weight >= 0.0) || !std::isfinite(P.loop_weight)) return false;
    if (P.min_kf_gap == 0) P.min_kf_gap = 20;
    if (P.covis_min == 0) P.covis_min = 100;
    if (P.loop_weight == 0.0) P.loop_weight = 10.0;
    return true;
}

vslam_status vslam_system::loop_check(const char* fn) const {
    if (monoMode) { set_error("%s: a mono session cannot close loops (stereo fixes the scale of the correction)", fn); return VSLAM_ERR_INVALID; }
    if (cfg.use_imu) { set_error("%s: an IMU session cannot close loops yet (its velocity and gravity frame would have to follow)", fn); return VSLAM_ERR_INVALID; }
    if (keyFrames.empty()) { set_error("%s: no tracked frame yet", fn); return VSLAM_ERR_INVALID; }
    return VSLAM_OK;
}

// map points that are not outliers, not active, created at least minKfGap keyframes ago; creation order, the most recent 65536
int vslam_system::loop_candidates(int minKfGap) {
    std::lock_guard<std::mutex> lk(mapMutex);
    rlIds.clear();
    std::vector<uint8_t> isActive(mapPoints.size(), 0);
    for (int a : active) isActive[a] = 1;
    const long long newest = (long long)latestKF - minKfGap;
    for (int m = 0; m < (int)mapPoints.size(); m++)
        if (!mpOutlier[m] && !isActive[m] && mapPoints[m].kdx <= newest) rlIds.push_back(m);
    if (rlIds.size() > 65536) rlIds.erase(rlIds.begin(), rlIds.end() - 65536);
    return (int)rlIds.size();
}

// stage 1 (mapMutex held): a finished local BA is propagated, then the graph over every keyframe and the map points' references
vslam_status vslam_system::loop_build(int kfLoop, const M4& T_corr, const vslam_loop_params& P, vslam_loop_report* rep, LoopGraph& G) {
    if (LBADone) {                                         // a finished local BA is propagated first, as the next frame would
        VS_CHECK(change_poses_lca(endLBAIdx));
        LBADone = false;
    }
    const int K = (int)keyFrames.size();
    G.K = K;
    G.poses.assign((size_t)K * 16, 0.0); G.fresh.assign((size_t)K * 16, 0.0);
    G.fixed.assign(K, 0);
    G.fixed[0] = G.fixed[kfLoop] = 1;
    for (int k = 0; k < K; k++) memcpy(&G.poses[16 * (size_t)k], keyFrames[k].pose.data(), 16 * sizeof(double));
    std::vector<vslam_pgo_edge>& edges = G.edges;
    edges.clear();
    auto add = [&](int a, int b, const M4& Z, double w) {
        vslam_pgo_edge e{};
        e.i = a; e.j = b; e.w_rot = e.w_trans = w;
        memcpy(e.Z, Z.data(), 16 * sizeof(double));
        edges.push_back(e);
    };
    for (int k = 0; k < K; k++) {
        const int p = keyFrames[k].prevKF;
        if (p >= 0) add(p, k, m4_mul(keyFrames[p].poseInv, keyFrames[k].pose), 1.0);
    }
    rep->n_sequential = (int)edges.size();
    std::set<std::pair<int, int>> seen;
    for (int k = 0; k < K; k++)
        for (const auto& c : keyFrames[k].sortedKFWeights) {
            if (c.first < P.covis_min || c.second == k || c.second < 0 || c.second >= K) continue;
            const int a = std::min(k, c.second), b = std::max(k, c.second);
            if (!seen.insert({a, b}).second) continue;
            add(a, b, m4_mul(keyFrames[a].poseInv, keyFrames[b].pose), 1.0);
        }
    rep->n_covisibility = (int)edges.size() - rep->n_sequential;
    const M4 D = m4_mul(T_corr, camPoseInv);
    add(kfLoop, latestKF, m4_mul(keyFrames[kfLoop].poseInv, m4_mul(D, keyFrames[latestKF].pose)), P.loop_weight);
    rep->n_nodes = K; rep->n_edges = (int)edges.size();
    const int nMp = (int)mapPoints.size();
    G.nMp = nMp; G.nMoved = 0;
    G.xyz.assign((size_t)std::max(nMp, 1) * 3, 0.0); G.moved.assign((size_t)std::max(nMp, 1) * 3, 0.0);
    G.ref.assign(std::max(nMp, 1), -1);
    for (int m = 0; m < nMp; m++) {
        const SysMP& mp = mapPoints[m];
        for (int c = 0; c < 3; c++) G.xyz[3 * (size_t)m + c] = mp.wp[c];
        if (!mp.kfm.empty()) { G.ref[m] = mp.kfm[0].kf; G.nMoved++; }
    }
    return VSLAM_OK;
}

// stage 3 (mapMutex held): G.fresh and G.moved into the map
void vslam_system::loop_commit(const LoopGraph& G, vslam_loop_report* rep) {
    const int K = G.K;
    for (int m = 0; m < G.nMp; m++) for (int c = 0; c < 3; c++) mapPoints[m].wp[c] = G.moved[3 * (size_t)m + c];
    for (int k = 0; k < K; k++) keyFrames[k].setPose(m4_from(&G.fresh[16 * (size_t)k]));
    for (int k = 0; k < K; k++) {
        const int p = keyFrames[k].prevKF;
        if (p >= 0) keyFrames[k].refPose = m4_mul(keyFrames[p].poseInv, keyFrames[k].pose);
    }
    lca_finish(latestKF);
    rep->points_moved = G.nMoved;
}

// the active set: reloc_commit's rule under the new camera pose
vslam_status vslam_system::loop_activate(vslam_loop_report* rep) {
    const size_t n = (size_t)reloc_candidates();
    std::vector<double> xyz(3 * std::max<size_t>(n, 1)); std::vector<uint8_t> desc(32 * std::max<size_t>(n, 1)); std::vector<float> msd(std::max<size_t>(n, 1));
    reloc_fill_upload(xyz.data(), desc.data(), msd.data());
    std::vector<float> pl(2 * std::max<size_t>(n, 1)), pr(2 * std::max<size_t>(n, 1)); std::vector<int> ll(std::max<size_t>(n, 1)), lr(std::max<size_t>(n, 1));
    std::vector<uint8_t> inF(std::max<size_t>(n, 1)), inFR(std::max<size_t>(n, 1));
    if (n) VS_CHECK(vslam_world_to_frame(fm, camPoseInv.data(), (int)n, xyz.data(), msd.data(), (float)std::log((double)cfg.fe.scale), pl.data(), pr.data(),
                                         ll.data(), lr.data(), inF.data(), inFR.data()));
    {
        std::lock_guard<std::mutex> lk(mapMutex);
        active.clear();
        for (size_t j = 0; j < n; j++) {
            mpInFrame[rlIds[j]] = inF[j];
            if (inF[j]) active.push_back(rlIds[j]);
        }
        lastMatches.clear(); lastOutliers.clear();
        rep->n_active_after = (int)active.size();
    }
    rep->corrected = 1;
    return VSLAM_OK;
}

vslam_status vslam_system::loop_apply(int kfLoop, const M4& T_corr, const vslam_loop_params& P, vslam_loop_report* rep) {
    VS_HIP(hipSetDevice(cfg.device));
    {
        std::lock_guard<std::mutex> lk(mapMutex);
        LoopGraph G;
        VS_CHECK(loop_build(kfLoop, T_corr, P, rep, G));
        VS_CHECK(vslam_pose_graph_optimize(G.poses.data(), G.fixed.data(), G.K, G.edges.data(), (int)G.edges.size(), &P.pgo, cfg.device, G.fresh.data(), &rep->pgo));
        VS_CHECK(vslam_pose_graph_move_points(G.xyz.data(), G.ref.data(), G.poses.data(), G.fresh.data(), G.nMp, G.K, cfg.device, G.moved.data()));
        loop_commit(G, rep);
    }
    return loop_activate(rep);
}

void vslam_sys::loop_drift(const M4& T_corr, const M4& camPoseInv, vslam_loop_report* rep) {
    const M4 D = m4_mul(T_corr, camPoseInv);
    rep->drift_translation = std::sqrt(D[3] * D[3] + D[7] * D[7] + D[11] * D[11]);
    const double c = std::min(1.0, std::max(-1.0, (D[0] + D[5] + D[10] - 1.0) / 2.0));
    rep->drift_rotation = std::acos(c);
    memcpy(rep->T_wc_corrected, T_corr.data(), 16 * sizeof(double));
}

vslam_status vslam_system::loop_check_correct(const char* fn, int kfLoop, const double* T_wc_corrected) const {
    if (kfLoop < 0 || kfLoop >= (int)keyFrames.size() || kfLoop == latestKF) {
        set_error("%s: kf_loop %d (keyframes 0 .. %d, the latest excluded)", fn, kfLoop, (int)keyFrames.size() - 1);
        return VSLAM_ERR_INVALID;
    }
    for (int k = 0; k < 16; k++) if (!std::isfinite(T_wc_corrected[k])) { set_error("%s: non-finite pose", fn); return VSLAM_ERR_INVALID; }
    return VSLAM_OK;
}

vslam_status vslam_system::loop_check_close(const char* fn) const {
    if (!fm->stereoDone) { set_error("%s: the matcher holds no frame", fn); return VSLAM_ERR_INVALID; }
    return VSLAM_OK;
}

vslam_status vslam_system::correct_loop(int kfLoop, const double* T_wc_corrected, const vslam_loop_params* prm, vslam_loop_report* rep) {
    if (!T_wc_corrected || !rep) return VSLAM_ERR_INVALID;
    VS_CHECK(loop_check("vslam_system_correct_loop"));
    vslam_loop_params P;
    if (!resolve_loop_params(prm, P)) { set_error("vslam_system_correct_loop: negative or non-finite parameter"); return VSLAM_ERR_INVALID; }
    VS_CHECK(loop_check_correct("vslam_system_correct_loop", kfLoop, T_wc_corrected));
    *rep = vslam_loop_report{};
    rep->kf_loop = kfLoop;
    if (loop_busy()) { rep->busy = 1; return VSLAM_OK; }
    rep->success = 1;
    const M4 T_corr = m4_from(T_wc_corrected);
    loop_drift(T_corr, camPoseInv, rep);
    return loop_apply(kfLoop, T_corr, P, rep);
}

// kf_loop: the keyframe (not the latest) that observes the most inliers of the winning hypothesis
vslam_status vslam_system::loop_vote(const int* pairs, size_t n, const uint8_t* flags, int C, const char* fn, int* kfLoop) {
    *kfLoop = -1;
    std::vector<std::pair<int, int>> byKey;                // (key, candidate): correspondences are in ascending key order
    for (size_t p = 0; p < n; p++) if (pairs[p] >= 0) byKey.push_back({pairs[p], (int)p});
    std::sort(byKey.begin(), byKey.end());
    if ((int)byKey.size() != C) { set_error("%s: %d correspondences, %d pairs", fn, C, (int)byKey.size()); return VSLAM_ERR_HIP; }
    std::lock_guard<std::mutex> lk(mapMutex);
    std::vector<int> votes(keyFrames.size(), 0);
    for (int c = 0; c < C; c++) {
        if (!flags[c]) continue;
        for (const KfMatch& o : mapPoints[rlIds[byKey[c].second]].kfm) if (o.kf != latestKF) votes[o.kf]++;
    }
    int best = -1;
    for (int k = 0; k < (int)votes.size(); k++) if (votes[k] > 0 && (best < 0 || votes[k] > votes[best])) best = k;
    *kfLoop = best;
    return VSLAM_OK;
}

// close_loop's detection, shared with close_loop_imu: candidates, the relocalisation stage on the frame the matcher holds, the vote.
// rep->success and rep->kf_loop say whether a loop was found; T_corr is the claimed pose then.  Nothing of the session changes.
vslam_status vslam_system::loop_detect(const char* fn, const vslam_loop_params& P, const vslam_reloc_params& RP, vslam_loop_report* rep, M4& T_corr) {
    const size_t n = (size_t)loop_candidates(P.min_kf_gap);
    rep->n_candidates = (int)n;
    rep->reloc.n_points = (int)n;
    if ((int)n < RP.min_inliers) return VSLAM_OK;
    VS_HIP(hipSetDevice(cfg.device));
    std::vector<double> xyz(3 * n); std::vector<uint8_t> desc(32 * n); std::vector<float> msd(n);
    reloc_fill_upload(xyz.data(), desc.data(), msd.data());
    std::vector<int> pairs(n, -1);
    double T_cw[16];
    {
        // step D may clear stereo matches of the frame the matcher holds: saved here, restored below, so that nothing of the stage
        // reaches the session
        DevPool* pool = thread_pool(cfg.device);
        if (!pool) { set_error("no device pool"); return VSLAM_ERR_HIP; }
        const size_t c = (size_t)fm->cap;
        PoolBuf<uint8_t> save(pool);
        VS_HIP(save.alloc(c * 16));
        uint8_t* s = save.p;
        VS_HIP(hipMemcpyAsync(s, fm->d_rightIdxs, c * 4, hipMemcpyDeviceToDevice, fm->stream));
        VS_HIP(hipMemcpyAsync(s + c * 4, fm->d_leftIdxs, c * 4, hipMemcpyDeviceToDevice, fm->stream));
        VS_HIP(hipMemcpyAsync(s + c * 8, fm->d_depth, c * 4, hipMemcpyDeviceToDevice, fm->stream));
        VS_HIP(hipMemcpyAsync(s + c * 12, fm->d_close, c, hipMemcpyDeviceToDevice, fm->stream));
        const vslam_status st = fm->relocalize(xyz.data(), desc.data(), (int)n, &P.reloc, T_cw, pairs.data(), &rep->reloc);
        VS_HIP(hipMemcpyAsync(fm->d_rightIdxs, s, c * 4, hipMemcpyDeviceToDevice, fm->stream));
        VS_HIP(hipMemcpyAsync(fm->d_leftIdxs, s + c * 4, c * 4, hipMemcpyDeviceToDevice, fm->stream));
        VS_HIP(hipMemcpyAsync(fm->d_depth, s + c * 8, c * 4, hipMemcpyDeviceToDevice, fm->stream));
        VS_HIP(hipMemcpyAsync(fm->d_close, s + c * 12, c, hipMemcpyDeviceToDevice, fm->stream));
        VS_HIP(hipStreamSynchronize(fm->stream));
        VS_CHECK(st);
    }
    if (!rep->reloc.success) return VSLAM_OK;
    {
        const int C = fm->rlLast[3];
        std::vector<uint8_t> flags(std::max(C, 1), 0);
        VS_CHECK(fm->relocalize_debug(nullptr, 0, nullptr, 0, nullptr, 0, flags.data(), C, nullptr));
        int best = -1;
        VS_CHECK(loop_vote(pairs.data(), n, flags.data(), C, fn, &best));
        if (best < 0) return VSLAM_OK;
        rep->kf_loop = best;
    }
    rep->success = 1;
    T_corr = m4_rigid_inv(m4_from(T_cw));
    loop_drift(T_corr, camPoseInv, rep);
    return VSLAM_OK;
}

vslam_status vslam_system::close_loop(const vslam_loop_params* prm, vslam_loop_report* rep) {
    if (!rep) return VSLAM_ERR_INVALID;
    VS_CHECK(loop_check("vslam_system_close_loop"));
    vslam_loop_params P;
    vslam_reloc_params RP;
    if (!resolve_loop_params(prm, P)) { set_error("vslam_system_close_loop: negative or non-finite parameter"); return VSLAM_ERR_INVALID; }
    VS_CHECK(reloc_resolve_params(&P.reloc, RP));
    VS_CHECK(loop_check_close("vslam_system_close_loop"));
    *rep = vslam_loop_report{};
    rep->kf_loop = -1;
    if (loop_busy()) { rep->busy = 1; return VSLAM_OK; }
    M4 T_corr;
    VS_CHECK(loop_detect("vslam_system_close_loop", P, RP, rep, T_corr));
    if (!rep->success || P.detect_only) return VSLAM_OK;
    return loop_apply(rep->kf_loop, T_corr, P, rep);
}

// ---- loop closing of a stereo + IMU session (vslam_hip.h): the yaw-only correction ------------------
vslam_status vslam_system::loop_check_imu(const char* fn) const {
    if (monoMode) { set_error("%s: a mono session cannot close loops (stereo fixes the scale of the correction)", fn); return VSLAM_ERR_INVALID; }
    if (!cfg.use_imu) { set_error("%s: the session has no IMU (vslam_system_close_loop / _correct_loop serve it)", fn); return VSLAM_ERR_INVALID; }
    if (relocPending) { set_error("%s: a two-phase relocalisation is pending (the session has a pose but no velocity yet)", fn); return VSLAM_ERR_INVALID; }
    const double* g = cfg.gravity;
    const double n2 = g[0] * g[0] + g[1] * g[1] + g[2] * g[2];
    if (!std::isfinite(n2) || !(n2 > 0.0)) { set_error("%s: the session's gravity is zero or not finite", fn); return VSLAM_ERR_INVALID; }
    if (keyFrames.empty()) { set_error("%s: no tracked frame yet", fn); return VSLAM_ERR_INVALID; }
    return VSLAM_OK;
}

// the rotation angle of R (row-major 3x3), accurate at small angles too: atan2(|vee(R - R^T)| / 2, (tr R - 1) / 2)
static double rotation_angle(const double* R) {
    const double q[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
    return std::atan2(0.5 * std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]), 0.5 * (R[0] + R[4] + R[8] - 1.0));
}

// T' = [Exp(theta g) R_cam | t_corr] with theta the twist of D = T_corr * camPose^-1 about g = gravity / |gravity| (closed form)
M4 vslam_sys::loop_project_yaw(const M4& T_corr, const M4& camPose, const M4& camPoseInv, const double* gravity, vslam_loop_imu_report* irep) {
    const double nrm = std::sqrt(gravity[0] * gravity[0] + gravity[1] * gravity[1] + gravity[2] * gravity[2]);
    const double g[3] = {gravity[0] / nrm, gravity[1] / nrm, gravity[2] / nrm};
    const M4 D = m4_mul(T_corr, camPoseInv);
    const double R[9] = {D[0], D[1], D[2], D[4], D[5], D[6], D[8], D[9], D[10]};
    const double q[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
    double Rg[3];
    mat3_vec(R, g, Rg);
    const double theta = std::atan2(g[0] * q[0] + g[1] * q[1] + g[2] * q[2], (R[0] + R[4] + R[8]) - (g[0] * Rg[0] + g[1] * Rg[1] + g[2] * Rg[2]));
    const double w[3] = {theta * g[0], theta * g[1], theta * g[2]};
    double Ex[9];
    so3_expmap(w, Ex);
    M4 Tp = m4_identity();
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) Tp[4 * r + c] = Ex[3 * r] * camPose[c] + Ex[3 * r + 1] * camPose[4 + c] + Ex[3 * r + 2] * camPose[8 + c];
        Tp[4 * r + 3] = T_corr[4 * r + 3];
    }
    double E[9];                                           // R'^T R_corr: what the projection drops
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) E[3 * r + c] = Tp[r] * T_corr[c] + Tp[4 + r] * T_corr[4 + c] + Tp[8 + r] * T_corr[8 + c];
    irep->yaw = theta;
    irep->tilt_dropped = rotation_angle(E);
    memcpy(irep->T_wc_projected, Tp.data(), 16 * sizeof(double));
    return Tp;
}

// stage 1 (mapMutex held): a finished local BA is propagated (the projection needs the camera pose the graph will see), the claim
// is projected, then loop_build on the projected pose
vslam_status vslam_system::loop_build_imu(int kfLoop, const M4& T_corr, const vslam_loop_params& P, vslam_loop_report* rep,
                                          vslam_loop_imu_report* irep, LoopGraph& G) {
    if (LBADone) {
        VS_CHECK(change_poses_lca(endLBAIdx));
        LBADone = false;
    }
    const M4 Tp = loop_project_yaw(T_corr, camPose, camPoseInv, cfg.gravity, irep);
    G.camBefore = camPose;
    return loop_build(kfLoop, Tp, P, rep, G);
}

// between the solve and the move of the map points: a map point whose first observing keyframe came back with the same bytes
// is not touched
void vslam_sys::loop_hold_unmoved(vslam_system::LoopGraph& G) {
    G.nMoved = 0;
    for (int m = 0; m < G.nMp; m++) {
        const int r = G.ref[m];
        if (r < 0) continue;
        if (!memcmp(&G.poses[16 * (size_t)r], &G.fresh[16 * (size_t)r], 16 * sizeof(double))) G.ref[m] = -1;
        else G.nMoved++;
    }
}

// stage 3 (mapMutex held): loop_commit, then the world-frame IMU state follows the camera: dR = R_cam,new R_cam,old^T
void vslam_system::loop_commit_imu(const LoopGraph& G, vslam_loop_report* rep, vslam_loop_imu_report* irep) {
    loop_commit(G, rep);
    double dR[9];
    imu_follow_camera(G.camBefore, dR);
    for (int k = 0; k < 3; k++) irep->velocity[k] = velocity[k];
}

// (mapMutex held) velocity and predVelocity turned by dR = R_cam,new R_cam,old^T; dR [9] out
void vslam_system::imu_follow_camera(const M4& camBefore, double* dR) {
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++)
            dR[3 * r + c] = camPose[4 * r] * camBefore[4 * c] + camPose[4 * r + 1] * camBefore[4 * c + 1] + camPose[4 * r + 2] * camBefore[4 * c + 2];
    double v[3], pv[3];
    mat3_vec(dR, velocity, v);
    mat3_vec(dR, predVelocity, pv);
    for (int k = 0; k < 3; k++) { velocity[k] = v[k]; predVelocity[k] = pv[k]; }
}

vslam_status vslam_system::loop_apply_imu(int kfLoop, const M4& T_corr, const vslam_loop_params& P, vslam_loop_report* rep, vslam_loop_imu_report* irep) {
    VS_HIP(hipSetDevice(cfg.device));
    {
        std::lock_guard<std::mutex> lk(mapMutex);
        LoopGraph G;
        VS_CHECK(loop_build_imu(kfLoop, T_corr, P, rep, irep, G));
        VS_CHECK(vslam_pose_graph_optimize_yaw(G.poses.data(), G.fixed.data(), G.K, G.edges.data(), (int)G.edges.size(), cfg.gravity, &P.pgo, cfg.device,
                                               G.fresh.data(), &rep->pgo));
        loop_hold_unmoved(G);
        VS_CHECK(vslam_pose_graph_move_points(G.xyz.data(), G.ref.data(), G.poses.data(), G.fresh.data(), G.nMp, G.K, cfg.device, G.moved.data()));
        loop_commit_imu(G, rep, irep);
    }
    return loop_activate(rep);
}

void vslam_system::loop_imu_report_init(vslam_loop_imu_report* irep) const {
    *irep = vslam_loop_imu_report{};
    memcpy(irep->T_wc_projected, camPose.data(), 16 * sizeof(double));
    for (int k = 0; k < 3; k++) irep->velocity_before[k] = irep->velocity[k] = velocity[k];
}

vslam_status vslam_system::correct_loop_imu(int kfLoop, const double* T_wc_corrected, const vslam_loop_params* prm, vslam_loop_report* rep,
                                            vslam_loop_imu_report* irep) {
    static const char* const fn = "vslam_system_correct_loop_imu";
    if (!T_wc_corrected || !rep || !irep) return VSLAM_ERR_INVALID;
    VS_CHECK(loop_check_imu(fn));
    vslam_loop_params P;
    if (!resolve_loop_params(prm, P)) { set_error("%s: negative or non-finite parameter", fn); return VSLAM_ERR_INVALID; }
    VS_CHECK(loop_check_correct(fn, kfLoop, T_wc_corrected));
    *rep = vslam_loop_report{};
    rep->kf_loop = kfLoop;
    loop_imu_report_init(irep);
    if (loop_busy()) { rep->busy = 1; return VSLAM_OK; }
    rep->success = 1;
    const M4 T_corr = m4_from(T_wc_corrected);
    loop_drift(T_corr, camPoseInv, rep);
    return loop_apply_imu(kfLoop, T_corr, P, rep, irep);
}

vslam_status vslam_system::close_loop_imu(const vslam_loop_params* prm, vslam_loop_report* rep, vslam_loop_imu_report* irep) {
    static const char* const fn = "vslam_system_close_loop_imu";
    if (!rep || !irep) return VSLAM_ERR_INVALID;
    VS_CHECK(loop_check_imu(fn));
    vslam_loop_params P;
    vslam_reloc_params RP;
    if (!resolve_loop_params(prm, P)) { set_error("%s: negative or non-finite parameter", fn); return VSLAM_ERR_INVALID; }
    VS_CHECK(reloc_resolve_params(&P.reloc, RP));
    VS_CHECK(loop_check_close(fn));
    *rep = vslam_loop_report{};
    rep->kf_loop = -1;
    loop_imu_report_init(irep);
    if (loop_busy()) { rep->busy = 1; return VSLAM_OK; }
    M4 T_corr;
    VS_CHECK(loop_detect(fn, P, RP, rep, T_corr));
    if (!rep->success) return VSLAM_OK;
    if (P.detect_only) {                                   // (the projection of the claim under the camera pose as it is: nothing is propagated)
        loop_project_yaw(T_corr, camPose, camPoseInv, cfg.gravity, irep);
        return VSLAM_OK;
    }
    return loop_apply_imu(rep->kf_loop, T_corr, P, rep, irep);
}

// The duplicate map points of a revisited place (vslam_hip.h): B = the non-outlier map points created up to latestKF - min_kf_gap,
// A = those created since, vslam_fuse_search under the current camera, the commit of fuse_host.hpp.  In stages, shared with
// vslam_batch_fuse_loop: fuse_check (the refusals), fuse_sets (the two sets and their upload arrays), the search, fuse_commit.
// mapMutex is held by one holder from fuse_sets to fuse_commit: nothing may touch the map between them.
bool vslam_sys::resolve_fuse_loop_params(const char* fn, const vslam_fuse_loop_params* prm, vslam_fuse_loop_params& P) {
    P = prm ? *prm : vslam_fuse_loop_params{};
    const vslam_fuse_params& S = P.search;
    if (P.min_kf_gap < 0 || S.max_hamming < 0 || !(S.radius >= 0) || !(S.depth_ratio >= 0) || !std::isfinite(S.radius) || !std::isfinite(S.depth_ratio)) {
        set_error("%s: negative or non-finite parameter", fn); return false;
    }
    if (S.depth_ratio > 0 && S.depth_ratio < 1) { set_error("%s: depth_ratio %g lies inside (0, 1)", fn, (double)S.depth_ratio); return false; }
    if (P.min_kf_gap == 0) P.min_kf_gap = 20;
    return true;
}

// stage 1 (mapMutex held): a finished local BA is propagated, then the sets A and B, their positions and descriptors, the lane of the search
vslam_status vslam_system::fuse_sets(const vslam_fuse_loop_params& P, vslam_fuse_loop_report* rep, FuseSets& F) {
    if (LBADone) {                                         // a finished local BA is propagated first, as the next frame would
        VS_CHECK(change_poses_lca(endLBAIdx));
        LBADone = false;
    }
    std::vector<int>& idA = F.idA; std::vector<int>& idB = F.idB;
    idA.clear(); idB.clear();
    const long long newest = (long long)latestKF - P.min_kf_gap;
    for (int m = 0; m < (int)mapPoints.size(); m++) {
        if (mpOutlier[m]) continue;
        (mapPoints[m].kdx <= newest ? idB : idA).push_back(m);
    }
    if (idA.size() > 65536) idA.erase(idA.begin(), idA.end() - 65536);
    if (idB.size() > 65536) idB.erase(idB.begin(), idB.end() - 65536);
    const int nA = (int)idA.size(), nB = (int)idB.size();
    rep->n_a = nA; rep->n_b = nB;
    fusedPairs.clear();
    std::vector<double>& xyz = F.xyz; std::vector<uint8_t>& desc = F.desc;
    xyz.assign(3 * (size_t)(nA + nB) + 1, 0.0);
    desc.assign(32 * (size_t)(nA + nB) + 1, 0);
    auto fill = [&](const std::vector<int>& ids, size_t at) {
        for (size_t j = 0; j < ids.size(); j++) {
            const SysMP& mp = mapPoints[ids[j]];
            for (int c = 0; c < 3; c++) xyz[3 * (at + j) + c] = mp.wp[c];
            memcpy(&desc[32 * (at + j)], mp.desc, 32);
        }
    };
    fill(idA, 0); fill(idB, (size_t)nA);
    F.match.assign(std::max(nA, 1), -1); F.best.assign(4 * (size_t)std::max(nA, 1), 0);
    F.T_cw = camPoseInv;
    F.lane = vslam_fuse_lane{F.T_cw.data(), cfg.rig.fx, cfg.rig.fy, cfg.rig.cx, cfg.rig.cy, cfg.rig.width, cfg.rig.height,
                             xyz.data(), desc.data(), nA, xyz.data() + 3 * (size_t)nA, desc.data() + 32 * (size_t)nA, nB, F.match.data(), F.best.data()};
    return VSLAM_OK;
}

// stage 3 (mapMutex held): the search's matches into the map
void vslam_system::fuse_commit(const FuseSets& F, vslam_fuse_loop_report* rep) {
    const int nA = (int)F.idA.size();
    std::vector<std::pair<int, int>> pairs;                // ascending a: idA is in creation order
    for (int j = 0; j < nA; j++) if (F.match[j] >= 0) pairs.push_back({F.idA[j], F.idB[F.match[j]]});
    rep->n_active_after = (int)active.size();
    if (pairs.empty()) return;
    const vslam_fuse::CommitCounts c = vslam_fuse::merge_observations(pairs, mapPoints, keyFrames, mpOutlier, mpInFrame);
    for (int k : c.refresh) calc_connections(keyFrames[k]);
    vslam_fuse::merge_active(pairs, mapPoints.size(), active, mpInFrame);
    lastMatches.clear(); lastOutliers.clear();
    for (const auto& pr : pairs) { fusedPairs.push_back(pr.first); fusedPairs.push_back(pr.second); }
    rep->n_fused = c.nFused; rep->n_obs_moved = c.nMoved; rep->n_obs_dropped = c.nDropped;
    rep->n_keyframes_touched = (int)c.touched.size();
    rep->n_active_after = (int)active.size();
}

vslam_status vslam_system::fuse_loop(const vslam_fuse_loop_params* prm, vslam_fuse_loop_report* rep) {
    return fuse_loop_run("vslam_system_fuse_loop", false, prm, rep);
}

// stereo + IMU sessions: the same stages (fusion is geometry and bookkeeping; the IMU state is not touched)
vslam_status vslam_system::fuse_loop_imu(const vslam_fuse_loop_params* prm, vslam_fuse_loop_report* rep) {
    return fuse_loop_run("vslam_system_fuse_loop_imu", true, prm, rep);
}

vslam_status vslam_system::fuse_loop_run(const char* fn, bool imu, const vslam_fuse_loop_params* prm, vslam_fuse_loop_report* rep) {
    if (!rep) return VSLAM_ERR_INVALID;
    VS_CHECK(imu ? loop_check_imu(fn) : loop_check(fn));
    vslam_fuse_loop_params P;
    if (!resolve_fuse_loop_params(fn, prm, P)) return VSLAM_ERR_INVALID;
    *rep = vslam_fuse_loop_report{};
    if (loop_busy()) { rep->busy = 1; return VSLAM_OK; }
    VS_HIP(hipSetDevice(cfg.device));
    std::lock_guard<std::mutex> lk(mapMutex);
    FuseSets F;
    VS_CHECK(fuse_sets(P, rep, F));
    const vslam_fuse_lane& Q = F.lane;
    VS_CHECK(vslam_fuse_search(Q.T_cw, Q.fx, Q.fy, Q.cx, Q.cy, Q.w, Q.h, Q.a_xyz, Q.a_desc, Q.n_a, Q.b_xyz, Q.b_desc, Q.n_b,
                               &P.search, cfg.device, Q.match, Q.best, &rep->search));
    fuse_commit(F, rep);
    return VSLAM_OK;
}

// ---- vslam_system_global_ba (vslam_hip.h) ------------------------------------------------------
bool vslam_sys::resolve_system_gba_params(const char* fn, const vslam_system_gba_params* prm, vslam_system_gba_params& P) {
    P = prm ? *prm : vslam_system_gba_params{};
    if (P.gba.max_iterations < 0 || !(P.gba.lambda0 >= 0.0) || !std::isfinite(P.gba.lambda0) || !(P.edge_weight >= 0.0) || !std::isfinite(P.edge_weight)) {
        set_error("%s: negative or non-finite parameter", fn); return false;
    }
    return true;
}

vslam_status vslam_system::gba_check(const char* fn, const vslam_system_gba_params* prm, vslam_system_gba_params& P) const {
    VS_CHECK(loop_check(fn));
    return resolve_system_gba_params(fn, prm, P) ? VSLAM_OK : VSLAM_ERR_INVALID;
}

// A map point whose observation rays never open wider than this at the current values carries no factor: its depth is not
// observable, and a Levenberg-Marquardt pass walks it towards infinity.  0.9998 (1.15 degrees) is the usual triangulation bound.
// On the corridor walk after close_loop + fuse_loop it holds back 101 of 801 points with two or more factors, among them three
// at 500 - 700 m and one seen at the same pixel from the first keyframe and from the one that came back to it; without the
// guard those four move by 5e3 .. 3e10 m in twenty trials while the cost falls by 1e-3, with it no point moves by more than 0.53 m.
constexpr double GBA_MIN_PARALLAX_COS = 0.9998;

// steps 1 - 4 (mapMutex held): every keyframe, every map point that is not an outlier, ba_collect's pair flags, the sequential edges
vslam_status vslam_system::gba_flatten(double edgeWeight, GbaFlat& F) {
    if (LBADone) {                                         // a finished local BA is propagated first, as the next frame would
        VS_CHECK(change_poses_lca(endLBAIdx));
        LBADone = false;
    }
    const int K = (int)keyFrames.size();
    F.kfPose.resize((size_t)K * 16); F.kfId.resize(K); F.kfFixed.resize(K); F.kfLocal.assign(K, 1);
    for (int k = 0; k < K; k++) {
        const SysKF& kf = keyFrames[k];
        memcpy(&F.kfPose[16 * (size_t)k], kf.pose.data(), 16 * sizeof(double));
        F.kfId[k] = kf.numb; F.kfFixed[k] = (k == 0 || kf.fixed) ? 1 : 0;
    }
    std::vector<std::array<double, 3>> rays;
    F.allMps.clear(); F.pk.clear(); F.pl.clear(); F.pf.clear(); F.puv.clear(); F.poct.clear(); F.pobj.clear();
    for (int m = 0; m < (int)mapPoints.size(); m++) if (!mpOutlier[m]) F.allMps.push_back(m);
    const int Lm = (int)F.allMps.size();
    F.mpOut.assign(std::max(Lm, 1), 0);
    F.lm.resize((size_t)std::max(Lm, 1) * 3);
    for (int i = 0; i < Lm; i++) {
        const int m = F.allMps[i];
        const SysMP& mp = mapPoints[m];
        for (int c = 0; c < 3; c++) F.lm[3 * (size_t)i + c] = mp.wp[c];
        if (mp.kfm.empty() || (!mpInFrame[m] && (int)mp.kfm.size() < 3)) { F.mpOut[i] = 1; continue; }      // (no factor; an outlier at the commit)
        const size_t q0 = F.pk.size();
        for (const KfMatch& o : mp.kfm) {
            if (o.kf < 0 || o.kf >= K) continue;
            const SysKeys& keys = keyFrames[o.kf].keys;
            int flags;
            if (o.l >= 0) flags = (keys.close[o.l] && o.r >= 0) ? 3 : 1;
            else if (o.r >= 0) flags = 2;
            else continue;
            F.pk.push_back(o.kf); F.pl.push_back(i); F.pf.push_back((uint8_t)flags);
            F.puv.push_back(o.l >= 0 ? keys.kL[o.l].x : 0.f); F.puv.push_back(o.l >= 0 ? keys.kL[o.l].y : 0.f);
            F.puv.push_back(o.r >= 0 ? keys.kR[o.r].x : 0.f); F.puv.push_back(o.r >= 0 ? keys.kR[o.r].y : 0.f);
            F.poct.push_back(o.l >= 0 ? keys.kL[o.l].octave : 0); F.poct.push_back(o.r >= 0 ? keys.kR[o.r].octave : 0);
            F.pobj.push_back({o.kf, m, o.l, o.r});
        }
        // the parallax guard: unit rays from the observing camera centres (the right camera's for a right factor) to the point
        rays.clear();
        for (size_t q = q0; q < F.pk.size(); q++) {
            const M4& T = keyFrames[F.pk[q]].pose;
            for (int side = 0; side < 2; side++) {
                if (!((F.pf[q] >> side) & 1)) continue;
                const double b = side ? (double)cfg.rig.baseline : 0.0;
                const double d[3] = {mp.wp[0] - (T[3] + T[0] * b), mp.wp[1] - (T[7] + T[4] * b), mp.wp[2] - (T[11] + T[8] * b)};
                const double nrm = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
                rays.push_back({d[0] / nrm, d[1] / nrm, d[2] / nrm});
            }
        }
        double minCos = 1.0;
        for (size_t a = 0; a < rays.size(); a++)
            for (size_t c = 0; c < a; c++) minCos = std::min(minCos, rays[a][0] * rays[c][0] + rays[a][1] * rays[c][1] + rays[a][2] * rays[c][2]);
        if (rays.size() >= 2 && !(minCos <= GBA_MIN_PARALLAX_COS)) for (size_t q = q0; q < F.pk.size(); q++) F.pf[q] = 0;
    }
    F.edges.clear();
    if (edgeWeight > 0.0)
        for (int k = 0; k < K; k++) {
            const int p = keyFrames[k].prevKF;
            if (p < 0) continue;
            vslam_pgo_edge e{};
            e.i = p; e.j = k; e.w_rot = e.w_trans = edgeWeight;
            const M4 Z = m4_mul(keyFrames[p].poseInv, keyFrames[k].pose);
            memcpy(e.Z, Z.data(), 16 * sizeof(double));
            F.edges.push_back(e);
        }
    const int NP = (int)F.pk.size();
    vslam_ba_problem& P = F.P;
    P = vslam_ba_problem{};
    P.rig = cfg.rig; P.n_levels = nLev; P.sigma_factor = sigmaF.data(); P.inv_sigma_factor = invSigmaF.data();
    P.n_kf = K; P.kf_pose_wc = F.kfPose.data(); P.kf_id = F.kfId.data(); P.kf_fixed = F.kfFixed.data(); P.kf_local = F.kfLocal.data();
    P.n_lm = Lm; P.lm_xyz = F.lm.data(); P.n_pairs = NP; P.pair_kf = F.pk.data(); P.pair_lm = F.pl.data(); P.pair_flags = F.pf.data();
    P.pair_uv = F.puv.data(); P.pair_octave = F.poct.data();
    F.kfOut.assign((size_t)K * 16, 0.0); F.lmOut.assign((size_t)std::max(Lm, 1) * 3, 0.0); F.wrong.assign(std::max(NP, 1), 0);
    return VSLAM_OK;
}

// step 6 (mapMutex held): the write-back of ba_commit_a on the whole map; upd: the map points whose position was stored
void vslam_system::gba_commit(GbaFlat& F, vslam_system_gba_report* rep, std::vector<int>& upd) {
    const int K = (int)F.kfFixed.size(), Lm = (int)F.allMps.size(), NP = (int)F.pk.size();
    std::vector<int> nFac(std::max(Lm, 1), 0);
    for (int q = 0; q < NP; q++) nFac[F.pl[q]] += (F.pf[q] & 1) + ((F.pf[q] >> 1) & 1);
    int nWrong = 0, nOut = 0;
    for (int q = 0; q < NP; q++) {
        if (!F.wrong[q]) continue;
        nWrong++;
        SysKF& c = keyFrames[F.pobj[q].kf];
        SysMP& mp = mapPoints[F.pobj[q].mp];
        const int e = mp.find(F.pobj[q].kf);
        if (e < 0) continue;
        const int l = mp.kfm[e].l, r = mp.kfm[e].r;
        if (l >= 0) { c.lmpL[l] = -1; c.unF[l] = -1; }              // KeyFrame::eraseMPConnection
        if (r >= 0) { c.lmpR[r] = -1; c.unFR[r] = -1; }
        mp.kfm.erase(mp.kfm.begin() + e);                            // MapPoint::eraseKFConnection
    }
    for (int k = 0; k < K; k++) if (!F.kfFixed[k]) keyFrames[k].setPose(m4_from(&F.kfOut[16 * (size_t)k]));      // (an isolated keyframe's bytes are its own)
    upd.clear();
    for (int i = 0; i < Lm; i++) {
        const int m = F.allMps[i];
        SysMP& mp = mapPoints[m];
        if (F.mpOut[i] || (!mpInFrame[m] && (int)mp.kfm.size() < 3)) { mpOutlier[m] = 1; nOut++; }
        else if (nFac[i] >= 2) { for (int c = 0; c < 3; c++) mp.wp[c] = F.lmOut[3 * (size_t)i + c]; upd.push_back(m); }
    }
    rep->n_wrong = nWrong; rep->n_outliers = nOut;
}

// steps 6 and 7 up to the camera (mapMutex held): the commit, the refresh request of the moved points, every refPose, the camera
vslam_status vslam_system::gba_finish(GbaFlat& F, vslam_system_gba_report* rep) {
    std::vector<int> upd;
    gba_commit(F, rep, upd);
    VS_CHECK(ba_request_refresh(upd));
    for (int k = 0; k < (int)keyFrames.size(); k++) {
        const int p = keyFrames[k].prevKF;
        if (p >= 0) keyFrames[k].refPose = m4_mul(keyFrames[p].poseInv, keyFrames[k].pose);
    }
    lca_finish(latestKF);
    return VSLAM_OK;
}

// the end of step 7 (takes mapMutex itself): the active set under the new camera pose
vslam_status vslam_system::gba_activate(vslam_system_gba_report* rep) {
    vslam_loop_report lr{};
    VS_CHECK(loop_activate(&lr));
    rep->n_active_after = lr.n_active_after;
    rep->success = 1;
    return VSLAM_OK;
}

// The stages are shared with vslam_batch_global_ba: gba_check, gba_flatten, the solve, gba_finish, gba_activate.  mapMutex is held by
// one holder from gba_flatten to gba_finish.
vslam_status vslam_system::global_ba(const vslam_system_gba_params* prm, vslam_system_gba_report* rep) {
    static const char* const fn = "vslam_system_global_ba";
    if (!rep) return VSLAM_ERR_INVALID;
    vslam_system_gba_params P;
    VS_CHECK(gba_check(fn, prm, P));
    *rep = vslam_system_gba_report{};
    if (loop_busy()) { rep->busy = 1; return VSLAM_OK; }
    if (keyFrames.size() < 2) return VSLAM_OK;
    VS_HIP(hipSetDevice(cfg.device));
    {
        std::lock_guard<std::mutex> lk(mapMutex);
        GbaFlat F;
        VS_CHECK(gba_flatten(P.edge_weight, F));
        rep->n_keyframes = F.P.n_kf; rep->n_landmarks = F.P.n_lm; rep->n_pairs = F.P.n_pairs; rep->n_edges = (int)F.edges.size();
        vslam_gba_result R{};
        R.kf_pose_wc = F.kfOut.data(); R.lm_xyz = F.lmOut.data(); R.pair_wrong = F.wrong.data();
        VS_CHECK(vslam_global_ba(&F.P, F.edges.empty() ? nullptr : F.edges.data(), (int)F.edges.size(), &P.gba, cfg.device, &R));
        rep->gba = R.report;
        VS_CHECK(gba_finish(F, rep));
    }
    return gba_activate(rep);
}

// ---- vslam_system_global_ba_imu (vslam_hip.h): the stages above around the yaw-only solve -------
vslam_status vslam_system::gba_check_imu(const char* fn, const vslam_system_gba_params* prm, vslam_system_gba_params& P) const {
    VS_CHECK(loop_check_imu(fn));
    return resolve_system_gba_params(fn, prm, P) ? VSLAM_OK : VSLAM_ERR_INVALID;
}

vslam_status vslam_system::global_ba_imu(const vslam_system_gba_params* prm, vslam_system_gba_report* rep, vslam_gba_imu_report* irep) {
    static const char* const fn = "vslam_system_global_ba_imu";
    if (!rep || !irep) return VSLAM_ERR_INVALID;
    vslam_system_gba_params P;
    VS_CHECK(gba_check_imu(fn, prm, P));
    *rep = vslam_system_gba_report{};
    *irep = vslam_gba_imu_report{};
    for (int k = 0; k < 3; k++) irep->velocity_before[k] = irep->velocity[k] = velocity[k];
    memcpy(irep->T_wc, camPose.data(), 16 * sizeof(double));
    if (loop_busy()) { rep->busy = 1; return VSLAM_OK; }
    if (keyFrames.size() < 2) return VSLAM_OK;
    VS_HIP(hipSetDevice(cfg.device));
    {
        std::lock_guard<std::mutex> lk(mapMutex);
        if (LBADone) {                                  // the propagation gba_flatten would make, made here: the camera pose the
            VS_CHECK(change_poses_lca(endLBAIdx));         // adjustment starts from is taken after it, as loop_build_imu takes camBefore
            LBADone = false;
        }
        const M4 camBefore = camPose;
        GbaFlat F;
        VS_CHECK(gba_flatten(P.edge_weight, F));
        rep->n_keyframes = F.P.n_kf; rep->n_landmarks = F.P.n_lm; rep->n_pairs = F.P.n_pairs; rep->n_edges = (int)F.edges.size();
        vslam_gba_result R{};
        R.kf_pose_wc = F.kfOut.data(); R.lm_xyz = F.lmOut.data(); R.pair_wrong = F.wrong.data();
        VS_CHECK(vslam_global_ba_yaw(&F.P, F.edges.empty() ? nullptr : F.edges.data(), (int)F.edges.size(), cfg.gravity, &P.gba, cfg.device, &R));
        rep->gba = R.report;
        VS_CHECK(gba_finish(F, rep));
        double dR[9], Rg[3];                               // the world-frame IMU state follows the camera, as in loop_commit_imu
        imu_follow_camera(camBefore, dR);
        const double nrm = std::sqrt(cfg.gravity[0] * cfg.gravity[0] + cfg.gravity[1] * cfg.gravity[1] + cfg.gravity[2] * cfg.gravity[2]);
        const double g[3] = {cfg.gravity[0] / nrm, cfg.gravity[1] / nrm, cfg.gravity[2] / nrm};
        const double q[3] = {dR[7] - dR[5], dR[2] - dR[6], dR[3] - dR[1]};
        mat3_vec(dR, g, Rg);
        irep->yaw = std::atan2(g[0] * q[0] + g[1] * q[1] + g[2] * q[2], (dR[0] + dR[4] + dR[8]) - (g[0] * Rg[0] + g[1] * Rg[1] + g[2] * Rg[2]));
        for (int k = 0; k < 3; k++) irep->velocity[k] = velocity[k];
        memcpy(irep->T_wc, camPose.data(), 16 * sizeof(double));
    }
    return gba_activate(rep);
}

// the flattened problem a global-BA call would build now (the test tap of vslam_system_global_ba_problem / _problem_imu)
static vslam_status gba_problem_tap(const char* fn, bool imu, vslam_system* s, double edge_weight, int32_t arrays, int32_t* sizes, double* kf_pose_wc,
                                    uint8_t* kf_fixed, uint8_t* kf_local, double* lm_xyz, int32_t* lm_index, int32_t* pair_kf,
                                    int32_t* pair_lm, uint8_t* pair_flags, float* pair_uv, int32_t* pair_octave,
                                    vslam_pgo_edge* edges, float* sigma_factor, float* inv_sigma_factor);

extern "C" {

vslam_status vslam_system_global_ba(vslam_system* s, const vslam_system_gba_params* params, vslam_system_gba_report* report) {
    if (!s) return VSLAM_ERR_INVALID;
    return s->global_ba(params, report);
}

vslam_status vslam_system_global_ba_imu(vslam_system* s, const vslam_system_gba_params* params, vslam_system_gba_report* report,
                                        vslam_gba_imu_report* imu_report) {
    if (!s) return VSLAM_ERR_INVALID;
    return s->global_ba_imu(params, report, imu_report);
}

vslam_status vslam_system_fuse_loop_imu(vslam_system* s, const vslam_fuse_loop_params* params, vslam_fuse_loop_report* report) {
    if (!s) return VSLAM_ERR_INVALID;
    return s->fuse_loop_imu(params, report);
}

vslam_status vslam_system_global_ba_problem(vslam_system* s, double edge_weight, int32_t arrays, int32_t* sizes, double* kf_pose_wc,
                                            uint8_t* kf_fixed, uint8_t* kf_local, double* lm_xyz, int32_t* lm_index, int32_t* pair_kf,
                                            int32_t* pair_lm, uint8_t* pair_flags, float* pair_uv, int32_t* pair_octave,
                                            vslam_pgo_edge* edges, float* sigma_factor, float* inv_sigma_factor) {
    return gba_problem_tap("vslam_system_global_ba_problem", false, s, edge_weight, arrays, sizes, kf_pose_wc, kf_fixed, kf_local, lm_xyz, lm_index, pair_kf,
                           pair_lm, pair_flags, pair_uv, pair_octave, edges, sigma_factor, inv_sigma_factor);
}

vslam_status vslam_system_global_ba_problem_imu(vslam_system* s, double edge_weight, int32_t arrays, int32_t* sizes, double* kf_pose_wc,
                                                uint8_t* kf_fixed, uint8_t* kf_local, double* lm_xyz, int32_t* lm_index, int32_t* pair_kf,
                                                int32_t* pair_lm, uint8_t* pair_flags, float* pair_uv, int32_t* pair_octave,
                                                vslam_pgo_edge* edges, float* sigma_factor, float* inv_sigma_factor) {
    return gba_problem_tap("vslam_system_global_ba_problem_imu", true, s, edge_weight, arrays, sizes, kf_pose_wc, kf_fixed, kf_local, lm_xyz, lm_index, pair_kf,
                           pair_lm, pair_flags, pair_uv, pair_octave, edges, sigma_factor, inv_sigma_factor);
}

}  // extern "C"

static vslam_status gba_problem_tap(const char* fn, bool imu, vslam_system* s, double edge_weight, int32_t arrays, int32_t* sizes, double* kf_pose_wc,
                                    uint8_t* kf_fixed, uint8_t* kf_local, double* lm_xyz, int32_t* lm_index, int32_t* pair_kf,
                                    int32_t* pair_lm, uint8_t* pair_flags, float* pair_uv, int32_t* pair_octave,
                                    vslam_pgo_edge* edges, float* sigma_factor, float* inv_sigma_factor) {
    if (!s || !sizes) return VSLAM_ERR_INVALID;
    vslam_system_gba_params prm{};
    prm.edge_weight = edge_weight;
    vslam_system_gba_params P;
    VS_CHECK(imu ? s->gba_check_imu(fn, &prm, P) : s->gba_check(fn, &prm, P));
    if (s->loop_busy()) { set_error("%s: a mapping pass is in flight", fn); return VSLAM_ERR_INVALID; }
    VS_HIP(hipSetDevice(s->cfg.device));
    std::lock_guard<std::mutex> lk(s->mapMutex);
    vslam_system::GbaFlat F;
    VS_CHECK(s->gba_flatten(P.edge_weight, F));
    const int K = F.P.n_kf, Lm = F.P.n_lm, NP = F.P.n_pairs, M = (int)F.edges.size(), nLev = F.P.n_levels;
    sizes[0] = K; sizes[1] = Lm; sizes[2] = NP; sizes[3] = M; sizes[4] = nLev;
    if (!arrays) return VSLAM_OK;
    if (!kf_pose_wc || !kf_fixed || !kf_local || !lm_xyz || !lm_index || !pair_kf || !pair_lm || !pair_flags || !pair_uv || !pair_octave || !edges ||
        !sigma_factor || !inv_sigma_factor) { set_error("%s: NULL array", fn); return VSLAM_ERR_INVALID; }
    memcpy(kf_pose_wc, F.kfPose.data(), (size_t)K * 128); memcpy(kf_fixed, F.kfFixed.data(), K); memcpy(kf_local, F.kfLocal.data(), K);
    if (Lm) { memcpy(lm_xyz, F.lm.data(), (size_t)Lm * 24); memcpy(lm_index, F.allMps.data(), (size_t)Lm * 4); }
    if (NP) {
        memcpy(pair_kf, F.pk.data(), (size_t)NP * 4); memcpy(pair_lm, F.pl.data(), (size_t)NP * 4); memcpy(pair_flags, F.pf.data(), NP);
        memcpy(pair_uv, F.puv.data(), (size_t)NP * 16); memcpy(pair_octave, F.poct.data(), (size_t)NP * 8);
    }
    if (M) memcpy(edges, F.edges.data(), (size_t)M * sizeof(vslam_pgo_edge));
    memcpy(sigma_factor, s->sigmaF.data(), (size_t)nLev * 4); memcpy(inv_sigma_factor, s->invSigmaF.data(), (size_t)nLev * 4);
    return VSLAM_OK;
}

extern "C" {

vslam_status vslam_system_fuse_loop(vslam_system* s, const vslam_fuse_loop_params* params, vslam_fuse_loop_report* report) {
    if (!s) return VSLAM_ERR_INVALID;
    return s->fuse_loop(params, report);
}

vslam_status vslam_system_map_point_descriptors(vslam_system* s, int32_t cap, int32_t* n_out, uint8_t* desc) {
    if (!s || !n_out) return VSLAM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(s->mapMutex);
    const int n = (int)s->mapPoints.size();
    *n_out = n;
    if (n > cap) return VSLAM_ERR_CAPACITY;
    if (desc) for (int i = 0; i < n; i++) memcpy(desc + 32 * (size_t)i, s->mapPoints[i].desc, 32);
    return VSLAM_OK;
}

vslam_status vslam_system_map_point_observations(vslam_system* s, int32_t cap_points, int32_t cap_obs, int32_t* n_out, int32_t* n_obs_out,
                                                 int32_t* offsets, int32_t* triples) {
    if (!s || !n_out || !n_obs_out) return VSLAM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(s->mapMutex);
    const int n = (int)s->mapPoints.size();
    long long nObs = 0;
    for (const SysMP& mp : s->mapPoints) nObs += (long long)mp.kfm.size();
    *n_out = n; *n_obs_out = (int32_t)nObs;
    if (!offsets && !triples) return VSLAM_OK;
    if (n > cap_points || nObs > cap_obs || !offsets || !triples) return VSLAM_ERR_CAPACITY;
    int q = 0;
    for (int i = 0; i < n; i++) {
        offsets[i] = q;
        for (const KfMatch& o : s->mapPoints[i].kfm) { triples[3 * q] = o.kf; triples[3 * q + 1] = o.l; triples[3 * q + 2] = o.r; q++; }
    }
    offsets[n] = q;
    return VSLAM_OK;
}

vslam_status vslam_system_keyframe_points(vslam_system* s, int32_t kf, int32_t cap_l, int32_t cap_r, int32_t* n_l_out, int32_t* n_r_out,
                                          int32_t* lmp_l, int32_t* lmp_r) {
    if (!s || !n_l_out || !n_r_out) return VSLAM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(s->mapMutex);
    if (kf < 0 || kf >= (int)s->keyFrames.size()) { set_error("vslam_system_keyframe_points: keyframe %d of %d", kf, (int)s->keyFrames.size()); return VSLAM_ERR_INVALID; }
    const SysKF& K = s->keyFrames[kf];
    *n_l_out = (int)K.lmpL.size(); *n_r_out = (int)K.lmpR.size();
    if (!lmp_l && !lmp_r) return VSLAM_OK;
    if ((int)K.lmpL.size() > cap_l || (int)K.lmpR.size() > cap_r || !lmp_l || !lmp_r) return VSLAM_ERR_CAPACITY;
    std::copy(K.lmpL.begin(), K.lmpL.end(), lmp_l);
    std::copy(K.lmpR.begin(), K.lmpR.end(), lmp_r);
    return VSLAM_OK;
}

vslam_status vslam_system_fused_pairs(vslam_system* s, int32_t cap, int32_t* n_out, int32_t* pairs) {
    if (!s || !n_out) return VSLAM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(s->mapMutex);
    const int n = (int)s->fusedPairs.size() / 2;
    *n_out = n;
    if (n > cap) return VSLAM_ERR_CAPACITY;
    if (pairs) std::copy(s->fusedPairs.begin(), s->fusedPairs.end(), pairs);
    return VSLAM_OK;
}

vslam_status vslam_system_correct_loop(vslam_system* s, int32_t kf_loop, const double* T_wc_corrected, const vslam_loop_params* params,
                                       vslam_loop_report* report) {
    if (!s) return VSLAM_ERR_INVALID;
    const vslam_status st = s->correct_loop(kf_loop, T_wc_corrected, params, report);
    if (st == VSLAM_OK) memcpy(report->T_wc, s->camPose.data(), 16 * sizeof(double));
    return st;
}

vslam_status vslam_system_close_loop(vslam_system* s, const vslam_loop_params* params, vslam_loop_report* report) {
    if (!s) return VSLAM_ERR_INVALID;
    const vslam_status st = s->close_loop(params, report);
    if (st == VSLAM_OK) memcpy(report->T_wc, s->camPose.data(), 16 * sizeof(double));
    return st;
}

vslam_status vslam_system_correct_loop_imu(vslam_system* s, int32_t kf_loop, const double* T_wc_corrected, const vslam_loop_params* params,
                                           vslam_loop_report* report, vslam_loop_imu_report* imu_report) {
    if (!s) return VSLAM_ERR_INVALID;
    const vslam_status st = s->correct_loop_imu(kf_loop, T_wc_corrected, params, report, imu_report);
    if (st == VSLAM_OK) memcpy(report->T_wc, s->camPose.data(), 16 * sizeof(double));
    return st;
}

vslam_status vslam_system_close_loop_imu(vslam_system* s, const vslam_loop_params* params, vslam_loop_report* report,
                                         vslam_loop_imu_report* imu_report) {
    if (!s) return VSLAM_ERR_INVALID;
    const vslam_status st = s->close_loop_imu(params, report, imu_report);
    if (st == VSLAM_OK) memcpy(report->T_wc, s->camPose.data(), 16 * sizeof(double));
    return st;
}

vslam_status vslam_system_active_points(vslam_system* s, int32_t cap, int32_t* n_out, int32_t* index) {
    if (!s || !n_out) return VSLAM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(s->mapMutex);
    const int n = (int)s->active.size();
    *n_out = n;
    if (n > cap) return VSLAM_ERR_CAPACITY;
    if (index) for (int i = 0; i < n; i++) index[i] = s->active[i];
    return VSLAM_OK;
}

vslam_status vslam_system_covisibility(vslam_system* s, int32_t cap, int32_t* n_out, int32_t* triples) {
    if (!s || !n_out) return VSLAM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(s->mapMutex);
    int n = 0;
    for (const SysKF& kf : s->keyFrames) n += (int)kf.sortedKFWeights.size();
    *n_out = n;
    if (n > cap) return VSLAM_ERR_CAPACITY;
    if (!triples) return VSLAM_OK;
    int q = 0;
    for (const SysKF& kf : s->keyFrames)
        for (const auto& c : kf.sortedKFWeights) { triples[3 * q] = kf.numb; triples[3 * q + 1] = c.second; triples[3 * q + 2] = c.first; q++; }
    return VSLAM_OK;
}

vslam_status vslam_system_map_point_keyframes(vslam_system* s, int32_t cap, int32_t* n_out, int32_t* first_observer, int32_t* creator) {
    if (!s || !n_out) return VSLAM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(s->mapMutex);
    const int n = (int)s->mapPoints.size();
    *n_out = n;
    if (n > cap) return VSLAM_ERR_CAPACITY;
    for (int i = 0; i < n; i++) {
        if (first_observer) first_observer[i] = s->mapPoints[i].kfm.empty() ? -1 : s->mapPoints[i].kfm[0].kf;
        if (creator) creator[i] = (int32_t)s->mapPoints[i].kdx;
    }
    return VSLAM_OK;
}

}  // extern "C"
