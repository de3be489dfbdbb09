// Mono + IMU session behind the vslam_system handle: VSlamSystem::TrackMonoIMU -> FeatureTracker::TrackImageMonoIMU
// (src/System.cpp:82-85, src/FeatureTracker.cpp:1280-1495).  The numerical stages are the library's kernels (extraction,
// PredictNextPoseIMU's pre-integration, the mono tracking block, radius matching into resident key blocks, mono triangulation,
// descriptor selection); the KeyFrame / MapPoint bookkeeping is host C++ on the records of system.hpp.
//
// Reference behaviour kept as it is:
//   * PredictNextPoseIMU runs first on EVERY call and advances predVelocity, also on calls the movement gate then refuses; it
//     starts from the camera pose, which a refused call does not move;
//   * the gate (Converter::checkSufficientMovement) is tested before the frame-0 branch; its thresholds are float literals
//     held in doubles (0.1f, 5.0f);
//   * at initialisation the query side of addMappointsMono is the FIRST keyframe (actKeyF = allFramesPoses), and the three
//     matchByRadius calls share one claim table indexed by the TARGET's key indices;
//   * numOfMonoMPs is never written, so the keyframe rule is always true: every tracked call inserts a keyframe.  Its
//     calcConnections runs while its localMapPoints are all null, so its window holds only itself and no map point is created
//     after initialisation.  The window is still collected from sortedKFWeights; it is empty by construction.
// Choice made here: the claim table has max(current frame's keys, largest target) entries, all -1 (the reference sizes it by
// the current frame and reads / writes past its end for a larger target).
#include "system.hpp"
#include "track_dev.hpp"

using namespace vslam;
using namespace vslam_sys;

vslam_status vslam_system::init_mono(const vslam_system_config* c, double fps) {
    if (!c) return VSLAM_ERR_INVALID;
    if (c->use_imu != 1 || c->local_mapping != 0 || !(fps > 0)) {
        set_error("vslam_system_create_mono: use_imu must be 1, local_mapping 0 (no LocalMapper exists in this mode) and fps > 0");
        return VSLAM_ERR_INVALID;
    }
    cfg = *c;
    if (cfg.window <= 0) cfg.window = 10;
    if (cfg.window > 16) { set_error("vslam_system: window > 16 keyframes is not supported by the new-point pipeline"); return VSLAM_ERR_INVALID; }
    monoMode = true; monoFps = fps;
    VS_CHECK(vslam_extractor_create(&cfg.fe, cfg.rig.width, cfg.rig.height, 1, cfg.device, &fe));
    VS_CHECK(vslam_matcher_create(&cfg.rig, fe, 0, nullptr, 0, &fm));
    nLev = cfg.fe.n_levels;
    scalePyr.resize(nLev); sigmaF.resize(nLev); invSigmaF.resize(nLev);
    VS_CHECK(vslam_extractor_tables(fe, scalePyr.data(), nullptr, sigmaF.data(), invSigmaF.data(), nullptr, nullptr));
    bool zero = true;
    for (int i = 0; i < 16; i++) zero &= cfg.T_wc_init[i] == 0.0;
    const M4 T0 = zero ? m4_identity() : m4_from(cfg.T_wc_init);
    camPose = T0; camPoseInv = m4_affine_inv(T0); camRefPose = m4_identity();
    predNPose = T0; predNPoseInv = camPoseInv; predNPoseRef = m4_identity(); lastKFPoseInv = m4_identity();
    for (int k = 0; k < 3; k++) { velocity[k] = cfg.velocity_init[k]; predVelocity[k] = 0.0; }     // (predVelocity starts at zero: include/FeatureTracker.h)
    return VSLAM_OK;
}

vslam_status vslam_system::fetch_keys_mono(SysKeys& k) {
    int nL = 0, n = 0;
    VS_CHECK(vslam_extractor_count(fe, 0, &nL));
    k.kL.resize(nL); k.dL.resize((size_t)nL * 32); k.kR.clear(); k.dR.clear();
    if (nL) VS_CHECK(vslam_extractor_fetch(fe, 0, k.kL.data(), k.dL.data(), nL, &n));
    k.rightIdxs.assign(nL, -1); k.leftIdxs.clear(); k.depth.assign(nL, -1.f); k.close.assign(nL, 0);
    return VSLAM_OK;
}

void vslam_system::update_poses(const M4& poseEst) {
    const M4 prevWPoseInv = camPoseInv;
    camRefPose = m4_mul(lastKFPoseInv, poseEst);
    camPose = poseEst; camPoseInv = m4_affine_inv(poseEst);
    predNPoseRef = m4_mul(prevWPoseInv, poseEst);
    predNPose = m4_mul(poseEst, predNPoseRef);
    predNPoseInv = m4_affine_inv(predNPose);
}

void vslam_system::insert_keyframe_mono(SysKeys& keys, const M4& estimPose, int frame, bool first) {
    const M4 refPose = first ? m4_identity() : m4_mul(keyFrames[latestKF].poseInv, estimPose);
    keyFrames.emplace_back();
    SysKF& kf = keyFrames.back();
    const int numb = (int)keyFrames.size() - 1;
    kf.numb = numb; kf.frameIdx = frame; kf.refPose = refPose; kf.setPose(estimPose);
    kf.keys = std::move(keys);
    keys = SysKeys{};
    kf.unF.assign(kf.keys.kL.size(), -1); kf.lmpL.assign(kf.keys.kL.size(), -1);
    if (first) kf.fixed = true;
    else { kf.prevKF = latestKF; keyFrames[latestKF].nextKF = numb; calc_connections(kf); }      // (localMapPoints all null: no connection)
    latestKF = numb;
    lastKFPoseInv = m4_affine_inv(estimPose);
    allFrames.push_back({true, numb, -1, m4_identity()});
}

// addMappointsMono (:1497-1555) + addNewMapPoints (:1557-1578) for the window actKeyF (keyframe numbers, front = lastKF = the query)
vslam_status vslam_system::add_mappoints_mono(const std::vector<int>& actKeyF, std::vector<int>& matchedL, int* newPoints, int* radiusMatches) {
    *newPoints = 0; *radiusMatches = 0;
    const int last = actKeyF.front();
    std::vector<int> win;                          // the window without repetitions of lastKF (:1514), lastKF first
    win.push_back(last);
    for (int k : actKeyF) if (k != last) win.push_back(k);
    const int nK = (int)win.size(), nT = nK - 1;
    if (nT == 0) return VSLAM_OK;                  // a window of one: keyframeIdxMatchs[i].size() == 1 < minNumberOfKFsForMp everywhere
    if (nK > 16) { set_error("vslam_system: a mono window of %d keyframes exceeds the 16 of the triangulation kernel", nK); return VSLAM_ERR_CAPACITY; }
    const SysKeys& LK = keyFrames[last].keys;
    const int nP = (int)LK.kL.size();
    // key blocks: the keyframes' slots, or a block for this call where a keyframe has none
    std::vector<void*> tmp;
    auto freeTmp = [&]() { for (void* p : tmp) hipFree(p); tmp.clear(); };
    std::vector<const void*> blocks(nK, nullptr);
    std::vector<int> nKeys(nK);
    size_t tabLen = matchedL.size();
    for (int e = 0; e < nK; e++) {
        SysKF& kf = keyFrames[win[e]];
        nKeys[e] = (int)kf.keys.kL.size();
        if (e) tabLen = std::max(tabLen, (size_t)nKeys[e]);
        if (!kf.dkeys) {
            void* blk = nullptr;
            if (hipSetDevice(cfg.device) != hipSuccess || hipMalloc(&blk, vslam_kf_keys_bytes(nKeys[e], 0)) != hipSuccess) { freeTmp(); set_error("vslam_system: no device memory for a key block"); return VSLAM_ERR_HIP; }
            tmp.push_back(blk);
            vslam_kf_view v{};
            v.n_left = nKeys[e]; v.kps_l = kf.keys.kL.data(); v.desc_l = kf.keys.dL.data(); v.right_idxs = kf.keys.rightIdxs.data();
            const vslam_status st = vslam_kf_keys_upload(&v, cfg.device, blk);
            if (st != VSLAM_OK) { freeTmp(); return st; }
            blocks[e] = blk;
        } else blocks[e] = kf.dkeys;
    }
    matchedL.resize(tabLen, -1);                   // the claim-table rule (header comment)
    std::vector<int> mo((size_t)nT * std::max(nP, 1), -1), nm(nT, 0);
    vslam_status st = vslam_match_by_radius_window(fm, blocks[0], nP, blocks.data() + 1, nKeys.data() + 1, nT, 120.f, matchedL.data(), (int)matchedL.size(), mo.data(), nm.data());
    freeTmp();
    VS_CHECK(st);
    for (int t = 0; t < nT; t++) *radiusMatches += nm[t];
    if (nP == 0) return VSLAM_OK;
    // keyframeIdxMatchs -> the triangulation problem
    std::vector<int> nViews(nP, 1), viewKf((size_t)nP * nK, 0), viewOct((size_t)nP * nK, 0), viewIdx((size_t)nP * nK, -1);
    std::vector<float> viewXy((size_t)nP * nK * 2, 0.f);
    for (int i = 0; i < nP; i++) {
        auto put = [&](int e, int kfSlot, int idx) {
            const vslam_keypoint& kp = keyFrames[win[kfSlot]].keys.kL[idx];
            const size_t at = (size_t)i * nK + e;
            viewKf[at] = kfSlot; viewIdx[at] = idx; viewXy[2 * at] = kp.x; viewXy[2 * at + 1] = kp.y; viewOct[at] = kp.octave;
        };
        put(0, 0, i);
        for (int t = 0; t < nT; t++) { const int j = mo[(size_t)t * nP + i]; if (j >= 0) put(nViews[i]++, t + 1, j); }
    }
    std::vector<double> poses((size_t)nK * 16), xyz((size_t)nP * 3);
    std::vector<int> ids(nK), nObs(nP);
    std::vector<uint8_t> acc(nP), keep((size_t)nP * nK);
    for (int e = 0; e < nK; e++) { memcpy(&poses[16 * (size_t)e], keyFrames[win[e]].pose.data(), 16 * sizeof(double)); ids[e] = win[e]; }
    vslam_mono_points_problem P{};
    P.rig = cfg.rig; P.n_levels = nLev; P.sigma_factor = sigmaF.data(); P.n_kf = nK; P.kf_pose_wc = poses.data(); P.kf_id = ids.data();
    P.n_points = nP; P.n_views = nViews.data(); P.view_kf = viewKf.data(); P.view_xy = viewXy.data(); P.view_octave = viewOct.data();
    vslam_mono_points_result R{};
    R.accepted = acc.data(); R.xyz = xyz.data(); R.n_obs = nObs.data(); R.keep = keep.data();
    VS_CHECK(vslam_mono_new_points(&P, &R, cfg.device));
    // MapPoint::calcDescriptor of every point to be created, BEFORE the map is touched: nothing below this call can fail
    std::vector<int> make, start(1, 0), best;
    std::vector<uint8_t> descs;
    for (int i = 0; i < nP; i++) {
        if (nViews[i] < 2 || !acc[i]) continue;    // minNumberOfKFsForMp (:1526), calculateMPFromMono (:1529)
        make.push_back(i);
        for (int e = 0; e < nViews[i]; e++) {
            if (!keep[(size_t)i * nK + e]) continue;           // views checkReprojError left in matchesOfPoint
            const uint8_t* d = keyFrames[win[viewKf[(size_t)i * nK + e]]].keys.dL.data() + (size_t)viewIdx[(size_t)i * nK + e] * 32;
            descs.insert(descs.end(), d, d + 32);
        }
        start.push_back((int)(descs.size() / 32));
    }
    best.assign(std::max<size_t>(make.size(), 1), -1);
    if (!descs.empty()) VS_CHECK(vslam_calc_descriptors(descs.data(), start.data(), (int)make.size(), cfg.device, best.data()));
    std::vector<int> unused;
    for (size_t q = 0; q < make.size(); q++) {
        const int i = make[q];
        const int mi = new_map_point();
        SysMP& mp = mapPoints.back();
        for (int c = 0; c < 3; c++) mp.wp[c] = xyz[3 * (size_t)i + c];
        memcpy(mp.desc, LK.dL.data() + (size_t)i * 32, 32);
        mp.kdx = last; mp.idx = mi;
        for (int e = 0; e < nViews[i]; e++) {
            if (!keep[(size_t)i * nK + e]) continue;
            mp.kfm.push_back({win[viewKf[(size_t)i * nK + e]], viewIdx[(size_t)i * nK + e], -1});
        }
        mp_update(mp, last, unused, mi);           // MapPoint::update(lastKF); its calcDescriptor is `best`
        if (start[q + 1] > start[q] && best[q] >= 0) memcpy(mp.desc, descs.data() + (size_t)(start[q] + best[q]) * 32, 32);
        for (const KfMatch& o : mp.kfm) { SysKF& kf = keyFrames[o.kf]; kf.lmpL[o.l] = mi; kf.unF[o.l] = (int)mp.kdx; }      // addConnectionMono
        active.push_back(mi);
        (*newPoints)++;
    }
    return VSLAM_OK;
}

// the keys of a frame that is about to become a keyframe into the session's next key slot (not yet adopted: a failure later in
// the call leaves the slot free); *slot = null when a frame of this size fits no slot
vslam_status vslam_system::upload_keys_block(const SysKeys& keys, void** slot) {
    const int nL = (int)keys.kL.size();
    *slot = reserve_key_slot(nL, 0);
    if (!*slot) return VSLAM_OK;
    vslam_kf_view v{};
    v.n_left = nL; v.kps_l = keys.kL.data(); v.desc_l = keys.dL.data(); v.right_idxs = keys.rightIdxs.data();
    v.estimated_depth = keys.depth.data(); v.close_flags = keys.close.data();
    return vslam_kf_keys_upload(&v, cfg.device, *slot);
}

// takes the keyframe insert_keyframe_mono has just appended out again (a device step of the same call failed)
void vslam_system::undo_keyframe_mono(int prevLatest, const M4& prevLastKFPoseInv) {
    keyFrames.pop_back();
    allFrames.pop_back();
    latestKF = prevLatest;
    if (prevLatest >= 0) keyFrames[prevLatest].nextKF = -1;
    lastKFPoseInv = prevLastKFPoseInv;
}

// Converter::checkSufficientMovement (include/Conversions.h:112-137); the thresholds are `constexpr double x {0.1f}` / `{5.0f}`
static bool sufficient_movement(const M4& a, const M4& b) {
    const double dx = b[3] - a[3], dy = b[7] - a[7], dz = b[11] - a[11];
    const double baseline = std::sqrt(dx * dx + dy * dy + dz * dz);
    double tr = 0;                                 // trace(R1^T R2)
    for (int i = 0; i < 3; i++) { double s = 0; for (int k = 0; k < 3; k++) s += a[4 * k + i] * b[4 * k + i]; tr += s; }
    double c = (tr - 1.0) / 2.0;
    c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
    const double angle = std::acos(c) * (180.0 / M_PI);
    if (baseline < (double)0.1f) return false;
    if (angle < (double)5.0f) return false;
    return true;
}

vslam_status vslam_system::track_mono(const uint8_t* L, int stride, int channels, bool onDevice, int frame, const vslam_imu_bucket* imu,
                                      double* T_wc_out, vslam_mono_frame_report* rep) {
    if (!monoMode) { set_error("vslam_system_track_mono_imu: not a mono session (vslam_system_create_mono)"); return VSLAM_ERR_INVALID; }
    if (!L || !T_wc_out) return VSLAM_ERR_INVALID;
    if (!imu || imu->n <= 0 || !imu->acceleration || !imu->angular_velocity || !imu->timestamps_ns) {
        set_error("vslam_system_track_mono_imu: the call needs its IMU bucket (n >= 1)");
        return VSLAM_ERR_INVALID;
    }
    if ((channels != 1 && channels != 3 && channels != 4) || (long long)stride < (long long)cfg.rig.width * channels) {
        set_error("vslam_system_track_mono_imu: channels %d (1, 3 or 4), stride %d (at least width x channels)", channels, stride);
        return VSLAM_ERR_INVALID;
    }
    VS_HIP(hipSetDevice(cfg.device));
    SysFrameCtx& c = ctx;
    c.frame = frame; c.imu = imu;
    vslam_mono_frame_report out{};
    out.frame = frame;
    auto finish = [&]() {
        std::lock_guard<std::mutex> lk(mapMutex);
        out.n_keyframes = (int)keyFrames.size(); out.n_map_points = (int)mapPoints.size(); out.n_active_after = (int)active.size();
        memcpy(T_wc_out, camPose.data(), sizeof(double) * 16);
        if (rep) *rep = out;
    };
    // PredictNextPoseIMU (:1307, :1036-1106): from the camera pose, predVelocity and initialBias; dt starts at mHz / mFps
    frame_imu_input(c);
    double pred[16], pv[3];
    const double pv0[3] = {predVelocity[0], predVelocity[1], predVelocity[2]};
    if (!monoInitialized) {          // (a tracked call gets the same prediction from its tracking block: no wait of its own)
        VS_CHECK(fm->imu_predict(&c.in, pv0, (double)cfg.imu_hz / monoFps, pred, pv));
        predNPose = m4_from(pred); predNPoseInv = m4_affine_inv(predNPose);
        for (int k = 0; k < 3; k++) predVelocity[k] = pv[k];
        if (!sufficient_movement(camPose, predNPose)) {                          // :1312 - nothing is extracted
            lastMatches.clear(); lastOutliers.clear();
            out.state = 0;
            finish();
            return VSLAM_OK;
        }
    }
    // extractKeysNew (the colour conversions of :1292-1303 are the extractor's load)
    if (channels != 1) { const uint8_t* ptrs[1] = {L}; VS_CHECK(fe->set_images_color(ptrs, stride, channels, onDevice, true)); }
    else if (onDevice) VS_CHECK(vslam_extractor_set_image_device(fe, 0, L, stride));
    else VS_CHECK(vslam_extractor_set_image_host(fe, 0, L, stride));
    VS_CHECK(vslam_extractor_run(fe));
    if (frame == 0 || kfsUntilInitialized < 3) {                                 // bootstrap (:1315-1330)
        SysKeys keys;
        VS_CHECK(fetch_keys_mono(keys));
        void* slot = nullptr;
        VS_CHECK(upload_keys_block(keys, &slot));                                // a later initialisation reads it on the device
        {
            std::lock_guard<std::mutex> lk(mapMutex);
            const M4 poseEst = predNPose;                                        // poseEst = predNPose (:1321)
            update_poses(poseEst);
            insert_keyframe_mono(keys, poseEst, frame, kfsUntilInitialized == 0);
            if (slot) adopt_key_slot(keyFrames.back(), slot);
            kfsUntilInitialized++;
            lastMatches.clear(); lastOutliers.clear();
        }
        out.state = 1; out.keyframe_inserted = 1;
        finish();
        return VSLAM_OK;
    }
    if (!monoInitialized) {                                                      // initialisation (:1359-1377)
        SysKeys keys;
        VS_CHECK(fetch_keys_mono(keys));
        std::vector<int> matchedL(keys.kL.size(), -1);
        void* slot = nullptr;
        VS_CHECK(upload_keys_block(keys, &slot));
        {
            std::lock_guard<std::mutex> lk(mapMutex);
            const M4 poseEst = predNPose;
            const int prevLatest = latestKF; const M4 prevInv = lastKFPoseInv;
            insert_keyframe_mono(keys, poseEst, frame, false);
            if (slot) keyFrames.back().dkeys = slot;
            std::vector<int> actKeyF;                                            // actKeyF = map->allFramesPoses (:1367)
            for (const SysFrame& f : allFrames) if (f.isKF) actKeyF.push_back(f.kf);
            const vslam_status st = add_mappoints_mono(actKeyF, matchedL, &out.new_points, &out.radius_matches);
            if (st != VSLAM_OK) { undo_keyframe_mono(prevLatest, prevInv); return st; }      // (its device steps precede every map write)
            if (slot) keySlotsUsed++;                                            // the slot is taken now
            monoInitialized = true;
            update_poses(poseEst);
            lastMatches.clear(); lastOutliers.clear();
        }
        out.state = 2; out.keyframe_inserted = 1;
        finish();
        return VSLAM_OK;
    }
    // ---- tracked call (:1379-1494) --------------------------------------------------------------------------------------------
    const int N = frame_candidates(c);
    {
        const size_t need = (size_t)std::max(N, 1) * (24 + 32 + 4);
        if (need > upCap) { if (h_up) hipHostFree(h_up); upCap = need + need / 2; VS_HIP(hipHostMalloc((void**)&h_up, upCap, hipHostMallocDefault)); }
        double* xyz = (double*)h_up; uint8_t* desc = h_up + (size_t)N * 24; float* msd = (float*)(h_up + (size_t)N * 56);
        frame_fill_upload(c, xyz, desc, msd);
        VS_CHECK(fm->track_upload_map(xyz, desc, msd, N));
    }
    // PredictNextPoseIMU of a tracked call is the tracking block's own (same inputs: camera pose, predVelocity, initialBias)
    VS_CHECK(fm->track_frame_mono(&c.in, pv0, monoFps, c.T_cw, &c.tr, &c.imuOut, pred, pv));
    predNPose = m4_from(pred); predNPoseInv = m4_affine_inv(predNPose);
    for (int k = 0; k < 3; k++) predVelocity[k] = pv[k];
    const int M = c.tr.n_active;
    int nL = 0;
    VS_CHECK(vslam_extractor_count(fe, 0, &nL));
    {
        const size_t need = (size_t)std::max(M, 1) * 14 + (size_t)std::max(nL, 1) * 4 + (size_t)std::max(N, 1) + 64;
        if (need > dnCap) { if (h_dn) hipHostFree(h_dn); dnCap = need + need / 2; VS_HIP(hipHostMalloc((void**)&h_dn, dnCap, hipHostMallocDefault)); }
        VS_CHECK(fm->track_fetch_state(h_dn, M, nL, N));
    }
    const uint8_t* p = h_dn;
    const int* mt = (const int*)p; p += (size_t)M * 8;
    const int* actIdx = (const int*)p; p += (size_t)M * 4;
    std::vector<int> matchedL((const int*)p, (const int*)p + nL); p += (size_t)nL * 4;
    const uint8_t* outl = p; p += M;
    const uint8_t* inF = p; p += M;
    const uint8_t* visL = p;
    SysKeys keys;
    VS_CHECK(fetch_keys_mono(keys));
    const M4 poseEst = m4_rigid_inv(m4_from(c.T_cw));                            // (paired with the solve's own T_wc -> T_cw inversion)
    {
        std::lock_guard<std::mutex> lk(mapMutex);
        std::vector<int> act(M);
        for (int j = 0; j < N; j++) mpInFrame[c.cand[j]] = visL[j] != 0;       // removeOutOfFrameMPsMono (:941-967)
        for (int i = 0; i < M; i++) { act[i] = c.cand[actIdx[i]]; mpInFrame[act[i]] = inF[i] != 0; }
        const std::vector<int> prevActive = active;
        active = act;
        // keyframe rule (:1471): `numOfMonoMPs < minNStereo` holds always (numOfMonoMPs stays 0) - every tracked call inserts one.
        // It keeps its host keys only: nothing on the device reads the keys of a keyframe inserted after the initialisation.
        insertKeyFrameCount = 0;
        const int prevLatest = latestKF; const M4 prevInv = lastKFPoseInv;
        insert_keyframe_mono(keys, poseEst, frame, false);
        std::vector<int> actKeyF;
        mapping_window(actKeyF);                                                 // lastKF + getConnectedKFs: lastKF alone
        const vslam_status st = add_mappoints_mono(actKeyF, matchedL, &out.new_points, &out.radius_matches);
        if (st != VSLAM_OK) { undo_keyframe_mono(prevLatest, prevInv); active = prevActive; return st; }
        update_poses(poseEst);
        for (int i = 0; i < M; i++) {                                            // setActiveOutliers (:1016-1034)
            SysMP& mp = mapPoints[act[i]];
            if (mt[2 * i] >= 0 && !outl[i]) mp.unMCnt = 0; else mp.unMCnt++;
            if (!outl[i] && mp.unMCnt < 20) continue;
            mpOutlier[act[i]] = 1;
        }
        for (int k = 0; k < 3; k++) velocity[k] = c.imuOut.velocity[k];          // mVelocity = mNewVelocity (:1494)
        for (int k = 0; k < 6; k++) bias[k] = c.imuOut.bias[k];                  // initialBias as the last solve left it (:569)
        lastMatches.assign(mt, mt + (size_t)M * 2); lastOutliers.assign(outl, outl + M);
    }
    out.state = 3; out.keyframe_inserted = 1;
    out.n_active = M; out.n_inliers = c.tr.n_inliers; out.rounds = c.tr.rounds; out.lm_iterations = c.tr.lm_iterations; out.last_radius = c.tr.last_radius;
    finish();
    return VSLAM_OK;
}

extern "C" {

vslam_status vslam_system_create_mono(const vslam_system_config* config, double fps, vslam_system** out) {
    if (!out || !config) return VSLAM_ERR_INVALID;
    *out = nullptr;
    vslam_system* s = new (std::nothrow) vslam_system();
    if (!s) return VSLAM_ERR_INVALID;
    const vslam_status st = s->init_mono(config, fps);
    if (st != VSLAM_OK) { s->release(); delete s; return st; }
    *out = s;
    return VSLAM_OK;
}

vslam_status vslam_system_track_mono_imu(vslam_system* s, const uint8_t* left, int32_t stride, int32_t channels, int32_t on_device,
                                         int32_t frame_number, const vslam_imu_bucket* imu, double* T_wc_out, vslam_mono_frame_report* report) {
    if (!s) return VSLAM_ERR_INVALID;
    return s->track_mono(left, stride, channels, on_device != 0, frame_number, imu, T_wc_out, report);
}

vslam_status vslam_system_memory(vslam_system* s, int32_t* key_slots_used, int64_t* key_slab_bytes) {
    if (!s) return VSLAM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(s->mapMutex);
    if (key_slots_used) *key_slots_used = s->key_slots_total();
    if (key_slab_bytes) *key_slab_bytes = (int64_t)(s->keySlabs.size() * s->keySlot * (size_t)s->keySlotsPerSlab);
    return VSLAM_OK;
}

vslam_status vslam_system_map_points(vslam_system* s, int32_t cap, int32_t* n_out, double* xyz, uint8_t* is_outlier) {
    if (!s || !n_out) return VSLAM_ERR_INVALID;
    std::lock_guard<std::mutex> lk(s->mapMutex);
    const int n = (int)s->mapPoints.size();
    *n_out = n;
    if (n > cap) return VSLAM_ERR_CAPACITY;
    for (int i = 0; i < n; i++) {
        if (xyz) for (int c = 0; c < 3; c++) xyz[3 * (size_t)i + c] = s->mapPoints[i].wp[c];
        if (is_outlier) is_outlier[i] = s->mpOutlier[i];
    }
    return VSLAM_OK;
}

}  // extern "C"
