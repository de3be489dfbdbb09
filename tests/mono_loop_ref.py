"""Test-side restatement of FeatureTracker::TrackImageMonoIMU (src/FeatureTracker.cpp:1280-1495) on index-based records,
built only from the CPU stage functions of pyoracle (Extractor.extract, imu_preintegrate / imu_predict, world_to_frame,
match_projection_mono, estimate_pose_mono, match_by_radius, mono_new_points, calc_descriptor) and the record types of
vo_system.  Test infrastructure only.

What it keeps of the reference, point by point:
  1. PredictNextPoseIMU (:1036-1106) runs first on every call, from the camera pose (which a refused call does not move),
     predVelocity and initialBias; it overwrites predNPose and advances predVelocity, also on calls the gate then refuses.
     predVelocity is never synchronised with the velocity the pose solve estimates (mVelocity).
  2. The movement gate (:1312, include/Conversions.h:112-137): until the map is initialised a call returns at once unless the
     translation between camera pose and prediction is >= 0.1f m AND the rotation is >= 5 degrees; tested before the frame-0
     branch.  The thresholds are float literals held in doubles: 0.1f = 0.100000001490116..., so a baseline of exactly 0.1
     (double) is refused.
  3. Bootstrap (:1315-1330): the first three accepted calls (and any call with frameNumb == 0) extract, updatePoses, and insert
     a keyframe at the IMU-predicted pose: initializeMono (:125-145, fixed) first, insertKeyFrameMono (:844-869) after.
     (The reference hands insertKeyFrameMono the MEMBER predNPose, which updatePoses has just overwritten with the constant-
     velocity extrapolation; this library places the keyframe at the IMU prediction, as initializeMono and the initialising call
     do - recorded in DESIGN.md section 6.)
  4. Initialisation (:1359-1377) on the fourth accepted call: insertKeyFrameMono at the prediction, actKeyF = every keyframe so
     far, the query side is the FIRST keyframe; matchByRadius(rad 120) into the others in list order on ONE claim table indexed
     by the target's key indices (length: max(current frame's keys, largest target), all -1); calculateMPFromMono +
     checkReprojError (po.mono_new_points, keyframe 0 = first keyframe) for points with >= 2 views; MapPoint::update(lastKF);
     addConnectionMono per surviving view; the pose is the prediction.
  5. Tracked calls (:1379-1494): removeOutOfFrameMPsMono, the rounds at rad 1200, poseEst, a keyframe on EVERY call (numOfMonoMPs
     stays 0), whose window (collected from sortedKFWeights, as getConnectedKFs does) is empty because its localMapPoints are all
     null when calcConnections runs - so no map point is created after initialisation; updatePoses, setActiveOutliers,
     mVelocity = mNewVelocity.
  6. No LocalMapper."""
import numpy as np
import pyoracle as po
from vo_system import affine_inv, rigid_inv, MapPoint, KeyFrame, System as _StereoSystem

F32 = np.float32
REFUSED, BOOTSTRAP, INITIALISED, TRACKED = 0, 1, 2, 3
BASELINE_THRESHOLD = float(F32(0.1))       # static constexpr double baselineThreshold {0.1f}
ANGLE_THRESHOLD = float(F32(5.0))          # static constexpr double angleThreshold {5.0f}


def gate_inputs(T1, T2):
    """(baseline [m], rotation angle [degrees]) of Converter::checkSufficientMovement"""
    d = T2[:3, 3] - T1[:3, 3]
    baseline = float(np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))
    tr = 0.0
    for i in range(3):
        tr += float(T1[0, i] * T2[0, i] + T1[1, i] * T2[1, i] + T1[2, i] * T2[2, i])
    c = min(1.0, max(-1.0, (tr - 1.0) / 2.0))
    return baseline, float(np.arccos(c) * (180.0 / np.pi))


def gate_accepts(baseline, angle_deg):
    if baseline < BASELINE_THRESHOLD:
        return False
    if angle_deg < ANGLE_THRESHOLD:
        return False
    return True


class MonoLoop:
    """FeatureTracker + Map of one mono + IMU session.  imu: dict(prm = po.imu_params(...), hz)."""

    def __init__(self, rig, nfeat, fps, T0=None, imu=None, window=10, velocity=None):
        self.rig, self.fps, self.imu, self.window = rig, float(fps), imu, window
        self.ex = po.Extractor(nfeat)
        self.scale, self.sigma, self.invSigma = self.ex.scalePyramid, self.ex.sigmaFactor, self.ex.InvSigmaFactor
        self.nLev = 8
        self.logScale = F32(np.log(np.float64(F32(1.2))))
        T0 = np.eye(4) if T0 is None else np.array(T0, np.float64)
        self.camPose = T0.copy(); self.camPoseInv = affine_inv(T0); self.camRefPose = np.eye(4)
        self.predNPose = T0.copy(); self.predNPoseInv = affine_inv(T0); self.predNPoseRef = np.eye(4)
        self.lastKFPoseInv = np.eye(4)
        self.latestKF = None
        self.keyFrames, self.allFrames, self.mapPoints, self.active = [], [], [], []
        self.monoInitialized = False; self.KFsUntilInitialized = 0
        self.predVelocity = np.zeros(3); self.bias = np.zeros(6)
        self.velocity = np.zeros(3) if velocity is None else np.array(velocity, np.float64)     # Camera::mVelocity at start
        self.log = []

    # ---- pieces ---------------------------------------------------------------------------------------------------------
    def _predict(self, S, dts):                       # PredictNextPoseIMU (:1036-1106)
        d = np.array(dts, np.float64).copy()
        if len(d) == 1:
            d[0] = self.imu["hz"] / self.fps            # dt's start value survives for a single-sample bucket only (:1067)
        pim = po.imu_preintegrate(self.imu["prm"], self.bias, S, d)
        sj = po.imu_predict(self.imu["prm"], pim, po.nav_state(self.camPose[:3, :3], self.camPose[:3, 3], self.predVelocity))
        T = np.eye(4); T[:3, :3] = sj[:9].reshape(3, 3); T[:3, 3] = sj[9:12]
        return T, sj[12:15].copy()

    def _update_poses(self, poseEst):                 # updatePoses (:1699-1708)
        prevWPoseInv = self.camPoseInv
        self.camRefPose = self.lastKFPoseInv @ poseEst
        self.camPose = poseEst.copy(); self.camPoseInv = affine_inv(poseEst)
        self.predNPoseRef = prevWPoseInv @ poseEst
        self.predNPose = poseEst @ self.predNPoseRef
        self.predNPoseInv = affine_inv(self.predNPose)

    def _insert_keyframe(self, kps, desc, pose, frameIdx, first):      # initializeMono / insertKeyFrameMono
        ref = None if first else self.latestKF.poseInv @ pose
        kf = KeyFrame(len(self.keyFrames), frameIdx, pose, ref)
        kf.keyF = True; kf.fixed = bool(first)
        kf.keys = dict(kpsL=kps.copy(), descL=desc.copy())
        kf.unMatchedF = np.full(len(kps), -1, np.int32); kf.localMapPoints = [None] * len(kps); kf.localMapPointsR = []
        if not first:
            kf.prevKF = self.latestKF; self.latestKF.nextKF = kf
            _StereoSystem.calc_connections(kf)          # localMapPoints all null: no connection
        self.keyFrames.append(kf); self.latestKF = kf
        self.lastKFPoseInv = affine_inv(pose)
        self.allFrames.append(kf)
        return kf

    def _window(self, lastKF):                        # actKeyF = {lastKF} + KeyFrame::getConnectedKFs (src/KeyFrame.cpp:87-101)
        act = [lastKF]
        for _, c in lastKF.sortedKFWeights:
            if c is not lastKF:
                act.append(c)
            if len(act) >= self.window:
                break
        return act

    def _mp_update(self, mp, kf):                     # MapPoint::update(KeyFrame*) (src/Map.cpp:58-100), left observation only
        mp.lastObsKF = kf
        d = mp.wp - kf.pose[:3, 3]
        dist = F32(np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))
        level = int(kf.keys["kpsL"]["octave"][mp.kFMatches[kf][0]])
        mp.maxScaleDist = F32(dist * self.scale[level])
        mp.minScaleDist = F32(mp.maxScaleDist / self.scale[self.nLev - 1])
        ds = [k.keys["descL"][l] for k, (l, _) in mp.kFMatches.items() if l != -1]      # calcDescriptor (:145-210)
        mp.desc = ds[po.calc_descriptor(np.stack(ds))].copy()

    def _add_mappoints(self, actKeyF, matchedL):      # addMappointsMono (:1497-1555) + addNewMapPoints (:1557-1578)
        lastKF = actKeyF[0]
        win = [lastKF] + [k for k in actKeyF if k.numb != lastKF.numb]
        nK = len(win)
        info = dict(new_points=0, radius_matches=0, per_target=[], table=None)
        if nK == 1:
            return info
        kL, dL = lastKF.keys["kpsL"], lastKF.keys["descL"]
        nP = len(kL)
        n_tab = max([len(matchedL)] + [len(k.keys["kpsL"]) for k in win[1:]])         # the claim-table length rule
        tab = np.full(n_tab, -1, np.int32); tab[:len(matchedL)] = matchedL
        views = [[(0, i)] for i in range(nP)]         # keyframeIdxMatchs
        for t, kf in enumerate(win[1:]):
            nt = len(kf.keys["kpsL"])
            n, sub, out = po.match_by_radius(self.ex, self.rig, kL, dL, kf.keys["kpsL"], kf.keys["descL"], tab[:nt], 120.0)
            tab[:nt] = sub
            info["radius_matches"] += int(n); info["per_target"].append(int(n))
            for i in np.nonzero(out >= 0)[0]:
                views[i].append((t + 1, int(out[i])))
        info["table"] = tab
        nV = np.array([len(v) for v in views], np.int32)
        vk = np.zeros((nP, nK), np.int32); vxy = np.zeros((nP, nK, 2), F32); vo = np.zeros((nP, nK), np.int32)
        for i, v in enumerate(views):
            for e, (s, j) in enumerate(v):
                kp = win[s].keys["kpsL"][j]
                vk[i, e] = s; vxy[i, e] = (kp["x"], kp["y"]); vo[i, e] = kp["octave"]
        if nP == 0:
            return info
        r = po.mono_new_points(self.rig, self.sigma, np.stack([k.pose for k in win]), [k.numb for k in win], nV, vk, vxy, vo)
        created = []
        for i in range(nP):
            if nV[i] < 2 or not r["accepted"][i]:     # minNumberOfKFsForMp, calculateMPFromMono
                continue
            mp = MapPoint(r["xyz"][i], dL[i], lastKF.numb, len(self.mapPoints))
            for e, (s, j) in enumerate(views[i]):
                if r["keep"][i, e]:                   # the views checkReprojError left in matchesOfPoint
                    mp.kFMatches[win[s]] = [j, -1]
            self._mp_update(mp, lastKF)
            for kf, (l, _) in mp.kFMatches.items():   # addConnectionMono
                kf.localMapPoints[l] = mp; kf.unMatchedF[l] = mp.kdx
            self.active.append(mp); self.mapPoints.append(mp)
            created.append(mp)
        info["new_points"] = len(created); info["created"] = created
        return info

    # ---- TrackImageMonoIMU ------------------------------------------------------------------------------------------------
    def track(self, image, frame_number, bucket):
        S, dts = bucket[0], bucket[1]
        rig = self.rig
        pred, pv = self._predict(S, dts)
        self.predNPose = pred; self.predNPoseInv = affine_inv(pred)
        self.predVelocity = pv
        baseline, angle = gate_inputs(self.camPose, pred)
        lg = dict(frame=frame_number, baseline=baseline, angle=angle, nActive=0, nIn=0, rounds=0, radius=0.0, iters=0,
                  matches=np.zeros((0, 2), np.int32), outliers=np.zeros(0, np.uint8), new_points=0, radius_matches=0, keyframe=False)

        def done(state):
            lg.update(state=state, pose=self.camPose.copy(), n_keyframes=len(self.keyFrames), n_map_points=len(self.mapPoints),
                      n_active_after=len(self.active))
            self.log.append(lg)
            return self.camPose.copy()

        if not self.monoInitialized and not gate_accepts(baseline, angle):
            return done(REFUSED)
        kL, dL = self.ex.extract(image)
        if frame_number == 0 or self.KFsUntilInitialized < 3:
            poseEst = pred.copy()
            self._update_poses(poseEst)
            self._insert_keyframe(kL, dL, poseEst, frame_number, self.KFsUntilInitialized == 0)
            self.KFsUntilInitialized += 1
            lg["keyframe"] = True
            return done(BOOTSTRAP)
        if not self.monoInitialized:
            poseEst = pred.copy()
            self._insert_keyframe(kL, dL, poseEst, frame_number, False)
            info = self._add_mappoints(list(self.allFrames), np.full(len(kL), -1, np.int32))
            self.monoInitialized = True
            self._update_poses(poseEst)
            lg.update(keyframe=True, new_points=info["new_points"], radius_matches=info["radius_matches"], init=info)
            return done(INITIALISED)
        # tracked call: removeOutOfFrameMPsMono under the prediction, the match / solve rounds at rad 1200
        predInv = rigid_inv(pred)
        cand = [mp for mp in self.active if not mp.isOutlier]
        if cand:
            xyz = np.stack([mp.wp for mp in cand]); msd = np.array([mp.maxScaleDist for mp in cand], F32)
            uL, vL, lL, visL = po.world_to_frame(rig, predInv, False, xyz, msd, self.logScale)
        else:
            xyz = np.zeros((0, 3)); uL = vL = np.zeros(0, F32); lL = np.zeros(0, np.int32); visL = np.zeros(0, np.uint8)
        for j, mp in enumerate(cand):
            mp.inFrame = bool(visL[j])
        keep = np.nonzero(visL)[0]
        act = [cand[j] for j in keep]
        self.active = list(act)
        M = len(act)
        mps = np.zeros(M, po.MPV_DTYPE)
        if M:
            mps["desc"] = np.stack([mp.desc for mp in act])
            mps["predLx"], mps["predLy"], mps["scaleLevelL"] = uL[keep], vL[keep], lL[keep]
        mps["inFrame"] = 1
        pts = xyz[keep] if M else np.zeros((0, 3))
        mL = np.full(len(kL), -1, np.int32); mt = np.full((M, 2), -1, np.int32)
        outl = np.zeros(M, np.uint8); mpo = np.zeros(M, np.uint8)
        rad, nIn, prevIn, prevrad, toBreak, rounds, iters = 1200.0, -1, -1, 1200.0, False, 0, 0
        while nIn < 50:
            rounds += 1
            _, mL, mt, _ = po.match_projection_mono(self.ex, rig, mps, kL, dL, mL, mt, rad)
            r = po.estimate_pose_mono(rig, self.invSigma, pts, mps["inFrame"], mpo, mt, outl, kL, self.imu["prm"], self.camPose,
                                      self.velocity, self.bias, S, dts)
            outl, nIn = r["outliers"], r["nIn"]
            iters += r["iterations"]
            if nIn < 50 and not toBreak:
                mL[:] = -1; mt[:] = -1; outl[:] = 0
                if nIn < prevIn:
                    rad = prevrad; toBreak = True
                else:
                    prevrad = rad; prevIn = nIn; rad += 30.0
            else:
                break
            if rounds > 3 and not toBreak:
                toBreak = True
        poseEst = rigid_inv(r["T_cw"])
        # the keyframe rule (:1471) is always true; the new keyframe's window holds only itself
        kf = self._insert_keyframe(kL, dL, poseEst, frame_number, False)
        info = self._add_mappoints(self._window(kf), mL)
        self._update_poses(poseEst)
        for i in range(M):                            # setActiveOutliers (:1016-1034)
            mp = act[i]
            if mt[i, 0] >= 0 and not outl[i]:
                mp.unMCnt = 0
            else:
                mp.unMCnt += 1
            if not outl[i] and mp.unMCnt < 20:
                continue
            mp.isOutlier = True
        self.velocity = r["vel"].copy(); self.bias = r["bias"].copy()
        lg.update(keyframe=True, nActive=M, nIn=int(nIn), rounds=rounds, radius=float(rad), iters=iters, matches=mt.copy(),
                  outliers=outl.copy(), new_points=info["new_points"], radius_matches=info["radius_matches"])
        return done(TRACKED)


# ---- the sequence every mono test runs ---------------------------------------------------------------------------------------
G = (0.0, 9.81, 0.0)
NOISE = (1.6968e-4, 1.9393e-5, 2.0e-3, 3.0e-3)     # gyro density, gyro walk, acc density, acc walk
NFEAT = 1500
_RUN = {}


def imu_config():
    import synth
    return dict(prm=po.imu_params(G, NOISE[0], NOISE[2], NOISE[1], NOISE[3], synth.T_BC1), hz=200)


def reference_run():
    """the restatement over synth.MONO_CALLS, computed once per process and left unchanged"""
    if "run" not in _RUN:
        import synth
        rig = synth.RIGS["euroc"]
        loop = MonoLoop(rig, NFEAT, synth.MONO_FPS, T0=synth.mono_arc_pose(0), imu=imu_config())
        for k, f in enumerate(synth.MONO_CALLS):
            S, dts, _ = synth.mono_bucket(k)
            loop.track(synth.mono_frame(f)[0], f, (S, dts))
        _RUN["run"] = loop
    return _RUN["run"]
