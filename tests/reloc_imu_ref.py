"""CPU restatement of the relocalisation of a stereo + IMU session (vslam_system_relocalize_imu,
vslam_batch_relocalize_imu): the velocity from TWO relocalised poses and the IMU bucket between them.  No reference counterpart.

The rule (reinit_velocity), on the oracle's pre-integration and prediction:
    pim  = imu_preintegrate(bucket, integration bias = biasGood)          dt = pim.deltaTij
    pred = imu_predict(pim, (R_prev, t_prev, v = 0))                      pred.R, pred.t, pred.v
    T_new = (R_cw^T, -R_cw^T t_cw)      with  t_new[i] = -((R_cw[0][i] t[0] + R_cw[1][i] t[1]) + R_cw[2][i] t[2])
    velocity_prev[i] = (t_new[i] - pred.t[i]) / dt
    velocity[i]      = pred.v[i] + velocity_prev[i]
    rot_residual     = sqrt(sum over (r, c) in row-major order of (pred.R[r][c] - R_new[r][c])^2)
The prediction is affine in the start velocity (t_j = t_i + R_i (dP + dt R_i^T v + ...), v_j = v_i + R_i dV), so velocity_prev is
exactly the v0 whose prediction lands on t_new, and velocity the v1 that v0 implies.

The session (Session wraps a vo_system.System): biasGood follows bias after every tracked frame with nIn >= 50; a call runs the
front end and reloc_ref.relocalize (mode 0) / reloc_p3p_ref.relocalize (mode 1) over the non-outlier map points; a success commits
the pose as vslam_system_relocalize does - with the identity predicted motion for the first pose (pending is set, velocity and bias
stay), with the predicted motion of updatePoses, velocity = the rule's, bias = biasGood for the second (pending is cleared); a
failure clears pending and changes nothing else."""
import numpy as np
import reloc_ref as rr
import vo_system


def reinit_velocity(oracle, prm, bias_good, samples, dts, T_wc_prev, T_cw_new):
    """dict(dt, velocity_prev, velocity, rot_residual, pred) from the bucket (samples (n, 6): acc, gyro; dts (n))"""
    T_wc_prev = np.asarray(T_wc_prev, np.float64); T = np.asarray(T_cw_new, np.float64)
    pim = oracle.imu_preintegrate(prm, np.asarray(bias_good, np.float64), samples, dts)
    pred = oracle.imu_predict(prm, pim, oracle.nav_state(T_wc_prev[:3, :3], T_wc_prev[:3, 3], np.zeros(3)))
    dt = float(pim[0])
    vp = np.zeros(3); v = np.zeros(3)
    for i in range(3):
        tn = -((T[0, i] * T[0, 3] + T[1, i] * T[1, 3]) + T[2, i] * T[2, 3])
        vp[i] = (tn - pred[9 + i]) / dt
        v[i] = pred[12 + i] + vp[i]
    s = 0.0
    for r in range(3):
        for c in range(3):
            d = pred[3 * r + c] - T[c, r]
            s = s + d * d
    return dict(dt=dt, velocity_prev=vp, velocity=v, rot_residual=float(np.sqrt(s)), pred=pred)


class Session:
    """a vo_system.System in IMU mode with the relocalisation state of item 23"""

    def __init__(self, oracle, rig, nfeat, prm, T0, velocity, local_mapping=True):
        self.po = oracle; self.rig = rig; self.prm = prm
        self.s = vo_system.System(rig, nfeat, T0=T0, imu=dict(prm=prm), local_mapping=local_mapping)
        self.s.velocity = np.array(velocity, np.float64)
        self.pending = 0
        self.bias_good = self.s.bias.copy()

    def track(self, L, R, n, bucket):
        assert not self.pending, "tracking is refused between the two poses"
        P = self.s.track(L, R, n, imu_bucket=bucket)
        if n > 0 and self.s.log[-1]["nIn"] >= 50:
            self.bias_good = self.s.bias.copy()
        return P

    def _land(self):
        """what the top of System.track does before the frame: a finished local BA's pose chain"""
        s = self.s
        assert s.pending is None          # (the synchronous schedule: nothing is in flight between frames)
        if s.LBADone:
            s.change_poses_lca(s.endLBAIdx)
            s.LBADone = False

    def relocalize(self, L, R, bucket=None, mode=0):
        """-> (T_wc, report fields of reloc_ref.relocalize, IMU report dict)"""
        s, po, rig = self.s, self.po, self.rig
        second = bool(self.pending)
        self._land()
        mps = [mp for mp in s.mapPoints if not mp.isOutlier]
        xyz = np.stack([mp.wp for mp in mps]); desc = np.stack([mp.desc for mp in mps])
        kL, dL = s.exL.extract(L); kR, dR = s.exR.extract(R)
        st = po.stereo_match(s.exL, s.exR, rig, kL, dL, kR, dR)
        if mode == 0:
            w = rr.relocalize(po, rig, s.invSigma, xyz, desc, kL, dL, kR, st)
        else:
            import reloc_p3p_ref as rp
            w = rp.relocalize(po, rig, s.invSigma, xyz, desc, kL, dL, kR, st, mode=1)
        irep = dict(phase=0, dt=0.0, velocity_prev=np.zeros(3), velocity=np.zeros(3), bias=np.zeros(6), rot_residual=0.0)
        if not w["success"]:
            self.pending = 0
            return s.camPose.copy(), w, irep
        T_cw = w["T_cw"]
        poseEst = vo_system.rigid_inv(T_cw)
        if second:
            S, dts = bucket
            v = reinit_velocity(po, self.prm, self.bias_good, S, dts, s.camPose, T_cw)
            irep.update(phase=2, dt=v["dt"], velocity_prev=v["velocity_prev"], velocity=v["velocity"], bias=self.bias_good.copy(),
                        rot_residual=v["rot_residual"])
        else:
            irep["phase"] = 1
        # the commit of vslam_system_relocalize: addFrame, the pose state, the active list from the in-frame test
        msd = np.array([mp.maxScaleDist for mp in mps], np.float32)
        _, _, _, vis = po.world_to_frame(rig, T_cw, False, xyz, msd, s.logScale)
        f = vo_system.KeyFrame(len(s.keyFrames), -1, poseEst, s.latestKF.poseInv @ poseEst)
        f.prevKF = s.latestKF
        s.allFrames.append(f)
        prevInv = s.camPoseInv
        s.camRefPose = s.lastKFPoseInv @ poseEst
        s.camPose = poseEst.copy(); s.camPoseInv = vo_system.affine_inv(poseEst)
        s.predNPoseRef = (prevInv @ poseEst) if second else np.eye(4)
        s.predNPose = poseEst @ s.predNPoseRef
        s.predNPoseInv = vo_system.affine_inv(s.predNPose)
        s.active = []
        for j, mp in enumerate(mps):
            mp.inFrame = bool(vis[j])
            if vis[j]:
                s.active.append(mp)
        if second:
            s.velocity = irep["velocity"].copy(); s.bias = self.bias_good.copy()
            self.pending = 0
        else:
            self.pending = 1
        return poseEst, w, irep
