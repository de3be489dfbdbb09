"""GPU parity of the device-resident per-frame tracking loop (initializeMap -> removeOutOfFrameMPs ->
{match, pose LM} retry loop -> PredictMPsPosition -> refine) against the same sequence composed from
the CPU oracle's stage functions."""
import numpy as np
import pytest
import synth

pytestmark = pytest.mark.gpu


def rigid_inv(T):
    Ti = np.eye(4)
    Rt = T[:3, :3].T.copy()
    Ti[:3, :3] = Rt
    for i in range(3):
        Ti[i, 3] = -(Rt[i, 0] * T[0, 3] + Rt[i, 1] * T[1, 3] + Rt[i, 2] * T[2, 3])
    return Ti


def oracle_init_map(rig, ex, kL, dL, st, T_wc):
    idx = np.nonzero(st["depth"] > 0)[0]
    xyz = np.zeros((len(idx), 3)); msd = np.zeros(len(idx), np.float32)
    R, t = T_wc[:3, :3], T_wc[:3, 3]
    for j, i in enumerate(idx):
        zp = float(st["depth"][i]); xp = (float(kL["x"][i]) - rig["cx"]) * zp / rig["fx"]; yp = (float(kL["y"][i]) - rig["cy"]) * zp / rig["fy"]
        pw = [(R[c, 0] * xp + R[c, 1] * yp + R[c, 2] * zp) + t[c] for c in range(3)]
        xyz[j] = pw
        d = [pw[c] - t[c] for c in range(3)]
        dist = np.float32(np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))
        msd[j] = np.float32(dist * ex.scalePyramid[kL["octave"][i]])
    return xyz, dL[idx].copy(), msd


def oracle_track(oracle, rig, ex, keys, st, mp, T_wc_pred, frame_number, imu=None, outlier=None):
    """outlier: MapPoint::isOutlier per map point (removeOutOfFrameMPs drops those before the visibility test)"""
    kL, dL, kR, dR = keys
    xyz, desc, msd = mp
    log_scale = np.float32(np.log(np.float64(np.float32(1.2))))
    T_cw = rigid_inv(T_wc_pred)
    uL, vL, lL, visL = oracle.world_to_frame(rig, T_cw, False, xyz, msd, log_scale)
    uR, vR, lR, visR = oracle.world_to_frame(rig, T_cw, True, xyz, msd, log_scale)
    keep = visL & visR
    if outlier is not None:
        keep = keep & ~np.asarray(outlier, bool)
    act = np.nonzero(keep)[0]
    M = len(act)
    mps = np.zeros(M, oracle.MPV_DTYPE)
    mps["desc"] = desc[act]
    mps["predLx"], mps["predLy"], mps["predRx"], mps["predRy"] = uL[act], vL[act], uR[act], vR[act]
    mps["scaleLevelL"], mps["scaleLevelR"] = lL[act], lR[act]
    mps["inFrame"] = 1; mps["inFrameR"] = 1
    pts = xyz[act]
    mL = np.full(len(kL), -1, np.int32); mR = np.full(len(kR), -1, np.int32)
    mt = np.full((M, 2), -1, np.int32); outl = np.zeros(M, np.uint8)
    mpo = np.zeros(M, np.uint8)
    state = dict(st)
    est = T_cw.copy()
    rad = 120.0 if frame_number == 1 else 10.0
    nIn, prevIn, prevrad, toBreak, rounds, iters = -1, -1, rad, False, 0, 0

    imu_state = list(imu) if imu is not None else None

    def solve(est, mt, outl, state):
        if imu is not None:     # IMU branch: the initial pose comes from the IMU prediction, `est` is ignored
            r = oracle.estimate_pose_imu(rig, ex.InvSigmaFactor, pts, mps["inFrame"], mps["inFrameR"], mpo, mt, outl, kL, kR,
                                         state["rightIdxs"], state["leftIdxs"], state["depth"], state["close"], *imu_state)
            imu_state[3] = r["bias"].copy()   # initialBias = b1 after every solve (src/FeatureTracker.cpp:405)
        else:
            r = oracle.estimate_pose(rig, ex.InvSigmaFactor, pts, mps["inFrame"], mps["inFrameR"], mpo, mt, outl, kL, kR,
                                     state["rightIdxs"], state["leftIdxs"], state["depth"], state["close"], est)
        for k in ("rightIdxs", "leftIdxs", "depth", "close"):
            state[k] = r[k]
        return r

    while nIn < 50:
        rounds += 1
        _, mL, mR, mt, _ = oracle.match_projection(ex, rig, mps, kL, dL, kR, dR, state["rightIdxs"], state["leftIdxs"], mL, mR, mt, rad)
        r = solve(est, mt, outl, state)
        est, mt, outl, nIn = r["T_cw"], r["matches"], r["outliers"], r["nIn"]
        iters += r["iterations"]
        if nIn < 50 and not toBreak:
            est = T_cw.copy(); mL[:] = -1; mR[:] = -1; mt[:] = -1; outl[:] = 0
            if nIn < prevIn:
                rad = prevrad; toBreak = True
            else:
                prevrad = rad; prevIn = nIn; rad += 30.0
        else:
            break
        if rounds > 3 and not toBreak:
            toBreak = True
    # PredictMPsPosition
    uL, vL, lL, visL = oracle.world_to_frame(rig, est, False, pts, msd[act], log_scale)
    uR, vR, lR, visR = oracle.world_to_frame(rig, est, True, pts, msd[act], log_scale)
    for i in range(M):
        mps["inFrame"][i] = visL[i]; mps["inFrameR"][i] = visR[i]
        if visL[i]:
            mps["predLx"][i], mps["predLy"][i], mps["scaleLevelL"][i] = uL[i], vL[i], lL[i]
        elif mt[i, 0] >= 0:
            mL[mt[i, 0]] = -1; mt[i, 0] = -1
        if visR[i]:
            mps["predRx"][i], mps["predRy"][i], mps["scaleLevelR"][i] = uR[i], vR[i], lR[i]
        elif mt[i, 1] >= 0:
            mR[mt[i, 1]] = -1; mt[i, 1] = -1
        if outl[i]:
            outl[i] = 0
            if mt[i, 0] >= 0:
                mL[mt[i, 0]] = -1; mt[i, 0] = -1
            if mt[i, 1] >= 0:
                mR[mt[i, 1]] = -1; mt[i, 1] = -1
    _, mL, mR, mt, _ = oracle.match_projection(ex, rig, mps, kL, dL, kR, dR, state["rightIdxs"], state["leftIdxs"], mL, mR, mt, 4.0)
    r = solve(est, mt, outl, state)
    return dict(T_cw=r["T_cw"], nIn=r["nIn"], nStereo=r["nStereo"], matches=r["matches"], outliers=r["outliers"],
                act=act, rounds=rounds, last_radius=rad, iters=iters + r["iterations"], state=state, vel=r.get("vel"), bias=r.get("bias"))


@pytest.mark.parametrize("f0,f1,frame_number", [(4, 5, 7), (8, 10, 1), (2, 3, 3)])
def test_track_frame_parity(oracle, capi, f0, f1, frame_number):
    _track_frame_parity(oracle, capi, f0, f1, frame_number)


def _track_frame_parity(oracle, capi, f0, f1, frame_number, rig_name="euroc", nfeat=1500, min_active=150):
    rig = synth.RIGS[rig_name]
    La, Ra, Ta = synth.stereo_frame(f0, rig_name)
    Lb, Rb, Tb = synth.stereo_frame(f1, rig_name)
    oL, oR = oracle.Extractor(nfeat), oracle.Extractor(nfeat)
    ge = capi.Extractor(rig["w"], rig["h"], nfeat, batch=2)
    m = capi.Matcher(rig, ge, 0, ge, 1)
    # frame a: map initialisation
    kL, dL = oL.extract(La); kR, dR = oR.extract(Ra)
    st = oracle.stereo_match(oL, oR, rig, kL, dL, kR, dR)
    mp = oracle_init_map(rig, oL, kL, dL, st, Ta)
    ge.extract([La, Ra]); m.stereo_match(); capi.tracker_init_map(m, Ta)
    # frame b: track with a constant-velocity style prediction (ground truth of an intermediate time)
    pred = synth.pose_at(f1 - 0.3, rig["fps"])
    kL, dL = oL.extract(Lb); kR, dR = oR.extract(Rb)
    st = oracle.stereo_match(oL, oR, rig, kL, dL, kR, dR)
    ref = oracle_track(oracle, rig, oL, (kL, dL, kR, dR), st, mp, pred, frame_number)
    ge.extract([Lb, Rb]); m.stereo_match()
    T_cw, rep = capi.tracker_track(m, pred, frame_number)
    mt, outl, act = capi.tracker_fetch(m)
    assert rep["n_map_points"] == len(mp[0]) and rep["n_active"] == len(ref["act"]) and rep["n_active"] > min_active
    assert np.array_equal(act, ref["act"])
    assert rep["rounds"] == ref["rounds"] and rep["lm_iterations"] == ref["iters"]
    assert (rep["n_inliers"], rep["n_stereo"]) == (ref["nIn"], ref["nStereo"])
    assert np.abs(T_cw - ref["T_cw"]).max() < 1e-9
    assert np.array_equal(mt, ref["matches"]) and np.array_equal(outl, ref["outliers"])
    st2 = m.stereo_fetch(len(kL), len(kR))
    assert np.array_equal(st2["rightIdxs"], ref["state"]["rightIdxs"]) and np.array_equal(st2["close"], ref["state"]["close"])
    # tracking recovers the true pose of frame b
    assert np.abs(rigid_inv(T_cw) - Tb).max() < 0.05
    assert rep["n_inliers"] >= 50
    return ge, rep


def test_track_frame_imu_parity(oracle, capi):
    """Stereo + IMU mode (C2): the same loop with the IMU branch of the pose solve."""
    rig = synth.RIGS["euroc"]
    f0, f1 = 9, 10
    La, Ra, Ta = synth.stereo_frame(f0)
    Lb, Rb, Tb = synth.stereo_frame(f1)
    oL, oR = oracle.Extractor(1500), oracle.Extractor(1500)
    ge = capi.Extractor(rig["w"], rig["h"], 1500, batch=2)
    m = capi.Matcher(rig, ge, 0, ge, 1)
    kL, dL = oL.extract(La); kR, dR = oR.extract(Ra)
    st = oracle.stereo_match(oL, oR, rig, kL, dL, kR, dR)
    mp = oracle_init_map(rig, oL, kL, dL, st, Ta)
    ge.extract([La, Ra]); m.stereo_match(); capi.tracker_init_map(m, Ta)
    G = (0.0, 9.81, 0.0); NOISE = (1.6968e-4, 1.9393e-5, 2.0e-3, 3.0e-3)
    h = 1e-4
    v_prev = (synth.pose_at(f0 + h * 20)[:3, 3] - synth.pose_at(f0 - h * 20)[:3, 3]) / (2 * h)
    S, dts, _ = synth.imu_samples(f0, f1, noise_seed=5)
    ts = np.arange(len(dts)) * 5e6
    prm = oracle.imu_params(G, NOISE[0], NOISE[2], NOISE[1], NOISE[3], synth.T_BC1)
    pred = synth.pose_at(f1 - 0.3)
    kL, dL = oL.extract(Lb); kR, dR = oR.extract(Rb)
    st = oracle.stereo_match(oL, oR, rig, kL, dL, kR, dR)
    ref = oracle_track(oracle, rig, oL, (kL, dL, kR, dR), st, mp, pred, 5, imu=(prm, Ta, v_prev, np.zeros(6), S, dts))
    ge.extract([Lb, Rb]); m.stereo_match()
    T_cw, rep, vel, bias = capi.tracker_track_imu(m, pred, 5, G, NOISE, synth.T_BC1, Ta, v_prev, np.zeros(6), S[:, :3], S[:, 3:], ts, 200)
    mt, outl, act = capi.tracker_fetch(m)
    assert rep["rounds"] == ref["rounds"] and rep["lm_iterations"] == ref["iters"]
    assert (rep["n_inliers"], rep["n_stereo"]) == (ref["nIn"], ref["nStereo"]) and rep["n_inliers"] >= 50
    assert np.abs(T_cw - ref["T_cw"]).max() < 1e-8
    assert np.abs(vel - ref["vel"]).max() < 1e-8 and np.abs(bias - ref["bias"]).max() < 1e-9
    assert np.array_equal(mt, ref["matches"]) and np.array_equal(outl, ref["outliers"])
    assert np.abs(rigid_inv(T_cw) - Tb).max() < 0.05


def test_pipelined_two_extractor_pairs_match_serial(capi):
    """Frame-level pipelining: extraction of frame n+1 on its own thread / extractor pair while
    frame n is matched and tracked, ordered only by HIP events (no host sync in run / stereo_match / init_map).
    Every per-frame result must be bit-identical to the serial single-extractor run."""
    import threading, queue
    rig = synth.RIGS["euroc"]
    w, h = rig["w"], rig["h"]
    frames = [synth.stereo_frame(f) for f in range(3, 9)]
    preds = [synth.pose_at(f - 0.3) for f in range(3, 9)]
    NREP = 3                                           # replay the sequence a few times to give races a chance

    def track(m, fe, i):
        m.stereo_match()
        out = None
        if i > 0:
            T, rep = capi.tracker_track(m, preds[i], 5)
            mt, outl, act = capi.tracker_fetch(m)
            out = (T.copy(), rep["n_inliers"], rep["n_stereo"], rep["lm_iterations"], mt.copy(), outl.copy(), dict(rep, keys=(len(fe.fetch(0)[0]), len(fe.fetch(1)[0]))))
        capi.tracker_init_map(m, frames[i][2])
        return out

    # serial reference
    fe = capi.Extractor(w, h, 1500, batch=2)
    m = capi.Matcher(rig, fe, 0, fe, 1)
    ref = []
    for n in range(NREP * len(frames)):
        i = n % len(frames)
        fe.set_image(0, frames[i][0]); fe.set_image(1, frames[i][1])
        fe.run()
        ref.append(track(m, fe, i))
    # pipelined
    fes = [capi.Extractor(w, h, 1500, batch=2) for _ in range(2)]
    mp = capi.Matcher(rig, fes[0], 0, fes[0], 1)
    free = threading.Semaphore(2)
    ready = queue.Queue()
    total = NREP * len(frames)

    def extract_worker():
        for n in range(total):
            free.acquire()
            i = n % len(frames)
            f = fes[n % 2]
            f.set_image(0, frames[i][0]); f.set_image(1, frames[i][1])
            f.run()
            ready.put(n)

    th = threading.Thread(target=extract_worker, daemon=True)
    th.start()
    got = []
    for _ in range(total):
        n = ready.get(timeout=60)
        f = fes[n % 2]
        mp.bind_extractors(f, 0, f, 1)
        got.append(track(mp, f, n % len(frames)))
        free.release()
    th.join(timeout=60)
    assert all(f.ssc_stats() == (1, 0) for f in fes)
    for n, (a, b) in enumerate(zip(ref, got)):
        assert (a is None) == (b is None)
        if a is None:
            continue
        assert np.array_equal(a[0], b[0]) and a[1:4] == b[1:4], (n, a[6], b[6], np.abs(a[0] - b[0]).max())
        assert np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5]), n


def test_sequence_odometry_accuracy(capi, tmp_path):
    """End to end on a rendered sequence (no ground truth fed back): frame-to-frame stereo odometry through the C ABI
    - extract, stereo match, track against the map built from the PREVIOUS ESTIMATE, rebuild the map at the new
    estimate, constant-velocity prediction - written with vslam_save_trajectory and scored with the ATE / RPE tools
    (SURVEY section 8f row N4).  Frame-to-frame drift without BA over 25 frames stays at the millimetre level."""
    import trajectory as tj
    rig = synth.RIGS["euroc"]
    n = 25
    ge = capi.Extractor(rig["w"], rig["h"], 1500, batch=2)
    m = capi.Matcher(rig, ge, 0, ge, 1)
    gt, est = [], []
    for f in range(n):
        L, R, T = synth.stereo_frame(f)
        gt.append(T)
        ge.extract([L, R]); m.stereo_match()
        if f == 0:
            est.append(T.copy())                       # the first pose anchors the trajectory
        else:
            pred = est[-1] @ (rigid_inv(est[-2]) @ est[-1]) if f > 1 else est[-1]
            T_cw, rep = capi.tracker_track(m, pred, 1 if f == 1 else 5)
            assert rep["n_inliers"] >= 50, (f, rep)
            est.append(rigid_inv(T_cw))
        capi.tracker_init_map(m, est[-1])
    gt, est = np.stack(gt), np.stack(est)
    p = str(tmp_path / "traj.txt")
    capi.save_trajectory(p, None, np.ones(n, np.uint8), est)
    back = tj.read_kitti(p)
    ate = tj.ate_rmse(est, gt)
    te, re_ = tj.rpe(est, gt)
    path_len = np.linalg.norm(np.diff(gt[:, :3, 3], axis=0), axis=1).sum()
    print("sequence odometry: path %.3f m  ATE %.5f m  RPE %.5f m / %.6f rad" % (path_len, ate, te, re_))
    assert path_len > 0.25
    # measured: ATE 2.4 mm on a 0.30 m path, RPE 1.9 mm / 0.7 mrad per frame (rendered images with sensor noise)
    assert ate < 0.006 and te < 0.004 and re_ < 0.002, (ate, te, re_, path_len)
    assert abs(tj.ate_rmse(back, gt) - ate) < 1e-3      # the 6-significant-digit file carries the same answer
