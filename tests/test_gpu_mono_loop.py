"""The mono + IMU closed loop behind vslam_system (VSlamSystem::TrackMonoIMU) against its CPU restatement (tests/mono_loop_ref.py),
call by call on the sequence of tests/test_mono_loop_ref.py: EuRoC rig 752 x 480, 1500 features, 17 calls - two refused by the
movement gate, three bootstrap keyframes, the initialisation, ten tracked calls that hold the map and one that runs every retry
round and loses it."""
import os
import numpy as np
import pytest
import synth
import mono_loop_ref as ml

pytestmark = pytest.mark.gpu
RIG = synth.RIGS["euroc"]
IMU = dict(gravity=ml.G, noise=ml.NOISE, T_bs=synth.T_BC1, hz=200)
REPORT_FIELDS = ("state", "keyframe_inserted", "n_active", "n_inliers", "rounds", "last_radius", "new_points", "radius_matches",
                 "n_keyframes", "n_map_points", "n_active_after")


def bucket(k):
    S, _, ts = synth.mono_bucket(k)
    return S[:, :3], S[:, 3:], ts


def new_session(capi, **kw):
    return capi.MonoSystem(RIG, ml.NFEAT, synth.MONO_FPS, T0=synth.mono_arc_pose(0), imu=IMU, **kw)


def feed(ms, k, how="gray", capi=None, keep=None):
    img = synth.mono_frame(synth.MONO_CALLS[k])[0]
    if how == "bgr":
        img = np.repeat(img[:, :, None], 3, axis=2)
    elif how == "bgra":
        img = np.concatenate([np.repeat(img[:, :, None], 3, axis=2), np.full(img.shape + (1,), 255, np.uint8)], axis=2)
    elif how == "device":
        d = capi.DeviceImage(img)
        keep.append(d)
        return ms.track(d.ptr, synth.MONO_CALLS[k], bucket(k), channels=1, on_device=True)
    return ms.track(img, synth.MONO_CALLS[k], bucket(k))


@pytest.fixture(scope="module")
def gpu_run(capi, tmp_path_factory):
    """the whole sequence once, gray host frames; everything the tests compare, read out call by call"""
    ms = new_session(capi)
    calls = []
    for k in range(len(synth.MONO_CALLS)):
        T, rep = feed(ms, k)
        mt, ol = ms.last_frame()
        calls.append(dict(T=T, rep=rep, matches=mt, outliers=ol, counts=ms.counts(), points=ms.map_points()[0] if rep["state"] == 2 else None))
    path = str(tmp_path_factory.mktemp("mono") / "trajectory.txt")
    ms.save_trajectory(path)
    out = dict(calls=calls, kf=ms.keyframes(), memory=ms.memory(), counts=ms.counts(), trajectory=open(path).read().splitlines())
    ms.close()
    return out


def test_call_by_call_parity(gpu_run):
    lg = ml.reference_run().log
    prev = synth.mono_arc_pose(0)
    for k, (g, r) in enumerate(zip(gpu_run["calls"], lg)):
        rep = g["rep"]
        want = dict(state=r["state"], keyframe_inserted=int(r["keyframe"]), n_active=r["nActive"], n_inliers=r["nIn"], rounds=r["rounds"],
                    last_radius=r["radius"], new_points=r["new_points"], radius_matches=r["radius_matches"], n_keyframes=r["n_keyframes"],
                    n_map_points=r["n_map_points"], n_active_after=r["n_active_after"])
        got = {f: rep[f] for f in REPORT_FIELDS}
        assert got == want, (k, got, want)
        assert rep["frame"] == synth.MONO_CALLS[k]
        assert g["counts"]["keyframes"] == r["n_keyframes"] and g["counts"]["map_points"] == r["n_map_points"]
        assert g["counts"]["active"] == r["n_active_after"]
        assert np.array_equal(g["matches"], r["matches"]) and np.array_equal(g["outliers"], r["outliers"]), k
        assert np.abs(g["T"] - r["pose"]).max() < 1e-6, (k, np.abs(g["T"] - r["pose"]).max())
        if r["state"] == ml.REFUSED:
            assert np.array_equal(g["T"], prev)           # a refused call returns the previous pose unchanged
        prev = g["T"]
    assert sum(r["state"] == ml.TRACKED for r in lg) >= 8 and any(r["outliers"].any() for r in lg)
    assert gpu_run["calls"][-1]["rep"]["rounds"] == 5 and gpu_run["calls"][-1]["rep"]["n_inliers"] < 50      # the retry rounds ran


def test_keyframes_map_points_trajectory_and_slots(gpu_run):
    ref = ml.reference_run()
    fi, P = gpu_run["kf"]
    assert list(fi) == [kf.frameIdx for kf in ref.keyFrames]
    for k, kf in enumerate(ref.keyFrames):
        assert np.abs(P[k] - kf.pose).max() < 1e-6
    init = next(g for g in gpu_run["calls"] if g["rep"]["state"] == 2)
    want = np.stack([mp.wp for mp in ref.mapPoints])
    assert init["points"].shape == want.shape and len(want) >= 200
    assert (np.abs(init["points"] - want).max(axis=1) / np.maximum(1.0, np.abs(want).max(axis=1))).max() < 1e-9
    # allFrames holds accepted calls only: one trajectory line each
    accepted = sum(r["state"] != ml.REFUSED for r in ref.log)
    assert gpu_run["counts"]["frames"] == accepted == len(gpu_run["trajectory"]) == 15
    # only the bootstrap keyframes and the initialising one hold a key slot; the keyframes of tracked calls hold none
    slotted = sum(r["state"] in (ml.BOOTSTRAP, ml.INITIALISED) for r in ref.log)
    assert gpu_run["memory"]["key_slots_used"] == slotted == 4 < gpu_run["counts"]["keyframes"]
    assert gpu_run["memory"]["key_slab_bytes"] > 0


@pytest.mark.parametrize("how", ["bgr", "bgra", "device"])
def test_first_calls_fed_three_ways(capi, gpu_run, how):
    ms = new_session(capi)
    keep = []
    for k in range(8):
        T, rep = feed(ms, k, how, capi, keep)
        g = gpu_run["calls"][k]
        assert np.array_equal(T, g["T"]) and rep == g["rep"], (how, k)
        mt, ol = ms.last_frame()
        assert np.array_equal(mt, g["matches"]) and np.array_equal(ol, g["outliers"])
    ms.close()


def test_errors_leave_the_session_unchanged(capi, gpu_run):
    ms = new_session(capi)
    for k in range(3):
        feed(ms, k)
    before = ms.counts()
    img = synth.mono_frame(synth.MONO_CALLS[3])[0]
    e3 = np.zeros((0, 3))
    for bad in (None, (e3, e3, np.zeros(0))):              # NULL and empty bucket
        with pytest.raises(capi.VslamError) as ei:
            ms.track(img, synth.MONO_CALLS[3], bad)
        assert ei.value.status == capi.ERR_INVALID
    with pytest.raises(capi.VslamError) as ei:            # a stereo call on the mono session
        capi.System.track(ms, img, img, synth.MONO_CALLS[3], imu_bucket=bucket(3))
    assert ei.value.status == capi.ERR_INVALID
    with pytest.raises(capi.VslamError) as ei:            # channels
        ms.track(img.ctypes.data, synth.MONO_CALLS[3], bucket(3), channels=2, on_device=True)
    assert ei.value.status == capi.ERR_INVALID
    assert ms.counts() == before
    for k in range(3, 8):                                  # the next calls are those of the undisturbed run, bit for bit
        T, rep = feed(ms, k)
        assert np.array_equal(T, gpu_run["calls"][k]["T"]) and rep == gpu_run["calls"][k]["rep"], k
    ms.close()
    # the mono call on a stereo session
    L, R, _ = synth.stereo_frame(0)
    S, dts, _ = synth.imu_samples(0, 1)
    b = (S[:, :3], S[:, 3:], np.arange(len(dts)) * 5e6)
    a, u = (capi.System(RIG, ml.NFEAT, T0=synth.pose_at(0), imu=IMU, local_mapping=0) for _ in range(2))
    with pytest.raises(capi.VslamError) as ei:
        capi.MonoSystem.track(a, L, 0, b)
    assert ei.value.status == capi.ERR_INVALID
    assert a.counts() == u.counts()
    Ta, ra = a.track(L, R, 0)
    Tu, ru = u.track(L, R, 0)
    assert np.array_equal(Ta, Tu) and ra == ru and a.counts() == u.counts()
    a.close(); u.close()
    # creation
    for kw, fps in ((dict(imu=None), 20.0), (dict(imu=IMU, local_mapping=1), 20.0), (dict(imu=IMU, local_mapping=2), 20.0),
                    (dict(imu=IMU), 0.0), (dict(imu=IMU), -20.0)):
        with pytest.raises(capi.VslamError) as ei:
            capi.MonoSystem(RIG, ml.NFEAT, fps, T0=synth.mono_arc_pose(0), **kw)
        assert ei.value.status == capi.ERR_INVALID


def _swing(yaw_deg, lift):
    """from rest at mono_arc_pose(0) to rest `yaw_deg` / `lift` away within 10 frames (cosine ease), as the sequence's knots"""
    def pose(i, fps=synth.MONO_FPS):
        e = 0.5 * (1.0 - np.cos(np.pi * min(max(i / 10.0, 0.0), 1.0)))
        a = np.radians(yaw_deg * e)
        Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        T = np.eye(4)
        T[:3, :3] = np.diag([-1.0, -1.0, 1.0]) @ Ry
        T[:3, 3] = [0.0, 0.4 - lift * e, 0.0]
        return T
    return pose


@pytest.mark.parametrize("yaw,lift,state", [(8.0, 0.05, 0), (2.0, 0.15, 0), (8.0, 0.097, 0), (8.0, 0.106, 1), (5.3, 0.15, 1), (4.7, 0.15, 0)])
def test_gate_in_the_library(capi, yaw, lift, state):
    """The movement gate of the session itself, on first calls whose bucket holds a chosen motion: enough rotation but too little
    translation, the reverse, and both conditions a few per cent on either side of their thresholds.  A refused call returns
    the start pose and inserts nothing; the decision and the pose equal the restatement's."""
    pose = _swing(yaw, lift)
    S, dts, _ = synth.imu_samples(0, 10, fps=synth.MONO_FPS, pose_fn=pose)
    img = synth.random_image(RIG["w"], RIG["h"], 7)
    ref = ml.MonoLoop(RIG, ml.NFEAT, synth.MONO_FPS, T0=pose(0), imu=ml.imu_config())
    Pr = ref.track(img, 10, (S, dts))
    lg = ref.log[-1]
    assert lg["state"] == state and abs(lg["baseline"] - lift) < 0.04 * lift and abs(lg["angle"] - yaw) < 0.05      # the bucket holds the motion
    ms = capi.MonoSystem(RIG, ml.NFEAT, synth.MONO_FPS, T0=pose(0), imu=IMU)
    T, rep = ms.track(img, 10, (S[:, :3], S[:, 3:], np.arange(len(dts)) * 5e6))
    assert rep["state"] == state and rep["keyframe_inserted"] == state and ms.counts()["keyframes"] == state
    assert np.abs(T - Pr).max() < 1e-6
    if state == 0:
        assert np.array_equal(T, pose(0))
    ms.close()
