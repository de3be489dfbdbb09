"""Loop closing of a stereo + IMU session (vslam_system_correct_loop_imu / vslam_system_close_loop_imu; DESIGN.md section 6
item 29) on the room scene, driven as tests/test_gpu_reloc_imu.py drives it: EuRoC rig, 1 500 features, source frames 0, 2, ..
with the IMU buckets of synth.imu_samples, local_mapping = 0 so that runs repeat.  The claim is projected to a rotation about
gravity and a translation, the keyframes are corrected by the yaw-only pose-graph solve (restated by tests/pgo_yaw_ref.py on the
graph rebuilt here from the session's taps and the documented edge rules), and the velocity turns with the camera.
Case (d), vslam_system_close_loop_imu on a found loop, runs on the corridor scene: a smooth out-and-back whose position along the
corridor is P (1 - cos(2 pi n / N)) / 2 with P = 1 m and N = 80, so that the IMU sees no velocity jump at the turn."""
import functools
import numpy as np
import pytest
import synth
# (one HIP runtime per process: torch renders the corridor of case (d) and comes before libvslam_hip.so, as tests/test_gpu_loop.py explains)
import torch  # noqa: F401,E402
import pgo_ref as pr
import pgo_yaw_ref as py

pytestmark = pytest.mark.gpu
RIG = synth.RIGS["euroc"]
FPS = RIG["fps"]
G = (0.0, 9.81, 0.0)
GHAT = np.array([0.0, 1.0, 0.0])
NOISE = (1.6968e-4, 1.9393e-5, 2.0e-3, 3.0e-3)
IMU = dict(gravity=G, noise=NOISE, T_bs=synth.T_BC1, hz=200)
SRC = list(range(0, 42, 2))            # 21 frames: the run holds at least 3 keyframes (asserted)


def _velocity(f):
    h = 1e-4
    return (synth.pose_at(f + h * FPS, FPS)[:3, 3] - synth.pose_at(f - h * FPS, FPS)[:3, 3]) / (2 * h)


def _bucket(f0, f1):
    S, dts, _ = synth.imu_samples(f0, f1, FPS, noise_seed=0x1A00 + f1)
    return S[:, :3], S[:, 3:], np.arange(len(dts)) * 5e6


def run(capi, **kw):
    """an IMU session over SRC, ending on a plain frame; returns (session, last pose, number of frames)"""
    synth.prerender(SRC + [SRC[-1] + 2, SRC[-1] + 4])
    s = capi.System(RIG, 1500, T0=synth.pose_at(0, FPS), imu=dict(IMU, velocity=_velocity(0)), local_mapping=kw.pop("local_mapping", 0), **kw)
    T = None
    for n, f in enumerate(SRC):
        L, R, _ = synth.stereo_frame(f)
        T, rep = s.track(L, R, n, imu_bucket=_bucket(SRC[n - 1], f) if n else None)
        assert n == 0 or rep["n_inliers"] >= 50, (f, rep["n_inliers"])
    return s, T, len(SRC)


def track_on(s, n):
    """the next two IMU frames; returns their inlier counts"""
    out = []
    for q in range(2):
        f = SRC[-1] + 2 * (q + 1)
        L, R, _ = synth.stereo_frame(f)
        _, rep = s.track(L, R, n + q, imu_bucket=_bucket(f - 2, f))
        out.append(rep["n_inliers"])
    return out


def snapshot(s):
    st = s.imu_state()
    fi, P = s.keyframes()
    xyz, ol = s.map_points()
    mt, lo = s.last_frame()
    return (s.counts(), fi.tobytes(), P.tobytes(), xyz.tobytes(), ol.tobytes(), s.active_points().tobytes(), mt.tobytes(), lo.tobytes(),
            s.covisibility().tobytes(), st["velocity"].tobytes(), st["bias"].tobytes(), st["bias_good"].tobytes(), st["pending"])


def test_pure_tilt_claim_changes_nothing(capi):
    """(a): the claim is the camera pose tilted by 2 degrees about an axis perpendicular to gravity.  The projection drops all of
    it: no yaw, zero iterations, keyframes and map points bitwise as they were, and the session tracks on."""
    s, T, n = run(capi)
    fi, P_old = s.keyframes()
    assert len(P_old) >= 3
    X_old, _ = s.map_points()
    st = s.imu_state()
    e = np.array([1.0, 0.0, 0.0])
    T_corr = pr.make_pose(pr.so3_exp(np.deg2rad(2.0) * e) @ T[:3, :3], T[:3, 3])
    rep, irep = s.correct_loop_imu(0, T_corr)
    print("yaw", irep["yaw"], "tilt dropped", irep["tilt_dropped"], "pgo", rep["pgo"])
    assert rep["busy"] == 0 and rep["success"] == 1 and rep["corrected"] == 1
    assert abs(irep["yaw"]) <= 1e-12 and abs(irep["tilt_dropped"] - np.deg2rad(2.0)) <= 1e-9
    assert abs(rep["drift_rotation"] - np.deg2rad(2.0)) <= 1e-9           # (the report of the unprojected claim)
    assert rep["T_wc_corrected"].tobytes() == T_corr.tobytes()
    assert rep["pgo"]["iterations"] == 0
    assert s.keyframes()[1].tobytes() == P_old.tobytes() and s.map_points()[0].tobytes() == X_old.tobytes()
    st2 = s.imu_state()
    assert np.abs(st2["velocity"] - st["velocity"]).max() <= 1e-14 and np.abs(irep["velocity"] - st2["velocity"]).max() == 0
    assert st2["bias"].tobytes() == st["bias"].tobytes() and st2["bias_good"].tobytes() == st["bias_good"].tobytes() and st2["pending"] == 0
    inl = track_on(s, n)
    print("inliers after the call:", inl)
    assert min(inl) >= 50
    s.close()


def test_yaw_claim_against_the_restatement(capi):
    """(b): a claim of 0.2 degrees about gravity, a tilt of 1 degree and 1 cm, anchored at keyframe 0"""
    s, T, n = run(capi)
    fi, P_old = s.keyframes()
    K = len(P_old)
    assert K >= 3
    latest, kf_loop = K - 1, 0
    X_old, outl = s.map_points()
    first_obs, _ = s.map_point_keyframes()
    cov = s.covisibility()
    st = s.imu_state()
    e = np.array([0.0, 0.0, 1.0])
    R_claim = pr.so3_exp(np.deg2rad(0.2) * GHAT) @ pr.so3_exp(np.deg2rad(1.0) * e) @ T[:3, :3]
    T_corr = pr.make_pose(R_claim, T[:3, 3] + np.array([0.01, 0.0, 0.0]))
    rep, irep = s.correct_loop_imu(kf_loop, T_corr)
    assert rep["busy"] == 0 and rep["corrected"] == 1 and rep["kf_loop"] == kf_loop
    # the projection, restated
    Tp, th, tilt = py.project_claim(T_corr, T, G)
    print("yaw", irep["yaw"], "ref", th, "tilt dropped", irep["tilt_dropped"], "ref", tilt)
    assert abs(irep["yaw"] - th) <= 1e-12 and abs(irep["tilt_dropped"] - tilt) <= 1e-12
    assert np.abs(irep["T_wc_projected"] - Tp).max() <= 1e-12
    assert abs(th - np.deg2rad(0.2)) <= 1e-3 and abs(tilt - np.deg2rad(1.0)) <= 1e-3
    assert rep["T_wc_corrected"].tobytes() == T_corr.tobytes()
    # the graph by the documented rules: sequential, covisibility >= 100 (each unordered pair once), the loop edge of the PROJECTED pose
    edges = [(k - 1, k, pr.rigid_inv(P_old[k - 1]) @ P_old[k], 1.0, 1.0) for k in range(1, K)]
    seen = set()
    for k, o, w in cov:
        a, b = min(k, o), max(k, o)
        if w >= 100 and k != o and (a, b) not in seen:
            seen.add((a, b))
            edges.append((a, b, pr.rigid_inv(P_old[a]) @ P_old[b], 1.0, 1.0))
    D = Tp @ np.linalg.inv(T)
    edges.append((kf_loop, latest, pr.rigid_inv(P_old[kf_loop]) @ D @ P_old[latest], 10.0, 10.0))
    assert (rep["n_nodes"], rep["n_sequential"], rep["n_covisibility"], rep["n_edges"]) == (K, K - 1, len(seen), len(edges))
    fixed = np.zeros(K, np.uint8); fixed[[0, kf_loop]] = 1
    want, wrep = py.optimize(P_old, fixed, edges, G)
    _, P_new = s.keyframes()
    print("pgo", rep["pgo"], "ref", wrep, "max diff", np.abs(P_new - want).max())
    assert np.abs(P_new - want).max() <= 1e-7
    assert (rep["pgo"]["accepted"], rep["pgo"]["rejected"]) == (wrep["accepted"], wrep["rejected"]) and wrep["accepted"] >= 1
    assert np.abs(P_new[latest] - P_old[latest]).max() > 1e-3            # the correction arrived
    # roll and pitch about gravity: untouched, for every keyframe and the camera
    for k in range(K):
        dR = P_new[k][:3, :3] @ P_old[k][:3, :3].T
        assert np.abs(dR @ GHAT - GHAT).max() <= 1e-12, k
    dR = rep["T_wc"][:3, :3] @ T[:3, :3].T
    assert np.abs(dR @ GHAT - GHAT).max() <= 1e-12
    # the velocity turns with the camera; bias and the pending flag stay
    st2 = s.imu_state()
    assert irep["velocity_before"].tobytes() == st["velocity"].tobytes() and irep["velocity"].tobytes() == st2["velocity"].tobytes()
    assert np.abs(st2["velocity"] - dR @ st["velocity"]).max() <= 1e-12
    assert abs(np.linalg.norm(st2["velocity"]) - np.linalg.norm(st["velocity"])) <= 1e-12 and np.linalg.norm(st["velocity"]) > 0.05
    assert st2["bias"].tobytes() == st["bias"].tobytes() and st2["bias_good"].tobytes() == st["bias_good"].tobytes() and st2["pending"] == 0
    # map points move with their first observing keyframe
    X_new, outl_new = s.map_points()
    assert np.array_equal(outl, outl_new)
    assert np.abs(X_new - pr.move_points(X_old, first_obs, P_old, P_new)).max() <= 1e-9
    inl = track_on(s, n)
    print("inliers after the correction:", inl)
    assert min(inl) >= 50
    s.close()


def test_state_machine(capi):
    """(c): every refusal leaves the session bitwise as it was; busy under local_mapping = 2; the 6-DoF calls still refuse"""
    def refused(call, word=None):
        with pytest.raises(capi.VslamError) as ex:
            call()
        return ex.value.status == capi.ERR_INVALID and (word is None or word in str(ex.value))

    s, T, n = run(capi)
    snap = snapshot(s)
    K = s.counts()["keyframes"]
    for kf in (-1, K - 1, K):                              # out of range, or the latest keyframe
        assert refused(lambda: s.correct_loop_imu(kf, T))
    bad = T.copy(); bad[0, 3] = np.nan
    assert refused(lambda: s.correct_loop_imu(0, bad))
    assert refused(lambda: s.correct_loop_imu(0, T, loop_weight=-1.0)) and refused(lambda: s.close_loop_imu(min_kf_gap=-1))
    assert refused(lambda: s.correct_loop_imu(0, T, lambda0=-1.0))
    assert refused(lambda: s.close_loop_imu(mode=2))
    # the 6-DoF calls go on refusing an IMU session
    assert refused(lambda: s.close_loop(), "IMU") and refused(lambda: s.correct_loop(0, T), "IMU")
    assert snapshot(s) == snap
    # detection alone changes nothing either (the room has no revisited place at this gap: no loop, or one that is only reported)
    rep, irep = s.close_loop_imu(detect_only=1, min_kf_gap=2)
    assert rep["corrected"] == 0 and snapshot(s) == snap
    # a pending two-phase relocalisation
    L, R, _ = synth.stereo_frame(SRC[-1])
    _, rr, ir = s.relocalize_imu(L, R, n)
    assert rr["success"] == 1 and ir["phase"] == 1 and s.imu_state()["pending"] == 1
    snap = snapshot(s)
    assert refused(lambda: s.correct_loop_imu(0, T), "pending") and refused(lambda: s.close_loop_imu(), "pending")
    assert snapshot(s) == snap
    s.close()
    # sessions the call does not serve
    L0, R0, _ = synth.stereo_frame(0)
    plain = capi.System(RIG, 1500, T0=synth.pose_at(0, FPS), local_mapping=0)
    assert refused(lambda: plain.close_loop_imu())          # (no IMU, and no frame yet)
    plain.track(L0, R0, 0)
    before = (plain.counts(), plain.keyframes()[1].tobytes(), plain.map_points()[0].tobytes())
    assert refused(lambda: plain.close_loop_imu(), "no IMU") and refused(lambda: plain.correct_loop_imu(0, np.eye(4)), "no IMU")
    assert (plain.counts(), plain.keyframes()[1].tobytes(), plain.map_points()[0].tobytes()) == before
    plain.close()
    mono = capi.MonoSystem(RIG, 1500, synth.MONO_FPS, imu=IMU)
    assert refused(lambda: mono.close_loop_imu(), "mono") and refused(lambda: mono.correct_loop_imu(0, np.eye(4)), "mono")
    mono.close()
    fresh = capi.System(RIG, 1500, imu=IMU, local_mapping=0)
    assert refused(lambda: fresh.close_loop_imu(), "no tracked frame") and refused(lambda: fresh.correct_loop_imu(0, np.eye(4)), "no tracked frame")
    fresh.close()


def test_busy_under_asynchronous_mapping(capi):
    """local_mapping = 2: a call between the hand-over of a mapping pass and its landing reports busy and does nothing"""
    synth.prerender(SRC)
    s = capi.System(RIG, 1500, T0=synth.pose_at(0, FPS), imu=dict(IMU, velocity=_velocity(0)), local_mapping=2, mapping_delay=2)
    busy = 0
    for n, f in enumerate(SRC):
        L, R, _ = synth.stereo_frame(f)
        T, rep = s.track(L, R, n, imu_bucket=_bucket(SRC[n - 1], f) if n else None)
        if s.counts()["keyframes"] < 2:
            continue
        fi, P = s.keyframes()
        v = s.imu_state()["velocity"].copy()
        r, ir = s.correct_loop_imu(0, T)                    # (the claim is the pose itself: a call that is served changes nothing either)
        if r["busy"]:
            busy += 1
            assert r["success"] == 0 and r["corrected"] == 0 and s.keyframes()[1].tobytes() == P.tobytes()
            assert s.imu_state()["velocity"].tobytes() == v.tobytes() and ir["yaw"] == 0.0
    print("busy calls:", busy)
    assert busy >= 1
    s.close()


# ---- (d): a smooth out-and-back of the corridor ------------------------------------------------------------------------------------
P_WALK, N_WALK = 1.0, 80               # metres out, frames out and back (the issue's starting values; they held on the GPU)
GAP = 2                                # min_kf_gap of every call here, as in tests/test_gpu_loop.py
N_FRAMES = N_WALK + 3                  # the walk and the two frames after the return


def walk_pose(n, fps=FPS):
    """world <- left camera at frame n of the walk: synth.corridor_pose at the source frame that lies
    P (1 - cos(2 pi n / N)) / 2 metres along the corridor (0.5 m/s at `fps`: 40 source frames per metre)"""
    return synth.corridor_pose(P_WALK * (1.0 - np.cos(2.0 * np.pi * n / N_WALK)) / 2.0 * fps / 0.5, fps)


@functools.lru_cache(maxsize=None)
def corridor_walk():
    """(left images, right images, true poses) of frames 0 .. N_WALK + 2, rendered once with a noise seed per frame"""
    rig = RIG
    planes = synth.TorchPlanes(synth.make_corridor(11), "cuda", torch.float32)
    tex = torch.from_numpy(synth.texture(0xC0FFEE).astype(np.float32)).to("cuda")
    ext = np.eye(4); ext[0, 3] = rig["bl"]
    poses = np.array([walk_pose(n) for n in range(N_FRAMES)])
    L = np.stack([synth.render_torch(planes, tex, rig, poses[n], "cuda", noise_seed=5000 + 2 * n).cpu().numpy() for n in range(N_FRAMES)])
    R = np.stack([synth.render_torch(planes, tex, rig, poses[n] @ ext, "cuda", noise_seed=5001 + 2 * n).cpu().numpy() for n in range(N_FRAMES)])
    for a in (L, R, poses):
        a.setflags(write=False)
    return L, R, poses


def walk_velocity(n):
    h = 1e-4
    return (walk_pose(n + h * FPS)[:3, 3] - walk_pose(n - h * FPS)[:3, 3]) / (2 * h)


@functools.lru_cache(maxsize=None)
def walk_bucket(n):
    """the IMU samples between frames n - 1 and n of the walk"""
    S, dts, _ = synth.imu_samples(n - 1, n, FPS, noise_seed=0x2B00 + n, pose_fn=walk_pose)
    return S[:, :3], S[:, 3:], np.arange(len(dts)) * 5e6


def drive_walk(capi, first=0, hook=None):
    """an IMU session over frames first .. N_WALK of the walk; hook(session, n, T, report) after every frame"""
    L, R, poses = corridor_walk()
    s = capi.System(RIG, 1500, T0=poses[first], imu=dict(IMU, velocity=walk_velocity(first)), local_mapping=0)
    Ts, reps = [], []
    for n in range(first, N_WALK + 1):
        T, rep = s.track(L[n], R[n], n - first, imu_bucket=walk_bucket(n) if n > first else None)
        Ts.append(T); reps.append(rep)
        if hook:
            hook(s, n, T, rep)
    return s, Ts, reps


def check_correction(P_old, P_new, T_old, T_new, st_old, st_new, irep):
    """the invariants of (b) after a committed correction"""
    for k in range(len(P_old)):
        dR = P_new[k][:3, :3] @ P_old[k][:3, :3].T
        assert np.abs(dR @ GHAT - GHAT).max() <= 1e-12, k
    dR = T_new[:3, :3] @ T_old[:3, :3].T
    assert np.abs(dR @ GHAT - GHAT).max() <= 1e-12
    assert irep["velocity_before"].tobytes() == st_old["velocity"].tobytes() and irep["velocity"].tobytes() == st_new["velocity"].tobytes()
    assert np.abs(st_new["velocity"] - dR @ st_old["velocity"]).max() <= 1e-12
    assert abs(np.linalg.norm(st_new["velocity"]) - np.linalg.norm(st_old["velocity"])) <= 1e-12
    assert st_new["bias"].tobytes() == st_old["bias"].tobytes() and st_new["bias_good"].tobytes() == st_old["bias_good"].tobytes()
    assert st_new["pending"] == 0


@functools.lru_cache(maxsize=None)
def alone(first):
    """a session driven alone over frames first .. N_WALK, then close_loop_imu: what tests/test_gpu_batch_loop_imu.py compares a
    lane with.  Returns (report, IMU report, keyframe poses before, after, IMU state after)."""
    import vslam_capi
    s, Ts, reps = drive_walk(vslam_capi, first)
    P_old = s.keyframes()[1]
    rep, irep = s.close_loop_imu(min_kf_gap=GAP)
    out = (rep, irep, P_old, s.keyframes()[1], s.imu_state())
    s.close()
    return out


def test_close_loop_imu_on_the_corridor_walk(capi):
    """(d): detect_only after EVERY frame leaves the session bitwise alone and finds nothing before the return; at the return a
    loop is found against a keyframe of the way out, the projected pose is the truth within 3 x 1.5e-3 (the bound and source of
    tests/test_gpu_loop.py), the full call commits the yaw-only correction with the invariants of (b), and two further frames track."""
    L, R, truth = corridor_walk()
    log = []

    def hook(s, n, T, rep):
        before = snapshot(s)
        d, ir = s.close_loop_imu(detect_only=1, min_kf_gap=GAP)
        assert snapshot(s) == before, n
        assert d["T_wc"].tobytes() == T.tobytes() and d["corrected"] == 0 and d["busy"] == 0
        log.append((n, d, ir, before[0]["keyframes"]))

    s, Ts, reps = drive_walk(capi, 0, hook)
    print("inliers: min %d; keyframes %d" % (min(r["n_inliers"] for r in reps[1:]), s.counts()["keyframes"]))
    assert min(r["n_inliers"] for r in reps[1:]) >= 50
    kf_out = max(k for n, d, ir, k in log if n <= N_WALK // 2)
    assert kf_out >= 5
    for n, d, ir, k in log:
        print(n, "success", d["success"], "cand", d["n_candidates"], "kf_loop", d["kf_loop"], "inl", d["reloc"]["n_inliers"], "kfs", k)
        if n <= N_WALK // 2:
            assert d["success"] == 0                       # nothing to close before the return
    n, d, ir, k = log[-1]
    assert n == N_WALK and d["success"] == 1 and 0 <= d["kf_loop"] < kf_out
    err = np.abs(ir["T_wc_projected"] - truth[N_WALK]).max()
    print("projected pose against the ground truth: %.3e; yaw %.3e, tilt dropped %.3e" % (err, ir["yaw"], ir["tilt_dropped"]))
    assert err <= 3 * 1.5e-3
    Tp, th, tilt = py.project_claim(d["T_wc_corrected"], Ts[-1], G)
    assert abs(ir["yaw"] - th) <= 1e-12 and abs(ir["tilt_dropped"] - tilt) <= 1e-12 and np.abs(ir["T_wc_projected"] - Tp).max() <= 1e-12
    # the full call
    P_old = s.keyframes()[1]
    st = s.imu_state()
    rep, irep = s.close_loop_imu(min_kf_gap=GAP)
    print({k: v for k, v in rep.items() if k not in ("T_wc", "T_wc_corrected", "reloc")}, "yaw", irep["yaw"])
    assert rep["success"] == 1 and rep["corrected"] == 1 and rep["kf_loop"] == d["kf_loop"]
    assert irep["yaw"] == ir["yaw"] and irep["T_wc_projected"].tobytes() == ir["T_wc_projected"].tobytes()      # (local_mapping 0: nothing to propagate)
    P_new = s.keyframes()[1]
    assert np.abs(P_new - P_old).max() > 0 and P_new[rep["kf_loop"]].tobytes() == P_old[rep["kf_loop"]].tobytes()
    check_correction(P_old, P_new, Ts[-1], rep["T_wc"], st, s.imu_state(), irep)
    for q in (1, 2):
        T, r = s.track(L[N_WALK + q], R[N_WALK + q], N_WALK + q, imu_bucket=walk_bucket(N_WALK + q))
        print("frame after the correction:", r["n_inliers"], "inliers")
        assert r["n_inliers"] >= 50
    s.close()
