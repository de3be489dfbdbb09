"""Loop closing of a stereo session (vslam_system_close_loop / vslam_system_correct_loop) on the corridor scene: one session
walks out along the corridor and back over the same source frames in reverse.  Detection is checked at the return, the
correction against the numpy restatement of the pose-graph solve (tests/pgo_ref.py) on the graph rebuilt here from the
session's taps and the documented edge rules."""
import functools
import numpy as np
import pytest
import synth
# One HIP runtime per process: the corridor is rendered by torch (synth.corridor_sequence); if libvslam_hip.so is loaded first and
# torch afterwards, the process holds two copies of the runtime and the second to start finds no device.  Importing torch first
# makes the loader hand one copy to both - tests/test_multi.py and bench.py do the same.
import torch  # noqa: F401,E402
import pgo_ref as pr

pytestmark = pytest.mark.gpu

RIG = synth.RIGS["euroc"]
# source frames between two frames of the walk (2.5 cm at the corridor's 0.5 m/s), and frames on the way out.  Found on the GPU
# (1 500 features): with stride 1 and 40 frames the session has 10 (local_mapping 0) / 7 (1) keyframes at the turn-round, never
# fewer than 239 inliers, and tracks on after a correction.  Larger strides do not give a usable walk: with 2 and 3 the frames
# after a committed correction are lost (10 - 31 inliers), with 3 the session is also 0.35 - 0.44 m from the truth at the end,
# with 4 and 6 it already loses the turn-round (9 - 19 inliers for fifteen frames and more).
STRIDE = 1
N_OUT = 40
GAP = 2                       # min_kf_gap of every call here


@functools.lru_cache(maxsize=None)
def walk():
    """(left images, right images, true poses) of the way out, rendered once; frame j of the way back is frame N_OUT - 2 - j"""
    Ls, Rs, poses, _ = synth.corridor_sequence("euroc", N_OUT, "cuda", frame_step=STRIDE)
    L, R = Ls.cpu().numpy(), Rs.cpu().numpy()
    for a in (L, R, poses):
        a.setflags(write=False)
    return L, R, poses


def schedule():
    return list(range(N_OUT)) + list(range(N_OUT - 2, -1, -1))


def run(capi, local_mapping, hook=None, upto=None, **kw):
    """tracks the walk; hook(session, n, j, T, report) after every frame.  Returns (session, poses, reports)."""
    L, R, poses = walk()
    s = capi.System(RIG, 1500, T0=poses[0], local_mapping=local_mapping, **kw)
    Ts, reps = [], []
    for n, j in enumerate(schedule()[:upto]):
        T, rep = s.track(L[j], R[j], n)
        Ts.append(T); reps.append(rep)
        if hook:
            hook(s, n, j, T, rep)
    return s, Ts, reps


def snapshot(s):
    """everything the taps show of a session, as bytes"""
    kf_idx, kf_pose = s.keyframes()
    xyz, outl = s.map_points()
    mt, ol = s.last_frame()
    return (s.counts(), kf_idx.tobytes(), kf_pose.tobytes(), xyz.tobytes(), outl.tobytes(), s.active_points().tobytes(), mt.tobytes(), ol.tobytes(),
            s.covisibility().tobytes())


@pytest.mark.parametrize("local_mapping", [0, 1, 2])
def test_detection_leaves_the_session_alone(capi, local_mapping):
    """(a), (b), (e): close_loop with detect_only after EVERY frame.  No call changes anything the taps show (bitwise), and its
    report's camera pose is the tracked one; on the way out no loop is found; back at the start one is, against a keyframe of
    the way out; with local_mapping = 2 calls between hand-over and landing report busy.
    local_mapping = 0: the whole run also tracks frame for frame as a run without the calls - poses bitwise, reports equal; this
    is what shows that nothing of step D reaches the matcher the next frame uses.  With local mapping on that comparison cannot
    be made: two runs WITHOUT any call already differ from each other (measured with this walk at stride 3: local_mapping 1 from
    frame 3 on, up to 1.9e-2 in a pose entry; local_mapping 2 from frame 5 on, 8.4e-6) - the local BA's result is not
    reproducible run to run, with or without this change.  The tracking path is the same code in all three modes."""
    kw = dict(mapping_delay=2) if local_mapping == 2 else {}
    log = []

    def hook(s, n, j, T, rep):
        before = snapshot(s)
        d = s.close_loop(detect_only=1, min_kf_gap=GAP)
        assert snapshot(s) == before, n
        assert d["T_wc"].tobytes() == T.tobytes() and d["corrected"] == 0
        log.append((n, j, d, before[0]["keyframes"]))

    s, Tg, Rg = run(capi, local_mapping, hook, **kw)
    assert min(r["n_inliers"] for r in Rg[1:]) >= 50       # the walk is tracked throughout
    if local_mapping == 0:
        plain, Tp, Rp = run(capi, local_mapping, **kw)
        plain.close()
        for n in range(len(Tp)):
            assert Tg[n].tobytes() == Tp[n].tobytes(), n
            assert Rg[n] == Rp[n], n
    kf_out = max(k for n, j, d, k in log if n < N_OUT)
    assert kf_out >= 5                                     # at least four keyframes beyond the first on the way out
    for n, j, d, k in log:
        print(n, j, "busy", d["busy"], "success", d["success"], "cand", d["n_candidates"], "kf_loop", d["kf_loop"], "inl", d["reloc"]["n_inliers"],
              "drift", d["drift_translation"], "kfs", k)
        if n < N_OUT:
            assert d["success"] == 0                       # (a): nothing to close before the return
    if local_mapping == 2:
        assert any(d["busy"] for n, j, d, k in log)
        for n, j, d, k in log:
            if d["busy"]:
                assert d["success"] == 0 and d["n_candidates"] == 0
    else:
        assert not any(d["busy"] for n, j, d, k in log)
    # (b): the last frame is the first frame again
    n, j, d, k = [e for e in log if not e[2]["busy"]][-1]
    assert j <= 1 and d["success"] == 1 and 0 <= d["kf_loop"] < kf_out
    _, _, truth = walk()
    err = np.abs(d["T_wc_corrected"] - truth[j]).max()
    print("relocalised pose against the ground truth: %.3e" % err)
    # the bound of tests/test_gpu_reloc.py::test_relocalise_rendered_frames against the ground truth: three times the
    # restatement's own error there (1.17e-3 .. 1.50e-3 over its frames)
    assert err <= 3 * 1.5e-3
    s.close()


def in_frame(T_wc, X):
    Xc = (X - T_wc[:3, 3]) @ T_wc[:3, :3]                    # R^T (X - t)
    z = Xc[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        u = RIG["fx"] * Xc[:, 0] / z + RIG["cx"]
        v = RIG["fy"] * Xc[:, 1] / z + RIG["cy"]
    inside = (z > 0) & (u >= 0) & (v >= 0) & (u < RIG["w"]) & (v < RIG["h"])
    margin = np.minimum(np.minimum(np.abs(u), np.abs(v)), np.minimum(np.abs(u - RIG["w"]), np.abs(v - RIG["h"])))
    return inside, (margin < 1e-6) | (np.abs(z) < 1e-9)      # (second: too close to a border to call)


def read_trajectory(s, tmp_path, name):
    p = str(tmp_path / name)
    s.save_trajectory(p)
    rows = np.loadtxt(p).reshape(-1, 3, 4)
    out = np.tile(np.eye(4), (len(rows), 1, 1))
    out[:, :3, :] = rows
    return out


@pytest.mark.parametrize("local_mapping", [0, 1])
def test_correct_loop_with_injected_drift(capi, tmp_path, local_mapping):
    """(c): the camera is said to be 0.3 m and 2 degrees away from where the session believes it is, anchored at keyframe 1"""
    L, R, truth = walk()
    s, Ts, reps = run(capi, local_mapping)
    n = len(Ts)
    while reps[-1]["keyframe_inserted"]:                   # (a local BA whose poses have not been propagated would move keyframes
        T, rep = s.track(L[0], R[0], n)                    #  inside the call: end on a plain frame)
        Ts.append(T); reps.append(rep); n += 1
    fidx, P_old = s.keyframes()
    K = len(P_old)
    latest, kf_loop = K - 1, 1
    X_old, outl = s.map_points()
    first_obs, _ = s.map_point_keyframes()
    traj_old = read_trajectory(s, tmp_path, "before.txt")
    cov = s.covisibility()
    drift = pr.make_pose(pr.so3_exp(np.array([0.0, np.deg2rad(2.0), 0.0])), np.array([0.3, 0.0, 0.0]))
    T_corr = truth[0] @ drift
    rep = s.correct_loop(kf_loop, T_corr)
    assert rep["busy"] == 0 and rep["corrected"] == 1 and rep["kf_loop"] == kf_loop
    # the graph by the documented rules: sequential, covisibility >= 100 (each unordered pair once), the loop edge
    edges = [(k - 1, k, pr.rigid_inv(P_old[k - 1]) @ P_old[k], 1.0, 1.0) for k in range(1, K)]
    seen = set()
    for k, o, w in cov:
        a, b = min(k, o), max(k, o)
        if w >= 100 and k != o and (a, b) not in seen:
            seen.add((a, b))
            edges.append((a, b, pr.rigid_inv(P_old[a]) @ P_old[b], 1.0, 1.0))
    D = T_corr @ np.linalg.inv(Ts[-1])
    edges.append((kf_loop, latest, pr.rigid_inv(P_old[kf_loop]) @ D @ P_old[latest], 10.0, 10.0))
    assert (rep["n_nodes"], rep["n_sequential"], rep["n_covisibility"], rep["n_edges"]) == (K, K - 1, len(seen), len(edges))
    fixed = np.zeros(K, np.uint8); fixed[[0, kf_loop]] = 1
    want, wrep = pr.optimize(P_old, fixed, edges)
    _, P_new = s.keyframes()
    print("pgo", rep["pgo"], "ref", wrep, "max diff", np.abs(P_new - want).max(), "drift", rep["drift_translation"], rep["drift_rotation"])
    assert np.abs(P_new - want).max() <= 1e-7
    assert P_new[0].tobytes() == P_old[0].tobytes() and P_new[kf_loop].tobytes() == P_old[kf_loop].tobytes()
    assert np.abs(P_new[latest] - P_old[latest]).max() > 0.05          # the correction arrived
    # map points move with their first observing keyframe
    X_new, outl_new = s.map_points()
    assert np.array_equal(outl, outl_new)
    X_want = pr.move_points(X_old, first_obs, P_old, P_new)
    assert np.abs(X_new - X_want).max() <= 1e-9 and rep["points_moved"] == int((first_obs >= 0).sum())
    # the camera follows the latest keyframe; so does every plain frame of the trajectory (the file carries 6 digits)
    T_cam = P_new[latest] @ np.linalg.inv(P_old[latest]) @ Ts[-1]
    assert np.abs(rep["T_wc"] - T_cam).max() <= 1e-9
    traj_new = read_trajectory(s, tmp_path, "after.txt")
    assert len(traj_new) == len(traj_old) == len(Ts)
    kf_of = np.maximum.accumulate(np.where(np.isin(np.arange(len(Ts)), fidx), np.arange(len(Ts)), 0))
    where = {f: k for k, f in enumerate(fidx)}
    for f in range(len(Ts)):
        k = where[kf_of[f]]
        exp = P_new[k] if f in where else P_new[k] @ np.linalg.inv(P_old[k]) @ traj_old[f]
        assert np.abs(traj_new[f] - exp)[:3].max() <= 2e-5, f
    # the active set: every non-outlier map point inside the left image under the new camera pose, in creation order
    inside, unsure = in_frame(rep["T_wc"], X_new)
    act = s.active_points()
    assert np.all(np.diff(act) > 0) and rep["n_active_after"] == len(act)
    got = np.zeros(len(X_new), bool); got[act] = True
    wanted = inside & (outl_new == 0)
    assert np.array_equal(got[~unsure], wanted[~unsure]) and not got[outl_new != 0].any()
    assert len(s.last_frame()[0]) == 0
    before = s.counts()
    assert before["keyframes"] == K and before["frames"] == len(Ts)
    # tracking goes on from the corrected pose
    for q, j in enumerate((1, 2)):
        T, r = s.track(L[j], R[j], n + q)
        print("frame after the correction:", r["n_inliers"], "inliers")
        assert r["n_inliers"] >= 50
    s.close()


def test_close_loop_at_the_return(capi):
    """(d): the full call at the return hands map points of the way out back to the tracker"""
    L, R, truth = walk()
    s, Ts, reps = run(capi, 1)
    _, creator = s.map_point_keyframes()
    kf_out = max(r["n_keyframes"] for r in reps[:N_OUT])
    act = s.active_points()
    old = creator[act] < kf_out                            # created on the way out and tracked ever since (the far end wall)
    rep = s.close_loop(min_kf_gap=GAP)
    print({k: v for k, v in rep.items() if k not in ("T_wc", "T_wc_corrected")})
    assert rep["success"] == 1 and rep["corrected"] == 1 and 0 <= rep["kf_loop"] < kf_out
    act2 = s.active_points()
    cand_old = creator[act2] < kf_out
    print("active before: %d (%d old), after: %d (%d old)" % (len(act), old.sum(), len(act2), cand_old.sum()))
    # the candidates were by definition not active before the call; after it the active set holds the way out's points again
    assert cand_old.sum() >= old.sum() + 50 and rep["n_active_after"] == len(act2)
    n = len(Ts)
    for q, j in enumerate((1, 2, 3)):
        T, r = s.track(L[j], R[j], n + q)
        assert r["n_inliers"] >= 50                       # no lost frame
    s.close()


def test_refusals(capi):
    L, R, truth = walk()
    s = capi.System(RIG, 1500, T0=truth[0], local_mapping=0)

    def refused(call):
        with pytest.raises(capi.VslamError) as ex:
            call()
        return ex.value.status == capi.ERR_INVALID

    assert refused(lambda: s.close_loop()) and refused(lambda: s.correct_loop(0, np.eye(4)))       # no tracked frame yet
    T, _ = s.track(L[0], R[0], 0)
    state = (s.counts(), s.keyframes()[1].tobytes(), s.map_points()[0].tobytes())
    for kf in (-1, 0, 1):                                  # keyframe 0 is the latest: equal to it or out of range
        assert refused(lambda: s.correct_loop(kf, T))
    bad = T.copy(); bad[0, 3] = np.nan
    assert refused(lambda: s.correct_loop(0, bad))
    assert refused(lambda: s.close_loop(min_kf_gap=-1)) and refused(lambda: s.close_loop(loop_weight=-1.0))
    assert refused(lambda: s.close_loop(mode=2))
    assert (s.counts(), s.keyframes()[1].tobytes(), s.map_points()[0].tobytes()) == state
    rep = s.close_loop(min_kf_gap=GAP)                     # one keyframe: no candidates
    assert rep["success"] == 0 and rep["n_candidates"] == 0 and rep["corrected"] == 0
    s.close()
    imu = dict(gravity=(0.0, 9.81, 0.0), noise=(1.7e-4, 2e-5, 2e-3, 3e-3), T_bs=np.eye(4), hz=200)
    si = capi.System(RIG, 1500, T0=truth[0], imu=imu, local_mapping=0)
    si.track(L[0], R[0], 0)
    assert refused(lambda: si.close_loop()) and refused(lambda: si.correct_loop(0, T))
    assert si.counts()["keyframes"] == 1
    si.close()
    sm = capi.MonoSystem(RIG, 1500, RIG["fps"], T0=truth[0], imu=imu)
    assert refused(lambda: sm.close_loop()) and refused(lambda: sm.correct_loop(0, T))
    sm.close()
