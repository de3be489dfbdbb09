"""The stereo tracking frame's slow half - the reference's retry rule (src/FeatureTracker.cpp:1184-1233), which runs only when
the first matching round ends with fewer than 50 inliers: host-driven rounds, the reset of a failed round, the radius widened
by 30 px, the fall-back to the previous radius when a wider round does worse, the cap after round 4, the ungated refinement
and, in IMU mode, the bias chained through every retried solve - pinned at three levels:

1. the matcher (tracker_set_map + tracker_track[_imu]) against oracle_track, one frame per branch of the rule;
2. the session (vslam_system) against the oracle's closed loop on schedules whose jumps make frames retry, end lost, and
   insert keyframes while lost;
3. vslam_batch / vslam_fleet, where a retried lane leaves the step another way than its neighbours (state fetched again in
   the one-session layout, packed keys dropped, retry launches after the next frames' extraction was prefetched): every lane
   must equal the single session of its schedule.

Every case asserts the ORACLE's round count for its inputs first, so none can decay into a one-round frame."""
import numpy as np
import pytest
import synth
from test_gpu_track import oracle_track, oracle_init_map, rigid_inv
from test_gpu_system import _run, _check
from test_gpu_batch import _single, _batched, _same, G, NOISE

pytestmark = pytest.mark.gpu

RIG_NAME, NFEAT = "euroc", 1500

# ---- 1. matcher level ----------------------------------------------------------------------------------------------------------
_FRAMES = {}


def _frame(oracle, f):
    """oracle extraction + stereo match of rendered frame f and the map initializeMap makes of it at its true pose:
    computed once, shared by the cases, never modified (every user copies what it changes)"""
    if f not in _FRAMES:
        rig = synth.RIGS[RIG_NAME]
        L, R, T = synth.stereo_frame(f, RIG_NAME)
        oL, oR = oracle.Extractor(NFEAT), oracle.Extractor(NFEAT)
        kL, dL = oL.extract(L); kR, dR = oR.extract(R)
        st = oracle.stereo_match(oL, oR, rig, kL, dL, kR, dR)
        _FRAMES[f] = dict(L=L, R=R, T=T, ex=oL, keys=(kL, dL, kR, dR), st=st, map=oracle_init_map(rig, oL, kL, dL, st, T))
    return _FRAMES[f]


def _imu_inputs(oracle, f0, f1):
    """the setup of test_gpu_track.test_track_frame_imu_parity"""
    h = 1e-4
    v_prev = (synth.pose_at(f0 + h * 20)[:3, 3] - synth.pose_at(f0 - h * 20)[:3, 3]) / (2 * h)
    S, dts, _ = synth.imu_samples(f0, f1, noise_seed=5)
    prm = oracle.imu_params(G, NOISE[0], NOISE[2], NOISE[1], NOISE[3], synth.T_BC1)
    return dict(prm=prm, T_prev=synth.stereo_frame(f0, RIG_NAME)[2], v_prev=v_prev, S=S, dts=dts, ts=np.arange(len(dts)) * 5e6)


def _oracle_frame(oracle, f1, mp, pred, frame_number, outlier=None, imu=None):
    rig = synth.RIGS[RIG_NAME]
    fr = _frame(oracle, f1)
    st = {k: np.array(v, copy=True) for k, v in fr["st"].items()}
    oimu = (imu["prm"], imu["T_prev"], imu["v_prev"], np.zeros(6), imu["S"], imu["dts"]) if imu else None
    return oracle_track(oracle, rig, fr["ex"], fr["keys"], st, mp, pred, frame_number, imu=oimu, outlier=outlier)


def _gpu_frame_equals(capi, oracle, f1, mp, pred, frame_number, ref, outlier=None, imu=None, pose_tol=1e-9):
    """the comparison of test_gpu_track._track_frame_parity on an uploaded map, plus the last radius"""
    rig = synth.RIGS[RIG_NAME]
    fr = _frame(oracle, f1)
    kL, _, kR, _ = fr["keys"]
    ge = capi.Extractor(rig["w"], rig["h"], NFEAT, batch=2)
    m = capi.Matcher(rig, ge, 0, ge, 1)
    ge.extract([fr["L"], fr["R"]]); m.stereo_match()
    capi.tracker_set_map(m, mp[0], mp[1], mp[2], is_outlier=outlier)
    if imu is None:
        T_cw, rep = capi.tracker_track(m, pred, frame_number)
    else:
        T_cw, rep, vel, bias = capi.tracker_track_imu(m, pred, frame_number, G, NOISE, synth.T_BC1, imu["T_prev"], imu["v_prev"], np.zeros(6),
                                                      imu["S"][:, :3], imu["S"][:, 3:], imu["ts"], 200)
    mt, outl, act = capi.tracker_fetch(m)
    dev = float(np.abs(T_cw - ref["T_cw"]).max())
    print("rounds %d (oracle %d)  inliers %d (%d)  last radius %g (%g)  pose deviation %.3e" %
          (rep["rounds"], ref["rounds"], rep["n_inliers"], ref["nIn"], rep["last_radius"], ref["last_radius"], dev))
    assert rep["n_map_points"] == len(mp[0]) and rep["n_active"] == len(ref["act"])
    assert np.array_equal(act, ref["act"])
    assert rep["rounds"] == ref["rounds"] and rep["lm_iterations"] == ref["iters"]
    assert rep["last_radius"] == ref["last_radius"]
    assert (rep["n_inliers"], rep["n_stereo"]) == (ref["nIn"], ref["nStereo"])
    assert np.array_equal(mt, ref["matches"]) and np.array_equal(outl, ref["outliers"])
    st2 = m.stereo_fetch(len(kL), len(kR))
    assert np.array_equal(st2["rightIdxs"], ref["state"]["rightIdxs"]) and np.array_equal(st2["close"], ref["state"]["close"])
    assert dev < pose_tol, dev
    if imu is not None:
        assert np.abs(vel - ref["vel"]).max() < 1e-8 and np.abs(bias - ref["bias"]).max() < 1e-9
    return T_cw, rep


@pytest.mark.parametrize("off,rounds,n_in,radius", [(12.0, 2, 235, 40.0), (20.0, 3, 214, 70.0)])
def test_retry_wider_radius_succeeds(oracle, capi, off, rounds, n_in, radius):
    """A prediction `off` frames old.  off = 12: the first round (10 px) fails, the second (40 px) succeeds.  off = 20: the
    radius is widened twice and the third round (70 px) succeeds; some map points leave the frame under this prediction
    (M < N).  Each failed round's matches, outlier flags and pose estimate must be reset before the next."""
    f0, f1 = 4, 5
    mp = _frame(oracle, f0)["map"]
    pred = synth.pose_at(f1 - off, synth.RIGS[RIG_NAME]["fps"])
    ref = _oracle_frame(oracle, f1, mp, pred, 7)
    assert (ref["rounds"], ref["nIn"], ref["last_radius"]) == (rounds, n_in, radius)
    if off == 20.0:
        assert (len(ref["act"]), len(mp[0])) == (627, 636)
    _gpu_frame_equals(capi, oracle, f1, mp, pred, 7, ref)


def test_retry_ends_lost(oracle, capi):
    """Map descriptors replaced by random bytes: no round reaches 50 inliers; the third round (70 px) does worse than the
    second, so the fourth falls back to the second's 40 px and the frame ends lost with 1 inlier - through the ungated
    refinement.  The solve on one inlier is poorly conditioned: measured pose deviation from the oracle on an MI355X
    4.2e-10 (tracked frames: 1e-16 .. 1e-15), inside the matcher level's 1e-9, which therefore stands."""
    f0, f1 = 4, 5
    xyz, desc, msd = _frame(oracle, f0)["map"]
    desc = np.random.default_rng(3).integers(0, 256, desc.shape, dtype=np.uint8)
    pred = synth.pose_at(f1 - 0.3, synth.RIGS[RIG_NAME]["fps"])
    ref = _oracle_frame(oracle, f1, (xyz, desc, msd), pred, 7)
    assert (ref["rounds"], ref["nIn"], ref["last_radius"]) == (4, 1, 40.0)
    _gpu_frame_equals(capi, oracle, f1, (xyz, desc, msd), pred, 7, ref)


def test_retry_empty_map_reaches_the_cap(oracle, capi):
    """No map point at all (M = 0: every launch of the rounds runs on its guard): inlier counts never fall, so the radius is
    widened after each of the four rounds and the capped fifth runs at 10 + 4 * 30."""
    f1 = 5
    mp = (np.zeros((0, 3)), np.zeros((0, 32), np.uint8), np.zeros(0, np.float32))
    pred = synth.pose_at(f1 - 0.3, synth.RIGS[RIG_NAME]["fps"])
    ref = _oracle_frame(oracle, f1, mp, pred, 7)
    assert (ref["rounds"], ref["nIn"], len(ref["act"]), ref["last_radius"]) == (5, 0, 0, 130.0)
    T_cw, rep = _gpu_frame_equals(capi, oracle, f1, mp, pred, 7, ref)
    assert np.abs(T_cw - rigid_inv(pred)).max() < 1e-12          # nothing to solve: the pose stays the prediction's


def test_first_frame_radius_needs_no_retry(oracle, capi):
    """Control: frame number 1 starts at 120 px, where the prediction that needs two rounds at 10 px succeeds at once."""
    f0, f1 = 4, 5
    mp = _frame(oracle, f0)["map"]
    pred = synth.pose_at(f1 - 12.0, synth.RIGS[RIG_NAME]["fps"])
    ref = _oracle_frame(oracle, f1, mp, pred, 1)
    assert (ref["rounds"], ref["last_radius"]) == (1, 120.0) and ref["nIn"] >= 50
    _gpu_frame_equals(capi, oracle, f1, mp, pred, 1, ref)


@pytest.mark.parametrize("off,rounds,n_in", [(12.0, 2, 248), (20.0, 3, 130)])
def test_retry_imu_bias_chained_through_rounds(oracle, capi, off, rounds, n_in):
    """Stereo + IMU: every retried solve integrates the bucket with, and pins b0 to, the bias the solve before it found."""
    f0, f1 = 9, 10
    mp = _frame(oracle, f0)["map"]
    imu = _imu_inputs(oracle, f0, f1)
    pred = synth.pose_at(f1 - off)
    ref = _oracle_frame(oracle, f1, mp, pred, 5, imu=imu)
    assert (ref["rounds"], ref["nIn"]) == (rounds, n_in)
    _gpu_frame_equals(capi, oracle, f1, mp, pred, 5, ref, imu=imu, pose_tol=1e-8)


def test_predict_compaction_across_chunks_with_outliers(oracle, capi):
    """The predict kernel's compaction beyond one 1024-point chunk (the running offset carried from chunk to chunk): the maps
    of two frames concatenated (N > 1024), every third point flagged isOutlier, every second point of the second half moved
    far behind the camera."""
    f1 = 5
    a, b = _frame(oracle, 4)["map"], _frame(oracle, 3)["map"]
    xyz = np.concatenate([a[0], b[0]]); desc = np.concatenate([a[1], b[1]]); msd = np.concatenate([a[2], b[2]])
    N, half = len(xyz), len(a[0])
    assert N > 1024 and half < 1024
    pred = synth.pose_at(f1 - 0.3, synth.RIGS[RIG_NAME]["fps"])
    xyz[half::2] = pred[:3, 3] - 50.0 * pred[:3, 2] + 0.01 * xyz[half::2]          # 50 m behind the predicted camera
    outlier = np.zeros(N, np.uint8); outlier[::3] = 1
    ref = _oracle_frame(oracle, f1, (xyz, desc, msd), pred, 7, outlier=outlier)
    act = ref["act"]
    assert not outlier[act].any() and ((act[act >= half] - half) % 2 == 1).all()
    assert (act < half).sum() > 150 and (act >= 1024).sum() > 50          # kept points on both sides of the chunk boundary
    T_cw, rep = _gpu_frame_equals(capi, oracle, f1, (xyz, desc, msd), pred, 7, ref, outlier=outlier)
    assert rep["n_inliers"] >= 50


# ---- 2. session level ----------------------------------------------------------------------------------------------------------
def _session(oracle, capi, frames, expect, use_imu=False, delay=0, pose_tol=1e-7):
    """expect: {position in `frames`: (rounds, inliers, keyframe inserted)} of the oracle's loop; every other tracked frame
    takes one round and is not lost.  Measured on an MI355X: the lost frames (7 .. 34 inliers) deviate from the oracle's
    poses by at most 1.6e-15, as the tracked ones do, so `_check` keeps its own tolerance for them."""
    ref, got, out = _run(oracle, capi, RIG_NAME, NFEAT, frames, use_imu=use_imu, delay=delay)
    for n, (f, T, Pr, Pg, lg, rep, last) in enumerate(out):
        if n == 0:
            continue
        if n in expect:
            assert (lg["rounds"], lg["nIn"], bool(lg["keyframe"])) == expect[n], (f, lg["rounds"], lg["nIn"], lg["keyframe"])
        else:
            assert lg["rounds"] == 1 and lg["nIn"] >= 50, (f, lg["rounds"], lg["nIn"])
    for (f, T, Pr, Pg, lg, rep, last) in out:
        print("frame %3d  rounds %d  inliers %3d  keyframe %d  pose deviation %.3e" %
              (f, lg.get("rounds", 0), lg["nIn"], lg["keyframe"], np.abs(Pg - Pr).max()))
    _check(ref, got, out, pose_tol=pose_tol)
    return out


NEAR = [0, 1, 2, 16, 17, 18, 19, 20]
FAR = [0, 2, 4, 60, 62, 64, 66, 68]
BACK = [0, 2, 20, 2, 4, 6, 8]


def test_session_retried_frames_with_and_without_keyframe(oracle, capi):
    """A jump of 14 frames: frame 16 needs two rounds and inserts nothing, frame 17 needs two rounds and inserts a keyframe."""
    _session(oracle, capi, NEAR, {3: (2, 184, False), 4: (2, 218, True)})


def test_session_lost_frame_inserts_keyframe_and_recovers(oracle, capi):
    """A jump of 56 frames: frame 60 ends lost after four rounds (14 inliers) and inserts a keyframe; the session tracks on
    from that keyframe's points."""
    out = _session(oracle, capi, FAR, {3: (4, 14, True), 4: (1, 85, True)})
    assert [o[4]["nIn"] for o in out[5:]] == [205, 194, 132]


@pytest.mark.parametrize("delay,lost", [(0, (24, 20, 27, 32)), (4, (24, 20, 26, 34))])
def test_session_stays_lost_like_the_oracle(oracle, capi, delay, lost):
    """Forth and back: after frame 20 (three rounds) the schedule returns to frame 2 and the session stays lost for four
    frames in a row, each after three rounds, each inserting a keyframe - frame by frame as the oracle's loop.
    delay = 4: the timed mode (new points of the passes handed over while lost arrive a frame later)."""
    expect = {2: (3, 143, True)}
    expect.update({3 + k: (3, n_in, True) for k, n_in in enumerate(lost)})
    _session(oracle, capi, BACK, expect, delay=delay)


def test_session_imu_lost_then_saved_on_the_capped_round(oracle, capi):
    """Stereo + IMU over the jump of 56 frames (a bucket of 559 samples): frame 60 ends lost after three rounds, frame 62
    succeeds on the capped fifth round; the bias is chained through every one of those solves."""
    _session(oracle, capi, FAR, {3: (3, 7, True), 4: (5, 119, True)}, use_imu=True, pose_tol=1e-6)


def test_session_imu_retried_frames(oracle, capi):
    """Stereo + IMU over the jump of 14 frames (a bucket of 139 samples): frames 16 and 17 need two rounds each."""
    frames = NEAR[:6]
    assert 10 * (frames[3] - frames[2]) - 1 == 139
    ref, got, out = _run(oracle, capi, RIG_NAME, NFEAT, frames, use_imu=True)
    assert [o[4]["rounds"] for o in out[1:]] == [1, 1, 2, 2, 1]
    _check(ref, got, out, pose_tol=1e-6)


# ---- 3. batch and fleet --------------------------------------------------------------------------------------------------------
SCHEDULES = [list(range(0, 16, 2)), NEAR, FAR]
STARTS = [0, 0, 1]
_SINGLES = {}


def _singles(capi, use_imu, mapping, delay, np_delay):
    """the single sessions of the three schedules (one run per mode, shared by the batch tests); asserts that they contain
    what the comparison is about: retried frames in lanes 1 and 2, at least one of them inserting a keyframe"""
    key = (use_imu, mapping, delay, np_delay)
    if key not in _SINGLES:
        _SINGLES[key] = [_single(capi, RIG_NAME, NFEAT, sc, use_imu, mapping, delay, np_delay) for sc in SCHEDULES]
    one = _SINGLES[key]
    rounds = [[r["rounds"] for (_, r, _) in o[0][1:]] for o in one]
    assert max(rounds[0]) == 1 and max(rounds[1]) > 1 and max(rounds[2]) > 1, rounds
    assert any(r["rounds"] > 1 and r["keyframe_inserted"] for o in one[1:] for (_, r, _) in o[0][1:])
    # steps on which a lane retries beside a lane that tracks in one round
    per_step = {}
    for b, o in enumerate(one):
        for n, (_, r, _) in enumerate(o[0]):
            if n > 0:
                per_step.setdefault(STARTS[b] + n, []).append(r["rounds"])
    assert sum(1 for v in per_step.values() if max(v) > 1 and min(v) == 1) >= 2, per_step
    return one


@pytest.mark.parametrize("use_imu,mapping,delay,np_delay", [(False, 1, 0, 1), (False, 2, 4, 2), (True, 1, 0, 1)])
def test_batch_retried_lane_equals_single_session(capi, use_imu, mapping, delay, np_delay):
    """Three lanes in lockstep: one that never retries, two whose jumps make them retry (and insert keyframes while retrying:
    the packed keys of those steps are dropped) on steps where the other lanes do not."""
    one = _singles(capi, use_imu, mapping, delay, np_delay)
    lanes = _batched(capi, RIG_NAME, NFEAT, SCHEDULES, STARTS, use_imu, mapping, delay, np_delay)
    for b in range(len(SCHEDULES)):
        _same(one[b], lanes[b])


def test_batch_retried_lane_with_prefetch_equals_single_session(capi):
    """The same lanes on device-resident images through track_prefetch: a retried lane's rounds are launched after the next
    step's extraction has been enqueued on the extractor's other output set."""
    rig = synth.RIGS[RIG_NAME]
    one = _singles(capi, False, 1, 0, 1)
    B = len(SCHEDULES)
    nSteps = max(STARTS[b] + len(SCHEDULES[b]) for b in range(B))
    dev, masks, fnums = {}, [], []
    for step in range(nSteps):
        fn = [step - STARTS[b] for b in range(B)]
        mask = [int(0 <= fn[b] < len(SCHEDULES[b])) for b in range(B)]
        for b in range(B):
            if mask[b]:
                L, R, _ = synth.stereo_frame(SCHEDULES[b][fn[b]], RIG_NAME)
                dev[(step, b)] = (capi.DeviceImage(np.ascontiguousarray(L)), capi.DeviceImage(np.ascontiguousarray(R)))
        masks.append(mask); fnums.append([max(n, 0) if m else 0 for n, m in zip(fn, mask)])
    bt = capi.Batch(rig, NFEAT, B, T0s=[synth.pose_at(sc[0], rig["fps"]) for sc in SCHEDULES], local_mapping=1, host_threads=3)
    out = [[] for _ in range(B)]
    for step in range(nSteps):
        mask = masks[step]
        Ls = [dev[(step, b)][0].ptr if mask[b] else None for b in range(B)]
        Rs = [dev[(step, b)][1].ptr if mask[b] else None for b in range(B)]
        nL = nR = nmask = None
        if step + 1 < nSteps:
            nmask = masks[step + 1]
            nL = [dev[(step + 1, b)][0].ptr if nmask[b] else None for b in range(B)]
            nR = [dev[(step + 1, b)][1].ptr if nmask[b] else None for b in range(B)]
        T, reps = bt.track_prefetch(Ls, Rs, fnums[step], nL, nR, mask=mask, next_mask=nmask, stride=rig["w"])
        for b in range(B):
            if mask[b]:
                out[b].append((T[b].copy(), reps[b], bt.system(b).last_frame() if fnums[step][b] > 0 else None))
    lanes = [(out[b], bt.system(b).counts(), bt.system(b).keyframes()) for b in range(B)]
    bt.close()
    for d in dev.values():
        d[0].free(); d[1].free()
    for b in range(B):
        _same(one[b], lanes[b])


def test_fleet_groupings_agree_on_retried_and_lost_frames(capi):
    """vslam_fleet on a device-resident frame list with a jump of 56 frames, replayed as a ping-pong by 5 sessions that start
    at different phases: unbatched, two lockstep groups (3 + 2) and one group of 5 (whose driver prefetches the next frames'
    extraction) must report the same run - including the rounds spent retrying and the frames that ended lost."""
    rig = synth.RIGS[RIG_NAME]
    src = [0, 2, 4, 60, 62, 64, 66, 68, 70, 72]
    frames = [synth.stereo_frame(f, RIG_NAME) for f in src]
    imgs = [(capi.DeviceImage(f[0]), capi.DeviceImage(f[1])) for f in frames]
    poses = np.stack([f[2] for f in frames])
    cfg = capi.system_config(rig, NFEAT, local_mapping=1)
    out = []
    for lanes in (0, 3, 5):
        fl = capi.Fleet(cfg, 5, [a.ptr for a, _ in imgs], [b.ptr for _, b in imgs], rig["w"], True, poses=poses, lanes=lanes)
        r1 = fl.run(6)
        r2 = fl.run(4)                 # a second job continues the sequences (and the prefetch chain)
        fl.close()
        out.append((r1, r2))
    for a, b in imgs:
        a.free(); b.free()
    print({k: (out[0][0][k], out[0][1][k]) for k in ("frames", "keyframes", "sum_inliers", "min_inliers", "lost_frames", "sum_rounds")})
    assert out[0][0]["frames"] == 30 and out[0][1]["frames"] == 20
    assert out[0][0]["sum_rounds"] > out[0][0]["frames"] and out[0][0]["lost_frames"] >= 1
    for k in ("frames", "keyframes", "sum_inliers", "min_inliers", "lost_frames", "sum_rounds"):
        for j in (1, 2):
            assert out[j][0][k] == out[0][0][k] and out[j][1][k] == out[0][1][k], (k, j, out[j][0][k], out[0][0][k], out[j][1][k], out[0][1][k])
