"""A lane per robot: the lanes of a vslam_batch have their own cameras (rig intrinsics / baseline) and their own start and end
(vslam_batch_restart_lane).  Yardstick: the single-session path - capi.System with that lane's rig on that lane's frames (itself
pinned to the restated loop by tests/test_gpu_system.py); comparison: the one test_gpu_batch._same makes (every integer report field,
match tables, counts, keyframe lists, poses to 1e-9 - the allowance for the local BA's LDS-atomic summation order).  Each lane's
frames are rendered with that lane's own rig."""
import os
import numpy as np
import pytest
import synth
from test_gpu_batch import _same, _single, _velocity, _bucket, G, NOISE, INT_KEYS

pytestmark = pytest.mark.gpu

# the second camera: other focal length, principal point and baseline (close = depth <= 40 x baseline: 6.4 m against 4.4 m)
synth.RIGS["euroc_b"] = dict(synth.RIGS["euroc"], fx=458.0, fy=458.0, cx=360.0, cy=248.0, bl=0.16)
A, B = "euroc", "euroc_b"
NFEAT = 1500
S0, S1, S2 = list(range(0, 60, 2)), list(range(6, 66, 2)), list(range(12, 64, 2))      # (test_batch_lanes_equal_single_sessions' schedules)
FPS = synth.RIGS[A]["fps"]

_REFS = {}


def _ref(capi, rig_name, frames, use_imu, mapping, delay, np_delay):
    """the single session of (rig, schedule, mode): computed once, shared by the tests, never modified"""
    key = (rig_name, tuple(frames), use_imu, mapping, delay, np_delay)
    if key not in _REFS:
        synth.prerender(frames, rig_name)
        _REFS[key] = _single(capi, rig_name, NFEAT, frames, use_imu, mapping, delay, np_delay)
    return _REFS[key]


def _totals(ref):
    return sum(r["keyframe_inserted"] for _, r, _ in ref[0]), sum(r["mapping_ran"] for _, r, _ in ref[0])


def _drive(capi, lanes, use_imu, mapping, delay, np_delay, before_step=None):
    """lanes[b] = dict(start=step, segments=[(rig name, source frames), ...]): segment k > 0 begins the step after segment k - 1
    ended, in a new session made by restart_lane.  Returns res[b][k] = (per-frame (pose, report, last_frame), counts, keyframes)
    read when the segment ended, and mem[b][k] = (memory() at the segment's end, memory() right after the restart that followed).
    before_step(bt, step) runs between two steps."""
    nB = len(lanes)
    imu = dict(gravity=G, noise=NOISE, T_bs=synth.T_BC1, hz=200) if use_imu else None
    first = [ln["segments"][0] for ln in lanes]
    for ln in lanes:
        for rn, fr in ln["segments"]:
            synth.prerender(fr, rn)
    bt = capi.Batch(None, NFEAT, nB, rigs=[synth.RIGS[rn] for rn, _ in first], T0s=[synth.pose_at(fr[0], FPS) for _, fr in first], imu=imu,
                    velocities=[_velocity(fr[0], FPS) for _, fr in first] if use_imu else None, local_mapping=mapping, host_threads=3,
                    mapping_delay=delay, mapping_np_delay=np_delay)
    # (lane, segment, n) of every step
    plan = []
    for ln in lanes:
        p = [None] * ln["start"]
        for k, (_, fr) in enumerate(ln["segments"]):
            p += [(k, n) for n in range(len(fr))]
        plan.append(p)
    nSteps = max(len(p) for p in plan)
    res = [[[[], None, None] for _ in ln["segments"]] for ln in lanes]
    mem = [[[None, None] for _ in ln["segments"]] for ln in lanes]
    for step in range(nSteps):
        if before_step is not None:
            before_step(bt, step)
        Ls, Rs, fn, bk, mask = [None] * nB, [None] * nB, [0] * nB, [None] * nB, [0] * nB
        cur = [None] * nB
        for b in range(nB):
            at = plan[b][step] if step < len(plan[b]) else None
            if at is None:
                continue
            k, n = at
            rn, fr = lanes[b]["segments"][k]
            if k > 0 and n == 0:
                if k % 2 == 1 and (rn, fr) == lanes[b]["segments"][0] == lanes[b]["segments"][k - 1]:
                    bt.restart_lane(b)           # (the lane's previous configuration: config = NULL)
                else:
                    bt.restart_lane(b, rig=synth.RIGS[rn], T0=synth.pose_at(fr[0], FPS), velocity=_velocity(fr[0], FPS) if use_imu else None)
                mem[b][k - 1][1] = bt.memory()
            Ls[b], Rs[b], _ = synth.stereo_frame(fr[n], rn)
            fn[b] = n; mask[b] = 1; cur[b] = (k, n, len(fr))
            if use_imu and n > 0:
                bk[b] = _bucket(fr[n - 1], fr[n], FPS)
        T, reps = bt.track(Ls, Rs, fn, imu_buckets=bk if use_imu else None, mask=mask)
        for b in range(nB):
            if cur[b] is None:
                continue
            k, n, nf = cur[b]
            res[b][k][0].append((T[b].copy(), reps[b], bt.system(b).last_frame() if n > 0 else None))
            if n == nf - 1:
                res[b][k][1], res[b][k][2] = bt.system(b).counts(), bt.system(b).keyframes()
                mem[b][k][0] = bt.memory()
    bt.close()
    return [[tuple(s) for s in r] for r in res], mem


# ---- 1. mixed rigs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_imu,mapping,delay,np_delay", [(False, 1, 0, 1), (True, 2, 4, 2)])
def test_mixed_rig_lanes_equal_single_sessions(capi, use_imu, mapping, delay, np_delay):
    """Lanes with rigs [B, A, B] (the odd rig at lane 0 and at a later lane: a leak of lane 0's rig shows in either direction), 30
    frames each, one lane joining at step 3: every lane equals the single session of ITS rig on ITS frames - through the merged depth
    / close refresh of the lanes' local BAs (one launch for the pairs of all lanes, close threshold per keyframe) and, in mapping
    mode 2, through the engine's cohorts that mix the lanes' problems.  Before the feature Batch(...) refuses the configs."""
    mode = (use_imu, mapping, delay, np_delay)
    ra, rb = _ref(capi, A, S1, *mode), _ref(capi, B, S1, *mode)
    # the same schedule under the two rigs must differ in what the tracker counts, and both runs must reach the local BA's write-back:
    # otherwise this test could not tell a lane that runs on the wrong rig
    diff = [(n, k, r1[k], r2[k]) for n, ((_, r1, _), (_, r2, _)) in enumerate(zip(ra[0], rb[0])) for k in INT_KEYS if r1[k] != r2[k]]
    print("rig A / rig B on one schedule: %d differing integer report fields, first %s; keyframes / local BAs: A %s, B %s"
          % (len(diff), diff[:3], _totals(ra), _totals(rb)))
    assert diff
    for r in (ra, rb):
        nKF, nBA = _totals(r)
        assert nKF >= 4 and nBA >= 1, (nKF, nBA)
    rigs, scheds, starts = [B, A, B], [S0, S1, S2], [0, 0, 3]
    res, _ = _drive(capi, [dict(start=st, segments=[(rn, sc)]) for rn, sc, st in zip(rigs, scheds, starts)], *mode)
    for b in range(3):
        nKF, nBA = _same(_ref(capi, rigs[b], scheds[b], *mode), res[b][0])
        print("lane %d (%s): %d keyframes, %d local BAs compared" % (b, rigs[b], nKF, nBA))
        # a lane of each rig went through a local BA's write-back (lane 2 joins late on a shorter schedule and need not reach one)
        assert nKF >= 4 and (nBA >= 1 or b == 2)


def test_mixed_rig_lanes_through_the_capacity_fallback(capi):
    """The same mixed-rig batch (mapping on the engine, IMU) with the arena form of the merged refresh refused
    (VSLAM_REFRESH_FORCE_CAPACITY: as if the pinned arena had no room): serve_requests then serves the lanes' pairs through the
    synchronous form with the same per-keyframe thresholds, and every lane still equals its single session."""
    mode = (True, 2, 4, 2)
    rigs, scheds, starts = [B, A, B], [S0, S1, S2], [0, 0, 3]
    os.environ["VSLAM_REFRESH_FORCE_CAPACITY"] = "1"
    try:
        res, _ = _drive(capi, [dict(start=st, segments=[(rn, sc)]) for rn, sc, st in zip(rigs, scheds, starts)], *mode)
    finally:
        del os.environ["VSLAM_REFRESH_FORCE_CAPACITY"]
    nBA = [_same(_ref(capi, rigs[b], scheds[b], *mode), res[b][0])[1] for b in range(3)]
    assert nBA[0] >= 1 and nBA[1] >= 1, nBA


# ---- 2. the merged refresh in isolation ---------------------------------------------------------------------------------------
def _refresh_request(bl, seed):
    """2 keyframes, 10 landmarks each seen by both (20 pairs): depths on both sides of 40 x 0.11 and 40 x 0.16, some exactly on a
    threshold (keyframe 0 is the identity, so its depth IS the landmark's z)"""
    rng = np.random.default_rng(seed)
    thA, thB = np.float32(0.11) * np.float32(40), np.float32(0.16) * np.float32(40)
    z = np.array([1.0, 4.3, float(thA), np.nextafter(np.float64(thA), 10.0), 5.0, 6.3, float(thB), np.nextafter(np.float64(thB), 10.0), 7.0, 20.0])
    lm = np.stack([rng.uniform(-1, 1, 10), rng.uniform(-0.5, 0.5, 10), z], axis=1)
    T1 = np.eye(4)
    a = 0.01 * (1 + seed % 3)
    T1[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    T1[:3, 3] = [0.2, 0.01, -0.03]
    poses = np.stack([np.eye(4), T1])
    pk = np.repeat([0, 1], 10).astype(np.int32); pl = np.tile(np.arange(10), 2).astype(np.int32)
    pw = np.zeros(20, np.uint8); pw[[3, 17]] = 1
    lo = np.zeros(10, np.uint8); lo[8] = 1
    cd = rng.uniform(0.5, 9.0, 20).astype(np.float32); cd[5] = -1.0; cd[12] = 0.0
    return dict(rig=dict(synth.RIGS[A], bl=bl), poses=poses, lm=lm, lo=lo, pk=pk, pl=pl, pw=pw, cd=cd)


def _merge(reqs):
    ak = al = 0
    pk, pl = [], []
    for q in reqs:
        pk.append(q["pk"] + ak); pl.append(q["pl"] + al)
        ak += len(q["poses"]); al += len(q["lm"])
    cat = lambda k: np.concatenate([q[k] for q in reqs])
    return cat("poses"), cat("lm"), cat("lo"), np.concatenate(pk), np.concatenate(pl), cat("pw"), cat("cd")


@pytest.mark.parametrize("fallback", [False, True])
def test_merged_refresh_equals_per_request_calls(capi, fallback):
    if fallback:      # (the synchronous per-keyframe form behind the arena form: the group's capacity fallback)
        os.environ["VSLAM_REFRESH_FORCE_CAPACITY"] = "1"
    try:
        _merged_refresh_cases(capi)
    finally:
        os.environ.pop("VSLAM_REFRESH_FORCE_CAPACITY", None)


def _merged_refresh_cases(capi):
    """k_ba_refresh_depth on two requests of different cameras staged together (the form the lockstep group's serve_requests
    launches; close threshold read per keyframe) against vslam_ba_refresh_depth once per request with its own rig: depth, close and
    updated byte for byte.  With equal rigs the merged form equals the one-rig call on the same merged arrays (what a shared-rig
    group launched before)."""
    for bls in ((0.11, 0.16), (0.16, 0.11)):
        reqs = [_refresh_request(bls[0], 1), _refresh_request(bls[1], 2)]
        one = [capi.ba_refresh_depth(q["rig"], q["poses"], q["lm"], q["lo"], q["pk"], q["pl"], q["pw"], q["cd"]) for q in reqs]
        d, c, u = capi.ba_refresh_depth_merged([q["rig"] for q in reqs], [2, 2], *_merge(reqs))
        assert len(d) == 40
        for i, name in enumerate(("depth", "close", "updated")):
            want = np.concatenate([o[i] for o in one])
            got = (d, c, u)[i]
            assert want.tobytes() == got.tobytes(), (bls, name, np.nonzero(want != got)[0])
        # the inputs do tell the cameras apart: identity keyframe, landmark 4 at 5.0 m and landmark 6 exactly on 40 x 0.16
        for r, bl in enumerate(bls):
            cl = c[20 * r: 20 * r + 20]
            assert u[20 * r + 4] == 1 and cl[4] == (1 if bl == 0.16 else 0)
            assert cl[2] == 1 and cl[1] == 1 and cl[9] == 0                   # on 40 x 0.11 / below it / far: the same for both
            assert cl[6] == (1 if bl == 0.16 else 0) and cl[7] == 0           # exactly on 40 x 0.16; one ulp beyond it
            assert u[20 * r + 3] == 0 and u[20 * r + 5] == 0 and u[20 * r + 8] == 0 and u[20 * r + 12] == 0 and u[20 * r + 17] == 0
    for bl in (0.11, 0.16):
        reqs = [_refresh_request(bl, 1), _refresh_request(bl, 2)]
        m = _merge(reqs)
        want = capi.ba_refresh_depth(reqs[0]["rig"], *m)
        got = capi.ba_refresh_depth_merged([q["rig"] for q in reqs], [2, 2], *m)
        for w, g in zip(want, got):
            assert w.tobytes() == g.tobytes(), bl


# ---- 3. restart ----------------------------------------------------------------------------------------------------------------
MODE2 = (False, 2, 3, 1)


def _restart_point(ref):
    """the step right after the first report with a keyframe insertion that made it the session's fourth (or later) keyframe: a
    mapping job of the lane is in flight or queued then"""
    for n, (_, r, _) in enumerate(ref[0]):
        if r["keyframe_inserted"] and r["n_keyframes"] >= 4:
            return n + 1
    raise AssertionError("the reference run never inserts a fourth keyframe")


def test_restart_lane_mid_run(capi):
    """Two lanes, mapping on the engine (mode 2, delay 3).  Lane 0 runs its 30 frames uninterrupted; lane 1 runs S1 under rig A up to
    the step after a keyframe insertion (its new-point search is then queued or running), is restarted onto rig B at the pose of
    S2[0], and runs S2 from frame number 0.  Lane 0 equals System(A, S0) over the whole run, lane 1 before the restart the prefix of
    System(A, S1), after it System(B, S2) from its frame 0 - counts and keyframes included: nothing of the first generation is left."""
    r0, r1, r2 = _ref(capi, A, S0, *MODE2), _ref(capi, A, S1, *MODE2), _ref(capi, B, S2, *MODE2)
    cut = _restart_point(r1)
    print("restart of lane 1 before its step %d (of %d)" % (cut, len(S1)))
    assert 4 <= cut < len(S1)
    res, mem = _drive(capi, [dict(start=0, segments=[(A, S0)]), dict(start=0, segments=[(A, S1[:cut]), (B, S2)])], *MODE2)
    _same(r0, res[0][0])
    gen1 = res[1][0]
    assert len(gen1[0]) == cut
    _same((r1[0][:cut], gen1[1], gen1[2]), gen1)            # (per-frame part against the prefix; counts / keyframes are end-of-run read-outs)
    assert gen1[1]["frames"] == cut and gen1[1]["keyframes"] >= 4
    nKF, _ = _same(r2, res[1][1])
    assert nKF >= 2
    assert mem[1][0][1]["slabs_free"] > 0


# ---- 4. bounded memory, no stale state --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [MODE2, (True, 2, 4, 2)])
def test_restart_same_sequence_is_identical_and_bounded(capi, mode):
    """Lane 1 is restarted three times onto the SAME sequence and rig (lane 0 keeps running): the generations' reports are identical
    in every integer field and their poses agree to 1e-9 (each equals the single session), every generation inserts keyframes with
    local mapping on, the key slabs a generation hands back are the next one's - no growth of key_slab_bytes from the end of
    generation 2 to the end of generation 3 - and the free list is not empty right after a restart."""
    r1 = _ref(capi, A, S1, *mode)
    # a generation: up to two frames after the second keyframe insertion that follows the map's initialisation
    ins = [n for n, (_, r, _) in enumerate(r1[0]) if n > 0 and r["keyframe_inserted"]]
    assert len(ins) >= 2
    gl = min(ins[1] + 3, len(S1))
    gen = S1[:gl]
    print("generation: %d frames, keyframe insertions at %s" % (gl, ins[:2]))
    n0 = min(len(S0), 4 * gl)
    res, mem = _drive(capi, [dict(start=0, segments=[(A, S0[:n0])]), dict(start=0, segments=[(A, gen)] * 4)], *mode)
    _same((_ref(capi, A, S0, *mode)[0][:n0], res[0][0][1], res[0][0][2]), res[0][0])      # (the lane beside the restarts is not touched by them)
    g = res[1]
    for k in range(4):
        _same((r1[0][:gl], g[k][1], g[k][2]), g[k])                          # every generation = the prefix of the single session
        assert sum(r["keyframe_inserted"] for _, r, _ in g[k][0][1:]) >= 2
        assert g[k][1]["keyframes"] >= 3 and g[k][1]["frames"] == gl
    for k in range(1, 4):
        _same(g[0], g[k])                                                    # ... and the generations equal one another, read-outs included
    for k in range(3):
        print("generation %d: end %s, after restart %s" % (k + 1, mem[1][k][0], mem[1][k][1]))
        assert mem[1][k][1]["slabs_free"] > 0
    assert mem[1][1][0]["key_slab_bytes"] > 0
    assert mem[1][2][0]["key_slab_bytes"] == mem[1][1][0]["key_slab_bytes"]
    assert mem[1][3][0]["key_slab_bytes"] == mem[1][1][0]["key_slab_bytes"]


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------
def test_refused_restarts_leave_the_lane_alone(capi):
    """restart_lane with another image width, another n_features, the other IMU mode, another mapping_delay or a lane out of range
    is VSLAM_ERR_INVALID and the lane continues: it still equals its single session.  After a restart the first frame must carry
    frame number 0 (anything else: VSLAM_ERR_INVALID, nothing tracked), and raw frames need the lane's rectifiers bound again."""
    rigA = synth.RIGS[A]
    imu = dict(gravity=G, noise=NOISE, T_bs=synth.T_BC1, hz=200)
    bad = [dict(lane=1, rig=dict(rigA, w=rigA["w"] + 8)), dict(lane=1, nfeatures=NFEAT - 300), dict(lane=1, imu=imu), dict(lane=1, mapping_delay=2),
           dict(lane=2), dict(lane=-1)]
    seen = []

    def poke(bt, step):
        if step not in (2, 9):
            return
        for kw in bad:
            kw = dict(kw)
            lane = kw.pop("lane")
            with pytest.raises(capi.VslamError) as e:
                bt.restart_lane(lane, T0=synth.pose_at(40, FPS), **kw)
            assert e.value.status == capi.ERR_INVALID, (kw, e.value)
            seen.append(step)

    sc0, sc1 = S0[:16], S1[:16]
    res, _ = _drive(capi, [dict(start=0, segments=[(A, sc0)]), dict(start=0, segments=[(A, sc1)])], *MODE2, before_step=poke)
    assert len(seen) == 2 * len(bad)
    for b, (sc, full) in enumerate(((sc0, S0), (sc1, S1))):
        r = _ref(capi, A, full, *MODE2)
        nKF, _ = _same((r[0][:16], res[b][0][1], res[b][0][2]), res[b][0])
        assert nKF >= 2 and res[b][0][1]["frames"] == 16

    # frame number and rectifiers after a restart
    K = [[rigA["fx"], 0, rigA["cx"]], [0, rigA["fy"], rigA["cy"]], [0, 0, 1]]
    size = (rigA["w"], rigA["h"])
    rects = [capi.Rectifier(K, None, None, K, size, size) for _ in range(2)]
    bt = capi.Batch(rigA, NFEAT, 2, T0s=[synth.pose_at(sc[0], FPS) for sc in (S0, S1)], local_mapping=2, host_threads=2, mapping_delay=3,
                    mapping_np_delay=1)
    bt.set_rectifiers(-1, *rects)
    fr = [[synth.stereo_frame(sc[n], A) for n in range(3)] for sc in (S0, S1)]
    for n in range(2):
        bt.track([fr[0][n][0], fr[1][n][0]], [fr[0][n][1], fr[1][n][1]], [n, n], raw=(n == 1))      # (raw works while the rectifiers are bound)
    before = bt.system(0).counts()
    bt.restart_lane(1, T0=synth.pose_at(S1[0], FPS))
    assert bt.system(1).counts()["frames"] == 0 and bt.system(1).counts()["keyframes"] == 0
    with pytest.raises(capi.VslamError) as e:
        bt.track([fr[0][2][0], fr[1][2][0]], [fr[0][2][1], fr[1][2][1]], [2, 2])
    assert e.value.status == capi.ERR_INVALID
    assert bt.system(0).counts() == before and bt.system(1).counts()["frames"] == 0                  # nothing tracked, on either lane
    with pytest.raises(capi.VslamError) as e:
        bt.track([None, fr[1][0][0]], [None, fr[1][0][1]], [0, 0], mask=[0, 1], raw=True)
    assert e.value.status == capi.ERR_INVALID and bt.system(1).counts()["frames"] == 0
    bt.set_rectifiers(1, *rects)
    T, reps = bt.track([fr[0][2][0], fr[1][0][0]], [fr[0][2][1], fr[1][0][1]], [2, 0], raw=True)
    assert bt.system(1).counts()["frames"] == 1 and bt.system(1).counts()["keyframes"] == 1 and bt.system(0).counts()["frames"] == 3
    assert np.abs(T[1] - synth.pose_at(S1[0], FPS)).max() < 1e-9
    bt.close()
    for r in rects:
        r.close()


# ---- 6. the local-BA cohort of lanes with different cameras -----------------------------------------------------------------------
def test_mixed_rig_cohort_stays_batched(capi, oracle):
    """vslam_local_ba_batch on four tracker windows of two cameras, the odd one first: all four are planned into the batched launches
    (no problem runs on its own because its rig differs from problem 0's) and every lane equals its own vslam_local_ba call, by the
    bar of test_ba_batch_equals_single_calls.  The result does depend on the rig: a lane solved with the other camera differs."""
    from test_gpu_ba import _check_batch_lane
    ex = oracle.Extractor(1500)
    names = [B, A, B, A]
    probs = [synth.make_ba_problem(rig_name=nm, n_local=5 + i, n_fixed=2, n_lm=500 + 100 * i, seed=900 + i, outlier_frac=0.03) for i, nm in enumerate(names)]
    rigs = [synth.RIGS[nm] for nm in names]
    batch = capi.local_ba_batch(rigs, ex.sigmaFactor, ex.InvSigmaFactor, probs)
    plan = capi.local_ba_last_batch_plan()
    assert plan["status"] == 0 and (plan["n_batch"], plan["n_single"]) == (4, 0), plan
    for i, p in enumerate(probs):
        _check_batch_lane(capi.local_ba(rigs[i], ex.sigmaFactor, ex.InvSigmaFactor, p), batch[i], (i, names[i]))
    other = capi.local_ba(rigs[0], ex.sigmaFactor, ex.InvSigmaFactor, probs[1])
    assert np.abs(other["kf_pose"] - batch[1]["kf_pose"]).max() > 1e-6
