"""vslam_batch_relocalize_imu: lost lanes of a stereo + IMU lockstep group recover pose and velocity in two calls (DESIGN.md
section 6 item 23).  Yardstick: capi.System sessions driven alone through the same calls on the same frames (that path is pinned to
the CPU restatement by tests/test_gpu_reloc_imu.py).  Comparison: the one test_gpu_batch._same makes for the tracked frames
(integer report fields, match tables, counts and keyframe lists exactly, poses to 1e-9 - the allowance for the local BA's LDS-atomic
summation order); for the relocalisation calls the report integers and the phase equal, poses, velocities and dt to 1e-9."""
import numpy as np
import pytest
import synth
from test_gpu_batch import _same, _velocity, _bucket, G, NOISE

pytestmark = pytest.mark.gpu

RIG_NAME = "euroc"
RIG = synth.RIGS[RIG_NAME]
FPS = RIG["fps"]
NFEAT = 1500
IMU = dict(gravity=G, noise=NOISE, T_bs=synth.T_BC1, hz=200)
START = [0, 6, 12]                               # the lanes' first source frames (one rig: the lanes differ in T0); steps of 2
NTRACK = 6
REL_INT = ("success", "n_points", "n_pairs", "best_hypothesis", "best_count", "n_inliers", "n_stereo")


def _foreign(f):
    return synth.stereo_frame(f, RIG_NAME, scene_seed=9, tex_seed=0xBEEF)[:2]


def _script(b):
    """the calls of lane b after its NTRACK tracked frames (source frames START[b] + 2 n), as (kind, source frame, bucket's first
    source frame or None, foreign):
      lanes 0 and 2: first pose on their source frame START + 4; lane 1 is tracked meanwhile;
      lane 0: second pose on START + 6 with the bucket since START + 4; lane 2: a foreign frame as the second pose (fails: the flag drops);
      then two tracked steps of every lane - lane 0 from its second pose, lane 2 from its first (its velocity is the stale one)."""
    s = START[b]
    if b == 1:
        return [("track", s + 12, s + 10, False), ("track", s + 14, s + 12, False), ("track", s + 16, s + 14, False)]
    if b == 0:
        return [("reloc", s + 4, None, False), ("reloc", s + 6, s + 4, False), ("track", s + 8, s + 6, False), ("track", s + 10, s + 8, False)]
    return [("reloc", s + 4, None, False), ("reloc", s + 6, s + 4, True), ("track", s + 6, s + 4, False), ("track", s + 8, s + 6, False)]


# the call sequence, as lane masks: first poses of lanes 0 and 2 | lane 1 tracked | second poses of lanes 0 and 2 | two steps of all
CALLS = [("reloc", [1, 0, 1]), ("track", [0, 1, 0]), ("reloc", [1, 0, 1]), ("track", [1, 1, 1]), ("track", [1, 1, 1])]


def _lane_calls(b):
    """lane b's own entries of CALLS, in order: (call index, kind, source frame, bucket start, foreign)"""
    sc = _script(b)
    idx = [i for i, (_, mask) in enumerate(CALLS) if mask[b]]
    assert len(sc) == len(idx) and all(CALLS[i][0] == c[0] for i, c in zip(idx, sc)), (b, sc, idx)
    return [(i,) + c for i, c in zip(idx, sc)]


def _images(src, foreign):
    return _foreign(src) if foreign else synth.stereo_frame(src, RIG_NAME)[:2]


def _single(capi, b):
    s = capi.System(RIG, NFEAT, T0=synth.pose_at(START[b], FPS), imu=dict(IMU, velocity=_velocity(START[b], FPS)), local_mapping=1)
    out, rel = [], {}
    for n in range(NTRACK):
        f = START[b] + 2 * n
        L, R, _ = synth.stereo_frame(f, RIG_NAME)
        P, rep = s.track(L, R, n, imu_bucket=_bucket(f - 2, f, FPS) if n else None)
        out.append((P, rep, s.last_frame() if n > 0 else None))
    fn = NTRACK
    for (i, kind, src, b0, foreign) in _lane_calls(b):
        L, R = _images(src, foreign)
        bk = _bucket(b0, src, FPS) if b0 is not None else None
        if kind == "track":
            P, rep = s.track(L, R, fn, imu_bucket=bk)
            out.append((P, rep, s.last_frame()))
        else:
            T, rrep, irep = s.relocalize_imu(L, R, fn, imu_bucket=bk)
            rel[i] = (T, rrep, irep, s.counts(), s.imu_state())
        fn += 1
    res = (out, s.counts(), s.keyframes(), rel)
    s.close()
    return res


def _same_reloc(one, lane, what):
    (T1, r1, i1, c1, s1), (T2, r2, i2, c2, s2) = one, lane
    for k in REL_INT:
        assert r1[k] == r2[k], (what, k, r1[k], r2[k])
    assert i1["phase"] == i2["phase"], what
    assert np.abs(T1 - T2).max() <= 1e-9, what
    for k in ("velocity_prev", "velocity", "bias"):
        assert np.abs(i1[k] - i2[k]).max() <= 1e-9, (what, k)
    assert abs(i1["dt"] - i2["dt"]) <= 1e-12 and abs(i1["rot_residual"] - i2["rot_residual"]) <= 1e-9, what
    assert c1 == c2, what
    assert s1["pending"] == s2["pending"], what
    for k in ("velocity", "bias", "bias_good"):
        assert np.abs(s1[k] - s2[k]).max() <= 1e-9, (what, k)


def test_imu_lanes_relocalise_in_two_calls(capi):
    """Three IMU lanes of one rig started at source frames 0, 6 and 12, six tracked frames each, then the calls of CALLS.  Also: the
    idle lane's row, report and session are untouched by a call; a tracked step with a pending lane active fails, names the lane,
    and leaves the other lanes' next step equal to their single sessions."""
    synth.prerender(sorted({START[b] + 2 * n for b in range(3) for n in range(NTRACK + 3)}), RIG_NAME)
    singles = [_single(capi, b) for b in range(3)]
    # the single-session side first: the script does what its docstring says
    assert [singles[0][3][i][2]["phase"] for i in (0, 2)] == [1, 2]
    assert [singles[2][3][i][2]["phase"] for i in (0, 2)] == [1, 0] and singles[2][3][2][1]["success"] == 0
    assert singles[2][3][2][4]["pending"] == 0

    bt = capi.Batch(RIG, NFEAT, 3, T0s=[synth.pose_at(s, FPS) for s in START], imu=IMU, velocities=[_velocity(s, FPS) for s in START],
                    local_mapping=1, host_threads=3)
    out = [[] for _ in range(3)]
    for n in range(NTRACK):
        fr = [synth.stereo_frame(START[b] + 2 * n, RIG_NAME) for b in range(3)]
        bk = [_bucket(START[b] + 2 * n - 2, START[b] + 2 * n, FPS) if n else None for b in range(3)]
        T, reps = bt.track([f[0] for f in fr], [f[1] for f in fr], [n] * 3, imu_buckets=bk if n else None)
        for b in range(3):
            out[b].append((T[b].copy(), reps[b], bt.system(b).last_frame() if n > 0 else None))
    fn = [NTRACK] * 3
    rel = [{} for _ in range(3)]
    per_lane = [{c[0]: c for c in _lane_calls(b)} for b in range(3)]
    for i, (kind, mask) in enumerate(CALLS):
        Ls, Rs, bk = [None] * 3, [None] * 3, [None] * 3
        for b in range(3):
            if not mask[b]:
                continue
            _, _, src, b0, foreign = per_lane[b][i]
            Ls[b], Rs[b] = _images(src, foreign)
            bk[b] = _bucket(b0, src, FPS) if b0 is not None else None
        if kind == "track":
            if i == 1:
                # lanes 0 and 2 are between their two poses: a step that holds one of them is refused, names it, changes nothing
                L0, R0 = synth.stereo_frame(START[0] + 6, RIG_NAME)[:2]
                with pytest.raises(capi.VslamError) as e:
                    bt.track([L0, Ls[1], None], [R0, Rs[1], None], fn, imu_buckets=[_bucket(START[0] + 4, START[0] + 6, FPS), bk[1], None],
                             mask=[1, 1, 0])
                assert e.value.status == capi.ERR_INVALID and "lane 0" in str(e.value) and "relocalise once more" in str(e.value)
                assert bt.system(0).imu_state()["pending"] == 1 and bt.system(1).counts()["frames"] == NTRACK
            T, reps = bt.track(Ls, Rs, fn, imu_buckets=bk, mask=mask)
            for b in range(3):
                if mask[b]:
                    out[b].append((T[b].copy(), reps[b], bt.system(b).last_frame()))
        else:
            idle = (bt.system(1).counts(), bt.system(1).imu_state(), bt.system(1).last_frame())
            T, rreps, ireps = bt.relocalize_imu(Ls, Rs, fn, imu_buckets=bk if any(x is not None for x in bk) else None, mask=mask)
            assert rreps[1] is None and ireps[1] is None and not T[1].any()          # the idle lane's row and reports are not written
            now = (bt.system(1).counts(), bt.system(1).imu_state(), bt.system(1).last_frame())
            assert idle[0] == now[0] and all(np.array_equal(idle[1][k], now[1][k]) for k in ("velocity", "bias", "bias_good"))
            assert idle[1]["pending"] == now[1]["pending"] == 0 and np.array_equal(idle[2][0], now[2][0])
            for b in range(3):
                if mask[b]:
                    rel[b][i] = (T[b].copy(), rreps[b], ireps[b], bt.system(b).counts(), bt.system(b).imu_state())
        for b in range(3):
            fn[b] += mask[b]
    lanes = [(out[b], bt.system(b).counts(), bt.system(b).keyframes()) for b in range(3)]
    bt.close()

    for b in (0, 2):
        for i in (0, 2):
            _same_reloc(singles[b][3][i], rel[b][i], (b, i))
    assert rel[0][2][2]["phase"] == 2 and rel[0][2][4]["pending"] == 0
    assert np.array_equal(rel[0][2][4]["velocity"], rel[0][2][2]["velocity"]) and np.array_equal(rel[0][2][4]["bias"], rel[0][2][4]["bias_good"])
    # lane 2's failed second pose: the row is the unchanged camera pose (its first pose), the flag is down
    assert rel[2][2][1]["success"] == 0 and np.array_equal(rel[2][2][0], rel[2][0][0]) and rel[2][2][4]["pending"] == 0
    for b in range(3):
        nKF, nBA = _same(singles[b][:3], lanes[b])
        print("lane %d: %d keyframes, %d local BAs compared; inliers of its last two tracked frames %s"
              % (b, nKF, nBA, [lanes[b][0][-k][1]["n_inliers"] for k in (2, 1)]))
    print("lane 0: dt %.4f, velocity %s, rot_residual %.3e" % (rel[0][2][2]["dt"], rel[0][2][2]["velocity"], rel[0][2][2]["rot_residual"]))
    assert lanes[0][0][-1][1]["n_inliers"] >= 50 and lanes[0][0][-2][1]["n_inliers"] >= 50


def test_refusals_name_the_lane_and_change_nothing(capi):
    """a batch without IMU; a lane without a map; a second pose without its bucket"""
    synth.prerender([0, 2, 4], RIG_NAME)
    fr = [synth.stereo_frame(f, RIG_NAME) for f in (0, 2, 4)]
    plain = capi.Batch(RIG, NFEAT, 2, T0s=[synth.pose_at(0, FPS)] * 2, local_mapping=0)
    plain.track([fr[0][0]] * 2, [fr[0][1]] * 2, [0, 0])
    with pytest.raises(capi.VslamError) as e:
        plain.relocalize_imu([fr[1][0]] * 2, [fr[1][1]] * 2, [1, 1])
    assert e.value.status == capi.ERR_INVALID and "lane 0" in str(e.value) and "without IMU" in str(e.value)
    plain.close()
    bt = capi.Batch(RIG, NFEAT, 2, T0s=[synth.pose_at(0, FPS)] * 2, imu=IMU, velocities=[_velocity(0, FPS)] * 2, local_mapping=0)
    with pytest.raises(capi.VslamError) as e:
        bt.relocalize_imu([fr[1][0]] * 2, [fr[1][1]] * 2, [1, 1])
    assert e.value.status == capi.ERR_INVALID and "lane 0" in str(e.value) and "no map" in str(e.value)
    bt.track([fr[0][0]] * 2, [fr[0][1]] * 2, [0, 0])
    bk = _bucket(0, 2, FPS)
    bt.track([fr[1][0]] * 2, [fr[1][1]] * 2, [1, 1], imu_buckets=[bk, bk])
    before = [bt.system(b).counts() for b in range(2)]
    T, reps, ireps = bt.relocalize_imu([None, fr[1][0]], [None, fr[1][1]], [2, 2], mask=[0, 1])
    assert reps[1]["success"] == 1 and ireps[1]["phase"] == 1
    with pytest.raises(capi.VslamError) as e:
        bt.relocalize_imu([fr[2][0]] * 2, [fr[2][1]] * 2, [3, 3])               # lane 1 is between its poses and has no bucket
    assert e.value.status == capi.ERR_INVALID and "lane 1" in str(e.value) and "bucket" in str(e.value)
    assert bt.system(0).counts() == before[0] and bt.system(0).imu_state()["pending"] == 0 and bt.system(1).imu_state()["pending"] == 1
    # with the bucket the pair completes: lane 0 takes its first pose in the same call as lane 1 its second
    T, reps, ireps = bt.relocalize_imu([fr[2][0]] * 2, [fr[2][1]] * 2, [3, 3], imu_buckets=[None, _bucket(2, 4, FPS)])
    assert [ireps[b]["phase"] for b in range(2)] == [1, 2]
    bt.close()
