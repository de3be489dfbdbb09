"""vslam_batch_relocalize: lost lanes of a lockstep group recover from their own maps in one call.  Yardstick: capi.System driven
alone through the same call sequence on the same frames with the lane's rig (that path is pinned by tests/test_gpu_reloc.py and
tests/test_gpu_system.py).  Comparison: the one test_gpu_batch._same makes (integer report fields, match tables, counts and keyframe
lists exactly, poses to 1e-9 - the allowance for the local BA's LDS-atomic summation order); relocalisation report integers equal."""
import numpy as np
import pytest
import synth
from test_gpu_batch import _same, _velocity, _bucket, G, NOISE
import test_gpu_batch_lanes                      # noqa: F401  (defines synth.RIGS["euroc_b"])

pytestmark = pytest.mark.gpu

A, B = "euroc", "euroc_b"
NFEAT = 1500
FPS = synth.RIGS[A]["fps"]
STEP = 8                                         # source frames 0, 8, 16, ...: the euroc_b session inserts its FOURTH keyframe (the first one
                                                 # that gets a local-mapping pass) at step 12, the last of lane 0's 13 tracked frames
RIGS3, NTRACK = [B, A, B], [13, 9, 11]
REL_INT = ("success", "n_points", "n_pairs", "best_hypothesis", "best_count", "n_inliers", "n_stereo")


def _src(n):
    return STEP * n


def _foreign():
    return synth.stereo_frame(4, scene_seed=9, tex_seed=0xBEEF)[:2]


def _system(capi, rig_name, mode, imu=None):
    mapping, delay, np_delay = mode
    rig = synth.RIGS[rig_name]
    return capi.System(rig, NFEAT, T0=synth.pose_at(0, rig["fps"]), imu=imu, local_mapping=mapping, mapping_delay=delay, mapping_np_delay=np_delay)


def _single(capi, rig_name, mode, ntrack, reloc, after):
    """one session alone: ntrack frames, then (reloc = (L, R, frame number) or None) one relocalize call, then `after` =
    [(source frame, frame number), ...] tracked.  Returns (per-frame list, counts, keyframes, relocalisation record or None)."""
    s = _system(capi, rig_name, mode)
    out = []
    for n in range(ntrack):
        L, R, _ = synth.stereo_frame(_src(n), rig_name)
        P, rep = s.track(L, R, n)
        out.append((P, rep, s.last_frame() if n > 0 else None))
    rel = None
    if reloc is not None:
        T, rrep = s.relocalize(reloc[0], reloc[1], reloc[2])
        rel = (T, rrep, s.counts(), s.last_frame())
    for f, fn in after:
        L, R, _ = synth.stereo_frame(f, rig_name)
        P, rep = s.track(L, R, fn)
        out.append((P, rep, s.last_frame()))
    res = (out, s.counts(), s.keyframes(), rel)
    s.close()
    return res


def _same_reloc(one, lane):
    (T1, r1, c1, l1), (T2, r2, c2, l2) = one, lane
    for k in REL_INT:
        assert r1[k] == r2[k], (k, r1[k], r2[k])
    assert r1["lm"]["iterations"] == r2["lm"]["iterations"] and r1["lm"]["inner"] == r2["lm"]["inner"]
    assert np.abs(T1 - T2).max() <= 1e-9
    assert c1 == c2
    assert np.array_equal(l1[0], l2[0]) and np.array_equal(l1[1], l2[1])


@pytest.mark.parametrize("mode", [(0, 0, 0), (1, 0, 1), (2, 4, 2)])
def test_lost_lanes_relocalise_in_lockstep(capi, mode):
    """Three lanes with rigs [euroc_b, euroc, euroc_b] tracked 13, 9 and 11 frames (source frames 0, 8, 16, ...), then ONE relocalize
    call with mask [1, 0, 1]: lane 0 on its own frame 3 (recovers), lane 2 on a frame of another scene under another texture
    (refused), lane 1 idle; then two more tracked frames per lane.
    Checked on the CPU when the cases were chosen (the restated loop oracle/vo_system.py + tests/reloc_ref.py, euroc_b rig, these
    frames): keyframes of the 13-frame session at steps 0, 5, 10, 12; its map (1012 non-outlier points) recovers frame 3 with 191
    pairs, best count 187, 187 inliers, 9.4e-4 from the tracked pose of frame 3; the 11-frame session's map (490 points) gives 6
    pairs, best count 1, 1 inlier on the foreign frame: refused.
    A session hands its first local-mapping pass over at its fourth keyframe - here step 12.  In mode (2, 4, 2) the call's frame
    number for lane 0 is that step + mapping_np_delay (14): the pass's new points are due and land inside the call's begin phase,
    the local BA's window is collected and handed over inside the call, and its write-back lands at the second frame tracked
    afterwards (frame number 16 = step 12 + mapping_delay).  The keyframe step is read from the single session's reports and
    asserted below.  (Map points therefore change inside the call in that mode - by the landing pass, exactly as in the single
    session; in the other modes nothing is due and they must not.)"""
    mapping, delay, np_delay = mode
    for rn, nt in zip(RIGS3, NTRACK):
        synth.prerender([_src(n) for n in range(nt + 2)], rn)
    # the lanes' frame numbers at the call: the next one, or (mode 2) the one at which lane 0's pending new points are due
    probe = _single(capi, B, mode, NTRACK[0], None, [])
    kf_steps = [n for n, (_, r, _) in enumerate(probe[0]) if r["keyframe_inserted"]]
    fn0 = NTRACK[0]
    if mapping == 2:
        fn0 = kf_steps[-1] + np_delay
        # the fourth keyframe (the first with a pass) was inserted within the delay window before the call and after every frame
        # at which its results could have landed: they are still pending at the call, and the new points are due at fn0
        assert len(kf_steps) >= 4 and fn0 >= NTRACK[0] and fn0 - delay <= kf_steps[-1] and kf_steps[-1] + np_delay > NTRACK[0] - 1, (kf_steps, fn0)
    fns = [fn0, NTRACK[1], NTRACK[2]]
    own = synth.stereo_frame(_src(3), B)[:2]
    foreign = _foreign()
    rel_in = [(own[0], own[1], fns[0]), None, (foreign[0], foreign[1], fns[2])]
    # lane 0 goes on from its frame 3 (source frames of steps 4 and 5), the others from where they were
    after = [[(_src(4), fns[0] + 1), (_src(5), fns[0] + 2)],
             [(_src(NTRACK[1]), NTRACK[1]), (_src(NTRACK[1] + 1), NTRACK[1] + 1)],
             [(_src(NTRACK[2]), fns[2] + 1), (_src(NTRACK[2] + 1), fns[2] + 2)]]
    singles = [_single(capi, RIGS3[b], mode, NTRACK[b], rel_in[b], after[b]) for b in range(3)]
    # the single-session side first: lane 0's reference succeeded, lane 2's was refused
    assert singles[0][3][1]["success"] == 1 and singles[2][3][1]["success"] == 0
    assert singles[0][3][1]["n_inliers"] >= 50

    bt = capi.Batch(None, NFEAT, 3, rigs=[synth.RIGS[rn] for rn in RIGS3], T0s=[synth.pose_at(0, FPS)] * 3, local_mapping=mapping,
                    host_threads=3, mapping_delay=delay, mapping_np_delay=np_delay)
    out = [[] for _ in range(3)]
    for n in range(max(NTRACK)):
        mask = [int(n < NTRACK[b]) for b in range(3)]
        fr = [synth.stereo_frame(_src(n), RIGS3[b]) if mask[b] else (None, None) for b in range(3)]
        T, reps = bt.track([f[0] for f in fr], [f[1] for f in fr], [n] * 3, mask=mask)
        for b in range(3):
            if mask[b]:
                out[b].append((T[b].copy(), reps[b], bt.system(b).last_frame() if n > 0 else None))
    before = [bt.system(b).counts() for b in range(3)]
    T, rreps = bt.relocalize([own[0], None, foreign[0]], [own[1], None, foreign[1]], fns, mask=[1, 0, 1])
    rel = [(T[b].copy(), rreps[b], bt.system(b).counts(), bt.system(b).last_frame()) if rreps[b] is not None else None for b in range(3)]
    assert rreps[1] is None and not T[1].any()                   # the idle lane's row and report are not written
    for k in range(2):
        fr = [synth.stereo_frame(after[b][k][0], RIGS3[b]) for b in range(3)]
        T, reps = bt.track([f[0] for f in fr], [f[1] for f in fr], [after[b][k][1] for b in range(3)])
        for b in range(3):
            out[b].append((T[b].copy(), reps[b], bt.system(b).last_frame()))
    lanes = [(out[b], bt.system(b).counts(), bt.system(b).keyframes()) for b in range(3)]
    bt.close()

    # lane 0: recovered; one more frame on record, keyframes and map points as before, no match tables
    assert rel[0][1]["success"] == 1
    assert rel[0][2]["frames"] == before[0]["frames"] + 1
    assert rel[0][2]["keyframes"] == before[0]["keyframes"]
    assert len(rel[0][3][0]) == 0
    if mapping != 2:
        assert rel[0][2]["map_points"] == before[0]["map_points"]
    # lane 2: refused, its pose row is the unchanged camera pose (= the pose of its last tracked frame)
    assert rel[2][1]["success"] == 0 and np.array_equal(rel[2][0], out[2][NTRACK[2] - 1][0])
    for b in (0, 2):
        _same_reloc(singles[b][3], rel[b])
    for b in range(3):
        nKF, nBA = _same(singles[b][:3], lanes[b])
        print("mode %s lane %d: %d keyframes, %d local BAs compared; keyframe steps of lane 0 %s, relocalised at frame number %d"
              % (mode, b, nKF, nBA, kf_steps, fns[0]))
    print("lane 0 tracks on from the recovered pose with %s inliers" % [lanes[0][0][-k][1]["n_inliers"] for k in (2, 1)])


def test_imu_batch_is_refused(capi):
    imu = dict(gravity=G, noise=NOISE, T_bs=synth.T_BC1, hz=200)
    synth.prerender([0, 2, 4], A)
    rig = synth.RIGS[A]
    bt = capi.Batch(rig, NFEAT, 2, T0s=[synth.pose_at(0, FPS)] * 2, imu=imu, velocities=[_velocity(0, FPS)] * 2, local_mapping=0, host_threads=2)
    ss = [capi.System(rig, NFEAT, T0=synth.pose_at(0, FPS), imu=dict(imu, velocity=_velocity(0, FPS)), local_mapping=0) for _ in range(2)]

    def step(n):
        L, R, _ = synth.stereo_frame(2 * n, A)
        bk = _bucket(2 * (n - 1), 2 * n, FPS) if n > 0 else None
        T, reps = bt.track([L, L], [R, R], [n, n], imu_buckets=[bk, bk])
        for b in range(2):
            P, rep = ss[b].track(L, R, n, imu_bucket=bk)
            assert np.abs(P - T[b]).max() <= 1e-9
            for k in ("n_active", "n_inliers", "n_stereo", "rounds", "keyframe_inserted", "n_map_points"):
                assert rep[k] == reps[b][k], (n, b, k)

    step(0); step(1)
    L, R, _ = synth.stereo_frame(2, A)
    with pytest.raises(capi.VslamError) as e:
        bt.relocalize([L, L], [R, R], [2, 2])
    assert e.value.status == capi.ERR_INVALID and "lane 0" in str(e.value) and "IMU" in str(e.value)
    with pytest.raises(capi.VslamError) as e:
        bt.relocalize([None, L], [None, R], [2, 2], mask=[0, 1])
    assert e.value.status == capi.ERR_INVALID and "lane 1" in str(e.value)
    step(2)                                                       # nothing changed: the next step of all lanes equals the singles
    bt.close()
    for s in ss:
        s.close()


def test_restarted_lane_without_a_map_is_refused(capi):
    synth.prerender([0, 2, 4, 6], A)
    rig = synth.RIGS[A]
    bt = capi.Batch(rig, NFEAT, 2, T0s=[synth.pose_at(0, FPS)] * 2, local_mapping=1, host_threads=2)
    ss = [capi.System(rig, NFEAT, T0=synth.pose_at(0, FPS), local_mapping=1) for _ in range(2)]

    def same(T, reps, b, P, rep):
        assert np.abs(P - T[b]).max() <= 1e-9
        for k in ("n_active", "n_inliers", "n_stereo", "rounds", "keyframe_inserted", "n_keyframes", "n_map_points"):
            assert rep[k] == reps[b][k], (b, k)

    for n in range(3):
        L, R, _ = synth.stereo_frame(2 * n, A)
        T, reps = bt.track([L, L], [R, R], [n, n])
        for b in range(2):
            same(T, reps, b, *ss[b].track(L, R, n))
    bt.restart_lane(1)
    L, R, _ = synth.stereo_frame(4, A)
    with pytest.raises(capi.VslamError) as e:
        bt.relocalize([None, L], [None, R], [0, 1], mask=[0, 1])
    assert e.value.status == capi.ERR_INVALID and "lane 1" in str(e.value) and "no map" in str(e.value)
    with pytest.raises(capi.VslamError) as e:      # a masked lane without images (NULL device pointers)
        bt.relocalize([None, None], [None, None], [3, 0], mask=[1, 0], on_device=True)
    assert e.value.status == capi.ERR_INVALID and "lane 0" in str(e.value)
    # the next step of all lanes: lane 0 goes on, lane 1 starts its new session - as the singles do
    ss[1].close()
    ss[1] = capi.System(rig, NFEAT, T0=synth.pose_at(0, FPS), local_mapping=1)
    L3, R3, _ = synth.stereo_frame(6, A)
    L0, R0, _ = synth.stereo_frame(0, A)
    T, reps = bt.track([L3, L0], [R3, R0], [3, 0])
    same(T, reps, 0, *ss[0].track(L3, R3, 3))
    same(T, reps, 1, *ss[1].track(L0, R0, 0))
    assert bt.system(0).counts() == ss[0].counts() and bt.system(1).counts() == ss[1].counts()
    bt.close()
    for s in ss:
        s.close()


def test_relocalise_discards_a_pending_prefetch(capi):
    """a track_prefetch step (the next frames' extraction already in flight), then relocalize on one lane, then the step whose
    frames were prefetched: the same results as the run without prefetch.  The call runs with the batch's stage timing on (both
    runs): its five stages must show in vslam_batch_timings."""
    frames = [0, 2, 4, 6, 8]
    synth.prerender(frames, A)
    rig = synth.RIGS[A]
    imgs = [synth.stereo_frame(f, A) for f in frames]
    dev = [(capi.DeviceImage(f[0]), capi.DeviceImage(f[1])) for f in imgs]
    runs = []
    for prefetch in (False, True):
        bt = capi.Batch(rig, NFEAT, 2, T0s=[synth.pose_at(0, FPS)] * 2, local_mapping=1, host_threads=2)
        rec = []
        for n in range(4):
            if prefetch:
                T, reps = bt.track_prefetch([dev[n][0].ptr] * 2, [dev[n][1].ptr] * 2, [n, n], next_lefts=[dev[n + 1][0].ptr] * 2,
                                            next_rights=[dev[n + 1][1].ptr] * 2)
            else:
                T, reps = bt.track([imgs[n][0]] * 2, [imgs[n][1]] * 2, [n, n])
            rec.append((T.copy(), reps))
        bt.set_timing(True)
        bt.timings()                              # (read-and-reset)
        Tr, rr_ = bt.relocalize([imgs[2][0], None], [imgs[2][1], None], [4, 0], mask=[1, 0])
        assert rr_[0]["success"] == 1
        stages, _ = bt.timings()                  # the call's stages show in the batch's stage timers
        assert {"reloc_match", "reloc_pairs", "reloc_ransac", "reloc_refine", "reloc_inframe"} <= set(stages), sorted(stages)
        bt.set_timing(False)
        rec.append((Tr.copy(), [rr_[0]]))
        if prefetch:                              # exactly the prefetched pointers: the discarded prefetch must not be used
            T, reps = bt.track_prefetch([dev[4][0].ptr] * 2, [dev[4][1].ptr] * 2, [5, 4])
        else:
            T, reps = bt.track([imgs[4][0]] * 2, [imgs[4][1]] * 2, [5, 4])
        rec.append((T.copy(), reps))
        runs.append((rec, [bt.system(b).counts() for b in range(2)], [bt.system(b).last_frame() for b in range(2)]))
        bt.close()
    (ra, ca, la), (rb, cb, lb) = runs
    assert ca == cb
    for (Ta, pa), (Tb, pb) in zip(ra, rb):
        assert np.abs(Ta - Tb).max() <= 1e-9
        for x, y in zip(pa, pb):
            for k in x:
                if isinstance(x[k], (int, np.integer)):
                    assert x[k] == y[k], k
    for b in range(2):
        assert np.array_equal(la[b][0], lb[b][0]) and np.array_equal(la[b][1], lb[b][1])
    for a, b in dev:
        a.free(); b.free()
