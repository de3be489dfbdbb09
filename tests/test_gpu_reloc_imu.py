"""GPU tests of the relocalisation of stereo + IMU sessions (vslam_system_relocalize_imu, the rule taps vslam_imu_reinit_velocity
and vslam_imu_reinit_velocity_batch) against the CPU restatement (tests/reloc_imu_ref.py): the
velocity from two relocalised poses and the IMU bucket between them, the two-phase commit, and the state machine around it."""
import numpy as np
import pytest
import synth
import reloc_imu_ref as ri

pytestmark = pytest.mark.gpu
RIG = synth.RIGS["euroc"]
FPS = RIG["fps"]
G = (0.0, 9.81, 0.0)
NOISE = (1.6968e-4, 1.9393e-5, 2.0e-3, 3.0e-3)
HZ = 200
IMU = dict(gravity=G, noise=NOISE, T_bs=synth.T_BC1, hz=HZ)
SAMPLE_BIAS = np.array([0.03, -0.02, 0.05, 0.004, -0.003, 0.002])
BIAS_GOOD = np.array([0.02, -0.01, 0.03, 0.001, -0.002, 0.0015])
REP_INTS = ("success", "n_points", "n_pairs", "best_hypothesis", "best_count", "n_inliers", "n_stereo")


def _prm(oracle):
    return oracle.imu_params(G, NOISE[0], NOISE[2], NOISE[1], NOISE[3], synth.T_BC1)


def _velocity(f):
    h = 1e-4
    return (synth.pose_at(f + h * FPS, FPS)[:3, 3] - synth.pose_at(f - h * FPS, FPS)[:3, 3]) / (2 * h)


def _rigid_inv(T):
    Ti = np.eye(4)
    Rt = T[:3, :3].T.copy()
    Ti[:3, :3] = Rt
    for i in range(3):
        Ti[i, 3] = -(Rt[i, 0] * T[0, 3] + Rt[i, 1] * T[1, 3] + Rt[i, 2] * T[2, 3])
    return Ti


# ---- the rule alone ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def m(capi):
    ge = capi.Extractor(RIG["w"], RIG["h"], 1500, batch=2)
    return capi.Matcher(RIG, ge, 0, ge, 1)


def _dts(n):
    """the dt rule on 5 ms timestamps: a single sample takes 1 / hz"""
    return np.full(n, 1.0 / HZ if n == 1 else 0.005)


def _crafted(n, f0=10, seed=7):
    """n noisy, biased samples from frame f0 on; the second pose: the trajectory's pose at the bucket's end, moved by a few cm and
    turned by a few mrad (two relocalised poses are not consistent with the bucket to rounding)"""
    S, _, _ = synth.imu_samples(f0, f0 + n // 10 + 1, noise_seed=seed, bias=SAMPLE_BIAS)
    S = S[:n]
    Tp = synth.pose_at(f0)
    Tn = synth.pose_at(f0 + n * 0.005 * 20).copy()
    c, s = np.cos(2e-3), np.sin(2e-3)
    Tn[:3, :3] = Tn[:3, :3] @ np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    Tn[:3, 3] += np.array([0.012, -0.007, 0.009])
    return S, np.arange(n) * 5e6, Tp, _rigid_inv(Tn)


def _allow(ref, dt):
    """the allowance tests/test_gpu_imu_preint.py grants the pre-integration's prediction (1e-12 max(1, |ref|) per entry), times
    (1 + 2 / dt): the rule adds a subtraction, a division by dt and an addition per component"""
    return 1e-12 * np.maximum(1.0, np.abs(ref)) * (1.0 + 2.0 / dt)


def _check_rule(got, ref, what):
    dt = ref["dt"]
    assert abs(got["dt"] - dt) <= 1e-12 * max(1.0, dt), (what, got["dt"], dt)
    for k in ("velocity_prev", "velocity"):
        err = np.abs(got[k] - ref[k])
        print("%s: %s error %.2e (allowed %.2e)" % (what, k, err.max(), _allow(ref[k], dt).min()))
        assert (err <= _allow(ref[k], dt)).all(), (what, k, err, _allow(ref[k], dt))
    err = abs(got["rot_residual"] - ref["rot_residual"])
    print("%s: rot_residual %.6e, error %.2e" % (what, ref["rot_residual"], err))
    assert err <= _allow(ref["rot_residual"], dt), (what, err)
    assert np.abs(ref["velocity_prev"]).max() > 0.05 and ref["rot_residual"] > 1e-4      # (values that matter)


@pytest.mark.parametrize("n", [1, 2, 12, 13, 25])
def test_rule_tap_against_the_restatement(oracle, capi, m, n):
    """bucket sizes 1 (the dt0 rule), 2, 12, 13 (PIM_CHUNK is 12) and 25, a non-zero biasGood"""
    S, ts, Tp, Tcw = _crafted(n)
    got = capi.imu_reinit_velocity(m, G, NOISE, synth.T_BC1, Tp, BIAS_GOOD, S[:, :3], S[:, 3:], ts, HZ, Tcw)
    ref = ri.reinit_velocity(oracle, _prm(oracle), BIAS_GOOD, S, _dts(n), Tp, Tcw)
    _check_rule(got, ref, "n %d" % n)


@pytest.mark.parametrize("sizes", [(13, 0, 1), (25, 0, 12)])
def test_rule_tap_lanes_with_an_idle_middle_lane(oracle, capi, m, sizes):
    """one launch of each kernel for three lanes; the idle lane's row comes back as it went in"""
    lanes, refs = [], []
    for b, n in enumerate(sizes):
        if n == 0:
            lanes.append((G, NOISE, synth.T_BC1, np.eye(4), np.zeros(6), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0), HZ, np.eye(4)))
            refs.append(None)
            continue
        S, ts, Tp, Tcw = _crafted(n, f0=10 + 4 * b, seed=7 + b)
        bias = BIAS_GOOD * (1.0 + 0.5 * b)
        lanes.append((G, NOISE, synth.T_BC1, Tp, bias, S[:, :3], S[:, 3:], ts, HZ, Tcw))
        refs.append(ri.reinit_velocity(oracle, _prm(oracle), bias, S, _dts(n), Tp, Tcw))
    out = capi.imu_reinit_velocity_batch(m, lanes, fill=-7.25)
    for b, ref in enumerate(refs):
        if ref is None:
            assert (out[b] == -7.25).all()
            continue
        got = dict(dt=out[b, 0], velocity_prev=out[b, 1:4], velocity=out[b, 4:7], rot_residual=out[b, 7])
        _check_rule(got, ref, "lane %d, n %d" % (b, sizes[b]))


# ---- the session ---------------------------------------------------------------------------------------------------------------
def _bucket(f0, f1):
    S, dts, _ = synth.imu_samples(f0, f1, FPS, noise_seed=0x1A00 + f1)
    return (S, dts), (S[:, :3], S[:, 3:], np.arange(len(dts)) * 5e6)


def _same_report(rep, want, what):
    for k in REP_INTS:
        assert rep[k] == want[k], (what, k, rep[k], want[k])


@pytest.mark.parametrize("mode", [0, 1])
def test_session_two_phase_relocalisation(capi, oracle, mode):
    """EuRoC rig, 1500 features, source frames 0, 2, .., 24 tracked with IMU; relocalise on source frame 6 (first pose), on 8 with
    the bucket 6 -> 8 (second pose: the velocity), then track 10 and 12.  Call by call against the restatement; against the ground
    truth each pose error and the velocity error at most three times the restatement's own on the same frame (the convention of
    test_relocalise_rendered_frames).  The restatement's figures, measured on the CPU when the rule was chosen: first pose 1.27e-3,
    second 8.3e-4, velocity 2.1e-2 m/s, follow-up poses 1.43e-3 / 1.36e-3 with 358 / 341 inliers."""
    src = list(range(0, 26, 2))
    synth.prerender(src)
    T0 = synth.pose_at(0, FPS)
    ref = ri.Session(oracle, RIG, 1500, _prm(oracle), T0, _velocity(0))
    got = capi.System(RIG, 1500, T0=T0, imu=dict(IMU, velocity=_velocity(0)), local_mapping=1)
    for n, f in enumerate(src):
        L, R, _ = synth.stereo_frame(f)
        bo, bg = _bucket(src[n - 1], f) if n else (None, None)
        Pr = ref.track(L, R, n, bo)
        Pg, rep = got.track(L, R, n, imu_bucket=bg)
        assert np.abs(Pg - Pr).max() < 1e-7, (f, np.abs(Pg - Pr).max())
    st0 = got.imu_state()
    assert st0["pending"] == 0 and np.abs(st0["bias"]).max() > 0 and np.array_equal(st0["bias"], st0["bias_good"])
    before = got.counts()
    nfr = len(src)
    # ---- first pose ------------------------------------------------------------------------------------------------------------
    L, R, Tt = synth.stereo_frame(6)
    Pr, want, iw = ref.relocalize(L, R, None, mode)
    Pg, rep, irep = got.relocalize_imu(L, R, nfr, mode=mode)
    assert want["success"] == 1
    _same_report(rep, want, "first pose")
    assert irep["phase"] == 1 and iw["phase"] == 1
    assert np.abs(Pg - Pr).max() < 1e-7
    e_ref, e_got = np.abs(Pr - Tt).max(), np.abs(Pg - Tt).max()
    print("mode %d first pose (source 6): %d inliers, error %.3e (restatement %.3e)" % (mode, rep["n_inliers"], e_got, e_ref))
    assert e_got <= 3 * e_ref
    st1 = got.imu_state()
    assert st1["pending"] == 1
    for k in ("velocity", "bias", "bias_good"):
        assert np.array_equal(st1[k], st0[k]), k
    # ---- second pose: the velocity -----------------------------------------------------------------------------------------------
    L, R, Tt = synth.stereo_frame(8)
    bo, bg = _bucket(6, 8)
    Pr, want, iw = ref.relocalize(L, R, bo, mode)
    Pg, rep, irep = got.relocalize_imu(L, R, nfr + 1, imu_bucket=bg, mode=mode)
    assert want["success"] == 1
    _same_report(rep, want, "second pose")
    assert irep["phase"] == 2 and iw["phase"] == 2
    assert np.abs(Pg - Pr).max() < 1e-7
    dt = iw["dt"]
    assert abs(irep["dt"] - dt) <= 1e-12 and abs(dt - 0.095) < 1e-9
    for k in ("velocity_prev", "velocity"):
        assert np.abs(irep[k] - iw[k]).max() <= 2e-7 / dt, (k, np.abs(irep[k] - iw[k]).max())      # two poses at 1e-7 through the division
    # (nine entries of two rotations at 1e-7 each: the norm of the difference moves by at most 3 x 2e-7)
    assert abs(irep["rot_residual"] - iw["rot_residual"]) <= 6e-7
    e_ref, e_got = np.abs(Pr - Tt).max(), np.abs(Pg - Tt).max()
    v_ref, v_got = np.abs(iw["velocity"] - _velocity(8)).max(), np.abs(irep["velocity"] - _velocity(8)).max()
    print("mode %d second pose (source 8): %d inliers, error %.3e (restatement %.3e); dt %.4f, velocity error %.3e m/s (restatement %.3e), "
          "rot_residual %.3e" % (mode, rep["n_inliers"], e_got, e_ref, dt, v_got, v_ref, irep["rot_residual"]))
    assert e_got <= 3 * e_ref and v_got <= 3 * v_ref
    st2 = got.imu_state()
    assert st2["pending"] == 0
    assert np.array_equal(st2["velocity"], irep["velocity"])
    assert np.array_equal(st2["bias"], st0["bias_good"]) and np.array_equal(st2["bias_good"], st0["bias_good"])
    assert np.array_equal(irep["bias"], st0["bias_good"])
    after = got.counts()
    assert after["keyframes"] == before["keyframes"] and after["map_points"] == before["map_points"] and after["frames"] == before["frames"] + 2
    # ---- ordinary IMU frames again -------------------------------------------------------------------------------------------------
    for k, f in enumerate((10, 12)):
        L, R, Tt = synth.stereo_frame(f)
        bo, bg = _bucket(f - 2, f)
        Pr = ref.track(L, R, nfr + 2 + k, bo)
        Pg, rep = got.track(L, R, nfr + 2 + k, imu_bucket=bg)
        lg = ref.s.log[-1]
        e_ref, e_got = np.abs(Pr - Tt).max(), np.abs(Pg - Tt).max()
        print("mode %d follow-up (source %d): %d inliers, %d rounds, error %.3e (restatement %.3e)" % (mode, f, rep["n_inliers"], rep["rounds"], e_got, e_ref))
        assert rep["n_inliers"] >= 50
        assert (rep["n_active"], rep["n_inliers"], rep["n_stereo"], rep["rounds"]) == (lg["nActive"], lg["nIn"], lg["nStereo"], lg["rounds"])
        assert np.abs(Pg - Pr).max() < 1e-7
        assert e_got <= 3 * e_ref
    got.close()


# ---- the state machine -----------------------------------------------------------------------------------------------------------
def _snapshot(s):
    st = s.imu_state()
    fi, P = s.keyframes()
    xyz, ol = s.map_points()
    return dict(counts=s.counts(), v=st["velocity"], b=st["bias"], g=st["bias_good"], fi=fi, P=P, xyz=xyz, ol=ol)


def _equal(a, b, tol=0.0):
    """tol = 0: the same session before and after a call; 1e-9 between twins (a local BA sums with fp64 atomics, whose order varies
    from run to run: the convention of tests/test_gpu_reloc.py)"""
    assert a["counts"] == b["counts"]
    for k in ("fi", "ol"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("v", "b", "g", "P", "xyz"):
        assert a[k].shape == b[k].shape and np.abs(a[k] - b[k]).max() <= tol, k


def test_state_machine(capi):
    """Twin sessions through the same calls up to the first pose.  While the velocity is pending: a tracked frame and a second
    relocalisation without a bucket are refused with nothing changed; a foreign frame as the second pose fails, drops the flag
    and changes nothing else (against the twin, which is still pending); the session then recovers through a fresh pair of calls."""
    src = [0, 2, 4, 6, 8]
    synth.prerender(src + [10, 12])
    T0 = synth.pose_at(0, FPS)
    a, b = (capi.System(RIG, 1500, T0=T0, imu=dict(IMU, velocity=_velocity(0)), local_mapping=1) for _ in range(2))
    for n, f in enumerate(src):
        L, R, _ = synth.stereo_frame(f)
        bg = _bucket(src[n - 1], f)[1] if n else None
        a.track(L, R, n, imu_bucket=bg); b.track(L, R, n, imu_bucket=bg)
    L, R, _ = synth.stereo_frame(4)
    Pa, ra, ia = a.relocalize_imu(L, R, 5)
    Pb, rb, ib = b.relocalize_imu(L, R, 5, imu_bucket=_bucket(2, 4)[1])      # (the bucket of a first pose is ignored)
    assert ra["success"] == 1 and ia["phase"] == 1 and ib["phase"] == 1 and np.abs(Pa - Pb).max() < 1e-9
    assert a.imu_state()["pending"] == 1
    snap = _snapshot(a)
    # tracking while pending
    L6, R6, _ = synth.stereo_frame(6)
    with pytest.raises(capi.VslamError) as e:
        a.track(L6, R6, 6, imu_bucket=_bucket(4, 6)[1])
    assert e.value.status == capi.ERR_INVALID and "relocalise once more" in str(e.value)
    _equal(_snapshot(a), snap)
    assert a.imu_state()["pending"] == 1
    # the second pose without its bucket, or with an empty one
    for bk in (None, (np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0))):
        with pytest.raises(capi.VslamError) as e:
            a.relocalize_imu(L6, R6, 6, imu_bucket=bk)
        assert e.value.status == capi.ERR_INVALID and "bucket" in str(e.value)
        _equal(_snapshot(a), snap)
        assert a.imu_state()["pending"] == 1
    # a foreign frame as the second pose
    Lf, Rf, _ = synth.stereo_frame(6, scene_seed=9, tex_seed=0xBEEF)
    T, rep, irep = a.relocalize_imu(Lf, Rf, 6, imu_bucket=_bucket(4, 6)[1])
    assert rep["success"] == 0 and irep["phase"] == 0 and np.array_equal(T, Pa)
    assert a.imu_state()["pending"] == 0 and b.imu_state()["pending"] == 1
    _equal(_snapshot(a), snap)
    _equal(_snapshot(a), _snapshot(b), 1e-9)
    # a later success is a first pose again; the pair of calls recovers the session
    Pa, ra, ia = a.relocalize_imu(L6, R6, 7)
    assert ra["success"] == 1 and ia["phase"] == 1 and a.imu_state()["pending"] == 1
    L8, R8, _ = synth.stereo_frame(8)
    Pa, ra, ia = a.relocalize_imu(L8, R8, 8, imu_bucket=_bucket(6, 8)[1])
    assert ra["success"] == 1 and ia["phase"] == 2 and a.imu_state()["pending"] == 0
    L10, R10, Tt = synth.stereo_frame(10)
    P, rep = a.track(L10, R10, 9, imu_bucket=_bucket(8, 10)[1])
    assert rep["n_inliers"] >= 50 and np.abs(P - Tt).max() < 0.05
    a.close(); b.close()


def test_refusals(capi):
    """the _imu call on a session without IMU, on a mono session and on a session without a map; the old entry point on an IMU
    session (tests/test_gpu_reloc.py pins that too)"""
    L, R, _ = synth.stereo_frame(0)
    s = capi.System(RIG, 1500, local_mapping=0)
    s.track(L, R, 0)
    with pytest.raises(capi.VslamError) as e:
        s.relocalize_imu(L, R, 1)
    assert e.value.status == capi.ERR_INVALID and "without IMU" in str(e.value)
    ms = capi.MonoSystem(RIG, 1500, synth.MONO_FPS, imu=IMU)
    with pytest.raises(capi.VslamError) as e:
        capi.System.relocalize_imu(ms, L, R, 1)
    assert e.value.status == capi.ERR_INVALID and "mono" in str(e.value)
    si = capi.System(RIG, 1500, imu=IMU, local_mapping=0)
    with pytest.raises(capi.VslamError) as e:
        si.relocalize_imu(L, R, 1)
    assert e.value.status == capi.ERR_INVALID and "no map" in str(e.value)
    with pytest.raises(capi.VslamError) as e:
        si.relocalize(L, R, 1)
    assert e.value.status == capi.ERR_INVALID and "IMU" in str(e.value)
    for q in (s, ms, si):
        q.close()
