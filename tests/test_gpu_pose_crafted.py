"""GPU parity of the pose solve (k_pose_lm, pose_build_factors, pose_find_outliers; the IMU solve on the same helpers;
world_to_frame_cam) on the crafted cases of tests/pose_cases.py, which tests/test_pose_cases.py proves on the CPU to reach
the LM branches, the compaction boundaries and the chi2 / depth / cheirality bounds they are meant for, with reference
decisions that do not depend on the summation order.  Frames are loaded with stereo_finalize_arrays + set_keys: the
extractor never runs.  Every solve reloads its frame (the solve mutates rightIdxs, leftIdxs, depth and close), and the
oracle gets exactly the stereo state read back from the device.

Tolerances: decisions, counts, flags, matches and stereo arrays are equal; lambda to 1e-12 relative; T_cw within
max(1e-9, 10 x the case's spread over permutations of the map points), which is 1e-9 for every case here (the two
compaction cases that keep two factors only: the two points in the camera frame at 1e-9, the one rotation the data does
not fix against a rounding-error bound); finalError to 1e-9 relative; the initial error of
the compaction cases to 1e-10 relative (a sum of <= 3073 positive fp64 terms moves by ~3e-13 when reordered; one lost,
doubled or misplaced factor moves it by >= 1e-6, test_pose_cases.py::test_compact_case)."""
import numpy as np
import pytest
import synth
import pose_cases as pc

pytestmark = pytest.mark.gpu
RIG = pc.RIG


def new_matcher(capi):
    ge = capi.Extractor(RIG["w"], RIG["h"], 1500, batch=2)
    return capi.Matcher(RIG, ge, 0, ge, 1)


@pytest.fixture(scope="module")
def matcher(capi):
    """one extractor / matcher pair for every crafted frame (both key sets are overridden)"""
    return new_matcher(capi)


def load_frame(m, c):
    dL, dR = pc.descriptors(c)
    m.stereo_finalize_arrays(c["best"], c["depth"], c["sad"], len(c["kR"]))
    m.set_keys(0, c["kL"], dL)
    m.set_keys(1, c["kR"], dR)
    return m.stereo_fetch(len(c["kL"]), len(c["kR"]))


def solve(capi, m, c):
    """(stereo state before, result, stereo state after) of one solve on a freshly loaded frame"""
    st = load_frame(m, c)
    got = capi.estimate_pose(m, c["points"], c["inF"], c["inFR"], c["mpo"], c["matches"], c["out0"], c["T0"])
    return st, got, m.stereo_fetch(len(c["kL"]), len(c["kR"]))


def assert_decisions(got, st2, ref):
    assert (got["iterations"], got["inner"]) == (ref["iterations"], ref["inner"])
    assert (got["nIn"], got["nStereo"]) == (ref["nIn"], ref["nStereo"])
    assert np.array_equal(got["outliers"], ref["outliers"])
    assert np.array_equal(got["matches"], ref["matches"])
    assert np.array_equal(st2["rightIdxs"], ref["rightIdxs"]) and np.array_equal(st2["leftIdxs"], ref["leftIdxs"])
    assert np.array_equal(st2["close"], ref["close"])
    assert np.array_equal(st2["depth"].view(np.uint32), ref["depth"].view(np.uint32))


def assert_parity(got, st2, ref, spread, init_rel, case=None):
    tol = max(1e-9, 10 * spread)
    err = np.abs(got["T_cw"] - ref["T_cw"]).max()
    if case is not None and pc.two_factor(case):
        # two stereo factors fix five degrees of freedom: the two points in the camera frame are held to the 1e-9 of the
        # pose; the rotation about the line through them is set by the damping alone (pose_cases.two_factor_gauge_bound)
        R = got["T_cw"][:3, :3]
        assert np.abs(R.T @ R - np.eye(3)).max() < 1e-12 and np.array_equal(got["T_cw"][3], [0, 0, 0, 1])
        gauge, bound = pc.gauge_angle(got["T_cw"], ref["T_cw"]), pc.two_factor_gauge_bound(ref["initialError"], ref["iterations"])
        print("two factors: gauge angle %.2e rad (rounding bound %.1e), |dT| %.2e" % (gauge, bound, err))
        assert gauge <= bound
        err = np.abs(pc.factor_points_cam(case, got["T_cw"]) - pc.factor_points_cam(case, ref["T_cw"])).max()
    print("|dT| %.2e (bound %.1e)  initialError rel %.2e  lam %g" %
          (err, tol, abs(got["initialError"] - ref["initialError"]) / max(ref["initialError"], 1e-300), got["lam"]))
    assert abs(got["initialError"] - ref["initialError"]) <= init_rel * ref["initialError"]       # the factor list, before any step
    assert_decisions(got, st2, ref)
    assert abs(got["lam"] - ref["lam"]) <= 1e-12 * ref["lam"]
    assert err <= tol
    assert abs(got["finalError"] - ref["finalError"]) <= 1e-9 * max(1.0, ref["finalError"])


# ---- 1. the LM policy ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(pc.LM_CASES))
def test_lm_policy(oracle, capi, matcher, name):
    c = pc.lm_case(name)
    st, got, st2 = solve(capi, matcher, c)
    ref = pc.run_oracle(oracle, c, st)
    assert_parity(got, st2, ref, c["spread"], 1e-9)


# ---- 2. factor compaction ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,mask", pc.compact_ids())
def test_factor_compaction(oracle, capi, matcher, M, mask):
    c = pc.compact_case(M, mask)
    st, got, st2 = solve(capi, matcher, c)
    ref = pc.run_oracle(oracle, c, st)
    assert_parity(got, st2, ref, 0.0, 1e-10, case=c)


# ---- 3. the chi2 pass in isolation ---------------------------------------------------------------------------------------------
def assert_pass_only(c, got, st2, ref):
    """no factor: zero iterations, the pose back to the bit on both sides, everything else bit for bit"""
    for r in (got, ref):
        assert r["iterations"] == 0 and r["inner"] == 0 and r["initialError"] == 0
        assert np.array_equal(r["T_cw"].view(np.uint64), c["T0"].view(np.uint64))
    assert_decisions(got, st2, ref)


@pytest.mark.parametrize("kind,octave", sorted(pc.BOUND_OFFSETS))
def test_chi2_bound_alone(oracle, capi, matcher, kind, octave):
    """one point, on either side of the bound (M = 1: the smallest launch)"""
    for d, fails in zip(pc.BOUND_OFFSETS[(kind, octave)], (False, True)):
        c = pc.bound_probe(kind, octave, d)
        st, got, st2 = solve(capi, matcher, c)
        assert_pass_only(c, got, st2, pc.run_oracle(oracle, c, st))
        assert pc.bound_failed(kind, dict(close=st2["close"], outliers=got["outliers"]), c["key"]) == fails


def test_chi2_bounds(oracle, capi, matcher):
    c = pc.chi2_bounds_case()
    st, got, st2 = solve(capi, matcher, c)
    assert_pass_only(c, got, st2, pc.run_oracle(oracle, c, st))
    for i in c["excluded"]:
        assert got["outliers"][i] == c["out0"][i]


@pytest.mark.parametrize("fail", [True, False])
def test_shared_left_keys(oracle, capi, matcher, fail):
    c = pc.chain_case(pc.T_CHI2, fail=fail)
    st, got, st2 = solve(capi, matcher, c)
    assert_pass_only(c, got, st2, pc.run_oracle(oracle, c, st))
    assert (st2["close"][[ch["key"] for ch in c["chains"]]] == 0).all() == fail


# ---- 4. state kept on the matcher between calls --------------------------------------------------------------------------------
def _state_cases():
    cs = [pc.chain_case(pc.T_CHI2, fail=True, name="chains"), pc.chain_case(pc.T_CHI2, fail=False, name="chains-clean"),
          pc.chi2_bounds_case(), pc.compact_case(1, "all"), pc.compact_case(65, "alternate"), pc.compact_case(1024, "seventh"),
          pc.compact_case(1025, "all"), pc.compact_case(2049, "midtrip"), pc.compact_case(3073, "lane63")]
    return {c["name"]: c for c in cs}


def _snapshot(capi, m, c):
    st, got, st2 = solve(capi, m, c)
    out = {k: np.array(got[k]) for k in ("T_cw", "nIn", "nStereo", "matches", "outliers", "iterations", "inner", "initialError", "finalError", "lam")}
    out.update({"st_" + k: st2[k] for k in ("rightIdxs", "leftIdxs", "depth", "close")})
    return out


def test_state_across_calls(capi):
    """the same cases in increasing and in decreasing order of M and in an order that grows the pose buffers in the middle
    (1024 -> 1025, then back to small ones; a shared-key failure, then the same keys without one), each sequence on one
    matcher, against each case alone on a fresh matcher: every output identical, T_cw included (GPU against GPU)"""
    cases = _state_cases()
    alone = {n: _snapshot(capi, new_matcher(capi), c) for n, c in cases.items()}
    by_m = sorted(cases, key=lambda n: (len(cases[n]["points"]), n != "chains"))      # "chains" right before "chains-clean"
    assert by_m.index("chains-clean") == by_m.index("chains") + 1
    orders = [by_m, by_m[::-1],
              ["compact-1024-seventh", "compact-1025-all", "compact-1-all", "chains", "chains-clean", "chi2-bounds", "compact-3073-lane63",
               "chains-clean", "chains", "compact-65-alternate", "compact-2049-midtrip"]]
    for order in orders:
        m = new_matcher(capi)
        for n in order:
            got = _snapshot(capi, m, cases[n])
            for k, v in alone[n].items():
                same = np.array_equal(v.view(np.uint64), got[k].view(np.uint64)) if v.dtype == np.float64 else np.array_equal(
                    v.view(np.uint32), got[k].view(np.uint32)) if v.dtype == np.float32 else np.array_equal(v, got[k])
                assert same, (order, n, k)


# ---- 5. the IMU solve on the same helpers --------------------------------------------------------------------------------------
G = (0.0, 9.81, 0.0)
NOISE = (1.6968e-4, 1.9393e-5, 2.0e-3, 3.0e-3)      # gyro density, gyro walk, acc density, acc walk


def imu_solve_parity(oracle, capi, m, c, frame=6, gap=1, seed=1, bias=0.01):
    """the inputs, assertions and tolerances of tests/test_gpu_pose_imu.py::_imu_solve_parity on a crafted frame"""
    st = load_frame(m, c)
    fps = RIG["fps"]
    T_prev = synth.pose_at(frame - gap, fps)
    h = 1e-4
    v_prev = (synth.pose_at(frame - gap + h * fps, fps)[:3, 3] - synth.pose_at(frame - gap - h * fps, fps)[:3, 3]) / (2 * h)
    b_prev = np.full(6, bias) * np.array([1, -1, 0.5, 0.1, -0.1, 0.05])
    S, dts, _ = synth.imu_samples(frame - gap, frame, fps, noise_seed=seed + 1, bias=b_prev)
    ts = np.arange(len(dts)) * 5e6
    prm = oracle.imu_params(G, NOISE[0], NOISE[2], NOISE[1], NOISE[3], synth.T_BC1)
    ref = oracle.estimate_pose_imu(RIG, pc.INV_SIGMA, c["points"], c["inF"], c["inFR"], c["mpo"], c["matches"], c["out0"], c["kL"], c["kR"],
                                   st["rightIdxs"], st["leftIdxs"], st["depth"], st["close"], prm, T_prev, v_prev, b_prev, S, dts)
    got = capi.estimate_pose_imu(m, c["points"], c["inF"], c["inFR"], c["mpo"], c["matches"], c["out0"], G, NOISE, synth.T_BC1, T_prev,
                                 v_prev, b_prev, S[:, :3], S[:, 3:], ts, 200)
    assert ref["iterations"] >= 2
    assert (got["iterations"], got["inner"]) == (ref["iterations"], ref["inner"])
    assert np.abs(got["T_cw"] - ref["T_cw"]).max() < 1e-8
    assert np.abs(got["vel"] - ref["vel"]).max() < 1e-8 and np.abs(got["bias"] - ref["bias"]).max() < 1e-9
    assert abs(got["finalError"] - ref["finalError"]) <= 1e-8 * max(1.0, ref["finalError"])
    assert abs(got["initialError"] - ref["initialError"]) <= 1e-9 * max(1.0, ref["initialError"])
    assert (got["nIn"], got["nStereo"]) == (ref["nIn"], ref["nStereo"])
    assert np.array_equal(got["outliers"], ref["outliers"]) and np.array_equal(got["matches"], ref["matches"])
    st2 = m.stereo_fetch(len(c["kL"]), len(c["kR"]))
    for k in ("rightIdxs", "leftIdxs", "close"):
        assert np.array_equal(st2[k], ref[k])
    assert np.array_equal(st2["depth"].view(np.uint32), ref["depth"].view(np.uint32))
    return ref


IMU_SIZES = (1025, pc.IMU_LDS_FACTORS, pc.IMU_LDS_FACTORS + 1, 3073)
IMU_MASKS = ("lane0", "lane63", "wave3", "alternate", "seventh", "midtrip", "ends")


@pytest.mark.parametrize("M,mask", [(M, k) for M in IMU_SIZES for k in IMU_MASKS if pc.mask_keep(M, k) is not None])
def test_imu_solve_sparse_factors(oracle, capi, matcher, M, mask):
    """the sparse masks on both sides of the IMU kernel's LDS / HBM factor buffer threshold"""
    imu_solve_parity(oracle, capi, matcher, pc.compact_case(M, mask, pc.scene_pose()))


def test_imu_solve_shared_left_keys(oracle, capi, matcher):
    """the chains through the IMU solve: here the LM runs, every residual is unambiguous (exact, or 20 px off)"""
    c = pc.chain_case(pc.scene_pose(), fail=True, mpo=0)
    ref = imu_solve_parity(oracle, capi, matcher, c)
    assert (ref["close"][[ch["key"] for ch in c["chains"]]] == 0).all()
    for ch in c["chains"]:
        assert ref["matches"][ch["first_fail"], 1] == -1 and ref["leftIdxs"][ch["own"]] == -1


# ---- 6. worldToFrame at its edges ----------------------------------------------------------------------------------------------
def test_world_to_frame_edges(oracle, capi, matcher):
    pts, msd, n_edge, edges = pc.w2f_case(oracle)
    T = np.eye(4)
    uL, vL, lL, visL = oracle.world_to_frame(RIG, T, False, pts, msd, pc.LOG_SCALE)
    uR, vR, lR, visR = oracle.world_to_frame(RIG, T, True, pts, msd, pc.LOG_SCALE)
    pl, pr, ll, lr, vf, vr = capi.world_to_frame(matcher, T, pts, msd, pc.LOG_SCALE)
    assert np.array_equal(vf, visL) and np.array_equal(vr, visR)
    a, b = visL != 0, visR != 0                                     # pixel and level are written for a visible point only
    assert np.array_equal(pl[a, 0].view(np.uint32), uL[a].view(np.uint32)) and np.array_equal(pl[a, 1].view(np.uint32), vL[a].view(np.uint32))
    assert np.array_equal(pr[b, 0].view(np.uint32), uR[b].view(np.uint32)) and np.array_equal(pr[b, 1].view(np.uint32), vR[b].view(np.uint32))
    assert np.array_equal(ll[a], lL[a]) and np.array_equal(lr[b], lR[b])
    assert not pl[~a].any() and not pr[~b].any() and not ll[~a].any() and not lr[~b].any()
