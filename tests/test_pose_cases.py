"""CPU checks of the crafted pose-solve cases (tests/pose_cases.py): every case is run through the oracle and must reach
the branch it is meant for, and its reference decisions must not depend on the order in which the map points are summed -
the GPU test (tests/test_gpu_pose_crafted.py) holds the kernel to them exactly.  Run with -s for the per-case figures.

Branches of levenbergMarquardtX (oracle/vo_pose.cpp) and how they are reached:
  rejected step, lambda *= 10, inner > iterations .... LM_CASES "rejected" / "wrong-minimum"
  exit at lambda >= 1e5 .............................. "lambda-bound" (with and without an accepted step before)
  stop (|costChange| < relTol * error, step refused) . "stop": every point behind the camera, zero Jacobian, 0 / 0
  P.solve returns false ............................... "cholesky-fails": a NaN pivot at every lambda (first_lm_step shows it:
                                                        the oracle's report alone cannot tell it from ten rejections)
  solved with linChange < 0 ........................... NOT REACHED by an admissible case.  linChange = 0.5 d'(H + 2 lambda I)d
      is negative only as rounding noise of an ill-conditioned solve: a search over 59 000 near-centre points (z 1e-150 ..
      0.1, x and y up to 100 z) gave one hit, at lambda = 1e3 only, whose sign changed with the order of the map points.
      The kernel takes the same branch (sEval stays 0) for a failed solve, which IS covered.
"""
import os
import re
import numpy as np
import pytest
import pose_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PERM = 8


def admissible(oracle, case, st, ref, label):
    """the oracle's decisions on N_PERM random orders of the map points are those of the case's own order; returns the
    spread of T_cw over them - for a two-factor case (pose_cases.two_factor: the pose has a free rotation) the spread of
    what the data determines, the two factor points in the camera frame"""
    rng = np.random.Generator(np.random.PCG64(99))
    M = len(case["points"])
    spread = 0.0
    two = pc.two_factor(case)
    for _ in range(N_PERM):
        r = pc.run_oracle(oracle, case, st, perm=rng.permutation(M))
        assert (r["iterations"], r["inner"]) == (ref["iterations"], ref["inner"]), label
        assert (r["nIn"], r["nStereo"]) == (ref["nIn"], ref["nStereo"]), label
        assert np.array_equal(r["outliers"], ref["outliers"]) and np.array_equal(r["matches"], ref["matches"]), label
        for k in ("rightIdxs", "leftIdxs", "close"):
            assert np.array_equal(r[k], ref[k]), label
        if two:
            spread = max(spread, float(np.abs(pc.factor_points_cam(case, r["T_cw"]) - pc.factor_points_cam(case, ref["T_cw"])).max()))
        else:
            spread = max(spread, float(np.abs(r["T_cw"] - ref["T_cw"]).max()))
    assert spread <= 1e-8, (label, spread)
    return spread


def test_kernel_constants():
    """the shapes of section 2 are derived from these: if one changes, the sizes and masks need revisiting"""
    src = open(os.path.join(ROOT, "gtsam-vslam_amd", "csrc", "pose_dev.hpp")).read()
    assert int(re.search(r"constexpr int POSE_NT = (\d+);", src).group(1)) == 256 == pc.POSE_NT
    assert int(re.search(r"constexpr int POSE_BATCH = (\d+);", src).group(1)) == 4 == pc.POSE_BATCH
    imu = open(os.path.join(ROOT, "gtsam-vslam_amd", "csrc", "pose_imu.hip")).read()
    assert int(re.search(r"constexpr int POSE_IMU_LDS_FACTORS = (\d+);", imu).group(1)) == 2125 == pc.IMU_LDS_FACTORS
    assert pc.TRIP == 1024
    for edge in (64, 256, 1024, 2048):
        assert {edge - 1, edge, edge + 1} <= set(pc.COMPACT_SIZES)
    assert 3 * pc.TRIP + 1 in pc.COMPACT_SIZES                      # a fourth trip: the double-buffered table is reused twice


def test_level_table(oracle):
    assert np.array_equal(oracle.Extractor(1500).InvSigmaFactor, pc.INV_SIGMA)
    assert pc.CLOSE_TH == float(np.float32(pc.RIG["bl"]) * np.float32(40))


# ---- section 1 -----------------------------------------------------------------------------------------------------------------
_LM = {}


def _lm(oracle, name):
    if name not in _LM:
        c = pc.lm_case(name)
        st = pc.frame_state(oracle, c)
        ref = pc.run_oracle(oracle, c, st)
        _LM[name] = (c, st, ref, admissible(oracle, c, st, ref, name))
    return _LM[name]


@pytest.mark.parametrize("name", sorted(pc.LM_CASES))
def test_lm_case(oracle, name):
    c, st, ref, spread = _lm(oracle, name)
    M = len(c["points"])
    it, inner, lam = ref["iterations"], ref["inner"], ref["lam"]
    print("\n%-20s %-15s (iterations, inner, lam) = (%d, %d, %.0e)  nIn %d / %d  spread %.1e" % (name, c["branch"], it, inner, lam, ref["nIn"], M, spread))
    assert abs(spread - c["spread"]) <= 5e-4 * c["spread"] and c["spread"] <= 1e-8      # the table holds the measured figure
    assert np.isfinite(ref["initialError"]) and ref["initialError"] > 0
    nL = c["n_keys"][0]
    assert (st["rightIdxs"][:nL][c["best"][:nL] >= 0] >= 0).all()   # every key kept its pair through the finalize cuts
    b = c["branch"]
    if b == "rejected":
        assert inner > it >= 8 and lam < 1e5 and ref["nIn"] == M
    elif b == "wrong-minimum":
        assert inner > it and lam < 1e5 and ref["nIn"] < M
    elif b == "lambda-bound":
        assert lam >= 1e5 and inner >= it + 10
    elif b == "stop":
        assert (it, inner, lam) == (0, 0, 1e-5) and ref["finalError"] == ref["initialError"] and ref["nIn"] == 0
        assert np.abs(ref["T_cw"] - c["T0"]).max() < 1e-12
    elif b == "accepted":
        assert inner == it >= 4 and ref["nIn"] == M
    elif b == "cholesky-fails":
        assert (it, inner, lam) == (0, 10, 1e5) and ref["finalError"] == ref["initialError"]
        with np.errstate(all="ignore"):
            for k in range(10):                                     # not one of the ten solves succeeds
                assert pc.first_lm_step(c, st, 1e-5 * 10.0 ** k) == ("cholesky-fails", None)
    else:
        raise AssertionError(b)


def test_lm_set(oracle):
    """what the set must contain"""
    refs = {n: _lm(oracle, n) for n in pc.LM_CASES}
    rej = [n for n, (c, st, r, s) in refs.items() if r["inner"] > r["iterations"] and r["nIn"] == len(c["points"])]
    bound = [n for n, (c, st, r, s) in refs.items() if r["lam"] >= 1e5]
    stop = [n for n, (c, st, r, s) in refs.items() if r["iterations"] == 0 and r["inner"] == 0 and r["initialError"] > 0]
    acc = [n for n, (c, st, r, s) in refs.items() if r["inner"] == r["iterations"] >= 8]
    assert len(rej) >= 2 and len(bound) >= 2 and len(stop) >= 1 and len(acc) >= 1
    assert {len(c["points"]) for c, _, _, _ in refs.values()} >= {6, 40, 300}
    lams = [r["lam"] for _, _, r, _ in refs.values()]
    assert min(lams) <= 1e-16                                       # an accepted-only run drives lambda that far down


def test_well_conditioned_first_step_is_solved(oracle):
    """the restatement used above agrees with the oracle where a solve succeeds: an accepted first step has linChange > 0"""
    c = pc.lm_case("m7-cholesky-fails")
    c["points"] = c["points"][:-1]
    for k in ("matches", "inF", "inFR", "mpo", "out0"):
        c[k] = c[k][:-1]
    st = pc.frame_state(oracle, c)
    kind, lin = pc.first_lm_step(c, st)
    ref = pc.run_oracle(oracle, c, st)
    assert kind == "solved" and lin > 0 and ref["iterations"] == ref["inner"] >= 3 and ref["nIn"] == 6


# ---- section 2 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,mask", pc.compact_ids())
def test_compact_case(oracle, M, mask):
    c = pc.compact_case(M, mask)
    st = pc.frame_state(oracle, c)
    ref = pc.run_oracle(oracle, c, st)
    f = pc.factor_points(c)
    assert np.array_equal(f, np.nonzero(c["keep"])[0])              # exactly the mask's points carry a factor
    spread = admissible(oracle, c, st, ref, c["name"])
    # the GPU test's flat 1e-9 is at least 10 x the reference's own spread - of T_cw, or for the two cases with two factors
    # (both stereo: five of six degrees of freedom) of the two points in the camera frame
    assert spread <= 1e-10, (c["name"], spread)
    assert pc.two_factor(c) == ((M, mask) in ((65, "lane0"), (3073, "ends")))
    if pc.two_factor(c):
        assert (c["kind"][f] == pc.STEREO).all() and (st["close"][f] != 0).all() and (c["matches"][f] == f[:, None]).all()
        assert ref["iterations"] <= 4
        print("\n%-22s two factors: gauge rounding bound %.1e rad" % (c["name"], pc.two_factor_gauge_bound(ref["initialError"], ref["iterations"])))
    assert ref["iterations"] == ref["inner"]                        # a benign solve from 0.05 rad, 0.1 m
    gone = np.nonzero(~c["keep"])[0]
    if len(gone) >= 5:                                              # all five ways of removing a point occur
        m = c["matches"][gone]
        assert c["mpo"][gone].any() and c["out0"][gone].any() and (m == -1).all(axis=1).any()
        assert ((m[:, 0] >= 0) & (c["inF"][gone] == 0)).any() and ((m[:, 0] < 0) & (m[:, 1] >= 0) & (c["inFR"][gone] == 0)).any()
    if len(f) >= 40:                                                # all three factor types occur
        m = c["matches"][f]
        stereo = (m[:, 0] >= 0) & (m[:, 1] >= 0) & (st["close"][np.maximum(m[:, 0], 0)] != 0)
        lost = (m[:, 0] >= 0) & (m[:, 1] < 0) & (st["close"][np.maximum(m[:, 0], 0)] != 0)
        assert stereo.any() and lost.any() and (m[:, 0] < 0).any() and ((m[:, 0] >= 0) & ~stereo).any()
    # sharpness: taking any one factor away moves the initial error by four orders more than the GPU test tolerates
    worst = np.inf
    sample = pc.boundary_sample(c)
    lane, wave, trip = f % 64, f // 64, f // pc.TRIP
    for w in np.unique(wave):
        assert {f[wave == w][0], f[wave == w][-1]} <= set(sample)
    for t in np.unique(trip):
        assert {f[trip == t][0], f[trip == t][-1]} <= set(sample)
    for i in sample:
        mpo = c["mpo"].copy(); mpo[i] = 1
        e = pc.run_oracle(oracle, c, st, mpo=mpo)["initialError"]
        drop = (ref["initialError"] - e) / ref["initialError"]
        assert drop >= 1e-6, (c["name"], i, drop)
        worst = min(worst, drop)
    if len(f) == 0:
        assert ref["initialError"] == 0 and ref["iterations"] == 0
    print("\n%-22s factors %4d  (iterations, inner, lam) = (%d, %d, %.0e)  nIn %d nStereo %d  spread %.1e  smallest leave-one-out %.1e"
          % (c["name"], len(f), ref["iterations"], ref["inner"], ref["lam"], ref["nIn"], ref["nStereo"], spread, worst))


def test_compact_masks_reach_the_edges():
    k = pc.mask_keep(3073, "midtrip")
    assert k[:1024].all() and not k[1024:2048].any() and k[2048:].all()
    assert list(np.nonzero(pc.mask_keep(3073, "ends"))[0]) == [0, 3072]
    assert list(np.nonzero(pc.mask_keep(257, "lane63"))[0]) == [63, 127, 191, 255]
    assert list(np.nonzero(pc.mask_keep(257, "lane0"))[0]) == [0, 64, 128, 192, 256]
    assert list(np.nonzero(pc.mask_keep(1025, "wave3"))[0][[0, -1]]) == [192, 1023]
    assert not pc.mask_keep(63, "lane63").any() and not pc.mask_keep(65, "wave3").any()      # solves without any factor


# ---- section 3 -----------------------------------------------------------------------------------------------------------------
def _pass_only(ref, case):
    """no factor: the LM does not run, the pose comes back to the bit"""
    assert ref["iterations"] == 0 and ref["inner"] == 0 and ref["initialError"] == 0
    assert np.array_equal(ref["T_cw"].view(np.uint64), case["T0"].view(np.uint64))


@pytest.mark.parametrize("kind,octave", sorted(pc.BOUND_OFFSETS))
def test_bound_offsets(oracle, kind, octave):
    """the recorded offsets are the bisection's, adjacent doubles, one on either side of the oracle's decision"""
    d_in, d_out = pc.bound_bisect(oracle, kind, octave)
    assert (d_in, d_out) == pc.BOUND_OFFSETS[(kind, octave)] and np.nextafter(d_in, np.inf) == d_out
    r = pc.bound_radius(octave) * (0.5 if kind == "stereo_right" else 1.0)
    assert abs(d_in - r) < 1e-5 * r                                 # and they sit at sqrt(7.815 / InvSigmaFactor)
    for d, fails in ((d_in, False), (d_out, True)):
        c = pc.bound_probe(kind, octave, d)
        ref = pc.run_oracle(oracle, c)
        _pass_only(ref, c)
        assert pc.bound_failed(kind, ref, c["key"]) == fails
    print("\nbound %-12s octave %d: inlier up to %s (%.13f px), outlier from %s" % (kind, octave, d_in.hex(), d_in, d_out.hex()))


def test_chi2_bounds_case(oracle):
    c = pc.chi2_bounds_case()
    st = pc.frame_state(oracle, c)
    ref = pc.run_oracle(oracle, c, st)
    _pass_only(ref, c)
    assert len(c["expect"]) == 12
    for i, (kind, k, fails) in c["expect"].items():
        if kind == "stereo_right":
            assert st["close"][k] == 1 and ref["outliers"][i] == 0
            assert (ref["close"][k] == 0) == fails and (ref["matches"][i, 1] == -1) == fails
        else:
            assert ref["outliers"][i] == int(fails)
    # the depth bound: exactly float32(baseline) * 40 is not close any more
    zs = sorted(z for _, z in c["depth_pts"].values())
    assert zs[1] == pc.CLOSE_TH and np.nextafter(zs[0], np.inf) == zs[1] and np.nextafter(zs[1], np.inf) == zs[2]
    for i, (k, z) in c["depth_pts"].items():
        assert (c["T0"][:3, :3] @ c["points"][i] + c["T0"][:3, 3])[2] == z       # the pass sees that depth to the bit
        assert st["close"][k] == 1 and ref["outliers"][i] == 0
        assert (ref["close"][k] == 0) == (z < pc.CLOSE_TH)
        assert (ref["matches"][i, 1] == -1) == (z < pc.CLOSE_TH)
    for i in c["behind"]:
        assert ref["outliers"][i] == 1
    assert sorted((c["T0"][:3, :3] @ c["points"][i] + c["T0"][:3, 3])[2] for i in c["behind"]) == [-1.0, 0.0]
    for i in c["excluded"]:
        assert ref["outliers"][i] == c["out0"][i]
    assert {int(c["out0"][i]) for i in c["excluded"]} == {0, 1}
    print("\nchi2-bounds: nIn %d nStereo %d, %d of %d flagged" % (ref["nIn"], ref["nStereo"], int(ref["outliers"].sum()), len(ref["outliers"])))


def test_chain_case(oracle):
    """shared left keys: what the oracle does with each chain, spelled out"""
    c = pc.chain_case(pc.T_CHI2)
    clean = pc.chain_case(pc.T_CHI2, fail=False)
    st = pc.frame_state(oracle, c)
    ref = pc.run_oracle(oracle, c, st)
    st0 = pc.frame_state(oracle, clean)
    ref0 = pc.run_oracle(oracle, clean, st0)
    _pass_only(ref, c); _pass_only(ref0, clean)
    for k in ("rightIdxs", "leftIdxs", "close", "depth"):
        assert np.array_equal(st[k], st0[k]) and np.array_equal(ref0[k], st0[k])             # nothing fails: nothing changes
    assert np.array_equal(ref0["matches"], clean["matches"])
    assert ref["nIn"] == ref0["nIn"] == pc.CHAIN_M and not ref["outliers"].any()
    n_chain = sum(len(ch["order"]) for ch in c["chains"])
    assert ref0["nStereo"] == c["n_filler_stereo"] + n_chain
    lost = 0
    for ch in c["chains"]:
        k, f, order = ch["key"], ch["first_fail"], ch["order"]
        assert st["close"][k] == 1 and st["rightIdxs"][k] == ch["own"] and st["leftIdxs"][ch["own"]] == k
        lost += len(order) - order.index(f)                          # only the members before the first failure count as stereo
        assert ref["close"][k] == 0 and ref["rightIdxs"][k] == -1 and ref["depth"][k] == -1 and ref["leftIdxs"][ch["own"]] == -1
        for i in order:
            assert ref["matches"][i, 0] == k
            assert ref["matches"][i, 1] == (-1 if i == f else ch["rks"][i])
        if ch["other"] is not None:                                  # the failing match's own right key keeps its left partner
            assert ch["rks"][f] != ch["own"] and ref["leftIdxs"][ch["rks"][f]] == ch["other"] and ref["rightIdxs"][ch["other"]] == ch["rks"][f]
    assert ref["nStereo"] == ref0["nStereo"] - lost
    # the members of the chains sit in different threads, waves, slots of a thread and trips
    spans = [np.array(ch["order"]) for ch in c["chains"]]
    assert any(len(set(s // pc.TRIP)) > 1 for s in spans) and any(len(set(s % 256 // 64)) > 1 for s in spans)
    assert any({1023, 1024} <= set(s) for s in spans) and any(len(s) == 8 for s in spans)
    assert any(len([j for j in pc.CHAINS[n]["fail"]]) == 2 for n in range(len(spans)))
    print("\nchains: nStereo %d (all inliers: %d), %d keys lose their pair" % (ref["nStereo"], ref0["nStereo"], len(spans)))


# ---- section 6 -----------------------------------------------------------------------------------------------------------------
def test_w2f_case(oracle):
    pts, msd, n_edge, edges = pc.w2f_case(oracle)
    assert len(edges) == 16 and (msd > 0).all()
    lv = {}
    for right in (False, True):
        u, v, lvl, vis = oracle.world_to_frame(pc.RIG, np.eye(4), right, pts, msd, pc.LOG_SCALE)
        lv[right] = (lvl, vis)
        for r, a, b in edges:
            assert np.nextafter(a, np.inf) == b
        e = vis[:n_edge]
        assert 0 < e.sum() < n_edge
        assert set(lvl[n_edge:][vis[n_edge:] != 0]) == set(range(8))       # every level, both clamps included
    # the edge points come in fours around the oracle's decision: (x, a | b, x) - the decision flips between a and b only
    for q in range(16):
        right = edges[q][0]
        vis = lv[right][1][4 * q:4 * q + 4]
        assert vis[0] == vis[1] != vis[2] == vis[3]
    print("\nworld_to_frame: %d points, %d at the image edges" % (len(pts), n_edge))
