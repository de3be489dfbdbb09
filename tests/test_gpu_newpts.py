"""GPU parity of the new-point pipeline (calcAllMpsOfKFROnlyEst -> predictKeysPosR -> matchByProjectionRPredLBA ->
triangulateNewPoints -> checkReprojError) and of MapPoint::calcDescriptor: HIP through the C ABI vs the CPU oracle.
Candidate lists, match triples and accept flags bit-exact; triangulated positions within 1e-9 relative."""
import numpy as np
import pytest
import synth
import newpts_cases as nc

pytestmark = pytest.mark.gpu


def _window(oracle, frames, seed=0, mp_frac=0.3, rig_name="euroc", nfeat=1500):
    rig = synth.RIGS[rig_name]
    rng = np.random.default_rng(seed)
    oL, oR = oracle.Extractor(nfeat), oracle.Extractor(nfeat)
    kfs = []
    for f in frames:
        L, R, T = synth.stereo_frame(f, rig_name)
        kL, dL = oL.extract(L); kR, dR = oR.extract(R)
        st = oracle.stereo_match(oL, oR, rig, kL, dL, kR, dR)
        unF = np.where(rng.random(len(kL)) < 0.2, rng.integers(0, 1000, len(kL)), -1).astype(np.int32)
        unFR = np.where(rng.random(len(kR)) < 0.2, rng.integers(0, 1000, len(kR)), -1).astype(np.int32)
        kfs.append(dict(T_wc=T, id=f, kpsL=kL, descL=dL, kpsR=kR, descR=dR, rightIdxs=st["rightIdxs"], leftIdxs=st["leftIdxs"],
                        unF=unF, unFR=unFR, depth=st["depth"]))
    k0 = kfs[0]
    n0 = len(k0["kpsL"])
    has = (rng.random(n0) < mp_frac).astype(np.uint8)
    mpx = np.zeros((n0, 3)); mpd = np.zeros((n0, 32), np.uint8)
    T = k0["T_wc"]
    for i in range(n0):
        z = float(k0["depth"][i]) if k0["depth"][i] > 0 else rng.uniform(2, 8)
        pc = np.array([(k0["kpsL"]["x"][i] - rig["cx"]) * z / rig["fx"], (k0["kpsL"]["y"][i] - rig["cy"]) * z / rig["fy"], z])
        mpx[i] = T[:3, :3] @ pc + T[:3, 3] + rng.normal(0, 0.01, 3)
        d = k0["descL"][i].copy()
        for b in rng.integers(0, 256, 6):
            d[b >> 3] ^= np.uint8(1 << (b & 7))
        mpd[i] = d
    last = dict(depth=k0["depth"], hasMp=has, mpXyz=mpx, mpDesc=mpd)
    return rig, oL, kfs, last


@pytest.mark.parametrize("frames,seed", [((30, 24, 18, 12, 6), 0), ((20, 14, 8, 20, 2), 1), ((9,), 2)])
def test_find_new_points_parity(oracle, capi, frames, seed):
    _find_new_points_parity(oracle, capi, frames, seed)


def _find_new_points_parity(oracle, capi, frames, seed, rig_name="euroc", nfeat=1500):
    rig, oL, kfs, last = _window(oracle, frames, seed, rig_name=rig_name, nfeat=nfeat)
    ref = oracle.find_new_points(oL, rig, kfs, last)
    got = capi.find_new_points(rig, oL.scalePyramid, oL.sigmaFactor, kfs, last)
    assert got["n"] == ref["n"] and ref["n"] > 300
    assert np.array_equal(got["candL"], ref["candL"]) and np.array_equal(got["candR"], ref["candR"])
    assert np.array_equal(got["nObs"], ref["nObs"])
    assert np.array_equal(got["obs"], ref["obs"])
    assert np.array_equal(got["accepted"], ref["accepted"])
    a = ref["accepted"] > 0
    if len(frames) >= 5:
        assert a.sum() > 20                      # the window really produces new points
        scale = np.maximum(1.0, np.abs(ref["xyz"][a]).max(axis=1))
        assert (np.abs(got["xyz"][a] - ref["xyz"][a]).max(axis=1) / scale).max() < 1e-9
        # the new points lie where the scene is: their reprojection into lastKF matches the keypoint within a few px
        T = np.linalg.inv(kfs[0]["T_wc"])
        pc = (T[:3, :3] @ ref["xyz"][a].T).T + T[:3, 3]
        u = rig["fx"] * pc[:, 0] / pc[:, 2] + rig["cx"]
        assert np.abs(u - kfs[0]["kpsL"]["x"][ref["candL"][a]]).max() < 12.0
    else:
        assert a.sum() == 0


def test_calc_descriptor_parity(oracle, capi):
    rng = np.random.default_rng(5)
    lists = []
    for n in (1, 2, 3, 4, 7, 16, 33, 64, 5, 0, 9, 65, 130, 3, 257):        # > 64 observations: the histogram kernel
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        d = np.repeat(base[None], n, 0)
        for i in range(n):
            for b in rng.integers(0, 256, rng.integers(0, 40)):
                d[i, b >> 3] ^= np.uint8(1 << (b & 7))
        if n >= 4:
            d[1] = d[0]                          # exact duplicates: ties resolved by the first minimum
        lists.append(d)
    got = capi.calc_descriptors(lists)
    ref = [oracle.calc_descriptor(d) if len(d) else -1 for d in lists]
    assert list(got) == ref
    assert capi.calc_descriptors([np.zeros((65, 32), np.uint8)])[0] == 0         # all equal: the first one


def test_mono_map_point_creation_parity(oracle, capi):
    """vslam_mono_new_points (calculateMPFromMono + mono checkReprojError) vs the oracle: identical accept flags, view
    filters and counts; positions to 1e-9 relative (same DLT / Jacobi-SVD operation order, no FMA contraction)."""
    import synth
    sf = np.array([1.2 ** (2 * i) for i in range(8)], np.float32)
    for kw in (dict(), dict(n_kf=10, n_points=1500, seed=5, trans_sigma=0.05), dict(n_kf=2, n_points=70, seed=9, outlier_frac=0.3)):
        pr = synth.make_mono_points_problem(**kw)
        args = (pr["rig"], sf, pr["kf_pose"], pr["kf_id"], pr["n_views"], pr["view_kf"], pr["view_xy"], pr["view_oct"])
        ref, got = oracle.mono_new_points(*args), capi.mono_new_points(*args)
        assert np.array_equal(got["accepted"], ref["accepted"]) and ref["accepted"].sum() > 5
        assert np.array_equal(got["nObs"], ref["nObs"]) and np.array_equal(got["keep"], ref["keep"])
        m = ref["accepted"] > 0
        assert np.abs(got["xyz"][m] - ref["xyz"][m]).max() <= 1e-9 * np.abs(ref["xyz"][m]).max()


def test_keyframe_update_pose_parity(oracle, capi):
    """vslam_keyframe_update_pose (KeyFrame::updatePose) vs the oracle: identical drop flags, bit-identical moved
    landmarks and new pose."""
    import synth
    from test_oracle_newpts import _kf_update_args
    for kw in (dict(), dict(shift=0.3, seed=5, n_left=700, n_right=0), dict(seed=9, n_left=0, n_right=300, n_lm=400)):
        pr = synth.make_kf_update_problem(**kw)
        ref = oracle.keyframe_update_pose(*_kf_update_args(oracle, pr))
        got = capi.keyframe_update_pose(*_kf_update_args(capi, pr))
        assert np.array_equal(got["dropL"], ref["dropL"]) and np.array_equal(got["dropR"], ref["dropR"])
        assert np.array_equal(got["lm"], ref["lm"]) and np.array_equal(got["pose"], ref["pose"])


# ---- crafted windows (tests/newpts_cases.py; tests/test_oracle_newpts.py proves on the CPU that each is in its regime) ----------
def _assert_same(got, ref, what):
    """the bar of test_find_new_points_parity: everything bit-exact, accepted positions within 1e-9 relative"""
    assert got["n"] == ref["n"], what
    for f in ("candL", "candR", "nObs", "obs", "accepted"):
        assert np.array_equal(got[f], ref[f]), (what, f, np.nonzero(np.asarray(got[f] != ref[f]).reshape(len(ref[f]), -1).any(1))[0][:8])
    a = ref["accepted"] > 0
    if a.any():
        scale = np.maximum(1.0, np.abs(ref["xyz"][a]).max(axis=1))
        assert (np.abs(got["xyz"][a] - ref["xyz"][a]).max(axis=1) / scale).max() < 1e-9, what


def _crafted_parity(oracle, capi, c):
    ref = oracle.find_new_points(c.ex, c.g.rig, c.kfs, c.last)
    got = capi.find_new_points(c.g.rig, c.ex.scalePyramid, c.ex.sigmaFactor, c.kfs, c.last)
    _assert_same(got, ref, c.name)
    assert got["n"] == len(c.cands)
    # what the case guarantees: its accepted and rejected probes, each with the outcome it was built for
    assert int(got["accepted"].sum()) >= c.min_accepted and int((got["accepted"] == 0).sum()) >= c.min_rejected
    for name, f in c.finals.items():
        ci = c.probes[name]["cand"]
        assert got["accepted"][ci] == f["accepted"] and got["nObs"][ci] == f["nObs"], (c.name, name)
    for name, p in c.probes.items():
        if p["kf"] is not None and p["expect"].get("verdict", "").startswith("matched"):
            assert got["nObs"][p["cand"]] == 2 and got["obs"][p["cand"]][1].tolist() == [p["kf"]] + list(c.pairs[p["cand"]][p["kf"]]["out"]), (c.name, name)
        elif p["kf"] is not None:
            assert got["nObs"][p["cand"]] == 1, (c.name, name)
    return ref, got


@pytest.mark.parametrize("rig_name", nc.RIG_NAMES)
@pytest.mark.parametrize("name", list(nc.ALL_CASES))
def test_crafted_window_parity(oracle, capi, name, rig_name):
    _crafted_parity(oracle, capi, nc.get(oracle, name, rig_name))


@pytest.mark.parametrize("name", list(nc.PORTRAIT_CASES))
def test_portrait_window_parity(oracle, capi, name):
    """480 x 752: 101 grid rows, so the keys of rows >= 64 have cell indices beyond 4095 (more than 12 bits)"""
    _crafted_parity(oracle, capi, nc.get(oracle, name, "portrait"))


@pytest.mark.parametrize("rig_name", nc.RIG_NAMES)
def test_batch_of_unequal_lanes(oracle, capi, rig_name):
    """one vslam_find_new_points_batch call, lanes of n_left 0 / 70 / 1025 and n_kf 1 / 5 / 16: the grids are sized by the
    largest lane, the small lanes ignore the excess blocks; each lane equals its own single call and the oracle"""
    lanes = [nc.get(oracle, n, rig_name) for n in ("empty_last", "skip_mid_70", "row_counts_1025")]
    wins = [(c.kfs[:1] if c.name == "empty_last" else c.kfs, c.last) for c in lanes]
    assert [len(k[0]["kpsL"]) for k, _ in wins] == [0, 70, 1025] and [len(k) for k, _ in wins] == [1, 5, 16]
    ex, rig = lanes[0].ex, lanes[0].g.rig
    got = capi.find_new_points_batch(rig, ex.scalePyramid, ex.sigmaFactor, wins)
    for c, (kfs, last), g in zip(lanes, wins, got):
        one = capi.find_new_points(rig, ex.scalePyramid, ex.sigmaFactor, kfs, last)
        for f in ("n", "candL", "candR", "nObs", "obs", "accepted", "xyz"):
            assert np.array_equal(g[f], one[f]), (c.name, f)
        _assert_same(g, oracle.find_new_points(ex, rig, kfs, last), c.name)
    assert got[0]["n"] == 0 and got[1]["accepted"].sum() == 10 and got[2]["accepted"].sum() == 36
    # the lanes in another order: the largest first
    rev = capi.find_new_points_batch(rig, ex.scalePyramid, ex.sigmaFactor, wins[::-1])[::-1]
    for a, b in zip(got, rev):
        for f in ("n", "candL", "candR", "nObs", "obs", "accepted", "xyz"):
            assert np.array_equal(a[f], b[f])


def test_resident_keyframes_equal_host_keyframes(oracle, capi):
    """keyframes 1 and 3 of a five-keyframe window uploaded once (vslam_kf_keys_upload) and passed as device_keys, their
    host arrays still given for unF / unFR: the result is the all-host call's"""
    import torch
    c = nc.get(oracle, "skip_mid_70", "euroc")
    host = capi.find_new_points(c.g.rig, c.ex.scalePyramid, c.ex.sigmaFactor, c.kfs, c.last)
    blocks = {}
    for k in (1, 3):
        nb = capi.kf_keys_bytes(len(c.kfs[k]["kpsL"]), len(c.kfs[k]["kpsR"]))
        assert nb >= 28 * (len(c.kfs[k]["kpsL"]) + len(c.kfs[k]["kpsR"])) + 36 * (len(c.kfs[k]["kpsL"]) + len(c.kfs[k]["kpsR"]))
        blocks[k] = torch.zeros(nb, dtype=torch.uint8, device="cuda")
        capi.kf_keys_upload(c.kfs[k], blocks[k].data_ptr())
    torch.cuda.synchronize()
    # the host copies of the immutable arrays of a resident keyframe are not read: scramble them
    kfs = [dict(k) for k in c.kfs]
    for k in (1, 3):
        kfs[k]["descL"] = np.zeros_like(kfs[k]["descL"]); kfs[k]["descR"] = np.zeros_like(kfs[k]["descR"])
    res = capi.find_new_points(c.g.rig, c.ex.scalePyramid, c.ex.sigmaFactor, kfs, c.last, device_keys={k: b.data_ptr() for k, b in blocks.items()})
    for f in ("n", "candL", "candR", "nObs", "obs", "accepted", "xyz"):
        assert np.array_equal(res[f], host[f]), f
    assert res["accepted"].sum() == 10
    _assert_same(res, oracle.find_new_points(c.ex, c.g.rig, c.kfs, c.last), "resident")


def test_new_points_argument_checks(oracle, capi):
    """more than 16 keyframes and none are rejected before any launch; a result capacity below the candidate count is
    reported after the search (whose own buffers are sized by the last keyframe's key count) with n_candidates set and
    nothing written to the caller's arrays"""
    c = nc.get(oracle, "chunk_1025_65", "euroc")
    args = (c.g.rig, c.ex.scalePyramid, c.ex.sigmaFactor)
    with pytest.raises(capi.VslamError) as e:
        capi.find_new_points(*args, [c.kfs[0]] + [c.kfs[1]] * 16, c.last)
    assert e.value.status == capi.ERR_INVALID
    with pytest.raises(capi.VslamError) as e:
        capi.find_new_points(*args, c.kfs, c.last, n_kf=0)
    assert e.value.status == capi.ERR_INVALID
    with pytest.raises(capi.VslamError) as e:
        capi.find_new_points(*args, c.kfs, c.last, capacity=64)
    assert e.value.status == capi.ERR_CAPACITY and e.value.n_candidates == 65
    assert capi.find_new_points(*args, c.kfs, c.last, capacity=65)["n"] == 65
