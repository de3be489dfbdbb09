"""Crafted inputs of the mode-1 relocalisation tests (tests/test_reloc_p3p_ref.py on the CPU, tests/test_gpu_reloc_p3p.py on the
GPU): frames in the style of reloc_cases.frame_for_records whose every key is a correspondence, a share of them without a right
match, and the far scene of DESIGN.md section 6 (300 true pairs at 25 - 60 m, pixel noise on the right keys)."""
import numpy as np
import reloc_cases as rc
import reloc_p3p_ref as pp

RIG = rc.RIG
KP_DTYPE = rc.KP_DTYPE


def frame(C, outlier_frac, seed, rig=RIG, mode="pose", no_right=0.25):
    """C left keys at random pixels with a depth of 2 - 8 m, one map point per key carrying the key's descriptor (step A pairs
    point j with key j, step B' keeps all C); a share `no_right` of the keys has no right match (best = -1), the others a
    right key on the same row at the disparity.  mode as in reloc_cases.frame_for_records: "pose" (outlier_frac gross
    outliers), "collinear", "mirror" (the outliers lie behind the camera and project exactly onto their keys)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    T = rc.true_pose()
    R, t = T[:3, :3], T[:3, 3]
    u = rng.uniform(60, rig["w"] - 40, C).astype(np.float32); v = rng.uniform(40, rig["h"] - 40, C).astype(np.float32)
    z = rng.uniform(2.0, 8.0, C).astype(np.float32)
    kL = np.zeros(C, KP_DTYPE); kR = np.zeros(C, KP_DTYPE)
    kL["x"], kL["y"], kL["octave"], kL["size"] = u, v, rng.integers(0, 8, C), 31
    b = float(np.float32(rig["bl"]))
    kR["x"] = (u.astype(np.float64) - rig["fx"] * b / z.astype(np.float64)).astype(np.float32)
    kR["y"], kR["octave"], kR["size"] = v, kL["octave"], 31
    dL = rng.integers(0, 256, (C, 32), dtype=np.uint8); dR = rng.integers(0, 256, (C, 32), dtype=np.uint8)
    zp = z.astype(np.float64)
    Xc = np.stack([(u.astype(np.float64) - rig["cx"]) * zp / rig["fx"], (v.astype(np.float64) - rig["cy"]) * zp / rig["fy"], zp], axis=1)
    Xw = (Xc - t) @ R
    bad = rng.permutation(C)[:int(round(outlier_frac * C))]
    if mode == "pose":
        Xw[bad] = rng.uniform(-6, 6, (len(bad), 3))
    elif mode == "collinear":
        Xw = np.outer(rng.uniform(1, 9, C), np.array([0.3, -0.2, 0.9])) + np.array([0.5, 0.1, -0.4])
    elif mode == "mirror":
        Xw[bad] = (-Xc[bad] - t) @ R
        kR["x"][bad] = (rig["fx"] * (Xc[bad, 0] + b) / Xc[bad, 2] + rig["cx"]).astype(np.float32)
    best = np.arange(C, dtype=np.int32)
    best[rng.random(C) < no_right] = -1
    return dict(kL=kL, dL=dL, kR=kR, dR=dR, best=best, depth=z.copy(), sad=np.full(C, 10, np.int32), points=Xw, desc=dL.copy(),
                T_cw=T, n_keys=C, bad=bad)


def far_scene(seed=1, n=300, depth=(25.0, 60.0), sigma_r=0.25, sigma_l=0.0, rig=RIG, right=True):
    """n true pairs under reloc_cases.true_pose(): left keys at the true projection (+ N(0, sigma_l) px on x and y), right key
    x = true projection + N(0, sigma_r) px, the key's depth from that disparity, all octaves 0.  right = False: no key has a
    right match.  Returns the frame dict of `frame` plus `rec0` / `rec1`: the records of mode 0 (reloc_ref.pairs) and mode 1
    (reloc_p3p_ref.pairs) when every key keeps its stereo depth (no finalize cut)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    T = rc.true_pose()
    R, t = T[:3, :3], T[:3, 3]
    u = rng.uniform(60, rig["w"] - 40, n); v = rng.uniform(40, rig["h"] - 40, n); z = rng.uniform(depth[0], depth[1], n)
    Xc = np.stack([(u - rig["cx"]) * z / rig["fx"], (v - rig["cy"]) * z / rig["fy"], z], axis=1)
    Xw = (Xc - t) @ R
    b = float(np.float32(rig["bl"]))
    kL = np.zeros(n, KP_DTYPE); kR = np.zeros(n, KP_DTYPE)
    kL["x"] = (u + sigma_l * rng.normal(size=n)).astype(np.float32); kL["y"] = (v + sigma_l * rng.normal(size=n)).astype(np.float32)
    kL["size"] = 31; kR["size"] = 31
    kR["x"] = (u - rig["fx"] * b / z + sigma_r * rng.normal(size=n)).astype(np.float32); kR["y"] = kL["y"]
    disp = kL["x"].astype(np.float64) - kR["x"].astype(np.float64)
    ok = disp > 0                                       # (a key whose noisy disparity is not positive has no right match)
    zk = np.where(ok, rig["fx"] * b / np.where(ok, disp, 1.0), -1.0).astype(np.float32)
    dL = rng.integers(0, 256, (n, 32), dtype=np.uint8); dR = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    best = np.where(ok, np.arange(n), -1).astype(np.int32) if right else np.full(n, -1, np.int32)
    kw = np.arange(n, dtype=np.int32)
    rec0 = pp.rr.pairs(kw, Xw, kL, kR, zk if right else np.full(n, -1, np.float32), best, rig)
    rec1 = pp.pairs(kw, Xw, kL, kR, zk if right else np.full(n, -1, np.float32), best, rig)
    return dict(kL=kL, dL=dL, kR=kR, dR=dR, best=best, depth=zk, sad=np.full(n, 10, np.int32), points=Xw, desc=dL.copy(), T_cw=T,
                n_keys=n, rec0=rec0, rec1=rec1)


MARGIN = 1e-6
# The far scene's seeds start here.  Its triples are all inliers at 25 - 60 m, where two of a triple's solutions often nearly
# coincide (a small discriminant), so about one seed in twenty keeps MARGIN over 256 hypotheses; and on about half of the seeds
# mode 0 draws a triple lucky enough to pass min_inliers with a fraction of the 300 (seed 13, the first from seed 1 that keeps
# MARGIN: 238 of 297).  From 20 the first seed that keeps MARGIN is 21, where the restatement of mode 0 fails as it does on the
# fixed seed of tests/test_reloc_p3p_ref.py (best count 30 of 297 pairs).
FAR_SEED0 = 20
GPU_CASES = [dict(C=2), dict(C=3), dict(C=4), dict(C=64), dict(C=65), dict(C=200), dict(C=64, n_hypotheses=1), dict(C=64, n_hypotheses=1024),
             dict(C=64, mode="collinear"), dict(C=65, mode="mirror"), dict(far=True)]


def find_case(oracle, inv_sigma, C=0, mode="pose", far=False, **params):
    """The seed-advance rule of tests/test_gpu_reloc.py::hypothesis_case for mode 1: the first of at most 20 crafted seeds whose
    restatement keeps every tested residual a relative MARGIN away from the chi2 bound and every discriminant the solver
    branched on a relative MARGIN away from zero.  Returns (frame, stereo state, restatement result)."""
    for k in range(20):
        g = far_scene(seed=FAR_SEED0 + k) if far else frame(C, 0.4, 100 * C + k, mode=mode)
        st = oracle.stereo_finalize(g["best"], g["depth"], g["sad"], len(g["kR"]), RIG)
        ref = pp.relocalize(oracle, RIG, inv_sigma, g["points"], g["desc"], g["kL"], g["dL"], g["kR"], st, mode=1, **params)
        if ref["hyp"]["margin"] > MARGIN:
            break
    assert ref["hyp"]["margin"] > MARGIN, ref["hyp"]["margin"]
    return g, st, ref
