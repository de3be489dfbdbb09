"""Crafted inputs of the relocalisation tests (tests/test_reloc_ref.py on the CPU, tests/test_gpu_reloc.py on the GPU)."""
import numpy as np
import synth

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
RIG = synth.RIGS["euroc"]


def true_pose(seed=3):
    """a camera <- world pose far from the identity: 0.6 rad about a skew axis, metres of translation"""
    rng = np.random.Generator(np.random.PCG64(seed))
    w = rng.normal(size=3); w *= 0.6 / np.linalg.norm(w)
    th = np.linalg.norm(w); K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = rng.uniform(-2, 2, 3)
    return T


def flip_bits(desc, k, rng, avoid=()):
    """a copy of the 32-byte descriptor with k bits flipped, none of them in `avoid`; returns (descriptor, flipped bit list)"""
    free = np.setdiff1d(np.arange(256), np.asarray(avoid, np.int64))
    bits = rng.choice(free, size=k, replace=False)
    out = desc.copy()
    for b in bits:
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out, list(bits)


def records(C, outlier_frac, seed, rig=RIG, T_cw=None, exact=True):
    """C correspondence records (the dict of reloc_ref.pairs) from a known pose, the first round(outlier_frac * C) after a
    shuffle being gross outliers (their world point is unrelated).  exact: X_c = R X_w + t in fp64 (noise-free inliers)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    T = true_pose() if T_cw is None else T_cw
    R, t = T[:3, :3], T[:3, 3]
    u = rng.uniform(40, rig["w"] - 40, C); v = rng.uniform(40, rig["h"] - 40, C); z = rng.uniform(2.0, 8.0, C)
    Xc = np.stack([(u - rig["cx"]) * z / rig["fx"], (v - rig["cy"]) * z / rig["fy"], z], axis=1)
    Xw = (Xc - t) @ R                                   # R^T (Xc - t)
    if exact:
        Xc = np.stack([(R[r, 0] * Xw[:, 0] + R[r, 1] * Xw[:, 1] + R[r, 2] * Xw[:, 2]) + t[r] for r in range(3)], axis=1)
    bad = rng.permutation(C)[:int(round(outlier_frac * C))]
    Xw[bad] = rng.uniform(-6, 6, (len(bad), 3))
    b = float(np.float32(rig["bl"]))
    rec = dict(Xw=Xw, Xc=Xc, kx=(rig["fx"] * Xc[:, 0] / Xc[:, 2] + rig["cx"]).astype(np.float32),
               ky=(rig["fy"] * Xc[:, 1] / Xc[:, 2] + rig["cy"]).astype(np.float32),
               kxr=(rig["fx"] * (Xc[:, 0] - b) / Xc[:, 2] + rig["cx"]).astype(np.float32),
               octave=rng.integers(0, 8, C).astype(np.int32), p=np.arange(C, dtype=np.int32), i=np.arange(C, dtype=np.int32))
    good = np.ones(C, bool); good[bad] = False
    return rec, T, good


def frame_for_records(C, outlier_frac, seed, rig=RIG, mode="pose"):
    """A crafted frame + map whose step B yields exactly C correspondences: left keys at random pixels with a depth, right
    keys on the same row at the disparity, one map point per key carrying the key's own descriptor (so step A pairs point j
    with key j at distance 0).  The stereo finalize kernel cuts the nearest 1 % of the accepted pairs: `extra` sacrificial
    keys at 0.5 m take that cut (their winners are the pairs step B drops).
    mode: "pose" a known pose with outlier_frac gross outliers; "collinear" every world point on one line; "mirror" the
    outliers are points behind the camera that project exactly onto their keys.
    Returns dict(kL, dL, kR, dR, best, depth, sad, points, desc, T_cw, n_keys)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    extra = 0
    while extra != (C + extra) // 100:
        extra += 1
    n = C + extra
    T = true_pose()
    R, t = T[:3, :3], T[:3, 3]
    u = rng.uniform(60, rig["w"] - 40, n).astype(np.float32); v = rng.uniform(40, rig["h"] - 40, n).astype(np.float32)
    z = rng.uniform(2.0, 8.0, n).astype(np.float32)
    z[C:] = 0.5
    order = rng.permutation(n)                      # the sacrificial keys anywhere in the key order
    u, v, z = u[order], v[order], z[order]
    kL = np.zeros(n, KP_DTYPE); kR = np.zeros(n, KP_DTYPE)
    kL["x"], kL["y"], kL["octave"], kL["size"] = u, v, rng.integers(0, 8, n), 31
    kR["x"] = (u.astype(np.float64) - rig["fx"] * float(np.float32(rig["bl"])) / z.astype(np.float64)).astype(np.float32)
    kR["y"], kR["octave"], kR["size"] = v, kL["octave"], 31
    dL = rng.integers(0, 256, (n, 32), dtype=np.uint8); dR = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    zp = z.astype(np.float64)
    Xc = np.stack([(u.astype(np.float64) - rig["cx"]) * zp / rig["fx"], (v.astype(np.float64) - rig["cy"]) * zp / rig["fy"], zp], axis=1)
    Xw = (Xc - t) @ R
    if mode == "pose":
        live = np.nonzero(z > 1.0)[0]
        bad = rng.permutation(live)[:int(round(outlier_frac * C))]
        Xw[bad] = rng.uniform(-6, 6, (len(bad), 3))
    elif mode == "collinear":
        Xw = np.outer(rng.uniform(1, 9, n), np.array([0.3, -0.2, 0.9])) + np.array([0.5, 0.1, -0.4])
    elif mode == "mirror":
        # the "outliers" are the inliers' points mirrored through the camera centre (R X_w + t = -X_c), and their right keys sit
        # where the mirrored point's right projection falls: every residual of such a pair is zero under the true pose and only
        # the z > 0 test keeps it out of the count
        live = np.nonzero(z > 1.0)[0]
        bad = rng.permutation(live)[:int(round(outlier_frac * C))]
        Xw[bad] = (-Xc[bad] - t) @ R
        b = float(np.float32(rig["bl"]))
        kR["x"][bad] = (rig["fx"] * (Xc[bad, 0] + b) / Xc[bad, 2] + rig["cx"]).astype(np.float32)
    return dict(kL=kL, dL=dL, kR=kR, dR=dR, best=np.arange(n, dtype=np.int32), depth=z.copy(), sad=np.full(n, 10, np.int32),
                points=Xw, desc=dL.copy(), T_cw=T, n_keys=n)
