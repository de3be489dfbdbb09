"""Crafted inputs of the pose-solve tests (tests/test_pose_cases.py on the CPU, tests/test_gpu_pose_crafted.py on the GPU).

numpy and the project's synth module (its rigs and synthetic trajectory) only, no GPU.  A case is a dict: the frame
(kL, kR, best, depth, sad: what stereo_finalize_arrays and set_keys take), the
problem (points, matches, inF, inFR, mpo, out0) and the initial camera <- world pose T0.  Every frame carries the
sacrificial pairs at 0.5 m that the finalize kernel's nearest-1 % cut takes, so every other accepted pair survives it.

The shapes of section 2 follow the kernel's layout (pose_dev.hpp): map point i is handled by thread i % POSE_NT in slot
u = (i % 1024) / 256 of trip i / 1024, that is wave (i % 256) / 64, lane i % 64.
"""
import math
import numpy as np
import synth

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
RIG = synth.RIGS["euroc"]
FX, FY, CX, CY, W, H = RIG["fx"], RIG["fy"], RIG["cx"], RIG["cy"], RIG["w"], RIG["h"]
BL = float(np.float32(RIG["bl"]))                                   # the baseline as both implementations hold it
CLOSE_TH = float(np.float32(RIG["bl"]) * np.float32(40))            # float32(baseline) * closeNumber, as a double
POSE_NT, POSE_BATCH = 256, 4                                        # asserted against pose_dev.hpp by test_pose_cases.py
TRIP = POSE_NT * POSE_BATCH
IMU_LDS_FACTORS = 2125                                              # POSE_IMU_LDS_FACTORS (pose_imu.hip)
CHI2 = 7.815


def inv_sigma_table(n=8, scale=1.2):
    """InvSigmaFactor of the extractor: 1 / scale_l^2 with the scale an iterated float32 product"""
    s = np.float32(1.0)
    out = np.zeros(n, np.float32)
    for l in range(n):
        out[l] = np.float32(1.0) / (s * s)
        s = np.float32(s * np.float32(scale))
    return out


INV_SIGMA = inv_sigma_table()


# The cases are bit-reproducible inputs: products are written as plain multiply-add sums in a fixed order (no BLAS
# kernel, whose use of FMA depends on the CPU) and angles go through math.sin / math.cos.
def mm(A, B):
    """A @ B (2-D) or A @ v (1-D v) as sums of products in index order"""
    A = np.asarray(A, np.float64); B = np.asarray(B, np.float64)
    if B.ndim == 1:
        return np.array([sum(float(A[i, k]) * float(B[k]) for k in range(A.shape[1])) for i in range(A.shape[0])])
    return np.array([[sum(float(A[i, k]) * float(B[k, j]) for k in range(A.shape[1])) for j in range(B.shape[1])] for i in range(A.shape[0])])


def rot(axis, angle):
    a = [float(v) for v in axis]
    n = math.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
    a = [v / n for v in a]
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * mm(K, K)


def pose(R=None, t=(0, 0, 0)):
    T = np.eye(4)
    if R is not None:
        T[:3, :3] = R
    T[:3, 3] = t
    return T


def rigid_inv(T):
    Ti = np.eye(4)
    Ti[:3, :3] = T[:3, :3].T
    Ti[:3, 3] = -mm(T[:3, :3].T, T[:3, 3])
    return Ti


def sacrificial(n_acc):
    """how many extra pairs the nearest-1 % cut of the finalize kernel must find: extra == floor((n_acc + extra) / 100)"""
    extra = 0
    while extra != (n_acc + extra) // 100:
        extra += 1
    return extra


class Builder:
    """a frame and a problem, one map point at a time.  Pixels are float32 key coordinates; a point is given in the LEFT
    camera's frame and stored in the world of T_cw."""

    def __init__(self, T_cw, M, mpo=0):
        self.T = np.array(T_cw, np.float64)
        self.M = M
        self.kl, self.kr, self.best, self.depth = [], [], [], []
        self.points = np.zeros((M, 3))
        self.matches = np.full((M, 2), -1, np.int32)
        self.inF = np.ones(M, np.uint8); self.inFR = np.ones(M, np.uint8)
        self.mpo = np.full(M, mpo, np.uint8); self.out0 = np.zeros(M, np.uint8)
        self.used = np.zeros(M, bool)

    def lkey(self, x, y, octave, best=-1, depth=-1.0):
        self.kl.append((np.float32(x), np.float32(y), int(octave)))
        self.best.append(int(best)); self.depth.append(np.float32(depth))
        return len(self.kl) - 1

    def rkey(self, x, y, octave):
        self.kr.append((np.float32(x), np.float32(y), int(octave)))
        return len(self.kr) - 1

    def set_best(self, k, r, depth):
        self.best[k] = int(r); self.depth[k] = np.float32(depth)

    def world(self, pc):
        R, t = self.T[:3, :3], self.T[:3, 3]
        return mm(R.T, np.asarray(pc, np.float64) - t)

    def put(self, i, pc, first, second, inF=1, inFR=1, out0=0, world=None):
        assert not self.used[i]
        self.used[i] = True
        self.points[i] = self.world(pc) if world is None else world
        self.matches[i] = (first, second)
        self.inF[i], self.inFR[i], self.out0[i] = inF, inFR, out0

    def free_slots(self):
        return np.nonzero(~self.used)[0]

    def finish(self, T0, name, **more):
        assert self.used.all()
        nL, nR = len(self.kl), len(self.kr)
        extra = sacrificial(sum(b >= 0 for b in self.best))
        for e in range(extra):
            r = self.rkey(300.0 + e, 20.0, 0)
            self.lkey(400.0 + e, 20.0, 0, best=r, depth=0.5)
        kL = np.zeros(len(self.kl), KP_DTYPE); kR = np.zeros(len(self.kr), KP_DTYPE)
        for arr, src in ((kL, self.kl), (kR, self.kr)):
            if len(src):
                arr["x"] = [s[0] for s in src]; arr["y"] = [s[1] for s in src]; arr["octave"] = [s[2] for s in src]
            arr["size"] = 31
        c = dict(name=name, kL=kL, kR=kR, best=np.array(self.best, np.int32), depth=np.array(self.depth, np.float32),
                 sad=np.full(len(self.kl), 10, np.int32), points=self.points, matches=self.matches, inF=self.inF, inFR=self.inFR,
                 mpo=self.mpo, out0=self.out0, T0=np.array(T0, np.float64), n_keys=(nL, nR))
        c.update(more)
        return c


def cam_point(x, y, z, du=0.0, dv=0.0, right=False):
    """the point at depth z that projects at pixel (x + du, y + dv) of the left (or right) camera, in the LEFT camera's frame"""
    X = (float(x) + du - CX) * z / FX + (BL if right else 0.0)
    return np.array([X, (float(y) + dv - CY) * z / FY, z])


def disparity(z):
    return FX * BL / z


def descriptors(case):
    return np.zeros((len(case["kL"]), 32), np.uint8), np.zeros((len(case["kR"]), 32), np.uint8)


def frame_state(oracle, case):
    """the stereo state after the finalize cuts, as the oracle computes it"""
    return oracle.stereo_finalize(case["best"], case["depth"], case["sad"], len(case["kR"]), RIG)


def run_oracle(oracle, case, st=None, perm=None, mpo=None):
    """oracle.estimate_pose on the case; perm: the map points in that order (the results come back in the case's order)"""
    st = frame_state(oracle, case) if st is None else st
    a = [case["points"], case["inF"], case["inFR"], case["mpo"] if mpo is None else mpo, case["matches"], case["out0"]]
    if perm is not None:
        a = [x[perm] for x in a]
    ref = oracle.estimate_pose(RIG, INV_SIGMA, a[0], a[1], a[2], a[3], a[4], a[5], case["kL"], case["kR"],
                               st["rightIdxs"], st["leftIdxs"], st["depth"], st["close"], case["T0"])
    if perm is not None:
        for k in ("outliers", "matches"):
            back = np.empty_like(ref[k]); back[perm] = ref[k]; ref[k] = back
    return ref


# ---- sections 1 and 2: synthetic stereo scenes ---------------------------------------------------------------------------------
# point kinds of a mixed scene
STEREO, MONO_FAR, MONO_LOST, MONO_NOSTEREO, RIGHT_ONLY = range(5)


def scene(M, seed, T_cw, mixed, noise=0.3, plant=False, stereo_at=()):
    """M map points seen from T_cw, one left and one right key each (no shared keys): keys uniform in the image, octaves
    0 .. 7, depths 1.5 .. 8 m kept 0.2 m off the close bound, `noise` px of Gaussian noise on every observation.
    mixed = False: every point has both observations, matches (i, i).
    mixed = True: the five kinds above in a random pattern - stereo factors, the three ways to a left mono factor (a far
    key, a close key whose match lost its right index, a key without a stereo pair) and right-only factors.
    plant: every observation is moved by 0.5 .. 0.9 / InvSigmaFactor[octave] px in a random direction, so that every factor
    has a whitened residual of at least about 0.5 at the true pose.
    stereo_at: points of a mixed scene that are stereo factors whatever the pattern says (at 2 m or 3.5 m)."""
    rng =np.random.Generator(np.random.PCG64(seed))
    u = rng.uniform(60, W - 40, M); v = rng.uniform(40, H - 40, M); octv = rng.integers(0, 8, M)
    z = rng.uniform(1.5, 8.0, M)
    z[(z > 4.2) & (z < 4.6)] += 0.5
    kind = np.where(z < 4.4, STEREO, MONO_FAR)
    if mixed:
        kind = rng.integers(0, 5, M)
        near = (kind == STEREO) | (kind == MONO_LOST)
        z[near] = rng.uniform(1.5, 4.2, int(near.sum()))
        far = kind == MONO_FAR
        z[far] = rng.uniform(4.7, 8.0, int(far.sum()))
        for j, i in enumerate(stereo_at):
            kind[i] = STEREO; z[i] = 2.0 + 1.5 * (j % 2)
    b = Builder(T_cw, M)
    n = rng.normal(0, noise, (M, 4))
    if plant:
        d = rng.normal(0, 1, (M, 2)); d /= np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])[:, None]
        mag = rng.uniform(0.5, 0.9, M) / INV_SIGMA[octv].astype(np.float64)
        n[:, 0] += mag * d[:, 0]; n[:, 2] += mag * d[:, 0]; n[:, 1] += mag * d[:, 1]; n[:, 3] += mag * d[:, 1]
    for i in range(M):
        has = kind[i] in (STEREO, MONO_FAR, MONO_LOST)
        k = b.lkey(u[i] + n[i, 0], v[i] + n[i, 1], octv[i], best=i if has else -1, depth=z[i] if has else -1.0)
        r = b.rkey(u[i] - disparity(z[i]) + n[i, 2], v[i] + n[i, 3], octv[i])
        assert k == i and r == i
        m = {STEREO: (i, i), MONO_FAR: (i, i), MONO_LOST: (i, -1), MONO_NOSTEREO: (i, -1), RIGHT_ONLY: (-1, i)}[int(kind[i])]
        b.put(i, cam_point(u[i], v[i], z[i]), m[0], m[1])
    return b, kind


# -- section 1: the LM policy.  T_true = identity, start = [R(axis (0.3, 1, 0.2), angle) | t] ------------------------------------
LM_AXIS = (0.3, 1.0, 0.2)
# name: (M, seed, angle, t, the branch the oracle reaches, the spread of T_cw over 8 permutations of the map points as
# measured on the CPU, to four digits; test_pose_cases.py::test_lm_case measures it again and compares)
LM_CASES = {
    "m6-rejected-a":        (6, 1, 1.5, (2.5, -1.25, 0.838), "rejected", 1.324e-15),            # 13 / 28
    "m6-rejected-b":        (6, 6, 1.9, (3.167, -1.583, 1.061), "rejected", 1.915e-14),         # 17 / 37, lambda ends at 1e-2
    "m40-rejected":         (40, 7, 1.0, (1.667, -0.833, 0.558), "rejected", 1.584e-15),        # 10 / 19
    "m300-rejected":        (300, 5, 0.9, (1.5, -0.75, 0.503), "rejected", 2.564e-15),          # 11 / 26, lambda ends at 1e-1
    "m6-wrong-minimum":     (6, 7, 1.2, (2.0, -1.0, 0.67), "wrong-minimum", 4.331e-12),         # 12 / 23, one inlier left
    "m6-bound-no-step":     (6, 1, 2.0, (3.333, -1.667, 1.117), "lambda-bound", 0.0),     # 0 / 10: ten rejections in a row
    "m40-bound":            (40, 1, 2.0, (3.333, -1.667, 1.117), "lambda-bound", 1.551e-13),    # 2 / 14
    "m300-bound-a":         (300, 1, 1.2, (2.0, -1.0, 0.67), "lambda-bound", 1.430e-13),        # 2 / 14
    "m300-bound-b":         (300, 1, 2.0, (3.333, -1.667, 1.117), "lambda-bound", 2.534e-11),   # 2 / 14
    "m6-behind":            (6, 1, 3.0, (1.0, -0.5, 0.33), "stop", 0.0),                  # 0 / 0: zero Jacobian
    "m40-behind":           (40, 1, 3.0, (1.0, -0.5, 0.33), "stop", 0.0),
    "m300-behind":          (300, 1, 3.0, (1.0, -0.5, 0.33), "stop", 0.0),
    "m6-accepted-9":        (6, 2, 1.2, (2.0, -1.0, 0.67), "accepted", 2.606e-15),
    "m40-accepted-13":      (40, 1, 1.2, (2.0, -1.0, 0.67), "accepted", 2.570e-15),             # lambda down to 1e-18
    "m300-accepted-9":      (300, 1, 0.8, (1.333, -0.667, 0.447), "accepted", 1.900e-15),
    "m300-accepted-4":      (300, 1, 0.05, (0.083, -0.042, 0.028), "accepted", 2.090e-16),
    # non-finite normal equations (see lm_degenerate_case): the start is the identity
    "m7-cholesky-fails":    (6, 1, 0.0, (0.0, 0.0, 0.0), "cholesky-fails", 0.0),          # 0 / 10: every solve fails
}
# the extra map point of the degenerate case, in the frame of the start pose (the identity: world = camera frame,
# q = R^T (p - t) is exact).  z = 1e-160 > 0 passes the cheirality test and 1 / z^2 overflows; with x = 1e-20 the residual
# fx x / z is finite (its square too), its derivative fx x / z^2 is not, times -y = -0 that is NaN: H[0][0] is NaN and the
# first pivot is refused at every lambda.
DEGENERATE_POINTS = {"cholesky-fails": (1e-20, 0.0, 1e-160)}


def lm_case(name):
    M, seed, angle, t, branch, spread = LM_CASES[name]
    if branch in DEGENERATE_POINTS:
        return lm_degenerate_case(name)
    b, _ = scene(M, seed, np.eye(4), mixed=False)
    return b.finish(pose(rot(LM_AXIS, angle), t), name, branch=branch, spread=spread)


def lm_degenerate_case(name):
    """a 6-point scene seen from 0.2 rad and a few cm off the identity, the solve started AT the identity, plus one left mono
    point almost in the camera centre of the start pose: its Jacobian overflows while its residual stays finite"""
    M, seed, _, _, branch, spread = LM_CASES[name]
    T_true = pose(rot(LM_AXIS, 0.2), (0.05, -0.02, 0.03))
    src, _ = scene(M, seed, T_true, mixed=False)
    b = Builder(np.eye(4), M + 1)
    b.kl, b.kr, b.best, b.depth = src.kl, src.kr, src.best, src.depth
    for i in range(M):
        b.put(i, None, src.matches[i, 0], src.matches[i, 1], world=src.points[i])
    k = b.lkey(CX + 10.0, CY - 5.0, 0)
    b.put(M, None, k, -1, world=np.array(DEGENERATE_POINTS[branch]))
    return b.finish(np.eye(4), name, branch=branch, spread=spread)


# -- section 2: factor compaction ------------------------------------------------------------------------------------------------
COMPACT_SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 3073)
MASKS = ("all", "lane0", "lane63", "wave3", "alternate", "seventh", "midtrip", "ends")


# Two masks leave exactly two factors: (65, lane0) and (3073, ends).  Two points cannot fix a pose: what the data
# determines is where the two points lie in the camera frame - and that only if both are STEREO factors (two mono factors
# fix four numbers, not five), so these cases make them stereo.  The sixth degree of freedom, the rotation about the line
# through the two points, is set by the damping alone and moves with the order of summation (by 1e-9 .. 1e-7 rad over the
# scenes tried).  For these cases the tests hold the two points in the camera frame to the bar of the full pose elsewhere,
# and say so; see two_factor_gauge_bound for the gauge angle.
def two_factor(case):
    return len(factor_points(case)) == 2


def factor_points_cam(case, T_cw):
    """the map points that carry a factor, in the camera frame of T_cw"""
    P = case["points"][factor_points(case)]
    return np.stack([mm(T_cw[:3, :3], p) + T_cw[:3, 3] for p in P])


def gauge_angle(Ta, Tb):
    """angle of the rotation Ra Rb^T (small angles: from its skew part)"""
    D = mm(Ta[:3, :3], Tb[:3, :3].T)
    return 0.5 * math.sqrt((D[2, 1] - D[1, 2]) ** 2 + (D[0, 2] - D[2, 0]) ** 2 + (D[1, 0] - D[0, 1]) ** 2)


def two_factor_gauge_bound(initial_error, iterations):
    """a rounding-error bound on the gauge angle of a two-factor solve, not a parity bar.  Along the gauge direction e the
    exact gradient g.e and curvature e'He are zero, so accepted step k moves the gauge by fl(g.e) / lambda_k, lambda_k =
    1e-5 / 10^k.  fl(g.e) is the rounding error of a sum of 6 products J r: at most 6 * 2^-53 * max|J| * sum|r|, with
    max|J| <= fx (1 + tan^2) < 780 for a rotation column inside the image (InvSigmaFactor <= 1) and sum|r| <= sqrt(6 * 2 E0)
    at every step of a run that only accepts steps."""
    return 6 * 2.0 ** -53 * 780.0 * math.sqrt(12.0 * initial_error) * sum(10.0 ** k / 1e-5 for k in range(iterations))


def mask_keep(M, mask):
    """which map points keep their factor, or None when the mask does not apply at this size"""
    i = np.arange(M)
    lane, wave, trip = i % 64, (i % POSE_NT) // 64, i // TRIP
    if mask == "all": return np.ones(M, bool)
    if mask == "lane0": return lane == 0
    if mask == "lane63": return lane == 63
    if mask == "wave3": return wave == 3
    if mask == "alternate": return i % 2 == 0
    if mask == "seventh": return i % 7 == 3
    if mask == "midtrip": return trip != 1 if M >= 2049 else None         # a whole trip without a factor between two with
    if mask == "ends": return (i == 0) | (i == M - 1) if M == 3073 else None
    raise KeyError(mask)


def compact_ids():
    return [(M, mask) for M in COMPACT_SIZES for mask in MASKS if mask_keep(M, mask) is not None]


def scene_pose():
    """the camera <- world pose of the scenes of section 5: frame 6 of the synthetic trajectory (the IMU solve's prediction
    comes from the trajectory's IMU samples)"""
    return rigid_inv(synth.pose_at(6, RIG["fps"]))


COMPACT_POSE = pose(rot((0.2, -0.5, 1.0), 0.3), (0.4, -0.2, 0.7))    # camera <- world of the section 2 scenes


def near_start(T_cw):
    """0.05 rad and 0.1 m off T_cw"""
    return mm(pose(rot(LM_AXIS, 0.05), (0.06, -0.05, 0.0625)), T_cw)


def compact_case(M, mask, T_cw=None):
    """a mixed, planted scene with the factor of every point outside the mask removed, the five ways of removing one taken
    in turn: mp_is_outlier, mps_outliers, in_frame = 0 (on a left match), in_frame_r = 0 (on a right-only match), no match"""
    T_cw = COMPACT_POSE if T_cw is None else T_cw
    keep = mask_keep(M, mask)
    b, kind = scene(M, 7000 + M, T_cw, mixed=True, plant=True, stereo_at=np.nonzero(keep)[0] if keep.sum() == 2 else ())
    for way, i in enumerate(np.nonzero(~keep)[0]):
        way %= 5
        if way == 0: b.mpo[i] = 1
        elif way == 1: b.out0[i] = 1
        elif way == 2:
            if b.matches[i, 0] < 0: b.matches[i] = (i, -1)
            b.inF[i] = 0
        elif way == 3:
            b.matches[i] = (-1, i); b.inFR[i] = 0
        else: b.matches[i] = (-1, -1)
    c = b.finish(near_start(T_cw), "compact-%d-%s" % (M, mask), keep=keep, kind=kind)
    return c


def factor_points(case):
    """indices of the map points that carry a factor, in order (the rule of buildPoseFactors restated on the case's arrays)"""
    m = case["matches"]
    live = (case["mpo"] == 0) & (case["out0"] == 0)
    left = (m[:, 0] >= 0) & (case["inF"] != 0)
    right = (m[:, 0] < 0) & (m[:, 1] >= 0) & (case["inFR"] != 0)
    return np.nonzero(live & (left | right))[0]


def boundary_sample(case):
    """the first and the last factor of every wave (64 consecutive map points) and so of every trip"""
    f = factor_points(case)
    out = set()
    for w in np.unique(f // 64):
        g = f[f // 64 == w]
        out.add(int(g[0])); out.add(int(g[-1]))
    return sorted(out)


# ---- section 3: the chi2 pass in isolation -------------------------------------------------------------------------------------
T_CHI2 = pose(None, (1.0, -2.0, 3.0))           # identity rotation, integer translation: the pass runs at a pose known to the bit

# (kind, octave): (pixel of the key, depth of the point).  kind: "left" the left check of a mono point, "stereo_right" the
# right check of a close stereo point, "right_only" the check of a right-only point
BOUND_SPOTS = {("left", 0): (200.0, 100.0, 3.0), ("left", 7): (500.25, 300.5, 5.5),
               ("stereo_right", 0): (250.5, 150.0, 2.5), ("stereo_right", 7): (450.0, 350.25, 3.5),
               ("right_only", 0): (300.0, 200.5, 6.0), ("right_only", 7): (600.75, 120.0, 2.0)}
# the pixel offsets on either side of the chi2 bound: (largest inlier, smallest outlier), adjacent doubles, found by bisection
# on the oracle (bound_bisect below); test_pose_cases.py::test_bound_offsets repeats the bisection and compares
_h = float.fromhex
BOUND_OFFSETS = {("left", 0): (_h("0x1.65d3ff5aefca0p+1"), _h("0x1.65d3ff5aefca1p+1")),                # radius 2.7955 px
                 ("left", 7): (_h("0x1.408a70c4b546fp+3"), _h("0x1.408a70c4b5470p+3")),                # radius 10.017 px
                 ("right_only", 0): (_h("0x1.65d3ff5aefc40p+1"), _h("0x1.65d3ff5aefc41p+1")),
                 ("right_only", 7): (_h("0x1.408a70c4b545fp+3"), _h("0x1.408a70c4b5460p+3")),
                 ("stereo_right", 0): (_h("0x1.65d4215c7f1bfp+0"), _h("0x1.65d4215c7f1c0p+0")),        # radius / 2
                 ("stereo_right", 7): (_h("0x1.408a83272b9dfp+2"), _h("0x1.408a83272b9e0p+2"))}


def bound_radius(octave):
    return float(np.sqrt(CHI2 / float(INV_SIGMA[octave])))


def _put_bound(b, i, kind, octave, d):
    x, y, z = BOUND_SPOTS[(kind, octave)]
    if kind == "left":
        k = b.lkey(x, y, octave)
        b.put(i, cam_point(np.float32(x), np.float32(y), z, du=d), k, -1)
    elif kind == "right_only":
        r = b.rkey(x, y, octave)
        b.lkey(x, y, octave)
        b.put(i, cam_point(np.float32(x), np.float32(y), z, du=d, right=True), -1, r)
    else:
        # left residual d, right residual d + radius / 2: the right check crosses the bound at d = radius / 2
        r = b.rkey(x - disparity(z) - 0.5 * bound_radius(octave), y, octave)
        k = b.lkey(x, y, octave, best=r, depth=z)
        b.put(i, cam_point(np.float32(x), np.float32(y), z, du=d), k, r)
    return len(b.kl) - 1


def bound_probe(kind, octave, d):
    """one map point `d` px off its key (all flagged mp_is_outlier: no factor, the pass alone)"""
    b = Builder(T_CHI2, 1, mpo=1)
    k = _put_bound(b, 0, kind, octave, d)
    return b.finish(T_CHI2, "bound-%s-%d" % (kind, octave), key=k)


def bound_failed(kind, ref, key):
    return bool(ref["close"][key] == 0) if kind == "stereo_right" else bool(ref["outliers"][0] == 1)


def bound_bisect(oracle, kind, octave):
    """(largest offset the oracle accepts, smallest it refuses) between an accepted and a refused start, to adjacent doubles"""
    r = bound_radius(octave)
    lo, hi = (0.25 * r, 0.75 * r) if kind == "stereo_right" else (0.5 * r, 1.5 * r)

    def failed(d):
        c = bound_probe(kind, octave, d)
        return bound_failed(kind, run_oracle(oracle, c), c["key"])
    assert not failed(lo) and failed(hi)
    while True:
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            return lo, hi
        if failed(mid): hi = mid
        else: lo = mid


def _filler(b, rng, slots):
    """benign points for the unused slots, each on keys of its own: exact stereo inliers, far mono points, right-only points"""
    for n, i in enumerate(slots):
        x = rng.uniform(60, W - 40); y = rng.uniform(40, H - 40); o = int(rng.integers(0, 8))
        t = n % 3
        z = rng.uniform(1.5, 4.0) if t == 0 else rng.uniform(4.8, 8.0)
        r = b.rkey(x - disparity(z), y, o)
        k = b.lkey(x, y, o, best=r if t < 2 else -1, depth=z if t < 2 else -1.0)
        pc = cam_point(np.float32(x), np.float32(y), z)
        if t == 2:
            pc = cam_point(b.kr[r][0], b.kr[r][1], z, right=True)
        b.put(i, pc, k if t < 2 else -1, r, out0=n % 2)
    return len(range(0, len(slots), 3))                             # how many of them are stereo inliers


def chi2_bounds_case():
    """the chi2 bound from both sides at octaves 0 and 7 for the three checks, the depth bound, cheirality, the exclusions"""
    M = 40
    b = Builder(T_CHI2, M, mpo=1)
    i = 0
    expect = {}
    for (kind, octave), (d_in, d_out) in sorted(BOUND_OFFSETS.items()):
        for d, fails in ((d_in, False), (d_out, True)):
            k = _put_bound(b, i, kind, octave, d)
            expect[i] = (kind, k, fails)
            i += 1
    # the depth bound: a close stereo key whose right observation fails, the point at z = the bound and one ulp either side
    depth_pts = {}
    for z in (np.nextafter(CLOSE_TH, 0.0), CLOSE_TH, np.nextafter(CLOSE_TH, 10.0)):
        r = b.rkey(320.0 - disparity(z) + 20.0, 240.0 + 8 * i, 1)
        k = b.lkey(320.0, 240.0 + 8 * i, 1, best=r, depth=3.0)
        b.put(i, cam_point(np.float32(320.0), np.float32(240.0 + 8 * i), float(z)), k, r)
        depth_pts[i] = (k, float(z))
        i += 1
    # cheirality: z = 0 and z = -1 (in_frame set: the pass looks at them)
    behind = []
    for z in (0.0, -1.0):
        k = b.lkey(100.0 + i, 400.0, 2)
        b.put(i, np.array([0.1, 0.05, z]), k, -1, out0=0)
        behind.append(i); i += 1
    # exclusions: the outlier byte keeps its input value
    excluded = []
    for out0 in (0, 1):
        k = b.lkey(150.0 + i, 420.0, 0)
        b.put(i, cam_point(np.float32(150.0 + i), np.float32(420.0), 3.0, du=30.0), k, -1, inF=0, out0=out0); excluded.append(i); i += 1
        r = b.rkey(150.0 + i, 430.0, 0)
        b.put(i, cam_point(np.float32(150.0 + i), np.float32(430.0), 3.0, du=30.0, right=True), -1, r, inFR=0, out0=out0); excluded.append(i); i += 1
        b.put(i, np.array([0.0, 0.0, 2.0 - 3.0 * out0]), -1, -1, out0=out0); excluded.append(i); i += 1
    _filler(b, np.random.Generator(np.random.PCG64(31)), b.free_slots())
    return b.finish(T_CHI2, "chi2-bounds", expect=expect, depth_pts=depth_pts, behind=behind, excluded=excluded)


# chains of map points on one left key: (map point indices, which of them fail the right check).  The members sit in
# different threads (i, i + 1), waves (i, i + 64), slots of a thread (i, i + 256) and trips (i, i + 1024; 1023 / 1024).
CHAINS = (
    dict(at=(5, 261), fail=(0,)),                                   # 2: the first fails; the second is no longer stereo
    dict(at=(10, 266, 1034), fail=(1,)),                            # 3: inlier, fail, inlier - across a trip
    dict(at=(70, 71, 134), fail=(2,)),                              # 3: the last fails
    dict(at=(1023, 1024), fail=(1,)),                               # 2: across the trip boundary, the last fails
    dict(at=(1026, 767), fail=(0,)),                                # 2: the failing one has the higher index: 767 counts first
    dict(at=(20, 84, 276, 300, 532, 788, 1044, 1090), fail=(7,)),   # 8: the last fails
    dict(at=(30, 94, 286, 310, 542, 798, 1054, 1095), fail=(0,)),   # 8: the first fails
    dict(at=(40, 104, 296, 320, 552, 808, 1064, 1099), fail=(4,)),  # 8: a middle one fails
    dict(at=(50, 306, 1074, 1080), fail=(1, 2)),                    # two fail: only the lower index applies
    dict(at=(60, 316), fail=(1,), mismatch=True),                   # the failing match names another right key than rightIdxs[k]
)
CHAIN_M = 1100


def chain_case(T_cw, fail=True, mpo=1, T0=None, name="chains"):
    """CHAINS on keys of octave 0 .. 2, every member exactly on the shared left key (depths 2.0, 2.1, ..), its right key
    exactly at its own disparity, or 20 px off where it fails.  fail = False: the same keys and indices, nothing fails.
    rightIdxs[k] is the FIRST member's right key, except in the mismatch chain, where it is a key of its own that is also
    the stereo partner of nobody else; there a second left key holds the failing match's right key, and must keep it."""
    b = Builder(T_cw, CHAIN_M, mpo=mpo)
    info = []
    for c, ch in enumerate(CHAINS):
        x, y, o = 100.0 + 55 * c, 80.0 + 30 * c, c % 3
        k = b.lkey(x, y, o, best=-1, depth=2.5)
        order = sorted(ch["at"])
        rks = {}
        for j, i in enumerate(ch["at"]):
            z = 2.0 + 0.1 * j
            fails = fail and j in ch["fail"]
            r = b.rkey(x - disparity(z) + (20.0 if fails else 0.0), y, o)
            rks[i] = r
            b.put(i, cam_point(np.float32(x), np.float32(y), z), k, r)
        own = rks[ch["at"][0]]
        other = None
        if ch.get("mismatch"):
            own = b.rkey(x - disparity(2.5), y + 3.0, o)                 # rightIdxs[k]: not the failing match's right key
            failing = ch["at"][ch["fail"][0]]
            other = b.lkey(x + 9.0, y + 3.0, o, best=rks[failing], depth=3.0)    # another left key owns that right key
        b.set_best(k, own, 2.5)
        first_fail = min(ch["at"][j] for j in ch["fail"]) if fail else None
        info.append(dict(key=k, order=order, first_fail=first_fail, own=own, other=other, rks=rks))
    n_stereo = _filler(b, np.random.Generator(np.random.PCG64(32)), b.free_slots())
    return b.finish(T_cw if T0 is None else T0, name, chains=info, n_filler_stereo=n_stereo)


# ---- section 6: worldToFrame at its edges --------------------------------------------------------------------------------------
LOG_SCALE = np.float32(np.log(np.float32(1.2)))


def _flip(oracle, right, make, lo, hi):
    """adjacent doubles (a, b) between lo and hi with different visibility of make(.) under the oracle"""
    def vis(s):
        return int(oracle.world_to_frame(RIG, np.eye(4), right, make(s)[None, :], np.ones(1, np.float32), LOG_SCALE)[3][0])
    vlo = vis(lo)
    assert vlo != vis(hi)
    while True:
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            return lo, hi
        if vis(mid) == vlo: lo = mid
        else: hi = mid


def w2f_case(oracle):
    """points (in the frame of T_cw = identity) and their maxScaleDist:
    - u at 0 and at w, v at 0 and at h, for each camera: the two adjacent doubles on either side of the oracle's decision,
      at two depths (z = 2: 1 / z exact; z = 3.7)
    - z = 0, tiny positive, negative
    - the level prediction: maxScaleDist = dist * 1.2^k in float32, k = -2 .. 9, and its two float32 neighbours: ratios on,
      just under and just over a power of the scale factor, and both clamps"""
    pts, msd = [], []
    edges = []
    for right in (False, True):
        off = BL if right else 0.0
        for z in (2.0, 3.7):
            x0, x1 = (0 - CX) * z / FX + off, (W - CX) * z / FX + off
            y0, y1 = (0 - CY) * z / FY, (H - CY) * z / FY
            for make, c in ((lambda s, z=z: np.array([s, 0.01, z]), x0), (lambda s, z=z: np.array([s, 0.01, z]), x1),
                            (lambda s, z=z, off=off: np.array([off + 0.01, s, z]), y0), (lambda s, z=z, off=off: np.array([off + 0.01, s, z]), y1)):
                a, b2 = _flip(oracle, right, make, c - 1e-3, c + 1e-3)
                for s in (np.nextafter(a, -np.inf), a, b2, np.nextafter(b2, np.inf)):
                    pts.append(make(s)); msd.append(3.0)
                edges.append((right, a, b2))
    for p in ([0.0, 0.0, 0.0], [0.1, 0.1, 0.0], [0.0, 0.0, 1e-9], [0.0, 0.0, 1e-30], [1e-12, 0.0, 1e-9], [1e-7, -1e-7, 1e-9],
              [0.0, 0.0, -1e-9], [0.1, 0.1, -2.0], [BL, 0.0, 1e-9]):
        pts.append(np.array(p)); msd.append(1.0)
    n_edge = len(pts)
    one2 = np.float32(1.2)
    for p in ([0.3, -0.2, 2.0], [-1.0, 0.5, 4.0], [BL + 0.2, 0.1, 1.7], [0.0, 0.0, 7.5]):
        p = np.array(p)
        dist = np.float32(np.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]))
        for right_dist in (False, True):
            if right_dist:
                q = p - np.array([BL, 0, 0])
                dist = np.float32(np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]))
            for k in range(-2, 10):
                m = dist
                for _ in range(abs(k)):
                    m = np.float32(m * one2) if k > 0 else np.float32(m / one2)
                for m3 in (np.nextafter(m, np.float32(0)), m, np.nextafter(m, np.float32(np.inf))):
                    pts.append(p); msd.append(m3)
    return np.array(pts), np.array(msd, np.float32), n_edge, edges


# ---- the first tryLambda of a solve started at the identity, restated in Python floats -------------------------------------------
def first_lm_step(case, st, lam=1e-5):
    """("cholesky-fails", None) or ("solved", linChange) for the first damped solve of the case, T0 = identity: the oracle's
    buildPoseFactors / poseFactorResidual / chol_solve operation for operation (Python floats are IEEE doubles; inf and NaN
    propagate as in C).  The oracle's report cannot tell a failed solve from a rejected step; this can."""
    assert np.array_equal(case["T0"], np.eye(4))
    H = [[0.0] * 6 for _ in range(6)]
    g = [0.0] * 6
    for i in factor_points(case):
        first, second = (int(v) for v in case["matches"][i])
        x, y, z = (float(v) for v in case["points"][i])
        if first >= 0:
            kp = case["kL"][first]
            ftype = 0 if (st["close"][first] and second >= 0) else 1
        else:
            kp = case["kR"][second]
            ftype = 2
        sigma = 1.0 / float(INV_SIGMA[kp["octave"]])
        s = 1.0 / sigma
        assert z > 0
        iz = 1.0 / z
        if ftype == 0:
            obs = (float(kp["x"]), float(case["kR"][second]["x"]), float(kp["y"]))
            r = [(FX * x * iz + CX - obs[0]) * s, (FX * (x - BL) * iz + CX - obs[1]) * s, (FY * y * iz + CY - obs[2]) * s]
            al = [[FX * iz, 0.0, -FX * x * iz * iz], [FX * iz, 0.0, -FX * (x - BL) * iz * iz], [0.0, FY * iz, -FY * y * iz * iz]]
        else:
            xx = x - BL if ftype == 2 else x
            r = [(FX * xx * iz + CX - float(kp["x"])) * s, (FY * y * iz + CY - float(kp["y"])) * s]
            al = [[FX * iz, 0.0, -FX * xx * iz * iz], [0.0, FY * iz, -FY * y * iz * iz]]
        S = [[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]]
        for a in range(len(r)):
            J = [(al[a][0] * S[0][c] + al[a][1] * S[1][c] + al[a][2] * S[2][c]) * s for c in range(3)] + [-al[a][c] * s for c in range(3)]
            for p in range(6):
                g[p] -= J[p] * r[a]
                for q in range(6):
                    H[p][q] += J[p] * J[q]
    A = [row[:] for row in H]
    for p in range(6):
        A[p][p] += lam
    b = g[:]
    for j in range(6):
        d = A[j][j]
        for k in range(j):
            d -= A[j][k] * A[j][k]
        if not d > 0:
            return "cholesky-fails", None
        d = float(np.sqrt(d))
        A[j][j] = d
        for i in range(j + 1, 6):
            v = A[i][j]
            for k in range(j):
                v -= A[i][k] * A[j][k]
            A[i][j] = v / d
    for i in range(6):
        v = b[i]
        for k in range(i):
            v -= A[i][k] * b[k]
        b[i] = v / A[i][i]
    for i in range(5, -1, -1):
        v = b[i]
        for k in range(i + 1, 6):
            v -= A[k][i] * b[k]
        b[i] = v / A[i][i]
    dg = dHd = 0.0
    for i in range(6):
        dg += b[i] * g[i]
        v = 0.0
        for j in range(6):
            v += H[i][j] * b[j]
        dHd += b[i] * v
    return "solved", dg - 0.5 * dHd
