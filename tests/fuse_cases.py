"""Inputs shared by the tests of the duplicate search and of the commit of vslam_system_fuse_loop: the small map on which every
case of the merge occurs (tests/test_fuse_ref.py works it by hand, tests/test_fuse_host.py sends it through csrc/fuse_host.hpp),
and the crafted point sets of tests/test_gpu_fuse.py."""
import numpy as np

# ---- the commit: six map points, three keyframes (left tables of 6 keys, right tables of 4) ------------------------------------------
# P0, P1, P2 are the old copy (created by keyframes 0 / 0 / 1), P3, P4, P5 the new one (keyframe 2).  Pairs: (3 -> 0), (4 -> 1).
#   P3 = [(kf 2, l 0, r 0), (kf 1, l 4, -)]: keyframe 2 does not see P0 -> moved; keyframe 1 sees P0 already -> dropped.  P3 is active.
#   P4 = [(kf 2, l 1, -), (kf 1, -, r 2)]:   keyframe 2 sees P1 already -> dropped; the right-only observation of keyframe 1 -> moved.
#                                            P4 is not active.
#   P0 (kept) is not active and is appended; P1 (kept) is active and stays where it is; P2, P5 take no part.
COMMIT_PAIRS = [(3, 0), (4, 1)]
COMMIT_KDX = [0, 0, 1, 2, 2, 2]
COMMIT_LAST_OBS = [1, 2, 1, 2, 2, 2]
COMMIT_OBS = [
    [(0, 0, 0), (1, 0, -1)],
    [(0, 1, -1), (2, 3, -1)],
    [(1, 2, 1)],
    [(2, 0, 0), (1, 4, -1)],
    [(2, 1, -1), (1, -1, 2)],
    [(2, 2, -1)],
]
COMMIT_ACTIVE = [1, 2, 3, 5]
COMMIT_OUTLIER = [0, 0, 0, 0, 0, 0]
COMMIT_IN_FRAME = [0, 1, 1, 1, 0, 1]
N_LEFT, N_RIGHT = 6, 4


def commit_tables(obs=COMMIT_OBS, kdx=COMMIT_KDX, n_kf=3):
    """the keyframes' tables that belong to a list of observations"""
    t = [dict(lmpL=[-1] * N_LEFT, lmpR=[-1] * N_RIGHT, unF=[-1] * N_LEFT, unFR=[-1] * N_RIGHT) for _ in range(n_kf)]
    for m, lst in enumerate(obs):
        for kf, l, r in lst:
            if l >= 0:
                t[kf]["lmpL"][l] = m; t[kf]["unF"][l] = kdx[m]
            if r >= 0:
                t[kf]["lmpR"][r] = m; t[kf]["unFR"][r] = kdx[m]
    return t


# ---- the search: crafted records --------------------------------------------------------------------------------------------------
# identity pose, fx = fy = 1, cx = cy = 0: a point (u z, v z, z) with small integers u, v and a power-of-two-ish z projects to
# exactly (u, v, z) in fp64 and in float, so every gate below is decided by the written numbers alone
K_UNIT = (1.0, 1.0, 0.0, 0.0)
SIZE = (640, 480)
EYE = np.eye(4)


def points(uvz):
    """world points whose records under (EYE, K_UNIT) are the given (u, v, z) rows (z > 0), or exactly (x, y, z) for z <= 0"""
    a = np.asarray(uvz, np.float64).reshape(-1, 3)
    out = a.copy()
    pos = a[:, 2] > 0
    out[pos, 0] = a[pos, 0] * a[pos, 2]
    out[pos, 1] = a[pos, 1] * a[pos, 2]
    return out


def desc_with_bits(base, n, start=0):
    """a copy of descriptor `base` (32 bytes) with bits start .. start + n - 1 flipped: Hamming distance n"""
    d = np.array(base, np.uint8, copy=True)
    for b in range(start, start + n):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def random_desc(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)
