"""CPU restatement of the relocalisation stage (vslam_relocalize, include/vslam_hip.h; rules in DESIGN.md section 6).

The stage has no counterpart in the reference, so this file plays the role the oracle plays for the other stages: steps A - C
are written out from the rules, integer parts exact and fp64 arithmetic in the stated order (explicit sums, no dot products,
so that nothing is re-associated or fused); step D calls the oracle's motion-only pose solve.  tests/test_reloc_ref.py checks
this file on its own, tests/test_gpu_reloc.py pins the kernels to it."""
import numpy as np

DEFAULTS = dict(max_hamming=50, ratio_pct=80, n_hypotheses=256, seed=0x52454C4F, min_inliers=50)
CHI2 = 7.815
M32 = 0xFFFFFFFF


def params(**kw):
    """a zero / absent field takes its default"""
    p = dict(DEFAULTS)
    for k, v in kw.items():
        assert k in p, k
        if v:
            p[k] = int(v)
    return p


# ---- step A: global descriptor match ------------------------------------------------------------------------------------------
def hamming_matrix(desc_p, desc_l):
    a = np.ascontiguousarray(desc_p, np.uint8).reshape(-1, 32).view(np.uint64)      # (N, 4)
    b = np.ascontiguousarray(desc_l, np.uint8).reshape(-1, 32).view(np.uint64)      # (nL, 4)
    out = np.zeros((len(a), len(b)), np.int32)
    for s in range(0, len(a), 1024):
        x = a[s:s + 1024, None, :] ^ b[None, :, :]
        out[s:s + 1024] = np.bitwise_count(x).sum(axis=2, dtype=np.int32)
    return out


def match(desc_p, desc_l, max_hamming, ratio_pct):
    """returns d (N, 3) = (d1, i1, d2) per map point and key_winner (nL) = winning map point per key or -1"""
    N, nL = len(desc_p), len(desc_l)
    d = np.zeros((N, 3), np.int32)
    d[:, 0] = 257; d[:, 1] = -1; d[:, 2] = 257
    key_winner = np.full(nL, -1, np.int32)
    if N == 0 or nL == 0:
        return d, key_winner
    H = hamming_matrix(desc_p, desc_l)
    i1 = np.argmin(H, axis=1)                       # (first occurrence = lowest key index)
    d1 = H[np.arange(N), i1]
    if nL > 1:
        H2 = H.copy()
        H2[np.arange(N), i1] = 1 << 20
        d2 = H2.min(axis=1)
    else:
        d2 = np.full(N, 257, np.int32)
    d[:, 0] = d1; d[:, 1] = i1; d[:, 2] = d2
    best = {}
    for p in range(N):
        if int(d1[p]) <= max_hamming and 100 * int(d1[p]) < ratio_pct * int(d2[p]):
            packed = (int(d1[p]) << 32) | p
            k = int(i1[p])
            if k not in best or packed < best[k]:
                best[k] = packed
    for k, packed in best.items():
        key_winner[k] = packed & M32
    return d, key_winner


# ---- step B: correspondences -----------------------------------------------------------------------------------------------
def pairs(key_winner, points, kL, kR, depth, right_idxs, rig):
    """records in ascending key index: dict of arrays Xw (C, 3), Xc (C, 3), kx, ky, kxr (f4), octave, p, i"""
    keep = [i for i in range(len(key_winner)) if key_winner[i] >= 0 and depth[i] > 0 and right_idxs[i] >= 0]
    i = np.array(keep, np.int64)
    p = key_winner[i].astype(np.int64) if len(i) else np.zeros(0, np.int64)
    points = np.asarray(points, np.float64).reshape(-1, 3)
    zp = depth[i].astype(np.float64)
    kx = kL["x"][i].astype(np.float32); ky = kL["y"][i].astype(np.float32)
    Xc = np.zeros((len(i), 3))
    Xc[:, 0] = (kx.astype(np.float64) - rig["cx"]) * zp / rig["fx"]
    Xc[:, 1] = (ky.astype(np.float64) - rig["cy"]) * zp / rig["fy"]
    Xc[:, 2] = zp
    kxr = kR["x"][right_idxs[i]].astype(np.float32) if len(i) else np.zeros(0, np.float32)
    return dict(Xw=points[p].copy() if len(i) else np.zeros((0, 3)), Xc=Xc, kx=kx, ky=ky, kxr=kxr,
                octave=kL["octave"][i].astype(np.int32), p=p.astype(np.int32), i=i.astype(np.int32))


# ---- step C: hypotheses ----------------------------------------------------------------------------------------------------
def mix(s, h, j):
    x = (s ^ ((h * 0x9E3779B9) & M32) ^ ((j * 0x85EBCA6B) & M32)) & M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def sample(seed, h, C):
    """three distinct record indices of hypothesis h, or None (void)"""
    if C < 3:
        return None
    idx = []
    for j in range(16):
        v = (mix(seed, h, j) * C) >> 32
        if v not in idx:
            idx.append(v)
            if len(idx) == 3:
                return idx
    return None


def _frame(P0, P1, P2):
    a = [P1[k] - P0[k] for k in range(3)]
    na2 = a[0] * a[0] + a[1] * a[1] + a[2] * a[2]
    if na2 < 1e-12:
        return None
    na = np.sqrt(na2)
    e1 = [a[k] / na for k in range(3)]
    c = [P2[k] - P0[k] for k in range(3)]
    n = [e1[1] * c[2] - e1[2] * c[1], e1[2] * c[0] - e1[0] * c[2], e1[0] * c[1] - e1[1] * c[0]]
    nn2 = n[0] * n[0] + n[1] * n[1] + n[2] * n[2]
    if nn2 < 1e-12:
        return None
    nn = np.sqrt(nn2)
    e3 = [n[k] / nn for k in range(3)]
    e2 = [e3[1] * e1[2] - e3[2] * e1[1], e3[2] * e1[0] - e3[0] * e1[2], e3[0] * e1[1] - e3[1] * e1[0]]
    return e1, e2, e3


def triad(A, B):
    """camera <- world pose (R, t) with B_k = R A_k + t from three point pairs (rows of A: world, of B: camera), or None"""
    A = [[np.float64(v) for v in row] for row in A]
    B = [[np.float64(v) for v in row] for row in B]
    e = _frame(*A)
    if e is None:
        return None
    f = _frame(*B)
    if f is None:
        return None
    R = np.zeros((3, 3))
    for r in range(3):
        for c in range(3):
            R[r, c] = f[0][r] * e[0][c] + f[1][r] * e[1][c] + f[2][r] * e[2][c]
    t = np.zeros(3)
    for r in range(3):
        t[r] = B[0][r] - (R[r, 0] * A[0][0] + R[r, 1] * A[0][1] + R[r, 2] * A[0][2])
    return R, t


def chi2_values(rec, R, t, rig, inv_sigma):
    """(z, weighted squared stereo residual) of every record under (R, t); the value is meaningful where z > 0"""
    X = rec["Xw"]
    pc = [(R[r, 0] * X[:, 0] + R[r, 1] * X[:, 1] + R[r, 2] * X[:, 2]) + t[r] for r in range(3)]
    z = pc[2]
    b = np.float64(np.float32(rig["bl"]))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        invZ = 1.0 / z
        eu = rec["kx"].astype(np.float64) - (rig["fx"] * pc[0] * invZ + rig["cx"])
        ev = rec["ky"].astype(np.float64) - (rig["fy"] * pc[1] * invZ + rig["cy"])
        eur = rec["kxr"].astype(np.float64) - (rig["fx"] * (pc[0] - b) * invZ + rig["cx"])
        val = (eu * eu + ev * ev + eur * eur) * np.asarray(inv_sigma, np.float32)[rec["octave"]].astype(np.float64)
    return z, val


def inliers(rec, R, t, rig, inv_sigma):
    z, val = chi2_values(rec, R, t, rig, inv_sigma)
    with np.errstate(invalid="ignore"):
        return (z > 0) & ~(val > CHI2)


def hypotheses(rec, rig, inv_sigma, n_hypotheses, seed):
    """counts per hypothesis, the winner (lowest h among the largest counts), its pose and inlier flags, and `margin`: the
    smallest relative distance of any tested residual (z > 0, any valid hypothesis) to the chi2 bound"""
    C = len(rec["i"])
    counts = np.zeros(n_hypotheses, np.int32)
    poses = [None] * n_hypotheses
    margin = np.inf
    for h in range(n_hypotheses):
        idx = sample(seed, h, C)
        if idx is None:
            continue
        T = triad(rec["Xw"][idx], rec["Xc"][idx])
        if T is None:
            continue
        poses[h] = T
        z, val = chi2_values(rec, T[0], T[1], rig, inv_sigma)
        front = z > 0
        with np.errstate(invalid="ignore"):
            counts[h] = int(np.count_nonzero(front & ~(val > CHI2)))
            if front.any():
                margin = min(margin, float(np.nanmin(np.abs(val[front] - CHI2) / CHI2)))
    best = int(np.argmax(counts))                  # first maximum = lowest h
    best_count = int(counts[best])
    flags = np.zeros(C, np.uint8)
    T_cw = np.zeros((4, 4))
    if best_count > 0:
        R, t = poses[best]
        flags = inliers(rec, R, t, rig, inv_sigma).astype(np.uint8)
        T_cw[:3, :3] = R; T_cw[:3, 3] = t; T_cw[3, 3] = 1.0
    return dict(counts=counts, best=best, best_count=best_count, flags=flags, T_cw=T_cw, margin=margin)


# ---- the whole stage -------------------------------------------------------------------------------------------------------
def relocalize(oracle, rig, inv_sigma, points, desc, kL, dL, kR, st, **kw):
    """st: the frame's stereo state (rightIdxs, leftIdxs, depth, close).  Returns the report fields, T_cw (None on
    failure), pairs (N: key index or -1) and the intermediate results of steps A - C."""
    P = params(**kw)
    points = np.asarray(points, np.float64).reshape(-1, 3)
    N = len(points)
    d, key_winner = match(desc, dL, P["max_hamming"], P["ratio_pct"])
    rec = pairs(key_winner, points, kL, kR, st["depth"], st["rightIdxs"], rig)
    C = len(rec["i"])
    pr = np.full(N, -1, np.int32)
    pr[rec["p"]] = rec["i"]
    out = dict(success=0, n_points=N, n_pairs=C, best_hypothesis=0, best_count=0, n_inliers=0, n_stereo=0, T_cw=None, pairs=pr,
               d=d, key_winner=key_winner, rec=rec, hyp=None)
    hyp = hypotheses(rec, rig, inv_sigma, P["n_hypotheses"], P["seed"])
    out["hyp"] = hyp
    out["best_hypothesis"], out["best_count"] = hyp["best"], hyp["best_count"]
    if C < 3 or hyp["best_count"] <= 0:
        return out
    sel = np.nonzero(hyp["flags"])[0]
    M = len(sel)
    mt = np.stack([rec["i"][sel], st["rightIdxs"][rec["i"][sel]]], axis=1).astype(np.int32)
    ones = np.ones(M, np.uint8); zeros = np.zeros(M, np.uint8)
    r = oracle.estimate_pose(rig, inv_sigma, rec["Xw"][sel], ones, ones, zeros, mt, zeros, kL, kR, st["rightIdxs"], st["leftIdxs"],
                             st["depth"], st["close"], hyp["T_cw"])
    out["n_inliers"], out["n_stereo"] = r["nIn"], r["nStereo"]
    out["success"] = int(r["nIn"] >= P["min_inliers"])
    if out["success"]:
        out["T_cw"] = r["T_cw"]
    out["refined"] = r
    return out
