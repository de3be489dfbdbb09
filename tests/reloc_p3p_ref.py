"""CPU restatement of relocalisation mode 1 (vslam_reloc_params::mode = 1: hypotheses from 2D-3D correspondences; rules in
DESIGN.md section 6 and include/vslam_hip.h).  Step A and the sampling hash are those of tests/reloc_ref.py; step B', the P3P
solver and the scoring are written out here in the kernel's order: fp64 `+ - * /` and sqrt only, explicit sums, every product
and sum associated as written, so that the device (built with -ffp-contract=off) reproduces every value bit for bit and with
it every decision.  Step D calls the oracle's motion-only pose solve.

The solver (a degenerate conic of the pencil, as in Lambda Twist - Persson & Nordberg, ECCV 2018):
  depths l = (l1, l2, l3) along the unit bearings y_k obey  l^T M12 l = a12, l^T M13 l = a13, l^T M23 l = a23  (a_ij the squared
  distances of the world points, M_ij built from c_ij = y_i . y_j).  D1 = a23 M12 - a12 M23 and D2 = a23 M13 - a13 M23 are
  homogeneous in l.  A real root g of det(D1 + g D2) = 0 (a cubic: fixed start, CUBIC_STEPS Newton steps) makes D0 = D1 + g D2
  a pair of planes.  The pair is split through adj(D0) = -p p^T: N = D0 + [p]x has rank one, its rows are multiples of one
  plane's normal and its columns of the other's.  Each plane gives l1 = w0 l2 + w1 l3; with tau = l3 / l2 the other conic of
  the pencil becomes a quadratic in tau, l2 follows from a23.  REFINE_STEPS Gauss-Newton steps on the three original equations
  polish (l1, l2, l3); the pose is the one between the world triple's and the camera triple's orthonormal frames (reloc_ref._frame).
Solution slots: 0, 1 = first plane (rows), smaller / larger tau; 2, 3 = second plane (columns)."""
import numpy as np
import reloc_ref as rr
from reloc_ref import CHI2, _frame

CUBIC_STEPS = 16
REFINE_STEPS = 3
F = np.float64


def params(**kw):
    mode = int(kw.pop("mode", 0) or 0)
    p = rr.params(**kw)
    p["mode"] = mode
    return p


# ---- step B': correspondences -------------------------------------------------------------------------------------------------
def pairs(key_winner, points, kL, kR, depth, right_idxs, rig):
    """every winning pair, in ascending key index: Xw (C, 3), y (C, 3) unit bearing, kx, ky, kxr (f4; 0 without the flag),
    octave, p, i, stereo (bool)"""
    i = np.array([k for k in range(len(key_winner)) if key_winner[k] >= 0], np.int64)
    C = len(i)
    p = key_winner[i].astype(np.int64) if C else np.zeros(0, np.int64)
    points = np.asarray(points, np.float64).reshape(-1, 3)
    kx = kL["x"][i].astype(np.float32); ky = kL["y"][i].astype(np.float32)
    bx = (kx.astype(F) - rig["cx"]) / rig["fx"]
    by = (ky.astype(F) - rig["cy"]) / rig["fy"]
    n = np.sqrt((bx * bx + by * by) + 1.0)
    y = np.stack([bx / n, by / n, 1.0 / n], axis=1) if C else np.zeros((0, 3))
    stereo = (depth[i] > 0) & (right_idxs[i] >= 0) if C else np.zeros(0, bool)
    kxr = np.zeros(C, np.float32)
    if C:
        kxr[stereo] = kR["x"][right_idxs[i][stereo]]
    return dict(Xw=points[p].copy() if C else np.zeros((0, 3)), y=y, kx=kx, ky=ky, kxr=kxr, octave=kL["octave"][i].astype(np.int32),
                p=p.astype(np.int32), i=i.astype(np.int32), stereo=stereo)


# ---- step C': the solver ------------------------------------------------------------------------------------------------------
def _adj(a00, a01, a02, a11, a12, a22):
    """adjugate of a symmetric 3 x 3 matrix, as (00, 01, 02, 11, 12, 22)"""
    return (a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11,
            a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01)


def _tr(A, b):
    """trace(A b) of two symmetric matrices given as sextuples"""
    return ((A[0] * b[0] + A[3] * b[3]) + A[5] * b[5]) + 2.0 * ((A[1] * b[1] + A[2] * b[2]) + A[4] * b[4])


def _rel(v, scale):
    return float(abs(v) / scale) if scale > 0 else np.inf


def _cubic_root(b, c, d, info):
    """a real root of x^3 + b x^2 + c x + d: a start outside the stationary points, then CUBIC_STEPS Newton steps"""
    bb = b * b; tc = 3.0 * c
    info["margin"] = min(info["margin"], _rel(bb - tc, bb + abs(tc)))
    if bb >= tc:
        v = np.sqrt(bb - tc)
        t1 = (-b - v) / 3.0
        k = ((t1 + b) * t1 + c) * t1 + d
        if k > 0:
            r = t1 - np.sqrt(-k / (3.0 * t1 + b))
        else:
            t2 = (-b + v) / 3.0
            k = ((t2 + b) * t2 + c) * t2 + d
            r = t2 + np.sqrt(-k / (3.0 * t2 + b))
    else:
        r = -b / 3.0
        s = (3.0 * r + 2.0 * b) * r + c
        if (-s if s < 0 else s) < 1e-4:
            r = r + 1.0
    for _ in range(CUBIC_STEPS):
        fx = ((r + b) * r + c) * r + d
        fp = (3.0 * r + 2.0 * b) * r + c
        r = r - fx / fp
    return r


def _sq(v):
    return (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]


def _first_max(a, b, c):
    """index of the first largest of three"""
    k = 0; m = a
    if b > m: k = 1; m = b
    if c > m: k = 2
    return k


def depths(X, y, keep_negative=False):
    """the four depth-triple slots (None = void) of three (world point, unit bearing) pairs, the shared world frame (None = the
    whole triple is void) and info: `margin`, the smallest relative distance from zero of a discriminant the solver branched on"""
    info = dict(margin=np.inf)
    none = [None] * 4
    with np.errstate(all="ignore"):
        X = [[F(v) for v in row] for row in X]
        y = [[F(v) for v in row] for row in y]
        e = _frame(*X)
        if e is None:                                    # coincident or collinear world points
            return none, None, info
        for (i, j) in ((0, 1), (0, 2), (1, 2)):           # coincident bearings
            n = [y[i][1] * y[j][2] - y[i][2] * y[j][1], y[i][2] * y[j][0] - y[i][0] * y[j][2], y[i][0] * y[j][1] - y[i][1] * y[j][0]]
            if _sq(n) < 1e-12:
                return none, None, info
        d = [X[0][k] - X[1][k] for k in range(3)]; a12 = _sq(d)
        d = [X[0][k] - X[2][k] for k in range(3)]; a13 = _sq(d)
        d = [X[1][k] - X[2][k] for k in range(3)]; a23 = _sq(d)
        c12 = (y[0][0] * y[1][0] + y[0][1] * y[1][1]) + y[0][2] * y[1][2]
        c13 = (y[0][0] * y[2][0] + y[0][1] * y[2][1]) + y[0][2] * y[2][2]
        c23 = (y[1][0] * y[2][0] + y[1][1] * y[2][1]) + y[1][2] * y[2][2]
        zero = F(0.0)
        D1 = (a23, -(a23 * c12), zero, a23 - a12, a12 * c23, -a12)
        D2 = (a23, zero, -(a23 * c13), -a13, a13 * c23, a23 - a13)
        A1 = _adj(*D1); A2 = _adj(*D2)
        k0 = (D1[0] * A1[0] + D1[1] * A1[1]) + D1[2] * A1[2]
        k3 = (D2[0] * A2[0] + D2[1] * A2[1]) + D2[2] * A2[2]
        k1 = _tr(A1, D2)
        k2 = _tr(A2, D1)
        g = _cubic_root(k2 / k3, k1 / k3, k0 / k3, info)
        D0 = tuple(D1[k] + g * D2[k] for k in range(6))
        B = _adj(*D0)
        # adj(D0) = -p p^T: the column of the most negative diagonal entry
        k = _first_max(-B[0], -B[3], -B[5])
        bm = (B[0], B[3], B[5])[k]
        if not (bm < 0):
            return none, e, info
        col = ((B[0], B[1], B[2]), (B[1], B[3], B[4]), (B[2], B[4], B[5]))[k]
        s = np.sqrt(-bm)
        p = [col[0] / s, col[1] / s, col[2] / s]
        N = [[D0[0], D0[1] - p[2], D0[2] + p[1]],
             [D0[1] + p[2], D0[3], D0[4] - p[0]],
             [D0[2] - p[1], D0[4] + p[0], D0[5]]]
        kr = _first_max(_sq(N[0]), _sq(N[1]), _sq(N[2]))
        cols = [[N[0][q], N[1][q], N[2][q]] for q in range(3)]
        kc = _first_max(_sq(cols[0]), _sq(cols[1]), _sq(cols[2]))
        ag = -g if g < 0 else g
        E = D2 if ag <= 1.0 else D1                       # the conic of the pencil farther from D0
        out = []
        for n in (N[kr], cols[kc]):
            w0 = -(n[1] / n[0]); w1 = -(n[2] / n[0])
            qa = ((E[0] * w1) * w1 + (2.0 * E[2]) * w1) + E[5]
            hb = ((E[0] * w0) * w1 + E[1] * w1) + (E[2] * w0 + E[4])
            qc = ((E[0] * w0) * w0 + (2.0 * E[1]) * w0) + E[3]
            h2 = hb * hb; ac = qa * qc
            disc = h2 - ac
            if np.isfinite(disc):
                info["margin"] = min(info["margin"], _rel(disc, h2 + abs(ac)))
            if not (disc >= 0):
                out += [None, None]
                continue
            sq = np.sqrt(disc)
            for tau in ((-hb - sq) / qa, (-hb + sq) / qa):
                den = tau * (tau - 2.0 * c23) + 1.0
                l2 = np.sqrt(a23 / den)
                l3 = tau * l2
                l1 = w0 * l2 + w1 * l3
                if not keep_negative and not (tau > 0 and l1 > 0):
                    out.append(None)
                    continue
                for _ in range(REFINE_STEPS):
                    h1 = 0.5 * (((l1 * l1 + l2 * l2) - ((2.0 * c12) * l1) * l2) - a12)
                    h2_ = 0.5 * (((l1 * l1 + l3 * l3) - ((2.0 * c13) * l1) * l3) - a13)
                    h3 = 0.5 * (((l2 * l2 + l3 * l3) - ((2.0 * c23) * l2) * l3) - a23)
                    j11 = l1 - c12 * l2; j12 = l2 - c12 * l1
                    j21 = l1 - c13 * l3; j23 = l3 - c13 * l1
                    j32 = l2 - c23 * l3; j33 = l3 - c23 * l2
                    det = -((j11 * j23) * j32) - (j12 * j21) * j33
                    u = h2_ * j33 - j23 * h3
                    d1 = (-(h1 * (j23 * j32)) - j12 * u) / det
                    d2 = (j11 * u - h1 * (j21 * j33)) / det
                    d3 = ((h1 * (j21 * j32) - j11 * (h2_ * j32)) - j12 * (j21 * h3)) / det
                    l1 = l1 - d1; l2 = l2 - d2; l3 = l3 - d3
                ok = np.isfinite(l1) and np.isfinite(l2) and np.isfinite(l3)
                if not keep_negative:
                    ok = ok and l1 > 0 and l2 > 0 and l3 > 0
                out.append((l1, l2, l3) if ok else None)
        return out, e, info


def p3p(X, y, keep_negative=False):
    """the four solution slots of three (world point, unit bearing) pairs: (R, t, depths) with camera = R world + t, or None"""
    lam, e, info = depths(X, y, keep_negative)
    sols = []
    with np.errstate(all="ignore"):
        for l in lam:
            if l is None:
                sols.append(None)
                continue
            Y = [[l[k] * F(y[k][q]) for q in range(3)] for k in range(3)]
            f = _frame(*Y)
            if f is None:
                sols.append(None)
                continue
            R = np.zeros((3, 3))
            for r in range(3):
                for c in range(3):
                    R[r, c] = f[0][r] * e[0][c] + f[1][r] * e[1][c] + f[2][r] * e[2][c]
            t = np.zeros(3)
            for r in range(3):
                t[r] = Y[0][r] - (R[r, 0] * F(X[0][0]) + R[r, 1] * F(X[0][1]) + R[r, 2] * F(X[0][2]))
            sols.append((R, t, l) if np.isfinite(R).all() and np.isfinite(t).all() else None)
    return sols, info


# ---- step C': scoring ---------------------------------------------------------------------------------------------------------
def chi2_values(rec, R, t, rig, inv_sigma):
    """(z, weighted squared residual) of every record under (R, t): three rows with the stereo flag, two without"""
    X = rec["Xw"]
    pc = [(R[r, 0] * X[:, 0] + R[r, 1] * X[:, 1] + R[r, 2] * X[:, 2]) + t[r] for r in range(3)]
    z = pc[2]
    b = F(np.float32(rig["bl"]))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        invZ = 1.0 / z
        eu = rec["kx"].astype(F) - (rig["fx"] * pc[0] * invZ + rig["cx"])
        ev = rec["ky"].astype(F) - (rig["fy"] * pc[1] * invZ + rig["cy"])
        eur = rec["kxr"].astype(F) - (rig["fx"] * (pc[0] - b) * invZ + rig["cx"])
        w = np.asarray(inv_sigma, np.float32)[rec["octave"]].astype(F)
        val = np.where(rec["stereo"], (eu * eu + ev * ev + eur * eur) * w, (eu * eu + ev * ev) * w)
    return z, val


def inliers(rec, R, t, rig, inv_sigma):
    z, val = chi2_values(rec, R, t, rig, inv_sigma)
    with np.errstate(invalid="ignore"):
        return (z > 0) & ~(val > CHI2)


def hypotheses(rec, rig, inv_sigma, n_hypotheses, seed):
    """as reloc_ref.hypotheses: counts per hypothesis (the largest over its solution slots, the lowest slot on a tie), the
    winner, its pose and flags, `slot` per hypothesis (-1 void) and `margin`: the smallest relative distance of a tested
    residual to the chi2 bound or of a solver discriminant to zero"""
    C = len(rec["i"])
    counts = np.zeros(n_hypotheses, np.int32)
    slot = np.full(n_hypotheses, -1, np.int32)
    poses = [None] * n_hypotheses
    margin = np.inf
    for h in range(n_hypotheses):
        idx = rr.sample(seed, h, C)
        if idx is None:
            continue
        sols, info = p3p(rec["Xw"][idx], rec["y"][idx])
        margin = min(margin, info["margin"])
        best = -1
        for s, sol in enumerate(sols):
            if sol is None:
                continue
            z, val = chi2_values(rec, sol[0], sol[1], rig, inv_sigma)
            front = z > 0
            with np.errstate(invalid="ignore"):
                n = int(np.count_nonzero(front & ~(val > CHI2)))
                if front.any():
                    margin = min(margin, float(np.nanmin(np.abs(val[front] - CHI2) / CHI2)))
            if n > best:
                best = n; slot[h] = s; poses[h] = sol
        if best >= 0:
            counts[h] = best
    best = int(np.argmax(counts))
    best_count = int(counts[best])
    flags = np.zeros(C, np.uint8)
    T_cw = np.zeros((4, 4))
    if best_count > 0:
        R, t, _ = poses[best]
        flags = inliers(rec, R, t, rig, inv_sigma).astype(np.uint8)
        T_cw[:3, :3] = R; T_cw[:3, 3] = t; T_cw[3, 3] = 1.0
    return dict(counts=counts, slot=slot, best=best, best_count=best_count, flags=flags, T_cw=T_cw, margin=margin)


# ---- the whole stage ----------------------------------------------------------------------------------------------------------
def relocalize(oracle, rig, inv_sigma, points, desc, kL, dL, kR, st, **kw):
    """mode 1 of reloc_ref.relocalize (same arguments and result fields)"""
    P = params(**kw)
    points = np.asarray(points, np.float64).reshape(-1, 3)
    N = len(points)
    d, key_winner = rr.match(desc, dL, P["max_hamming"], P["ratio_pct"])
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
    mt = np.stack([rec["i"][sel], st["rightIdxs"][rec["i"][sel]]], axis=1).astype(np.int32)      # (a -1 stays: a left-only factor)
    ones = np.ones(M, np.uint8); zeros = np.zeros(M, np.uint8)
    r = oracle.estimate_pose(rig, inv_sigma, rec["Xw"][sel], ones, ones, zeros, mt, zeros, kL, kR, st["rightIdxs"], st["leftIdxs"],
                             st["depth"], st["close"], hyp["T_cw"])
    out["n_inliers"], out["n_stereo"] = r["nIn"], r["nStereo"]
    out["success"] = int(r["nIn"] >= P["min_inliers"])
    if out["success"]:
        out["T_cw"] = r["T_cw"]
    out["refined"] = r
    return out
