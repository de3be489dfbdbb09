"""Crafted windows for the new-point search (LocalMapper::findNewPoints: calcAllMpsOfKFROnlyEst, predictKeysPosR,
matchByProjectionRPredLBA, triangulateNewPoints, checkReprojError), shared by tests/test_oracle_newpts.py (CPU: every
case proves, with the oracle and the numpy restatement below, that it is in the regime it is named after) and
tests/test_gpu_newpts.py (GPU: parity on the same cases).  A plain module, not a conftest.  No images: keys,
descriptors, poses, unF / unFR, depth and map points are host-supplied; an oracle.Extractor only lends scalePyramid
and sigmaFactor.

THE RESTATEMENT (`candidates`, `pair`, `window`) is the per-(candidate, keyframe) rule written from the reference's
rule in Python, with the reference's types: projection in float64 (Python floats, evaluated left to right, no fused
multiply-add), maxDistScale / dist / dif and the ratio test in float32, predScale = ceil in double.  It says which gate
decided a pair:  skip, behind, outL, outR, no_key, octave, radius, unF, dist>50, ratio, parallax, matched-left,
matched-right  (when no key is admitted, the verdict is the furthest gate a key of either side reached; an
out-of-frame side counts as the earliest) and returns the best / second key of each side as (dist, level, visit
position, index).

CRAFTING.  A probe is a last-keyframe key with hasMp = 1, unF < 0 and explicit mpXyz / mpDesc, so its world point and
descriptor are free.  Its predicted pixel in the target keyframe comes from the restatement, the target keys sit at
chosen offsets from it, descriptors are the probe's with a chosen number of bits flipped.  Probes sit on a 72 x 64 px
grid of spots; `Builder.finish` asserts that no pair's 15 px neighbourhood holds a key of another probe.  Every
matching case has ten ordinary filler candidates that match in three keyframes and triangulate.

Rotations: the last keyframe and the target keyframes are axis-aligned, so that the border and predScale probes can be
placed to the last bit; the filler-only keyframes are yawed.

Nothing was found unreachable: the rank-deficient DLT (all rays identical: left-only keys at one pixel in keyframes
that share the last keyframe's pose, the map point off that ray so that the parallax gate, which looks at the
PREDICTED pixel, passes) and the cheirality reject (diverging rays from keyframes millimetres apart) are both built
and checked with oracle.triangulate_dlt.
"""
import math
import numpy as np

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
F32 = np.float32
RIG_NAMES = ("euroc", "kitti")
PORTRAIT = dict(w=480, h=752, cx=240.0, cy=376.0)        # overrides of synth.RIGS["euroc"]


# ---------------------------------------------------------------------------------------------------------------------
# the rule restated
class Geo:
    """rig + pyramid tables + the matching grid of assignKeysToGrids"""

    def __init__(self, rig, scale_pyramid, sigma_factor):
        self.rig = rig
        self.sp = np.asarray(scale_pyramid, F32)
        self.sigma = np.asarray(sigma_factor, F32)
        self.nLev = len(self.sp)
        self.logScale = F32(math.log(float(self.sp[1])))
        w, h = rig["w"], rig["h"]
        self.xGrids = 64
        self.yGrids = int(math.ceil(float(F32(64) / (F32(w) / F32(h)))))
        self.xMult, self.yMult = F32(self.xGrids) / F32(w), F32(self.yGrids) / F32(h)
        self.b = float(F32(rig["bl"]))
        # True: the scans behave as with the former key layout (12-bit cell field): a key whose cell index is >= 4096
        # is read with dist | 1 and visited at cell & 4095.  Only the portrait proofs set it, to show what that changes.
        self.old_cell_field = False


def _inv_pose(T):
    R, t = T[:3, :3], T[:3, 3]
    Ri = [[float(R[c][r]) for c in range(3)] for r in range(3)]
    ti = [-(Ri[r][0] * float(t[0]) + Ri[r][1] * float(t[1]) + Ri[r][2] * float(t[2])) for r in range(3)]
    return Ri, ti


def _to_cam(T_wc, X):
    R, t = _inv_pose(T_wc)
    return [R[r][0] * X[0] + R[r][1] * X[1] + R[r][2] * X[2] + t[r] for r in range(3)]


def _dist32(X, T_wc):
    d = [X[k] - float(T_wc[k, 3]) for k in range(3)]
    return F32(math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))


def candidates(g, kfs, last):
    """calcAllMpsOfKFROnlyEst -> list of dict(key, keyR, X, mds, desc) in the order of the last keyframe's keys"""
    k0, out = kfs[0], []
    T = k0["T_wc"]
    for i in range(len(k0["kpsL"])):
        if not last["hasMp"][i]:
            if not last["depth"][i] > 0:
                continue
            z = float(last["depth"][i])
            pc = [(float(k0["kpsL"]["x"][i]) - g.rig["cx"]) * z / g.rig["fx"], (float(k0["kpsL"]["y"][i]) - g.rig["cy"]) * z / g.rig["fy"], z]
            X = [float(T[r, 0]) * pc[0] + float(T[r, 1]) * pc[1] + float(T[r, 2]) * pc[2] + float(T[r, 3]) for r in range(3)]
            desc = k0["descL"][i]
        else:
            if k0["unF"][i] >= 0:
                continue
            X = [float(v) for v in last["mpXyz"][i]]
            desc = last["mpDesc"][i]
        mds = _dist32(X, T) * g.sp[int(k0["kpsL"]["octave"][i])]
        out.append(dict(key=i, keyR=int(k0["rightIdxs"][i]), X=X, mds=F32(mds), desc=np.asarray(desc, np.uint8)))
    return out


def predict(g, X, mds, T_wc):
    """predictKeysPosR + the scale prediction -> dict(z, hasL, hasR, pL, pR (float32 pairs), predScale, radius)"""
    rig = g.rig
    p = _to_cam(T_wc, X)
    r = dict(z=p[2], hasL=False, hasR=False, pL=(F32(0), F32(0)), pR=(F32(0), F32(0)))
    if not p[2] <= 0.0:
        invZ = 1.0 / p[2]
        u, v = rig["fx"] * p[0] * invZ + rig["cx"], rig["fy"] * p[1] * invZ + rig["cy"]
        uR = rig["fx"] * (p[0] - g.b) * invZ + rig["cx"]
        r["uv"] = (u, v, uR)
        w, h = rig["w"], rig["h"]
        if not (u < 15 or v < 15 or u >= w - 15 or v >= h - 15):
            r["hasL"], r["pL"] = True, (F32(u), F32(v))
        if not (uR < 15 or v < 15 or uR >= w - 15 or v >= h - 15):
            r["hasR"], r["pR"] = True, (F32(uR), F32(v))
    dif = F32(mds) / _dist32(X, T_wc)
    q = math.log(float(dif)) / float(g.logScale)
    ps = int(math.ceil(q))
    r["q"], r["dif"] = q, dif
    r["predScale"] = min(max(ps, 0), g.nLev - 1)
    r["radius"] = g.sp[r["predScale"]] * F32(4)
    return r


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(np.asarray(a, np.uint8), np.asarray(b, np.uint8))).sum())


_STAGES = ("out", "no_key", "octave", "radius", "unF")


def scan(g, px, py, ps, radius, kps, descs, unF, desc, sic):
    """One side of matchByProjectionRPredLBA: the keys of the grid window in the reference's visit order (rows, columns,
    then the order within a cell), its three tests, then the best / second bookkeeping.  sic: the left scan's rule for
    the level of a later-visited second.  -> dict(stage, best, sec, admitted, clamped)"""
    fl, ce = (lambda v: int(math.floor(float(v)))), (lambda v: int(math.ceil(float(v))))
    minX, maxX = max(0, fl((px - radius) * g.xMult)), min(g.xGrids - 1, ce((px + radius) * g.xMult))
    minY, maxY = max(0, fl((py - radius) * g.yMult)), min(g.yGrids - 1, ce((py + radius) * g.yMult))
    res = dict(stage="no_key", best=None, sec=None, admitted=[], clamped=[], seen=[])
    if minX >= g.xGrids or minY >= g.yGrids or maxX < 0 or maxY < 0:
        return res
    order = []
    for i in range(len(kps)):
        kx, ky = F32(kps["x"][i]), F32(kps["y"][i])
        rx, ry = int(np.rint(kx * g.xMult)), int(np.rint(ky * g.yMult))
        cx, cy = min(max(rx, 0), g.xGrids - 1), min(max(ry, 0), g.yGrids - 1)
        if minX <= cx <= maxX and minY <= cy <= maxY:
            cell = cy * g.xGrids + cx
            wrapped = g.old_cell_field and cell >= 4096
            order.append((cell & 4095 if wrapped else cell, i, cell, (rx, ry) != (cx, cy), int(wrapped)))
    order.sort()
    stage = 1
    best = sec = None          # (dist, level, visit position, index) / (dist, level2, visit position)
    for _, i, cell, clamped, bump in order:
        res["seen"].append(i)
        lev = int(kps["octave"][i])
        if lev > ps + 1 or lev < ps - 1:
            stage = max(stage, 2); continue
        if not (abs(F32(kps["x"][i]) - px) < radius and abs(F32(kps["y"][i]) - py) < radius):
            stage = max(stage, 3); continue
        if unF[i] >= 0:
            stage = max(stage, 4); continue
        res["admitted"].append(i)
        if clamped:
            res["clamped"].append(i)
        vp = (cell, i)
        dd = hamming(desc, descs[i]) | bump
        bd, sd = (best[0] if best else 256), (sec[0] if sec else 256)
        if dd < bd:
            if best:
                sec = (best[0], best[1], best[2])
            best = (dd, lev, vp, i)
        elif dd < sd:
            sec = (dd, best[1] if sic else lev, vp) if best else None
            if not best:       # a 256-bit key before any best: the reference leaves bestLev2 = bestLev = -1
                sec = None
    res["stage"] = "ok" if res["admitted"] else _STAGES[stage]
    res["best"], res["sec"] = best, sec
    return res


def pair(g, cand, kfs, k):
    """-> dict(verdict, hasL, hasR, predScale, radius, pL, pR, left, right (scan results), out (l, r) or None)"""
    K, k0 = kfs[k], kfs[0]
    if K["id"] == k0["id"]:
        return dict(verdict="skip", out=None)
    r = predict(g, cand["X"], cand["mds"], K["T_wc"])
    r["out"] = None
    if r["z"] <= 0.0:
        r["verdict"] = "behind"
        return r
    ps, rad = r["predScale"], r["radius"]
    L = Rr = dict(stage="out", best=None, sec=None, admitted=[], clamped=[], seen=[])
    if r["hasL"] and r["pL"][0] > 0 and r["pL"][1] > 0:
        L = scan(g, r["pL"][0], r["pL"][1], ps, rad, K["kpsL"], K["descL"], K["unF"], cand["desc"], True)
    if r["hasR"] and r["pR"][0] > 0 and r["pR"][1] > 0:
        Rr = scan(g, r["pR"][0], r["pR"][1], ps, rad, K["kpsR"], K["descR"], K["unFR"], cand["desc"], False)
    r["left"], r["right"] = L, Rr
    bdL, bdR = (L["best"][0] if L["best"] else 256), (Rr["best"][0] if Rr["best"] else 256)
    right = bdL > bdR
    S = Rr if right else L
    r["side"] = "right" if right else "left"
    if S["best"] is None:
        if L["admitted"] or Rr["admitted"]:
            r["verdict"] = "dist>50"            # only 256-bit keys
            return r
        sl, sr = _STAGES.index(L["stage"]), _STAGES.index(Rr["stage"])
        name = Rr["stage"] if sr > sl else L["stage"]
        r["verdict"] = ("outR" if sr > sl else "outL") if name == "out" else name
        return r
    bd, lev = S["best"][0], S["best"][1]
    sd, lev2 = (S["sec"][0], S["sec"][1]) if S["sec"] else (256, -1)
    if bd > 50:
        r["verdict"] = "dist>50"
        return r
    if lev == lev2 and F32(bd) >= F32(0.6) * F32(sd):
        r["verdict"] = "ratio"
        return r
    keyL, keyR = cand["key"], cand["keyR"]
    if right:
        kk = k0["kpsR"][keyR] if keyR >= 0 else k0["kpsL"][keyL]
        pp = r["pR"]
    else:
        kk, pp = k0["kpsL"][keyL], r["pL"]
    dx, dy = float(pp[0]) - float(kk["x"]), float(pp[1]) - float(kk["y"])
    r["parallax"] = math.sqrt(dx * dx + dy * dy)
    if not r["parallax"] > 10.0:
        r["verdict"] = "parallax"
        return r
    bi = S["best"][3]
    if right:
        l = int(K["leftIdxs"][bi])
        r["out"], r["verdict"] = (l if l >= 0 else -1, bi), "matched-right"
    else:
        rr = int(K["rightIdxs"][bi])
        r["out"], r["verdict"] = (bi, rr if rr >= 0 else -1), "matched-left"
    return r


def window(g, kfs, last):
    """-> (candidates, pairs[c][k] for k >= 1, raw[c] = [(0, keyL, keyR), (k, l, r) ...] before triangulation)"""
    cands = candidates(g, kfs, last)
    pairs, raw = [], []
    for c in cands:
        row, obs = {}, [(0, c["key"], c["keyR"])]
        for k in range(1, len(kfs)):
            row[k] = pair(g, c, kfs, k)
            if row[k]["out"] is not None:
                obs.append((k,) + row[k]["out"])
        pairs.append(row); raw.append(obs)
    return cands, pairs, raw


# ---------------------------------------------------------------------------------------------------------------------
# building
def flip(desc, nbits, start=0):
    """desc with bits start .. start + nbits - 1 inverted (Hamming distance nbits to the original)"""
    d = np.array(desc, np.uint8, copy=True)
    for b in range(start, start + nbits):
        d[(b >> 3) % 32] ^= np.uint8(1 << (b & 7))
    return d


def _pose(t, yaw=0.0):
    T = np.eye(4)
    c, s = math.cos(yaw), math.sin(yaw)
    T[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    T[:3, 3] = t
    return T


def straddle(f, lo, hi):
    """f(lo) is False, f(hi) is True, f monotone: -> adjacent doubles (a, b) with f(a) False and f(b) True"""
    assert not f(lo) and f(hi)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        if f(mid):
            hi = mid
        else:
            lo = mid
    return lo, hi


class Case:
    """name, g (Geo), kfs, last, probes {name: dict(key, kf, expect)}, finals {name: dict(accepted, nObs, rows)},
    min_accepted, min_rejected; cands / pairs / raw = the restatement's view of the window."""


class _Probe:
    pass


class Builder:
    Z = 4.0                      # depth of the ordinary points; keyframe offsets are given as pixel shifts at this depth

    def __init__(self, g, name, shifts=((28, 2), (-36, 3), (32, -6)), yaws=(0.0, 0.01, -0.008), last_z=0.0, ids=None, seed=11):
        self.g, self.name = g, name
        self.rng = np.random.default_rng(seed)
        rig = g.rig
        self.kf = [dict(T_wc=_pose([0, 0, last_z]), id=100, L=[], R=[])]
        for i, (sx, sy) in enumerate(shifts):
            t = [sx * self.Z / rig["fx"], sy * self.Z / rig["fy"], 0.0]
            self.kf.append(dict(T_wc=_pose(t, yaws[i] if i < len(yaws) else 0.0), id=(ids[i] if ids else 101 + i), L=[], R=[]))
        self.last = []           # entries of the last keyframe, in key order
        self.lastR = []
        self.probes, self.finals = {}, {}
        self.disp = rig["fx"] * g.b / self.Z
        mx = max(abs(s[0]) for s in shifts) if shifts else 0
        u0 = 30 + mx + self.disp + 20
        self.spots = [(float(u), float(v)) for v in range(50, rig["h"] - 45, 64) for u in np.arange(u0, rig["w"] - 30 - mx - 20, 72)]
        self.nspot = 0

    # -- geometry
    def spot(self, corner=False):
        u, v = self.spots[self.nspot]
        self.nspot += 1
        if corner:               # on a corner of four grid cells (cells are rounded: boundaries at half-integers)
            g = self.g
            u = (round(u * float(g.xMult) - 0.5) + 0.5) / float(g.xMult)
            v = (round(v * float(g.yMult) - 0.5) + 0.5) / float(g.yMult)
        return u, v

    def world(self, k, u, v, z=None):
        """the world point at pixel (u, v), depth z of keyframe k"""
        z = self.Z if z is None else z
        rig, T = self.g.rig, self.kf[k]["T_wc"]
        pc = np.array([(u - rig["cx"]) * z / rig["fx"], (v - rig["cy"]) * z / rig["fy"], z])
        return [float(x) for x in (T[:3, :3] @ pc + T[:3, 3])]

    def pix(self, k, X, right=False):
        p = _to_cam(self.kf[k]["T_wc"], X)
        rig = self.g.rig
        return (rig["fx"] * (p[0] - (self.g.b if right else 0.0)) / p[2] + rig["cx"], rig["fy"] * p[1] / p[2] + rig["cy"])

    def desc(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    # -- keys
    def key(self, k, side, x, y, octave, desc, unF=-1, owner=None):
        lst = self.kf[k]["R" if side else "L"]
        lst.append(dict(x=F32(x), y=F32(y), o=int(octave), d=np.array(desc, np.uint8), unF=unF, partner=-1, owner=owner))
        return len(lst) - 1

    def link(self, k, l, r):
        self.kf[k]["L"][l]["partner"] = r
        self.kf[k]["R"][r]["partner"] = l

    def last_key(self, x, y, octave, desc, hasMp=1, X=None, mpDesc=None, depth=0.0, unF=-1, right_xy=None, owner=None):
        e = dict(x=F32(x), y=F32(y), o=int(octave), d=np.array(desc, np.uint8), hasMp=hasMp, X=X if X is not None else [0.0, 0.0, 0.0],
                 mpDesc=np.array(mpDesc if mpDesc is not None else desc, np.uint8), depth=F32(depth), unF=unF, partner=-1, owner=owner)
        if right_xy is not None:
            self.lastR.append(dict(x=F32(right_xy[0]), y=F32(right_xy[1]), o=int(octave), d=np.array(desc, np.uint8), unF=-1, partner=e))
            e["partner"] = len(self.lastR) - 1
        self.last.append(e)
        return e

    # -- probes
    def probe(self, name, X, kf=1, o0=0, expect=None):
        """a map-point candidate at world point X; -> handle with the restatement's prediction in keyframe kf"""
        p = _Probe()
        p.name, p.X, p.kf, p.d = name, [float(x) for x in X], kf, self.desc()
        mds = _dist32(p.X, self.kf[0]["T_wc"]) * self.g.sp[o0]
        p.pr = predict(self.g, p.X, mds, self.kf[kf]["T_wc"])
        p.pL, p.pR, p.ps, p.rad = p.pr["pL"], p.pr["pR"], p.pr["predScale"], float(p.pr["radius"])
        if not p.pr["hasL"] and "uv" in p.pr:       # where the pixel would have been: for keys that must not be seen
            p.pL = (F32(p.pr["uv"][0]), F32(p.pr["uv"][1]))
        if not p.pr["hasR"] and "uv" in p.pr:
            p.pR = (F32(p.pr["uv"][2]), F32(p.pr["uv"][1]))
        p.e = self.last_key(float(p.pL[0]) + 30.0, float(p.pL[1]), o0, self.desc(), hasMp=1, X=p.X, mpDesc=p.d, owner=name)
        self.probes[name] = dict(entry=p.e, kf=kf, expect=dict(expect or {}))
        return p

    def at(self, name, kf=1, z=None, o0=0, corner=False, expect=None):
        u, v = self.spot(corner)
        return self.probe(name, self.world(kf, u, v, z), kf, o0, expect)

    def lkey(self, p, dx, dy, octave, bits, **kw):
        """a left key of the probe's target keyframe at its predicted left pixel + (dx, dy), `bits` away from its descriptor"""
        return self.key(p.kf, 0, float(p.pL[0]) + dx, float(p.pL[1]) + dy, octave, flip(p.d, bits, kw.pop("start", 0)), owner=p.name, **kw)

    def rkey(self, p, dx, dy, octave, bits, **kw):
        return self.key(p.kf, 1, float(p.pR[0]) + dx, float(p.pR[1]) + dy, octave, flip(p.d, bits, kw.pop("start", 0)), owner=p.name, **kw)

    def expect(self, p, **kw):
        self.probes[p.name]["expect"].update(kw)

    def track(self, name, X, kfs_sides, o0=0, octs=None, offs=None, last_sides="LR", last_off=(0.0, 0.0), depth_kind=False, bits=3):
        """a candidate observed at its true projections: kfs_sides = {k: "L" / "R" / "LR"}, offs = {(k, side): (dx, dy)}
        pixel offsets from the true projection, octs = {(k, side): octave} (default o0).  depth_kind: a stereo-depth
        candidate without a map point (its world point is then the back-projection of the float32 key and depth)."""
        octs, offs = octs or {}, offs or {}
        d = self.desc()
        u, v = self.pix(0, X)
        rxy = None
        if "R" in last_sides:
            uR, vR = self.pix(0, X, True)
            rxy = (uR, vR)
        zc = _to_cam(self.kf[0]["T_wc"], X)[2]
        e = self.last_key(u + last_off[0], v + last_off[1], o0, d if depth_kind else self.desc(), hasMp=0 if depth_kind else 1, X=X,
                          mpDesc=d, depth=zc if depth_kind else 0.0, right_xy=rxy, owner=name)
        idx = {}
        for k, sides in kfs_sides.items():
            l = r = None
            if "L" in sides:
                x, y = self.pix(k, X)
                dx, dy = offs.get((k, "L"), (0.0, 0.0))
                l = self.key(k, 0, x + dx, y + dy, octs.get((k, "L"), o0), flip(d, bits + k % 3), owner=name)
            if "R" in sides:
                x, y = self.pix(k, X, True)
                dx, dy = offs.get((k, "R"), (0.0, 0.0))
                r = self.key(k, 1, x + dx, y + dy, octs.get((k, "R"), o0), flip(d, bits + k % 3), owner=name)
            if l is not None and r is not None:
                self.link(k, l, r)
            idx[k] = (-1 if l is None else l, -1 if r is None else r)
        self.probes[name] = dict(entry=e, kf=None, expect={}, idx=idx)
        return e, idx

    def fillers(self, n=10, kfs=None):
        """ordinary candidates of both kinds, matched on both sides of every keyframe but the last -> accepted"""
        kfs = kfs if kfs is not None else [k for k in range(1, len(self.kf)) if self.kf[k]["id"] != self.kf[0]["id"]]
        for i in range(n):
            u, v = self.spot()
            X = self.world(1, u, v, self.Z * (0.92 + 0.02 * i))
            name = "fill%d" % i
            self.track(name, X, {k: "LR" for k in kfs}, o0=i % 3, depth_kind=bool(i % 2))
            if len(kfs) >= 2:
                self.finals[name] = dict(accepted=1, nObs=len(kfs) + 1)

    # -- assembly
    def finish(self, n_last=None, keep_pos=None, junk_seed=3):
        """n_last / keep_pos: pad the last keyframe to n_last keys with rejected ones (depth <= 0 without a map point, a
        map point with unF >= 0), the real entries landing on the ascending key indices keep_pos"""
        g, c = self.g, Case()
        c.name, c.g = self.name, g
        last = list(self.last)
        if n_last is not None:
            assert len(keep_pos) == len(last) and list(keep_pos) == sorted(set(keep_pos)) and keep_pos[-1] < n_last
            rng = np.random.default_rng(junk_seed)
            slots = [None] * n_last
            for e, pos in zip(last, keep_pos):
                slots[pos] = e
            for i in range(n_last):
                if slots[i] is None:
                    if i % 2:
                        slots[i] = dict(x=F32(rng.uniform(20, g.rig["w"] - 20)), y=F32(rng.uniform(20, g.rig["h"] - 20)), o=0, d=self.desc(), hasMp=0,
                                        X=[0.0, 0.0, 0.0], mpDesc=self.desc(), depth=F32(0.0 if i % 4 == 1 else -1.5), unF=-1, partner=-1, owner=None, junk=1)
                    else:
                        slots[i] = dict(x=F32(rng.uniform(20, g.rig["w"] - 20)), y=F32(rng.uniform(20, g.rig["h"] - 20)), o=1, d=self.desc(), hasMp=1,
                                        X=self.world(1, 300.0, 200.0), mpDesc=self.desc(), depth=F32(3.0), unF=int(i), partner=-1, owner=None, junk=1)
            last = slots
        for i, e in enumerate(last):
            e["index"] = i

        def keys(lst):
            a = np.zeros(len(lst), KP_DTYPE)
            for i, e in enumerate(lst):
                a["x"][i], a["y"][i], a["octave"][i], a["size"][i] = e["x"], e["y"], e["o"], 31.0
            return a

        def descs(lst):
            return np.array([e["d"] for e in lst], np.uint8).reshape(-1, 32)

        c.kfs = []
        for k, K in enumerate(self.kf):
            L, R = (last, self.lastR) if k == 0 else (K["L"], K["R"])
            if k == 0:
                ri = np.array([e["partner"] for e in L], np.int32).reshape(-1)
                li = np.array([e["partner"]["index"] for e in R], np.int32).reshape(-1)
            else:
                ri = np.array([e["partner"] for e in L], np.int32).reshape(-1)
                li = np.array([e["partner"] for e in R], np.int32).reshape(-1)
            c.kfs.append(dict(T_wc=K["T_wc"], id=K["id"], kpsL=keys(L), descL=descs(L), kpsR=keys(R), descR=descs(R), rightIdxs=ri, leftIdxs=li,
                              unF=np.array([e["unF"] for e in L], np.int32).reshape(-1), unFR=np.array([e["unF"] for e in R], np.int32).reshape(-1)))
        n0 = len(last)
        c.last = dict(depth=np.array([e["depth"] for e in last], F32).reshape(-1), hasMp=np.array([e["hasMp"] for e in last], np.uint8).reshape(-1),
                      mpXyz=np.array([e["X"] for e in last], np.float64).reshape(n0, 3), mpDesc=np.array([e["mpDesc"] for e in last], np.uint8).reshape(n0, 32))
        c.cands, c.pairs, c.raw = window(g, c.kfs, c.last)
        c.cand_of_key = {cd["key"]: i for i, cd in enumerate(c.cands)}
        c.probes = {}
        for name, p in self.probes.items():
            c.probes[name] = dict(key=p["entry"]["index"], cand=c.cand_of_key[p["entry"]["index"]], kf=p["kf"], expect=p["expect"], idx=p.get("idx"))
        c.finals = self.finals
        # isolation: whatever a pair's scans looked at belongs to its own probe
        owner_of = {cd["key"]: last[cd["key"]]["owner"] for cd in c.cands}
        for ci, cd in enumerate(c.cands):
            for k, pr in c.pairs[ci].items():
                for side, lst in (("left", self.kf[k]["L"]), ("right", self.kf[k]["R"])):
                    for i in pr.get(side, {}).get("seen", ()):
                        if lst[i]["owner"] != owner_of[cd["key"]] and "uv" in pr:
                            px = pr["pR" if side == "right" else "pL"]
                            assert max(abs(float(lst[i]["x"]) - float(px[0])), abs(float(lst[i]["y"]) - float(px[1]))) >= 15.0, \
                                (self.name, owner_of[cd["key"]], k, side, lst[i]["owner"])
        c.min_accepted = sum(1 for f in self.finals.values() if f.get("accepted"))
        c.min_rejected = len(c.cands) - c.min_accepted
        return c


# ---------------------------------------------------------------------------------------------------------------------
# match regimes (one target keyframe: 1; keyframes 2 and 3 hold filler keys only)
def case_gate_edges(g):
    b = Builder(g, "gate_edges"); b.fillers()
    rig, Z = g.rig, Builder.Z
    w, h = rig["w"], rig["h"]
    T1 = b.kf[1]["T_wc"]
    rows = [v for v in range(60, h - 60, 56)]

    def X_at(u, v):
        return b.world(1, u, v)

    def edge(axis, thresh, other, names, expects, right_keys):
        span = 2.0 * Z / rig["fx"]
        for which, name, ex in zip((0, 1), names, expects):      # (the two sides 40 px apart: they are doubles apart otherwise)
            o = other + 40.0 * which
            X0 = X_at(thresh if axis == 0 else o, o if axis == 0 else thresh)

            def f(x):
                X = list(X0); X[axis] = x
                return predict(g, X, F32(1), T1)["uv"][axis] >= thresh
            X = list(X0); X[axis] = straddle(f, X0[axis] - span, X0[axis] + span)[which]
            p = b.probe(name, X, expect=ex)
            b.lkey(p, 0.0, 0.0, p.ps, 2)
            if right_keys:
                b.rkey(p, 0.0, 0.0, p.ps, 2)
    ML, MR = "matched-left", "matched-right"
    # u < 15 is out, u == 15 is in (the right pixel, a disparity further left, is out either way)
    edge(0, 15.0, rows[0] + 0.0, ("u_lo", "u_at"), (dict(verdict="outL", hasL=False, hasR=False), dict(verdict=ML, hasL=True, hasR=False)), True)
    # u just below w - 15 is in; at w - 15 the left is out and the right, still inside, matches
    edge(0, w - 15.0, rows[1] + 0.0, ("uw_lo", "uw_at"), (dict(verdict=ML, hasL=True, hasR=True), dict(verdict=MR, hasL=False, hasR=True)), True)
    edge(1, 15.0, w * 0.5, ("v_lo", "v_at"), (dict(verdict="outL", hasL=False, hasR=False), dict(verdict=ML, hasL=True, hasR=True)), True)
    edge(1, h - 15.0, w * 0.5 + 90, ("vh_lo", "vh_at"), (dict(verdict=ML, hasL=True, hasR=True), dict(verdict="outL", hasL=False, hasR=False)), True)
    # the right pixel at its own left border: uR < 15 out, uR == 15 in (u = 15 + disparity is inside)
    for which, name, ex in ((0, "ur_lo", dict(verdict="no_key", hasL=True, hasR=False)), (1, "ur_at", dict(verdict=MR, hasL=True, hasR=True))):
        X0 = X_at(15.0 + b.disp, rows[2] + 40.0 * which)
        fr = lambda x: predict(g, [x, X0[1], X0[2]], F32(1), T1)["uv"][2] >= 15.0
        x = straddle(fr, X0[0] - 0.02, X0[0] + 0.02)[which]
        p = b.probe(name, [x, X0[1], X0[2]], expect=ex)
        b.rkey(p, 0.0, 0.0, p.ps, 2)
    # behind the target keyframe, and exactly in its plane (z == 0 is "behind": the test is z <= 0)
    u, v = b.spot()
    X = b.world(1, u, v)
    for name, z in (("behind", float(T1[2, 3]) - 1.0), ("z0", float(T1[2, 3]))):
        b.probe(name, [X[0], X[1], z], expect=dict(verdict="behind"))
    return b.finish()


def case_pred_scale(g):
    """Only q == 0 can be hit exactly (dif == 1.0f, whose logarithm is exactly 0).  Whether log(dif) / logScale is exactly 3
    for some float32 dif is a property of the libm at hand, so around 3 there are the two neighbouring doubles of the
    world point on either side of the flip, and no "at" probe."""
    b = Builder(g, "pred_scale")
    rig = g.rig
    T0, T1 = b.kf[0]["T_wc"], b.kf[1]["T_wc"]
    t1 = T1[:3, 3]
    rows = [v for v in range(50, rig["h"] - 45, 64) if abs(v - rig["cy"]) > 45]
    ucol = rig["cx"] - 14.0                           # the column of the points equidistant from keyframes 0 and 1
    b.spots = [s for s in b.spots if abs(s[0] - ucol) > 45 and abs(s[1] - rig["cy"]) > 45]
    b.fillers()

    def ps_of(X, o0):
        return predict(g, X, _dist32(X, T0) * g.sp[o0], T1)

    def ladder(p, admitted_octs, out_octs):
        # inadmissible octaves carry the probe's own descriptor, the admissible ones 5, 20, 35 bits: the first admissible wins,
        # clear of the ratio test
        keys = {}
        for j, o in enumerate(admitted_octs):
            keys[o] = b.lkey(p, -1.5 + j, 1.0, o, 5 + 15 * j)
        for j, o in enumerate(out_octs):
            b.lkey(p, 1.0 - 2 * j, -1.5, o, 0)
        return keys
    # the point equidistant from both keyframes: dif == sp[o0] up to the last bit.  Moving it along x crosses that value.
    def equidistant(row, o0, want):
        """world points near the equidistant plane at depth Z whose predScale is want[0] and want[1], as close to each other as doubles get"""
        y = (rows[row] - rig["cy"]) * b.Z / rig["fy"]
        x0 = (t1[0] * t1[0] + t1[1] * t1[1] - 2 * y * t1[1]) / (2 * t1[0])
        f = lambda x: ps_of([x, y, b.Z], o0)["predScale"] >= want[1]
        sgn = 1.0 if f(x0 + 0.05) else -1.0
        lo, hi = straddle(f, x0 - sgn * 0.05, x0 + sgn * 0.05)
        return [lo, y, b.Z], [hi, y, b.Z]
    # q == 0 exactly (dif == 1: the logarithm is exactly 0) -> predScale 0; one step further q > 0 -> predScale 1
    Xa, Xb = equidistant(0, 0, (0, 1))
    p = b.probe("q0_at", Xa, expect=dict(verdict="matched-left", predScale=0, q_le=0.0)); k = ladder(p, (0, 1), (2,)); b.expect(p, best=k[0])
    Xa, Xb = equidistant(1, 0, (0, 1))
    p = b.probe("q0_hi", Xb, expect=dict(verdict="matched-left", predScale=1, q_gt=0.0)); k = ladder(p, (2, 1, 0), (3,)); b.expect(p, best=k[2])
    # q just below / above 3 (dif next to scalePyramid[3])
    Xa, Xb = equidistant(2, 3, (3, 4))
    p = b.probe("q3_lo", Xa, o0=3, expect=dict(verdict="matched-left", predScale=3, q_le=3.0)); k = ladder(p, (2, 3, 4), (1, 5)); b.expect(p, best=k[2])
    Xa, Xb = equidistant(3, 3, (3, 4))
    p = b.probe("q3_hi", Xb, o0=3, expect=dict(verdict="matched-left", predScale=4, q_gt=3.0)); k = ladder(p, (5, 4, 3), (2, 6)); b.expect(p, best=k[5])
    # q <= -1 (clamps to 0) and q >= nLev (clamps to nLev - 1)
    n1 = math.sqrt(t1[0] ** 2 + t1[1] ** 2)
    p = b.probe("q_neg", [0.0, 0.0, 1.45 * n1], o0=0, expect=dict(verdict="matched-left", predScale=0, q_le=-1.0)); k = ladder(p, (0, 1), (2,)); b.expect(p, best=k[0])
    p = b.probe("q_big", [t1[0], t1[1], 0.5 * n1], o0=7, expect=dict(verdict="matched-left", predScale=g.nLev - 1, q_gt=float(g.nLev)))
    k = ladder(p, (7, 6), (5,)); b.expect(p, best=k[7])
    return b.finish()


def _search32(start, ok):
    """the float32 nearest to start for which ok() holds, walking both ways"""
    a = b_ = F32(start)
    for _ in range(4096):
        if ok(a):
            return a
        if ok(b_):
            return b_
        a, b_ = np.nextafter(a, F32(-np.inf)), np.nextafter(b_, F32(np.inf))
    raise AssertionError("no float32 found")


def case_radius_strict(g):
    b = Builder(g, "radius_strict"); b.fillers()
    rig = g.rig
    for name, ax, sg in (("dx_pos", 0, 1), ("dx_neg", 0, -1), ("dy_pos", 1, 1), ("dy_neg", 1, -1)):
        p = b.at(name, expect=dict(verdict="matched-left"))
        r, c = F32(p.rad), p.pL[ax]
        inside = _search32(float(c) + sg * (p.rad - 1e-3), lambda x: abs(F32(x) - c) < r and not abs(np.nextafter(F32(x), F32(sg * np.inf)) - c) < r)
        at = np.nextafter(inside, F32(sg * np.inf))
        assert not abs(at - c) < r
        xy = lambda val: (float(val) - float(p.pL[0]), 0.0) if ax == 0 else (0.0, float(val) - float(p.pL[1]))
        kin = b.lkey(p, *xy(inside), p.ps, 10)
        b.lkey(p, *xy(at), p.ps, 0)                       # at the radius: out, although its descriptor is the better one
        b.expect(p, best=kin)
    p = b.at("one_axis_out", expect=dict(verdict="radius"))
    b.lkey(p, 1.0, p.rad + 0.5, p.ps, 0)
    b.lkey(p, -(p.rad + 0.5), 1.0, p.ps, 0)
    # keys whose rounded grid cell lies beyond the last row / column and is clamped onto it (needs the largest radius)
    for name, u, v, dx, dy in (("clamp_row", rig["w"] * 0.5, rig["h"] - 16.0, 0.0, 13.0), ("clamp_col", rig["w"] - 16.0, rig["h"] * 0.5 + 20, 13.0, 0.0)):
        p = b.probe(name, b.world(1, u, v), o0=7, expect=dict(verdict="matched-left", clamped=True))
        assert p.ps == 7
        kk = b.lkey(p, dx, dy, 7, 6)
        b.expect(p, best=kk)
    return b.finish()


def case_unmatched_filter(g):
    b = Builder(g, "unmatched_filter"); b.fillers()
    p = b.at("left_next", expect=dict(verdict="matched-left"))
    b.lkey(p, 1.0, 0.0, p.ps, 5, unF=7); k = b.lkey(p, -1.0, 1.0, p.ps, 20); b.expect(p, best=k)
    p = b.at("left_none", expect=dict(verdict="unF"))
    b.lkey(p, 1.0, 0.0, p.ps, 5, unF=0)
    p = b.at("right_next", expect=dict(verdict="matched-right"))
    b.rkey(p, 1.0, 0.0, p.ps, 5, unF=3); k = b.rkey(p, -1.0, 1.0, p.ps, 20); b.expect(p, best=k)
    p = b.at("right_none", expect=dict(verdict="unF"))
    b.rkey(p, 1.0, 0.0, p.ps, 5, unF=12)
    return b.finish()


def _passes(b, portrait):
    """name prefixes of the passes that build a case's probes.  Landscape: one pass.  Portrait (480 x 752, 101 grid rows):
    "" on spots at y >= 500 (grid rows >= 67, cell indices beyond 4095), then "lo_": the same probes again at y < 440."""
    if not portrait:
        yield ""
        return
    cols = sorted({sp[0] for sp in b.spots})
    low = [sp for sp in b.spots[b.nspot:] if sp[1] < 440]
    b.spots, b.nspot = [(u, float(v)) for v in range(500, 715, 38) for u in cols], 0
    yield ""
    b.spots, b.nspot = low, 0
    yield "lo_"


_ORDER = {"col": ((-2.0, 1.0), (2.0, 1.0)), "row": ((1.0, -2.0), (1.0, 2.0)), "rowcol": ((2.0, -2.0), (-2.0, 2.0)), "idx": ((1.0, 1.0), (1.5, 1.5))}


def _two(b, p, side, order, first, second):
    """two keys of one side, `first` = (bits, octave) of the one visited first; -> (index of first, index of second)"""
    mk = b.rkey if side == "R" else b.lkey
    (x0, y0), (x1, y1) = _ORDER[order]
    i0 = mk(p, x0, y0, first[1], first[0])
    i1 = mk(p, x1, y1, second[1], second[0], start=64)
    return i0, i1


def case_second_level_rule(g, portrait=False):
    """best B = (27 bits, level 0), second S = (44 bits, level 1): 0.6f * 44 <= 27, so the pair is rejected exactly when
    the recorded second level equals the best level.  Left scan, S visited after B: the (sic) rule records B's level ->
    rejected; every other combination records S's own level -> accepted.  (27, 44) also sits next to the ratio boundary:
    read as (27, 45) it passes, 27 < 0.6f * 45.)"""
    b = Builder(g, "second_level_rule"); b.fillers()
    B, S = (27, 0), (44, 1)
    for pre in _passes(b, portrait):
        for side in "LR":
            M = "matched-right" if side == "R" else "matched-left"
            for order in ("col", "row", "rowcol", "idx"):
                p = b.at("%s%s_%s_after" % (pre, side, order), corner=True, expect=dict(verdict="ratio" if side == "L" else M, sec_level=0 if side == "L" else 1))
                assert p.ps in (0, 1)
                i0, i1 = _two(b, p, side, order, B, S); b.expect(p, best=i0, side=side)
                p = b.at("%s%s_%s_before" % (pre, side, order), corner=True, expect=dict(verdict=M, sec_level=1))
                i0, i1 = _two(b, p, side, order, S, B); b.expect(p, best=i1, side=side)
            # two keys at the best distance: the first visited is the best, the other the second at the same distance
            p = b.at("%s%s_tie_best" % (pre, side), corner=True, expect=dict(verdict="ratio" if side == "L" else M, sec_level=0 if side == "L" else 1))
            i0, i1 = _two(b, p, side, "col", (27, 0), (27, 1)); b.expect(p, best=i0, side=side, sec_dist=27)
            # two keys at the second distance, one before and one after the best: the earlier one's level is recorded
            mk = b.rkey if side == "R" else b.lkey
            p = b.at("%s%s_tie_second_own" % (pre, side), corner=True, expect=dict(verdict=M, sec_level=1, sec_dist=44))
            mk(p, -2.0, 1.0, 1, 44); kb = mk(p, 1.0, 1.0, 0, 27, start=64); mk(p, 2.5, 1.0, 0, 44, start=128); b.expect(p, best=kb, side=side)
            p = b.at("%s%s_tie_second_same" % (pre, side), corner=True, expect=dict(verdict="ratio", sec_level=0, sec_dist=44))
            mk(p, -2.0, 1.0, 0, 44); kb = mk(p, 1.0, 1.0, 0, 27, start=64); mk(p, 2.5, 1.0, 1, 44, start=128); b.expect(p, best=kb, side=side)
        if portrait and pre == "":
            # the best in grid row 63, the second (an odd distance) in row 64: visited after the best.  With a 12-bit cell
            # field row 64 wraps to row 0 and is visited first.
            u, _ = b.spot(corner=True)
            p = b.probe("L_straddle_63_64", b.world(1, u, 63.5 / float(g.yMult)), expect=dict(verdict="ratio", sec_level=0, sec_dist=43, side="L"))
            k = b.lkey(p, 1.0, -2.0, 0, 27); b.lkey(p, 1.0, 2.0, 1, 43, start=64); b.expect(p, best=k)
    return b.finish()


def case_left_right_choice(g, portrait=False):
    b = Builder(g, "left_right_choice"); b.fillers()
    for pre in _passes(b, portrait):
        # equal best distances: the left stays, with its own second (after the best: the best's level) -> ratio; the right alone would match
        p = b.at(pre + "equal", corner=True, expect=dict(verdict="ratio", side="L"))
        _two(b, p, "L", "col", (20, 0), (30, 1)); b.rkey(p, 0.0, 0.0, 0, 20)
        # right smaller by one: the right's second and levels replace the left's -> matched (the left's would reject)
        p = b.at(pre + "right_by_one", corner=True, expect=dict(verdict="matched-right", side="R"))
        _two(b, p, "L", "col", (20, 0), (30, 1)); i0, i1 = _two(b, p, "R", "col", (19, 0), (25, 1)); b.expect(p, best=i0)
        # the same with an even right distance (20 against 21: read as 21 against 21 the left would stay and be rejected)
        p = b.at(pre + "right_by_one_even", corner=True, expect=dict(verdict="matched-right", side="R"))
        _two(b, p, "L", "col", (21, 0), (31, 1)); i0, i1 = _two(b, p, "R", "col", (20, 0), (26, 1)); b.expect(p, best=i0)
        p = b.at(pre + "left_by_one", corner=True, expect=dict(verdict="matched-left", side="L"))
        k = b.lkey(p, 0.0, 0.0, 0, 18); b.rkey(p, 0.0, 0.0, 0, 19); b.expect(p, best=k)
        p = b.at(pre + "only_left", expect=dict(verdict="matched-left", side="L")); k = b.lkey(p, 1.0, 1.0, p.ps, 8); b.expect(p, best=k)
        p = b.at(pre + "only_right", expect=dict(verdict="matched-right", side="R")); k = b.rkey(p, 1.0, 1.0, p.ps, 8); b.expect(p, best=k)
    return b.finish()


RATIO_PAIRS = ((30, 50), (29, 50), (31, 50), (3, 5), (4, 5), (18, 30), (19, 30), (6, 10), (7, 10), (5, 10))


def case_thresholds(g, portrait=False):
    b = Builder(g, "thresholds"); b.fillers()
    for pre in _passes(b, portrait):
        p = b.at(pre + "d50", expect=dict(verdict="matched-left")); k = b.lkey(p, 0.5, 0.5, p.ps, 50); b.expect(p, best=k)
        p = b.at(pre + "d51", expect=dict(verdict="dist>50")); b.lkey(p, 0.5, 0.5, p.ps, 51)
        p = b.at(pre + "d50_right", expect=dict(verdict="matched-right")); k = b.rkey(p, 0.5, 0.5, p.ps, 50); b.expect(p, best=k)
        for bd, sd in RATIO_PAIRS:
            # equal levels, the second after the best; float32 as the reference: (float)best >= 0.6f * (float)sec rejects
            rej = bool(F32(bd) >= F32(0.6) * F32(sd))
            p = b.at("%sratio_%d_%d" % (pre, bd, sd), expect=dict(verdict="ratio" if rej else "matched-left", sec_dist=sd))
            k = b.lkey(p, -1.0, 0.5, p.ps, bd); b.lkey(p, 1.0, 0.5, p.ps, sd, start=64); b.expect(p, best=k)
        p = b.at(pre + "no_second", expect=dict(verdict="matched-left", sec_dist=None)); k = b.lkey(p, 0.5, 0.5, p.ps, 40); b.expect(p, best=k)
        # a key 256 bits away never becomes the best (the scan starts at 256 and is strict) nor the second
        p = b.at(pre + "d256_only", expect=dict(verdict="dist>50")); b.lkey(p, 0.5, 0.5, p.ps, 256)
        p = b.at(pre + "d256_second", expect=dict(verdict="matched-left", sec_dist=None)); k = b.lkey(p, -1.0, 0.5, p.ps, 45); b.lkey(p, 1.0, 0.5, p.ps, 256); b.expect(p, best=k)
    return b.finish()


def case_parallax(g):
    b = Builder(g, "parallax"); b.fillers()

    def last_x(c, want):
        """float32 x of the last keyframe's key so that pred - x is just below / exactly / just above 10"""
        c = F32(c)
        at = _search32(float(c) - 10.0, lambda x: float(c) - float(F32(x)) == 10.0)
        return {"below": np.nextafter(at, F32(np.inf)), "at": at, "above": np.nextafter(at, F32(-np.inf))}[want]
    for want, verdict in (("below", "parallax"), ("at", "parallax"), ("above", "matched-left")):
        p = b.at("left_" + want, expect=dict(verdict=verdict))
        b.lkey(p, 0.5, 0.5, p.ps, 6)
        p.e["x"], p.e["y"] = last_x(p.pL[0], want), p.pL[1]
    # a right match: against the candidate's right key if it has one ...
    for want, verdict in (("below", "parallax"), ("at", "parallax"), ("above", "matched-right")):
        p = b.at("right_has_" + want, expect=dict(verdict=verdict))
        b.rkey(p, 0.5, 0.5, p.ps, 6)
        far = want != "above"                             # the left key says the opposite
        p.e["x"], p.e["y"] = (F32(float(p.pR[0]) + 30.0) if far else F32(float(p.pR[0]) + 2.0)), p.pR[1]
        b.lastR.append(dict(x=last_x(p.pR[0], want), y=p.pR[1], o=0, d=b.desc(), unF=-1, partner=p.e))
        p.e["partner"] = len(b.lastR) - 1
    # ... else against its left key
    for want, verdict in (("below", "parallax"), ("above", "matched-right")):
        p = b.at("right_none_" + want, expect=dict(verdict=verdict))
        b.rkey(p, 0.5, 0.5, p.ps, 6)
        p.e["x"], p.e["y"] = last_x(p.pR[0], want), p.pR[1]
    return b.finish()


def case_output_mapping(g):
    b = Builder(g, "output_mapping"); b.fillers()
    p = b.at("right_with_left", expect=dict(verdict="matched-right"))
    r = b.rkey(p, 0.5, 0.5, p.ps, 6); l = b.lkey(p, 20.0, 0.0, p.ps, 0); b.link(1, l, r); b.expect(p, out=(l, r))
    p = b.at("right_without_left", expect=dict(verdict="matched-right")); r = b.rkey(p, 0.5, 0.5, p.ps, 6); b.expect(p, out=(-1, r))
    p = b.at("left_without_right", expect=dict(verdict="matched-left")); l = b.lkey(p, 0.5, 0.5, p.ps, 6); b.expect(p, out=(l, -1))
    p = b.at("left_with_right", expect=dict(verdict="matched-left"))
    l = b.lkey(p, 0.5, 0.5, p.ps, 6); r = b.rkey(p, 20.0, 0.0, p.ps, 0); b.link(1, l, r); b.expect(p, out=(l, r))
    return b.finish()


MATCH_CASES = dict(gate_edges=case_gate_edges, pred_scale=case_pred_scale, radius_strict=case_radius_strict,
                   unmatched_filter=case_unmatched_filter, second_level_rule=case_second_level_rule,
                   left_right_choice=case_left_right_choice, thresholds=case_thresholds, parallax=case_parallax,
                   output_mapping=case_output_mapping)
PORTRAIT_CASES = dict(thresholds=case_thresholds, second_level_rule=case_second_level_rule, left_right_choice=case_left_right_choice)


# ---------------------------------------------------------------------------------------------------------------------
# windows: skipped keyframe, tiny windows
def _spread(n_last, n):
    """n ascending key indices over 0 .. n_last - 1, the first and the last among them"""
    return sorted({int(x) for x in np.linspace(0, n_last - 1, n)})


def case_skip_mid(g, n_last=None):
    """a keyframe with the last keyframe's id in the middle of the window: never searched, although it holds every key"""
    b = Builder(g, "skip_mid" + ("_%d" % n_last if n_last else ""), shifts=((28, 2), (-25, 4), (-36, 3), (32, -6)), yaws=(0.0, 0.0, 0.01, -0.008), ids=(101, 100, 103, 104))
    b.fillers(kfs=[1, 2, 3, 4])
    for i in range(10):
        b.finals["fill%d" % i] = dict(accepted=1, nObs=4, kfs=[0, 1, 3, 4])
    return b.finish(n_last=n_last, keep_pos=_spread(n_last, 10)) if n_last else b.finish()


def case_single_kf(g):
    b = Builder(g, "single_kf", shifts=()); b.kf.append(dict(T_wc=_pose([0.2, 0, 0]), id=101, L=[], R=[]))
    b.spots = [(float(u), float(v)) for v in range(50, g.rig["h"] - 45, 64) for u in range(150, g.rig["w"] - 60, 72)]
    b.fillers(kfs=[1])
    del b.kf[1]
    b.finals = {}
    return b.finish()


def case_no_candidates(g):
    b = Builder(g, "no_candidates")
    b.fillers(4)
    b.finals, b.probes = {}, {}
    for e in b.last:
        if e["hasMp"]:
            e["unF"] = 5
        else:
            e["depth"] = F32(0.0)
    return b.finish()


def case_empty_last(g):
    b = Builder(g, "empty_last")
    b.fillers(3)
    b.finals, b.last, b.lastR, b.probes = {}, [], [], {}
    return b.finish()


# ---------------------------------------------------------------------------------------------------------------------
# triangulation and filter regimes
def _ring(n):
    """pixel shifts of n keyframes: alternating sides, 16 px and more (the parallax gate wants 10)"""
    return tuple(((18 + 3 * i) * (1 if i % 2 == 0 else -1), (i % 3) - 1) for i in range(n))


def case_obs_counts(g):
    b = Builder(g, "obs_counts", shifts=_ring(3), yaws=(0.0, 0.004, -0.003)); b.fillers(6)
    for i in range(4):
        u, v = b.spot()
        b.track("two_%d" % i, b.world(1, u, v), {1 + i % 3: "LR" if i % 2 else "L"}, last_sides="LR" if i < 2 else "L")
        b.finals["two_%d" % i] = dict(accepted=0, nObs=2, raw=True)
    for i in range(4):
        u, v = b.spot()
        ks = [k for k in (1, 2, 3) if k != 1 + i % 3]
        b.track("three_%d" % i, b.world(1, u, v), {k: ("LR" if i % 2 else "L") for k in ks}, last_sides="LR" if i < 2 else "L")
        b.finals["three_%d" % i] = dict(accepted=1, nObs=3)
    return b.finish()


def case_row_counts(g, n_last=None):
    """neighbouring candidates of one 64-thread group with 6, 8, 10 ... 64 DLT rows (64 = NP_MAX_ROWS: all 16 keyframes, both sides)"""
    b = Builder(g, "row_counts" + ("_%d" % n_last if n_last else ""), shifts=_ring(15), yaws=(0.0,) * 15)
    for j in range(30):
        S = 3 + j                                     # observation sides = rows / 2
        n_e = max(3, (S + 1) // 2)
        n_r = S - n_e
        u, v = b.spot()
        sides = {k: ("LR" if k < n_r else "L") for k in range(1, n_e)}
        b.track("rows_%d" % (2 * S), b.world(1, u, v), sides, last_sides="LR" if n_r > 0 else "L")
        b.finals["rows_%d" % (2 * S)] = dict(accepted=1, nObs=n_e, rows=2 * S)
    b.fillers(6)
    return b.finish(n_last=n_last, keep_pos=_spread(n_last, 36)) if n_last else b.finish()


def case_group_and_chunk_edges(g, n_last, n_cand):
    b = Builder(g, "chunk_%d_%d" % (n_last, n_cand), shifts=((28, 2), (-22, 3)), yaws=(0.0, 0.006))
    b.fillers(10)
    for i in range(n_cand - 10):                      # candidates of both kinds that match nothing
        X = b.world(1, 40.0 + 5 * i, 30.0, 30.0 + i)
        b.last_key(100.0 + i, 20.0, i % 4, b.desc(), hasMp=i % 2, X=X, depth=0.0 if i % 2 else 25.0 + i, owner="idle%d" % i)
    rng = np.random.default_rng(n_last)
    fixed = sorted({0, 1022, 1023, 1024, n_last - 1} & set(range(n_last)))
    rest = [int(x) for x in rng.choice([i for i in range(n_last) if i not in fixed], n_cand - len(fixed), replace=False)]
    return b.finish(n_last=n_last, keep_pos=sorted(fixed + rest))


def case_rank_deficient(g):
    """left-only keys at ONE pixel in keyframes that share the last keyframe's pose: every DLT row pair is the same, rank 2"""
    b = Builder(g, "rank_deficient", shifts=((0, 0), (0, 0), (0, 0), (30, 2), (-24, 3)), yaws=(0.0, 0.0, 0.0, 0.0, 0.005))
    b.fillers(6, kfs=[4, 5])
    for i, n in enumerate((3, 2)):                    # 4 and 3 observations
        u, v = b.spot()
        u, v = float(int(u)), float(int(v))
        p = b.probe("rank_%d" % (n + 1), b.world(1, u + 8.0, v + 8.0), o0=7)
        p.e["x"], p.e["y"] = F32(u), F32(v)
        assert p.ps == 7
        for k in range(1, n + 1):
            b.key(k, 0, u, v, 7 - (k % 2), flip(p.d, 4 + k), owner=p.name)
        b.finals[p.name] = dict(accepted=0, nObs=n + 1, raw=True, rank_deficient=True)
        b.probes[p.name]["expect"] = {}
        b.probes[p.name]["kf"] = None
    return b.finish()


def case_cheirality(g):
    """left-only rays from keyframes 2 and 4 mm to the right of the last one whose keys move RIGHT: they meet behind the cameras"""
    mm = 0.002 * g.rig["fx"] / Builder.Z
    b = Builder(g, "cheirality", shifts=((mm, 0), (2 * mm, 0), (30, 2), (-24, 3)), yaws=(0.0, 0.0, 0.0, 0.005))
    b.fillers(6, kfs=[3, 4])
    for i in range(2):
        u, v = b.spot()
        p = b.probe("behind_%d" % i, b.world(1, u + 8.0, v + 8.0), o0=7)
        p.e["x"], p.e["y"] = F32(u), F32(v)
        assert p.ps == 7
        for k in (1, 2):
            b.key(k, 0, u + (3.0 + i) * k, v, 7, flip(p.d, 4 + k), owner=p.name)
        b.finals[p.name] = dict(accepted=0, nObs=3, raw=True, behind=True)
        b.probes[p.name]["expect"] = {}
        b.probes[p.name]["kf"] = None
    return b.finish()


def case_reproj_filter(g):
    """level-0 keys 3.8 px off fail err > 7.815 * sigma[0] (2.8 px); level-2 keys survive the same offset (4.0 px)"""
    # the last keyframe 12 cm further back than the others and the probes near the centre column, where a sideways step
    # changes the distance least: 1 < dif < 1.2, predScale 1 in every keyframe, levels 0 .. 2 admissible (asserted below)
    b = Builder(g, "reproj_filter", shifts=_ring(5), yaws=(0.0, 0.0, 0.003, -0.003, 0.0), last_z=-0.12)
    central = [s for s in b.spots if abs(s[0] - g.rig["cx"]) < 150][:6]
    rest = sorted((s for s in b.spots if s not in central), key=lambda s: abs(s[0] - g.rig["cx"]))      # (the fillers: next to them)
    b.spots = central + rest
    all5 = {k: "LR" for k in range(1, 6)}
    OFF = (0.0, 3.8)

    # left fails, right passes: the entry stays with l = -1
    u, v = b.spot(); e, idx = b.track("left_fails", b.world(1, u, v), all5, offs={(2, "L"): OFF})
    b.finals["left_fails"] = dict(accepted=1, nObs=6, edit={2: ("L", -1)})
    # right fails without an earlier drop: the entry stays with r = -1
    u, v = b.spot(); e, idx = b.track("right_fails", b.world(1, u, v), all5, offs={(3, "R"): OFF})
    b.finals["right_fails"] = dict(accepted=1, nObs=6, edit={3: ("R", -1)})
    # the same offset on level-2 keys survives
    u, v = b.spot(); e, idx = b.track("high_level", b.world(1, u, v), all5, offs={(2, "L"): OFF, (2, "R"): OFF}, octs={(2, "L"): 2, (2, "R"): 2})
    b.finals["high_level"] = dict(accepted=1, nObs=6, edit={})
    # keyframe 1 (left only) dropped, then keyframe 3: left passes, right fails -> the compacted copy keeps the stale right index
    u, v = b.spot(); s = dict(all5); s[1] = "L"
    e, idx = b.track("stale_right", b.world(1, u, v), s, offs={(1, "L"): OFF, (3, "R"): OFF})
    b.finals["stale_right"] = dict(accepted=1, nObs=5, drop=[1], edit={})
    # the last keyframe's own entry fails: correctKF stays false
    u, v = b.spot(); e, idx = b.track("last_fails", b.world(1, u, v), all5, last_sides="L", last_off=OFF)
    b.finals["last_fails"] = dict(accepted=0, nObs=5, drop=[0], edit={})
    # three observations, one dropped: 2 < minCount
    u, v = b.spot(); e, idx = b.track("three_to_two", b.world(1, u, v), {1: "LR", 2: "L"}, offs={(2, "L"): OFF})
    b.finals["three_to_two"] = dict(accepted=0, nObs=2, drop=[2], edit={})
    b.fillers(6)
    c = b.finish()
    for name in ("left_fails", "right_fails", "high_level", "stale_right", "last_fails", "three_to_two"):
        assert all(pr["predScale"] == 1 for pr in c.pairs[c.probes[name]["cand"]].values()), name
    return c


TRI_CASES = dict(obs_counts=case_obs_counts, row_counts=case_row_counts, rank_deficient=case_rank_deficient, cheirality=case_cheirality,
                 reproj_filter=case_reproj_filter, skip_mid=case_skip_mid,
                 skip_mid_70=lambda g: case_skip_mid(g, 70), row_counts_1025=lambda g: case_row_counts(g, 1025),      # lanes of the batch test
                 chunk_1023_63=lambda g: case_group_and_chunk_edges(g, 1023, 63), chunk_1024_64=lambda g: case_group_and_chunk_edges(g, 1024, 64),
                 chunk_1025_65=lambda g: case_group_and_chunk_edges(g, 1025, 65))
TINY_CASES = dict(single_kf=case_single_kf, no_candidates=case_no_candidates, empty_last=case_empty_last)
ALL_CASES = dict(MATCH_CASES, **TRI_CASES, **TINY_CASES)

_CASES = {}


def geo_for(oracle, rig_name):
    import synth
    rig = dict(synth.RIGS["euroc"], **PORTRAIT) if rig_name == "portrait" else synth.RIGS[rig_name]
    ex = oracle.Extractor(500)
    return Geo(rig, ex.scalePyramid, ex.sigmaFactor), ex


def get(oracle, name, rig_name):
    """the case, built once per process; c.ex = an oracle extractor for the pyramid tables"""
    key = (name, rig_name)
    if key not in _CASES:
        g, ex = geo_for(oracle, rig_name)
        if rig_name == "portrait":
            c = PORTRAIT_CASES[name](g, portrait=True)
        else:
            c = ALL_CASES[name](g)
        c.ex, c.rig_name = ex, rig_name
        _CASES[key] = c
    return _CASES[key]


def expected_final(c, name):
    """obs rows after the reprojection filter as the case's construction predicts them (finals without `raw`)"""
    f, p = c.finals[name], c.probes[name]
    raw = c.raw[p["cand"]]
    if f.get("raw"):
        return [list(r) for r in raw]
    rows = []
    for (k, l, r) in raw:
        if k in f.get("drop", ()):
            continue
        if k in f.get("edit", {}):
            side, val = f["edit"][k]
            l, r = (val, r) if side == "L" else (l, val)
        rows.append([k, l, r])
    return rows
