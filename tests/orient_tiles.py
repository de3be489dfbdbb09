"""Crafted 48 x 48 patches for tests/test_gpu_orient_desc.py and tests/test_orient_flip_cases.py (no test in here).

A tile is a four-fold symmetric random texture, T(u, v) = T(-u, v) = T(u, -v) around its centre pixel (24, 24), values 40..200:
it adds nothing to the two moments of the radius-15 disc of the intensity centroid (m10 = sum u I, m01 = sum v I).  set_moments
then changes a few pixels so that the moments are EXACTLY the requested integers; the disc (+-15) and the descriptor's taps
(+-19, blurred: +-22) stay inside the tile, so tiles on one image do not see each other."""
import json
import os
import numpy as np

TILE = 48
C = 24            # centre pixel of a tile
HERE = os.path.dirname(os.path.abspath(__file__))
FLIP_CASES = os.path.join(HERE, "golden", "orient_flip_cases.json")


def sym_texture(rng):
    q = rng.integers(40, 201, size=(C + 1, C + 1))
    idx = np.abs(np.arange(TILE) - C)
    return q[np.ix_(idx, idx)].astype(np.int64)          # [v + C, u + C]


def _slots(umax, swap):
    """pixel groups that add to ONE moment only, heaviest first: (weight, [(u, v), ...] all of the same |u|, |v|); swap: for m01"""
    out = []
    for a in range(1, 16):                 # the coordinate that carries the moment
        for b in range(0, a):              # the other one, mirrored: its contributions cancel
            u, v = (b, a) if swap else (a, b)
            if abs(u) > umax[abs(v)]:
                continue
            out.append((a * (1 if b == 0 else 2), a, b))
    out.sort(key=lambda s: -s[0])
    return out


def _fill(tile, target, umax, swap):
    """add `target` to m10 (swap: m01) with pixels of |u| > |v| (swap: |v| > |u|), mirrored pairs so the other moment stays"""
    rem, sgn = abs(int(target)), (1 if target >= 0 else -1)
    for w, a, b in _slots(umax, swap):
        for side in (1, -1):               # pixels on the target's side go up, the ones opposite go down
            if rem < w:
                break
            pix = [(side * sgn * a, bb) for bb in ({b, -b})]
            if swap:
                pix = [(bb, aa) for aa, bb in pix]
            val = int(tile[pix[0][1] + C, pix[0][0] + C])
            d = min((255 - val) if side == 1 else val, rem // w)
            for u, v in pix:
                tile[v + C, u + C] += side * d
            rem -= d * w
    return rem


def capacity(tile, umax, swap, sign):
    t = tile.copy()
    return 10 ** 9 - _fill(t, sign * 10 ** 9, umax, swap)


def set_moments(tile, m10, m01, umax):
    """tile: a sym_texture (changed in place).  Raises if the pair is beyond what the tile's pixels can carry."""
    if _fill(tile, m10, umax, False) or _fill(tile, m01, umax, True):
        raise ValueError("moments (%d, %d) beyond the tile's capacity" % (m10, m01))
    assert tile.min() >= 0 and tile.max() <= 255
    return tile


def moments(tile, umax):
    """(m10, m01) of the disc, from the definition"""
    m10 = m01 = 0
    for v in range(-15, 16):
        for u in range(-umax[abs(v)], umax[abs(v)] + 1):
            m10 += u * int(tile[v + C, u + C])
            m01 += v * int(tile[v + C, u + C])
    return m10, m01


def mosaic(tiles, cols):
    """tiles -> (image u8, centres [(x, y)]) with `cols` tiles per row"""
    rows = (len(tiles) + cols - 1) // cols
    # (at least 288 px each way: the smallest pyramid level must still hold one FAST cell)
    img = np.full((max(rows * TILE, 288), max(cols * TILE, 288)), 120, np.int64)
    centres = []
    for i, t in enumerate(tiles):
        r, c = divmod(i, cols)
        img[r * TILE:(r + 1) * TILE, c * TILE:(c + 1) * TILE] = t
        centres.append((c * TILE + C, r * TILE + C))
    assert img.min() >= 0 and img.max() <= 255
    return img.astype(np.uint8), centres


def load_flip_cases():
    with open(FLIP_CASES) as f:
        return json.load(f)["cases"]


def flip_image(seed, umax):
    """one tile per recorded flip case, with exactly its moments"""
    rng = np.random.default_rng(seed)
    cases = load_flip_cases()
    tiles = [set_moments(sym_texture(rng), c["m10"], c["m01"], umax) for c in cases]
    img, centres = mosaic(tiles, 13)
    return cases, img, centres


def oracle_keys(oracle, oe, level_img, level, pts, response=50, trig="double"):
    """what the extractor must return for keypoints `pts` (level coordinates) of pyramid level `level`: orientation on the
    unblurred level, descriptor on its blurred copy, then the scaling of extractKeysNew"""
    blurred = oracle.blur(level_img)
    kps = np.zeros(len(pts), oracle.KP_DTYPE)
    desc = np.zeros((len(pts), 32), np.uint8)
    sc = oe.scalePyramid[level]
    for i, (x, y) in enumerate(pts):
        kp = np.zeros(1, oracle.KP_DTYPE)
        kp["x"], kp["y"], kp["size"], kp["response"] = x, y, oe.scaledPatchSize[level], response
        kp["octave"], kp["class_id"] = level, -1
        kp["angle"] = np.float32(oe.orientation(level_img, x, y))
        desc[i] = oracle.orb_descriptor(kp, blurred, trig=trig)
        if level != 0:
            kp["x"] = np.float32(x) * sc
            kp["y"] = np.float32(y) * sc
        kps[i] = kp[0]
    return kps, desc


def query(capi, pts, response=50):
    q = np.zeros(len(pts), capi.KP_DTYPE)
    for i, (x, y) in enumerate(pts):
        q[i]["x"], q[i]["y"], q[i]["response"] = x, y, response
    return q


def assert_same(got, want, what=""):
    gk, gd = got
    wk, wd = want
    assert len(gk) == len(wk), what
    for f in wk.dtype.names:
        a, b = gk[f], wk[f]
        if a.dtype.kind == "f":            # bit-exact, not merely ==
            a, b = a.view(np.uint32), b.view(np.uint32)
        bad = np.nonzero(a != b)[0]
        assert len(bad) == 0, "%s: field %s differs at keypoints %s" % (what, f, bad[:8].tolist())
    bad = np.nonzero((gd != wd).any(axis=1))[0]
    assert len(bad) == 0, "%s: descriptors differ at keypoints %s" % (what, bad[:8].tolist())
