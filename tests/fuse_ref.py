"""numpy restatement of the duplicate search and of the commit of vslam_system_fuse_loop (include/vslam_hip.h, DESIGN.md section 6
item 26).  No library import: the rules are written once more, in the operation order the header states, so that the device's
bytes can be compared with them.

  project(T_cw, K, size, xyz)            -> records (n, 4) float32: (u, v, z, 0), (NaN, NaN, -1, 0) for a point outside the image
  search(T_cw, K, size, A, descA, B, descB, radius, depth_ratio, max_hamming)
                                         -> match (nA) int32, best (nA, 4) int32, counts dict
  commit(pairs, obs, kf_tables, kdx, outlier, in_frame, active, last_obs_kf)
                                         -> the same containers after the merge (new objects), and the counts
"""
import numpy as np

DEFAULTS = dict(radius=4.0, depth_ratio=1.25, max_hamming=50)
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def project(T_cw, K, size, xyz):
    """rule 1: fp64 in the written order, then float32"""
    T = np.asarray(T_cw, np.float64).reshape(4, 4)
    X = np.asarray(xyz, np.float64).reshape(-1, 3)
    fx, fy, cx, cy = (np.float64(v) for v in K)
    w, h = size
    Xc = [(T[i, 0] * X[:, 0] + T[i, 1] * X[:, 1]) + T[i, 2] * X[:, 2] + T[i, 3] for i in range(3)]
    x, y, z = Xc
    rec = np.zeros((len(X), 4), np.float32)
    rec[:, :2] = np.nan                    # an invisible record: (NaN, NaN, -1) - it passes no gate at any depth_ratio
    rec[:, 2] = -1.0
    front = z > 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        invZ = 1.0 / z
        u = fx * x * invZ + cx
        v = fy * y * invZ + cy
    vis = front & ~((u < 0) | (v < 0) | (u >= w) | (v >= h))
    rec[vis, 0] = u[vis].astype(np.float32)
    rec[vis, 1] = v[vis].astype(np.float32)
    rec[vis, 2] = z[vis].astype(np.float32)
    return rec


def hamming(d, D):
    """256-bit distance of one descriptor (32) to each row of D (n, 32)"""
    return _POP[np.bitwise_xor(D, d[None, :])].sum(axis=1).astype(np.int32)


def gate(ra, RB, radius, depth_ratio):
    """rule 2 for one A record against every B record: float32 throughout, one rounding per operation"""
    r = np.float32(radius); q = np.float32(depth_ratio)
    with np.errstate(over="ignore", invalid="ignore"):
        du = ra[0] - RB[:, 0]; dv = ra[1] - RB[:, 1]
        d2 = du * du + dv * dv
        return (d2 <= r * r) & (RB[:, 2] <= q * ra[2]) & (ra[2] <= q * RB[:, 2])


def search_records(RA, descA, RB, descB, radius=0, depth_ratio=0, max_hamming=0):
    """rules 2 - 5 on records"""
    radius = radius or DEFAULTS["radius"]; depth_ratio = depth_ratio or DEFAULTS["depth_ratio"]; max_hamming = max_hamming or DEFAULTS["max_hamming"]
    descA = np.asarray(descA, np.uint8).reshape(-1, 32); descB = np.asarray(descB, np.uint8).reshape(-1, 32)
    nA, nB = len(RA), len(RB)
    best = np.tile(np.array([257, -1, 257, 0], np.int32), (nA, 1))
    winner = {}
    for a in range(nA):
        if nB == 0:
            break
        g = np.nonzero(gate(RA[a], RB, radius, depth_ratio))[0]
        if len(g) == 0:
            continue
        d = hamming(descA[a], descB[g])
        k = int(np.argmin(d))                      # the first minimum: the lowest index attaining d1
        d1, b1 = int(d[k]), int(g[k])
        rest = np.delete(d, k)
        best[a] = (d1, b1, int(rest.min()) if len(rest) else 257, len(g))
        if d1 <= max_hamming:
            key = (d1 << 32) | a
            if b1 not in winner or key < winner[b1]:
                winner[b1] = key
    match = np.full(nA, -1, np.int32)
    n_prop = 0
    for a in range(nA):
        d1, b1, _, ng = best[a]
        if ng > 0 and d1 <= max_hamming:
            n_prop += 1
            if (winner[int(b1)] & 0xFFFFFFFF) == a:
                match[a] = b1
    counts = dict(n_visible_a=int((RA[:, 2] > 0).sum()), n_visible_b=int((RB[:, 2] > 0).sum()), n_proposals=n_prop,
                  n_pairs=int((match >= 0).sum()))
    return match, best, counts


def search(T_cw, K, size, xyzA, descA, xyzB, descB, radius=0, depth_ratio=0, max_hamming=0):
    RA = project(T_cw, K, size, xyzA)
    RB = project(T_cw, K, size, xyzB)
    return search_records(RA, descA, RB, descB, radius, depth_ratio, max_hamming)


def commit(pairs, obs, kf_tables, kdx, outlier, in_frame, active, last_obs_kf):
    """The merge on plain Python containers.
    pairs: [(a, b)] ascending a; obs: per map point a list of (kf, l, r); kf_tables: per keyframe a dict of the lists lmpL, lmpR,
    unF, unFR; kdx / outlier / in_frame / last_obs_kf: per map point; active: the list of active map points.
    Returns (obs, kf_tables, outlier, in_frame, active, last_obs_kf, counts), all new objects."""
    obs = [list(map(tuple, o)) for o in obs]
    kf_tables = [{k: list(v) for k, v in t.items()} for t in kf_tables]
    outlier = list(outlier); in_frame = list(in_frame); active = list(active); last_obs_kf = list(last_obs_kf)
    moved = dropped = 0
    touched = set()
    for a, b in pairs:
        for (kf, l, r) in obs[a]:
            t = kf_tables[kf]
            if all(o[0] != kf for o in obs[b]):
                obs[b].append((kf, l, r))
                if l >= 0:
                    t["lmpL"][l] = b; t["unF"][l] = int(kdx[b])
                if r >= 0:
                    t["lmpR"][r] = b; t["unFR"][r] = int(kdx[b])
                moved += 1
            else:
                if l >= 0:
                    t["lmpL"][l] = -1; t["unF"][l] = -1
                if r >= 0:
                    t["lmpR"][r] = -1; t["unFR"][r] = -1
                dropped += 1
            touched.add(kf)
        obs[a] = []
        outlier[a] = 1; in_frame[a] = 0
        last_obs_kf[b] = max(last_obs_kf[b], last_obs_kf[a])
    if pairs:
        absorbed = {a for a, _ in pairs}
        active = [m for m in active if m not in absorbed]
        have = set(active)
        for b in sorted(b for _, b in pairs):
            in_frame[b] = 1
            if b not in have:
                active.append(b)
    # covisibility is recomputed for the touched keyframes and for every keyframe that observes a kept point
    refresh = sorted(touched | {kf for _, b in pairs for (kf, l, r) in obs[b]})
    counts = dict(n_fused=len(pairs), n_obs_moved=moved, n_obs_dropped=dropped, touched=sorted(touched), refresh=refresh,
                  n_active_after=len(active))
    return obs, kf_tables, outlier, in_frame, active, last_obs_kf, counts


def connections(kf, kf_tables, obs, n_keyframes):
    """KeyFrame::calcConnections restated: weights over the observations of the keyframe's map points (left table: every observation;
    right table: observations without a left index), entries with weight >= 15 sorted by (weight, keyframe) descending"""
    w = [0] * n_keyframes
    for m in kf_tables[kf]["lmpL"]:
        if m >= 0:
            for (k, l, r) in obs[m]:
                w[k] += 1
    for m in kf_tables[kf]["lmpR"]:
        if m >= 0:
            for (k, l, r) in obs[m]:
                if l < 0 and r >= 0:
                    w[k] += 1
    return sorted(((w[k], k) for k in range(n_keyframes) if w[k] >= 15), reverse=True)
