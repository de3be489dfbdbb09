"""CPU restatement of the pose-graph optimisation (vslam_pose_graph_optimize): the same residual,
retraction, analytic Jacobians and Levenberg-Marquardt schedule in numpy, with a DENSE solve of the damped normal equations.
The device solves the same system by a block-banded Cholesky after a reordering; neither changes the solution.

Poses are 4x4 world <- camera matrices; an edge is (i, j, Z, w_rot, w_trans) with Z measuring T_i^-1 T_j.  Graph builders for
the tests are at the end of the file."""
import numpy as np

DEFAULTS = dict(max_iterations=20, lambda0=1e-4)


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def so3_exp(w):
    """Rodrigues; first order when |w|^2 <= eps (the rule of the library's so3_expmap)"""
    w = np.asarray(w, np.float64)
    th2 = float(w @ w)
    W = skew(w)
    if th2 <= np.finfo(np.float64).eps:
        return np.eye(3) + W
    th = np.sqrt(th2)
    K = W / th
    s2 = np.sin(th / 2.0)
    return np.eye(3) + np.sin(th) * K + 2.0 * s2 * s2 * (K @ K)


def so3_log(R):
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    tr_3 = tr - 3.0
    if tr_3 < -1e-6:
        c = min(1.0, max(-1.0, (tr - 1.0) / 2.0))
        th = np.arccos(c)
        mag = th / (2.0 * np.sin(th))
    else:
        mag = 0.5 - tr_3 / 12.0 + tr_3 * tr_3 / 60.0
    return mag * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])


def make_pose(R, t):
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = t
    return T


def rigid_inv(T):
    R = T[:3, :3]
    return make_pose(R.T, -R.T @ T[:3, 3])


def retract(T, d):
    """T [Exp(a), b; 0, 1] with d = (a, b)"""
    R = T[:3, :3]
    return make_pose(R @ so3_exp(d[:3]), T[:3, 3] + R @ d[3:])


def edge_error(Ti, Tj, Z):
    """(R_D, t_D, R_E, t_E): D = T_i^-1 T_j, E = Z^-1 D, rigid inverses"""
    Ri, Rj, Rz = Ti[:3, :3], Tj[:3, :3], Z[:3, :3]
    RD = Ri.T @ Rj
    tD = Ri.T @ (Tj[:3, 3] - Ti[:3, 3])
    RE = Rz.T @ RD
    tE = Rz.T @ (tD - Z[:3, 3])
    return RD, tD, RE, tE


def residual(Ti, Tj, Z):
    _, _, RE, tE = edge_error(Ti, Tj, Z)
    return np.concatenate([so3_log(RE), tE])


def jacobians(Ti, Tj, Z):
    """(r, J_i, J_j): rows = residual components, columns = the pose's (a, b)"""
    RD, tD, RE, tE = edge_error(Ti, Tj, Z)
    w = so3_log(RE)
    th2 = float(w @ w)
    if th2 < 1e-10:
        c = 1.0 / 12.0
    else:
        th = np.sqrt(th2)
        c = 1.0 / th2 - (1.0 + np.cos(th)) / (2.0 * th * np.sin(th))
    W = skew(w)
    Jri = np.eye(3) + 0.5 * W + c * (W @ W)          # inverse right Jacobian of SO(3)
    RzT = Z[:3, :3].T
    Ji = np.zeros((6, 6))
    Jj = np.zeros((6, 6))
    Ji[:3, :3] = -Jri @ RD.T
    Ji[3:, :3] = RzT @ skew(tD)
    Ji[3:, 3:] = -RzT
    Jj[:3, :3] = Jri
    Jj[3:, 3:] = RE
    return np.concatenate([w, tE]), Ji, Jj


def edge_weights(e):
    return np.array([e[3]] * 3 + [e[4]] * 3, np.float64)


def cost(poses, edges):
    s = 0.0
    for e in edges:
        r = residual(poses[e[0]], poses[e[1]], np.asarray(e[2]))
        s += e[3] * float(r[:3] @ r[:3]) + e[4] * float(r[3:] @ r[3:])
    return s


def free_poses(n, fixed, edges):
    """indices of the free poses (not fixed, at least one edge) and the number of isolated ones"""
    deg = np.zeros(n, int)
    for e in edges:
        deg[e[0]] += 1
        deg[e[1]] += 1
    free = [k for k in range(n) if not fixed[k] and deg[k] > 0]
    iso = sum(1 for k in range(n) if not fixed[k] and deg[k] == 0)
    return free, iso


def linearize(poses, fixed, edges):
    """(H, g, free): H = J^T W J and g = J^T W r over the free poses, 6 columns each"""
    n = len(poses)
    free, _ = free_poses(n, fixed, edges)
    col = {k: 6 * c for c, k in enumerate(free)}
    H = np.zeros((6 * len(free), 6 * len(free)))
    g = np.zeros(6 * len(free))
    for e in edges:
        r, Ji, Jj = jacobians(poses[e[0]], poses[e[1]], np.asarray(e[2]))
        w = edge_weights(e)
        blocks = [(col[k], J) for k, J in ((e[0], Ji), (e[1], Jj)) if k in col]
        for ca, Ja in blocks:
            g[ca:ca + 6] += Ja.T @ (w * r)
            for cb, Jb in blocks:
                H[ca:ca + 6, cb:cb + 6] += Ja.T @ (w[:, None] * Jb)
    return H, g, free


def gradient_inf(poses, fixed, edges):
    """|J^T W r|_inf over the free poses: the stationarity measure (it does not depend on the solver)"""
    _, g, free = linearize(poses, fixed, edges)
    return float(np.abs(g).max()) if len(free) else 0.0


def has_free_gauge(n, fixed, edges):
    free, _ = free_poses(n, fixed, edges)
    idx = {k: c for c, k in enumerate(free)}
    parent = list(range(len(free)))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    anchored = [False] * len(free)
    for e in edges:
        a, b = idx.get(e[0]), idx.get(e[1])
        if a is not None and b is not None:
            parent[find(a)] = find(b)
    for e in edges:
        a, b = idx.get(e[0]), idx.get(e[1])
        if (a is None) != (b is None):
            anchored[find(a if a is not None else b)] = True
    return any(not anchored[find(c)] for c in range(len(free)))


def optimize(poses, fixed, edges, max_iterations=0, lambda0=0.0):
    """the schedule of vslam_pose_graph_optimize: (new poses, report dict)"""
    poses = [np.array(T, np.float64) for T in poses]
    n = len(poses)
    max_it = max_iterations or DEFAULTS["max_iterations"]
    lam = lambda0 or DEFAULTS["lambda0"]
    free, iso = free_poses(n, fixed, edges)
    c0 = cost(poses, edges)
    rep = dict(iterations=0, accepted=0, rejected=0, n_free=len(free), n_isolated=iso, initial_cost=c0, final_cost=c0, final_lambda=lam)
    if not (c0 > 1e-20) or not free:
        return np.array(poses), rep
    cur = c0
    acc = rej = 0
    stop = False
    while not stop:
        H, g, _ = linearize(poses, fixed, edges)
        dH = np.diag(H).copy()
        while True:
            try:
                delta = np.linalg.solve(H + lam * np.diag(dH), -g)
                ok = bool(np.all(np.isfinite(delta)))
            except np.linalg.LinAlgError:
                delta, ok = np.zeros_like(g), False
            trial = list(poses)
            for c, k in enumerate(free):
                trial[k] = retract(poses[k], delta[6 * c:6 * c + 6])
            cn = cost(trial, edges)
            tiny = ok and float(np.abs(delta).max()) < 1e-12      # (a failed solve's delta means nothing: the trial is only rejected)
            if ok and np.isfinite(cn) and cn < cur:
                rel = (cur - cn) / cur
                poses, cur = trial, cn
                acc += 1
                lam = max(lam / 3.0, 1e-12)
                if acc >= max_it or rel < 1e-10 or tiny:
                    stop = True
                break
            rej += 1
            lam *= 4.0
            if lam > 1e8 or tiny:
                stop = True
                break
    rep.update(iterations=acc + rej, accepted=acc, rejected=rej, final_cost=cur, final_lambda=lam)
    return np.array(poses), rep


def move_points(points, ref, T_old, T_new):
    out = np.array(points, np.float64).reshape(-1, 3).copy()
    for k in range(len(out)):
        r = int(ref[k])
        if r < 0:
            continue
        A, B = T_old[r], T_new[r]
        out[k] = B[:3, :3] @ (A[:3, :3].T @ (out[k] - A[:3, 3])) + B[:3, 3]
    return out


# ---- graphs of the tests ----------------------------------------------------------------------------------------------------
def random_pose(rng, rot, trans):
    return make_pose(so3_exp(rng.uniform(-1, 1, 3) * rot), rng.uniform(-1, 1, 3) * trans)


def circle_poses(n, radius=3.0):
    """n poses on a circle in the x-z plane, looking along the tangent"""
    out = []
    for k in range(n):
        a = 2.0 * np.pi * k / max(n, 1)
        out.append(make_pose(so3_exp(np.array([0.0, -a, 0.0])), np.array([radius * np.cos(a), 0.1 * np.sin(3 * a), radius * np.sin(a)])))
    return out


def noisy_edge(rng, truth, i, j, rot, trans, w_rot=1.0, w_trans=1.0):
    Z = rigid_inv(truth[i]) @ truth[j] @ random_pose(rng, rot, trans)
    return (i, j, Z, w_rot, w_trans)


def ring_graph(n, seed, rot=0.01, trans=0.02):
    """n poses on a circle: edges (k, k + 1), (k, k + 2) and the closing edge (n - 1, 0) - 2 n - 2 edges with measurement noise
    up to rot rad / trans m per edge; the start is the chain of the (k, k + 1) measurements (it has drifted); pose 0 is fixed"""
    rng = np.random.default_rng(seed)
    truth = circle_poses(n)
    edges = [noisy_edge(rng, truth, k, k + 1, rot, trans) for k in range(n - 1)]
    edges += [noisy_edge(rng, truth, k, k + 2, rot, trans) for k in range(n - 2)]
    edges.append(noisy_edge(rng, truth, n - 1, 0, rot, trans))
    poses = [truth[0]]
    for k in range(n - 1):
        poses.append(poses[-1] @ edges[k][2])
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    return np.array(poses), fixed, edges


def exact_graph(n=16, seed=3):
    """measurements computed from the poses themselves: the initial cost is rounding error"""
    rng = np.random.default_rng(seed)
    poses = [random_pose(rng, 1.0, 3.0) for _ in range(n)]
    edges = [(k, k + 1, rigid_inv(poses[k]) @ poses[k + 1], 1.0, 1.0) for k in range(n - 1)]
    edges.append((n - 1, 0, rigid_inv(poses[n - 1]) @ poses[0], 1.0, 1.0))
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    return np.array(poses), fixed, edges


def complete_graph(n=12, seed=5):
    """every pair of n poses with relative rotations up to 3.1 rad; the start is the truth disturbed by 0.1 rad / 0.1 m"""
    rng = np.random.default_rng(seed)
    truth = [make_pose(so3_exp(np.array([0.0, 3.1 * k / (n - 1), 0.0])), rng.uniform(-2, 2, 3)) for k in range(n)]
    edges = [noisy_edge(rng, truth, i, j, 0.005, 0.01) for i in range(n) for j in range(i + 1, n)]
    poses = [truth[0]] + [truth[k] @ random_pose(rng, 0.1, 0.1) for k in range(1, n)]
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    return np.array(poses), fixed, edges


def chain_graph(n, chord, seed=7, fixed_ids=(0,)):
    """an open chain of n poses with one extra edge `chord` = (a, b)"""
    rng = np.random.default_rng(seed)
    truth = [make_pose(so3_exp(np.array([0.0, 0.02 * k, 0.0])), np.array([0.1 * k, 0.0, 0.02 * k])) for k in range(n)]
    edges = [noisy_edge(rng, truth, k, k + 1, 0.002, 0.005) for k in range(n - 1)]
    edges.append(noisy_edge(rng, truth, chord[0], chord[1], 0.002, 0.005))
    poses = [truth[0]]
    for k in range(n - 1):
        poses.append(poses[-1] @ edges[k][2])
    fixed = np.zeros(n, np.uint8)
    fixed[list(fixed_ids)] = 1
    return np.array(poses), fixed, edges


def star_graph(n, seed=11, hub_fixed=True):
    """pose 0 tied to every other pose by TWO edges with independent noise (2 n - 2 edges; a single edge per pose could be met
    exactly: a final cost of rounding error); with the hub fixed no two free poses share an edge"""
    rng = np.random.default_rng(seed)
    truth = [random_pose(rng, 1.0, 3.0) for _ in range(n)]
    edges = [noisy_edge(rng, truth, 0, k, 0.01, 0.02) for k in range(1, n)]
    edges += [noisy_edge(rng, truth, 0, k, 0.01, 0.02) for k in range(1, n)]
    poses = [truth[0]] + [truth[k] @ random_pose(rng, 0.05, 0.1) for k in range(1, n)]
    fixed = np.zeros(n, np.uint8)
    fixed[0 if hub_fixed else 1] = 1
    return np.array(poses), fixed, edges
