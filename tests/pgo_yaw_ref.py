"""CPU restatement of the yaw-only (4-DoF) pose-graph optimisation (DESIGN.md section 6 item 29;
vslam_pose_graph_optimize_yaw): the residual, the 6-DoF Jacobians, the cost and the graph builders are pgo_ref's; a free pose
has the parameters (theta, delta) with the retraction T <- [Exp(theta g) R, t + delta] about the unit axis g, its Jacobian is
J6 M with M = [[R^T g, 0], [0, R^T]], and the schedule is the one of pgo_ref.optimize with a DENSE solve.

Also the projection that the loop calls of an IMU session apply to a claimed pose: the rotation about g closest to a rotation
(twist), in closed form."""
import numpy as np
import pgo_ref as pr


def unit_axis(axis):
    """g = axis / sqrt(x^2 + y^2 + z^2), the library's expression"""
    x, y, z = (float(v) for v in axis)
    n = np.sqrt(x * x + y * y + z * z)
    return np.array([x / n, y / n, z / n])


def retract(T, d, g):
    """[Exp(theta g) R, t + delta] with d = (theta, delta)"""
    return pr.make_pose(pr.so3_exp(d[0] * g) @ T[:3, :3], T[:3, 3] + d[1:])


def chain_factor(T, g):
    """M (6, 4): the 6-DoF local parameters (a, b) of pgo_ref.retract per unit of (theta, delta)"""
    R = T[:3, :3]
    M = np.zeros((6, 4))
    M[:3, 0] = R.T @ g
    M[3:, 1:] = R.T
    return M


def jacobians(Ti, Tj, Z, g):
    r, Ji, Jj = pr.jacobians(Ti, Tj, Z)
    return r, Ji @ chain_factor(Ti, g), Jj @ chain_factor(Tj, g)


def linearize(poses, fixed, edges, g):
    """(H, grad, free): H = J4^T W J4 and grad = J4^T W r over the free poses, 4 columns each"""
    n = len(poses)
    free, _ = pr.free_poses(n, fixed, edges)
    col = {k: 4 * c for c, k in enumerate(free)}
    H = np.zeros((4 * len(free), 4 * len(free)))
    grad = np.zeros(4 * len(free))
    for e in edges:
        r, Ji, Jj = jacobians(poses[e[0]], poses[e[1]], np.asarray(e[2]), g)
        w = pr.edge_weights(e)
        blocks = [(col[k], J) for k, J in ((e[0], Ji), (e[1], Jj)) if k in col]
        for ca, Ja in blocks:
            grad[ca:ca + 4] += Ja.T @ (w * r)
            for cb, Jb in blocks:
                H[ca:ca + 4, cb:cb + 4] += Ja.T @ (w[:, None] * Jb)
    return H, grad, free


def gradient_inf(poses, fixed, edges, axis):
    """|J4^T W r|_inf over the free poses"""
    _, grad, free = linearize(poses, fixed, edges, unit_axis(axis))
    return float(np.abs(grad).max()) if len(free) else 0.0


def optimize(poses, fixed, edges, axis, max_iterations=0, lambda0=0.0):
    """the schedule of pgo_ref.optimize over (theta, delta): (new poses, report dict)"""
    g = unit_axis(axis)
    poses = [np.array(T, np.float64) for T in poses]
    n = len(poses)
    max_it = max_iterations or pr.DEFAULTS["max_iterations"]
    lam = lambda0 or pr.DEFAULTS["lambda0"]
    free, iso = pr.free_poses(n, fixed, edges)
    c0 = pr.cost(poses, edges)
    rep = dict(iterations=0, accepted=0, rejected=0, n_free=len(free), n_isolated=iso, initial_cost=c0, final_cost=c0, final_lambda=lam)
    if not (c0 > 1e-20) or not free:
        return np.array(poses), rep
    cur = c0
    acc = rej = 0
    stop = False
    while not stop:
        H, grad, _ = linearize(poses, fixed, edges, g)
        dH = np.diag(H).copy()
        while True:
            try:
                delta = np.linalg.solve(H + lam * np.diag(dH), -grad)
                ok = bool(np.all(np.isfinite(delta)))
            except np.linalg.LinAlgError:
                delta, ok = np.zeros_like(grad), False
            trial = list(poses)
            for c, k in enumerate(free):
                trial[k] = retract(poses[k], delta[4 * c:4 * c + 4], g)
            cn = pr.cost(trial, edges)
            tiny = ok and float(np.abs(delta).max()) < 1e-12
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


# ---- the projection of a claimed pose -----------------------------------------------------------------------------------------
def twist(R, g):
    """the angle of the rotation about the unit axis g closest to R (it maximises tr(Exp(theta g)^T R)):
    atan2(g . q, tr R - g^T R g) with q = (R32 - R23, R13 - R31, R21 - R12)"""
    q = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return float(np.arctan2(g @ q, np.trace(R) - g @ R @ g))


def project_claim(T_corr, T_cam, axis):
    """(T', theta, tilt dropped): T' = [Exp(theta g) R_cam | t_corr] with theta the twist of D = T_corr T_cam^-1"""
    g = unit_axis(axis)
    RD = T_corr[:3, :3] @ T_cam[:3, :3].T
    th = twist(RD, g)
    Tp = pr.make_pose(pr.so3_exp(th * g) @ T_cam[:3, :3], T_corr[:3, 3])
    w = pr.so3_log(Tp[:3, :3].T @ T_corr[:3, :3])
    return Tp, th, float(np.linalg.norm(w))
