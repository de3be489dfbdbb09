"""CPU restatement of the global bundle adjustment (vslam_global_ba) in numpy, with a DENSE solve
of the damped reduced camera system.  The device solves the same system by a block-banded Cholesky after a reordering; neither
changes the solution.  This file is the authority on the rules:

factors      every set bit of pair_flags (bit 0 left, bit 1 right: the camera displaced by the baseline along x) is one two-row
             factor r = (projection - measurement) / sigma, sigma = 1 / inv_sigma_factor[octave]; q = R^T (X - t),
             u = fx x / z + cx, v = fy y / z + cy.  kf_id is not used.  Edges (i, j, Z, w_rot, w_trans) are pgo_ref's.
unknowns     poses by pgo_ref.retract (T [Exp(a), b]), landmarks additive
cost         sum r^2 over the factors on present landmarks + pgo_ref.cost(edges); no 1/2
presence     a landmark is present iff it has >= 2 factors; a keyframe is free iff it is not fixed and has a factor on a present
             landmark or an edge; everything else comes back bit for bit
gauge        a component of free keyframes (connected by shared present landmarks or edges) that shares no present landmark
             and no edge with a fixed keyframe is refused; so is a present factor with z <= 0 at the initial values
LM           pgo_ref.optimize's schedule; damping lambda diag(H) on the pose and the landmark diagonal before the elimination;
             a trial is rejected on a pivot that is not positive (a landmark's damped block or the reduced system), on a
             non-finite cost and on a factor with z <= 0
flags        chi2 of the local BA at the final values over pairs of kf_local keyframes on present landmarks

A problem is the dict vslam_capi.global_ba takes: rig (fx, fy, cx, cy, bl), kf_pose (K, 4, 4), kf_fixed, kf_local, lm (L, 3),
pair_kf, pair_lm, pair_flags, pair_uv (P, 4) float32, pair_oct (P, 2).  Problem builders for the tests are at the end."""
import numpy as np
import pgo_ref as pr

DEFAULTS = dict(max_iterations=20, lambda0=1e-4)
RIG = dict(w=640, h=480, fx=400.0, fy=410.0, cx=320.0, cy=240.0, bl=0.12, fps=20.0)
SCALE = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
SIGMA = (SCALE * SCALE).astype(np.float32)                 # sigma_factor
INV_SIGMA = (np.float32(1.0) / SIGMA).astype(np.float32)   # inv_sigma_factor


def camera(rig):
    return float(rig["fx"]), float(rig["fy"]), float(rig["cx"]), float(rig["cy"]), float(np.float32(rig["bl"]))     # (the ABI's baseline is a float)


class Structure:
    """presence, the free set and the factor arrays of a problem"""

    def __init__(self, prob, edges, inv_sigma):
        K, L = len(prob["kf_pose"]), len(prob["lm"])
        pk = np.asarray(prob["pair_kf"], np.int64); pl = np.asarray(prob["pair_lm"], np.int64)
        fl = np.asarray(prob["pair_flags"], np.int64) & 3
        nfac = (fl & 1) + (fl >> 1)
        fac = np.bincount(pl, weights=nfac, minlength=L).astype(np.int64) if len(pl) else np.zeros(L, np.int64)
        self.present = fac >= 2
        self.on_pair = (nfac > 0) & self.present[pl] if len(pl) else np.zeros(0, bool)
        fixed = np.asarray(prob["kf_fixed"]).astype(bool)
        tied = np.zeros(K, bool)
        tied[pk[self.on_pair]] = True
        for e in edges:
            tied[e[0]] = tied[e[1]] = True
        self.free = [k for k in range(K) if not fixed[k] and tied[k]]
        self.n_isolated = int(np.sum(~fixed & ~tied))
        self.col = -np.ones(K, np.int64)
        self.col[self.free] = np.arange(len(self.free))
        self.lms = np.flatnonzero(self.present)
        self.lcol = -np.ones(L, np.int64)
        self.lcol[self.lms] = np.arange(len(self.lms))
        uv = np.asarray(prob["pair_uv"], np.float32).reshape(-1, 4).astype(np.float64)
        octv = np.asarray(prob["pair_oct"], np.int64).reshape(-1, 2)
        isd = 1.0 / (1.0 / np.asarray(inv_sigma, np.float32).astype(np.float64))
        parts = []
        for side in (0, 1):
            sel = np.flatnonzero(self.on_pair & (((fl >> side) & 1) > 0))
            parts.append((sel, pk[sel], pl[sel], np.full(len(sel), side), uv[sel, 2 * side:2 * side + 2], isd[octv[sel, side]]))
        self.f_pair, self.f_kf, self.f_lm, self.f_side, self.f_z, self.f_is = (np.concatenate([p[i] for p in parts]) for i in range(6))
        self.n_factors = len(self.f_pair)
        self.n_thin = int(L - self.present.sum())
        self.fixed, self.pk, self.pl, self.K, self.L = fixed, pk, pl, K, L


def project(S, cam, poses, lm, jac):
    """(r (n, 2), z (n), Jp (n, 2, 6), Jl (n, 2, 3)) of every factor"""
    fx, fy, cx, cy, bl = cam
    R = poses[S.f_kf, :3, :3]
    q = np.einsum("nji,nj->ni", R, lm[S.f_lm] - poses[S.f_kf, :3, 3])
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    with np.errstate(all="ignore"):
        iz = 1.0 / z
        xx = x - bl * S.f_side
        r = np.stack([(fx * xx * iz + cx - S.f_z[:, 0]) * S.f_is, (fy * y * iz + cy - S.f_z[:, 1]) * S.f_is], 1)
        if not jac:
            return r, z, None, None
        n = len(z)
        al = np.zeros((n, 2, 3))
        al[:, 0, 0] = fx * iz; al[:, 0, 2] = -fx * xx * iz * iz
        al[:, 1, 1] = fy * iz; al[:, 1, 2] = -fy * y * iz * iz
        Sk = np.zeros((n, 3, 3))
        Sk[:, 0, 1] = -z; Sk[:, 0, 2] = y; Sk[:, 1, 0] = z; Sk[:, 1, 2] = -x; Sk[:, 2, 0] = -y; Sk[:, 2, 1] = x
        Jp = np.concatenate([al @ Sk, -al], 2) * S.f_is[:, None, None]
        Jl = (al @ np.transpose(R, (0, 2, 1))) * S.f_is[:, None, None]
    return r, z, Jp, Jl


def cost(S, cam, poses, lm, edges):
    """(cost, every factor in front of its camera)"""
    r, z, _, _ = project(S, cam, poses, lm, False)
    return float(np.sum(r * r)) + pr.cost(poses, edges), bool(np.all(z > 0))


def has_free_gauge(S, edges):
    nf = len(S.free)
    parent = list(range(nf))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    anchored = np.zeros(nf, bool)
    groups = [(S.col[S.pk[S.on_pair & (S.pl == l)]], S.fixed[S.pk[S.on_pair & (S.pl == l)]].any()) for l in S.lms] if nf else []
    ties = [(g[g >= 0], anc) for g, anc in groups]
    for e in edges:
        a, b = S.col[e[0]], S.col[e[1]]
        ties.append((np.array([c for c in (a, b) if c >= 0], np.int64), bool((a < 0 and S.fixed[e[0]]) or (b < 0 and S.fixed[e[1]]))))
    for g, _ in ties:
        for c in g[1:]:
            parent[find(int(g[0]))] = find(int(c))
    for g, anc in ties:
        if anc and len(g):
            anchored[find(int(g[0]))] = True
    return any(not anchored[find(c)] for c in range(nf))


def linearize(S, cam, poses, lm, edges):
    """(Hpp, gp, Hll (n, 3, 3), gl (n, 3), Hpl (6 nf, n, 3)): the undamped blocks over the free keyframes and present landmarks"""
    nf, nl = len(S.free), len(S.lms)
    r, _, Jp, Jl = project(S, cam, poses, lm, True)
    Hpp = np.zeros((nf, nf, 6, 6)); gp = np.zeros((nf, 6)); Hll = np.zeros((nl, 3, 3)); gl = np.zeros((nl, 3)); Hpl = np.zeros((nf, nl, 6, 3))
    lc = S.lcol[S.f_lm]
    np.add.at(Hll, lc, np.einsum("nai,naj->nij", Jl, Jl))
    np.add.at(gl, lc, np.einsum("nai,na->ni", Jl, r))
    fr = np.flatnonzero(S.col[S.f_kf] >= 0)
    kc = S.col[S.f_kf[fr]]
    np.add.at(Hpp, (kc, kc), np.einsum("nai,naj->nij", Jp[fr], Jp[fr]))
    np.add.at(gp, kc, np.einsum("nai,na->ni", Jp[fr], r[fr]))
    np.add.at(Hpl, (kc, lc[fr]), np.einsum("nai,naj->nij", Jp[fr], Jl[fr]))
    for e in edges:
        re, Ji, Jj = pr.jacobians(poses[e[0]], poses[e[1]], np.asarray(e[2]))
        w = pr.edge_weights(e)
        blocks = [(S.col[k], J) for k, J in ((e[0], Ji), (e[1], Jj)) if S.col[k] >= 0]
        for ca, Ja in blocks:
            gp[ca] += Ja.T @ (w * re)
            for cb, Jb in blocks:
                Hpp[ca, cb] += Ja.T @ (w[:, None] * Jb)
    Hpp = Hpp.transpose(0, 2, 1, 3).reshape(6 * nf, 6 * nf)
    Hpl = Hpl.transpose(0, 2, 1, 3).reshape(6 * nf, nl, 3)
    return Hpp, gp.reshape(-1), Hll, gl, Hpl


def solve(lin, lam):
    """(pose step, landmark steps, ok) of the damped system: landmarks eliminated, the reduced system solved densely"""
    Hpp, gp, Hll, gl, Hpl = lin
    nf6, nl = len(gp), len(gl)
    Hd = Hll.copy()
    idx = np.arange(3)
    Hd[:, idx, idx] *= 1.0 + lam
    try:
        if nl:
            np.linalg.cholesky(Hd)
        Hinv = np.linalg.inv(Hd) if nl else Hd
        Y = np.einsum("pnk,nkj->pnj", Hpl, Hinv)
        Sred = Hpp + lam * np.diag(np.diag(Hpp)) - Y.reshape(nf6, 3 * nl) @ Hpl.reshape(nf6, 3 * nl).T
        rhs = -(gp - np.einsum("pnj,nj->p", Y, gl))
        if nf6:
            np.linalg.cholesky(Sred)
        dp = np.linalg.solve(Sred, rhs) if nf6 else rhs
        dl = np.einsum("nij,nj->ni", Hinv, -gl - np.einsum("pnj,p->nj", Hpl, dp))
        ok = bool(np.all(np.isfinite(dp)) and np.all(np.isfinite(dl)))
    except np.linalg.LinAlgError:
        dp, dl, ok = np.zeros(nf6), np.zeros((nl, 3)), False
    return dp, dl, ok


def chi2(prob, S, cam, sigma, poses, lm):
    """(flags, smallest relative distance of a statistic from its threshold) over the pairs of kf_local keyframes on present landmarks"""
    fx, fy, cx, cy, bl = cam
    P = len(S.pk)
    wrong = np.zeros(P, np.uint8)
    margin = np.inf
    local = np.asarray(prob["kf_local"]).astype(bool)
    fl = np.asarray(prob["pair_flags"], np.int64) & 3
    uv = np.asarray(prob["pair_uv"], np.float32).reshape(-1, 4).astype(np.float64)
    octv = np.asarray(prob["pair_oct"], np.int64).reshape(-1, 2)
    sig = np.asarray(sigma, np.float32)
    for p in np.flatnonzero(S.on_pair & local[S.pk]):
        T = poses[S.pk[p]]
        q = T[:3, :3].T @ (lm[S.pl[p]] - T[:3, 3])
        out = []
        for side in (0, 1):
            if not (fl[p] >> side) & 1:
                out.append(False)
                continue
            x = q[0] - bl * side
            thr = float(np.float32(float(np.float32(7.815)) * float(sig[octv[p, side]])))
            if not q[2] > 0:
                out.append(True)
                continue
            eu = uv[p, 2 * side] - (fx * x + cx * q[2]) / q[2]
            ev = uv[p, 2 * side + 1] - (fy * q[1] + cy * q[2]) / q[2]
            stat = eu * eu + ev * ev
            margin = min(margin, abs(stat - thr) / thr)
            out.append(stat > thr)
        wrong[p] = out[0] or out[1]
    return wrong, margin


def optimize(prob, edges=(), sigma=SIGMA, inv_sigma=INV_SIGMA, max_iterations=0, lambda0=0.0):
    """the schedule of vslam_global_ba: dict(kf_pose, lm, pair_wrong, report, margin)"""
    edges = list(edges)
    S = Structure(prob, edges, inv_sigma)
    cam = camera(prob["rig"])
    poses = np.array(prob["kf_pose"], np.float64).reshape(-1, 4, 4)
    lm = np.array(prob["lm"], np.float64).reshape(-1, 3)
    poses0, lm0 = poses.copy(), lm.copy()
    if has_free_gauge(S, edges):
        raise ValueError("free gauge")
    _, z, _, _ = project(S, cam, poses, lm, False)
    if not np.all(z > 0):
        raise ValueError("pair %d is not in front of its camera" % int(S.f_pair[np.flatnonzero(~(z > 0))].min()))
    max_it = max_iterations or DEFAULTS["max_iterations"]
    lam = lambda0 or DEFAULTS["lambda0"]
    c0, _ = cost(S, cam, poses, lm, edges)
    acc = rej = 0
    cur = c0
    stop = not (c0 > 1e-20) or not (len(S.free) or len(S.lms))
    while not stop:
        lin = linearize(S, cam, poses, lm, edges)
        while True:
            dp, dl, ok = solve(lin, lam)
            trial = poses.copy()
            for c, k in enumerate(S.free):
                trial[k] = pr.retract(poses[k], dp[6 * c:6 * c + 6])
            tlm = lm.copy()
            tlm[S.lms] += dl
            cn, front = cost(S, cam, trial, tlm, edges)
            dmax = max(float(np.abs(dp).max()) if len(dp) else 0.0, float(np.abs(dl).max()) if len(dl) else 0.0)
            tiny = ok and dmax < 1e-12
            if ok and front and np.isfinite(cn) and cn < cur:
                rel = (cur - cn) / cur
                poses, lm, cur = trial, tlm, cn
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
    for k in range(S.K):
        if S.col[k] < 0:
            poses[k] = poses0[k]
    lm[~S.present] = lm0[~S.present]
    wrong, margin = chi2(prob, S, cam, sigma, poses, lm)
    rep = dict(iterations=acc + rej, accepted=acc, rejected=rej, n_free=len(S.free), n_isolated=S.n_isolated, n_present=len(S.lms),
               n_thin=S.n_thin, n_factors=S.n_factors, initial_cost=c0, final_cost=cur, final_lambda=lam)
    return dict(kf_pose=poses, lm=lm, pair_wrong=wrong, report=rep, margin=margin, structure=S)


# ---- problems of the tests ---------------------------------------------------------------------------------------------------
def look_z(x, y=0.0, z=0.0, yaw=0.0):
    """a camera at (x, y, z) looking along +z, turned by yaw about y"""
    return pr.make_pose(pr.so3_exp(np.array([0.0, yaw, 0.0])), np.array([x, y, z], np.float64))


def observe(rig, T, X, side):
    fx, fy, cx, cy, bl = camera(rig)
    q = T[:3, :3].T @ (X - T[:3, 3])
    return np.array([fx * (q[0] - bl * side) / q[2] + cx, fy * q[1] / q[2] + cy]), q[2]


def make_problem(truth, fixed, lm_true, views, seed, rig=RIG, pix_noise=0.3, pose_noise=(0.004, 0.01), point_noise=0.01, outlier_frac=0.0,
                 flags=None, local=None):
    """truth (K, 4, 4), lm_true (L, 3), views: [(kf, lm), ...] in pair order.  Measurements are the true projections plus noise
    of pix_noise * 1.2^octave pixels (gross outliers: + 25 px), rounded to float32; the start is the truth disturbed by
    pose_noise (rad, m) on the non-fixed keyframes and point_noise on the landmarks.  flags: the pair flags (default 3: left
    and right); the octave follows the depth."""
    rng = np.random.default_rng(seed)
    truth = np.array(truth, np.float64)
    K = len(truth)
    pk, pl, pf, puv, poct = [], [], [], [], []
    for p, (k, l) in enumerate(views):
        uL, depth = observe(rig, truth[k], lm_true[l], 0)
        uR, _ = observe(rig, truth[k], lm_true[l], 1)
        assert depth > 0.2, (k, l, depth)
        octv = int(np.clip(np.round(np.log(depth / 2.0) / np.log(1.2)), 0, 7))
        nz = rng.normal(0, pix_noise * float(SCALE[octv]), 4) if pix_noise else np.zeros(4)
        if outlier_frac and rng.random() < outlier_frac:
            nz = nz + rng.choice([-1.0, 1.0], 4) * rng.uniform(15, 35, 4)
        pk.append(k); pl.append(l); pf.append(3 if flags is None else int(flags[p]))
        puv.append(np.concatenate([uL, uR]) + nz); poct.append([octv, octv])
    fixed = np.asarray(fixed, np.uint8)
    start = truth.copy()
    for k in range(K):
        if not fixed[k]:
            start[k] = truth[k] @ pr.random_pose(rng, pose_noise[0], pose_noise[1])
    lm0 = np.asarray(lm_true, np.float64).reshape(-1, 3) + rng.normal(0, point_noise, (len(lm_true), 3)) if len(lm_true) else np.zeros((0, 3))
    return dict(rig=rig, kf_pose=start, kf_pose_true=truth, kf_fixed=fixed, kf_local=np.ones(K, np.uint8) if local is None else np.asarray(local, np.uint8),
                lm=lm0, lm_true=np.asarray(lm_true, np.float64).reshape(-1, 3), pair_kf=np.array(pk, np.int32), pair_lm=np.array(pl, np.int32),
                pair_flags=np.array(pf, np.uint8), pair_uv=np.array(puv, np.float32).reshape(-1, 4), pair_oct=np.array(poct, np.int32).reshape(-1, 2))


def cloud(rng, n, x0, x1):
    """n landmarks 2 - 5 m in front of cameras at x0 .. x1 on the x axis"""
    return np.stack([rng.uniform(x0 - 0.8, x1 + 0.8, n), rng.uniform(-0.8, 0.8, n), rng.uniform(2.0, 5.0, n)], 1)


def one_free(seed=1):
    rng = np.random.default_rng(seed)
    return make_problem([look_z(0.0), look_z(0.4)], [1, 0], cloud(rng, 8, 0.0, 0.4), [(k, l) for l in range(8) for k in range(2)], seed), []


def no_shared(seed=2, n_free=5):
    """free keyframes 1 .. n_free, each with six landmarks of its own that only the fixed keyframe 0 sees too"""
    rng = np.random.default_rng(seed)
    truth = [look_z(0.0)] + [look_z(0.3 * k, 0.05 * k) for k in range(1, n_free + 1)]
    lm = cloud(rng, 6 * n_free, 0.0, 0.3 * n_free)
    views = [(k, l) for l in range(len(lm)) for k in (0, 1 + l % n_free)]
    return make_problem(truth, [1] + [0] * n_free, lm, views, seed), []


def dense(seed=3, n_free=12, n_lm=40):
    """a fixed keyframe and n_free free ones on an arc, all seeing all landmarks"""
    rng = np.random.default_rng(seed)
    truth = [look_z(0.25 * k - 1.5, 0.02 * (k % 3), 0.0, -0.03 * (k - 6)) for k in range(n_free + 1)]
    lm = np.stack([rng.uniform(-1.2, 1.2, n_lm), rng.uniform(-0.8, 0.8, n_lm), rng.uniform(2.5, 5.0, n_lm)], 1)
    return make_problem(truth, [1] + [0] * n_free, lm, [(k, l) for l in range(n_lm) for k in range(n_free + 1)], seed), []


def long_list(seed=4, n_lm=300):
    """two free keyframes sharing n_lm landmarks; the fixed keyframe sees every tenth"""
    rng = np.random.default_rng(seed)
    truth = [look_z(0.0), look_z(0.4, 0.03), look_z(0.8, -0.02)]
    lm = cloud(rng, n_lm, 0.0, 0.8)
    views = [(k, l) for l in range(n_lm) for k in ((0, 1, 2) if l % 10 == 0 else (1, 2))]
    return make_problem(truth, [1, 0, 0], lm, views, seed), []


def chain(n_free=172, seed=5, per_kf=4, span=3):
    """keyframe 0 fixed, n_free free ones 0.3 m apart; per_kf landmarks start at every keyframe and are seen by `span` consecutive ones"""
    rng = np.random.default_rng(seed)
    K = n_free + 1
    truth = [look_z(0.3 * k, 0.02 * np.sin(0.7 * k), 0.01 * np.cos(0.3 * k), 0.02 * np.sin(0.2 * k)) for k in range(K)]
    lm, views = [], []
    for k in range(K - 1):
        ks = [q for q in range(k, k + span) if q < K]
        for X in cloud(rng, per_kf, 0.3 * ks[0], 0.3 * ks[-1]):
            views += [(q, len(lm)) for q in ks]
            lm.append(X)
    return make_problem(truth, [1] + [0] * n_free, np.array(lm), views, seed), []


def chain_loop(n_free=260, seed=6, per_kf=2):
    """out along x and back over the same ground: keyframe k > n_free / 2 stands beside keyframe n_free - k, and every landmark
    is seen by three consecutive keyframes of the way out and by the keyframes of the way back that stand beside them"""
    rng = np.random.default_rng(seed)
    K = n_free + 1
    half = n_free // 2
    xs = [0.3 * (k if k <= half else n_free - k) for k in range(K)]
    truth = [look_z(xs[k], 0.0 if k <= half else 0.06, 0.01 * np.cos(0.3 * k), 0.02 * np.sin(0.2 * k)) for k in range(K)]
    lm, views = [], []
    for k in range(half - 1):
        ks = [k, k + 1, k + 2]
        back = [n_free - q for q in ks if n_free - q > half and n_free - q < K]
        for X in cloud(rng, per_kf, xs[k], xs[k + 2]):
            views += [(q, len(lm)) for q in ks + sorted(back)]
            lm.append(X)
    return make_problem(truth, [1] + [0] * n_free, np.array(lm), views, seed), []


def mixed(seed=7):
    """left-only, right-only and both; every octave; a thin landmark; a landmark seen only by fixed keyframes; pairs with flags 0;
    an isolated keyframe; edges with one fixed end; duplicate edges"""
    rng = np.random.default_rng(seed)
    K = 9                                             # 0, 1 fixed; 2 .. 7 free; 8 isolated (only a flags-0 pair and a thin landmark)
    truth = [look_z(0.3 * k, 0.03 * (k % 2), 0.0, 0.02 * k) for k in range(K)]
    n = 48
    lm = np.stack([rng.uniform(-0.5, 2.8, n), rng.uniform(-0.8, 0.8, n), 2.0 * 1.2 ** (np.arange(n) % 8) * rng.uniform(0.97, 1.03, n)], 1)      # every octave
    views = []
    for l in range(n - 3):
        ks = sorted(rng.choice(np.arange(8), 4, replace=False))
        views += [(int(k), l) for k in ks]
    views += [(0, n - 3), (1, n - 3)]                 # seen only by the fixed keyframes
    views += [(8, n - 2)]                             # thin: one left factor
    views += [(8, 0), (3, n - 1), (4, n - 1)]         # flags 0 (the first), then landmark n - 1 with one left and one right factor
    flags = [(3, 3, 1, 2, 3, 3, 3, 1)[p % 8] for p in range(len(views) - 4)] + [1, 0, 1, 2]
    prob = make_problem(truth, [1, 1, 0, 0, 0, 0, 0, 0, 0], lm, views, seed, flags=flags, local=[1, 0, 1, 1, 1, 0, 1, 1, 1])
    t = prob["kf_pose_true"]
    e = lambda i, j, wr, wt: pr.noisy_edge(rng, list(t), i, j, 0.002, 0.004, wr, wt)
    edges = [e(1, 2, 50.0, 80.0), e(2, 3, 40.0, 40.0), e(7, 0, 30.0, 60.0), e(4, 5, 40.0, 40.0)]
    edges += [edges[1], e(0, 1, 10.0, 10.0)]          # a duplicate, and an edge between the fixed keyframes
    return prob, edges


def edges_only(seed=8):
    poses, fixed, edges = pr.ring_graph(8, seed)
    prob = dict(rig=RIG, kf_pose=poses, kf_fixed=fixed, kf_local=np.ones(8, np.uint8), lm=np.zeros((0, 3)), pair_kf=np.zeros(0, np.int32),
                pair_lm=np.zeros(0, np.int32), pair_flags=np.zeros(0, np.uint8), pair_uv=np.zeros((0, 4), np.float32), pair_oct=np.zeros((0, 2), np.int32))
    return prob, edges


def structure_only(seed=9):
    rng = np.random.default_rng(seed)
    truth = [look_z(0.3 * k, 0.02 * k) for k in range(5)]
    lm = cloud(rng, 30, 0.0, 1.2)
    views = [(int(k), l) for l in range(30) for k in sorted(rng.choice(5, 3, replace=False))]
    return make_problem(truth, [1] * 5, lm, views, seed, point_noise=0.05), []


def rejected(seed=10):
    """landmarks that start far behind their true depth, seen at a shallow angle: under lambda0 = 10 the first steps overshoot"""
    rng = np.random.default_rng(seed)
    truth = [look_z(0.0), look_z(0.3, 0.02), look_z(0.6, -0.02), look_z(0.9)]
    lm = np.stack([rng.uniform(-0.3, 1.2, 24), rng.uniform(-0.4, 0.4, 24), rng.uniform(0.5, 0.9, 24)], 1)
    prob = make_problem(truth, [1, 0, 0, 0], lm, [(k, l) for l in range(24) for k in range(4)], seed, point_noise=0.0, pose_noise=(0.02, 0.05))
    prob["lm"] = prob["lm"] + np.array([0.0, 0.0, 6.0])
    return prob, []


def outliers(seed=11):
    prob, _ = chain(40, seed, per_kf=8, span=4)
    rng = np.random.default_rng(seed)
    uv = prob["pair_uv"].copy()
    bad = rng.random(len(uv)) < 0.02
    uv[bad] += (rng.choice([-1.0, 1.0], (int(bad.sum()), 4)) * rng.uniform(15, 35, (int(bad.sum()), 4))).astype(np.float32)
    prob["pair_uv"] = uv
    prob["n_bad"] = int(bad.sum())
    return prob, []


CASES = dict(one_free=one_free, no_shared=no_shared, dense12=dense, long_list=long_list, chain172=chain, chain260_loop=chain_loop, mixed=mixed,
             edges_only=edges_only, structure_only=structure_only, rejected=rejected, outliers=outliers)
PARAMS = dict(rejected=dict(max_iterations=2, lambda0=10.0))
