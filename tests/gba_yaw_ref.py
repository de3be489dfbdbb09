"""CPU restatement of the yaw-only (4-DoF keyframe) global bundle adjustment (vslam_global_ba_yaw)
in numpy.  Everything but the keyframe parameterisation is gba_ref's, used as it is: Structure, project, cost, linearize (the
6-DoF blocks), solve, chi2, the refusals and the schedule.  A free keyframe has the parameters (theta, delta) with the
retraction T <- [Exp(theta g) R, t + delta] about the unit axis g (pgo_yaw_ref.retract); the linearised blocks are mapped through
the block-diagonal M of pgo_yaw_ref.chain_factor: Hpp4 = M^T Hpp M, gp4 = M^T gp, Hpl4 = M^T Hpl.  The cost does not depend on
the parameterisation.  This file is the authority on the rules.

optimize also returns `decision_margin`: how far the closest accept / reject or stop decision of the pass was from flipping,
    |c_new - c_cur| / c_cur          over the trials with a finite solve
    |rel - 1e-10| / 1e-10            over the accepted trials
A comparison of trial counts with the device is meaningful only where it is >= 1e-12: a condition on the INPUT, not a tolerance
on the code.  SEEDS holds, per case of gba_ref.CASES, a seed whose problem satisfies it under AXIS (found by search on the CPU;
test_gba_yaw_ref.py asserts it)."""
import numpy as np
import gba_ref as gr
import pgo_ref as pr
import pgo_yaw_ref as py

AXIS = (0.3, 0.9, -0.2)         # the tests' axis: not normalised, not aligned with a coordinate axis


def map_blocks(lin, S, poses, g):
    """the 6-DoF blocks of gba_ref.linearize through M = diag(M_k) over the free keyframes"""
    Hpp, gp, Hll, gl, Hpl = lin
    nf = len(S.free)
    M = np.zeros((6 * nf, 4 * nf))
    for c, k in enumerate(S.free):
        M[6 * c:6 * c + 6, 4 * c:4 * c + 4] = py.chain_factor(poses[k], g)
    return M.T @ Hpp @ M, M.T @ gp, Hll, gl, np.einsum("pq,pnj->qnj", M, Hpl)


def linearize(S, cam, poses, lm, edges, g):
    return map_blocks(gr.linearize(S, cam, poses, lm, edges), S, poses, g)


def retract_all(S, poses, lm, dp, dl, g):
    trial = poses.copy()
    for c, k in enumerate(S.free):
        trial[k] = py.retract(poses[k], dp[4 * c:4 * c + 4], g)
    tlm = lm.copy()
    tlm[S.lms] += dl
    return trial, tlm


def optimize(prob, edges=(), axis=AXIS, sigma=gr.SIGMA, inv_sigma=gr.INV_SIGMA, max_iterations=0, lambda0=0.0):
    """the schedule of vslam_global_ba_yaw: dict(kf_pose, lm, pair_wrong, report, margin, decision_margin, structure)"""
    g = py.unit_axis(axis)
    if not np.all(np.isfinite(g)):
        raise ValueError("the axis is zero or not finite")
    edges = list(edges)
    S = gr.Structure(prob, edges, inv_sigma)
    cam = gr.camera(prob["rig"])
    poses = np.array(prob["kf_pose"], np.float64).reshape(-1, 4, 4)
    lm = np.array(prob["lm"], np.float64).reshape(-1, 3)
    poses0, lm0 = poses.copy(), lm.copy()
    if gr.has_free_gauge(S, edges):
        raise ValueError("free gauge")
    _, z, _, _ = gr.project(S, cam, poses, lm, False)
    if not np.all(z > 0):
        raise ValueError("pair %d is not in front of its camera" % int(S.f_pair[np.flatnonzero(~(z > 0))].min()))
    max_it = max_iterations or gr.DEFAULTS["max_iterations"]
    lam = lambda0 or gr.DEFAULTS["lambda0"]
    c0, _ = gr.cost(S, cam, poses, lm, edges)
    acc = rej = 0
    cur = c0
    dm = np.inf
    stop = not (c0 > 1e-20) or not (len(S.free) or len(S.lms))
    while not stop:
        lin = linearize(S, cam, poses, lm, edges, g)
        while True:
            dp, dl, ok = gr.solve(lin, lam)
            trial, tlm = retract_all(S, poses, lm, dp, dl, g)
            cn, front = gr.cost(S, cam, trial, tlm, edges)
            dmax = max(float(np.abs(dp).max()) if len(dp) else 0.0, float(np.abs(dl).max()) if len(dl) else 0.0)
            tiny = ok and dmax < 1e-12
            if ok and np.isfinite(cn):
                dm = min(dm, abs(cn - cur) / cur)
            if ok and front and np.isfinite(cn) and cn < cur:
                rel = (cur - cn) / cur
                dm = min(dm, abs(rel - 1e-10) / 1e-10)
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
    wrong, margin = gr.chi2(prob, S, cam, sigma, poses, lm)
    rep = dict(iterations=acc + rej, accepted=acc, rejected=rej, n_free=len(S.free), n_isolated=S.n_isolated, n_present=len(S.lms),
               n_thin=S.n_thin, n_factors=S.n_factors, initial_cost=c0, final_cost=cur, final_lambda=lam)
    return dict(kf_pose=poses, lm=lm, pair_wrong=wrong, report=rep, margin=margin, decision_margin=float(dm), structure=S)


def gravity_error(new, old, axis):
    """max over the keyframes of |R_new R_old^T g - g|_inf"""
    g = py.unit_axis(axis)
    new = np.asarray(new).reshape(-1, 4, 4); old = np.asarray(old).reshape(-1, 4, 4)
    return float(max(np.abs(n[:3, :3] @ o[:3, :3].T @ g - g).max() for n, o in zip(new, old)))


# ---- the problems of tests/test_gpu_gba_yaw.py: gba_ref's builders at the shapes and seeds below ------------------------------
def two_free(seed=12):
    """keyframe 0 fixed, two free keyframes that share no landmark with each other: two diagonal blocks, no off-diagonal one"""
    return gr.no_shared(seed, n_free=2)


# `edges_only` and `structure_only` are decided by the last bit of the cost at gba_ref's default seeds (margins 1e-15); these
# are the first seeds from 1 whose problems satisfy decision_margin >= 1e-12 under AXIS (find_seed: 9.5e-11 and 1.6e-12)
SEEDS = dict(edges_only=12, structure_only=17)

# name -> (builder, keyword arguments): the problems the GPU test compares trial counts on
GPU_CASES = dict(
    one_free=(gr.one_free, {}),
    two_free=(two_free, {}),
    no_shared4=(gr.no_shared, dict(n_free=4)),
    no_shared5=(gr.no_shared, dict(n_free=5)),
    dense12=(gr.dense, dict(seed=21)),
    long_list=(gr.long_list, {}),
    chain40=(gr.chain, dict(n_free=40)),
    chain60_loop=(gr.chain_loop, dict(n_free=60)),
    mixed=(gr.mixed, dict(seed=21)),
    rejected=(gr.rejected, {}),
    outliers=(gr.outliers, {}),
    edges_only=(gr.edges_only, dict(seed=SEEDS["edges_only"])),
    structure_only=(gr.structure_only, dict(seed=SEEDS["structure_only"])),
)
PARAMS = dict(rejected=gr.PARAMS["rejected"])


def yaw_noise(seed=13, n_free=12, yaw=0.01, trans=0.03, axis=AXIS):
    """gba_ref.chain whose non-fixed keyframes start at [Exp(theta g) R_true, t_true + d], theta ~ N(0, yaw), d ~ N(0, trans): the
    disturbance lies in the space the yaw-only keyframes can move in"""
    prob, edges = gr.chain(n_free, seed, per_kf=6, span=4)
    rng = np.random.default_rng(seed + 1000)
    g = py.unit_axis(axis)
    start = np.array(prob["kf_pose_true"], np.float64)
    for k in range(len(start)):
        if not prob["kf_fixed"][k]:
            start[k] = py.retract(start[k], np.concatenate([[rng.normal(0, yaw)], rng.normal(0, trans, 3)]), g)
    return dict(prob, kf_pose=start), edges


def build(name):
    fn, kw = GPU_CASES[name]
    return fn(**kw)


def find_seed(builder, first=1, last=200, bound=1e-12, **kw):
    """the first seed whose problem has decision_margin >= bound under AXIS, or None"""
    for seed in range(first, last + 1):
        prob, edges = builder(seed=seed)
        try:
            if optimize(prob, edges, AXIS, **kw)["decision_margin"] >= bound:
                return seed
        except ValueError:
            continue
    return None
