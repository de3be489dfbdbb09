"""The numpy restatement of the global bundle adjustment (tests/gba_ref.py) checked on its own: Jacobians against central
differences, the cost against the local BA's checker, the pose-graph case, a known answer, and the distance of every chi2
statistic of the GPU tests' problems from its threshold."""
import functools
import numpy as np
import pytest
import gba_ref as gr
import pgo_ref as pr
import synth


@functools.lru_cache(maxsize=None)
def solved(name):
    prob, edges = gr.CASES[name]()
    return prob, edges, gr.optimize(prob, edges, **gr.PARAMS.get(name, {}))


def test_jacobians_against_central_differences():
    prob, edges = gr.mixed()
    S = gr.Structure(prob, edges, gr.INV_SIGMA)
    cam = gr.camera(prob["rig"])
    poses, lm = np.array(prob["kf_pose"]), np.array(prob["lm"])
    _, _, Jp, Jl = gr.project(S, cam, poses, lm, True)
    h = 1e-6
    worst = 0.0
    for f in range(0, S.n_factors, 7):
        k, l = S.f_kf[f], S.f_lm[f]
        for c in range(9):
            d = np.zeros(9)
            d[c] = h
            r = []
            for sgn in (1.0, -1.0):
                P2, L2 = poses.copy(), lm.copy()
                P2[k] = pr.retract(poses[k], sgn * d[:6])
                L2[l] = lm[l] + sgn * d[6:]
                r.append(gr.project(S, cam, P2, L2, False)[0][f])
            num = (r[0] - r[1]) / (2 * h)
            ana = Jp[f][:, c] if c < 6 else Jl[f][:, c - 6]
            worst = max(worst, float(np.abs(num - ana).max() / max(1.0, np.abs(ana).max())))
    print("worst relative Jacobian error", worst)
    assert worst < 1e-7            # central differences at h = 1e-6: truncation ~ h^2, rounding ~ 1e-16 / h


def test_initial_cost_is_twice_the_local_ba_error(oracle):
    """a synth.make_ba_problem instance without thin landmarks: every landmark the checker optimises is present here; its between
    factors measure the current relative poses, so they are zero at the start"""
    prob = synth.make_ba_problem(n_local=6, n_fixed=2, n_lm=300, seed=21, outlier_frac=0.0)
    fl = prob["pair_flags"].astype(int)
    fac = np.bincount(prob["pair_lm"], weights=(fl & 1) + (fl >> 1), minlength=len(prob["lm"]))
    keep = fac[prob["pair_lm"]] >= 2
    assert keep.sum() > 1000          # (pairs of landmarks with a single factor, if the seed has any, are dropped)
    prob = dict(prob, **{k: prob[k][keep] for k in ("pair_kf", "pair_lm", "pair_flags", "pair_uv", "pair_oct")})
    ex = oracle.Extractor(1500)
    ref = oracle.local_ba(prob["rig"], ex.sigmaFactor, ex.InvSigmaFactor, prob)
    S = gr.Structure(prob, [], ex.InvSigmaFactor)
    assert S.n_thin == int((fac < 2).sum()) and S.n_factors == ref["residuals"]
    c0, front = gr.cost(S, gr.camera(prob["rig"]), np.array(prob["kf_pose"]), np.array(prob["lm"]), [])
    print("cost", c0, "2 x initialError", 2 * ref["reports"][0]["initialError"])
    assert front and abs(c0 - 2 * ref["reports"][0]["initialError"]) <= 1e-11 * c0


def test_without_pairs_it_is_the_pose_graph_solve():
    for seed in (8, 9):
        prob, edges = gr.edges_only(seed)
        out = gr.optimize(prob, edges)
        want, rep = pr.optimize(prob["kf_pose"], prob["kf_fixed"], edges)
        assert np.abs(out["kf_pose"] - want).max() <= 1e-13
        for k in ("accepted", "rejected", "n_free", "n_isolated"):
            assert out["report"][k] == rep[k]
        assert out["report"]["final_cost"] == pytest.approx(rep["final_cost"], rel=1e-12)


def test_known_answer():
    """Exact observations rounded to float32, as the ABI carries them.  To first order the minimiser moves from the truth by
    -(J^T J)^-1 J^T e, e the whitened rounding errors: |dx|_2 <= |e|_2 / sigma_min(J).  A measurement below 1024 px is rounded by
    at most 2^-15 px (half an ulp of [512, 1024)); the whitening is at most 1.  The test allows twice that bound (second-order
    terms, the stop rule)."""
    rng = np.random.default_rng(31)
    truth = [gr.look_z(0.3 * k, 0.03 * (k % 2), 0.0, 0.03 * k) for k in range(5)]
    lm = gr.cloud(rng, 40, 0.0, 1.2)
    views = [(int(k), l) for l in range(40) for k in sorted(rng.choice(5, 4, replace=False))]
    prob = gr.make_problem(truth, [1, 0, 0, 0, 0], lm, views, 31, pix_noise=0.0)
    assert np.abs(prob["pair_uv"]).max() < 1024 and float(gr.INV_SIGMA.max()) <= 1.0
    out = gr.optimize(prob, [])
    S = out["structure"]
    Hpp, _, Hll, _, Hpl = gr.linearize(S, gr.camera(prob["rig"]), np.array(prob["kf_pose_true"]), np.array(prob["lm_true"]), [])
    n6, nl = len(Hpp), len(Hll)
    H = np.zeros((n6 + 3 * nl, n6 + 3 * nl))
    H[:n6, :n6] = Hpp
    H[:n6, n6:] = Hpl.reshape(n6, 3 * nl)
    H[n6:, :n6] = Hpl.reshape(n6, 3 * nl).T
    for l in range(nl):
        H[n6 + 3 * l:n6 + 3 * l + 3, n6 + 3 * l:n6 + 3 * l + 3] = Hll[l]
    bound = 2.0 * np.sqrt(2 * S.n_factors) * 2.0 ** -15 / np.sqrt(np.linalg.eigvalsh(H)[0])
    dp = np.abs(out["kf_pose"] - prob["kf_pose_true"]).max()
    dl = np.abs(out["lm"] - prob["lm_true"]).max()
    print("bound", bound, "pose", dp, "landmark", dl, out["report"])
    assert out["report"]["final_cost"] < 2 * S.n_factors * 2.0 ** -30
    assert dp <= bound and dl <= bound


@pytest.mark.parametrize("name", list(gr.CASES))
def test_no_statistic_sits_on_its_threshold(name):
    """the GPU tests compare flags exactly: no chi2 statistic of their problems may lie within 1e-9 (relative) of its threshold"""
    prob, edges, out = solved(name)
    print(name, out["report"], "flags", int(out["pair_wrong"].sum()), "margin", out["margin"])
    assert out["margin"] > 1e-9
    S = out["structure"]
    start = np.asarray(prob["kf_pose"])
    assert all(out["kf_pose"][k].tobytes() == start[k].tobytes() for k in range(S.K) if S.col[k] < 0)
    assert out["report"]["final_cost"] <= out["report"]["initial_cost"]


def test_refusals_of_the_restatement():
    prob, _ = gr.one_free()
    with pytest.raises(ValueError, match="free gauge"):
        gr.optimize(dict(prob, kf_fixed=np.zeros(2, np.uint8)))
    lm = prob["lm"].copy()
    lm[2, 2] = -1.0
    with pytest.raises(ValueError, match="pair 4"):
        gr.optimize(dict(prob, lm=lm))
