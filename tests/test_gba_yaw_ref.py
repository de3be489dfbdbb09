"""The numpy restatement of the yaw-only global bundle adjustment (tests/gba_yaw_ref.py) checked on its own, on the CPU: gravity
is kept, the cost decreases, the pose-graph case equals pgo_yaw_ref, the all-fixed case equals gba_ref, the four keyframe
parameters' Jacobians against central differences, and the condition under which tests/test_gpu_gba_yaw.py may compare trial
counts with the device: no accept / reject or stop decision of a case within 1e-12 (relative) of flipping."""
import functools
import numpy as np
import pytest
import gba_ref as gr
import gba_yaw_ref as gy
import pgo_ref as pr
import pgo_yaw_ref as py


@functools.lru_cache(maxsize=None)
def solved(name):
    prob, edges = gy.build(name)
    return prob, edges, gy.optimize(prob, edges, gy.AXIS, **gy.PARAMS.get(name, {}))


@pytest.mark.parametrize("name", list(gy.GPU_CASES))
def test_gravity_is_kept_and_the_cost_decreases(name):
    prob, edges, out = solved(name)
    rep, S = out["report"], out["structure"]
    tilt = gy.gravity_error(out["kf_pose"], prob["kf_pose"], gy.AXIS)
    six = gr.optimize(prob, edges, **gy.PARAMS.get(name, {}))
    print(name, rep, "gravity error", tilt, "of the 6-DoF restatement", gy.gravity_error(six["kf_pose"], prob["kf_pose"], gy.AXIS))
    assert tilt <= 1e-12
    assert rep["final_cost"] <= rep["initial_cost"] and (rep["accepted"] == 0 or rep["final_cost"] < rep["initial_cost"])
    start = np.asarray(prob["kf_pose"])
    assert all(out["kf_pose"][k].tobytes() == start[k].tobytes() for k in range(S.K) if S.col[k] < 0)
    lm0 = np.asarray(prob["lm"], np.float64)
    assert all(out["lm"][l].tobytes() == lm0[l].tobytes() for l in np.flatnonzero(~S.present))


@pytest.mark.parametrize("name", list(gy.GPU_CASES))
def test_no_decision_hangs_on_the_last_bit(name):
    """a condition on the inputs of the GPU test, not a tolerance on the code"""
    _, _, out = solved(name)
    print(name, "decision margin", out["decision_margin"], "chi2 margin", out["margin"])
    assert out["decision_margin"] >= 1e-12
    assert out["margin"] > 1e-9


def test_recorded_seeds_are_the_first_that_qualify():
    assert gy.find_seed(gr.edges_only) == gy.SEEDS["edges_only"]
    assert gy.find_seed(gr.structure_only) == gy.SEEDS["structure_only"]


def test_without_pairs_it_is_the_yaw_pose_graph_solve():
    """The bound is the one test_gba_ref.py holds the 6-DoF restatement to against pgo_ref: 1e-13 on the poses.  The two
    restatements differ in association only (pgo_yaw_ref sums J4^T W J4 per edge, this one maps the summed 6-DoF blocks,
    M^T H M); at convergence the step that carries that rounding difference has shrunk far below it (measured: 4.4e-16).  The
    recorded seed only: at gba_ref's seeds 8 and 9 the last accept / reject decision hangs on the last bit of the cost (decision
    margins 1e-15), the two associations stop a trial apart there, and the poses then differ by 2.5e-12."""
    for seed in (gy.SEEDS["edges_only"],):
        prob, edges = gr.edges_only(seed)
        out = gy.optimize(prob, edges, gy.AXIS)
        assert out["decision_margin"] >= 1e-12
        want, rep = py.optimize(prob["kf_pose"], prob["kf_fixed"], edges, gy.AXIS)
        print("seed", seed, "difference", np.abs(out["kf_pose"] - want).max())
        assert np.abs(out["kf_pose"] - want).max() <= 1e-13
        for k in ("accepted", "rejected", "n_free", "n_isolated"):
            assert out["report"][k] == rep[k]
        assert out["report"]["final_cost"] == pytest.approx(rep["final_cost"], rel=1e-12)


def test_all_fixed_is_the_six_dof_restatement():
    """no keyframe parameter is left: the same arithmetic, the same bytes"""
    for seed in (9, gy.SEEDS["structure_only"]):
        prob, edges = gr.structure_only(seed)
        a, b = gy.optimize(prob, edges, gy.AXIS), gr.optimize(prob, edges)
        assert a["kf_pose"].tobytes() == b["kf_pose"].tobytes() and a["lm"].tobytes() == b["lm"].tobytes()
        assert np.array_equal(a["pair_wrong"], b["pair_wrong"]) and a["report"] == b["report"]


def test_jacobians_against_central_differences():
    """d r / d (theta, delta) of the projection factors and of the edges, as the mapped blocks use them: the gradient of the
    cost / 2 over the four parameters of every free keyframe"""
    prob, edges = gr.mixed()
    g = py.unit_axis(gy.AXIS)
    S = gr.Structure(prob, edges, gr.INV_SIGMA)
    cam = gr.camera(prob["rig"])
    poses, lm = np.array(prob["kf_pose"]), np.array(prob["lm"])
    _, gp4, _, _, _ = gy.linearize(S, cam, poses, lm, edges, g)
    r0, _, Jp, _ = gr.project(S, cam, poses, lm, True)
    h = 1e-6
    worst = worst_g = 0.0
    for c, k in enumerate(S.free):
        M = py.chain_factor(poses[k], g)
        fs = np.flatnonzero(S.f_kf == k)
        for q in range(4):
            d = np.zeros(4)
            d[q] = h
            r, cst = [], []
            for sgn in (1.0, -1.0):
                P2 = poses.copy()
                P2[k] = py.retract(poses[k], sgn * d, g)
                r.append(gr.project(S, cam, P2, lm, False)[0][fs])
                cst.append(gr.cost(S, cam, P2, lm, edges)[0])
            num = (r[0] - r[1]) / (2 * h)
            ana = (Jp[fs] @ M)[:, :, q]
            if len(fs):
                worst = max(worst, float(np.abs(num - ana).max() / max(1.0, np.abs(ana).max())))
            worst_g = max(worst_g, abs((cst[0] - cst[1]) / (4 * h) - gp4[4 * c + q]) / max(1.0, abs(gp4[4 * c + q])))
    print("worst relative Jacobian error", worst, "worst relative gradient error", worst_g)
    assert worst < 1e-7            # central differences at h = 1e-6: truncation ~ h^2, rounding ~ 1e-16 / h
    assert worst_g < 1e-6          # (the cost's curvature is larger: its h^2 term too)


def test_mapped_blocks_are_the_blocks_of_the_mapped_jacobian():
    """Hpp4 = M^T Hpp M is J4^T J4 of the stacked Jacobian; checked on the diagonal block and gradient of one keyframe"""
    prob, edges = gr.dense(seed=21)
    g = py.unit_axis(gy.AXIS)
    S = gr.Structure(prob, edges, gr.INV_SIGMA)
    cam = gr.camera(prob["rig"])
    poses, lm = np.array(prob["kf_pose"]), np.array(prob["lm"])
    H4, g4, _, _, Hpl4 = gy.linearize(S, cam, poses, lm, edges, g)
    r, _, Jp, Jl = gr.project(S, cam, poses, lm, True)
    c, k = 3, S.free[3]
    fs = np.flatnonzero(S.f_kf == k)
    J4 = Jp[fs] @ py.chain_factor(poses[k], g)
    assert np.allclose(H4[4 * c:4 * c + 4, 4 * c:4 * c + 4], np.einsum("nai,naj->ij", J4, J4), rtol=1e-12, atol=1e-9)
    assert np.allclose(g4[4 * c:4 * c + 4], np.einsum("nai,na->i", J4, r[fs]), rtol=1e-12, atol=1e-9)
    l = int(S.f_lm[fs[0]])
    fl = fs[S.f_lm[fs] == l]
    assert np.allclose(Hpl4[4 * c:4 * c + 4, S.lcol[l]], np.einsum("nai,naj->ij", Jp[fl] @ py.chain_factor(poses[k], g), Jl[fl]), rtol=1e-12, atol=1e-9)


def test_refusals_of_the_restatement():
    prob, _ = gr.one_free()
    with pytest.raises(ValueError, match="free gauge"):
        gy.optimize(dict(prob, kf_fixed=np.zeros(2, np.uint8)))
    with pytest.raises(ValueError, match="axis"):
        with np.errstate(all="ignore"):
            gy.optimize(prob, [], (0.0, 0.0, 0.0))
