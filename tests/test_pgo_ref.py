"""The CPU restatement of the pose-graph optimisation (tests/pgo_ref.py) checked on its own: the stage has no reference
counterpart, so the restatement is what the kernels are pinned to (tests/test_gpu_pgo.py) and has to stand by itself."""
import numpy as np
import pytest
import pgo_ref as pr


def test_exp_log_round_trip():
    rng = np.random.default_rng(0)
    for scale in (1e-9, 1e-4, 0.3, 2.0, 3.1):
        w = rng.uniform(-1, 1, 3)
        w *= scale / np.linalg.norm(w)
        R = pr.so3_exp(w)
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14
        assert np.abs(pr.so3_log(R) - w).max() < 1e-9 * max(1.0, scale / (np.pi - scale))


@pytest.mark.parametrize("rot", [1e-7, 0.05, 1.0, 3.0])
def test_jacobians_against_central_differences(rot):
    rng = np.random.default_rng(1)
    h = 1e-6
    for _ in range(5):
        Ti, Tj = pr.random_pose(rng, 2.0, 3.0), pr.random_pose(rng, 2.0, 3.0)
        Z = pr.rigid_inv(Ti) @ Tj @ pr.random_pose(rng, rot, 0.5)
        _, Ji, Jj = pr.jacobians(Ti, Tj, Z)
        for which, J in ((0, Ji), (1, Jj)):
            num = np.zeros((6, 6))
            for k in range(6):
                d = np.zeros(6)
                d[k] = h
                if which == 0:
                    rp, rm = pr.residual(pr.retract(Ti, d), Tj, Z), pr.residual(pr.retract(Ti, -d), Tj, Z)
                else:
                    rp, rm = pr.residual(Ti, pr.retract(Tj, d), Z), pr.residual(Ti, pr.retract(Tj, -d), Z)
                num[:, k] = (rp - rm) / (2 * h)
            assert np.abs(num - J).max() <= 1e-6, (rot, which, np.abs(num - J).max())


def test_exact_graph_returns_unchanged():
    poses, fixed, edges = pr.exact_graph()
    out, rep = pr.optimize(poses, fixed, edges)
    assert rep["initial_cost"] <= 1e-20
    assert rep["iterations"] == 0 and rep["accepted"] == 0 and rep["rejected"] == 0
    assert out.tobytes() == poses.tobytes()


@pytest.mark.parametrize("n", [2, 8, 64])
def test_ring_converges_to_a_stationary_point(n):
    poses, fixed, edges = pr.ring_graph(n, seed=n)
    g0 = pr.gradient_inf(poses, fixed, edges)
    out, rep = pr.optimize(poses, fixed, edges)
    assert rep["accepted"] >= 1 and rep["accepted"] <= 20
    assert rep["final_cost"] < rep["initial_cost"]
    assert abs(rep["final_cost"] - pr.cost(out, edges)) <= 1e-12 * rep["initial_cost"]
    assert pr.gradient_inf(out, fixed, edges) <= 1e-6 * g0
    assert out[0].tobytes() == poses[0].tobytes()          # the fixed pose does not move by a bit
    for T in out:
        assert np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() < 1e-12 and tuple(T[3]) == (0.0, 0.0, 0.0, 1.0)


def test_complete_graph_with_large_rotations():
    poses, fixed, edges = pr.complete_graph()
    assert max(np.linalg.norm(pr.so3_log(np.asarray(e[2])[:3, :3])) for e in edges) > 3.0
    g0 = pr.gradient_inf(poses, fixed, edges)
    out, rep = pr.optimize(poses, fixed, edges)
    assert pr.gradient_inf(out, fixed, edges) <= 1e-6 * g0
    assert out[0].tobytes() == poses[0].tobytes()


def test_fixed_isolated_and_fixed_fixed_edges():
    poses, fixed, edges = pr.chain_graph(12, (2, 9), fixed_ids=(0, 5))
    poses = np.concatenate([poses, poses[-1:] @ pr.make_pose(np.eye(3), [1.0, 0, 0])])      # pose 12: free, no edge
    fixed = np.concatenate([fixed, [0]]).astype(np.uint8)
    base = pr.cost(poses, edges)
    edges.append((0, 5, np.eye(4), 2.0, 3.0))             # between fixed poses: cost only
    out, rep = pr.optimize(poses, fixed, edges)
    assert rep["n_isolated"] == 1 and rep["n_free"] == 10
    extra = pr.cost(poses, edges[-1:])
    assert abs(rep["initial_cost"] - (base + extra)) <= 1e-12 * (base + extra)
    for k in (0, 5, 12):
        assert out[k].tobytes() == poses[k].tobytes()
    assert rep["final_cost"] >= extra and rep["final_cost"] < rep["initial_cost"]
    # duplicate edges add up: twice the list = twice the weights
    e2 = [(i, j, Z, 2 * a, 2 * b) for (i, j, Z, a, b) in edges]
    o1, r1 = pr.optimize(poses, fixed, edges + edges)
    o2, r2 = pr.optimize(poses, fixed, e2)
    assert np.abs(o1 - o2).max() < 1e-9 and abs(r1["final_cost"] - r2["final_cost"]) <= 1e-9 * r2["final_cost"]


def test_free_gauge_is_detected():
    poses, fixed, edges = pr.ring_graph(8, 1)
    assert not pr.has_free_gauge(8, fixed, edges)
    assert pr.has_free_gauge(8, np.zeros(8, np.uint8), edges)
    # two components, one anchored
    e2 = [e for e in edges if not ({e[0], e[1]} & {4, 5, 6, 7}) or {e[0], e[1]} <= {4, 5, 6, 7}]
    assert pr.has_free_gauge(8, fixed, e2)


def test_move_points():
    rng = np.random.default_rng(2)
    A = np.array([pr.random_pose(rng, 1.0, 2.0) for _ in range(4)])
    B = A.copy()
    B[1:] = np.array([pr.random_pose(rng, 1.0, 2.0) for _ in range(3)])
    X = rng.uniform(-5, 5, (50, 3))
    ref = rng.integers(-1, 4, 50)
    Y = pr.move_points(X, ref, A, B)
    for k in range(50):
        if ref[k] <= 0:
            assert Y[k].tobytes() == X[k].tobytes() or np.abs(Y[k] - X[k]).max() < 1e-14
        else:
            Xc = (np.linalg.inv(A[ref[k]]) @ np.append(X[k], 1.0))
            assert np.abs((B[ref[k]] @ Xc)[:3] - Y[k]).max() < 1e-12
