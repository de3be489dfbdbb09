"""The yaw-only restatement (tests/pgo_yaw_ref.py) against itself, on the CPU: its analytic gradient against central differences
of the cost, the invariance of the axis under every pose change, its final cost against the 6-DoF restatement's, and the
projection of a claimed pose (the twist about the axis, in closed form).

Bounds: the gradient within 1e-7 of |g|_inf (central differences with h = 1e-6 on costs of O(1e-2 .. 1): truncation h^2 and
rounding eps * cost / h are both far below; measured 3e-10), the axis within 1e-12 (a product of three rotation matrices of
rounding error 1e-16 each), a tilt's twist within 1e-15 (the atan2 of a numerator that is a rounding error of sin(2 deg) terms)."""
import functools
import numpy as np
import pytest
import pgo_ref as pr
import pgo_yaw_ref as py

Y = np.array([0.0, 1.0, 0.0])
TILTED = np.array([0.3, -2.0, 0.5])            # (not unit length: the restatement normalises as the library does)

GRAPHS = {
    "ring16": lambda: pr.ring_graph(16, 16),
    "chain3": lambda: pr.chain_graph(3, (0, 2)),
}


@functools.lru_cache(maxsize=None)
def graph(name):
    poses, fixed, edges = GRAPHS[name]()
    poses.setflags(write=False)
    fixed.setflags(write=False)
    return poses, fixed, edges


@functools.lru_cache(maxsize=None)
def solved(name, axis_name):
    poses, fixed, edges = graph(name)
    out, rep = py.optimize(poses, fixed, edges, {"y": Y, "tilted": TILTED}[axis_name])
    out.setflags(write=False)
    return out, rep


@pytest.mark.parametrize("axis", [Y, TILTED], ids=["y", "tilted"])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_gradient_against_central_differences(name, axis):
    poses, fixed, edges = graph(name)
    g = py.unit_axis(axis)
    _, grad, free = py.linearize(poses, fixed, edges, g)
    h = 1e-6
    num = np.zeros_like(grad)
    for c, k in enumerate(free):
        for p in range(4):
            d = np.zeros(4)
            d[p] = h
            plus = list(poses); plus[k] = py.retract(poses[k], d, g)
            minus = list(poses); minus[k] = py.retract(poses[k], -d, g)
            num[4 * c + p] = (pr.cost(plus, edges) - pr.cost(minus, edges)) / (2 * h)
    # cost = sum w |r|^2: its gradient is 2 J^T W r
    err = np.abs(num - 2.0 * grad).max() / np.abs(2.0 * grad).max()
    print(name, axis, "gradient error", err)
    assert err <= 1e-7


@pytest.mark.parametrize("axis_name", ["y", "tilted"])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_axis_is_invariant_and_cost_not_below_6dof(name, axis_name):
    poses, fixed, edges = graph(name)
    g = py.unit_axis({"y": Y, "tilted": TILTED}[axis_name])
    out, rep = solved(name, axis_name)
    assert rep["accepted"] >= 1 and rep["final_cost"] < rep["initial_cost"]
    for k in range(len(poses)):
        dR = out[k][:3, :3] @ poses[k][:3, :3].T
        assert np.abs(dR @ g - g).max() <= 1e-12, k
    assert out[0].tobytes() == poses[0].tobytes()
    out6, rep6 = pr.optimize(poses, fixed, edges)
    print(name, axis_name, rep, "6-DoF", rep6["final_cost"])
    assert rep["final_cost"] >= rep6["final_cost"]
    # what the 6-DoF solve does to the axis: the reason for this solve
    tilt6 = max(np.abs(out6[k][:3, :3] @ poses[k][:3, :3].T @ g - g).max() for k in range(len(poses)))
    assert tilt6 > 1e-4
    assert py.gradient_inf(out, fixed, edges, g) <= 1e-6 * py.gradient_inf(poses, fixed, edges, g)


@pytest.mark.parametrize("axis", [Y, TILTED], ids=["y", "tilted"])
def test_projection_identities(axis):
    g = py.unit_axis(axis)
    for psi in (-3.0, -0.4, 0.0, 1e-9, 0.2 * np.pi / 180, 2.5):
        assert abs(py.twist(pr.so3_exp(psi * g), g) - psi) <= 1e-15 * max(1.0, abs(psi)) + 1e-16
    e = np.cross(g, [1.0, 0.0, 0.0])
    e /= np.linalg.norm(e)
    for a in (2.0 * np.pi / 180, -0.7):
        assert abs(py.twist(pr.so3_exp(a * e), g)) <= 1e-15


def test_projection_of_a_claim_is_idempotent():
    rng = np.random.default_rng(5)
    for axis in (Y, TILTED):
        g = py.unit_axis(axis)
        T_cam = pr.random_pose(rng, 1.0, 3.0)
        e = np.cross(g, [0.0, 0.0, 1.0]); e /= np.linalg.norm(e)
        T_corr = pr.make_pose(pr.so3_exp(0.2 * np.pi / 180 * g) @ pr.so3_exp(1.0 * np.pi / 180 * e) @ T_cam[:3, :3], T_cam[:3, 3] + [0.01, 0.0, 0.0])
        Tp, th, tilt = py.project_claim(T_corr, T_cam, axis)
        assert abs(th - 0.2 * np.pi / 180) <= 1e-4 and abs(tilt - 1.0 * np.pi / 180) <= 1e-4
        dR = Tp[:3, :3] @ T_cam[:3, :3].T
        assert np.abs(dR @ g - g).max() <= 1e-15
        Tpp, th2, tilt2 = py.project_claim(Tp, T_cam, axis)
        assert abs(th2 - th) <= 1e-15 and tilt2 <= 1e-15 and np.abs(Tpp - Tp).max() <= 1e-15
