"""The velocity rule of an IMU relocalisation's second pose (tests/reloc_imu_ref.py: reinit_velocity) on known answers.  The rule
has no reference counterpart: the restatement is what the kernel is pinned to (tests/test_gpu_reloc_imu.py), so it stands here
against closed forms.  Every tolerance is the figure the restatement gave against the closed form when the case was written
(in the docstring), times the stated factor."""
import numpy as np
import pytest
import synth
import reloc_imu_ref as ri

G = (0.0, 9.81, 0.0)
NOISE = (1.6968e-4, 1.9393e-5, 2.0e-3, 3.0e-3)
DT = 0.005
EPS = np.finfo(np.float64).eps
FACTOR = 8.0       # over the measured figure: the closed forms and the restatement round differently, the figure is one sample of that


def _prm(oracle):
    return oracle.imu_params(G, NOISE[0], NOISE[2], NOISE[1], NOISE[3], synth.T_BC1)


def _expm(w):
    th = np.linalg.norm(w)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + W if th < 1e-12 else np.eye(3) + np.sin(th) / th * W + (1 - np.cos(th)) / th ** 2 * W @ W


def _T(R, t):
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = t
    return T


def _rigid_inv(T):
    return _T(T[:3, :3].T, -T[:3, :3].T @ T[:3, 3])


R0 = _expm(np.array([0.3, -0.2, 0.5]))
P0 = np.array([1.5, -0.4, 2.0])
BRS = np.asarray(synth.T_BC1, np.float64)[:3, :3]
ARM = np.asarray(synth.T_BC1, np.float64)[:3, 3]


@pytest.mark.parametrize("n", [1, 2, 13, 19])
def test_constant_specific_force_gives_the_analytic_velocities(oracle, n):
    """No rotation, constant world acceleration a, start velocity v0, exact samples: the integrator is exact for a constant
    specific force, t_new = p0 + v0 T + a T^2 / 2, so velocity_prev = v0 and velocity = v0 + a T (T = n dt = deltaTij).
    Measured: |velocity_prev - v0| and |velocity - (v0 + a T)| between 2.2e-14 (n = 2) and 1.62e-13 m/s (n = 19) - roundings of
    positions of ~2 m, 2e-16 each, through the division by dt; rot_residual exactly 0 (no rotation: pred.R is R_prev bit for bit;
    held to 9 eps, one rounding in each of nine unit-size entries)."""
    a = np.array([0.7, -0.3, 1.1]); v0 = np.array([0.4, 0.25, -0.6])
    bias = np.array([0.02, -0.01, 0.03, 0.001, -0.002, 0.0015])
    f_body = R0.T @ (a - np.array(G))
    S = np.tile(np.concatenate([BRS.T @ f_body + bias[:3], BRS.T @ np.zeros(3) + bias[3:]]), (n, 1))
    T = n * DT
    t_new = P0 + v0 * T + 0.5 * a * T * T
    r = ri.reinit_velocity(oracle, _prm(oracle), bias, S, np.full(n, DT), _T(R0, P0), _rigid_inv(_T(R0, t_new)))
    e0 = np.abs(r["velocity_prev"] - v0).max(); e1 = np.abs(r["velocity"] - (v0 + a * T)).max()
    print("n %d: dt %.3f  velocity_prev error %.2e  velocity error %.2e  rot_residual %.2e" % (n, r["dt"], e0, e1, r["rot_residual"]))
    assert r["dt"] == pytest.approx(T, rel=1e-14)
    assert e0 <= FACTOR * 1.62e-13 and e1 <= FACTOR * 1.62e-13
    assert r["rot_residual"] <= 9 * EPS


@pytest.mark.parametrize("n", [2, 19])
def test_pure_rotation_at_rest_gives_zero_velocities(oracle, n):
    """The camera turns about its own centre at a constant body rate w and does not move; the IMU sits at the lever arm of T_bc1
    and measures, exactly, the specific force there: w x (w x arm) - R(t)^T g in body axes, sampled at the start of each period
    (the integrator rotates a sample by the attitude at the start of its period, so R(t_k) acc_k = -g for every k).
    correctMeasurementsBySensorPose takes the lever arm's term w x (w x arm) out again - left in, it alone would put
    |w x (w x arm)| T = 2.7e-3 m/s (n = 19) into the velocities - and the tangent integrator is exact for a constant rate
    (theta = w T), so both velocities and rot_residual are at rounding level.  Measured: |velocity_prev| 1.60e-13, |velocity|
    1.67e-13 m/s, rot_residual 4.1e-14 (n = 19: nineteen accumulated steps of theta against one closed-form exponential)."""
    w = np.array([0.4, -0.5, 0.3])
    T = n * DT
    S = np.zeros((n, 6))
    for k in range(n):
        Rk = R0 @ _expm(w * k * DT)
        S[k, :3] = BRS.T @ (np.cross(w, np.cross(w, ARM)) - Rk.T @ np.array(G))
        S[k, 3:] = BRS.T @ w
    R1 = R0 @ _expm(w * T)
    r = ri.reinit_velocity(oracle, _prm(oracle), np.zeros(6), S, np.full(n, DT), _T(R0, P0), _rigid_inv(_T(R1, P0)))
    e0 = np.abs(r["velocity_prev"]).max(); e1 = np.abs(r["velocity"]).max()
    print("n %d: |velocity_prev| %.2e  |velocity| %.2e  rot_residual %.2e" % (n, e0, e1, r["rot_residual"]))
    assert e0 <= FACTOR * 1.67e-13 and e1 <= FACTOR * 1.67e-13
    assert r["rot_residual"] <= FACTOR * 4.1e-14
    # the lever arm's term alone would be |w x (w x arm)| T: the bounds are far below it only because the correction removes it
    lever = np.linalg.norm(np.cross(w, np.cross(w, ARM))) * T
    print("      the lever arm's term alone: %.2e m/s" % lever)
    assert lever > 1e6 * FACTOR * 1.67e-13


def test_prediction_from_velocity_prev_lands_on_the_new_pose(oracle):
    """Affinity: predicting the same bucket from (T_prev, velocity_prev) reproduces t_new and velocity.  On a noisy bucket of the
    synthetic trajectory, between two poses that are NOT consistent with it (a perturbed second pose).  The bounds are reasoned,
    not measured (the measured figures, 1.4e-17 m and 0, are too lucky to scale): the prediction's velocity is v_i + R dV with dV
    independent of v_i - the rule's own sum, one rounding: 4 eps max(1, |v|); its position is t_i + R (dP + dt R^T v_i), i.e. the
    rule's quotient times dt through a rotation and back, a handful of roundings of values of the size of t: 16 eps max(1, |t|)."""
    S, dts, _ = synth.imu_samples(6, 8, noise_seed=3)
    bias = np.array([0.01, 0.02, -0.01, 0.001, 0.0, -0.001])
    Tp = synth.pose_at(6)
    Tn = synth.pose_at(8).copy()
    Tn[:3, 3] += np.array([0.02, -0.01, 0.015])
    prm = _prm(oracle)
    r = ri.reinit_velocity(oracle, prm, bias, S, dts, Tp, _rigid_inv(Tn))
    pim = oracle.imu_preintegrate(prm, bias, S, dts)
    sj = oracle.imu_predict(prm, pim, oracle.nav_state(Tp[:3, :3], Tp[:3, 3], r["velocity_prev"]))
    et = np.abs(sj[9:12] - Tn[:3, 3]).max(); ev = np.abs(sj[12:15] - r["velocity"]).max()
    print("dt %.4f: |t - t_new| %.2e  |v - velocity| %.2e  rot_residual %.2e" % (r["dt"], et, ev, r["rot_residual"]))
    assert r["dt"] == pytest.approx(float(np.sum(dts)), rel=1e-14)
    assert et <= 16 * EPS * max(1.0, np.abs(Tn[:3, 3]).max()) and ev <= 4 * EPS * max(1.0, np.abs(r["velocity"]).max())
    assert np.abs(r["velocity_prev"]).max() > 0.05              # (a velocity that matters: the check is not about zeros)
    assert np.abs(sj[:9] - r["pred"][:9]).max() == 0.0          # the rotation does not depend on the start velocity
