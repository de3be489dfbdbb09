"""GPU pre-integration (k_imu_preintegrate / k_imu_preintegrate_b through the vslam_imu_preintegrate[_batch] test taps,
which stage and launch a bucket exactly as a pose solve does) against the oracle's restatement and against references
computed here (numpy, mpmath).  Every field is compared: deltaTij, preint (theta, position, velocity), H_biasAcc,
H_biasOmega, the 15x15 covariance, the information matrix Lam and the predicted state.

Shapes and the branch each one exists to reach:
  n = 1, 2, 11, 12          one partial / one full chunk of PIM_CHUNK = 12 samples (no carry between chunks)
  n = 13, 23..25, 37, 100,  the chunk boundary: the state, covariance and bias Jacobians carried from one chunk into
      200, 201, 400, 2000   the next (n = 24 ends exactly on a boundary, 13 / 25 / 37 / 201 one sample past one)
  gyro exactly 0            the nearZero branches of so3_expmap / dexp_apply_inv on the device
  |w| T = 3 rad             fast rotation: the tangent integrator far from its small-angle regime
  jittered timestamps       the host dt rule of imu_stage (next timestamp, last sample reuses the previous dt) on
                            irregular spacing with a 3x gap
  batch, n = 9/0/1/12/13/200  k_imu_preintegrate_b: a different n per lane, an idle lane (n = 0, early return, outputs
                            untouched) and the takeFrom bias hand-over of the rechained pre-integration
"""
import numpy as np
import pytest
import synth

pytestmark = pytest.mark.gpu
G = (0.0, 9.81, 0.0)
NOISE = (1.6968e-4, 1.9393e-5, 2.0e-3, 3.0e-3)      # gyro density, gyro walk, acc density, acc walk
HZ = 200
SAMPLE_BIAS = np.array([0.03, -0.02, 0.05, 0.004, -0.003, 0.002])      # bias in the synthetic measurements
BIAS_HAT = np.array([0.02, -0.01, 0.03, 0.001, -0.002, 0.0015])         # integration bias (bias_prev)
SWEEP = (1, 2, 11, 12, 13, 23, 24, 25, 37, 100, 201, 400)
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def m(capi):
    rig = synth.RIGS["euroc"]
    ge = capi.Extractor(rig["w"], rig["h"], 1500, batch=2)
    return capi.Matcher(rig, ge, 0, ge, 1)


def _dts(ts):
    """the reference's dt rule: dt_i = t_{i+1} - t_i, the last sample reuses the previous dt, a single sample 1 / hz"""
    d, dt = np.empty(len(ts)), 1.0 / HZ
    for i in range(len(ts)):
        if i + 1 < len(ts):
            dt = (ts[i + 1] - ts[i]) / 1e9
        d[i] = dt
    return d


def _bucket(n, f0=10, seed=7):
    """n noisy, biased samples of the synthetic trajectory from frame f0 on (longer spans for longer buckets)"""
    S, _, _ = synth.imu_samples(f0, f0 + n // 10 + 1, noise_seed=seed, bias=SAMPLE_BIAS)
    assert len(S) >= n
    return S[:n]


def _state(f0):
    T = synth.pose_at(f0)
    h = 1e-4
    v = (synth.pose_at(f0 + h * 20)[:3, 3] - synth.pose_at(f0 - h * 20)[:3, 3]) / (2 * h)
    return T, v


def _gpu(capi, m, S, ts, bias, T_prev, v_prev, T_bs=synth.T_BC1):
    return capi.imu_preintegrate(m, G, NOISE, T_bs, T_prev, v_prev, bias, S[:, :3], S[:, 3:], ts, HZ)


def _ref(oracle, S, dts, bias, T_prev, v_prev, T_bs=synth.T_BC1):
    prm = oracle.imu_params(G, NOISE[0], NOISE[2], NOISE[1], NOISE[3], T_bs)
    pim = oracle.imu_preintegrate(prm, bias, S, dts)
    return pim, oracle.imu_predict(prm, pim, oracle.nav_state(T_prev[:3, :3], T_prev[:3, 3], v_prev))


def _parity(pim, pred, rpim, rpred, what):
    """deltaTij, preint, H_biasAcc, H_biasOmega, biasHat and the prediction within 1e-12 * max(1, |ref|) per entry; the
    covariance within 1e-12 * max|cov|"""
    for sl, name in ((slice(0, 64), "deltaTij/preint/Hba/Hbg"), (slice(289, 295), "biasHat")):
        err = np.abs(pim[sl] - rpim[sl]) / np.maximum(1.0, np.abs(rpim[sl]))
        assert err.max() <= 1e-12, (what, name, int(np.argmax(err)), err.max())
    err = np.abs(pred - rpred) / np.maximum(1.0, np.abs(rpred))
    assert err.max() <= 1e-12, (what, "prediction", int(np.argmax(err)), err.max())
    C, Cr = pim[64:289], rpim[64:289]
    assert np.abs(C - Cr).max() <= 1e-12 * np.abs(Cr).max(), (what, "cov", np.abs(C - Cr).max() / np.abs(Cr).max())


def _check_information(pim, Lam, what):
    """Lam against the inverse of the GPU's own covariance at 50 digits (mpmath).  The covariance is badly scaled (its
    2-norm condition number is 1e9..1e12, almost all of it from the units of its blocks), and a Cholesky-based inverse
    is insensitive to diagonal scaling (van der Sluis), so the bar uses the condition number k of the equilibrated
    matrix D^-1/2 cov D^-1/2: per entry |Lam_ij - inv_ij| <= 2 N k eps sqrt(inv_ii inv_jj), N = 15.  The bar is
    asserted to be far below 1, so an all-zero, a wrong-column or an unsymmetric Lam misses it by orders of magnitude."""
    import mpmath
    C = pim[64:289].reshape(15, 15)
    assert np.isfinite(C).all() and np.isfinite(Lam).all(), what
    assert np.abs(C - C.T).max() <= 1e-13 * np.abs(C).max(), (what, "cov not symmetric")
    assert np.linalg.eigvalsh(C).min() > 0, (what, "cov not positive definite")
    d = 1.0 / np.sqrt(np.diag(C))
    k = np.linalg.cond(C * d[:, None] * d[None, :])
    with mpmath.workdps(50):
        inv = mpmath.matrix(C.tolist()) ** -1
        ref = np.array([[float(inv[i, j]) for j in range(15)] for i in range(15)])
    tol = 2 * 15 * k * EPS
    assert tol < 1e-6, (what, "equilibrated cov too ill-conditioned for a meaningful bar", k)
    scale = np.sqrt(np.outer(np.diag(ref), np.diag(ref)))
    assert np.abs(Lam).max() > 0, (what, "Lam all zero: the information matrix was not formed")
    err = (np.abs(Lam - ref) / scale).max()
    assert err <= tol, (what, "Lam vs 50-digit inverse", err, tol, k)
    assert (np.abs(Lam - Lam.T) / scale).max() <= tol, (what, "Lam not symmetric")


@pytest.mark.parametrize("n", SWEEP)
def test_preintegration_sweep_parity_and_information(oracle, capi, m, n):
    S = _bucket(n)
    ts = np.arange(n) * 5e6
    T_prev, v_prev = _state(10)
    pim, Lam, pred = _gpu(capi, m, S, ts, BIAS_HAT, T_prev, v_prev)
    rpim, rpred = _ref(oracle, S, _dts(ts), BIAS_HAT, T_prev, v_prev)
    assert pim[0] == pytest.approx(n / HZ, rel=1e-13)
    _parity(pim, pred, rpim, rpred, n)
    _check_information(pim, Lam, n)


@pytest.mark.parametrize("n,gap_at", [(25, 13), (37, 11), (201, 120)])
def test_preintegration_irregular_timestamps(oracle, capi, m, n, gap_at):
    """+-0.5 ms jitter on 5 ms spacing plus one 3x gap: the oracle gets the dts the reference rule derives from the
    timestamps; deltaTij is their (sequential) sum."""
    rng = np.random.default_rng(n)
    steps = 5_000_000 + rng.integers(-500_000, 500_001, n - 1)
    steps[gap_at] = 15_000_000
    ts = (5_000_000_000 + np.concatenate([[0], np.cumsum(steps)])).astype(np.float64)
    dts = _dts(ts)
    assert len(set(dts.tolist())) > n // 2 and dts.max() > 2.5 * dts.min()
    S = _bucket(n, seed=11)
    T_prev, v_prev = _state(10)
    pim, Lam, pred = _gpu(capi, m, S, ts, BIAS_HAT, T_prev, v_prev)
    rpim, rpred = _ref(oracle, S, dts, BIAS_HAT, T_prev, v_prev)
    _parity(pim, pred, rpim, rpred, ("jitter", n))
    tot = 0.0
    for d in dts:
        tot += d
    assert abs(pim[0] - tot) <= 1e-15 * tot * n
    _check_information(pim, Lam, ("jitter", n))


def _expm(w):
    th = np.linalg.norm(w)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + W if th < 1e-12 else np.eye(3) + np.sin(th) / th * W + (1 - np.cos(th)) / th ** 2 * W @ W


def test_preintegration_constant_motion_first_principles(capi, m):
    """Identity sensor pose, constant body rate and specific force (2000 samples at 2 kHz, 167 chunks): theta = w T
    exactly (the tangent integrator is exact for a constant rate), velocity / position against fine quadrature of
    R(w t) a (as the oracle's own test does)."""
    w = np.array([0.3, -0.2, 0.5]); a = np.array([0.4, 9.6, -0.7])
    n = 2000
    S = np.tile(np.concatenate([a, w]), (n, 1))
    ts = np.arange(n) * 5e5
    pim, Lam, pred = _gpu(capi, m, S, ts, np.zeros(6), np.eye(4), np.zeros(3), T_bs=np.eye(4))
    T = n * 5e-4
    assert abs(pim[0] - T) < 1e-12
    assert np.abs(pim[1:4] - w * T).max() < 1e-12
    K = 20000
    tq = (np.arange(K) + 0.5) * (T / K)
    Ra = np.array([_expm(w * t) @ a for t in tq])
    vel = Ra.sum(0) * (T / K)
    pos = np.cumsum(Ra * (T / K), 0).sum(0) * (T / K)
    assert np.abs(pim[7:10] - vel).max() < 2e-3 and np.abs(pim[4:7] - pos).max() < 2e-3
    C = pim[64:289].reshape(15, 15)
    assert np.abs(C - C.T).max() <= 1e-13 * np.abs(C).max() and np.linalg.eigvalsh(C).min() > 0


@pytest.mark.parametrize("n", [1, 12, 25])
def test_preintegration_stationary_near_zero(oracle, capi, m, n):
    """A resting IMU (gyro exactly 0, specific force -g in the body frame, identity sensor pose): theta stays exactly 0
    (the nearZero branches), the measured velocity / position increments are -g T and -g T^2 / 2, the prediction from
    rest is rest; no NaN / Inf anywhere, cov symmetric positive definite; parity with the oracle."""
    T_prev, _ = _state(10)
    R = T_prev[:3, :3]
    f = R.T @ -np.asarray(G)
    S = np.tile(np.concatenate([f, np.zeros(3)]), (n, 1))
    ts = np.arange(n) * 5e6
    pim, Lam, pred = _gpu(capi, m, S, ts, np.zeros(6), T_prev, np.zeros(3), T_bs=np.eye(4))
    assert np.isfinite(pim).all() and np.isfinite(Lam).all() and np.isfinite(pred).all()
    T = n / HZ
    assert np.abs(pim[1:4]).max() == 0.0
    assert np.abs(pim[7:10] - f * T).max() < 1e-12 and np.abs(pim[4:7] - 0.5 * f * T * T).max() < 1e-12
    assert np.abs(pred[:9] - R.ravel()).max() < 1e-12
    assert np.abs(pred[9:12] - T_prev[:3, 3]).max() < 1e-12 and np.abs(pred[12:15]).max() < 1e-12
    rpim, rpred = _ref(oracle, S, _dts(ts), np.zeros(6), T_prev, np.zeros(3), T_bs=np.eye(4))
    _parity(pim, pred, rpim, rpred, ("stationary", n))
    _check_information(pim, Lam, ("stationary", n))


def test_bias_jacobians_central_differences_of_the_gpu(capi, m):
    """H_biasAcc / H_biasOmega of the GPU against central differences of the GPU tap itself (bias +- h), n = 37."""
    n = 37
    S = _bucket(n, seed=5)
    ts = np.arange(n) * 5e6
    T_prev, v_prev = _state(10)
    pim0, _, _ = _gpu(capi, m, S, ts, BIAS_HAT, T_prev, v_prev)
    Hba, Hbg = pim0[10:37].reshape(9, 3), pim0[37:64].reshape(9, 3)
    h = 1e-6
    for k in range(6):
        e = np.zeros(6); e[k] = h
        fp = _gpu(capi, m, S, ts, BIAS_HAT + e, T_prev, v_prev)[0][1:10]
        fm = _gpu(capi, m, S, ts, BIAS_HAT - e, T_prev, v_prev)[0][1:10]
        num = (fp - fm) / (2 * h)
        ana = Hba[:, k] if k < 3 else Hbg[:, k - 3]
        assert np.abs(num - ana).max() < 1e-6, (k, num, ana)
    assert np.abs(Hba).max() > 1e-3 and np.abs(Hbg).max() > 1e-3


def test_fast_rotation(oracle, capi, m):
    """|w| = 3 rad/s over a 1 s bucket (n = 200): the integrated angle is 3 rad, close to pi.  theta = w T; parity with
    the oracle (sensor pose T_bc1, constant specific force)."""
    w = np.array([1.0, 2.0, -2.0])          # |w| = 3
    a = np.array([0.5, -9.7, 1.2])
    n = 200
    S = np.tile(np.concatenate([a, w]), (n, 1))
    ts = np.arange(n) * 5e6
    pim, Lam, pred = _gpu(capi, m, S, ts, np.zeros(6), np.eye(4), np.zeros(3), T_bs=np.eye(4))
    assert np.abs(pim[1:4] - w * 1.0).max() < 1e-12
    T_prev, v_prev = _state(10)
    S2 = S + SAMPLE_BIAS
    pim, Lam, pred = _gpu(capi, m, S2, ts, BIAS_HAT, T_prev, v_prev)
    rpim, rpred = _ref(oracle, S2, _dts(ts), BIAS_HAT, T_prev, v_prev)
    _parity(pim, pred, rpim, rpred, "fast")
    assert 2.9 < np.linalg.norm(pim[1:4]) < 3.1
    _check_information(pim, Lam, "fast")


def test_batched_lanes_equal_single_lane_tap(capi, m):
    """One k_imu_preintegrate_b launch with lanes of n = 9, 0 (idle), 1, 12 (takeFrom: the bias of a solve's io block
    becomes the integration bias on the device), 13 and 200: every active lane equals the single-lane tap bit for bit
    (the same device function); the idle lane's outputs keep the sentinel."""
    ns = [9, 0, 1, 12, 13, 200]
    sentinel = -7.25
    args, single_bias = [], []
    for b, n in enumerate(ns):
        S = _bucket(max(n, 1), f0=10 + 3 * b, seed=20 + b)[:n]
        ts = np.arange(n) * 5e6
        T_prev, v_prev = _state(10 + 3 * b)
        bias = BIAS_HAT * (1 + 0.1 * b)
        args.append((G, NOISE, synth.T_BC1, T_prev, v_prev, bias, S[:, :3], S[:, 3:], ts, HZ))
        single_bias.append(bias)
    io = [None] * len(ns)
    io[3] = np.concatenate([[0.1, -0.2, 0.3], BIAS_HAT * -0.5])
    single_bias[3] = io[3][3:]
    pim, Lam, pred = capi.imu_preintegrate_batch(m, args, solve_io=io, fill=sentinel)
    assert (pim[1] == sentinel).all() and (Lam[1] == sentinel).all() and (pred[1] == sentinel).all()
    for b, n in enumerate(ns):
        if n == 0:
            continue
        a = list(args[b]); a[5] = single_bias[b]
        p1, L1, r1 = capi.imu_preintegrate(m, *a)
        assert np.array_equal(pim[b], p1) and np.array_equal(Lam[b], L1) and np.array_equal(pred[b], r1), (b, n)
        assert np.array_equal(pim[b][289:295], single_bias[b]), b
    with pytest.raises(capi.VslamError):          # a pose solve still rejects an empty bucket
        capi.imu_preintegrate(m, *args[1])
