"""GPU parity of every launch plan of the batched local BA (vslam_local_ba_batch).  The batch picks its Schur, solve and
back-substitution kernels from the cohort's shape (largest window, slots and factors per landmark, lambda candidates); each
case here reaches a named plan, read back with vslam_local_ba_last_batch_plan, and checks
  - every lane against its own vslam_local_ba call (the bar of test_ba_batch_equals_single_calls), and
  - at least one lane against the oracle (the bar of test_gpu_ba._compare).
The plans themselves are pinned on the CPU by test_ba_plan.py."""
import numpy as np
import pytest
import synth
from test_gpu_ba import _check_batch_lane, _check_vs_oracle

pytestmark = pytest.mark.gpu


def _shape(prob):
    """vslam_ba_lane_shape of a problem's first-pass graph, counted here from the pairs"""
    fl = prob["pair_flags"].astype(np.int64) & 3
    on = fl != 0
    kf, lm, nfac = prob["pair_kf"][on], prob["pair_lm"][on], (fl[on] & 1) + (fl[on] >> 1)
    free = prob["kf_fixed"][kf] == 0
    per_lm = np.bincount(lm, weights=nfac, minlength=len(prob["lm"])).astype(np.int64)
    slots = np.bincount(np.unique(lm[free] * len(prob["kf_pose"]) + kf[free]) // len(prob["kf_pose"]), minlength=len(prob["lm"]))
    n_kf = len(np.unique(kf))
    return dict(n_free_kf=len(np.unique(kf[free])), n_points=len(np.unique(lm)), n_factors=int(nfac.sum()), n_edges=max(n_kf - 1, 0),
                n_pairs=len(prob["pair_kf"]), max_slots=max(1, int(slots.max(initial=0))), max_factors=max(1, int(per_lm.max(initial=0))))


def _run(oracle, capi, probs, oracle_lanes, lookahead=4, solver=0):
    """batch + one-problem calls of every lane; the oracle for the lanes named; returns the batch's plan, which must be the one
    vslam_local_ba_batch_plan gives for the lanes' shapes"""
    ex = oracle.Extractor(1500)
    rig = synth.RIGS["euroc"]
    batch = capi.local_ba_batch(rig, ex.sigmaFactor, ex.InvSigmaFactor, probs)
    plan = capi.local_ba_last_batch_plan()
    assert plan == capi.local_ba_batch_plan([_shape(p) for p in probs], lookahead, solver), plan
    for i, p in enumerate(probs):
        _check_batch_lane(capi.local_ba(rig, ex.sigmaFactor, ex.InvSigmaFactor, p), batch[i], (i, lookahead, solver))
    for i in oracle_lanes:
        _check_vs_oracle(oracle.local_ba(rig, ex.sigmaFactor, ex.InvSigmaFactor, probs[i]), batch[i], probs[i])
    return plan


def _kernels(plan):
    return plan["schur_kernel"], plan["schur_waves"], plan["schur_shared_w"], plan["back_kernel"], plan["back_waves"]


def test_ba_batch_plan_production_shape(oracle, capi):
    """The mapping cohort of a lockstep group: 8 tracker windows of 4-10 free keyframes, <= 12 views per landmark, outliers.
    Plan: k_ba_schur2 (8 waves) + the one-wave MFMA solve + k_ba_back2 (4 waves).  Every lane against the oracle."""
    probs = [synth.make_ba_problem(n_local=4 + (i * 5) % 7, n_fixed=1 + i % 3, n_lm=400 + 150 * i, seed=400 + i,
                                   outlier_frac=0.02 + 0.03 * (i % 3)) for i in range(8)]
    plan = _run(oracle, capi, probs, range(8))
    assert plan["status"] == 0 and (plan["n_batch"], plan["n_single"]) == (8, 0), plan
    assert _kernels(plan) == ("schur2", 8, 0, "back2", 4) and plan["solves"] == {"mfma64"}, plan
    assert plan["f_max"] == 10 and plan["max_factors"] <= 24


# F = 10 windows whose persistent landmarks are seen (left and right) by every one of K keyframes of a hovering camera:
# max_factors = 2K drives the k_ba_schur2 staging - its waves halve, k_ba_back2 halves its own (the LDS fix), then k_ba_schur
@pytest.mark.parametrize("K,plan_kernels", [
    (12, ("schur2", 8, 0, "back2", 4)),
    (50, ("schur2", 4, 0, "back2", 4)),
    (100, ("schur2", 2, 0, "back2", 4)),
    (150, ("schur2", 2, 0, "back2", 2)),
    (225, ("schur", 12, 1, "back", 8)),
])
def test_ba_batch_plan_view_ladder(oracle, capi, K, plan_kernels):
    many = synth.make_ba_problem(n_local=10, n_fixed=K - 10, n_lm=300, seed=70 + K, kf_step=0.1, n_persist=30)
    small = synth.make_ba_problem(n_local=6, n_fixed=2, n_lm=500, seed=71 + K)
    plan = _run(oracle, capi, [many, small], [0])
    assert plan["status"] == 0 and plan["n_batch"] == 2 and plan["max_factors"] == 2 * K and plan["max_slots"] == 10, plan
    assert _kernels(plan) == plan_kernels, plan
    assert plan["back_lds"] <= 160 * 1024 and plan["schur_lds"] <= 160 * 1024


# (F, lookahead) -> Schur kernel, waves, shared W staging with the MFMA solves; k_ba_back (8 waves) beyond tracker windows
WINDOW_PLANS = {
    (10, 1): ("schur2", 8, 0), (10, 2): ("schur2", 8, 0), (10, 4): ("schur2", 8, 0),
    (11, 1): ("schur", 16, 0), (11, 2): ("schur", 16, 1), (11, 4): ("schur", 2, 1),
    (12, 1): ("schur", 16, 0), (12, 2): ("schur", 16, 1), (12, 4): ("schur", 16, 0),
    (14, 1): ("schur", 16, 0), (14, 2): ("schur", 8, 1), (14, 4): ("schur", 16, 0),
    (16, 1): ("schur", 16, 0), (16, 2): ("schur", 16, 0), (16, 4): ("schur", 16, 0),
    (20, 1): ("schur", 4, 0), (20, 2): ("schur", 4, 0), (20, 4): ("schur", 4, 0),
}


@pytest.mark.parametrize("F", [10, 11, 12, 14, 16, 20])
def test_ba_batch_plan_window_ladder(oracle, capi, F):
    """Each window size as its own cohort (next to a 4-keyframe window of test_ba_batch_equals_single_calls), with 1 / 2 / 4 lambda candidates and with the MFMA and
    the wave / LDS solves: shared and per-candidate W staging of k_ba_schur, the MFMA-64, MFMA and wave solves; with the wave
    solves a window beyond 60 unknowns goes to the one-problem path.  Persistent landmarks make max_slots = F."""
    big = synth.make_ba_problem(n_local=F, n_fixed=2, n_lm=700, seed=500 + F, n_persist=8, outlier_frac=0.05)
    small = synth.make_ba_problem(n_local=4, n_fixed=2, n_lm=400, seed=32)
    try:
        for solver in (0, 1):
            capi.local_ba_set_solver(solver)
            for nb in (1, 2, 4):
                capi.local_ba_set_lookahead(nb, -1, 1)
                plan = _run(oracle, capi, [big, small], [0] if (solver, nb) == (0, 4) else [], nb, solver)
                assert plan["status"] == 0 and plan["lookahead"] == nb, (solver, nb, plan)
                if solver == 0 or F <= 10:
                    assert plan["max_slots"] == F and plan["f_max"] == F, plan
                if solver == 0:
                    assert (plan["n_batch"], plan["n_single"]) == (2, 0), plan
                    assert _kernels(plan)[:3] == WINDOW_PLANS[(F, nb)], (nb, plan)
                    assert plan["solves"] == ({"mfma64"} if F <= 10 else {"mfma64", "mfma"}), plan
                    if F > 10:
                        assert (plan["back_kernel"], plan["back_waves"], plan["back_shared"]) == ("back", 8, int(nb > 1)), plan
                else:
                    assert (plan["n_batch"], plan["n_single"]) == ((2, 0) if F <= 10 else (1, 1)), plan
                    assert _kernels(plan) == ("schur2", 8, 0, "back2", 4) and plan["solves"] == {"wave"}, plan
    finally:
        capi.local_ba_set_lookahead(0, -1, 1)
        capi.local_ba_set_solver(-1)


def test_ba_batch_plan_ragged_cohort(oracle, capi):
    """Lanes of very different size in one cohort: 3000 landmarks next to 5-landmark windows, an empty graph, and a 20-keyframe
    window next to a 21-keyframe one (the one-problem path inside the call, like the empty graph)."""
    probs = [synth.make_ba_problem(n_local=10, n_fixed=3, n_lm=3000, seed=801),
             synth.make_ba_problem(n_local=3, n_fixed=1, n_lm=0, seed=802, n_persist=5),
             synth.make_ba_problem(n_local=5, n_fixed=2, n_lm=0, seed=803, n_persist=5),
             synth.make_ba_problem(n_local=20, n_fixed=2, n_lm=900, seed=804),
             synth.make_ba_problem(n_local=21, n_fixed=2, n_lm=900, seed=805)]
    empty = synth.make_ba_problem(n_local=3, n_fixed=1, n_lm=40, seed=806)
    for k in ("pair_kf", "pair_lm", "pair_flags", "pair_uv", "pair_oct"):
        empty[k] = empty[k][:0]
    probs.append(empty)
    plan = _run(oracle, capi, probs, [0, 3])
    assert plan["status"] == 0 and (plan["n_batch"], plan["n_single"]) == (4, 2), plan
    assert plan["f_max"] == 20 and plan["lp_max"] > 2500 and plan["solves"] == {"mfma64", "mfma"}, plan
    assert plan["schur_kernel"] == "schur" and plan["back_kernel"] == "back", plan
