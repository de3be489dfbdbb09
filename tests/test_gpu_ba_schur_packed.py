"""GPU parity of k_ba_schur2's packed accumulator (upper 6x6 blocks only, gtsam-vslam_amd/csrc/ba_packed.hpp) and of k_ba_reduce
summing packed partials.  Every case is a small cohort that must run k_ba_schur2; every lane is checked against its own
vslam_local_ba call (k_ba_schur, row-major - the independent form inside the project) and one lane against the oracle."""
import pytest
import synth
from test_gpu_ba_plans import _run

pytestmark = pytest.mark.gpu


def _schur2(plan, n_batch):
    assert plan["status"] == 0 and (plan["n_batch"], plan["n_single"]) == (n_batch, 0), plan
    assert plan["schur_kernel"] == "schur2" and plan["back_kernel"] == "back2", plan


def test_packed_per_lane_system_sizes(oracle, capi):
    """F = 1, 2, 3 and 10 in one launch: each lane packs with its own F (a single block at F = 1), not the cohort's largest."""
    probs = [synth.make_ba_problem(n_local=1, n_fixed=2, n_lm=60, seed=901),
             synth.make_ba_problem(n_local=2, n_fixed=2, n_lm=120, seed=902),
             synth.make_ba_problem(n_local=3, n_fixed=1, n_lm=200, seed=903),
             synth.make_ba_problem(n_local=10, n_fixed=3, n_lm=300, seed=904)]
    plan = _run(oracle, capi, probs, [3])
    _schur2(plan, 4)
    assert plan["f_max"] == 10
    # the LDS asked for: the packed system (55 blocks of 37 + 60 doubles, rounded to even: 2 096, not the 3 660 row-major) and a
    # staging region per landmark-wave (ba2_stage_doubles)
    fac, slots = plan["max_factors"], plan["max_slots"]
    ints = fac + 2 * (slots + 1)
    stage = ((fac * 20 + 2 * slots * 18 + 10 + (ints + 1) // 2) + 1) & ~1
    assert plan["schur_lds"] == 8 * (2096 + plan["schur_waves"] * stage), plan


@pytest.mark.parametrize("lookahead", [1, 2, 4])
@pytest.mark.parametrize("max_views", [4, 5])
def test_packed_bench_like_views(oracle, capi, max_views, lookahead):
    """The headline run's shape (about 5 factors and 3 slots per landmark: max_views 4 and 5 bracket it) with 1, 2 and 4 lambda
    candidates - a partial set and a reduce per candidate."""
    probs = [synth.make_ba_problem(n_local=10, n_fixed=4, n_lm=400, seed=910 + max_views, max_views=max_views),
             synth.make_ba_problem(n_local=6, n_fixed=2, n_lm=150, seed=920 + max_views, max_views=max_views)]
    try:
        capi.local_ba_set_lookahead(lookahead, -1, 1)
        plan = _run(oracle, capi, probs, [0], lookahead)
    finally:
        capi.local_ba_set_lookahead(0, -1, 1)
    _schur2(plan, 2)
    assert plan["lookahead"] == lookahead and plan["f_max"] == 10, plan


def test_packed_all_55_blocks(oracle, capi):
    """Persistent landmarks seen by all 10 free keyframes touch every block of the triangle: the block phase takes two passes
    (32 + 23 blocks)."""
    probs = [synth.make_ba_problem(n_local=10, n_fixed=2, n_lm=200, seed=930, n_persist=6),
             synth.make_ba_problem(n_local=4, n_fixed=2, n_lm=100, seed=931)]
    plan = _run(oracle, capi, probs, [0])
    _schur2(plan, 2)
    assert plan["max_slots"] == 10, plan


def test_packed_first_and_last_free_index(oracle, capi):
    """Two free keyframes among eight fixed ones: landmarks without any free slot, and slots only at the first or the last free
    index (blocks (0,0), (0,1), (1,1))."""
    probs = [synth.make_ba_problem(n_local=2, n_fixed=8, n_lm=300, seed=940),
             synth.make_ba_problem(n_local=2, n_fixed=8, n_lm=200, seed=941, max_views=4)]
    plan = _run(oracle, capi, probs, [0])
    _schur2(plan, 2)
    assert plan["f_max"] == 2, plan


def test_packed_one_partial(oracle, capi, monkeypatch):
    """One workgroup per lane: one partial holds the whole system."""
    monkeypatch.setenv("VSLAM_BA_LMBLOCKS", "1")
    probs = [synth.make_ba_problem(n_local=10, n_fixed=3, n_lm=300, seed=950),
             synth.make_ba_problem(n_local=5, n_fixed=2, n_lm=200, seed=951)]
    plan = _run(oracle, capi, probs, [0])
    _schur2(plan, 2)
    assert plan["schur_blocks"] == 1, plan


def test_packed_partials_of_idle_workgroups(oracle, capi, monkeypatch):
    """64 workgroups of 8 landmark-waves per lane (the cohort's largest lane sets the grid): the 100-landmark lane leaves most of
    its workgroups without a landmark, and they flush zeros that the reduce sums."""
    monkeypatch.setenv("VSLAM_BA_LMBLOCKS", "64")
    probs = [synth.make_ba_problem(n_local=10, n_fixed=3, n_lm=1250, seed=952),
             synth.make_ba_problem(n_local=10, n_fixed=3, n_lm=100, seed=953)]
    plan = _run(oracle, capi, probs, [1])
    _schur2(plan, 2)
    assert plan["schur_blocks"] == 64 and plan["schur_waves"] == 8 and plan["lp_max"] > 1024, plan


@pytest.mark.parametrize("layout", [0, 1])
def test_row_major_layout_switch(oracle, capi, monkeypatch, layout):
    """The developer forms of the same kernel body: row-major with pitch n (0) and n + 1 (1), partials and reduce row-major."""
    monkeypatch.setenv("VSLAM_BA_SCHUR2_LAYOUT", str(layout))
    probs = [synth.make_ba_problem(n_local=10, n_fixed=3, n_lm=300, seed=960, n_persist=3),
             synth.make_ba_problem(n_local=3, n_fixed=1, n_lm=150, seed=961, max_views=4)]
    plan = _run(oracle, capi, probs, [0])
    _schur2(plan, 2)
