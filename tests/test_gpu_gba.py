"""vslam_global_ba against the numpy restatement (tests/gba_ref.py) on the shapes where the kernels can go wrong - one column, no
shared landmark (b = 0), a band as wide as the matrix, a block list across 64 and 256 entries, 172 free keyframes (the first size
the local BA refuses), 260 block columns with a loop the reordering has to absorb, the mixed and the legal special cases - and
every refusal and limit.  Tolerances are the pose-graph tests': 1e-7 absolute per pose entry and per landmark coordinate, 1e-9
relative on the initial and the final cost, the same accepted and rejected trials, equal flags; fixed, isolated and thin items bit
for bit; a second call returns the same bytes."""
import functools
import numpy as np
import pytest
import gba_ref as gr

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def case(name):
    """(problem, edges, parameters, the restatement's result): computed once, never modified"""
    prob, edges = gr.CASES[name]()
    prm = gr.PARAMS.get(name, {})
    ref = gr.optimize(prob, edges, **prm)
    for a in list(prob.values()) + [ref["kf_pose"], ref["lm"], ref["pair_wrong"]]:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return prob, edges, prm, ref


def run(capi, prob, edges=None, **prm):
    return capi.global_ba(prob["rig"], gr.SIGMA, gr.INV_SIGMA, prob, edges, **prm)


@pytest.mark.parametrize("name", list(gr.CASES))
def test_against_restatement(capi, name):
    prob, edges, prm, ref = case(name)
    got = run(capi, prob, edges, **prm)
    rep, rrep, S = got["report"], ref["report"], ref["structure"]
    dl = np.abs(got["lm"] - ref["lm"]).max() if len(ref["lm"]) else 0.0
    print(name, rep, "ref", rrep, "max pose diff", np.abs(got["kf_pose"] - ref["kf_pose"]).max(), "max landmark diff", dl,
          "flags", int(got["pair_wrong"].sum()), "margin", ref["margin"])
    for k in ("n_free", "n_isolated", "n_present", "n_thin", "n_factors"):
        assert rep[k] == rrep[k], k
    assert rep["iterations"] == rep["accepted"] + rep["rejected"]
    assert (rep["accepted"], rep["rejected"]) == (rrep["accepted"], rrep["rejected"])        # the same trials as the restatement
    assert abs(rep["initial_cost"] - rrep["initial_cost"]) <= 1e-9 * rrep["initial_cost"]
    assert abs(rep["final_cost"] - rrep["final_cost"]) <= 1e-9 * rrep["final_cost"]
    assert rep["final_lambda"] == pytest.approx(rrep["final_lambda"], rel=1e-12)
    assert np.abs(got["kf_pose"] - ref["kf_pose"]).max() <= 1e-7
    assert dl <= 1e-7
    assert np.array_equal(got["pair_wrong"], ref["pair_wrong"])
    start = np.asarray(prob["kf_pose"], np.float64)
    for k in range(len(start)):
        if S.col[k] < 0:
            assert got["kf_pose"][k].tobytes() == start[k].tobytes(), k          # fixed and isolated keyframes: not a bit
    lm0 = np.asarray(prob["lm"], np.float64)
    for l in np.flatnonzero(~S.present):
        assert got["lm"][l].tobytes() == lm0[l].tobytes(), l                       # thin landmarks: not a bit
    again = run(capi, prob, edges, **prm)
    assert again["kf_pose"].tobytes() == got["kf_pose"].tobytes() and again["lm"].tobytes() == got["lm"].tobytes()
    assert again["pair_wrong"].tobytes() == got["pair_wrong"].tobytes() and again["report"] == rep


def test_shapes_of_the_cases(capi):
    """what each case is there for"""
    rep = lambda name: run(capi, *case(name)[:2], **case(name)[2])["report"]
    r = rep("one_free")
    assert (r["n_free"], r["half_bandwidth"]) == (1, 0)
    r = rep("no_shared")
    assert r["n_free"] == 5 and r["half_bandwidth"] == 0
    r = rep("dense12")
    assert r["n_free"] == 12 and r["half_bandwidth"] == 11 and r["n_present"] == 40
    r = rep("long_list")
    assert r["n_free"] == 2 and r["half_bandwidth"] == 1 and r["n_present"] == 300
    r = rep("chain172")
    assert r["n_free"] == 172 and r["half_bandwidth"] <= 3
    # out and back: a breadth-first numbering from the far end has at most two keyframes per level side by side, each landmark
    # joins three consecutive levels of both legs: the band stays a handful of blocks although keyframes 0 and 260 share landmarks
    r = rep("chain260_loop")
    assert r["n_free"] == 260 and r["half_bandwidth"] <= 8
    r = rep("mixed")
    assert (r["n_free"], r["n_isolated"], r["n_thin"]) == (6, 1, 1)
    r = rep("edges_only")
    assert (r["n_present"], r["n_factors"], r["n_free"]) == (0, 0, 7)
    r = rep("structure_only")
    assert (r["n_free"], r["half_bandwidth"]) == (0, 0) and r["accepted"] >= 1
    r = rep("rejected")
    assert r["rejected"] >= 1 and r["accepted"] <= 2
    prob, _, _, ref = case("outliers")
    assert ref["pair_wrong"].sum() >= prob["n_bad"] // 2 and ref["margin"] > 1e-9


def test_edges_only_is_the_pose_graph_solve(capi):
    prob, edges, _, _ = case("edges_only")
    got = run(capi, prob, edges)
    out, rep = capi.pose_graph_optimize(prob["kf_pose"], prob["kf_fixed"], edges)
    assert np.abs(got["kf_pose"] - out).max() <= 1e-12
    assert (got["report"]["accepted"], got["report"]["rejected"]) == (rep["accepted"], rep["rejected"])


def test_timers(capi):
    prob, edges, _, _ = case("dense12")
    capi.global_ba_set_timing(True)
    try:
        run(capi, prob, edges)
        t = capi.global_ba_timings()
    finally:
        capi.global_ba_set_timing(False)
    assert set(t) == {"gba_linearize", "gba_landmarks", "gba_assemble", "gba_band_chol", "gba_back", "gba_cost", "gba_chi2"}
    assert all(v >= 0 for v in t.values())


def refused(capi, status, prob, edges=None, text=None, **prm):
    with pytest.raises(capi.VslamError) as e:
        run(capi, prob, edges, **prm)
    assert e.value.status == status, str(e.value)
    if text:
        assert text in str(e.value), str(e.value)


def test_refusals(capi):
    prob, _, _, _ = case("one_free")
    mod = lambda **kw: dict({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in prob.items()}, **kw)
    INV = capi.ERR_INVALID
    refused(capi, INV, prob, max_iterations=-1)
    refused(capi, INV, prob, lambda0=-1.0)
    refused(capi, INV, prob, lambda0=float("nan"))
    refused(capi, INV, mod(kf_fixed=np.zeros(2, np.uint8)), text="free gauge")
    pk = prob["pair_kf"].copy(); pk[3] = 2
    refused(capi, INV, mod(pair_kf=pk), text="pair 3")
    pl = prob["pair_lm"].copy(); pl[5] = -1
    refused(capi, INV, mod(pair_lm=pl), text="pair 5")
    po = prob["pair_oct"].copy(); po[4, 1] = 8
    refused(capi, INV, mod(pair_oct=po), text="pair 4")
    lm = prob["lm"].copy(); lm[2, 2] = -1.0                  # behind both cameras: its first pair is 4
    refused(capi, INV, mod(lm=lm), text="pair 4 (keyframe 0, landmark 2)")
    lm = prob["lm"].copy(); lm[0, 0] = np.inf
    refused(capi, INV, mod(lm=lm))
    E = np.eye(4)
    refused(capi, INV, prob, [(1, 1, E, 1.0, 1.0)], text="edge 0")
    refused(capi, INV, prob, [(0, 2, E, 1.0, 1.0)], text="edge 0")
    refused(capi, INV, prob, [(0, 1, E, -1.0, 1.0)], text="edge 0")
    refused(capi, INV, prob, [(0, 1, E * np.nan, 1.0, 1.0)], text="edge 0")
    # two free keyframes tied to each other by an edge and to nothing fixed
    prob3 = mod(kf_pose=np.concatenate([prob["kf_pose"], prob["kf_pose"][1:] @ gr.look_z(0.3), prob["kf_pose"][1:] @ gr.look_z(0.6)]),
                kf_fixed=np.array([1, 0, 0, 0], np.uint8), kf_local=np.ones(4, np.uint8))
    refused(capi, INV, prob3, [(2, 3, gr.look_z(0.3), 1.0, 1.0)], text="free gauge")
    assert run(capi, prob3, [(2, 3, gr.look_z(0.3), 1.0, 1.0), (3, 0, gr.look_z(-1.0), 1.0, 1.0)])["report"]["n_free"] == 3


def big(n_kf, n_lm, pk, pl, fixed0=True):
    fixed = np.zeros(n_kf, np.uint8)
    fixed[0] = fixed0
    P = len(pk)
    return dict(rig=gr.RIG, kf_pose=np.tile(np.eye(4), (n_kf, 1, 1)), kf_fixed=fixed, kf_local=np.ones(n_kf, np.uint8), lm=np.tile([0.0, 0.0, 3.0], (n_lm, 1)),
                pair_kf=np.asarray(pk, np.int32), pair_lm=np.asarray(pl, np.int32), pair_flags=np.full(P, 3, np.uint8),
                pair_uv=np.zeros((P, 4), np.float32), pair_oct=np.zeros((P, 2), np.int32))


def test_limits(capi):
    """VSLAM_ERR_CAPACITY, decided on the host before anything is sized or launched"""
    CAP = capi.ERR_CAPACITY
    refused(capi, CAP, big(16385, 1, [0, 1], [0, 0]), text="keyframes")
    refused(capi, CAP, big(2, 1048577, [0, 1], [0, 0]), text="landmarks")
    refused(capi, CAP, big(2, 1, np.zeros(2097153, np.int32), np.zeros(2097153, np.int32)), text="pairs")
    edges = np.zeros(262145, capi.PGO_EDGE_DTYPE)
    refused(capi, CAP, big(2, 1, [0, 1], [0, 0]), edges, text="edges")
    # one landmark seen by 4097 free keyframes: 4097^2 > 16 777 216 list entries at most
    refused(capi, CAP, big(4098, 1, np.arange(4098), np.zeros(4098, np.int32)), text="block lists")
    # one landmark seen by 600 free keyframes: every pair of them shares it, b = 599, 600 * 600 blocks > 262 144
    refused(capi, CAP, big(601, 1, np.arange(601), np.zeros(601, np.int32)), text="band")
