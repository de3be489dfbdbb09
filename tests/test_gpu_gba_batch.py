"""vslam_global_ba_batch: a lane's poses, landmarks, pair_wrong and report are, byte for byte, what vslam_global_ba returns for that
problem alone with the same parameters, whatever the order and company of the lanes.  The cases and the rig are those of
tests/gba_ref.py; the lanes of one call stop in different rounds (4 .. 29 trials) and differ in every size a kernel's grid or a
table offset depends on: no pair (edges only), no free keyframe (structure only), no edge, no listed block, half-bandwidths from
0 to 11, one keyframe to 261.  Two lanes are also held to the numpy restatement directly with the bounds of tests/test_gpu_gba.py.
Every refusal names its lane and leaves the sentinel-filled outputs of every lane alone."""
import functools
import struct
import numpy as np
import pytest
import gba_ref as gr
import test_gpu_gba as tg

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
FIRST = [n for n in gr.CASES if n != "rejected"]          # the lanes of the first call, in this order
SECOND = ["rejected", "one_free", "mixed"]                # the lanes of the call with gr.PARAMS["rejected"]


@functools.lru_cache(maxsize=None)
def problem(name):
    """(problem, edges) of a case: built once, never modified"""
    prob, edges = gr.CASES[name]()
    for a in prob.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return prob, edges


def lane(prob, edges=None, **kw):
    return dict(rig=prob["rig"], sigma_factor=gr.SIGMA, inv_sigma_factor=gr.INV_SIGMA, prob=prob, edges=edges, **kw)


def named(name, **kw):
    return lane(*problem(name), **kw)


def report_bytes(rep):
    ints = ("iterations", "accepted", "rejected", "n_free", "n_isolated", "n_present", "n_thin", "n_factors", "half_bandwidth")
    return struct.pack("<9i3d", *[rep[k] for k in ints], rep["initial_cost"], rep["final_cost"], rep["final_lambda"])


def same_bytes(a, b):
    return (a["kf_pose"].tobytes() == b["kf_pose"].tobytes() and a["lm"].tobytes() == b["lm"].tobytes() and
            a["pair_wrong"].tobytes() == b["pair_wrong"].tobytes() and report_bytes(a["report"]) == report_bytes(b["report"]))


_single = {}


def single(capi, name, **prm):
    """vslam_global_ba on a case, once per (case, parameters)"""
    key = (name, tuple(sorted(prm.items())))
    if key not in _single:
        _single[key] = tg.run(capi, *problem(name), **prm)
    return _single[key]


_first = []


def first_call(capi):
    """ONE call with every case but `rejected` as a lane, default parameters: {name: result}, computed once"""
    if not _first:
        _first.append(dict(zip(FIRST, capi.global_ba_batch([named(n) for n in FIRST]))))
    return _first[0]


def test_lane_equals_single_call(capi):
    got = first_call(capi)
    its = []
    for name in FIRST:
        want = single(capi, name)
        print(name, got[name]["report"])
        assert same_bytes(got[name], want), name
        its.append(got[name]["report"]["iterations"])
    # the inputs make the lanes stop in different rounds (the restatement: 4, 4, 5, 7, 22, 29, 29 trials among them)
    assert len(set(its)) >= 4, its
    reps = {n: got[n]["report"] for n in FIRST}
    assert reps["edges_only"]["n_factors"] == 0 and len(problem("edges_only")[0]["pair_kf"]) == 0          # P = 0
    assert reps["structure_only"]["n_free"] == 0 and reps["structure_only"]["accepted"] >= 1               # n_free = 0
    assert len(problem("mixed")[1]) > 0 and len(problem("one_free")[1]) == 0                                # M > 0 beside M = 0
    bs = sorted(r["half_bandwidth"] for r in reps.values() if r["n_free"] > 1)
    assert bs[0] <= 1 and bs[-1] == 11 and len(set(bs)) >= 4, bs
    # the second call: one parameter set for all, a lane with a rejected trial
    prm = gr.PARAMS["rejected"]
    got2 = capi.global_ba_batch([named(n) for n in SECOND], **prm)
    for name, g in zip(SECOND, got2):
        print(name, g["report"])
        assert same_bytes(g, single(capi, name, **prm)), name
    assert got2[0]["report"]["rejected"] >= 1


@pytest.mark.parametrize("name", ["mixed", "outliers"])
def test_lane_against_restatement(capi, name):
    """the bounds of tests/test_gpu_gba.py::test_against_restatement on a lane of the first call"""
    _, _, _, ref = tg.case(name)
    got = first_call(capi)[name]
    rep, rrep = got["report"], ref["report"]
    dp = np.abs(got["kf_pose"] - ref["kf_pose"]).max()
    dl = np.abs(got["lm"] - ref["lm"]).max()
    print(name, rep, "ref", rrep, "max pose diff", dp, "max landmark diff", dl)
    for k in ("n_free", "n_isolated", "n_present", "n_thin", "n_factors"):
        assert rep[k] == rrep[k], k
    assert (rep["accepted"], rep["rejected"]) == (rrep["accepted"], rrep["rejected"])
    assert rep["iterations"] == rep["accepted"] + rep["rejected"]
    assert abs(rep["initial_cost"] - rrep["initial_cost"]) <= 1e-9 * rrep["initial_cost"]
    assert abs(rep["final_cost"] - rrep["final_cost"]) <= 1e-9 * rrep["final_cost"]
    assert dp <= 1e-7 and dl <= 1e-7
    assert np.array_equal(got["pair_wrong"], ref["pair_wrong"])


def test_order_and_company(capi):
    base = first_call(capi)
    names = FIRST[::-1] + ["mixed"]                      # reversed, and one case in two lanes
    got = capi.global_ba_batch([named(n) for n in names])
    for name, g in zip(names, got):
        assert same_bytes(g, base[name]), name
    alone, = capi.global_ba_batch([named("outliers")])
    assert same_bytes(alone, base["outliers"])


def test_more_lanes_than_a_wave(capi):
    cyc = ["one_free", "no_shared", "mixed", "edges_only", "structure_only"]
    names = [cyc[i % 5] for i in range(70)]
    got = capi.global_ba_batch([named(n) for n in names])
    for i, (name, g) in enumerate(zip(names, got)):
        assert same_bytes(g, single(capi, name)), (i, name)


def test_per_lane_rigs(capi):
    rng = np.random.default_rng(21)
    truth = [gr.look_z(0.3 * k, 0.02 * k, 0.0, 0.01 * k) for k in range(5)]
    lm = gr.cloud(rng, 30, 0.0, 1.2)
    views = [(k, l) for l in range(30) for k in range(5) if (k + l) % 4]
    rigs = [gr.RIG, dict(gr.RIG, fx=520.0, fy=515.0, cx=300.0, cy=250.0, bl=0.2)]
    probs = [gr.make_problem(truth, [1, 0, 0, 0, 0], lm, views, 21, rig=r) for r in rigs]
    got = capi.global_ba_batch([lane(p) for p in probs])
    for p, g in zip(probs, got):
        assert g["report"]["accepted"] >= 1
        assert same_bytes(g, tg.run(capi, p))
    assert got[0]["kf_pose"].tobytes() != got[1]["kf_pose"].tobytes()


def sentinel_out(prob):
    K, L, P = len(prob["kf_pose"]), len(prob["lm"]), len(prob["pair_kf"])
    return dict(kf_pose=np.full((max(K, 1), 4, 4), np.nan), lm=np.full((max(L, 1), 3), np.nan), pair_wrong=np.full(max(P, 1), SENTINEL, np.uint8))


def untouched(out):
    return bool(np.isnan(out["kf_pose"]).all() and np.isnan(out["lm"]).all() and (out["pair_wrong"] == SENTINEL).all())


def test_idle_lane_and_in_place(capi):
    prob, _ = problem("one_free")
    empty = dict(prob, kf_pose=np.zeros((0, 4, 4)), kf_fixed=np.zeros(0, np.uint8), kf_local=np.zeros(0, np.uint8))      # n_kf == 0: idle
    out = sentinel_out(prob)
    pm, em = problem("mixed")
    mine = dict(pm, kf_pose=np.array(pm["kf_pose"], np.float64), lm=np.array(pm["lm"], np.float64))
    got = capi.global_ba_batch([named("one_free"), lane(empty, out=out), None, lane(mine, em, in_place=True)])
    assert untouched(out) and got[2] is None
    assert same_bytes(got[0], single(capi, "one_free"))
    want = single(capi, "mixed")
    assert same_bytes(got[3], want)
    assert mine["kf_pose"].tobytes() == want["kf_pose"].tobytes() and mine["lm"].tobytes() == want["lm"].tobytes()     # the problem's own arrays
    assert got[3]["report"]["accepted"] >= 1


def refused(capi, status, lanes, text=None, **prm):
    """the call is refused with `status`, the message holds every string of `text`, and no lane's sentinel-filled output is written"""
    outs = []
    for ln in lanes:
        if ln is not None and "out" not in ln:
            ln["out"] = sentinel_out(ln["prob"])
        outs.append(None if ln is None else ln["out"])
    with pytest.raises(capi.VslamError) as e:
        capi.global_ba_batch(lanes, **prm)
    assert e.value.status == status, str(e.value)
    for t in text or ():
        assert t in str(e.value), str(e.value)
    for o in outs:
        assert o is None or untouched(o)


def test_refusals(capi):
    prob, _ = problem("one_free")
    mod = lambda **kw: dict({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in prob.items()}, **kw)
    INV, CAP = capi.ERR_INVALID, capi.ERR_CAPACITY
    good = lambda: named("mixed")
    refused(capi, INV, [good(), lane(mod(kf_fixed=np.zeros(2, np.uint8))), good()], text=("lane 1", "free gauge"))
    lm = prob["lm"].copy(); lm[2, 2] = -1.0
    refused(capi, INV, [good(), good(), lane(mod(lm=lm))], text=("lane 2", "pair 4 (keyframe 0, landmark 2)"))
    lm = prob["lm"].copy(); lm[0, 0] = np.inf
    refused(capi, INV, [lane(mod(lm=lm)), good()], text=("lane 0", "non-finite"))
    refused(capi, INV, [good(), lane(prob, [(0, 1, np.eye(4) * np.nan, 1.0, 1.0)])], text=("lane 1", "edge 0"))
    refused(capi, INV, [good(), good()], max_iterations=-1)
    refused(capi, INV, [good()], lambda0=float("nan"))
    refused(capi, INV, [])
    refused(capi, CAP, [None] * 1025, text=("1025 lanes",))
    # a lane beyond the single call's own limit is named
    refused(capi, CAP, [good(), lane(tg.big(16385, 1, [0, 1], [0, 0]))], text=("lane 1", "keyframes"))
    # 17 lanes of 16 384 keyframes each (the single call's limit) on the same input arrays: 278 528 > 262 144 in all
    big = tg.big(16384, 1, [0, 1], [0, 0])
    shared = sentinel_out(big)
    refused(capi, CAP, [lane(big, out=shared) for _ in range(17)], text=("keyframes", "in all"))
    # 5 lanes of 1 048 576 landmarks each: 5 242 880 > 4 194 304 in all
    big = tg.big(2, 1048576, [0, 1], [0, 0])
    shared = sentinel_out(big)
    refused(capi, CAP, [lane(big, out=shared) for _ in range(5)], text=("landmarks", "in all"))


def test_timers_and_binding(capi):
    capi.global_ba_set_timing(True)
    try:
        got = capi.global_ba_batch([named("dense12"), None, named("edges_only")], max_iterations=3)
        t = capi.global_ba_timings()
    finally:
        capi.global_ba_set_timing(False)
    assert set(t) == {"gba_linearize", "gba_landmarks", "gba_assemble", "gba_band_chol", "gba_back", "gba_cost", "gba_chi2"}
    assert all(v >= 0 for v in t.values())
    assert got[1] is None and got[0]["report"]["accepted"] == 3 and got[0]["kf_pose"].shape == (13, 4, 4)
    assert same_bytes(got[0], tg.run(capi, *problem("dense12"), max_iterations=3))
