"""vslam_pose_graph_optimize_yaw / _batch against the numpy restatement (tests/pgo_yaw_ref.py) on the shapes where the 4x4 kernels
can go wrong: 1, 2, 3, 4 and 7 free poses (three block columns per wave: remainders 1, 2, 0, 1 and a second wave; the columns of
a ring have incidence lists of different lengths), no free-free edge (b = 0), a band as wide as the matrix and wider than the
back substitution's parts, a chain of 300 (several workgroups, a chord that the reordering absorbs), a hub (b >= 25), a tilted
and an un-normalised axis, the legal special cases and every refusal of the 6-DoF call plus those of the axis.
Tolerances are those of tests/test_gpu_pgo.py, for the same reasons: 1e-7 absolute per pose entry, 1e-9 relative on the costs,
the same trials as the restatement, |J4^T W r|_inf <= 1e-6 of its initial value evaluated by the restatement."""
import ctypes as C
import functools
import numpy as np
import pytest
import pgo_ref as pr
import pgo_yaw_ref as py

pytestmark = pytest.mark.gpu

Y = (0.0, 1.0, 0.0)
TILTED = (0.3, -2.0, 0.5)
SENTINEL = 0xA5


def hub_graph():
    return pr.star_graph(51, seed=13, hub_fixed=False)           # pose 0 free with 100 edges (two per neighbour), pose 1 fixed


def special_graph():
    poses, fixed, edges = pr.chain_graph(12, (2, 9), fixed_ids=(0, 5))
    poses = np.concatenate([poses, poses[-1:] @ pr.make_pose(np.eye(3), [1.0, 0, 0])])      # pose 12: free, no edge
    fixed = np.concatenate([fixed, [0]]).astype(np.uint8)
    edges = edges + [(0, 5, np.eye(4), 2.0, 3.0)] + edges[3:6] + [(8, 7, pr.rigid_inv(np.asarray(edges[7][2])), 0.5, 0.0)]
    return poses, fixed, edges


GRAPHS = {
    "free1": lambda: pr.ring_graph(2, 2),
    "free2": lambda: pr.ring_graph(3, 3),
    "free3": lambda: pr.ring_graph(4, 4),
    "free4": lambda: pr.ring_graph(5, 5),
    # (free7 and star: other seeds than the 6-DoF file's 8 and 11.  The solve converges quadratically, so the last trials of a run
    # change the cost near its rounding error, and with those seeds the last bits decide how many trials there are: ring 8 ends
    # in rejected trials whose |delta|_inf sits at the 1e-12 stop (2 in numpy, 1 on the device, poses 1.3e-12 apart), star 11 has
    # a third trial that lowers the cost by 1.2e-15 of it, 5 units in its last place (accepted at once in numpy, after three
    # repeats on the device, poses 7e-13 apart).  "The same trials" needs graphs whose every accepted trial gains more than
    # the noise of the cost's sum: here the smallest gain is 4e-15 of the cost (free4) and the star's is 1.3e-14)
    "free7": lambda: pr.ring_graph(8, 7),
    "star": lambda: pr.star_graph(9, seed=16),
    "complete12": pr.complete_graph,
    "chain300": lambda: pr.chain_graph(300, (3, 290)),
    "hub100": hub_graph,
    "special": special_graph,
}
CASES = [(nm, "y") for nm in GRAPHS] + [("free7", "tilted"), ("complete12", "tilted"), ("hub100", "tilted")]
AXES = {"y": Y, "tilted": TILTED}


@functools.lru_cache(maxsize=None)
def graph(name):
    poses, fixed, edges = GRAPHS[name]()
    poses.setflags(write=False)
    fixed.setflags(write=False)
    return poses, fixed, edges


@functools.lru_cache(maxsize=None)
def case(name, axis):
    """(poses, fixed, edges, reference poses, reference report, initial gradient): computed once, never modified"""
    poses, fixed, edges = graph(name)
    ref, rep = py.optimize(poses, fixed, edges, AXES[axis])
    ref.setflags(write=False)
    return poses, fixed, edges, ref, rep, py.gradient_inf(poses, fixed, edges, AXES[axis])


@pytest.mark.parametrize("name,axis", CASES)
def test_against_restatement(capi, name, axis):
    poses, fixed, edges, ref, rrep, g0 = case(name, axis)
    g = py.unit_axis(AXES[axis])
    out, rep = capi.pose_graph_optimize_yaw(poses, fixed, edges, AXES[axis])
    grad = py.gradient_inf(out, fixed, edges, AXES[axis])
    print(name, axis, rep, "ref", rrep, "max pose diff", np.abs(out - ref).max(), "gradient", grad, "of", g0)
    assert rep["n_free"] == rrep["n_free"] and rep["n_isolated"] == rrep["n_isolated"]
    assert rep["iterations"] == rep["accepted"] + rep["rejected"] and 1 <= rep["accepted"] <= 20
    assert (rep["accepted"], rep["rejected"]) == (rrep["accepted"], rrep["rejected"])        # the same trials as the restatement
    assert abs(rep["initial_cost"] - rrep["initial_cost"]) <= 1e-9 * rrep["initial_cost"]
    assert np.abs(out - ref).max() <= 1e-7
    assert abs(rep["final_cost"] - rrep["final_cost"]) <= 1e-9 * rrep["final_cost"]
    assert grad <= 1e-6 * g0
    free, _ = pr.free_poses(len(poses), fixed, edges)
    for k in range(len(poses)):
        if k not in free:
            assert out[k].tobytes() == poses[k].tobytes(), k         # fixed and isolated poses: not a bit
        dR = out[k][:3, :3] @ poses[k][:3, :3].T
        assert np.abs(dR @ g - g).max() <= 1e-12, k                  # roll and pitch about the axis: untouched
    # two calls on the same input return the same bytes
    out2, rep2 = capi.pose_graph_optimize_yaw(poses, fixed, edges, AXES[axis])
    assert out2.tobytes() == out.tobytes() and rep2 == rep


def test_bandwidths_and_6dof_comparison(capi):
    rep = {nm: capi.pose_graph_optimize_yaw(*graph(nm), Y)[1] for nm in ("star", "free1", "complete12", "chain300", "hub100")}
    assert rep["star"]["half_bandwidth"] == 0 and rep["free1"]["half_bandwidth"] == 0
    assert rep["complete12"]["half_bandwidth"] == 10
    assert rep["chain300"]["n_free"] == 299 and rep["chain300"]["half_bandwidth"] <= 5
    assert rep["hub100"]["n_free"] == 50 and rep["hub100"]["half_bandwidth"] >= 25
    # the same host numbering as the 6-DoF call, and never a lower final cost than it reaches
    for nm in ("free7", "chain300"):
        r6 = capi.pose_graph_optimize(*graph(nm))[1]
        r4 = capi.pose_graph_optimize_yaw(*graph(nm), Y)[1]
        assert (r4["n_free"], r4["half_bandwidth"], r4["initial_cost"]) == (r6["n_free"], r6["half_bandwidth"], r6["initial_cost"])
        assert r4["final_cost"] >= r6["final_cost"]


def test_unnormalised_axis_returns_the_same_bytes(capi):
    """The library divides the axis by sqrt(x^2 + y^2 + z^2) in fp64 whatever its length.  Three cases in which that division
    provably gives the same unit axis, hence the SAME BYTES: (0, 3, 0) against (0, 1, 0) (sqrt(9) = 3 and 3 / 3 = 1 exactly);
    an axis against four times itself (a power of two scales squares, sum, root and quotient exactly); and TILTED against its
    own unit axis as numpy computes it with the library's expression - normalising a unit axis again may move its last bit in
    general, so the test first checks that for this axis it does not (the same IEEE operations as the host code)."""
    poses, fixed, edges = graph("free7")
    want = capi.pose_graph_optimize_yaw(poses, fixed, edges, Y)
    got = capi.pose_graph_optimize_yaw(poses, fixed, edges, (0.0, 3.0, 0.0))
    assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1]
    want = capi.pose_graph_optimize_yaw(poses, fixed, edges, TILTED)
    got = capi.pose_graph_optimize_yaw(poses, fixed, edges, tuple(4.0 * v for v in TILTED))
    assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1]
    unit = py.unit_axis(TILTED)
    assert py.unit_axis(unit).tobytes() == unit.tobytes()
    got = capi.pose_graph_optimize_yaw(poses, fixed, edges, unit)
    assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1]


def test_special_cases(capi):
    poses, fixed, edges, ref, rrep, _ = case("special", "y")
    out, rep = capi.pose_graph_optimize_yaw(poses, fixed, edges, Y)
    assert rep["n_isolated"] == 1 and rep["n_free"] == 10
    assert out[12].tobytes() == poses[12].tobytes()                  # the isolated pose
    # exact measurements: zero iterations
    p, f, e = pr.exact_graph()
    out, rep = capi.pose_graph_optimize_yaw(p, f, e, TILTED)
    assert rep["initial_cost"] <= 1e-20 and rep["iterations"] == 0 and out.tobytes() == p.tobytes()
    # all poses fixed
    p, f, e = graph("free7")
    out, rep = capi.pose_graph_optimize_yaw(p, np.ones(8, np.uint8), e, Y)
    assert rep["n_free"] == 0 and rep["iterations"] == 0 and out.tobytes() == p.tobytes()
    assert abs(rep["final_cost"] - pr.cost(p, e)) <= 1e-9 * rep["final_cost"]
    # parameters
    out, rep = capi.pose_graph_optimize_yaw(p, f, e, Y, max_iterations=2, lambda0=10.0)
    r2, rr2 = py.optimize(p, f, e, Y, max_iterations=2, lambda0=10.0)
    assert rep["accepted"] == 2 and rr2["accepted"] == 2 and rep["rejected"] == rr2["rejected"]
    assert np.abs(out - r2).max() <= 1e-7 and abs(rep["final_lambda"] - rr2["final_lambda"]) <= 1e-12 * rr2["final_lambda"]


def test_singular_system_is_rejected_until_lambda_runs_out(capi):
    """every edge of free pose 3 has zero weights: its 4x4 diagonal block is exactly zero, every trial meets a pivot that is not
    positive and is rejected until lambda passes 1e8: 20 trials (tests/test_gpu_pgo.py has the count); nothing moves"""
    poses, fixed, edges = graph("free7")
    ez = [(i, j, Z, 0.0, 0.0) if 3 in (i, j) else (i, j, Z, a, b) for (i, j, Z, a, b) in edges]
    want, wrep = py.optimize(poses, fixed, ez, Y)
    out, rep = capi.pose_graph_optimize_yaw(poses, fixed, ez, Y)
    assert (wrep["accepted"], wrep["rejected"]) == (0, 20) and (rep["accepted"], rep["rejected"], rep["iterations"]) == (0, 20, 20)
    assert out.tobytes() == poses.tobytes() and want.tobytes() == poses.tobytes()
    assert rep["final_cost"] == rep["initial_cost"] and abs(rep["final_lambda"] - wrep["final_lambda"]) <= 1e-12 * wrep["final_lambda"]


def test_refusals(capi):
    poses, fixed, edges = graph("free7")
    I = np.eye(4)

    def status(p=poses, f=fixed, e=edges, axis=Y, **kw):
        with pytest.raises(capi.VslamError) as ex:
            capi.pose_graph_optimize_yaw(p, f, e, axis, **kw)
        return ex.value.status

    assert status(axis=(0.0, 0.0, 0.0)) == capi.ERR_INVALID
    assert status(axis=(0.0, np.nan, 1.0)) == capi.ERR_INVALID
    assert status(axis=(np.inf, 0.0, 1.0)) == capi.ERR_INVALID
    assert status(e=edges + [(3, 3, I, 1.0, 1.0)]) == capi.ERR_INVALID
    assert status(e=edges + [(3, 8, I, 1.0, 1.0)]) == capi.ERR_INVALID
    assert status(e=edges + [(-1, 2, I, 1.0, 1.0)]) == capi.ERR_INVALID
    bad = poses.copy(); bad[4, 1, 3] = np.nan
    assert status(p=bad) == capi.ERR_INVALID
    Zi = I.copy(); Zi[0, 0] = np.inf
    assert status(e=edges + [(1, 2, Zi, 1.0, 1.0)]) == capi.ERR_INVALID
    assert status(e=edges + [(1, 2, I, np.nan, 1.0)]) == capi.ERR_INVALID
    assert status(e=edges + [(1, 2, I, -1.0, 1.0)]) == capi.ERR_INVALID
    assert status(e=edges + [(1, 2, I, 1.0, -1e-3)]) == capi.ERR_INVALID
    assert status(lambda0=-1.0) == capi.ERR_INVALID
    assert status(max_iterations=-1) == capi.ERR_INVALID
    assert status(f=np.zeros(8, np.uint8)) == capi.ERR_INVALID                       # a free gauge
    p2 = np.concatenate([poses, poses[:2]]); f2 = np.concatenate([fixed, [0, 0]]).astype(np.uint8)
    assert status(p=p2, f=f2, e=edges + [(8, 9, I, 1.0, 1.0)]) == capi.ERR_INVALID    # a component without a fixed pose
    big = np.tile(I, (16385, 1, 1)); fb = np.zeros(16385, np.uint8); fb[0] = 1
    assert status(p=big, f=fb, e=[(0, 1, I, 1.0, 1.0)]) == capi.ERR_CAPACITY
    many = np.tile(capi.pgo_edges([(0, 1, I, 1.0, 1.0)] * 2), 131073)
    assert status(p=poses[:2], f=fixed[:2], e=many) == capi.ERR_CAPACITY
    hub = np.tile(I, (1100, 1, 1)); fh = np.zeros(1100, np.uint8); fh[1] = 1
    assert status(p=hub, f=fh, e=[(0, k, I, 1.0, 1.0) for k in range(1, 1100)]) == capi.ERR_CAPACITY


# ---- the batched call: a lane is, byte for byte, its single call ---------------------------------------------------------------
MIX = [("free7", "y"), ("hub100", "tilted"), None, ("free1", "y"), ("complete12", "tilted"), ("chain300", "y"), ("free2", "tilted"),
       ("star", "y"), ("special", "y"), ("free7", "tilted")]


def call_batch(capi, lanes, bad_axis_lane=None):
    """lanes: (name, axis) or None.  Every output and report starts as sentinel bytes: (status, [output bytes], [report or None])"""
    B = len(lanes)
    tab = (capi.PgoYawGraph * B)()
    reps = (capi.PgoReport * B)()
    C.memset(reps, SENTINEL, C.sizeof(reps))
    outs, keep = [], []
    for k, ln in enumerate(lanes):
        if ln is None:
            outs.append(np.full(128, SENTINEL, np.uint8))
            tab[k].graph = capi.PgoGraph(None, None, 0, None, 0, outs[k].ctypes.data)
            continue
        poses, fixed, edges = graph(ln[0])
        ea = capi.pgo_edges(edges)
        keep.append(ea)
        outs.append(np.full(poses.nbytes, SENTINEL, np.uint8))
        tab[k].graph = capi.PgoGraph(poses.ctypes.data, fixed.ctypes.data, len(poses), ea.ctypes.data, len(edges), outs[k].ctypes.data)
        tab[k].axis[:] = (0.0, 0.0, 0.0) if k == bad_axis_lane else AXES[ln[1]]
    st = capi.lib().vslam_pose_graph_optimize_yaw_batch(tab, B, None, 0, reps)
    sentinel_rep = bytes([SENTINEL]) * C.sizeof(capi.PgoReport)
    return st, [o.tobytes() for o in outs], [None if bytes(reps[k]) == sentinel_rep else capi._pgo_report_dict(reps[k]) for k in range(B)]


def test_batch_lane_equals_single_call_bitwise(capi):
    st, outs, reps = call_batch(capi, MIX)
    assert st == capi.OK, capi.lib().vslam_last_error()
    for k, ln in enumerate(MIX):
        if ln is None:
            assert outs[k] == bytes([SENTINEL]) * len(outs[k]) and reps[k] is None       # the idle middle lane: nothing written
            continue
        want, wrep = capi.pose_graph_optimize_yaw(*graph(ln[0]), AXES[ln[1]])
        assert reps[k] == wrep, ln
        assert outs[k] == want.tobytes(), ln
    assert outs[0] != outs[-1]                                      # (the lanes' own axes did apply: one graph, two axes)
    assert len({r["iterations"] for r in reps if r}) > 1            # lanes stop in different rounds
    # the lanes in another order
    st2, outs2, reps2 = call_batch(capi, MIX[::-1])
    assert st2 == capi.OK and outs2 == outs[::-1] and reps2 == reps[::-1]
    # a lane with a zero axis: refused, the lane named, nothing written in any lane
    st3, outs3, reps3 = call_batch(capi, MIX, bad_axis_lane=4)
    assert st3 == capi.ERR_INVALID and b"lane 4" in capi.lib().vslam_last_error()
    assert all(o == bytes([SENTINEL]) * len(o) for o in outs3) and all(r is None for r in reps3)


def test_python_binding_of_the_batch(capi):
    res = capi.pose_graph_optimize_yaw_batch([graph("free7") + (Y,), None, graph("star") + (TILTED,)])
    assert res[1] is None
    for r, (nm, ax) in ((res[0], ("free7", Y)), (res[2], ("star", TILTED))):
        want, wrep = capi.pose_graph_optimize_yaw(*graph(nm), ax)
        assert r[0].tobytes() == want.tobytes() and r[1] == wrep
